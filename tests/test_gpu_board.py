"""GPU: checkerboards assembled on the device (ccal_kernels_board.hip: ccal_assemble_checkerboards_batch,
ccal_detect_checkerboards_batch / _dev, Context.assemble_checkerboards_batch / detect_checkerboards_batch / _dev,
api.detect_checkerboard_points / detect_checkerboard with fused=True).

The oracle of the assembly is tests/board_ref.py, the numpy f64 yardstick of the rule in include/ccal.h; the oracle of the fused
call is the STAGED chain on the same context - ccal_detect_corners_batch, ccal_refine_corners_batch - with the yardstick on the host.
Every comparison is exact: found, flags, stats, idx and the bits of xy_out.  Every output is prefilled with a sentinel, and rows that
are not written keep it.  Nothing is larger than 320 x 240.  The yardstick runs every attempt of an image in Python loops (0.5 s for
a frame of 35 kept rows); each reference is computed once and shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import board_ref  # noqa: E402
import detect_ref  # noqa: E402
from test_board_cpu import synthetic  # noqa: E402
from test_detect_cpu import PATTERN, _candidates, _inner, expected_labelling  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, -3.25
IP, LP, DP = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
COLS, ROWS = PATTERN
SQ = detect_ref.BOARD_SQUARE
OPTS = dict(step=1, nms_radius=5, min_response=1, rel_q10=102, cand_cap=4096, half_win=5, max_iterations=30, eps=1e-3, cols=COLS, rows=ROWS)
A_OUTS = ("found", "xy", "idx", "flags", "stats")
D_OUTS = ("found", "xy", "flags", "stats")


def _code(dtype):
    return _ffi.PIX_U8 if np.dtype(dtype) == np.uint8 else _ffi.PIX_U16


def _outs(m, nw, with_idx):
    out = {"found": np.full(m, SENT_I, dtype=np.int32), "flags": np.full(m, SENT_I, dtype=np.int32),
           "stats": np.full((m, 4), SENT_I, dtype=np.int32), "xy": np.full((m, nw, 2), SENT_F)}
    if with_idx:
        out["idx"] = np.full((m, nw), SENT_I, dtype=np.int32)
    return out


def raw_assemble(ctx, xy_list, hess_list, cols=COLS, rows=ROWS, **change):
    """The C entry point, every output prefilled with a sentinel: {"rc"} + A_OUTS.  change: n, offsets, "null": pointers passed as NULL."""
    n_img = len(xy_list)
    offs = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum([len(x) for x in xy_list], out=offs[1:])
    xy = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in xy_list] + [np.zeros((0, 2))]))
    hess = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.float64).reshape(-1, 3) for h in hess_list] + [np.zeros((0, 3))]))
    a = dict(n=n_img, offsets=offs, null=())
    a.update(change)
    offs = np.ascontiguousarray(a["offsets"], dtype=np.int64)
    out = _outs(max(n_img, 1), max(cols * rows, 1), True)
    inp = {"offsets": offs.ctypes.data_as(LP), "xy_in": xy.ctypes.data_as(DP), "hess": hess.ctypes.data_as(DP)}
    g = lambda name: None if name in a["null"] else inp[name]                        # noqa: E731
    p = lambda name, t: None if name in a["null"] else out[name].ctypes.data_as(t)      # noqa: E731
    out["rc"] = ctx.lib.ccal_assemble_checkerboards_batch(ctx.handle, a["n"], g("offsets"), g("xy_in"), g("hess"), cols, rows, p("found", IP),
                                                          p("xy", DP), p("idx", IP), p("flags", IP), p("stats", IP))
    return out


def raw_detect(ctx, images, o, fn=None, ptr=None, **change):
    """A fused C entry point on a batch [n][H][W], every output prefilled with a sentinel: {"rc"} + D_OUTS."""
    images = np.ascontiguousarray(images)
    n_img, H, W = images.shape
    a = dict(dtype=_code(images.dtype), w=W, h=H, n=n_img, null=(), opts_null=False)
    a.update(change)
    opts = _ffi.DetectCheckerboardsOpts(**o)
    out = _outs(max(n_img, 1), max(int(o["cols"]) * int(o["rows"]), 1) if 0 < o["cols"] * o["rows"] < 1000 else 1, False)
    p = lambda name, t: None if name in a["null"] else out[name].ctypes.data_as(t)      # noqa: E731
    fn = fn or ctx.lib.ccal_detect_checkerboards_batch
    img_ptr = None if "images" in a["null"] else C.c_void_p(images.ctypes.data if ptr is None else ptr)
    out["rc"] = fn(ctx.handle, a["dtype"], a["w"], a["h"], a["n"], img_ptr, None if a["opts_null"] else C.byref(opts),
                   p("found", IP), p("xy", DP), p("flags", IP), p("stats", IP))
    return out


def untouched(out):
    return all(bool((out[k] == (SENT_F if out[k].dtype == np.float64 else SENT_I)).all()) for k in out if k != "rc")


def bits(out, k=None):
    return b"".join((out[key] if k is None else out[key][k]).tobytes() for key in A_OUTS if key in out)


_WANT = {}


def want(xy, hess, cols=COLS, rows=ROWS):
    """The yardstick's answer for one image, computed once per input."""
    xy, hess = np.ascontiguousarray(xy, dtype=np.float64), np.ascontiguousarray(hess, dtype=np.float64)
    key = (xy.tobytes(), hess.tobytes(), cols, rows)
    if key not in _WANT:
        _WANT[key] = board_ref.assemble(xy, hess, cols, rows)
    return _WANT[key]


def check(got, wants, where=""):
    """Exact: found, flags, stats, and for an image with a board its idx and the bits of its positions; the sentinel otherwise."""
    assert got["rc"] == _ffi.OK, where
    for k, w in enumerate(wants):
        at = (where, k)
        assert (int(got["found"][k]), int(got["flags"][k]), got["stats"][k].tolist()) == (w["found"], w["flags"], [int(s) for s in w["stats"]]), at
        if w["found"]:
            assert got["xy"][k].tobytes() == np.ascontiguousarray(w["xy"]).tobytes(), at
            assert "idx" not in got or np.array_equal(got["idx"][k], w["idx"]), at
        else:
            assert (got["xy"][k] == SENT_F).all() and ("idx" not in got or (got["idx"][k] == SENT_I).all()), at


def strays(k, count, seed, lo=0.8, hi=1.22):
    """Frame k's candidates with `count` strays added, each with a true corner's Hessian scaled by lo .. hi and farther than 5 px in
    x or y from every other candidate, in a random input order."""
    xy, hess = _candidates(k)
    inner = np.flatnonzero(_inner(xy, detect_ref.board_frames()[1][k]))
    rng = np.random.default_rng(seed)
    pts = xy
    while len(pts) < len(xy) + count:
        p = rng.uniform([6.0, 6.0], [detect_ref.BOARD_W - 7.0, detect_ref.BOARD_H - 7.0])
        if np.abs(pts - p).max(axis=1).min() > 5.0:
            pts = np.concatenate([pts, p[None]])
    eh = hess[rng.choice(inner, count)] * rng.uniform(lo, hi, (count, 1))
    order = rng.permutation(len(pts))
    return pts[order], np.concatenate([hess, eh])[order]


# ---- 1. the assembly against the yardstick ----------------------------------------------------------------------------------------------
def test_the_three_frames(gpu_ctx):
    cands = [_candidates(k) for k in range(3)]
    wants = [want(*c) for c in cands]
    assert all(w["found"] == 1 and w["stats"][0] == 35 for w in wants)
    got = raw_assemble(gpu_ctx, [c[0] for c in cands], [c[1] for c in cands])
    check(got, wants, "frames")
    print("stats", got["stats"].tolist())
    again = raw_assemble(gpu_ctx, [c[0] for c in cands], [c[1] for c in cands])
    assert bits(again) == bits(got)                                      # two runs: the same bits
    lean = raw_assemble(gpu_ctx, [c[0] for c in cands], [c[1] for c in cands], null=("idx", "stats"))
    assert lean["rc"] == _ffi.OK and (lean["idx"] == SENT_I).all() and (lean["stats"] == SENT_I).all()
    assert all(lean[key].tobytes() == got[key].tobytes() for key in ("found", "xy", "flags"))
    # a permuted copy: the same positions, idx mapped through the permutation
    perms = [np.random.default_rng(40 + k).permutation(len(c[0])) for k, c in enumerate(cands)]
    turned = raw_assemble(gpu_ctx, [c[0][p] for c, p in zip(cands, perms)], [c[1][p] for c, p in zip(cands, perms)])
    assert turned["rc"] == _ffi.OK and turned["xy"].tobytes() == got["xy"].tobytes() and turned["stats"].tobytes() == got["stats"].tobytes()
    for k, p in enumerate(perms):
        assert np.array_equal(p[turned["idx"][k]], got["idx"][k]), k


def test_stray_candidates_in_one_batch_of_24(gpu_ctx):
    """Eight stray sets (six strong strays each, random input order) for each of the three frames, one launch."""
    cases = [strays(k, 6, seed) for k in range(3) for seed in range(1000, 1008)]
    wants = [want(*c) for c in cases]
    base = [want(*_candidates(k)) for k in range(3)]
    for n, w in enumerate(wants):
        assert w["found"] == 1 and w["xy"].tobytes() == base[n // 8]["xy"].tobytes() and w["stats"][0] == 41
    got = raw_assemble(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases])
    check(got, wants, "strays")


def test_row_counts_around_the_pattern_size(gpu_ctx):
    """No rows, 34 and exactly 35 usable rows (the inner corners alone), an image of unusable rows only, in one launch."""
    xy, hess = _candidates(1)
    inner = np.flatnonzero(_inner(xy, detect_ref.board_frames()[1][1]))
    assert len(inner) == 35
    bad_xy, bad_h = xy[:40].copy(), hess[:40].copy()
    bad_xy[::2, 0] = np.nan
    bad_h[1::2] = [3.0, 2.0, 1.0]
    cases = [(np.zeros((0, 2)), np.zeros((0, 3))), (xy[inner[:34]], hess[inner[:34]]), (xy[inner], hess[inner]), (bad_xy, bad_h), (xy, hess)]
    wants = [want(*c) for c in cases]
    assert [w["found"] for w in wants] == [0, 0, 1, 0, 1] and [w["stats"][0] for w in wants] == [0, 0, 35, 0, 35]
    check(raw_assemble(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases]), wants, "row counts")


@pytest.mark.parametrize("kept", [63, 64, 65, 130])
def test_kept_counts_at_the_lane_boundaries(gpu_ctx, kept):
    """Strays at 1 .. 1.21 of a true corner's strength, all kept with the 35 inner corners: a lane holds one candidate, then two,
    then three.  Equal to the yardstick whether a board is found or not."""
    cases = [strays(k, kept - 35, 2000 + kept, 1.0, 1.1) for k in (0, 2)]
    wants = [want(*c) for c in cases]
    assert all(w["stats"][0] == kept for w in wants)
    got = raw_assemble(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases])
    print(f"kept {kept}: found {got['found'].tolist()}, stats {got['stats'].tolist()}")
    check(got, wants, f"kept {kept}")


@pytest.mark.parametrize("case", ["corner", "inside", "opposite corner", "6 x 5"])
def test_incomplete_boards_exhaust_every_attempt(gpu_ctx, case):
    xy, hess = _candidates()
    inner = np.flatnonzero(_inner(xy, detect_ref.board_frames()[1][0]))
    cols = 6 if case == "6 x 5" else COLS
    if case != "6 x 5":
        keep = np.arange(len(xy)) != {"corner": inner[0], "inside": inner[17], "opposite corner": inner[-1]}[case]
        xy, hess = xy[keep], hess[keep]
    w = want(xy, hess, cols, ROWS)
    assert w["found"] == 0 and w["stats"][0] >= 30 and w["stats"][1:] == [0, -1, -1]        # all 4 n attempts looked at, none won
    check(raw_assemble(gpu_ctx, [xy], [hess], cols, ROWS), [w], case)


def test_square_and_smallest_patterns(gpu_ctx):
    cases = []
    for k in range(3):
        xy, hess = _candidates(k)
        truth = detect_ref.board_frames()[1][k].reshape(ROWS, COLS, 2)[:, 1:6].reshape(-1, 2)
        keep = _inner(xy, truth)
        cases.append((xy[keep], hess[keep]))
    wants = [want(*c, 5, 5) for c in cases]
    assert all(w["found"] == 1 for w in wants)
    check(raw_assemble(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases], 5, 5), wants, "5 x 5")
    two = [synthetic(2, 2), tuple(a[::-1] for a in synthetic(2, 2)), synthetic(3, 3)]
    wants = [want(*c, 2, 2) for c in two]
    assert [w["found"] for w in wants] == [1, 1, 0]                       # a 3 x 3 lattice holds four 2 x 2 windows
    check(raw_assemble(gpu_ctx, [c[0] for c in two], [c[1] for c in two], 2, 2), wants, "2 x 2")
    big = synthetic(20, 20, pitch=12.0)                                  # the largest pattern: the answer is known, the yardstick would take minutes
    got = raw_assemble(gpu_ctx, [big[0]], [big[1]], 20, 20)
    assert got["rc"] == _ffi.OK and got["found"][0] == 1 and got["flags"][0] == 0 and got["stats"][0, 0] == 400 and got["stats"][0, 1] >= 1
    assert got["idx"][0].tolist() == list(range(400)) and got["xy"][0].tobytes() == big[0].tobytes()


# ---- 2. the kept limit -----------------------------------------------------------------------------------------------------------------
def saddle_field(dtype=np.uint8):
    """29 x 21 = 609 isolated saddles of ONE polarity (a 2 x 2 chequer of 4 px squares on grey, every 11 px): all of one strength, so
    all are kept, and none has a neighbour of the opposite polarity, so nothing links and the host function answers at once."""
    img = np.full((240, 320), 128, dtype=np.float64)
    for cy in range(8, 232, 11):
        for cx in range(6, 314, 11):
            img[cy - 4:cy, cx - 4:cx] = 215.0; img[cy:cy + 4, cx:cx + 4] = 215.0
            img[cy - 4:cy, cx:cx + 4] = 40.0; img[cy:cy + 4, cx - 4:cx] = 40.0
    return img.astype(dtype) if dtype == np.uint8 else (img * 257.0).astype(np.uint16)


def test_the_kept_limit(gpu_ctx):
    xy, hess = synthetic(27, 19)
    assert len(xy) == 513
    ok = _candidates(0)
    got = raw_assemble(gpu_ctx, [ok[0], xy, xy[:-1]], [ok[1], hess, hess[:-1]])
    assert got["rc"] == _ffi.OK and got["found"].tolist() == [1, 0, 0] and got["flags"].tolist() == [0, _ffi.BOARD_FLAG_KEPT_LIMIT, 0]
    assert got["stats"][1].tolist() == [513, 0, -1, -1] and got["stats"][2, 0] == 512
    assert (got["xy"][1:] == SENT_F).all() and (got["idx"][1:] == SENT_I).all()
    check(got, [want(*ok), want(xy, hess), None][:2], "limit")
    # through the images: more than 512 saddles kept - the fused call flags the image, the api goes the staged way for it
    imgs = np.stack([saddle_field(), detect_ref.board_frames()[0][0]])
    kw = dict(nms_radius=3, half_win=3)
    res = gpu_ctx.detect_checkerboards_batch(imgs, COLS, ROWS, nms_radius=3, half_win=3)
    assert res[0][0] == 0 and res[0][2] == _ffi.BOARD_FLAG_KEPT_LIMIT and res[0][3][0] > 512, (res[0][2], res[0][3])
    assert res[1][0] == 1 and res[1][2] == 0
    fused = api.detect_checkerboard_points(list(imgs), PATTERN, SQ, ctx=gpu_ctx, fused=True, **kw)
    assert fused == api.detect_checkerboard_points(list(imgs), PATTERN, SQ, ctx=gpu_ctx, **kw) and fused[0] is None and fused[1] is not None


# ---- 3. the fused call against the staged chain -----------------------------------------------------------------------------------------
def staged(ctx, images, o):
    """The oracle: the two stage calls on `ctx`, the yardstick on the host.  Per image the yardstick's dict, flags with the cap's bit."""
    images = np.ascontiguousarray(images)
    found = ctx.detect_corners_batch(images, o["step"], o["nms_radius"], o["min_response"], o["rel_q10"] / 1024.0, o["cand_cap"])
    xy, status, _, _ = ctx.refine_corners_batch(images, [f[0].astype(np.float64) for f in found], o["half_win"], o["max_iterations"], o["eps"])
    out = []
    for k, f in enumerate(found):
        good = status[k] == _ffi.OK
        w = dict(want(xy[k][good], f[1][good].astype(np.float64), o["cols"], o["rows"]))
        w["flags"] = w["flags"] | (_ffi.BOARD_FLAG_CAND_CAP if f[3] > o["cand_cap"] else 0)
        w["count"] = f[3]
        out.append(w)
    return out


def cropped(dtype=np.uint8):
    """Frame 0 with its left 45 % painted over in the background's white: a partial board."""
    img = detect_ref.board_frames(dtype)[0][0].copy()
    img[:, :int(0.45 * img.shape[1])] = img[0, 0]
    return img


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_fused_call_against_the_staged_chain(gpu_ctx, dtype):
    frames, truth = detect_ref.board_frames(dtype)
    imgs = np.concatenate([frames, np.full_like(frames[:1], 90), cropped(dtype)[None]])
    wants = staged(gpu_ctx, imgs, OPTS)
    assert [w["found"] for w in wants] == [1, 1, 1, 0, 0] and wants[3]["stats"] == [0, 0, -1, -1] and wants[4]["stats"][0] > 0
    got = raw_detect(gpu_ctx, imgs, OPTS)
    check(got, wants, np.dtype(dtype).name)
    print(np.dtype(dtype).name, "stats", got["stats"].tolist())
    again = raw_detect(gpu_ctx, imgs, OPTS)
    assert bits(again) == bits(got)
    lean = raw_detect(gpu_ctx, imgs, OPTS, null=("stats",))
    assert lean["rc"] == _ffi.OK and (lean["stats"] == SENT_I).all() and lean["xy"].tobytes() == got["xy"].tobytes()
    points = api.detect_checkerboard_points(list(imgs), PATTERN, SQ, ctx=gpu_ctx)
    assert [p is not None for p in points] == [True, True, True, False, False]
    worst = 0.0
    for k in range(3):
        assert points[k] == {i: (float(x), float(y)) for i, (x, y) in enumerate(got["xy"][k])}
        worst = max(worst, float(np.linalg.norm(got["xy"][k] - expected_labelling(truth[k]), axis=1).max()))
    print(f"worst distance to the true corner pixel: {worst:.5f} px")
    assert worst <= detect_ref.BOARD_BOUND
    assert api.detect_checkerboard_points(list(imgs), PATTERN, SQ, ctx=gpu_ctx, fused=True) == points


def test_a_candidate_cap_below_the_count(gpu_ctx):
    imgs = detect_ref.board_frames()[0]
    full = staged(gpu_ctx, imgs, OPTS)
    assert all(w["count"] > 45 for w in full)
    o = dict(OPTS, cand_cap=45)
    wants = staged(gpu_ctx, imgs, o)
    assert all(w["flags"] == _ffi.BOARD_FLAG_CAND_CAP for w in wants)
    got = raw_detect(gpu_ctx, imgs, o)
    check(got, wants, "cand_cap 45")
    print("cand_cap 45: found", got["found"].tolist(), "stats", got["stats"].tolist())


# ---- 4. batch shape ------------------------------------------------------------------------------------------------------------------------
def test_image_by_image_reversed_and_129_images(gpu_ctx):
    """k_chain_offsets scans the per-image candidate counts 64 images per round: 129 images - the three frames in turn, image 64 a
    blank one - make two carries and a zero count on the first lane of a round."""
    frames = detect_ref.board_frames()[0]
    imgs = np.concatenate([frames, np.full_like(frames[:1], 90), cropped()[None]])
    whole = raw_detect(gpu_ctx, imgs, OPTS)
    check(whole, staged(gpu_ctx, imgs, OPTS), "whole")
    for k in range(len(imgs)):
        alone = raw_detect(gpu_ctx, imgs[k:k + 1], OPTS)
        assert alone["rc"] == _ffi.OK and bits(alone, 0) == bits(whole, k), k
    back = raw_detect(gpu_ctx, imgs[::-1], OPTS)
    assert [bits(back, len(imgs) - 1 - k) for k in range(len(imgs))] == [bits(whole, k) for k in range(len(imgs))]
    many = np.ascontiguousarray(frames[np.arange(129) % 3])
    many[64] = 0
    got = raw_detect(gpu_ctx, many, OPTS)
    assert got["rc"] == _ffi.OK
    for k in range(129):
        if k != 64:
            assert bits(got, k) == bits(whole, k % 3), k
    assert got["found"][64] == 0 and got["flags"][64] == 0 and got["stats"][64].tolist() == [0, 0, -1, -1] and (got["xy"][64] == SENT_F).all()
    # the assembly alone: image by image and reversed
    cases = [_candidates(0), (np.zeros((0, 2)), np.zeros((0, 3))), strays(1, 6, 1003), _candidates(2)]
    batch = raw_assemble(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases])
    check(batch, [want(*c) for c in cases], "assembly batch")
    for k, c in enumerate(cases):
        assert bits(raw_assemble(gpu_ctx, [c[0]], [c[1]]), 0) == bits(batch, k), k
    back = raw_assemble(gpu_ctx, [c[0] for c in cases[::-1]], [c[1] for c in cases[::-1]])
    assert [bits(back, 3 - k) for k in range(4)] == [bits(batch, k) for k in range(4)]


def test_no_images_and_images_without_a_domain_are_valid(gpu_ctx):
    for fn in (gpu_ctx.lib.ccal_detect_checkerboards_batch, gpu_ctx.lib.ccal_detect_checkerboards_dev):
        got = raw_detect(gpu_ctx, np.zeros((0, 48, 64), dtype=np.uint8), OPTS, fn=fn, null=D_OUTS + ("images",))
        assert got["rc"] == _ffi.OK
    assert raw_assemble(gpu_ctx, [], [], null=A_OUTS + ("offsets", "xy_in", "hess"))["rc"] == _ffi.OK
    assert gpu_ctx.detect_checkerboards_dev(0, _ffi.PIX_U8, 64, 48, 0, COLS, ROWS) == [] == gpu_ctx.assemble_checkerboards_batch([], [], COLS, ROWS)
    tiny = raw_detect(gpu_ctx, np.full((2, 6, 40), 9, dtype=np.uint8), OPTS)                          # 6 rows: no domain at step 1
    assert tiny["rc"] == _ffi.OK and (tiny["found"] == 0).all() and (tiny["flags"] == 0).all() and tiny["stats"].tolist() == [[0, 0, -1, -1]] * 2
    assert (tiny["xy"] == SENT_F).all()


# ---- 5. chunks, the poison, the _dev entry -----------------------------------------------------------------------------------------------
def test_a_batch_cut_into_chunks(dev_ctx, gpu_ctx, monkeypatch):
    """The library runs a batch whose block would exceed 256 MB in chunks of whole images; the second library reads the limit from
    CCAL_TEST_BOARD_CHUNK_BYTES (tests only).  A limit of one byte is an image per chunk; 25 kB holds two images of the assembly's
    batch (about 11 kB each) and 800 kB two of the fused calls' (about 360 kB with the image, 280 kB without).  Host and device
    entry: the product's bits."""
    import torch
    frames = detect_ref.board_frames()[0]
    imgs = np.concatenate([frames, np.full_like(frames[:1], 90), cropped()[None]])
    whole = raw_detect(gpu_ctx, imgs, OPTS)
    assert whole["rc"] == _ffi.OK and whole["found"].tolist() == [1, 1, 1, 0, 0]
    cases = [_candidates(0), (np.zeros((0, 2)), np.zeros((0, 3))), strays(1, 6, 1003), _candidates(2)]
    batch = raw_assemble(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases])
    assert batch["rc"] == _ffi.OK
    raw = torch.from_numpy(imgs.copy()).cuda()
    torch.cuda.synchronize()
    for limit in ("1", "25000", "800000"):
        monkeypatch.setenv("CCAL_TEST_BOARD_CHUNK_BYTES", limit)
        got = raw_detect(dev_ctx, imgs, OPTS)
        assert got["rc"] == _ffi.OK and bits(got) == bits(whole), limit
        got = raw_detect(dev_ctx, imgs, OPTS, fn=dev_ctx.lib.ccal_detect_checkerboards_dev, ptr=raw.data_ptr())
        assert got["rc"] == _ffi.OK and bits(got) == bits(whole), limit
        got = raw_assemble(dev_ctx, [c[0] for c in cases], [c[1] for c in cases])
        assert got["rc"] == _ffi.OK and bits(got) == bits(batch), limit


def test_parity_on_poisoned_workspace(dev_ctx, gpu_ctx, monkeypatch):
    """The second library with CCAL_TEST_POISON_ALLOC=1 (tests/test_gpu_poison.py): every double of the calls' blocks starts as NaN
    bytes in every chunk; each is written before it is read."""
    frames = detect_ref.board_frames(np.uint16)[0]
    imgs = np.concatenate([frames, np.full_like(frames[:1], 90), cropped(np.uint16)[None]])
    cases = [_candidates(0), (np.zeros((0, 2)), np.zeros((0, 3))), strays(1, 6, 1003), synthetic(27, 19)]
    clean_d, clean_a = raw_detect(gpu_ctx, imgs, OPTS), raw_assemble(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases])
    monkeypatch.setenv("CCAL_TEST_POISON_ALLOC", "1")
    got_d, got_a = raw_detect(dev_ctx, imgs, OPTS), raw_assemble(dev_ctx, [c[0] for c in cases], [c[1] for c in cases])
    assert clean_d["rc"] == got_d["rc"] == _ffi.OK and bits(got_d) == bits(clean_d)
    assert clean_a["rc"] == got_a["rc"] == _ffi.OK and bits(got_a) == bits(clean_a)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_dev_entry_point_on_a_block_written_by_remap_dev(gpu_ctx, dtype):
    """The images go through ccal_remap_dev with an identity map into a torch-allocated block; ccal_detect_checkerboards_dev follows
    on the context's stream without a synchronise in between."""
    import torch
    imgs = np.ascontiguousarray(detect_ref.board_frames(dtype)[0])
    n, H, W = imgs.shape
    host = raw_detect(gpu_ctx, imgs, OPTS)
    assert host["rc"] == _ffi.OK and host["found"].tolist() == [1, 1, 1]
    xm, ym = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    m = gpu_ctx.undistort_map_from_arrays(np.ascontiguousarray(xm), np.ascontiguousarray(ym))
    try:
        src = torch.from_numpy(imgs.view(np.uint8).copy()).cuda()
        dst = torch.zeros_like(src)
        torch.cuda.synchronize()
        m.remap_dev(src.data_ptr(), dst.data_ptr(), _code(dtype), 1, W, H, n)
        dev = raw_detect(gpu_ctx, imgs, OPTS, fn=gpu_ctx.lib.ccal_detect_checkerboards_dev, ptr=dst.data_ptr())
        assert dst.cpu().numpy().tobytes() == imgs.tobytes()
    finally:
        m.close()
    assert dev["rc"] == _ffi.OK and bits(dev) == bits(host)
    wrapped = gpu_ctx.detect_checkerboards_dev(dst.data_ptr(), _code(dtype), W, H, n, COLS, ROWS)
    for k, (found, xy, flags, stats) in enumerate(wrapped):
        assert (found, flags, stats.tolist()) == (1, 0, host["stats"][k].tolist()) and xy.tobytes() == host["xy"][k].tobytes()


# ---- 6. invalid arguments --------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(gpu_ctx):
    imgs = detect_ref.board_frames()[0][:2]
    nan, inf = float("nan"), float("inf")
    bad_opts = [dict(step=0), dict(step=5), dict(nms_radius=0), dict(nms_radius=16), dict(min_response=0), dict(rel_q10=-1), dict(rel_q10=1025),
                dict(cand_cap=0), dict(cand_cap=4097), dict(half_win=0), dict(half_win=16), dict(max_iterations=0), dict(eps=-1.0),
                dict(eps=nan), dict(eps=inf), dict(cols=1), dict(cols=21), dict(rows=1), dict(rows=21), dict(cols=-7)]
    bad_args = [dict(dtype=2), dict(dtype=-1), dict(w=0), dict(h=-1), dict(n=-1), dict(w=65536, h=32768), dict(opts_null=True),
                dict(null=("images",)), dict(null=("found",)), dict(null=("xy",)), dict(null=("flags",))]
    for fn in (gpu_ctx.lib.ccal_detect_checkerboards_batch, gpu_ctx.lib.ccal_detect_checkerboards_dev):
        for change in bad_opts:
            got = raw_detect(gpu_ctx, imgs, dict(OPTS, **change), fn=fn)
            assert got["rc"] == _ffi.ERR_INVALID_ARG and untouched(got) and gpu_ctx.last_error(), change
        for change in bad_args:
            got = raw_detect(gpu_ctx, imgs, OPTS, fn=fn, **change)
            assert got["rc"] == _ffi.ERR_INVALID_ARG and untouched(got) and gpu_ctx.last_error(), change
    xy, hess = _candidates(0)
    for cols, rows in ((1, 5), (21, 5), (7, 1), (7, 21)):
        got = raw_assemble(gpu_ctx, [xy], [hess], cols, rows)
        assert got["rc"] == _ffi.ERR_INVALID_ARG and untouched(got) and gpu_ctx.last_error(), (cols, rows)
    many = np.tile(xy, (80, 1))[:4097], np.tile(hess, (80, 1))[:4097]
    changes = [dict(n=-1), dict(offsets=[1, len(xy)]), dict(offsets=[0, -1]), dict(null=("offsets",)), dict(null=("xy_in",)),
               dict(null=("hess",)), dict(null=("found",)), dict(null=("xy",)), dict(null=("flags",))]
    for change in changes:
        got = raw_assemble(gpu_ctx, [xy], [hess], **change)
        assert got["rc"] == _ffi.ERR_INVALID_ARG and untouched(got) and gpu_ctx.last_error(), change
    got = raw_assemble(gpu_ctx, [xy, many[0]], [hess, many[1]])                                       # 4097 rows in an image
    assert got["rc"] == _ffi.ERR_INVALID_ARG and untouched(got) and gpu_ctx.last_error()
    assert raw_assemble(gpu_ctx, [xy, many[0][:4096]], [hess, many[1][:4096]])["rc"] == _ffi.OK
    with pytest.raises(ValueError):
        gpu_ctx.detect_checkerboards_batch(np.zeros((1, 45, 67, 3), dtype=np.uint8), COLS, ROWS)          # colour
    with pytest.raises(ValueError):
        gpu_ctx.detect_checkerboards_batch(np.zeros((1, 45, 67), dtype=np.float32), COLS, ROWS)
    with pytest.raises(ValueError):
        gpu_ctx.assemble_checkerboards_batch([xy], [hess[:-1]], COLS, ROWS)


# ---- 7. the engine and api layers ----------------------------------------------------------------------------------------------------------
def test_context_and_api_wrappers(gpu_ctx):
    cands = [_candidates(k) for k in range(3)] + [(np.zeros((0, 2)), np.zeros((0, 3)))]
    got = gpu_ctx.assemble_checkerboards_batch([c[0] for c in cands], [c[1] for c in cands], COLS, ROWS)
    for (found, xy, idx, flags, stats), c in zip(got, cands):
        w = want(*c)
        assert (found, flags, stats.tolist()) == (w["found"], w["flags"], w["stats"])
        if found:
            assert xy.tobytes() == w["xy"].tobytes() and np.array_equal(idx, w["idx"]) and idx.dtype == np.int32
            assert board_ref.as_dict(w) == api.assemble_checkerboard(c[0], c[1], PATTERN, SQ)
        else:
            assert xy is None and idx is None
    frames = detect_ref.board_frames()[0]
    imgs = list(frames) + [cropped(), np.full_like(frames[0], 90)]
    wants = staged(gpu_ctx, np.stack(imgs), OPTS)
    res = gpu_ctx.detect_checkerboards_batch(np.stack(imgs), COLS, ROWS)                              # the defaults are OPTS
    for (found, xy, flags, stats), w in zip(res, wants):
        assert (found, flags, stats.tolist()) == (w["found"], w["flags"], w["stats"])
        assert (xy is None and not found) or xy.tobytes() == w["xy"].tobytes()
    fused = api.detect_checkerboard(imgs, PATTERN, SQ, ctx=gpu_ctx, fused=True)
    assert fused == api.detect_checkerboard(imgs, PATTERN, SQ, ctx=gpu_ctx)
    assert [f is not None for f in fused] == [True, True, True, False, False] and sorted(fused[0].features) == list(range(35))
    assert api.detect_checkerboard([], PATTERN, SQ, ctx=gpu_ctx, fused=True) == []
    sq = api.detect_checkerboard_points(imgs[:1], (5, 5), SQ, ctx=gpu_ctx, fused=True)                # a 7 x 5 board is no 5 x 5 board
    assert sq == api.detect_checkerboard_points(imgs[:1], (5, 5), SQ, ctx=gpu_ctx) == [None]
