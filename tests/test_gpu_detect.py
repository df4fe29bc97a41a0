"""GPU: the saddle detector (ccal_kernels_detect.hip, ccal_detect_corners_batch / _dev, api.detect_checkerboard) against
tests/detect_ref.py, the numpy int64 yardstick of the rule stated in include/ccal.h.

Bounds.  The rule is integer arithmetic and its outputs are decisions, so counts, positions, Hessians and responses are compared
with np.array_equal: no tolerance anywhere but the end-to-end test, whose positions pass through the f64 refinement (1e-9 px, the
suite's bound for f64 against f64).  Images are 6 x 6 up to 160 x 160, and one of 40 x 600; every case takes well under a second."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_ref  # noqa: E402
import detect_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77
PATTERN = (ref.BOARD_COLS, ref.BOARD_ROWS)


def _code(dtype):
    return _ffi.PIX_U8 if np.dtype(dtype) == np.uint8 else _ffi.PIX_U16


def raw_detect(ctx, imgs, s, r, min_response=1, rel_q10=102, cap=4096, fn=None, ptr=None, with_response=True):
    """The C entry point on [n][H][W] images with every output prefilled with SENTINEL: (count [n], xy [n][cap][2], hess [n][cap][3],
    response [n][cap])."""
    imgs = np.ascontiguousarray(imgs)
    n, H, W = imgs.shape
    count = np.full(max(n, 1), SENTINEL, dtype=np.int32)
    xy = np.full((max(n, 1), cap, 2), SENTINEL, dtype=np.int32); hess = np.full((max(n, 1), cap, 3), SENTINEL, dtype=np.int32)
    resp = np.full((max(n, 1), cap), SENTINEL, dtype=np.int64)
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    fn = fn or ctx.lib.ccal_detect_corners_batch
    rc = fn(ctx.handle, _code(imgs.dtype), W, H, n, C.c_void_p(imgs.ctypes.data if ptr is None else ptr), s, r, min_response, rel_q10, cap,
            count.ctypes.data_as(ip), xy.ctypes.data_as(ip), hess.ctypes.data_as(ip), resp.ctypes.data_as(lp) if with_response else None)
    assert rc == _ffi.OK, ctx.last_error()
    return count, xy, hess, resp


def check_against_yardstick(got, imgs, s, r, min_response=1, rel_q10=102, cap=4096, where=""):
    count, xy, hess, resp = got
    total = 0
    for k, img in enumerate(imgs):
        want = ref.detect(img, s, r, min_response, rel_q10, cap)
        m = min(want["count"], cap)
        assert count[k] == want["count"], (where, k, count[k], want["count"])
        assert np.array_equal(xy[k, :m], want["xy"]), (where, k)
        assert np.array_equal(hess[k, :m], want["hess"]), (where, k)
        assert np.array_equal(resp[k, :m], want["response"]), (where, k)
        assert (xy[k, m:] == SENTINEL).all() and (hess[k, m:] == SENTINEL).all() and (resp[k, m:] == SENTINEL).all(), (where, k)
        total += want["count"]
    return total


def parity_images(dtype, s):
    """{name: [n][H][W]} - the images every parity case runs on."""
    rng = np.random.default_rng(500 + s)
    scale = 257 if dtype == np.uint16 else 1
    side = 2 * (s + 2)
    out = {
        "grid 160 x 160": corner_ref.grid_fixture(310 + s, dtype=dtype)[0][None],
        # noise over the whole range, and four grey levels only: plateaus and equal maxima, which the tie rule decides
        "67 x 45": np.stack([rng.integers(0, 256, (45, 67)) * scale, rng.integers(0, 4, (45, 67)) * scale]).astype(dtype),
        "domain 2 x 2": (rng.integers(0, 256, (3, side + 2, side + 2)) * scale).astype(dtype),
        "domain 1 x 40": (rng.integers(0, 256, (2, side + 40, side + 1)) * scale).astype(dtype),
        "no domain": (rng.integers(0, 256, (2, 40, side)) * scale).astype(dtype),
        # more than 512 domain rows: k_detect_rows scans 256 rows per round and carries the count from round to round
        "40 x 600": (rng.integers(0, 256, (600, 40)) * scale).astype(dtype)[None],
    }
    if dtype == np.uint16:
        out["extreme 3 x 3"] = ref.extreme_blocks()[None]
        out["extreme 7 x 7"] = ref.extreme_blocks(block=7)[None]
    return out


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 5, 15])
@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_parity(gpu_ctx, dtype, s, r):
    """count, xy, hess and response equal the yardstick's, bit for bit; the rows past the count keep the caller's bytes."""
    for name, imgs in parity_images(dtype, s).items():
        n = check_against_yardstick(raw_detect(gpu_ctx, imgs, s, r), imgs, s, r, where=name)
        loose = check_against_yardstick(raw_detect(gpu_ctx, imgs, s, r, rel_q10=0), imgs, s, r, rel_q10=0, where=name + ", every maximum")
        print(f"{name}: {n} candidates at rel_q10 102, {loose} local maxima")
        if name == "no domain":
            assert n == loose == 0
        if name.startswith(("grid", "67")):
            assert loose >= n > 0
        if name.startswith("40 x 600"):                     # the input cannot go stale: candidates in each of the three rounds of rows
            rows = ref.detect(imgs[0], s, r, 1, 102, 4096)["xy"][:, 1] - (s + 2)
            assert set((rows // 256).tolist()) == {0, 1, 2}, name


@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_periodic_pattern_ties_across_tiles(gpu_ctx, dtype, s):
    """A pattern of period 8 with nms_radius 8: every maximum has equal ones exactly 8 px away, also beyond the 32 px tile borders;
    only the tie rule decides which stand."""
    imgs = ref.periodic8(dtype=dtype)[None]
    for q10 in (0, 512):
        check_against_yardstick(raw_detect(gpu_ctx, imgs, s, 8, rel_q10=q10), imgs, s, 8, rel_q10=q10, where=f"periodic q10 {q10}")
    assert ref.detect(imgs[0], s, 8, 1, 0)["count"] >= 1


# ---- 2. cap and batch shape ---------------------------------------------------------------------------------------------------------
def test_cap_keeps_the_first_in_row_major_order(gpu_ctx):
    img = corner_ref.grid_fixture(77)[0]
    want = ref.detect(img, 1, 5, 1, 563)
    inner = np.linalg.norm(want["xy"][:, None, :] - corner_ref.grid_fixture(77)[1][None], axis=2).min(axis=1) < 1.5
    assert want["count"] == 25 and inner.all(), "the fixture: exactly the 25 saddles above 0.55 of the strongest (the patch rims stay below 0.46)"
    count, xy, hess, resp = raw_detect(gpu_ctx, img[None], 1, 5, rel_q10=563, cap=4)
    assert count[0] == 25
    check_against_yardstick((count, xy, hess, resp), img[None], 1, 5, rel_q10=563, cap=4)
    key = xy[0, :, 1].astype(np.int64) * img.shape[1] + xy[0, :, 0]
    assert (np.diff(key) > 0).all()
    # response_out is optional
    c2, xy2, hess2, resp2 = raw_detect(gpu_ctx, img[None], 1, 5, rel_q10=563, cap=4, with_response=False)
    assert np.array_equal(xy2, xy) and np.array_equal(hess2, hess) and (resp2 == SENTINEL).all()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_batch_equals_single_calls_and_repeats(gpu_ctx, dtype):
    imgs = np.stack([corner_ref.batch_fixture(dtype=dtype)[0][k] for k in range(5)])
    imgs[3] = 7                                                          # a flat image in the middle of the batch
    first = raw_detect(gpu_ctx, imgs, 1, 3, rel_q10=51, cap=32)
    again = raw_detect(gpu_ctx, imgs, 1, 3, rel_q10=51, cap=32)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for k in range(5):
        one = raw_detect(gpu_ctx, imgs[k:k + 1], 1, 3, rel_q10=51, cap=32)
        for a, b in zip(first, one):
            assert a[k].tobytes() == b[0].tobytes(), k
    assert first[0][3] == 0 and first[0].sum() > 0
    check_against_yardstick(first, imgs, 1, 3, rel_q10=51, cap=32)
    # the engine's wrapper: the same numbers, cut to the counts
    for k, (xy, hess, resp, count) in enumerate(gpu_ctx.detect_corners_batch(imgs, 1, 3, 1, 51 / 1024.0, 32)):
        m = min(count, 32)
        assert count == first[0][k] and np.array_equal(xy, first[1][k, :m]) and np.array_equal(hess, first[2][k, :m])
        assert np.array_equal(resp, first[3][k, :m])


def test_no_images_is_valid(gpu_ctx):
    for fn in (gpu_ctx.lib.ccal_detect_corners_batch, gpu_ctx.lib.ccal_detect_corners_dev):
        assert fn(gpu_ctx.handle, _ffi.PIX_U8, 67, 45, 0, None, 1, 5, 1, 102, 16, None, None, None, None) == _ffi.OK
    assert gpu_ctx.detect_corners_dev(0, _ffi.PIX_U8, 67, 45, 0) == []


@pytest.mark.parametrize("limit", [1, 400000])
def test_a_batch_cut_into_chunks(dev_ctx, gpu_ctx, monkeypatch, limit):
    """The library runs a batch whose workspace would exceed one 256 MB block in chunks.  The second library reads the limit from
    CCAL_TEST_DETECT_CHUNK_BYTES (tests only): 1 byte - every image a chunk of its own -, and 400 000 bytes - chunks of 3, 3 and 1
    of seven 67 x 45 images at nms_radius 1 (108 KB of slots, rows and image each).  Host and device entry: the product's bytes."""
    import torch
    rng = np.random.default_rng(9)
    imgs = np.concatenate([corner_ref.batch_fixture()[0], rng.integers(0, 256, (2, 45, 67)).astype(np.uint8)])
    imgs[4] = 3                                                          # a flat image in the middle
    whole = raw_detect(gpu_ctx, imgs, 1, 1, rel_q10=20, cap=16)
    assert (whole[0] > 16).any() and whole[0][4] == 0
    check_against_yardstick(whole, imgs, 1, 1, rel_q10=20, cap=16)
    monkeypatch.setenv("CCAL_TEST_DETECT_CHUNK_BYTES", str(limit))
    raw = torch.from_numpy(imgs.copy()).cuda()
    torch.cuda.synchronize()
    for got in (raw_detect(dev_ctx, imgs, 1, 1, rel_q10=20, cap=16),
                raw_detect(dev_ctx, imgs, 1, 1, rel_q10=20, cap=16, fn=dev_ctx.lib.ccal_detect_corners_dev, ptr=raw.data_ptr())):
        for x, y in zip(whole, got):
            assert x.tobytes() == y.tobytes()


# ---- 3. threshold -------------------------------------------------------------------------------------------------------------------
def test_threshold(gpu_ctx):
    img = corner_ref.grid_fixture(77)[0]
    every = ref.detect(img, 1, 5, 1, 0)
    rmax = every["rmax"]
    resp = np.sort(every["response"])[::-1]
    # a rel_q10 whose threshold falls strictly between two neighbouring candidates of the yardstick
    cut = next(q for q in range(1, 1024) for i in range(len(resp) - 1) if resp[i + 1] < (rmax >> 10) * q <= resp[i] and resp[i + 1] >= 1)
    for q10 in (0, cut, 1024):
        imgs = img[None]
        check_against_yardstick(raw_detect(gpu_ctx, imgs, 1, 5, rel_q10=q10), imgs, 1, 5, rel_q10=q10, where=f"q10 {q10}")
    n_cut = ref.detect(img, 1, 5, 1, cut)["count"]
    assert ref.detect(img, 1, 5, 1, 1024)["count"] <= n_cut < every["count"]
    assert ref.detect(img, 1, 5, 1, cut - 1)["count"] >= n_cut
    # min_response: just reached by the strongest, then above it
    for minr, n in ((rmax, 1), (rmax + 1, 0)):
        got = raw_detect(gpu_ctx, img[None], 1, 5, min_response=minr, rel_q10=0)
        assert got[0][0] == n
        check_against_yardstick(got, img[None], 1, 5, min_response=minr, rel_q10=0)


# ---- 4. the _dev entry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_dev_entry_point_gives_the_host_calls_bits(gpu_ctx, dtype):
    import torch
    imgs = corner_ref.batch_fixture(dtype=dtype)[0]
    host = raw_detect(gpu_ctx, imgs, 1, 5, rel_q10=51, cap=32)
    raw = torch.from_numpy(imgs.view(np.uint8).copy()).cuda()                        # the bytes of the image block, torch-allocated
    torch.cuda.synchronize()
    dev = raw_detect(gpu_ctx, imgs, 1, 5, rel_q10=51, cap=32, fn=gpu_ctx.lib.ccal_detect_corners_dev, ptr=raw.data_ptr())
    assert host[0].sum() > 0
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()
    wrapped = gpu_ctx.detect_corners_dev(raw.data_ptr(), _code(dtype), imgs.shape[2], imgs.shape[1], len(imgs), 1, 5, 1, 51 / 1024.0, 32)
    assert [w[3] for w in wrapped] == list(host[0])


# ---- invalid arguments ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(gpu_ctx):
    img = np.zeros((2, 45, 67), dtype=np.uint8)
    good = dict(dtype=_ffi.PIX_U8, w=67, h=45, n=2, img=C.c_void_p(img.ctypes.data), s=1, r=5, minr=1, q10=102, cap=8, count=True, xy=True,
                hess=True)
    bad = [dict(s=0), dict(s=5), dict(r=0), dict(r=16), dict(minr=0), dict(minr=-5), dict(q10=-1), dict(q10=1025), dict(cap=0),
           dict(dtype=2), dict(dtype=-1), dict(w=0), dict(h=-1), dict(n=-1), dict(w=65536, h=32768), dict(img=None), dict(count=False),
           dict(xy=False), dict(hess=False)]
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    for fn in (gpu_ctx.lib.ccal_detect_corners_batch, gpu_ctx.lib.ccal_detect_corners_dev):
        for change in bad:
            a = dict(good, **change)
            count = np.full(2, SENTINEL, dtype=np.int32); xy = np.full((2, 8, 2), SENTINEL, dtype=np.int32)
            hess = np.full((2, 8, 3), SENTINEL, dtype=np.int32); resp = np.full((2, 8), SENTINEL, dtype=np.int64)
            rc = fn(gpu_ctx.handle, a["dtype"], a["w"], a["h"], a["n"], a["img"], a["s"], a["r"], a["minr"], a["q10"], a["cap"],
                    count.ctypes.data_as(ip) if a["count"] else None, xy.ctypes.data_as(ip) if a["xy"] else None,
                    hess.ctypes.data_as(ip) if a["hess"] else None, resp.ctypes.data_as(lp))
            assert rc == _ffi.ERR_INVALID_ARG, change
            assert all((v == SENTINEL).all() for v in (count, xy, hess, resp)), change
            assert gpu_ctx.last_error()
    with pytest.raises(ValueError):
        gpu_ctx.detect_corners_batch(np.zeros((1, 45, 67, 3), dtype=np.uint8))                              # colour
    with pytest.raises(ValueError):
        gpu_ctx.detect_corners_batch(img, rel_threshold=float("nan"))


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_detect_checkerboard_equals_the_cpu_pipeline(gpu_ctx, dtype):
    from test_detect_cpu import cpu_pipeline, expected_labelling
    imgs, truth = ref.board_frames(dtype)
    pts = api.detect_checkerboard_points(list(imgs), PATTERN, ref.BOARD_SQUARE, half_win=ref.BOARD_HALF_WIN, ctx=gpu_ctx)
    frames = api.detect_checkerboard(list(imgs), PATTERN, ref.BOARD_SQUARE, half_win=ref.BOARD_HALF_WIN, ctx=gpu_ctx)
    assert len(pts) == len(frames) == 3
    for k in range(3):
        want = cpu_pipeline(imgs[k])
        assert want is not None and pts[k] is not None and sorted(pts[k]) == sorted(want) == list(range(35))
        d = max(max(abs(pts[k][i][0] - want[i][0]), abs(pts[k][i][1] - want[i][1])) for i in range(35))
        got = np.array([pts[k][i] for i in range(35)])
        worst = float(np.linalg.norm(got - expected_labelling(truth[k]), axis=1).max())
        print(f"frame {k}: max |d position| against the CPU pipeline {d:.3e} px, worst distance to the truth {worst:.5f} px")
        assert d <= 1e-9 and worst <= ref.BOARD_BOUND
        f = frames[k]
        assert f is not None and f.time_ns == k and f.img_w_h == (ref.BOARD_W, ref.BOARD_H) and sorted(f.features) == list(range(35))
        for i in range(35):
            assert f.features[i].p2d == (float(np.float32(pts[k][i][0])), float(np.float32(pts[k][i][1])))
            assert f.features[i].p3d == ((i % 7) * ref.BOARD_SQUARE, (i // 7) * ref.BOARD_SQUARE, 0.0)
    blank = api.detect_checkerboard([np.full((60, 80), 9, dtype=dtype), imgs[0][:60, :80]], PATTERN, ref.BOARD_SQUARE, ctx=gpu_ctx)
    assert blank == [None, None]                                         # a flat frame, and a frame that shows a part of the board


# ---- 6. the allocation poison --------------------------------------------------------------------------------------------------------
def test_parity_on_poisoned_workspace(dev_ctx, monkeypatch):
    """The second library with CCAL_TEST_POISON_ALLOC=1 (tests/test_gpu_poison.py): the slots' payload and the stored rows start as
    0xFF bytes in every call; a kernel that read one it had not written would return -1s."""
    monkeypatch.setenv("CCAL_TEST_POISON_ALLOC", "1")
    for dtype in (np.uint8, np.uint16):
        imgs = parity_images(dtype, 1)["67 x 45"]
        for r in (1, 5):
            check_against_yardstick(raw_detect(dev_ctx, imgs, 1, r, rel_q10=0, cap=64), imgs, 1, r, rel_q10=0, cap=64, where="poisoned")
    grid = corner_ref.grid_fixture(311)[0][None]
    check_against_yardstick(raw_detect(dev_ctx, grid, 1, 5), grid, 1, 5, where="poisoned grid")
