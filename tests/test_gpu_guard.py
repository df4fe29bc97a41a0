"""GPU: every one-shot call with guard bands round every slice of its device block (CallBlock, csrc/ccal_call.hpp).

A one-shot entry point cuts ONE device allocation into slices that start on 256-byte boundaries.  A kernel that stores past the end of
its slice, or in front of it, faults nothing: the bytes are the block's own - the slack up to the next boundary, or the head of the
neighbouring slice, which an upload or a clear usually overwrites before anyone looks.  The second library with
CCAL_TEST_GUARD_SLICES=1 lays the block out with a guard of 0xA5 bytes in front of the first slice and from the EXACT end of every
present slice over at least 256 bytes, and finish() reads the guards back: the first damaged byte is CCAL_ERR_HIP with the call, the
slice's ordinal and the byte's distance from the slice's end in the context's message.

1. the proof that the check sees a stray byte (ccal_test_guard_damage: a block of three slices, one byte damaged by the host);
2. every one-shot call under the guard, on the smallest cases of the parity tests' own factories that sit on an edge where a store can
   run over (caps below the counts, 63 / 64 / 65 rows, chunks of uneven size, odd widths): CCAL_OK, and bit for bit the outputs of the
   same call on the same context without the variable - the layout must not leak into a result;
3. the list of calls is complete: every *_batch name of _ffi.SYMBOLS but ccal_solve_batch (persistent workspaces: another design) and
   the one-shot calls of other names were run here, and csrc/ holds as many CallBlock construction sites as this file knows of.

No tolerance anywhere: exact statuses, exact messages, equal bytes.  Every case takes well under a second on the device; the inputs
that need a numpy yardstick to be built (the board candidates) are computed once and shared with tests/test_gpu_board.py."""
import ctypes as C
import functools
import glob
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_ref  # noqa: E402
import detect_ref  # noqa: E402
import pnp_ref  # noqa: E402
import quad_ref  # noqa: E402
import rdh_ref  # noqa: E402
import render_ref  # noqa: E402
import small_factors as sf  # noqa: E402
import tag_ref  # noqa: E402
import tagchain_ref  # noqa: E402
import test_gpu_board as t_board  # noqa: E402
import test_gpu_detect as t_detect  # noqa: E402
import test_gpu_detect_tags as t_chain  # noqa: E402
import test_gpu_quads as t_quads  # noqa: E402
import test_gpu_rdh as t_rdh  # noqa: E402
import test_gpu_refine as t_refine  # noqa: E402
import test_gpu_render as t_render  # noqa: E402
import test_gpu_rig_refine as t_rig  # noqa: E402
import test_gpu_tags as t_tags  # noqa: E402
import test_gpu_undistort as t_und  # noqa: E402
import undistort_ref  # noqa: E402
from test_board_cpu import synthetic  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = "CCAL_TEST_GUARD_SLICES"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, LP, DP = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)

# The one-shot calls: every name here has to be run under the guard by a test of this module (test_every_one_shot_call_was_guarded).
# ccal_project_points and ccal_unproject_points share one construction site, ccal_propose_quads_batch has two (the second block holds
# the stored rows); the _dev forms go through their _batch form's site.
ONE_SHOT_CALLS = (
    "ccal_detect_corners_batch", "ccal_refine_corners_batch", "ccal_propose_quads_batch", "ccal_decode_tags_batch", "ccal_detect_tags_batch",
    "ccal_assemble_checkerboards_batch", "ccal_detect_checkerboards_batch", "ccal_render_targets_batch", "ccal_remap",
    "ccal_project_points", "ccal_unproject_points", "ccal_refine_poses_batch", "ccal_refine_rig_poses_batch", "ccal_pnp_batch",
    "ccal_rdh_batch", "ccal_init_poses_division", "ccal_convert_model", "ccal_test_merge_points", "ccal_test_select_tags")
# CallBlock construction sites in csrc/: the 19 of the calls above and the one of ccal_test_guard_damage.  A call that adds one has to
# come here: into ONE_SHOT_CALLS, into a test below, and into this number.
CONSTRUCTION_SITES = 19 + 1
RAN = set()


@pytest.fixture(scope="module", autouse=True)
def _product_library_first(gpu_ctx):
    """The product library is loaded into the global scope, the second one locally: torch, which hands the _dev forms their images,
    finds the GPU only through the HIP runtime the product library brought in - as in every module that uses both contexts."""


def _flat(x):
    """The bytes of a result: arrays, numbers, and lists / tuples / dicts of them, in order."""
    if isinstance(x, dict):
        return b"".join(str(k).encode() + b"=" + _flat(x[k]) + b";" for k in sorted(x, key=str))
    if isinstance(x, (list, tuple)):
        return b"[" + b",".join(_flat(v) for v in x) + b"]"
    if x is None:
        return b"None"
    a = np.ascontiguousarray(x)
    return str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()


def both(monkeypatch, call, fn, where=""):
    """fn() without the variable and with it: the guarded run came back (a damaged guard is an error status, which fn raises or
    asserts on) with the unguarded run's bytes.  Returns the unguarded result."""
    monkeypatch.delenv(GUARD, raising=False)
    plain = fn()
    monkeypatch.setenv(GUARD, "1")
    try:
        guarded = fn()
    finally:
        monkeypatch.delenv(GUARD, raising=False)
    assert _flat(guarded) == _flat(plain), (call, where)
    RAN.add(call)
    return plain


def ok(ctx, out):
    """A raw helper's dict: CCAL_OK, or the context's message."""
    assert out["rc"] == _ffi.OK, ctx.last_error()
    return out


def _on_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


# ---- 1. the check itself ------------------------------------------------------------------------------------------------------------
def _damage(ctx, slice_, from_end, delta):
    fn = ctx.lib.ccal_test_guard_damage
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64]
    rc = fn(ctx.handle, slice_, from_end, delta)
    return rc, (ctx.last_error() if rc != _ffi.OK else "")


# the block: double x 5 (40 bytes, 216 of slack), an absent slice, int32 x 65 (260 bytes, 252 of slack); guards of slack + 256 bytes
DAMAGE = [
    ("the first byte past slice 0, in its slack", (0, 1, 0), "guard after slice 0 damaged, 0 bytes past the slice's end"),
    ("the last byte of slice 0's guard", (0, 1, 216 + 256 - 1), "guard after slice 0 damaged, 471 bytes past the slice's end"),
    ("the first byte past slice 2", (2, 1, 0), "guard after slice 2 damaged, 0 bytes past the slice's end"),
    ("the last byte in front of slice 0", (0, 0, -1), "guard in front of the block damaged, 1 bytes in front of the first slice"),
    ("a byte inside slice 2", (2, 1, -1), None),
]


@pytest.mark.parametrize("what,pos,message", DAMAGE, ids=[d[0] for d in DAMAGE])
def test_the_guard_sees_one_stray_byte(dev_ctx, monkeypatch, what, pos, message):
    """One byte written by a host-issued memset inside the block's own allocation: with the variable the call ends in CCAL_ERR_HIP
    and names the slice the guard follows and the distance; a byte inside a slice is nobody's business.  Without the variable the
    same positions all end in CCAL_OK: the product path has no guards and checks nothing (the byte in front of slice 0 lies outside
    that block, the hook does not write it)."""
    monkeypatch.delenv(GUARD, raising=False)
    assert _damage(dev_ctx, *pos) == (_ffi.OK, "")
    monkeypatch.setenv(GUARD, "1")
    rc, msg = _damage(dev_ctx, *pos)
    if message is None:
        assert (rc, msg) == (_ffi.OK, "")
    else:
        assert rc == _ffi.ERR_HIP and msg == "ccal_test_guard_damage: " + message, (rc, msg)
    monkeypatch.setenv(GUARD, "0")                                      # only "1" switches it on
    assert _damage(dev_ctx, *pos) == (_ffi.OK, "")


# ---- 2. the image stages ------------------------------------------------------------------------------------------------------------
def test_detect_corners(dev_ctx, monkeypatch):
    """u8 and u16 at 67 x 45 (nms_radius 1 and 5: 24 x 21 and 8 x 7 slots), a candidate cap below the count, a batch of images too small
    for a domain beside one that has one, seven images in chunks of 3, 3 and 1, the _dev form."""
    call = "ccal_detect_corners_batch"
    for dtype in (np.uint8, np.uint16):
        imgs = t_detect.parity_images(dtype, 1)
        for r in (1, 5):
            got = both(monkeypatch, call, lambda: t_detect.raw_detect(dev_ctx, imgs["67 x 45"], 1, r, rel_q10=0, cap=4096), f"67 x 45 r {r}")
            capped = both(monkeypatch, call, lambda: t_detect.raw_detect(dev_ctx, imgs["67 x 45"], 1, r, rel_q10=0, cap=7), f"cap 7 r {r}")
            assert (got[0] > 7).all() and np.array_equal(capped[0], got[0])
        none = both(monkeypatch, call, lambda: t_detect.raw_detect(dev_ctx, imgs["no domain"], 1, 5), "no domain")
        assert (none[0] == 0).all()
        both(monkeypatch, call, lambda: t_detect.raw_detect(dev_ctx, imgs["domain 2 x 2"], 1, 5, rel_q10=0), "domain 2 x 2")
    rng = np.random.default_rng(9)
    seven = np.concatenate([corner_ref.batch_fixture()[0], rng.integers(0, 256, (2, 45, 67)).astype(np.uint8)])
    seven[4] = 3
    whole = both(monkeypatch, call, lambda: t_detect.raw_detect(dev_ctx, seven, 1, 1, rel_q10=20, cap=16), "seven")
    assert (whole[0] > 16).any() and whole[0][4] == 0
    raw = _on_device(seven)
    monkeypatch.setenv("CCAL_TEST_DETECT_CHUNK_BYTES", "400000")
    for kw in (dict(), dict(fn=dev_ctx.lib.ccal_detect_corners_dev, ptr=raw.data_ptr())):
        cut = both(monkeypatch, call, lambda: t_detect.raw_detect(dev_ctx, seven, 1, 1, rel_q10=20, cap=16, **kw), "chunks of 3, 3, 1")
        assert _flat(cut) == _flat(whole)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_refine_corners(dev_ctx, monkeypatch, dtype):
    """0, 1, 63, 64 and 65 corners in the five images of one call; the _dev form."""
    imgs, xy = corner_ref.batch_fixture(dtype=dtype)
    assert tuple(len(p) for p in xy) == (0, 1, 63, 64, 65)
    h = corner_ref.BATCH_HALF_WIN
    host = both(monkeypatch, "ccal_refine_corners_batch", lambda: dev_ctx.refine_corners_batch(imgs, xy, h, 8, 0.0))
    raw = _on_device(imgs)
    code = _ffi.PIX_U8 if dtype == np.uint8 else _ffi.PIX_U16
    dev = both(monkeypatch, "ccal_refine_corners_batch",
               lambda: dev_ctx.refine_corners_dev(raw.data_ptr(), code, corner_ref.BATCH_W, corner_ref.BATCH_H, len(imgs), xy, h, 8, 0.0), "_dev")
    assert _flat(dev) == _flat(host)


def test_propose_quads(dev_ctx, monkeypatch):
    """A cap of one row, out-edge lists that overflow, five images of 130, 0, 65, 4 and 130 points - whole, in chunks of (0, 1), (2, 3),
    (4), an image per chunk, and through the _dev form, whose chunks do not hold the pixels."""
    call = "ccal_propose_quads_batch"
    for name in ("cap 1", "out-edge overflow", "five images"):
        case = quad_ref.parity_case(name)
        both(monkeypatch, call, lambda: ok(dev_ctx, t_quads.raw_propose(dev_ctx, case)), name)
    lean = quad_ref.parity_case("five images")
    both(monkeypatch, call, lambda: ok(dev_ctx, t_quads.raw_propose(dev_ctx, lean, want_quads=False)), "no quads_out")
    case = quad_ref.batch_case()
    whole = both(monkeypatch, call, lambda: ok(dev_ctx, t_quads.raw_propose(dev_ctx, case)), "batch")
    raw = _on_device(case["images"])
    for which in (0, 1):
        monkeypatch.setenv("CCAL_TEST_QUADS_CHUNK_BYTES", str(quad_ref.CHUNK_LIMITS_HOST[which]))
        cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_quads.raw_propose(dev_ctx, case)), f"chunks {which}")
        assert t_quads.bits(cut) == t_quads.bits(whole)
        monkeypatch.setenv("CCAL_TEST_QUADS_CHUNK_BYTES", str(quad_ref.CHUNK_LIMITS_DEV[which]))
        cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_quads.raw_propose(dev_ctx, case, fn=dev_ctx.lib.ccal_propose_quads_dev, ptr=raw.data_ptr())),
                   f"_dev chunks {which}")
        assert t_quads.bits(cut) == t_quads.bits(whole)


def test_decode_tags(dev_ctx, monkeypatch):
    """Three images of which the middle one has no quads - whole, an image per chunk, the first two together; without the optional
    outputs; a table of 65 codes; the _dev form."""
    call = "ccal_decode_tags_batch"
    case = tag_ref.batch_case()
    assert len(case["quads_list"][1]) == 0
    whole = both(monkeypatch, call, lambda: ok(dev_ctx, t_tags.raw_decode(dev_ctx, case)), "batch")
    both(monkeypatch, call, lambda: ok(dev_ctx, t_tags.raw_decode(dev_ctx, case, optional=False)), "lean")
    table = next(c for c in tag_ref.table_cases() if len(c["codes"]) == 65)
    both(monkeypatch, call, lambda: ok(dev_ctx, t_tags.raw_decode(dev_ctx, table)), "table of 65")
    raw = _on_device(case["images"])
    for which in (0, 1):
        monkeypatch.setenv("CCAL_TEST_TAGS_CHUNK_BYTES", str(tag_ref.CHUNK_LIMITS_HOST[which]))
        cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_tags.raw_decode(dev_ctx, case)), f"chunks {which}")
        assert t_tags.bits(cut) == t_tags.bits(whole)
        monkeypatch.setenv("CCAL_TEST_TAGS_CHUNK_BYTES", str(tag_ref.CHUNK_LIMITS_DEV[which]))
        cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_tags.raw_decode(dev_ctx, case, fn=dev_ctx.lib.ccal_decode_tags_dev, ptr=raw.data_ptr())),
                   f"_dev chunks {which}")
        assert t_tags.bits(cut) == t_tags.bits(whole)


def test_detect_tags(dev_ctx, monkeypatch):
    """The mixed batch (a frame, a blank image, a checkerboard without tags, a cropped frame); the four frames with a tag cap, a quad
    cap, a candidate cap and all three below the counts; the four frames in chunks of 3 and 1 - the block is sized for the chunk of
    three and serves the chunk of one - and of 1; the _dev form."""
    call = "ccal_detect_tags_batch"
    mixed = tagchain_ref.mixed_batch(np.uint8)
    o = tagchain_ref.opts(np.uint8, mixed.shape[2], mixed.shape[1])
    got = both(monkeypatch, call, lambda: ok(dev_ctx, t_chain.raw_detect(dev_ctx, mixed, o)), "mixed")
    assert got["count"][1] == 0 and got["count"][3] == 4
    frames = t_chain.frames(np.uint8)
    for caps in (dict(tag_cap=2), dict(quad_cap=1), dict(cand_cap=60), dict(cand_cap=90, quad_cap=2, tag_cap=1)):
        oc = tagchain_ref.opts(np.uint8, **caps)
        got = both(monkeypatch, call, lambda: ok(dev_ctx, t_chain.raw_detect(dev_ctx, frames, oc)), str(caps))
        assert (got["flags"] != 0).all()
    o = tagchain_ref.opts(np.uint8, nms_radius=3)
    whole = both(monkeypatch, call, lambda: ok(dev_ctx, t_chain.raw_detect(dev_ctx, frames, o)), "frames")
    raw = _on_device(frames)
    for per_chunk in (3, 1):
        monkeypatch.setenv("CCAL_TEST_TAGCHAIN_CHUNK_BYTES", str(tagchain_ref.chunk_limit(False, frames.shape[1:], 1, o, len(t_chain.CODES), per_chunk)))
        cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_chain.raw_detect(dev_ctx, frames, o)), f"chunks of {per_chunk}")
        assert t_chain.bits(cut) == t_chain.bits(whole)
        monkeypatch.setenv("CCAL_TEST_TAGCHAIN_CHUNK_BYTES", str(tagchain_ref.chunk_limit(True, frames.shape[1:], 1, o, len(t_chain.CODES), per_chunk)))
        cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_chain.raw_detect(dev_ctx, frames, o, fn=dev_ctx.lib.ccal_detect_tags_dev, ptr=raw.data_ptr())),
                   f"_dev chunks of {per_chunk}")
        assert t_chain.bits(cut) == t_chain.bits(whole)


@functools.lru_cache(maxsize=None)
def _kept(kept):
    """Two frames' candidates with strays, `kept` rows kept each (tests/test_gpu_board.py: test_kept_counts_at_the_lane_boundaries)."""
    return tuple(t_board.strays(k, kept - 35, 2000 + kept, 1.0, 1.1) for k in (0, 2))


@pytest.mark.parametrize("kept", [63, 64, 65])
def test_assemble_checkerboards_kept_counts(dev_ctx, monkeypatch, kept):
    cases = _kept(kept)
    got = both(monkeypatch, "ccal_assemble_checkerboards_batch",
               lambda: ok(dev_ctx, t_board.raw_assemble(dev_ctx, [c[0] for c in cases], [c[1] for c in cases])), f"kept {kept}")
    assert (got["stats"][:, 0] == kept).all()


def test_assemble_checkerboards_limits_patterns_and_chunks(dev_ctx, monkeypatch):
    """The kept limit exceeded by one row (513) beside a frame and a batch member without rows; the smallest pattern (2 x 2: the call
    refuses a side of 1) and a square one (5 x 5); the largest (20 x 20: 400 corners); four images in chunks of one and of two."""
    call = "ccal_assemble_checkerboards_batch"
    frame = t_board._candidates(0)
    over = synthetic(27, 19)
    got = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_assemble(dev_ctx, [frame[0], over[0], over[0][:-1], np.zeros((0, 2))],
                                                                           [frame[1], over[1], over[1][:-1], np.zeros((0, 3))])), "kept limit")
    assert got["flags"].tolist() == [0, _ffi.BOARD_FLAG_KEPT_LIMIT, 0, 0] and got["stats"][1, 0] == 513 and got["stats"][2, 0] == 512
    two = [synthetic(2, 2), synthetic(3, 3)]
    got = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_assemble(dev_ctx, [c[0] for c in two], [c[1] for c in two], 2, 2)), "2 x 2")
    assert got["found"].tolist() == [1, 0]
    five = synthetic(5, 5)
    got = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_assemble(dev_ctx, [five[0]], [five[1]], 5, 5)), "5 x 5")
    assert got["found"].tolist() == [1]
    big = synthetic(20, 20, pitch=12.0)
    got = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_assemble(dev_ctx, [big[0]], [big[1]], 20, 20)), "20 x 20")
    assert got["found"].tolist() == [1]
    cases = [frame, (np.zeros((0, 2)), np.zeros((0, 3))), _kept(65)[0], _kept(63)[1]]
    whole = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_assemble(dev_ctx, [c[0] for c in cases], [c[1] for c in cases])), "four")
    for limit in ("1", "25000"):
        monkeypatch.setenv("CCAL_TEST_BOARD_CHUNK_BYTES", limit)
        cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_assemble(dev_ctx, [c[0] for c in cases], [c[1] for c in cases])), limit)
        assert t_board.bits(cut) == t_board.bits(whole)


def test_detect_checkerboards(dev_ctx, monkeypatch):
    """Three frames, a flat image and a partial board, u8 and u16; a candidate cap below the counts; a field of 609 saddles that
    exceeds the kept limit; 129 images (two carries of the offset scan, image 64 blank); chunks of one and of two; the _dev form."""
    call = "ccal_detect_checkerboards_batch"
    for dtype in (np.uint8, np.uint16):
        frames = detect_ref.board_frames(dtype)[0]
        imgs = np.concatenate([frames, np.full_like(frames[:1], 90), t_board.cropped(dtype)[None]])
        whole = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_detect(dev_ctx, imgs, t_board.OPTS)), np.dtype(dtype).name)
        assert whole["found"].tolist() == [1, 1, 1, 0, 0]
    capped = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_detect(dev_ctx, frames, dict(t_board.OPTS, cand_cap=45))), "cand_cap 45")
    assert (capped["flags"] == _ffi.BOARD_FLAG_CAND_CAP).all()
    field = np.stack([t_board.saddle_field(), detect_ref.board_frames()[0][0]])
    over = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_detect(dev_ctx, field, dict(t_board.OPTS, nms_radius=3, half_win=3))), "saddle field")
    assert over["flags"].tolist() == [_ffi.BOARD_FLAG_KEPT_LIMIT, 0] and over["found"].tolist() == [0, 1]
    frames = detect_ref.board_frames()[0]
    many = np.ascontiguousarray(frames[np.arange(129) % 3])
    many[64] = 0
    got = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_detect(dev_ctx, many, t_board.OPTS)), "129 images")
    assert got["found"][64] == 0 and got["found"].sum() == 128
    imgs = np.concatenate([frames, np.full_like(frames[:1], 90), t_board.cropped()[None]])
    whole = t_board.raw_detect(dev_ctx, imgs, t_board.OPTS)
    raw = _on_device(imgs)
    for limit in ("1", "800000"):
        monkeypatch.setenv("CCAL_TEST_BOARD_CHUNK_BYTES", limit)
        for kw in (dict(), dict(fn=dev_ctx.lib.ccal_detect_checkerboards_dev, ptr=raw.data_ptr())):
            cut = both(monkeypatch, call, lambda: ok(dev_ctx, t_board.raw_detect(dev_ctx, imgs, t_board.OPTS, **kw)), f"chunk limit {limit}")
            assert t_board.bits(cut) == t_board.bits(whole)


def test_render_targets(dev_ctx, monkeypatch):
    """130 x 67 at supersampling 1 with first_id 4, one pixel, a u16 case of odd width, 65 images in chunks of 7 (the last of 2)."""
    call = "ccal_render_targets_batch"
    cases = t_render.CASES
    odd_u16 = next(c for c in render_ref.parity_cases() if c["dtype"] == np.uint16 and c["width"] % 2 == 1 and c["width"] > 1)
    for case in (cases["grid opencv5 130 x 67 s 1 first_id 4"], cases["board kb4 1 x 1"], odd_u16):
        both(monkeypatch, call, lambda: t_render._render(dev_ctx, case), case["name"])
    case = cases["grid eucm 65 images s 1"]
    whole = both(monkeypatch, call, lambda: t_render._render(dev_ctx, case), "65 images")
    monkeypatch.setenv("CCAL_TEST_RENDER_CHUNK_BYTES", str(7 * 67 * 45))
    cut = both(monkeypatch, call, lambda: t_render._render(dev_ctx, case), "65 images by 7")
    assert np.array_equal(cut, whole)


@pytest.mark.parametrize("n_img", [1, 5])
@pytest.mark.parametrize("dtype,ch", [(np.uint8, 3), (np.uint16, 1)], ids=["u8x3", "u16"])
def test_remap(dev_ctx, monkeypatch, dtype, ch, n_img):
    """Maps of 37 x 23 and 130 x 67 pixels - 851 and 8710: no multiple of 4 - and the map with NaN, infinite and border coordinates."""
    imgs = t_und._images(dtype, ch, n_img)
    for name, maps in (("37 x 23", t_und._random_maps(37, 23)), ("130 x 67", t_und._random_maps(130, 67)), ("edges", t_und._edge_maps())):
        m = dev_ctx.undistort_map_from_arrays(*maps)
        try:
            both(monkeypatch, "ccal_remap", lambda: m.remap(imgs), name)
        finally:
            m.close()


@pytest.mark.parametrize("name", t_und.MODELS)
def test_project_and_unproject_points(dev_ctx, monkeypatch, name):
    m, p = t_und._mp(name)
    for n in (1, 255, 256, 257):
        xyz = undistort_ref.seeded_rays(m, n)
        both(monkeypatch, "ccal_project_points", lambda: dev_ctx.project_points(m, p, xyz), f"{name} n {n}")
        uv = undistort_ref.seeded_pixels(p, n, t_und.W, t_und.H)
        both(monkeypatch, "ccal_unproject_points", lambda: dev_ctx.unproject_points(m, p, uv), f"{name} n {n}")


# ---- 3. the pose calls --------------------------------------------------------------------------------------------------------------
REFINE_COUNTS = [4, 5, 63, 64, 65, 128, 129, 300, 0]


@pytest.mark.parametrize("with_errors", [False, True], ids=["no errors", "errors"])
def test_refine_poses(dev_ctx, monkeypatch, with_errors):
    """Problems of 4 .. 300 points and one of none: all nine in one call, five of them, each of 65 and 0 points alone."""
    m, par, X, U, start, _ = t_refine._shape_frames(REFINE_COUNTS)
    for sel in (list(range(9)), [8, 2, 3, 4, 7], [4], [8]):
        out = both(monkeypatch, "ccal_refine_poses_batch",
                   lambda: dev_ctx.refine_poses_batch(m, par, [X[f] for f in sel], [U[f] for f in sel], start[sel], 1.0, 4, t_refine._tight(),
                                                      with_errors=with_errors), str(sel))
        assert [int(v) for v in out[3]] == [REFINE_COUNTS[f] for f in sel]


@pytest.mark.parametrize("with_errors", [False, True], ids=["no errors", "errors"])
def test_refine_rig_poses(dev_ctx, monkeypatch, with_errors):
    """The nine slots of tests/test_gpu_rig_refine.py over the cameras of rig B: segments of 4 .. 300 points, slots that one camera
    alone sees, an empty segment between two full ones - all nine, five, one."""
    rig, slots, start, _, _ = t_rig._shape_slots()
    assert [len(s) for s in t_rig.SHAPES].count(1) >= 1
    for sel in (list(range(9)), [8, 7, 6, 5, 4], [2], [0]):
        out = both(monkeypatch, "ccal_refine_rig_poses_batch",
                   lambda: t_rig._run(dev_ctx, rig, [slots[s] for s in sel], start[sel], t_refine._tight(), with_errors=with_errors), str(sel))
        assert [int(v) for v in out[3]] == [t_rig._total(slots[s]) for s in sel]


def test_pnp_batch(dev_ctx, monkeypatch):
    """Ragged frames of a cube of 100 points and of the hinged boards, exact normalised points; with and without the cost."""
    for board in (synth.cube_points(100), synth.hinged_boards()):
        sp = synth.make_problem(5, "eucm", board=board, ragged=True)
        fr = [(int(sp.obs_offsets[o]), int(sp.obs_offsets[o + 1])) for o in range(sp.n_obs)]
        X = [sp.p3d[a:b].astype(np.float64) for a, b in fr]
        xn = [pnp_ref.true_normalised_points(X[f], sp.poses_gt[f]) for f in range(len(fr))]
        for n_prob in (1, 5):
            for with_cost in (True, False):
                out = both(monkeypatch, "ccal_pnp_batch", lambda: dev_ctx.pnp_batch(X[:n_prob], xn[:n_prob], 4, with_cost=with_cost), f"{n_prob} problems")
                assert (out[1] == [len(x) for x in X[:n_prob]]).all()


def test_rdh_batch(dev_ctx, monkeypatch):
    """100 and 65 hypotheses (no multiples of 64); problems of 1024 pairs (the last size staged in LDS) and of 1025 (global memory),
    alone and beside small ones; with and without the per-hypothesis outputs."""
    lds = 1024                                                          # RDH_LDS_PAIRS, csrc/ccal_rdh.hpp
    assert f"RDH_LDS_PAIRS = {lds};" in open(os.path.join(ROOT, "camera_intrinsic_calibration_rs_amd", "csrc", "ccal_rdh.hpp")).read()
    pairs = {n: rdh_ref.exact_pairs(-0.3, t_rdh.H_TRUE, n, seed=n) for n in (6, 65, lds, lds + 1)}
    for sizes in ([lds], [lds + 1], [6, lds, 65], [65, lds + 1, 6]):
        for n_hyp, per in ((100, True), (65, False)):
            out = both(monkeypatch, "ccal_rdh_batch",
                       lambda: dev_ctx.rdh_batch([pairs[n] for n in sizes], [7 + k for k in range(len(sizes))], n_hyp, per_hypothesis=per),
                       f"{sizes} {n_hyp}")
            assert (out["n_valid"] > 0).all()


def test_init_poses_division(dev_ctx, monkeypatch):
    ff = t_rdh._division_view(-0.3, [0.2, -0.3, 0.1, -0.3, -0.25, 0.9])
    both(monkeypatch, "ccal_init_poses_division", lambda: api.init_pose(ff, -0.3, ctx=dev_ctx))


def test_convert_model(dev_ctx, monkeypatch):
    case = sf.load()["convert"][0]
    out = both(monkeypatch, "ccal_convert_model", lambda: sf.run_convert(dev_ctx.lib, dev_ctx.handle, case), case["name"])
    assert out["rc"] == _ffi.OK


# ---- 4. the two decision-kernel hooks -----------------------------------------------------------------------------------------------
def test_merge_points_hook(dev_ctx, monkeypatch):
    """Images of 0, 1, 63, 64, 65 and 130 points on the half-pixel lattice of tests/test_gpu_detect_tags.py, with and without statuses."""
    rng = np.random.default_rng(20)
    xy_list, status_list = [], []
    for n, span in [(0, 4), (1, 4), (63, 24), (64, 24), (65, 24), (130, 40)]:
        xy_list.append(rng.integers(0, span, (n, 2)).astype(np.float64) * 0.5 + rng.choice([0.0, 1e-9, -1e-9], (n, 2)))
        status_list.append(rng.choice([_ffi.OK, _ffi.OK, _ffi.ERR_NO_CONVERGENCE, _ffi.NO_RESULT], n).astype(np.int32))
    for statuses in (status_list, None):
        both(monkeypatch, "ccal_test_merge_points", lambda: t_chain.hook_merge(dev_ctx, xy_list, statuses, 1.0))


def test_select_tags_hook(dev_ctx, monkeypatch):
    """Images of 1, 64, 65 and 130 decoded quads, 40 stored rows per image: the inputs of tests/test_gpu_detect_tags.py, smaller."""
    rng = np.random.default_rng(21)
    sizes, rows = (1, 64, 65, 130), 40
    n, m = sum(sizes), len(sizes)
    offs = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(sizes, out=offs[1:])
    reason = rng.choice([_ffi.TAG_OK, _ffi.TAG_OK, _ffi.TAG_OK, _ffi.TAG_BORDER, _ffi.TAG_NO_CODE], n).astype(np.int32)
    tag_id, rot, ham = (rng.integers(0, hi, n).astype(np.int32) for hi in (60, 4, 3))
    margin = rng.integers(1, 6, n).astype(np.float64) * 0.5
    corners = rng.random((n, 4, 2)) * 300.0
    fn = dev_ctx.lib.ccal_test_select_tags
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, LP, IP, IP, IP, IP, DP, DP, C.c_int, IP, IP, IP, IP, IP, DP, DP]

    def run():
        out = {"count": np.full(m, -77, np.int32), "n_ok": np.full(m, -77, np.int32), "id": np.full((m, rows), -77, np.int32),
               "rot": np.full((m, rows), -77, np.int32), "hamming": np.full((m, rows), -77, np.int32),
               "corners": np.full((m, rows, 4, 2), -3.25), "margin": np.full((m, rows), -3.25)}
        out["rc"] = fn(dev_ctx.handle, m, offs.ctypes.data_as(LP), reason.ctypes.data_as(IP), tag_id.ctypes.data_as(IP), rot.ctypes.data_as(IP),
                       ham.ctypes.data_as(IP), corners.ctypes.data_as(DP), margin.ctypes.data_as(DP), rows, out["count"].ctypes.data_as(IP),
                       out["n_ok"].ctypes.data_as(IP), out["id"].ctypes.data_as(IP), out["rot"].ctypes.data_as(IP),
                       out["hamming"].ctypes.data_as(IP), out["corners"].ctypes.data_as(DP), out["margin"].ctypes.data_as(DP))
        return ok(dev_ctx, out)

    got = both(monkeypatch, "ccal_test_select_tags", run)
    assert got["count"][3] > rows and got["count"][0] <= 1


# ---- 5. nothing was forgotten -------------------------------------------------------------------------------------------------------
def test_every_one_shot_call_was_guarded():
    """Last in the module.  Every one-shot call was run under the guard above; every *_batch name of the bindings is a one-shot call
    but ccal_solve_batch, whose workspaces are persistent blocks; and csrc/ constructs a CallBlock at exactly the sites counted here."""
    batch = {name for name, _, _ in _ffi.SYMBOLS if name.endswith("_batch")} - {"ccal_solve_batch"}
    assert batch <= set(ONE_SHOT_CALLS), sorted(batch - set(ONE_SHOT_CALLS))
    assert set(ONE_SHOT_CALLS) <= RAN, sorted(set(ONE_SHOT_CALLS) - RAN)
    sites = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "camera_intrinsic_calibration_rs_amd", "csrc", "*.h*"))):
        sites += len(re.findall(r"^\s*(?:ccal::)?CallBlock \w+\(ctx\);", open(path).read(), flags=re.M))
    assert sites == CONSTRUCTION_SITES, sites
