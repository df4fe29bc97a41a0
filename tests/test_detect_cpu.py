"""CPU: the saddle detector's yardstick (tests/detect_ref.py, the numpy restatement of the rule include/ccal.h states at
ccal_detect_corners_batch) on images that can be checked by hand, the whole pipeline detect -> refine -> assemble on the rendered
board fixture, api.assemble_checkerboard on its own, and the argument rules of the entry points that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_ref  # noqa: E402
import detect_ref as ref  # noqa: E402
from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

PATTERN = (ref.BOARD_COLS, ref.BOARD_ROWS)


# ---- 1. the yardstick on hand-checkable images ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_one_saddle_gives_one_candidate(dtype):
    img = corner_ref.render(64, 64, [[30.3, 33.6]], 11, dtype=dtype, radius=80)            # the patch covers the image: no rim
    d = ref.detect(img, step=1, nms_radius=5, min_response=1, rel_q10=102)
    assert d["count"] == 1 and d["xy"].shape == (1, 2)
    assert np.abs(d["xy"][0] - [30.3, 33.6]).max() <= 1.0
    assert d["response"][0] == d["rmax"] > 0


def test_flat_and_edge_give_none():
    flat = np.full((40, 50), 77, dtype=np.uint8)
    edge = np.where(np.arange(50)[None, :] < 23, 30, 200).astype(np.uint8).repeat(40, axis=0)
    for s in (1, 2, 4):
        assert ref.detect(flat, step=s)["count"] == 0
        for e in (edge, edge.T.copy()):                                           # hyy = hxy = 0 (hxx = hxy = 0) exactly
            assert (ref.response(e, s)[0] == 0).all() and ref.detect(e, step=s)["count"] == 0


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_response_of_quadratics_is_the_closed_form(s):
    """I = xy + c: S = 256 (xy + c) (the binomial kernel is symmetric: odd moments vanish, the xy moment factorises), hxx = hyy = 0,
    hxy = 256 * 4 s^2, R = (1024 s^2)^2 = -16 s^4 det H * 256^2 with det H = -1.  I = (x^2 - y^2) / 2 + c over even coordinates
    doubled: the image 2 (x^2 - y^2) + c has hxx = 256 * 4 s^2, hyy = -hxx, hxy = 0, R = 16 * (1024 s^2)^2 - the same saddle, four
    times as steep, 16 times the response."""
    yy, xx = np.mgrid[0:24, 0:24].astype(np.int64)
    R, hxx, hyy, hxy = ref.response((xx * yy + 100).astype(np.uint16), s)
    assert (hxx == 0).all() and (hyy == 0).all() and (hxy == 1024 * s * s).all() and (R == (1024 * s * s) ** 2).all()
    R, hxx, hyy, hxy = ref.response((2 * (xx * xx - yy * yy) + 2000).astype(np.uint16), s)
    assert (hxx == 1024 * s * s).all() and (hyy == -1024 * s * s).all() and (hxy == 0).all() and (R == 16 * (1024 * s * s) ** 2).all()


def test_extreme_magnitudes_stay_below_the_stated_bound():
    for block in (3, 7):
        img = ref.extreme_blocks(block=block)
        assert ref.smooth(img).max() <= 256 * 65535
        for s in (1, 2, 3, 4):
            R, hxx, hyy, hxy = ref.response(img, s)
            assert max(np.abs(hxx).max(), np.abs(hyy).max(), np.abs(hxy).max()) <= 2 ** 25 and np.abs(R).max() < 2 ** 55
    assert ref.detect(ref.extreme_blocks(), step=1, nms_radius=1)["count"] > 0
    assert ref.detect(ref.extreme_blocks(block=7), step=4, nms_radius=1)["count"] > 0


def test_small_images_and_the_tie_rule():
    rng = np.random.default_rng(3)
    for s in (1, 4):
        side = 2 * (s + 2)                                                # no domain
        assert ref.detect(rng.integers(0, 255, (side, side)).astype(np.uint8), step=s)["count"] == 0
        assert ref.response(rng.integers(0, 255, (side + 1, side + 1)).astype(np.uint8), s)[0].shape == (1, 1)
    # equal maxima 8 px apart with nms_radius 8: of two that see each other the first in row-major order stands
    d = ref.detect(ref.periodic8(), step=1, nms_radius=8, min_response=1, rel_q10=0)
    assert d["count"] >= 1
    xy = d["xy"]
    assert (np.maximum(np.abs(xy[:, None, 0] - xy[None, :, 0]), np.abs(xy[:, None, 1] - xy[None, :, 1]))[~np.eye(len(xy), dtype=bool)] > 8).all()


# ---- 2. the whole pipeline on the CPU -----------------------------------------------------------------------------------------------
def cpu_pipeline(img):
    d = ref.detect(img, step=1, nms_radius=5, min_response=1, rel_q10=round(1024 * 0.1))
    r = corner_ref.refine(img, d["xy"].astype(np.float64), ref.BOARD_HALF_WIN, 30, 1e-3)
    good = r["status"] == corner_ref.OK
    return api.assemble_checkerboard(r["xy"][good], d["hess"][good], PATTERN, ref.BOARD_SQUARE)


def expected_labelling(truth):
    """The true corner pixels [rows * cols, 2] under the rule: of the board's two rotations the one whose id 0 is smallest in (y, x)."""
    a, b = truth[0], truth[-1]
    return truth if (a[1], a[0]) < (b[1], b[0]) else truth[::-1]


def test_fixture_is_what_it_says():
    imgs, truth = ref.board_frames()
    assert imgs.shape == (3, ref.BOARD_H, ref.BOARD_W) and truth.shape == (3, 35, 2)
    lams = {f[0] for f in ref.BOARD_FRAMES}
    assert 0.0 in lams and len(lams) == 2
    assert max(abs(f[1]) for f in ref.BOARD_FRAMES) > 45.0 and max(f[2] for f in ref.BOARD_FRAMES) == 35.0
    for t in truth:
        assert t.min() >= 12.0 and (t[:, 0] <= ref.BOARD_W - 13).all() and (t[:, 1] <= ref.BOARD_H - 13).all()
        g = t.reshape(ref.BOARD_ROWS, ref.BOARD_COLS, 2)
        steps = np.concatenate([np.linalg.norm(np.diff(g, axis=0), axis=2).ravel(), np.linalg.norm(np.diff(g, axis=1), axis=2).ravel()])
        assert 21.0 <= steps.min() and steps.max() <= 38.0


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_every_frame_assembles_onto_the_true_corners(dtype):
    imgs, truth = ref.board_frames(dtype)
    worst = 0.0
    for k in range(len(imgs)):
        found = cpu_pipeline(imgs[k])
        assert found is not None, f"frame {k} did not assemble"
        assert sorted(found) == list(range(35))
        pts = np.array([found[i] for i in range(35)])
        worst = max(worst, float(np.linalg.norm(pts - expected_labelling(truth[k]), axis=1).max()))
    print(f"worst distance to the true corner pixel: {worst:.5f} px")
    assert worst <= ref.BOARD_BOUND


# ---- 3. assemble_checkerboard on its own ------------------------------------------------------------------------------------------
def _candidates(k=0):
    img = ref.board_frames()[0][k]
    d = ref.detect(img, step=1, nms_radius=5, min_response=1, rel_q10=102)
    r = corner_ref.refine(img, d["xy"].astype(np.float64), ref.BOARD_HALF_WIN, 30, 1e-3)
    good = r["status"] == corner_ref.OK
    return r["xy"][good], d["hess"][good]


def _inner(xy, truth):
    return np.linalg.norm(xy[:, None, :] - truth[None], axis=2).min(axis=1) < 2.0


def test_a_missing_corner_gives_none():
    xy, hess = _candidates()
    base = api.assemble_checkerboard(xy, hess, PATTERN, ref.BOARD_SQUARE)
    assert base is not None
    inner = np.flatnonzero(_inner(xy, ref.board_frames()[1][0]))
    for drop in (inner[0], inner[17], inner[-1]):                        # a corner of the lattice, one inside, the opposite corner
        keep = np.arange(len(xy)) != drop
        assert api.assemble_checkerboard(xy[keep], hess[keep], PATTERN, ref.BOARD_SQUARE) is None
    assert api.assemble_checkerboard(xy[:10], hess[:10], PATTERN, ref.BOARD_SQUARE) is None
    assert api.assemble_checkerboard(np.zeros((0, 2)), np.zeros((0, 3)), PATTERN, ref.BOARD_SQUARE) is None
    assert api.assemble_checkerboard(xy, hess, (6, 5), ref.BOARD_SQUARE) is None      # the board is not 6 x 5


STRAY_SEEDS = range(1000, 1040)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_spurious_points_and_input_order_change_nothing(k):
    """Six stray candidates anywhere in the image, board included, each with the Hessian of a random true corner at 0.64 to 1.5
    times its strength (the hardest kind: weaker ones are set aside by strength), for every seed of STRAY_SEEDS; and the input in a
    random order.  The one condition on a stray is the detector's own: no two candidates of one image lie within nms_radius (5 px)
    of each other in both x and y, so a stray is redrawn until it is farther than that from every candidate."""
    xy, hess = _candidates(k)
    base = api.assemble_checkerboard(xy, hess, PATTERN, ref.BOARD_SQUARE)
    assert base is not None
    inner = np.flatnonzero(_inner(xy, ref.board_frames()[1][k]))
    inside = 0
    for seed in STRAY_SEEDS:
        rng = np.random.default_rng(seed)
        extra = []
        while len(extra) < 6:
            p = rng.uniform([6.0, 6.0], [ref.BOARD_W - 7.0, ref.BOARD_H - 7.0])
            if np.abs(np.concatenate([xy, np.array(extra).reshape(-1, 2)]) - p).max(axis=1).min() > 5.0:
                extra.append(p)
        extra = np.array(extra)
        inside += int((np.linalg.norm(extra[:, None, :] - xy[inner][None], axis=2).min(axis=1) < 25.0).sum())
        eh = hess[rng.choice(inner, 6)] * rng.uniform(0.8, 1.22, (6, 1))     # the response scales with the square: 0.64 .. 1.5
        order = rng.permutation(len(xy) + 6)
        got = api.assemble_checkerboard(np.concatenate([xy, extra])[order], np.concatenate([hess, eh])[order], PATTERN, ref.BOARD_SQUARE)
        assert got == base, seed
    assert inside >= 40, "the strays do fall among the board's corners"
    perm = np.random.default_rng(40 + k).permutation(len(xy))
    assert api.assemble_checkerboard(xy[perm], hess[perm], PATTERN, ref.BOARD_SQUARE) == base


def test_square_pattern_takes_the_rotation_with_id0_first():
    """5 x 5 corners cut out of the 7 x 5 board: four admissible rotations, id 0 is the lattice corner smallest in (y, x), and the
    labelling is right-handed."""
    for k in range(3):
        xy, hess = _candidates(k)
        truth = ref.board_frames()[1][k].reshape(ref.BOARD_ROWS, ref.BOARD_COLS, 2)[:, 1:6].reshape(-1, 2)
        keep = _inner(xy, truth)
        out = api.assemble_checkerboard(xy[keep], hess[keep], (5, 5), ref.BOARD_SQUARE)
        assert out is not None and sorted(out) == list(range(25))
        g = np.array([out[i] for i in range(25)]).reshape(5, 5, 2)
        corners = [tuple(g[0, 0][::-1]), tuple(g[0, 4][::-1]), tuple(g[4, 0][::-1]), tuple(g[4, 4][::-1])]
        assert min(corners) == corners[0]
        e_c, e_r = g[0, 1] - g[0, 0], g[1, 0] - g[0, 0]
        assert e_c[0] * e_r[1] - e_c[1] * e_r[0] > 0.0
        t = truth.reshape(5, 5, 2)
        same = [np.rot90(t, q) for q in range(4)]                        # rot90 acts on the two leading axes
        assert min(float(np.linalg.norm(g - s, axis=2).max()) for s in same) <= ref.BOARD_BOUND


# ---- 4. argument rules that need no device --------------------------------------------------------------------------------------
def test_argument_rules_without_a_device():
    """What can be rejected without a device: a NULL context (CCAL_ERR_INVALID_ARG from both entry points, whatever else is
    passed) and the argument checks of api.detect_checkerboard / assemble_checkerboard, which raise before they reach the library.
    The parameter ranges are checked behind a valid context, and a context needs a device: tests/test_gpu_detect.py holds them."""
    lib = _ffi.load()
    cnt = np.zeros(1, dtype=np.int32)
    for fn in (lib.ccal_detect_corners_batch, lib.ccal_detect_corners_dev):
        assert fn(None, 0, 8, 8, 0, None, 1, 5, 1, 102, 16, None, None, None, None) == _ffi.ERR_INVALID_ARG
        assert fn(None, 0, 8, 8, 1, None, 1, 5, 1, 102, 16, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None,
                  None) == _ffi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        api.detect_checkerboard([np.zeros((20, 20), np.uint8), np.zeros((20, 21), np.uint8)], PATTERN, 0.03)      # two sizes
    with pytest.raises(ValueError):
        api.detect_checkerboard([np.zeros((20, 20, 3), np.uint8)], PATTERN, 0.03)                                 # colour
    with pytest.raises(ValueError):
        api.detect_checkerboard([np.zeros((20, 20), np.float32)], PATTERN, 0.03)                                  # not u8 / u16
    assert api.detect_checkerboard([], PATTERN, 0.03) == []
    with pytest.raises(ValueError):
        api.assemble_checkerboard(np.zeros((3, 2)), np.zeros((2, 3)), PATTERN, 0.03)
    with pytest.raises(ValueError):
        api.assemble_checkerboard(np.zeros((3, 2)), np.zeros((3, 3)), (1, 5), 0.03)
