"""CPU: the renderer's yardstick (tests/render_ref.py) reproduces the fixtures the detectors were built on, every case of the GPU
parity tests meets the near cap on the yardstick alone, the recorded round-trip errors are what the numpy chains measure, and the
API refuses bad arguments before any GPU call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref  # noqa: E402
import render_ref as rr  # noqa: E402
import tag_ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, engine, synth  # noqa: E402
from camera_intrinsic_calibration_rs_amd.engine import CcalError  # noqa: E402

CASES = {c["name"]: c for c in rr.parity_cases()}


def _pinhole(f, w, h):
    """OPENCV5 without distortion: the division camera of the fixtures at lam = 0."""
    return [f, f, (w - 1) / 2.0, (h - 1) / 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]


# ---- the rule is the fixtures' ------------------------------------------------------------------------------------------------------
def test_reproduces_render_board(oracle):
    lam, rot, tilt, axis, centre = detect_ref.BOARD_FRAMES[0]
    assert lam == 0.0
    c, r, sq = detect_ref.BOARD_COLS, detect_ref.BOARD_ROWS, detect_ref.BOARD_SQUARE
    W, H = detect_ref.BOARD_W, detect_ref.BOARD_H
    pose = rr.pose6(*detect_ref.board_pose(c, r, sq, rot, tilt, axis, centre))
    for dtype in (np.uint8, np.uint16):
        img, counts, near = rr.render(oracle, rr.OPENCV5, _pinhole(detect_ref.BOARD_F, W, H), W, H, pose, rr.board_target(c, r, sq, margin=np.inf),
                                      dtype, near=dtype == np.uint8)
        assert (counts[..., 2] == 0).all()                       # a white plane: no background
        want = detect_ref.board_frames(dtype)[0][0]
        if near is None:
            assert (img != want).mean() <= rr.NEAR_CAP
        else:
            assert (near > 0).mean() <= rr.NEAR_CAP and np.array_equal(img[near == 0], want[near == 0])


@pytest.mark.parametrize("k", [0, 3])
def test_reproduces_render_aprilgrid(oracle, k):
    lam, rot, tilt, axis = tag_ref.GRID_FRAMES[k]
    assert lam == 0.0
    W, H = tag_ref.GRID_W, tag_ref.GRID_H
    pose = rr.pose6(*tag_ref.grid_pose(tag_ref.GRID, rot, tilt, axis, (0.002, -0.003, 0.40)))
    img, _, near = rr.render(oracle, rr.OPENCV5, _pinhole(tag_ref.GRID_F, W, H), W, H, pose,
                             rr.grid_target(tag_ref.GRID, tag_ref.grid_family(), tag_ref.GRID_BORDER, margin=np.inf))
    want = tag_ref.grid_frames()[0][k]
    assert (near > 0).mean() <= rr.NEAR_CAP and np.array_equal(img[near == 0], want[near == 0])


def test_pose_rt_is_rodrigues():
    rng = np.random.default_rng(5)
    for pose in list(rng.normal(size=(8, 6))) + [np.array([0.0, 0.0, 0.0, 1.0, 2.0, 3.0]), np.array([np.pi, 0.0, 0.0, 0.0, 0.0, 1.0])]:
        R, tb = rr.pose_rt(pose)
        assert np.abs(R - synth.rodrigues(pose[:3])).max() < 1e-15 and np.abs(tb - R.T @ pose[3:]).max() < 1e-15
        assert np.abs(rr.pose_rt(rr.pose6(R, pose[3:]))[0] - R).max() < 1e-14


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_near_cap(oracle, name):
    case = CASES[name]
    img, near = rr.yardstick(oracle, case)
    assert img.shape == (len(case["poses"]), case["height"], case["width"]) and img.dtype == case["dtype"]
    # one near pixel is always allowed: 0.1 % of the one-pixel image is less than a pixel
    assert (near > 0).sum() <= max(rr.NEAR_CAP * near.size, 0 if near.size > 1 else 1), (name, int((near > 0).sum()), near.size)


def test_the_cases_show_what_they_are_for(oracle):
    """The content the cases are named after is in the yardstick's images: background where the domain ends, where the board is off
    screen and beyond the plane's horizon; the mirror image from behind; all three classes in one pixel."""
    img, _ = rr.yardstick(oracle, CASES["board ucm domain"])
    assert img[0, 0, 0] == 77 and img[0, -1, -1] == 77 and img[0, 22, 33] != 77          # the corners have no ray
    img, _ = rr.yardstick(oracle, CASES["grid eucm domain"])
    assert img[0, 0, 0] == 77 and img[0, -1, 0] == 77 and (img[0] != 77).mean() > 0.5
    assert (rr.yardstick(oracle, CASES["board eucm off screen"])[0] == 9).all()
    hz, _ = rr.yardstick(oracle, CASES["board kb4 horizon"])
    assert (hz[0] == 0).mean() > 0.2 and (hz[0] == 215).mean() > 0.2                       # beyond the horizon, and the white plane
    one, _ = rr.yardstick(oracle, CASES["board kb4 1 x 1"])
    assert 40 * 257 < one[0, 0, 0] < 215 * 257                                               # black and white squares in the one pixel
    for name in ("board ucm", "grid ucm", "board opencv5", "grid kb4"):
        img, _ = rr.yardstick(oracle, CASES[name])
        assert all((im == 0).any() and (im > 0).mean() > 0.05 for im in img), name          # sheet and background in every image
        assert not np.array_equal(img[0], img[2])


# ---- the recorded round-trip errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [rr.UCM, rr.EUCM])
def test_recorded_round_trip_errors(oracle, m):
    """The two closed-form lenses are measured again here (a second or so per frame); the Newton-based yardstick of KB4 and OPENCV5
    takes a quarter of a minute per 512 x 512 frame: `python tests/render_ref.py` measures all four."""
    for worst, recorded in ((rr.measure_board(oracle, m), rr.RT_BOARD_WORST[m]), (rr.measure_grid(oracle, m), rr.RT_GRID_WORST[m])):
        assert recorded - 1e-5 <= worst <= recorded, (worst, recorded)


def test_round_trip_poses_are_listed_for_every_model():
    for m in (rr.UCM, rr.EUCM, rr.KB4, rr.OPENCV5):
        assert 2 <= len(rr.RT_BOARD_POSES[m]) <= 3 and 2 <= len(rr.RT_GRID_POSES[m]) <= 3
        assert rr.RT_BOARD_WORST[m] > 0 and rr.RT_GRID_WORST[m] > 0 and rr.rt_bound(rr.RT_BOARD_WORST[m]) == 1.5 * rr.RT_BOARD_WORST[m]
        assert rr.rt_board_poses(m).shape == (len(rr.RT_BOARD_POSES[m]), 6)


# ---- argument checks that need no device ----------------------------------------------------------------------------------------------
def test_api_refuses_bad_arguments_without_a_device():
    model = api.GenericModel("eucm", synth.GT_PARAMS[synth.MODEL_EUCM], 512, 512)
    fam = api.TagFamily("seeded", rr.family().bits, rr.family().codes)
    board = api.AprilGridBoard(0.03, 0.3, 2, 3)
    pose = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.3]])
    container = api.GenericModel("eucmt", [1.0] * 8, 512, 512)
    for call in (lambda: api.render_checkerboard(container, pose, (7, 5), 0.03), lambda: api.render_aprilgrid(container, pose, board, fam)):
        with pytest.raises(CcalError) as e:
            call()
        assert e.value.code == _ffi.ERR_UNSUPPORTED
    for bad in (np.zeros((2, 5)), np.zeros(6), [[0.0] * 7]):
        with pytest.raises(ValueError, match="poses"):
            api.render_checkerboard(model, bad, (7, 5), 0.03)
        with pytest.raises(ValueError, match="poses"):
            api.render_aprilgrid(model, bad, board, fam)
    with pytest.raises(ValueError, match="dtype"):
        api.render_checkerboard(model, pose, (7, 5), 0.03, dtype=np.float32)
    with pytest.raises(ValueError, match="width and height"):
        api.render_checkerboard(api.GenericModel("eucm", synth.GT_PARAMS[synth.MODEL_EUCM], 512.5, 512), pose, (7, 5), 0.03)


def test_defaults_and_the_null_context():
    lib = _ffi.load()
    t = engine.checkerboard_target(7, 5, 0.03)
    o = engine.render_opts(t)
    assert (o.supersample, o.black, o.white, o.background, o.margin) == (4, 40.0, 215.0, 0.0, 0.03)
    g = engine.aprilgrid_target(0.03, 0.3, 2, 3, 0, 36, rr.family().codes)
    assert engine.render_opts(g).margin == 0.03 * (1.0 + 0.3) and g.n_codes == len(rr.family().codes)
    o = engine.render_opts(t, supersample=2, margin=float("inf"), background=7)
    assert (o.supersample, o.margin, o.background, o.black) == (2, float("inf"), 7.0, 40.0)
    assert lib.ccal_render_set_defaults(None, C.byref(o)) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_render_set_defaults(C.byref(t), None) == _ffi.ERR_INVALID_ARG
    for fn in (lib.ccal_render_targets_batch, lib.ccal_render_targets_dev):
        assert fn(None, 0, None, 0, 8, 8, 0, None, C.byref(t), C.byref(o), None) == _ffi.ERR_INVALID_ARG
