"""CPU: the undistortion yardstick (tests/undistort_ref.py) agrees with itself, the inputs the GPU tests draw meet the boundary
caps of the issue on the yardstick alone, and the API refuses bad arguments before any GPU call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth  # noqa: E402
from camera_intrinsic_calibration_rs_amd.engine import CcalError  # noqa: E402

MODELS = ["ucm", "eucm", "kb4", "opencv5"]
W = H = 512


def _model(name):
    return api.GenericModel(name, synth.GT_PARAMS[synth.MODEL_NAMES[name]], W, H)


# ---- the yardstick agrees with itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ch", [(np.uint8, 1), (np.uint8, 3), (np.uint16, 1)])
def test_identity_map_gives_the_identical_image(dtype, ch):
    rng = np.random.default_rng(1)
    shape = (48, 64) if ch == 1 else (48, 64, ch)
    img = rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    xs, ys = np.meshgrid(np.arange(64, dtype=np.float32), np.arange(48, dtype=np.float32))
    out, valid = ref.remap(img, xs, ys)
    assert valid.all() and out.dtype == img.dtype and np.array_equal(out, img)


def test_known_weights_on_a_2x2_image():
    img = np.array([[10, 20], [30, 50]], dtype=np.uint8)
    xmap = np.array([[0.5, 0.25, 1.0, 0.0, 0.5]], dtype=np.float32)
    ymap = np.array([[0.5, 0.0, 0.75, 1.0, 1.0]], dtype=np.float32)
    out, valid = ref.remap(img, xmap, ymap)
    # (10 + 20 + 30 + 50) / 4 = 27.5 -> 28 (ties round up); 12.5 -> 13; 20 + 0.75 * 30 = 42.5 -> 43; 30; 40
    assert valid.all() and out.tolist() == [[28, 13, 43, 30, 40]]


def test_invalid_entries_give_zero():
    img = np.full((4, 5), 200, dtype=np.uint16)
    xmap = np.array([[-1e-3, 4.001, np.nan, np.inf, -np.inf, -0.0, 4.0, 2.0]], dtype=np.float32)
    ymap = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, -0.0, 3.0, 3.001]], dtype=np.float32)
    out, valid = ref.remap(img, xmap, ymap)
    assert valid.tolist() == [[False, False, False, False, False, True, True, False]]
    assert out.tolist() == [[0, 0, 0, 0, 0, 200, 200, 0]]


def test_new_camera_matrix_formula():
    rays = np.array([[0.0, -0.5, 1.0], [2.0, 0.0, 2.0], [0.0, 1.5, 1.0], [-0.25, 0.0, 1.0]])
    K = ref.new_camera_matrix(rays, 0.25, 100, 80)
    # x/z in [-0.25, 1], y/z in [-0.5, 1.5]: ratios 100 / 1.25 = 80 and 80 / 2 = 40
    assert np.allclose(K, [[0.25 * 80 + 0.75 * 40, 0, 100 * 0.25 / 1.25], [0, 50.0, 80 * 0.5 / 2.0], [0, 0, 1]], rtol=1e-15)
    rays[2, 2] = -1.0
    assert ref.new_camera_matrix(rays, 0.25, 100, 80) is None


def test_map_rays_rotate_by_the_transpose():
    K = np.array([[100.0, 0, 10.0], [0, 50.0, 5.0], [0, 0, 1]])
    a = np.deg2rad(90.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rays = ref.map_rays(K, R, 21, 11).reshape(11, 21, 3)
    assert np.allclose(rays[5, 10], R.T @ [0.0, 0.0, 1.0]) and np.allclose(rays[0, 20], R.T @ [0.1, -0.1, 1.0])


@pytest.mark.parametrize("name", MODELS)
def test_newton_unprojection_round_trips(oracle, name):
    m = synth.MODEL_NAMES[name]
    p = synth.GT_PARAMS[m]
    uv = ref.edge_midpoints(p, W, H)
    rays = ref.unproject_newton(oracle, m, p, uv)
    assert (rays[:, 2] > 0).all() and np.abs(oracle.project(m, p, rays) - uv).max() < 1e-9


# ---- the GPU tests' inputs meet the issue's caps on the yardstick alone -----------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_seeded_inputs_meet_the_boundary_caps(name):
    m = synth.MODEL_NAMES[name]
    p = synth.GT_PARAMS[m]
    for n in (1, 63, 64, 65, 1000):
        valid, near = ref.project_valid(m, p, ref.seeded_rays(m, n))
        assert near.sum() <= 0.001 * n
        if n == 1000:
            assert valid.any() and (name == "kb4" or (~valid).any())
        if m in (ref.UCM, ref.EUCM):
            valid, near = ref.unproject_domain(m, p, ref.seeded_pixels(p, n, W, H))
            assert near.sum() <= 0.001 * n
            if n == 1000:
                assert valid.any() and (~valid).any()


def test_raised_alpha_puts_an_edge_midpoint_outside_the_domain():
    p = list(synth.GT_PARAMS[synth.MODEL_EUCM])
    assert ref.unproject_domain(ref.EUCM, p, ref.edge_midpoints(p, W, H))[0].all()
    p[4] = 0.8
    valid, near = ref.unproject_domain(ref.EUCM, p, ref.edge_midpoints(p, W, H))
    assert not valid[1] and not near.any()


# ---- argument errors are raised before any GPU call (no context exists on this machine) ---------------------------------------------
@pytest.fixture()
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a GPU context was requested")
    monkeypatch.setattr(api, "_ctx", boom)


@pytest.mark.parametrize("balance", [-0.1, 1.5, float("nan")])
def test_bad_balance(no_gpu, balance):
    with pytest.raises(ValueError):
        _model("eucm").estimate_new_camera_matrix_for_undistort(balance)


def test_container_model_is_unsupported(no_gpu):
    m = api.GenericModel("eucmt", [190.0, 190.0, 255.0, 257.0, 0.6, 1.0, 0.0, 0.0], W, H)
    calls = [lambda: m.project(np.zeros((2, 3))), lambda: m.unproject(np.zeros((2, 2))),
             lambda: m.estimate_new_camera_matrix_for_undistort(0.5), lambda: m.init_undistort_map(np.eye(3), (8, 8))]
    for call in calls:
        with pytest.raises(CcalError) as e:
            call()
        assert e.value.code == _ffi.ERR_UNSUPPORTED


def test_shape_and_dtype_mismatches(no_gpu):
    m = _model("kb4")
    f32 = lambda *s: np.zeros(s, dtype=np.float32)
    bad = [lambda: m.project(np.zeros((4, 2))), lambda: m.unproject(np.zeros((4, 3))), lambda: m.unproject(np.zeros(4)),
           lambda: m.init_undistort_map(np.eye(4), (8, 8)), lambda: m.init_undistort_map(np.eye(3), (8, 0)),
           lambda: m.init_undistort_map(np.eye(3), (8, 8), rotation=np.eye(2)),
           lambda: m.estimate_new_camera_matrix_for_undistort(0.5, (0, 10)),
           lambda: api.remap(np.zeros((4, 4), np.uint8), f32(3, 3), f32(3, 4)),               # maps of two shapes
           lambda: api.remap(np.zeros((4, 4), np.uint8), np.zeros((3, 3)), np.zeros((3, 3))),    # f64 maps
           lambda: api.remap(np.zeros((4, 4), np.float32), f32(3, 3), f32(3, 3)),             # float image
           lambda: api.remap(np.zeros((4, 4, 3), np.uint16), f32(3, 3), f32(3, 3)),           # u16 x 3
           lambda: api.remap(np.zeros((4, 4, 2), np.uint8), f32(3, 3), f32(3, 3)),            # two channels
           lambda: api.remap(np.zeros((2, 4, 4, 3), np.uint8), f32(3, 3), f32(3, 3)),         # a batch
           lambda: api.remap(np.zeros(4, np.uint8), f32(3, 3), f32(3, 3))]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")
