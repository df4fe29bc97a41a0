"""CPU: the host side of the calibration from detections alone - find_best_two_frames_idx (src/util.rs:168-219),
homography_to_focal (src/optimization/homography.rs:274-325, host code of the library), the sampler twin of the RANSAC kernel,
CalibParams (src/types.rs:6-10) - and the numpy yardstick tests/rdh_ref.py on exact division-model pairs."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rdh_ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth  # noqa: E402


def _frame(points, w=512, h=512):
    return api.FrameFeature(0, (w, h), {i: api.FeaturePoint((float(u), float(v)), (0.0, 0.0, 0.0)) for i, (u, v) in enumerate(points)})


def _box(cx, cy, half, n=4):
    """n points, the first four the corners of a square: bounding box (2 half)^2, centroid (cx, cy)."""
    pts = [(cx - half, cy - half), (cx + half, cy - half), (cx - half, cy + half), (cx + half, cy + half)]
    return pts + [(cx, cy)] * (n - 4)


def test_new_names_are_importable():
    for name in ("CalibParams", "find_best_two_frames_idx", "radial_distortion_homography", "homography_to_focal", "init_pose",
                 "rdh_sample_indices"):
        assert callable(getattr(api, name)), name
    lib = _ffi.load()
    for name in ("ccal_rdh_batch", "ccal_radial_distortion_homography", "ccal_homography_to_focal", "ccal_init_poses_division"):
        assert hasattr(lib, name)
    assert b"0.3.0" in lib.ccal_version()


def test_best_two_frames_area_first_centroid_second():
    frames = [
        _frame(_box(250, 250, 40, 6)),        # 0
        None,
        _frame(_box(256, 256, 120, 6)),       # 2: largest bounding box
        _frame(_box(60, 70, 30, 6)),          # 3: centroid farthest from the mean centroid
        _frame(_box(256, 256, 250, 5)),       # 4: larger still, but fewer corners: not a candidate
        _frame(_box(300, 240, 50, 6)),        # 5
    ]
    assert api.find_best_two_frames_idx(frames, False) == (2, 3)


def test_best_two_frames_only_maximal_corner_count_and_ties():
    frames = [_frame(_box(100, 100, 200, 4)), _frame(_box(200, 200, 10, 8)), None, _frame(_box(300, 300, 10, 8))]
    # candidates 1 and 3: equal areas and equal distances from the mean centroid -> the later one, twice
    assert api.find_best_two_frames_idx(frames, False) == (3, 3)
    frames.append(_frame(_box(310, 300, 11, 8)))
    assert api.find_best_two_frames_idx(frames, False) == (4, 1)


def test_best_two_frames_random_pick_is_reproducible():
    frames = [_frame(_box(50 + 10 * i, 60, 20, 6)) for i in range(12)] + [None, _frame(_box(10, 10, 5, 5))]
    a = api.find_best_two_frames_idx(frames, True, seed=5)
    assert a == api.find_best_two_frames_idx(frames, True, seed=5)
    assert a[0] != a[1] and all(0 <= i < 12 for i in a)
    picks = {api.find_best_two_frames_idx(frames, True, seed=s) for s in range(20)}
    assert len(picks) > 5


def _focal_model(f, R, t):
    """H of a plane z = 0 seen by a pinhole of focal f: K [r1 r2 t]."""
    K = np.diag([f, f, 1.0])
    return K @ np.stack([R[:, 0], R[:, 1], t], axis=1)


def test_homography_to_focal_recovers_a_pinhole_focal():
    R = synth.rodrigues(np.array([0.3, -0.4, 0.2]))
    H = _focal_model(0.8, R, np.array([0.1, -0.2, 1.5]))
    f = api.homography_to_focal(H)
    assert f is not None and abs(f - 0.8) < 1e-9
    assert abs(api.homography_to_focal(3.7 * H) - 0.8) < 1e-9             # scale of H does not matter


def test_homography_to_focal_branches():
    # (f0, f1) = (None, None): the identity - 0/0 everywhere
    assert api.homography_to_focal(np.eye(3)) is None
    # both candidates of both estimates negative
    assert api.homography_to_focal([[1, 0.5, 0.3], [0.5, -1, 0.3], [0.2, 0.1, 1]]) is None
    # the estimate from the first two rows alone (the third row's candidates are both negative: -2 / 0.5 and -2 / 0.75),
    # one positive candidate: d1 = 1, d2 = 1 - 1 - 4 = -4, v1 = 6 / 1, v2 = (9 - 4) / -4
    H = np.array([[1.0, 0.0, 2.0], [1.0, 2.0, -3.0], [0.5, 1.0, 1.0]])
    assert abs(api.homography_to_focal(H) - np.sqrt(6.0)) < 1e-12
    # both candidates positive: the larger when |d1| > |d2|, else the smaller
    H = np.array([[2.0, 0.0, 1.0], [1.0, 1.0, -2.0], [1.0, 0.5, 1.0]])
    #   d1 = 2, d2 = 4 - 1 - 1 = 2 -> not greater: the smaller of v1 = 2 / 2, v2 = 3 / 2
    assert abs(api.homography_to_focal(H) - 1.0) < 1e-12
    H = np.array([[2.0, 0.0, 1.0], [1.5, 1.0, -2.0], [1.0, 0.5, 1.0]])
    #   d1 = 3, d2 = 4 - 2.25 - 1 = 0.75 -> the larger of v1 = 2 / 3, v2 = 3 / 0.75
    assert abs(api.homography_to_focal(H) - 2.0) < 1e-12
    # a zero third row divides by zero: +inf is a positive candidate, as in the reference's arithmetic
    assert api.homography_to_focal([[1.0, 0.0, 2.0], [1.0, 1.0, -3.0], [0.0, 0.0, 1.0]]) == np.inf
    # neither: third row v1 = 0, v2 = -4; first two rows 0/0 and -0
    H = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.5, -1.0, 1.0]])
    assert api.homography_to_focal(H) is None
    # the estimate from the third row alone
    H = np.array([[1.0, 1.0, 0.0], [0.0, 2.0, 0.0], [0.5, -1.0, 1.0]])
    #   third row: v1 = -(1) / -0.5 = 2, v2 = (1 - 1 - 4) / 0.75 < 0 -> sqrt(2); first two rows: -0 / 2 = -0 and 0 / -2: none
    assert abs(api.homography_to_focal(H) - np.sqrt(2.0)) < 1e-12
    # both estimates: geometric mean
    H = np.array([[1.0, 1.0, 2.0], [1.0, 2.0, -3.0], [0.5, -1.0, 1.0]])
    fa = np.sqrt(6.0 / 3.0)                                                # v1 = 6 / 3, v2 = 5 / (2 - 5) < 0
    fb = np.sqrt(6.0)                                                      # v1 = -(1 + 2) / -0.5 = 6, v2 = (2 - 5) / 0.75 < 0
    assert abs(api.homography_to_focal(H) - np.sqrt(fa * fb)) < 1e-12


def test_sample_indices():
    s = api.rdh_sample_indices(42, 144, 1000)
    assert s.shape == (1000, 6) and s.min() >= 0 and s.max() < 144
    srt = np.sort(s, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                               # six distinct indices
    assert np.array_equal(s, api.rdh_sample_indices(42, 144, 1000))
    assert not np.array_equal(s, api.rdh_sample_indices(43, 144, 1000))
    assert len(np.unique(s)) == 144                                        # every pair is drawn
    assert np.array_equal(s[:10], api.rdh_sample_indices(42, 144, 10))     # hypothesis h does not depend on n_hyp
    assert sorted(api.rdh_sample_indices(1, 6, 3)[2].tolist()) == list(range(6))
    with pytest.raises(ValueError):
        api.rdh_sample_indices(1, 5, 3)


def test_calib_params_plumbing(tmp_path):
    p = api.CalibParams()
    assert (p.fixed_focal, p.disabled_distortion_num, p.one_focal) == (None, 0, False)
    q = api.CalibParams(fixed_focal=190.5, disabled_distortion_num=2, one_focal=True)
    path = tmp_path / "params.json"
    path.write_text(json.dumps(q.to_json_obj()))
    assert api.CalibParams.from_json_obj(json.loads(path.read_text())) == q
    assert api.CalibParams.from_json_obj({}) == p
    m = api.GenericModel("kb4", [1.0] * 8, 0, 0)
    m.set_w_h(640, 480)
    assert (m.width(), m.height()) == (640.0, 480.0)


@pytest.mark.parametrize("lam", [-0.05, -0.3, -0.6])
def test_yardstick_recovers_exact_pairs(lam):
    H = np.array([[0.9, 0.1, 0.05], [-0.08, 1.05, -0.03], [0.1, -0.05, 1.0]])
    pairs = rdh_ref.exact_pairs(lam, H, 144, seed=1)
    samples = api.rdh_sample_indices(7, 144, 100)
    for route in ("svd", "qr"):
        lams, Hs, sc, best = rdh_ref.ransac(pairs, samples, route)
        assert (sc < 1e-9).all()
        assert abs(lams[best] - lam) <= 1e-9 * abs(lam)
        assert np.abs(Hs[best] / Hs[best][8] - H.ravel()).max() < 1e-9
