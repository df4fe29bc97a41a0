"""CPU: the yardstick of the sub-pixel corner refinement (tests/corner_ref.py, the rule of include/ccal.h at
ccal_refine_corners_batch) against the TRUTH of rendered saddles, its status rules, the decision margins the GPU tests rely on, and
the argument checks of api.refine_corners / api.redetect_corners that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import api  # noqa: E402
from camera_intrinsic_calibration_rs_amd.api import redetect_corners, refine_corners  # noqa: E402  (absent: the feature is not there)

HALF_WINS = sorted(ref.TRUTH_SEEDS)


@pytest.fixture(scope="module")
def truth_runs():
    """Per half_win: (true centres, the yardstick's result) on the committed seed - computed once, shared, left unchanged."""
    out = {}
    for h in HALF_WINS:
        img, centres, starts = ref.grid_fixture(ref.TRUTH_SEEDS[h])
        out[h] = (centres, ref.refine(img, starts, h, 30, 1e-3))
    return out


# ---- (a) truth --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", HALF_WINS)
def test_yardstick_converges_to_the_true_saddle(truth_runs, h):
    """25 tanh-profile saddles (sigma 1.2 px, amplitude 90 of 255, u8), starts up to 1.5 px off.  Measured worst error, px:
    h = 2: 0.07212, 3: 0.04133, 5: 0.03025, 7: 0.02663 (corner_ref.TRUTH_WORST); the bound is 1.5 x that."""
    centres, r = truth_runs[h]
    assert (r["status"] == ref.OK).all(), r["status"]
    err = np.hypot(*(r["xy"] - centres).T)
    print(f"h = {h}: worst error {err.max():.5f} px, iterations {r['iters'].min()} .. {r['iters'].max()}, bound {ref.TRUTH_BOUND[h]:.5f}")
    assert err.max() <= ref.TRUTH_BOUND[h]
    assert h < 3 or ref.TRUTH_WORST[h] < 0.1          # a restatement that misses this is wrong: the bound is not to be raised
    assert np.isfinite(r["lam"]).all() and (r["lam"] > 0).all()


# ---- (b) status rules -------------------------------------------------------------------------------------------------------------
def _one(img, x, y, h, max_it=30, eps=1e-3):
    r = ref.refine(img, [[x, y]], h, max_it, eps)
    return int(r["status"][0]), r["xy"][0], int(r["iters"][0]), float(r["lam"][0])


def test_flat_and_single_edge_are_not_pd():
    flat = np.full((45, 67), 77, dtype=np.uint8)
    edge = np.zeros((45, 67), dtype=np.uint8)
    edge[:, 30:] = 200                                  # an exactly vertical step
    for img in (flat, edge):
        for x, y in ((30.0, 20.0), (29.7, 20.3)):       # pixel centres and fractions: the difference form keeps both exact
            st, xy, it, lam = _one(img, x, y, 3)
            assert st == ref.NOT_PD and it == 0 and tuple(xy) == (x, y)
            assert lam == 0.0


def test_inside_rule_is_exact_at_the_border():
    img, centres, _ = ref.grid_fixture(ref.TRUTH_SEEDS[3])
    H, W = img.shape
    h = 3
    for x, y in ((h + 1.0, 40.0), (40.0, h + 1.0), (W - 2.0 - h, 40.0), (40.0, H - 2.0 - h)):
        st, _, _, lam = _one(img, x, y, h, max_it=1, eps=0.0)
        assert st != ref.NO_RESULT or not np.isnan(lam)             # the start was evaluated: it is inside
        assert not np.isnan(lam)
    for x, y in ((np.nextafter(h + 1.0, 0.0), 40.0), (40.0, np.nextafter(h + 1.0, 0.0)),
                 (np.nextafter(W - 2.0 - h, np.inf), 40.0), (40.0, np.nextafter(H - 2.0 - h, np.inf)),
                 (np.nan, 40.0), (40.0, np.nan), (np.inf, 40.0), (40.0, -np.inf)):
        st, xy, it, lam = _one(img, x, y, h)
        assert st == ref.NO_RESULT and it == 0 and np.isnan(lam)
        assert np.array_equal(xy, [x, y], equal_nan=True)           # the position as given


def test_far_starts_end_in_the_drift_rule():
    img, centres, starts = ref.drift_fixture()
    r = ref.refine(img, starts, 2, 30, 1e-3)
    drifted = (r["status"] == ref.NO_RESULT) & (r["iters"] > 0)
    print(f"h = 2, starts 2.5 px off: {drifted.sum()} of {len(starts)} end in the drift rule, statuses {np.bincount(r['status'])}")
    assert drifted.sum() >= 1
    assert np.array_equal(r["xy"][drifted], starts[drifted])       # the position as given
    assert np.isfinite(r["lam"][drifted]).all()                     # an iterate was evaluated


# ---- (c) margins ------------------------------------------------------------------------------------------------------------------
def test_fixture_seeds_leave_every_decision_a_margin():
    """What tests/test_gpu_corners.py relies on: no corner of its cases decides within 1e-7 of a threshold, so none has to be left
    out (the GPU test's cap is 2 %; here it is 0 % on the yardstick alone), and every lambda_min it compares is either exact or
    well conditioned (corner_ref.lambda_well_conditioned: the 1e-9 relative bound cannot hold for a rank-deficient patch whose det
    is rounding noise, whatever the kernel does)."""
    runs = [(name, img, xy, h) for name, (img, xy, h) in ref.parity_cases().items()]
    for dtype in (np.uint8, np.uint16):
        imgs, xy_list = ref.batch_fixture(dtype=dtype)
        runs += [(f"batch {np.dtype(dtype).name} {k}", imgs[k], xy_list[k], ref.BATCH_HALF_WIN) for k in range(len(imgs))]
    img, _, starts = ref.drift_fixture()
    runs.append(("drift", img, starts, 2))
    for name, img, xy, h in runs:
        for it, eps in ((30, 1e-3), (8, 0.0)):
            r = ref.refine(img, xy, h, it, eps)
            if eps > 0.0:
                near = (r["margin_e"] <= 1e-7) | (r["margin_det"] <= 1e-7)
                assert not near.any(), (name, r["margin_e"].min(), r["margin_det"].min())
            bad = ~ref.lambda_well_conditioned(r)
            assert not bad.any(), (name, it, np.flatnonzero(bad), r["ratio"][bad])


# ---- (d) argument checks that need no device -----------------------------------------------------------------------------------
def _frame(pts):
    return api.FrameFeature(5, (67, 45), {k: api.FeaturePoint(p, (0.1 * k, 0.0, 0.0)) for k, p in enumerate(pts)})


def test_refine_corners_argument_checks():
    img = np.zeros((45, 67), dtype=np.uint8)
    f = _frame([(30.0, 20.0)])
    with pytest.raises(ValueError):
        refine_corners([img, img], [f])                                         # frames / images length mismatch
    assert refine_corners([None, None], [None, None]) == [None, None]           # None frames pass through, no image is read
    assert refine_corners([], []) == []
    for kw in ({"half_win": 0}, {"half_win": 16}, {"max_iterations": 0}, {"eps": -1.0}, {"eps": np.nan}, {"eps": np.inf},
               {"min_lambda": np.nan}):
        with pytest.raises(ValueError):
            refine_corners([img], [f], **kw)
    for bad in (np.zeros((45, 67), dtype=np.float32), np.zeros((45, 67, 3), dtype=np.uint8), np.zeros(67, dtype=np.uint8)):
        with pytest.raises(ValueError):
            refine_corners([bad], [f])
    with pytest.raises(ValueError):
        refine_corners([img, np.zeros((46, 67), dtype=np.uint8)], [f, f])       # two sizes
    with pytest.raises(ValueError):
        refine_corners([img, np.zeros((45, 67), dtype=np.uint16)], [f, f])      # two types


def test_redetect_corners_argument_checks():
    img = np.zeros((45, 67), dtype=np.uint8)
    model = api.GenericModel("eucm", [200.0, 200.0, 33.0, 22.0, 0.6, 1.1], 67, 45)
    pose = api.RvecTvec((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    board = {0: (0.0, 0.0, 0.0)}
    assert redetect_corners([img, img], model, {}, board) == [None, None]       # no pose: nothing to do, no device
    assert redetect_corners([img], model, {0: pose}, {}) == [None]              # no board points
    with pytest.raises(ValueError):
        redetect_corners([img], model, {1: pose}, board)                        # a pose for a frame without an image
    with pytest.raises(ValueError):
        redetect_corners([img], model, {0: pose}, board, half_win=0)
    with pytest.raises(ValueError):
        redetect_corners([np.zeros((45, 67), dtype=np.float64)], model, {0: pose}, board)
    with pytest.raises(api.CcalError):
        redetect_corners([img], api.GenericModel("eucmt", [1.0] * 8, 67, 45), {0: pose}, board)
