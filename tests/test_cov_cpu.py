"""CPU: the definition of ccal_covariance (include/ccal.h, "calibration uncertainty") on the numpy yardsticks of tests/cov_ref.py -
the dense inverse, the Schur route the device takes and the mpmath truth agree; the leverages sum to the number of free parameters;
fixed parameters; the definition against 200 noise draws solved by the oracle; the pivot rule; the Python mirrors' argument checks."""
import functools

import numpy as np
import pytest

import cov_ref as cr
from camera_intrinsic_calibration_rs_amd import api, synth
from camera_intrinsic_calibration_rs_amd.engine import Problem

EPS = 2.0 ** -52
MODELS = ["ucm", "eucm", "kb4", "opencv5"]


@functools.lru_cache(maxsize=None)
def _case(name, one_focal=False):
    from oracle import binding as ob
    sp = synth.make_problem(4, "eucm", n_cams=2, seed=9) if name == "rig2" else cr.small_case(name, one_focal)
    op = ob.OracleProblem.from_synth(sp)
    ci = cr.CovInputs(op, *cr.solved_point(op, sp))
    return sp, ci, cr.dense(ci), cr.schur(ci)


def _bound(ci):
    """What two f64 routes to the same inverse may differ by, entry by entry relative to sqrt(C_ii C_jj): a Cholesky-based inverse of a
    matrix of n unknowns carries a relative error of the order n eps kappa, kappa the condition number after Jacobi scaling (the
    measure is invariant under that scaling); a factor 8 for the constants of the products around it."""
    kappa, n = cr.scaled_cond(ci)
    return 8.0 * n * EPS * kappa


@pytest.mark.parametrize("name,one_focal", [(m, f) for m in MODELS for f in (False, True)] + [("rig2", False)])
def test_dense_schur_and_truth_agree(oracle, name, one_focal):
    sp, ci, d, s = _case(name, one_focal)
    t = cr.truth(ci)
    bound = _bound(ci)
    devs = {"schur-dense": cr.deviation(s, d), "dense-truth": cr.deviation(d, t), "schur-truth": cr.deviation(s, t)}
    print(name, one_focal, "n_free", ci.n_free, "bound %.2e" % bound, {k: ["%.2e" % x for x in v] for k, v in devs.items()},
          "pivot ratios V %.3g S %.3g" % (s["v_ratio"], s["s_ratio"]))
    for k, v in devs.items():
        assert max(v) <= bound, (k, v, bound)
    for o in (d, s, t):
        assert (o["dof"], o["n_free"], o["n_posed"]) == (2 * ci.N - ci.n_free, ci.n_free, ci.n_slots)
        assert abs(o["cost"] - t["cost"]) <= 64 * EPS * t["cost"]


@pytest.mark.parametrize("one_focal", [False, True])
@pytest.mark.parametrize("name", MODELS)
def test_leverages_sum_to_n_free(oracle, name, one_focal):
    sp, ci, d, s = _case(name, one_focal)
    for o in (d, s):
        assert abs(o["leverage_sum"] - ci.n_free) <= _bound(ci) * ci.n_free, (o["leverage_sum"], ci.n_free)
        assert o["leverage"].min() >= 0.0 and o["leverage"].max() <= 2.0


def test_leverages_sum_two_camera_rig(oracle):
    sp, ci, d, s = _case("rig2")
    assert ci.n_free == 18 + 6 * 4
    for o in (d, s):
        assert abs(o["leverage_sum"] - ci.n_free) <= _bound(ci) * ci.n_free


def test_fixed_parameters_are_deleted_columns(oracle):
    """fixed focal and the last two distortion parameters: zero rows and columns, and the rest equals the dense inverse of H with
    those columns deleted by hand"""
    from oracle import binding as ob
    sp = cr.small_case("opencv5")
    op = ob.OracleProblem.from_synth(sp)
    intr = sp.intr_gt.copy()
    op.disable_distortions(2, intr)
    op.fix_param(0, 0)
    ci = cr.CovInputs(op, intr, sp.poses_gt)
    fixed = [0, 7, 8]
    assert list(np.nonzero(ci.fixed)[0]) == fixed and ci.n_free == 6 + 18
    d, s = cr.dense(ci), cr.schur(ci)
    n = ci.K + 6 * ci.n_slots
    H = np.zeros((n, n))
    for o in range(ci.n_obs):
        cols = ci.full_cols(o)
        H[np.ix_(cols, cols)] += ci.Jb[o].T @ ci.Jb[o]
    Hd = np.linalg.inv(np.delete(np.delete(H, fixed, 0), fixed, 1))
    free = [i for i in range(ci.K) if i not in fixed]
    ref = d["sigma2"] * Hd[:len(free), :len(free)]
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    for o in (d, s):
        assert not o["cov_cam"][fixed].any() and not o["cov_cam"][:, fixed].any()
        assert np.max(np.abs(o["cov_cam"][np.ix_(free, free)] - ref) / scale) <= _bound(ci)
    assert max(cr.deviation(s, d)) <= _bound(ci)
    assert abs(s["leverage_sum"] - 24) <= _bound(ci) * 24


@pytest.mark.parametrize("model", ["eucm", "opencv5"])
def test_definition_against_noise_draws(oracle, model):
    """200 draws of 0.1 px noise on make_problem(12, model, noise_px=0, seed=3), each solved by the oracle from the ground truth: the
    empirical standard deviation of every camera and pose parameter over the predicted one (the mean predicted variance) lies in
    0.8 .. 1.25 - 200 draws give a standard deviation to 5 %, the bounds are about five standard errors - and sigma2 recovers the
    noise variance (dof ~ 3 400: its mean over 200 draws has a standard error of 0.17 %; 1 % asked)."""
    import dataclasses
    from oracle import binding as ob
    clean = synth.make_problem(12, model, noise_px=0.0, seed=3)
    uv0 = clean.p2d.astype(np.float64)
    est_c, est_p, var_c, var_p, s2 = [], [], [], [], []
    for seed in range(1000, 1200):
        noise = 0.1 * synth.normal01(seed, uv0.size).reshape(uv0.shape)
        sp = dataclasses.replace(clean, p2d=(uv0 + noise).astype(np.float32))
        op = ob.OracleProblem.from_synth(sp)
        intr, poses, _, rep = op.solve(sp.intr_gt, sp.poses_gt)
        assert rep.status == 0
        out = cr.schur(cr.CovInputs(op, intr, poses))
        P = len(out["cov_cam"])
        est_c.append(intr[0, :P]); est_p.append(poses.ravel())
        var_c.append(np.diag(out["cov_cam"])); var_p.append(np.concatenate([np.diag(c) for c in out["cov_poses"]]))
        s2.append(out["sigma2"])
    rc = np.std(est_c, axis=0, ddof=1) / np.sqrt(np.mean(var_c, axis=0))
    rp = np.std(est_p, axis=0, ddof=1) / np.sqrt(np.mean(var_p, axis=0))
    print(model, "camera %.3f .. %.3f" % (rc.min(), rc.max()), "poses %.3f .. %.3f" % (rp.min(), rp.max()), "sigma2 / 0.01 = %.4f" % (np.mean(s2) / 0.01))
    assert 0.8 <= rc.min() and rc.max() <= 1.25, rc
    assert 0.8 <= rp.min() and rp.max() <= 1.25, (rp.min(), rp.max())
    assert abs(np.mean(s2) / 0.01 - 1.0) <= 0.01


def test_collinear_frame_trips_the_pivot_rule(oracle):
    from oracle import binding as ob
    sp = cr.collinear_problem()
    op = ob.OracleProblem.from_synth(sp)
    with pytest.raises(cr.NotPD) as e:
        cr.schur(cr.CovInputs(op, sp.intr_gt, sp.poses_gt))
    print("collinear frame: pivot ratio %.3g" % e.value.ratio)
    assert e.value.bad_slot == 1 and e.value.ratio <= cr.PIVOT_REL
    # and the well-posed problems sit far above it
    for name in MODELS:
        s = _case(name)[3]
        assert s["v_ratio"] > 1e-3 and s["s_ratio"] > 1e-6, (name, s["v_ratio"], s["s_ratio"])


def test_python_mirrors_check_arguments_without_a_device():
    p = Problem.__new__(Problem)                    # no library call is reached
    p.n_cams, p.n_slots, p.n_corners, p.K, p.handle = 2, 3, 10, 18, None
    with pytest.raises(ValueError, match="without intr"):
        p.covariance(None, np.zeros((3, 6)))
    with pytest.raises(ValueError, match="poses is missing"):
        p.covariance(np.zeros((2, 10)))
    with pytest.raises(ValueError, match="extr is missing"):
        p.covariance(np.zeros((2, 10)), np.zeros((3, 6)))
    with pytest.raises(ValueError, match="no frame"):
        api.calibration_uncertainty([None, None], api.GenericModel("ucm", [1, 1, 1, 1, 0.5], 10, 10), {})
    with pytest.raises(ValueError, match="no frame"):
        api.rig_uncertainty([api.GenericModel("ucm", [1, 1, 1, 1, 0.5], 10, 10)], [api.RvecTvec((0, 0, 0), (0, 0, 0))], {}, [[None]])
    # one focal: fy repeats fx's column of the reduced system
    cov = np.diag([4.0, 1.0, 1.0, 0.0])
    names, std, corr = api._camera_block(api.GenericModel("ucm", [1, 1, 1, 1, 0.5], 10, 10), cov, 0, True)
    assert names == ["fx", "fy", "cx", "cy", "alpha"] and list(std) == [2.0, 2.0, 1.0, 1.0, 0.0]
    assert corr[0, 1] == 1.0 and not corr[4].any() and not np.isnan(corr).any()
