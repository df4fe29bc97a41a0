"""ccal_solve_batch: independent problems solved side by side from one host thread (the per-camera calib_camera calls of a
rig, the retries of src/bin/camera_calibration.rs:205-246) - the same verdicts, iteration counts and accept / reject sequences as
solving them one after the other; results equal up to the order of summation (1e-11): a problem's launches are sized for its share
of the GPU (other lane mappings), and session-sized single-camera problems of one model advance in lockstep, one launch per step."""
import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import _ffi, synth
from camera_intrinsic_calibration_rs_amd.engine import CcalError, Context, Problem, default_opts

pytestmark = pytest.mark.gpu


def _cases():
    return [synth.make_problem(300, "eucm", seed=11, outlier_frac=0.02), synth.make_problem(200, "kb4", seed=12, xy_same_focal=True),
            synth.make_problem(40, "eucm", n_cams=2, seed=13), synth.make_problem(150, "ucm", seed=14, ragged=True),
            synth.make_problem(120, "opencv5", seed=15)]


@pytest.mark.parametrize("method", [_ffi.METHOD_GN, _ffi.METHOD_LM])
@pytest.mark.parametrize("own_context", [True, False])
def test_batch_equals_sequential(method, own_context):
    sps = _cases()
    shared = Context(0)
    ctxs = [Context(0) if own_context else shared for _ in sps]
    probs = [Problem.from_synth(c, s) for c, s in zip(ctxs, sps)]
    for p in probs:
        p.apply_reference_bounds()
    opts = default_opts(method)
    seq = [p.solve(s.intr0, s.poses0, s.extr0, opts=opts) for p, s in zip(probs, sps)]
    reps, res = Problem.solve_batch(probs, opts, starts=[(s.intr0, s.poses0, s.extr0) for s in sps])
    def same(a, b):
        np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-13)
    for (i0, p0, e0, r0), rep, (i1, p1, e1) in zip(seq, reps, res):
        assert (rep.status, rep.iterations, rep.lm_accepted, rep.lm_rejected) == (r0.status, r0.iterations, r0.lm_accepted, r0.lm_rejected)
        same(rep.final_cost, r0.final_cost); same(rep.initial_cost, r0.initial_cost)
        same(i1, i0); same(p1, p0); same(e1, e0)
    # device-resident form: starting points uploaded, results left on the device
    for p, s in zip(probs, sps):
        p.upload_params(s.intr0, s.poses0, s.extr0)
    reps2, none = Problem.solve_batch(probs, opts)
    assert none is None
    for p, (i0, p0, e0, r0), rep in zip(probs, seq, reps2):
        i1, p1, e1 = p.download_params()
        assert rep.iterations == r0.iterations
        same(rep.final_cost, r0.final_cost); same(i1, i0); same(p1, p0)
    for p in probs:
        p.close()


@pytest.mark.parametrize("method", [_ffi.METHOD_GN, _ffi.METHOD_LM])
def test_lockstep_groups(method):
    """Session-sized single-camera problems of one model and focal mode advance in lockstep - ONE launch per optimizer step for the
    whole group (k_gram1v_batch): members of different sizes (different iteration counts, different row counts - the grid is the
    largest one's), a member that finishes early, LM rejections on one member only, a member whose frames do not cover every slot
    (its starting point arrives through k_unpack1 instead of the first launch), host pointers and the device-resident form; two
    groups (EUCM, one-focal KB4, OPENCV5 - which takes the single-launch form only as a batch member) plus a rig that takes the
    per-context path in the same call."""
    import dataclasses
    sps = [synth.make_problem(300, "eucm", seed=31, outlier_frac=0.02), synth.make_problem(120, "eucm", seed=32, ragged=True),
           synth.make_problem(12, "eucm", seed=1, outlier_frac=0.05, ragged=True, init_perturb=0.8),          # LM rejects steps here
           synth.make_problem(625, "eucm", seed=34), synth.make_problem(200, "kb4", seed=35, xy_same_focal=True),
           synth.make_problem(90, "kb4", seed=36, xy_same_focal=True, ragged=True), synth.make_problem(30, "eucm", n_cams=2, seed=37),
           synth.make_problem(150, "opencv5", seed=38), synth.make_problem(260, "opencv5", seed=39, outlier_frac=0.01)]
    # member 1: drop the last slot's frame -> not every slot observed (no fold)
    s1 = sps[1]
    keep = np.nonzero(s1.obs_slot != s1.n_slots - 1)[0]
    offs = np.concatenate([[0], np.cumsum((s1.obs_offsets[1:] - s1.obs_offsets[:-1])[keep])]).astype(np.int64)
    idx = np.concatenate([np.arange(s1.obs_offsets[o], s1.obs_offsets[o + 1]) for o in keep])
    sps[1] = dataclasses.replace(s1, obs_cam=s1.obs_cam[keep].copy(), obs_slot=s1.obs_slot[keep].copy(), obs_offsets=offs,
                                 p3d=s1.p3d[idx].copy(), p2d=s1.p2d[idx].copy())
    ctxs = [Context(0) for _ in sps]
    probs = [Problem.from_synth(c, s) for c, s in zip(ctxs, sps)]
    for p in probs:
        p.apply_reference_bounds()
    opts = default_opts(method)
    seq = [p.solve(s.intr0, s.poses0, s.extr0, opts=opts, raise_on_error=False) for p, s in zip(probs, sps)]
    if method == _ffi.METHOD_LM:
        assert seq[2][3].lm_rejected >= 1
    for rep_i in range(2):                            # twice: the second batch starts behind the first one's last launches
        reps, res = Problem.solve_batch(probs, opts, starts=[(s.intr0, s.poses0, s.extr0) for s in sps])
        for (i0, p0, e0, r0), rep, (i1, p1, e1) in zip(seq, reps, res):
            assert (rep.status, rep.iterations, rep.lm_accepted, rep.lm_rejected) == (r0.status, r0.iterations, r0.lm_accepted, r0.lm_rejected)
            np.testing.assert_allclose(rep.final_cost, r0.final_cost, rtol=1e-11)
            np.testing.assert_allclose(i1, i0, rtol=1e-11, atol=1e-13); np.testing.assert_allclose(p1, p0, rtol=1e-11, atol=1e-13)
    for p, s in zip(probs, sps):
        p.upload_params(s.intr0, s.poses0, s.extr0)
    reps2, _ = Problem.solve_batch(probs, opts)
    for p, (i0, p0, e0, r0), rep in zip(probs, seq, reps2):
        i1, p1, e1 = p.download_params()
        assert (rep.status, rep.iterations) == (r0.status, r0.iterations)
        np.testing.assert_allclose(i1, i0, rtol=1e-11, atol=1e-13); np.testing.assert_allclose(p1, p0, rtol=1e-11, atol=1e-13)
    # and a plain ccal_solve on a member afterwards (its own stream again) still gives its result
    i2, p2, _, r2 = probs[0].solve(sps[0].intr0, sps[0].poses0, opts=opts)
    np.testing.assert_array_equal(i2, seq[0][0]); np.testing.assert_array_equal(p2, seq[0][1])
    for p in probs:
        p.close()


def test_batch_reports_each_problems_own_verdict():
    """One problem of the batch has no step (a frame with a rank-deficient pose block: tiny-solver's None): its report says
    NOT_PD, the others solve; the call itself succeeds."""
    good = synth.make_problem(50, "eucm", seed=3)
    bad = synth.make_problem(6, "eucm", seed=4)
    bad.p3d[: bad.obs_offsets[1]] = bad.p3d[0]            # every corner of frame 0 the same board point: its 6 x 6 block is singular
    ctxs = [Context(0), Context(0)]
    probs = [Problem.from_synth(ctxs[0], good), Problem.from_synth(ctxs[1], bad)]
    reps, res = Problem.solve_batch(probs, default_opts(_ffi.METHOD_GN), starts=[(good.intr0, good.poses0, None), (bad.intr0, bad.poses0, None)])
    assert reps[0].status == _ffi.OK and reps[0].iterations >= 2
    assert reps[1].status in (_ffi.ERR_NOT_PD, _ffi.ERR_NONFINITE)
    _, _, _, r0 = probs[0].solve(good.intr0, good.poses0)
    assert r0.final_cost == pytest.approx(reps[0].final_cost, rel=1e-11)
    for p in probs:
        p.close()


def test_a_failing_member_of_a_lockstep_group_does_not_take_its_neighbours_down(monkeypatch):
    """when one member's preparation fails (out of memory for its workspace, ...) the others of the lockstep group
    still solve and every report carries its own problem's verdict; the failing member's context alone holds the reason.  The
    failure is injected through the second library's test hook (the product has none)."""
    import ctypes as C
    lib = _ffi.load_legacy()
    sps = [synth.make_problem(200, "eucm", seed=40 + i) for i in range(3)]
    ctxs = [Context(0, lib=lib) for _ in sps]
    probs = [Problem.from_synth(c, s) for c, s in zip(ctxs, sps)]
    solo = [p.solve(s.intr0, s.poses0)[3] for p, s in zip(probs, sps)]
    monkeypatch.setenv("CCAL_TEST_FAIL_BATCH_MEMBER", "1")
    hs = (C.c_void_p * 3)(*[p.handle for p in probs])
    reps = (_ffi.Report * 3)()
    for p, s in zip(probs, sps):
        p.upload_params(s.intr0, s.poses0, s.extr0)
    opts = default_opts(0)
    rc = lib.ccal_solve_batch(hs, 3, C.byref(opts), None, None, None, reps)
    monkeypatch.delenv("CCAL_TEST_FAIL_BATCH_MEMBER")
    assert rc == _ffi.ERR_NO_MEMORY                          # the call reports the first non-verdict failure ...
    assert reps[1].status == _ffi.ERR_NO_MEMORY and "injected" in ctxs[1].last_error()
    for k in (0, 2):                                         # ... and the neighbours have solved
        assert reps[k].status == _ffi.OK and reps[k].iterations == solo[k].iterations
        assert reps[k].final_cost == pytest.approx(solo[k].final_cost, rel=1e-11)
        assert "injected" not in ctxs[k].last_error()
    # and the batch works again afterwards, all three
    reps2, _ = Problem.solve_batch(probs, opts, starts=[(s.intr0, s.poses0, s.extr0) for s in sps])
    assert [r.status for r in reps2] == [0, 0, 0] and [r.iterations for r in reps2] == [r.iterations for r in solo]
    for p in probs:
        p.close()


def _assert_same_as_alone(alone, reps, results):
    """the file's comparison: verdict, iteration count and accept / reject sequence equal, costs and parameters to 1e-11"""
    def same(a, b):
        np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-13)
    for (i0, p0, e0, r0), rep, (i1, p1, e1) in zip(alone, reps, results):
        assert (rep.status, rep.iterations, rep.lm_accepted, rep.lm_rejected) == (r0.status, r0.iterations, r0.lm_accepted, r0.lm_rejected)
        same(rep.final_cost, r0.final_cost); same(rep.initial_cost, r0.initial_cost)
        same(i1, i0); same(p1, p0); same(e1, e0)


@pytest.mark.parametrize("method", [_ffi.METHOD_GN, _ffi.METHOD_LM])
def test_a_context_with_lockstep_members_and_a_problem_of_its_own(method):
    """Context A holds two members of a lockstep group AND a rig that takes the per-context path; context B holds the group's third
    member.  The members on A share one stream - the group's own when A comes first, another one when the order is reversed and B's
    is the group's - and A's rig is solved on the caller's thread behind the group, never by A's helper thread."""
    sps = [synth.make_problem(40, "eucm", seed=51), synth.make_problem(60, "eucm", seed=52, outlier_frac=0.02),
           synth.make_problem(20, "eucm", n_cams=2, seed=53), synth.make_problem(50, "eucm", seed=54)]
    a, b = Context(0), Context(0)
    probs = [Problem.from_synth(c, s) for c, s in zip((a, a, a, b), sps)]
    for p in probs:
        p.apply_reference_bounds()
    opts = default_opts(method)
    alone = [p.solve(s.intr0, s.poses0, s.extr0, opts=opts) for p, s in zip(probs, sps)]
    starts = [(s.intr0, s.poses0, s.extr0) for s in sps]
    reps, res = Problem.solve_batch(probs, opts, starts=starts)
    _assert_same_as_alone(alone, reps, res)
    reps, res = Problem.solve_batch(probs[::-1], opts, starts=starts[::-1])          # the group's first context is B
    _assert_same_as_alone(alone[::-1], reps, res)
    for p, s in zip(probs, sps):                                                         # device-resident form
        p.upload_params(s.intr0, s.poses0, s.extr0)
    reps, none = Problem.solve_batch(probs, opts)
    assert none is None
    _assert_same_as_alone(alone, reps, [p.download_params() for p in probs])
    for p in probs:
        p.close()


@pytest.mark.parametrize("method", [_ffi.METHOD_GN, _ffi.METHOD_LM])
def test_members_sent_back_by_the_group_are_solved_on_their_own(method, monkeypatch):
    """The plan groups by size, model and lane mapping; whether a problem's workspace takes single-launch groups at all is known
    only once it is prepared.  With the second library's CCAL_FUSE_ELIM=0 (read when the workspace is made: the separate elimination
    launch) three problems are planned as one group, every one of them is sent back and solved on its own behind the group - with
    the results of solving it alone, and again in a second batch."""
    lib = _ffi.load_legacy()
    sps = [synth.make_problem(60, "eucm", seed=60 + i) for i in range(3)]
    probs = [Problem.from_synth(Context(0, lib=lib), s) for s in sps]
    for p in probs:
        p.apply_reference_bounds()
    opts = default_opts(method)
    monkeypatch.setenv("CCAL_FUSE_ELIM", "0")
    alone = [p.solve(s.intr0, s.poses0, s.extr0, opts=opts) for p, s in zip(probs, sps)]      # workspaces (and the choice) made under the switch
    starts = [(s.intr0, s.poses0, s.extr0) for s in sps]
    for _ in range(2):
        reps, res = Problem.solve_batch(probs, opts, starts=starts)
        _assert_same_as_alone(alone, reps, res)
    monkeypatch.delenv("CCAL_FUSE_ELIM")
    for p in probs:
        p.close()


def test_batch_argument_checks():
    sp = synth.make_problem(10, "eucm")
    ctx = Context(0)
    p = Problem.from_synth(ctx, sp)
    with pytest.raises(CcalError):
        Problem.solve_batch([p, p], default_opts(0))                 # the same problem twice
    reps, _ = Problem.solve_batch([], default_opts(0))
    assert reps == []
    p.close()


def test_calib_cameras_equals_per_camera_calib_camera(gpu_ctx):
    """api.calib_cameras = the tool's per-camera loop (src/bin/camera_calibration.rs:255-265) through one ccal_solve_batch."""
    from camera_intrinsic_calibration_rs_amd import api
    sp = synth.make_problem(24, "eucm", n_cams=3, seed=21)
    frames = [api.frames_from_synth(sp, c) for c in range(3)]
    frames[1][5] = None
    cams0 = [api.GenericModel("eucm", sp.intr0[c, :6], 512, 512) for c in range(3)]
    for fixed_focal in (False, True):
        batch = api.calib_cameras(frames, cams0, True, 0, fixed_focal)
        for c in range(3):
            one = api.calib_camera(frames[c], cams0[c], True, 0, fixed_focal, None, ctx=gpu_ctx)
            assert (one is None) == (batch[c] is None)
            np.testing.assert_allclose(batch[c][0].params(), one[0].params(), rtol=1e-11, atol=1e-13)
            assert sorted(batch[c][1]) == sorted(one[1])
            for k in one[1]:
                np.testing.assert_allclose(batch[c][1][k].as6(), one[1][k].as6(), rtol=1e-11, atol=1e-13)


def test_calib_cameras_over_a_device_list(gpu_ctx):
    """calib_cameras(devices=[...]): every camera's context placed round-robin on the listed GPUs ([0, 0] on the 1-GPU box, every
    visible GPU otherwise) - the per-camera loop's results."""
    import torch
    from camera_intrinsic_calibration_rs_amd import api
    nd = torch.cuda.device_count()
    devs = list(range(nd)) if nd > 1 else [0, 0]
    sp = synth.make_problem(30, "eucm", n_cams=3, seed=23, ragged=True)
    frames = [api.frames_from_synth(sp, c) for c in range(3)]
    cams0 = [api.GenericModel("eucm", sp.intr0[c, :6], 512, 512) for c in range(3)]
    batch = api.calib_cameras(frames, cams0, False, 0, False, devices=devs)
    for c in range(3):
        one = api.calib_camera(frames[c], cams0[c], False, 0, False, None, ctx=gpu_ctx)
        np.testing.assert_allclose(batch[c][0].params(), one[0].params(), rtol=1e-11, atol=1e-13)
        assert sorted(batch[c][1]) == sorted(one[1])
        for k in one[1]:
            np.testing.assert_allclose(batch[c][1][k].as6(), one[1][k].as6(), rtol=1e-11, atol=1e-13)


def test_calib_cameras_raises_when_the_fixed_focal_resolve_fails(monkeypatch):
    """calib_camera `.unwrap()`s its second, fixed-focal solve (src/util.rs:463): a camera whose re-optimisation ends NOT_PD
    must not come back as a silently copied result.  The failing verdict is injected into the second ccal_solve_batch's
    reports (a real one is hard to provoke once the first solve has converged)."""
    from camera_intrinsic_calibration_rs_amd import api
    sp = synth.make_problem(12, "eucm", n_cams=2, seed=22)
    frames = [api.frames_from_synth(sp, c) for c in range(2)]
    cams0 = [api.GenericModel("eucm", sp.intr0[c, :6], 512, 512) for c in range(2)]
    real = Problem.solve_batch
    calls = []

    def patched(problems, opts=None, starts=None):
        reps, res = real(problems, opts, starts)
        calls.append(len(problems))
        if len(calls) == 2:
            reps[1].status = _ffi.ERR_NOT_PD
        return reps, res

    monkeypatch.setattr(Problem, "solve_batch", staticmethod(patched))
    with pytest.raises(CcalError) as ei:
        api.calib_cameras(frames, cams0, True, 0, True)
    assert ei.value.code == _ffi.ERR_NOT_PD and calls == [2, 2]
