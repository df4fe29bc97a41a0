"""Every solve form the dispatch code picks with default switches, on POISONED memory, against the oracle.

The GPU parity tests elsewhere run on device memory that happens to be clean (fresh hipMalloc memory is zero in practice, the
session's contexts hand out blocks that earlier tests filled with plausible numbers): a kernel that reads a slice nobody wrote
goes unseen there.  Here each case runs on a FRESH context of the second library (libccal_hip_legacy.so, -DCCAL_TEST_HOOKS) with
CCAL_TEST_POISON_ALLOC=1: every block of doubles the library allocates - fresh or handed back by the context's block cache - is
filled with 0xFF bytes (a quiet NaN) before the library's own clears and uploads (test_poison_f64, csrc/ccal_solver_ws.hip).  A result
that depends on what was in memory before turns into NaN or a wrong verdict.  Each case must

  * equal the oracle at the suite's tolerances: |dr| <= 1e-10, |dJ| <= 1e-11 max(1, |J|), S / b 1e-9 of their largest entry, cost
    1e-12 relative, the same status, iteration count and LM accept / reject counts, final cost 1e-9, intrinsics 1e-6 relative,
    poses (and extrinsics) 1e-7 absolute;
  * be finite and bit-identical to the same case on a fresh context of the same library without the hook.

The last test holds the PRODUCT library to the path real sessions take: one context, a problem created, solved and destroyed, then
problems of other models and sizes whose blocks come out of the context's cache (ccal_internal.hpp: ctx_alloc) - bit-identical to
the same problems on a fresh context."""
import dataclasses
import functools
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth
from camera_intrinsic_calibration_rs_amd.engine import Context, Problem, default_opts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = "CCAL_TEST_POISON_ALLOC"
GN, LM = _ffi.METHOD_GN, _ffi.METHOD_LM


# ---- harness ---------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b, where=""):
    """Results of the two runs: dicts of arrays / floats / tuples, equal bit for bit (NaN included) and finite."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            assert np.isfinite(x).all(), f"{where}{k}: not finite on the poisoned context"
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{where}{k}: poisoned and clean runs differ"


def _second_library_only():
    """In a child process: the second library stands in for the product everywhere (default_opts, api), so that the product is
    never loaded.  The tests' processes load the product RTLD_GLOBAL first; the second library's calls into its own twice-compiled
    functions (normal_ws_ensure_general, ccal_build_normal_dev, ...) would then bind to the product's copies, hook-less."""
    from camera_intrinsic_calibration_rs_amd import _ffi as ffi
    assert ffi._lib is None
    ffi._lib = ffi.load_legacy()
    return ffi._lib


def _child(q, fn, args, poison):
    sys.path.insert(0, ROOT)
    if poison:
        os.environ[POISON] = "1"
    lib = _second_library_only()
    from camera_intrinsic_calibration_rs_amd.engine import Context as Ctx
    ctx = Ctx(0, lib=lib)
    try:
        out = fn(ctx, *args)
    finally:
        ctx.close()
    q.put(out)


def _in_child(target, args, timeout=240):
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    proc = ctxm.Process(target=target, args=(q,) + tuple(args))
    proc.start()
    try:
        res = q.get(timeout=timeout)
    except Exception:
        if proc.is_alive():
            proc.kill()                          # exactly the child started here
        proc.join(10)
        raise AssertionError(f"the child process hung or crashed (exit code {proc.exitcode})")
    proc.join(60)
    assert proc.exitcode == 0
    return res


def _poisoned_and_clean(fn, *args):
    """fn(ctx, *args) -> dict of results, run in a fresh process on a fresh context of the second library without the hook, then
    in another with it; returns the poisoned run's results after holding them to the clean run's bits."""
    clean = _in_child(_child, (fn, args, False))
    poisoned = _in_child(_child, (fn, args, True))
    _bits_equal(poisoned, clean)
    return poisoned


@functools.lru_cache(maxsize=None)
def _oracle_solve(key, method):
    """The oracle's solve of a case (8 threads, cached per module: several tests hold the GPU against the same solve)."""
    from oracle import binding
    sp = _case(key)
    op = binding.OracleProblem.from_synth(sp)
    binding.set_solve_threads(8)
    try:
        return op.solve(sp.intr0, sp.poses0, sp.extr0, opts=default_opts(method))
    finally:
        binding.set_solve_threads(1)


def _check_eval(r, J, ro, Jo):
    assert np.isfinite(r).all() and np.isfinite(J).all()
    assert np.abs(r - ro).max() <= 1e-10
    assert (np.abs(J - Jo) / np.maximum(1.0, np.abs(Jo))).max() <= 1e-11


def _check_normal(S, b, cost, So, bo, costo):
    assert np.isfinite(S).all() and np.isfinite(b).all() and np.isfinite(cost)
    assert abs(cost - costo) <= 1e-12 * costo
    assert np.abs(S - So).max() <= 1e-9 * np.abs(So).max()
    assert np.abs(b - bo).max() <= 1e-9 * np.abs(bo).max()


def _check_solve(sp, res, ref):
    intr, poses, extr, rep = res
    io, po, eo, ro = ref
    assert rep.status == ro.status == 0
    assert (rep.iterations, rep.lm_accepted, rep.lm_rejected) == (ro.iterations, ro.lm_accepted, ro.lm_rejected)
    assert abs(rep.initial_cost - ro.initial_cost) <= 1e-12 * ro.initial_cost
    assert abs(rep.final_cost - ro.final_cost) <= 1e-9 * ro.final_cost
    for c in range(sp.n_cams):
        P = synth.MODEL_NPARAMS[int(sp.model[c])]
        assert (np.abs(intr[c, :P] - io[c, :P]) / np.maximum(np.abs(io[c, :P]), 1e-3)).max() <= 1e-6
    assert np.isfinite(poses).all()
    np.testing.assert_allclose(poses, po, rtol=0, atol=1e-7)
    np.testing.assert_allclose(extr, eo, rtol=0, atol=1e-7)


def _rep(rep):
    return (rep.status, rep.iterations, rep.lm_accepted, rep.lm_rejected, rep.lm_spec_misses, rep.initial_cost, rep.final_cost)


def _solve_results(gp, sp, method, pinned=False):
    i, p, e, r = gp.solve(sp.intr0, sp.poses0, sp.extr0, opts=default_opts(method), pinned=pinned)
    return {f"intr{method}": i, f"poses{method}": np.array(p), f"extr{method}": e, f"rep{method}": _rep(r)}, (i, np.array(p), e, r)


# the problems of the matrix (module-level builders: the oracle's cached solves key on the name)
_CASES = {
    "session600": lambda: synth.make_problem(600, "eucm", seed=0x7A11, ragged=True, noise_px=0.1),
    "ocv5_300": lambda: synth.make_problem(300, "opencv5", seed=0x0C5, outlier_frac=0.01),
    "ragged2500": lambda: synth.make_problem(2500, "eucm", ragged=True, seed=0xAB5, outlier_frac=0.01),
    "spread3000": lambda: synth.make_problem(3000, "kb4", seed=0x3000, outlier_frac=0.01),
    "staged9800": lambda: synth.make_problem(9800, "eucm", outlier_frac=0.01, seed=0x9800),
    "ragged10000": lambda: synth.make_problem(10000, "eucm", ragged=True, seed=0xC0FFEE + 77),
    "pinned400": lambda: synth.make_problem(400, "kb4", seed=0x400),
    "rig2": lambda: synth.make_problem(300, "eucm", n_cams=2, seed=0x2C, outlier_frac=0.01),
    "rig_schurq": lambda: synth.make_rig(1200, ["eucm", "eucm"], np.array([[0.0] * 6, [0.3, -0.25, 0.2, -0.1, 0.02, 0.01]]),
                                         seed=0x5C4, drop_frac=0.15),
    "rig_mixed": lambda: synth.make_rig(3200, ["kb4", "eucm"], np.array([[0.0] * 6, [0.05, -0.2, 0.1, 0.1, -0.02, 0.03]]),
                                        seed=0xA12, drop_frac=0.15),
}


@functools.lru_cache(maxsize=None)
def _case(key):
    return _CASES[key]()


def _run_eval(ctx, sp):
    gp = Problem.from_synth(ctx, sp)
    out = {}
    for loss in (False, True):
        out[f"r{loss}"], out[f"J{loss}"] = gp.eval(sp.intr0, sp.poses0, sp.extr0, apply_loss=loss)
    out["err"] = gp.reprojection_errors(sp.intr0, sp.poses0, sp.extr0)
    for c in range(sp.n_cams):
        out[f"val{c}"] = gp.validation(c, sp.intr0, sp.poses0, sp.extr0)
    gp.close()
    return out


def _run_solve(ctx, sp, methods, pinned=False):
    gp = Problem.from_synth(ctx, sp)
    out = {}
    for m in methods:
        out.update(_solve_results(gp, sp, m, pinned=pinned)[0])
    gp.close()
    return out


# ---- mode E, reprojection errors, validation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n_cams,frames", [("eucm", 1, 40), ("kb4", 1, 200), ("eucm", 2, 30), ("kb4", 2, 120)])
def test_mode_e_errors_and_validation(oracle, model, n_cams, frames):
    """ccal_eval (k_eval: one launch per camera, ccal_api.hip ccal_eval_dev), ccal_reprojection_errors (k_reproj_err) and
    ccal_validation: 40 x 144 = 5 760 corners per camera take the one-workgroup selection k_sel_one (n <= kSelOneMax = 8 192,
    ccal_kernels_stats.hip order_stats_device), 200 x 144 and 2 x 120 x 144 the histogram passes k_sel_hist / k_sel_sum /
    k_sel_finish."""
    sp = synth.make_problem(frames, model, n_cams=n_cams, seed=0xE0 + frames, outlier_frac=0.02)
    op = oracle.OracleProblem.from_synth(sp)
    out = _poisoned_and_clean(_run_eval, sp)
    for loss in (False, True):
        _check_eval(out[f"r{loss}"], out[f"J{loss}"], *op.eval(sp.intr0, sp.poses0, sp.extr0, apply_loss=loss, threads=8))
    assert np.abs(out["err"] - op.reprojection_errors(sp.intr0, sp.poses0, sp.extr0)).max() <= 1e-10
    for c in range(n_cams):
        a, m = out[f"val{c}"]
        ao, mo = op.validation(c, sp.intr0, sp.poses0, sp.extr0)
        assert abs(a - ao) <= 1e-9 and abs(m - mo) <= 1e-9


# ---- single-camera solves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,methods", [
    ("session600", (GN, LM)),       # poses 28.8 KB <= kZeroCopyBytes: zero-copy result, single-launch k_gram1v groups, folded unpack
    ("ocv5_300", (GN, LM)),         # fused_iter_rows() == 0 for OPENCV5 outside a batch: the three-launch form
    ("ragged2500", (GN, LM)),       # gram2_bin_plan bins 2 500 ragged frames: binned k_gram2b, three-launch form
    ("spread3000", (GN,)),          # kZeroCopyBytes < 144 KB <= kSpreadBytes: the result written to the host by every workgroup
    ("ragged10000", (GN, LM)),      # the benchmark's ragged workload: k_gram2i<..., SORTED=true> over the folded table
], ids=["session600", "ocv5_300", "ragged2500", "spread3000", "ragged10000"])
def test_single_camera_solve(oracle, key, methods):
    """Single-camera solves of every size class (csrc/ccal_normal.hpp: kZeroCopyBytes = 96 KB = 2 048 frames of poses,
    kSpreadBytes = 256 KB = 5 461 frames; FusedJob::begin chooses single-launch groups or the three-launch form) against the
    oracle on poisoned memory."""
    sp = _case(key)
    out = _poisoned_and_clean(_run_solve, sp, methods)
    for m in methods:
        _check_solve(sp, (out[f"intr{m}"], out[f"poses{m}"], out[f"extr{m}"], _Rep(*out[f"rep{m}"])), _oracle_solve(key, m))


@dataclasses.dataclass
class _Rep:
    status: int
    iterations: int
    lm_accepted: int
    lm_rejected: int
    lm_spec_misses: int
    initial_cost: float
    final_cost: float


def _run_staged(ctx, sp):
    gp = Problem.from_synth(ctx, sp)
    out = _solve_results(gp, sp, GN)[0]
    gp.upload_params(sp.intr0, sp.poses0, sp.extr0)
    rd = gp.solve_dev(default_opts(GN))
    out["dev_intr"], out["dev_poses"], _ = gp.download_params()
    out["dev_rep"] = _rep(rd)
    gp.close()
    return out


def test_staged_headline_solve_host_and_device(oracle):
    """9 800 x 144 uniform frames: poses (470 KB) beyond kSpreadBytes are staged through device copies, the loop runs single-launch
    groups of k_gram2i (FusedJob::begin); host pointers (ccal_solve) and the device-resident form (ccal_solve_dev +
    ccal_download_params)."""
    out = _poisoned_and_clean(_run_staged, _case("staged9800"))
    sp = _case("staged9800")
    _check_solve(sp, (out["intr0"], out["poses0"], out["extr0"], _Rep(*out["rep0"])), _oracle_solve("staged9800", GN))
    assert out["dev_rep"] == out["rep0"]
    np.testing.assert_array_equal(out["dev_intr"][0], out["intr0"][0]); np.testing.assert_array_equal(out["dev_poses"], out["poses0"])


def test_pinned_caller_poses(oracle):
    """A pose array the caller pinned (ccal_pin_buffer): ccal_solve reads the start from it and writes the result into it through its
    device address (pinned_device_ptr), no staging copy."""
    sp = _case("pinned400")
    out = _poisoned_and_clean(_run_solve, sp, (GN, LM), True)
    for m in (GN, LM):
        _check_solve(sp, (out[f"intr{m}"], out[f"poses{m}"], out[f"extr{m}"], _Rep(*out[f"rep{m}"])), _oracle_solve("pinned400", m))


# ---- normal equations -----------------------------------------------------------------------------------------------------------
def _run_normal(ctx, sp):
    gp = Problem.from_synth(ctx, sp)
    out = {}
    gp.upload_params(sp.intr0, sp.poses0, sp.extr0)
    gp.build_normal_dev(0.0)
    for lam in (0.0, 1e-3):
        out[f"S{lam}"], out[f"b{lam}"], out[f"c{lam}"] = gp.build_normal(sp.intr0, sp.poses0, sp.extr0, lam=lam)
    gp.close()
    return out


@pytest.mark.parametrize("key", ["single1000", "ragged2500", "rig2", "rig_schurq", "rig_mixed", "rig5"])
def test_build_normal(oracle, key):
    """ccal_build_normal_dev and ccal_build_normal at lambda = 0 and 1e-3: one camera (the register Gram kernel with the elimination
    fused into its tail, FusedWs), 2 500 ragged frames (binned k_gram2b), a two-camera rig (general loop: k_gram1v records, k_schur,
    k_reduce), a rig of two EUCM cameras over 1 200 slots with slots one camera does not see (k_schurq from 1 000 slots, records at
    fixed places: the missing ones are holes of G that must read as zeros - normal_ws_ensure_general), a ragged KB4 + EUCM rig over
    3 200 slots, some seen by one camera only (drop_frac; every camera's list holds >= 2 000 frames: a binned k_gram2g launch per
    camera, plan_list), and a five-camera KB4 rig (64 columns: one-wavefront k_schur workgroups, normal_ws_ensure_general)."""
    if key == "single1000":
        sp = synth.make_problem(1000, "eucm", seed=0x1000, outlier_frac=0.01)
    elif key == "rig5":
        ext = np.zeros((5, 6))
        for c in range(1, 5):
            ext[c] = [0.1 * c, -0.05 * c, 0.02, 0.05, -0.01 * c, 0.02]
        sp = synth.make_rig(200, ["kb4"] * 5, ext, seed=0x55, drop_frac=0.3)
    else:
        sp = _case(key)
    op = oracle.OracleProblem.from_synth(sp)
    out = _poisoned_and_clean(_run_normal, sp)
    for lam in (0.0, 1e-3):
        _check_normal(out[f"S{lam}"], out[f"b{lam}"], out[f"c{lam}"], *op.build_normal(sp.intr0, sp.poses0, sp.extr0, lam=lam))


# ---- rigs: the general loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["rig2", "rig_schurq", "rig_mixed"])
def test_rig_solve(oracle, key):
    """The general loop (GeneralJob, csrc/ccal_solver.hip: k_gram1v / k_gram2g records, k_schur, k_reduce, k_backsub): a two-camera rig of one model
    (one merged Gram launch), the k_schurq rig with holes in G, and the ragged KB4 + EUCM rig: 5 464 observation frames, more than
    the 4 000 up to which the Gram kernels' prologue forms the candidate poses, so the separate k_backsub launch runs
    (ccal_solver.hip: gen_backsub).  GN and LM."""
    sp = _case(key)
    out = _poisoned_and_clean(_run_solve, sp, (GN, LM))
    for m in (GN, LM):
        _check_solve(sp, (out[f"intr{m}"], out[f"poses{m}"], out[f"extr{m}"], _Rep(*out[f"rep{m}"])), _oracle_solve(key, m))


# ---- ccal_solve_batch -----------------------------------------------------------------------------------------------------------
def _run_batch(ctx0, sps):
    ctxs = [ctx0] + [Context(0, lib=ctx0.lib) for _ in sps[1:]]
    probs = [Problem.from_synth(c, s) for c, s in zip(ctxs, sps)]
    out = {}
    for m in (GN, LM):
        reps, res = Problem.solve_batch(probs, default_opts(m), starts=[(s.intr0, s.poses0, s.extr0) for s in sps])
        for k, (rep, (i, p, e)) in enumerate(zip(reps, res)):
            out[f"{k}intr{m}"], out[f"{k}poses{m}"], out[f"{k}extr{m}"], out[f"{k}rep{m}"] = i, p, e, _rep(rep)
    for p in probs:
        p.close()
    for c in ctxs[1:]:
        c.close()
    return out


def test_batch_lockstep_group(oracle):
    """Four session-sized EUCM problems, one context each: ONE lockstep group, one k_gram1v_batch launch per step for all four
    (ccal_solve_batch, the batch argument table)."""
    sps = [synth.make_problem(n, "eucm", seed=0xBA + n, outlier_frac=0.01, ragged=r) for n, r in ((300, False), (250, True), (200, False), (320, True))]
    out = _poisoned_and_clean(_run_batch, sps)
    for k, sp in enumerate(sps):
        op = oracle.OracleProblem.from_synth(sp)
        for m in (GN, LM):
            _check_solve(sp, (out[f"{k}intr{m}"], out[f"{k}poses{m}"], out[f"{k}extr{m}"], _Rep(*out[f"{k}rep{m}"])),
                         op.solve(sp.intr0, sp.poses0, sp.extr0, opts=default_opts(m)))


# ---- ccal_multi_solve, in-process transport -------------------------------------------------------------------------------------
def _child_multi(q, sp):
    """Fresh process (the in-process transport's threads and events stay out of the test process): two shards of GPU 0, the
    second library, clean and then poisoned."""
    sys.path.insert(0, ROOT)
    lib = _second_library_only()
    from camera_intrinsic_calibration_rs_amd import _ffi as ffi
    from camera_intrinsic_calibration_rs_amd.engine import MultiContext, MultiProblem, default_opts as dopts
    out = {}
    for tag in ("clean", "poisoned"):
        if tag == "poisoned":
            os.environ[POISON] = "1"
        mc = MultiContext([0, 0], transport=ffi.TRANSPORT_INPROC, lib=lib)
        mpb = MultiProblem.from_synth(mc, sp)
        res = {}
        for m in (GN, LM):
            i, p, e, r = mpb.solve(sp.intr0, sp.poses0, sp.extr0, opts=dopts(m))
            res[f"intr{m}"], res[f"poses{m}"], res[f"extr{m}"], res[f"rep{m}"] = i, np.array(p), e, _rep(r)
        res["val"] = mpb.validation(0, sp.intr0, sp.poses0, sp.extr0)
        out[tag] = res
        mpb.close(); mc.close()
    os.environ.pop(POISON, None)
    q.put(out)


def test_multi_solve_two_shards_in_process(oracle):
    """ccal_multi_solve over two shards of GPU 0 with the in-process transport: the deciding kernel adds the ranks' sums from the
    alternating `red` buffers of each rank (ccal_multi.hip inproc_post, NormalWs::red / FusedWs::red: two buffers each)."""
    sp = synth.make_problem(41, "eucm", n_cams=2, outlier_frac=0.01, ragged=True, seed=0x41)
    res = _in_child(_child_multi, (sp,))
    _bits_equal(res["poisoned"], res["clean"])
    out = res["poisoned"]
    op = oracle.OracleProblem.from_synth(sp)
    for m in (GN, LM):
        # the sharded solve sums in another order than one GPU: the oracle's tolerances, and the sharded suite's own bound on poses
        intr, poses, extr, rep = out[f"intr{m}"], out[f"poses{m}"], out[f"extr{m}"], _Rep(*out[f"rep{m}"])
        io, po, eo, ro = op.solve(sp.intr0, sp.poses0, sp.extr0, opts=default_opts(m))
        _check_solve(sp, (intr, poses, extr, rep), (io, po, eo, ro))
    ao, mo = op.validation(0, sp.intr0, sp.poses0, sp.extr0)
    assert abs(out["val"][0] - ao) <= 1e-9 and abs(out["val"][1] - mo) <= 1e-9


# ---- convert_model, init_poses, init_ucm ----------------------------------------------------------------------------------------
_EUCM_GT = [190.89618687183938, 190.87022285882367, 254.9375370481962, 256.86414483060787, 0.6283550447635853, 1.0458678747533083]
_KB4_GT = [190.9, 190.9, 255.0, 257.0, 0.003, 0.0007, -0.002, 0.0002]


def _run_convert_init(ctx, sp, su):
    out = {}
    for src, sp_, tgt, tp in (("eucm", _EUCM_GT, "kb4", [0.0] * 8), ("kb4", _KB4_GT, "eucm", [0, 0, 0, 0, 0.5, 1.0])):
        out[f"conv_{src}"] = np.asarray(api.convert_model(api.GenericModel(src, sp_, 512, 512), api.GenericModel(tgt, tp, 512, 512),
                                                          0, ctx=ctx).params())
    gp = Problem.from_synth(ctx, sp)
    out["poses"], out["used"] = gp.init_poses(sp.intr_gt)
    gp.close()
    frames = api.frames_from_synth(su)
    m = api.init_ucm(frames[0], frames[1], api.RvecTvec.from6(su.poses0[0]), api.RvecTvec.from6(su.poses0[1]),
                     init_f=su.intr_gt[0, 0] * 1.3, init_alpha=0.4, fixed_focal=False, ctx=ctx)
    out["ucm"] = np.asarray(m.params())
    return out


def test_convert_init_poses_init_ucm(oracle):
    """convert_model (k_convert_rays / k_convert_gram, ccal_convert.hip: the d_buf block) against the oracle's fit, ccal_init_poses
    (k_pose_init: poses in the problem's scratch block) against the ground truth, and init_ucm (two small solves on a problem of its
    own) - all bit-identical to the clean run."""
    sp = synth.make_problem(40, "kb4", ragged=True, seed=0x1417)
    su = synth.make_problem(2, "ucm", seed=77)
    gt = su.intr_gt[0]
    out = _poisoned_and_clean(_run_convert_init, sp, su)
    lo = {"kb4": ([0, 0, 0, 0, -1, -1, -1, -1], [1e4, 1e4, 512, 512, 1, 1, 1, 1]),
          "eucm": ([0, 0, 0, 0, 1e-6, 1e-6], [1e4, 1e4, 512, 512, 1.0, 100.0])}
    for src, sp_, tgt, tp in (("eucm", _EUCM_GT, "kb4", [0.0] * 8), ("kb4", _KB4_GT, "eucm", [0, 0, 0, 0, 0.5, 1.0])):
        p_o, n, rc = oracle.convert_model(api.GenericModel(src, sp_, 512, 512).model_id, sp_, api.GenericModel(tgt, tp, 512, 512).model_id,
                                          tp, 512, 512, 0, *lo[tgt])
        assert rc == 0 and n > 0
        np.testing.assert_allclose(out[f"conv_{src}"], p_o, rtol=1e-8, atol=1e-10)
    assert (out["used"] == np.diff(sp.obs_offsets)).all()
    assert np.abs(out["poses"][:, 3:] - sp.poses_gt[:, 3:]).max() < 0.01
    p = out["ucm"]
    assert p[0] == p[1] and abs(p[0] / gt[0] - 1) < 0.03 and abs(p[4] - gt[4]) < 0.05


# ---- the product library, blocks handed back by the context's cache --------------------------------------------------------------
def _product_run(ctx, sp):
    gp = Problem.from_synth(ctx, sp)
    out = {}
    out["r"], out["J"] = gp.eval(sp.intr0, sp.poses0, sp.extr0)
    out["S"], out["b"], out["cost"] = gp.build_normal(sp.intr0, sp.poses0, sp.extr0, lam=1e-3)
    for m in (GN, LM):
        out.update(_solve_results(gp, sp, m)[0])
    out["err"] = gp.reprojection_errors(sp.intr0, sp.poses0, sp.extr0)
    out["val"] = tuple(gp.validation(c, sp.intr0, sp.poses0, sp.extr0) for c in range(sp.n_cams))
    gp.close()
    return out


def test_product_blocks_reused_across_problems():
    """The path real sessions take on the library users load (a problem per camera and per retry, api.calib_camera): on ONE product
    context, a 1 000-frame EUCM problem is created, evaluated, solved, validated and destroyed; its blocks go to the context's cache
    with their contents.  ctx_alloc hands a cached block of B bytes to a request of R bytes (R rounded up to 256) when
    R <= B <= R + R / 4 + 4096.  The next problems are sized to land in that window:

      * 800 KB4 frames: J 800 x 144 x 2 x 14 doubles = 25.8 MB <= the EUCM problem's 1 000 x 144 x 2 x 12 x 8 = 27.6 MB
        <= 1.25 x 25.8 MB; r 1.84 MB against 2.30 MB (= 1.25 x 1.84 MB); the fused workspace, per-frame and stage blocks in between;
      * 900 ragged UCM frames (fewer corners: smaller r / J / errors blocks, the same per-frame blocks within 10 %);
      * a 450-frame two-camera EUCM rig (the general loop's blocks, new, and r / J of 900 frames' corners out of the cache).

    Each is bit-identical - mode E, normal equations, GN and LM, errors, validation - to the same problem on a fresh context."""
    big = synth.make_problem(1000, "eucm", seed=0xB16, outlier_frac=0.01)
    rest = [synth.make_problem(800, "kb4", seed=0x800, outlier_frac=0.01), synth.make_problem(900, "ucm", ragged=True, seed=0x900),
            synth.make_problem(450, "eucm", n_cams=2, seed=0x450)]
    shared = Context(0)
    try:
        _product_run(shared, big)
        for sp in rest:
            reused = _product_run(shared, sp)
            fresh_ctx = Context(0)
            try:
                fresh = _product_run(fresh_ctx, sp)
            finally:
                fresh_ctx.close()
            _bits_equal(reused, fresh, where=f"{sp.n_slots} frames: ")
    finally:
        shared.close()


def test_dirty_general_block_serves_next_rig():
    """A rig's general workspace is ONE device block (csrc/ccal_normal.hpp: GeneralLayout), so a destroyed rig leaves the context's
    cache one large dirty block - record buffers, partial sums, index tables, optimizer state - that the next rig of a similar size
    gets whole.  On one product context the rig_schurq case (two EUCM cameras over 1 200 slots, drop_frac 0.15: k_schurq, whose
    record buffers have holes that must read as zeros) is solved and destroyed; then a rig of 1 100 slots with another seed, whose
    holes fall elsewhere, runs mode E, ccal_build_normal, GN, LM, errors and validation - bit-identical to itself on a fresh context.

    The second rig receives the first one's block: ctx_alloc hands a cached block of B bytes to a request of R bytes when
    R <= B <= R + R / 4 + 4096.  tests/cpp/test_ws_layouts.cpp (`general 1200 2041`, `general 1100 1865`: slots and observation
    frames of the two rigs) gives B = 10 847 232 (10 855 424 with the sorted list of the first rig's 2 041 merged frames) and
    R = 9 945 600; the window ends at 12 436 096.  No other request of the second rig fits that block (its inputs are 3 MB, its
    mode-E outputs 2.5 and 37 MB)."""
    ext = np.array([[0.0] * 6, [0.3, -0.25, 0.2, -0.1, 0.02, 0.01]])
    second = synth.make_rig(1100, ["eucm", "eucm"], ext, seed=0x5C5, drop_frac=0.15)
    shared, fresh_ctx = Context(0), Context(0)
    try:
        _run_solve(shared, _case("rig_schurq"), (GN,))
        _bits_equal(_product_run(shared, second), _product_run(fresh_ctx, second), where="1 100 slots after 1 200: ")
    finally:
        fresh_ctx.close()
        shared.close()
