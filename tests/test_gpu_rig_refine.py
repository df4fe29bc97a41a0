"""GPU: board poses of a rig refined under fixed intrinsics and extrinsics (ccal_refine_rig_poses_batch, k_rig_pose_refine in
csrc/ccal_kernels_rig_refine.hip) - against ground truth on exact data, against the single-camera call for one camera with and
without an extrinsic, against the numpy yardstick tests/rig_refine_ref.py on noisy data with outliers, for first-order optimality with
a gradient the kernel's Jacobian has no part in, on the shapes where the segment loop, the lane loop and the four-wavefront workgroup
can go wrong, for empty and invalid rows, independence of the batch and determinism, the argument checks, the api level and on
poisoned memory."""
import ctypes as C

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth

import rig_refine_cases as cases
import rig_refine_ref as ref
import test_gpu_refine as single

pytestmark = pytest.mark.gpu

OK_ = _ffi.OK
_tight, _TO_ROUNDING = single._tight, single._TO_ROUNDING

# The yardstick's own figures on exactly the slots of these tests, measured in numpy and recorded in rig_refine_cases.py
# (EXPERIMENTS.md; tests/test_rig_refine_cpu.py holds the record to what rig_refine_cases.measure() gives).  Asserted at 10 x them.
# Exact data, yardstick against ground truth from the same perturbed start, each rig by its own figures: rig A rotation-matrix
# entries 1.124e-15, translation 2.220e-16 m (a slot that only KB4 sees), rig B 8.327e-16 and 4.441e-16 m (OPENCV5 + EUCM).
EXACT_DIFF_R = {k: 10 * v for k, v in cases.YARD_EXACT_R.items()}
EXACT_DIFF_T = {k: 10 * v for k, v in cases.YARD_EXACT_T.items()}
# The 24 noisy slots of rig A: the yardstick's runs from the start and from the ground truth differ by 2.380e-10 / 5.777e-11 m.
NOISY_DIFF_R = 10 * cases.YARD_NOISY_R
NOISY_DIFF_T = 10 * cases.YARD_NOISY_T
# The yardstick's own residual gradient on those slots, relative to the gradient at the start: 2.179e-9.
GRAD_REL = 10 * cases.YARD_GRAD_REL
assert max(*EXACT_DIFF_R.values(), *EXACT_DIFF_T.values(), NOISY_DIFF_R, NOISY_DIFF_T, GRAD_REL) <= 1e-6


def _run(ctx, rig, slots, start, opts=None, min_points=4, with_errors=False):
    return ctx.refine_rig_poses_batch(rig[0], rig[1], rig[2], slots, start, 1.0, min_points, opts, with_errors=with_errors)


def _total(slot):
    return sum(len(x) for _, x, _ in slot)


def _inv6(p):
    return api.RvecTvec.from6(p).inverse()


# ---- 1. exact data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_data(gpu_ctx, name):
    rig, slots, start, gt = cases.exact(name)
    poses, status, iters, used, cost0, cost = _run(gpu_ctx, rig, slots, start, _tight())
    dr = cases.dR(poses, gt); dt = float(np.abs(poses[:, 3:] - gt[:, 3:]).max())
    print(f"rig {name}: kernel dR {dr:.2e} dt {dt:.2e}; iters {iters.min()}..{iters.max()} cost0 {cost0.max():.3e} cost {cost.max():.3e}; "
          f"segments per slot {[len(s) for s in slots]}")
    assert (status == OK_).all(), status
    assert (used == [_total(s) for s in slots]).all()
    assert (cost <= cost0).all()
    assert dr <= EXACT_DIFF_R[name], dr
    assert dt <= EXACT_DIFF_T[name], dt


# ---- 2., 3. one camera: the single-camera call, without and with an extrinsic --------------------------------------------------------
def _single_camera_run(ctx):
    sp, m, par, X, U, poses0 = single._noisy_inputs(ctx, "eucm")
    out = ctx.refine_poses_batch(m, par, X, U, poses0, 1.0, 4, _tight(_TO_ROUNDING))
    return m, par, X, U, poses0, out


def test_one_camera_equals_the_single_camera_call(gpu_ctx):
    m, par, X, U, poses0, one = _single_camera_run(gpu_ctx)
    rig = ([m], [par], np.zeros((1, 6)))
    out = _run(gpu_ctx, rig, [[(0, X[f], U[f])] for f in range(40)], poses0, _tight(_TO_ROUNDING))
    dr = cases.dR(out[0], one[0]); dt = float(np.abs(out[0][:, 3:] - one[0][:, 3:]).max())
    dc = float(np.abs(out[5] / one[5] - 1).max()); dc0 = float(np.abs(out[4] / one[4] - 1).max())
    print(f"rig of one camera - single-camera call: dR {dr:.2e} dt {dt:.2e} cost {dc:.2e} cost0 {dc0:.2e}; iters {out[2].tolist()} / {one[2].tolist()}")
    assert out[1].tolist() == one[1].tolist() and (out[1] == OK_).all()
    assert out[3].tolist() == one[3].tolist()
    assert dr <= single.NOISY_DIFF_R and dt <= single.NOISY_DIFF_T, (dr, dt)
    assert dc <= 1e-9 and dc0 <= 1e-9, (dc, dc0)


def test_the_extrinsic_is_applied(gpu_ctx):
    """The same frames as a rig of one camera that sits at E = T_c_0 (0.9 rad, 0.3 m) from the rig frame: T_0_b = E^-1 o T_c_b."""
    m, par, X, U, poses0, one = _single_camera_run(gpu_ctx)
    E = np.array([0.9 * 2 / 3, -0.9 * 2 / 3, 0.9 / 3, 0.3 * 2 / 3, 0.3 / 3, -0.3 * 2 / 3])
    Ei = _inv6(E)
    rig = ([m], [par], E[None, :])
    start = np.stack([Ei.compose(api.RvecTvec.from6(p)).as6() for p in poses0])
    out = _run(gpu_ctx, rig, [[(0, X[f], U[f])] for f in range(40)], start, _tight(_TO_ROUNDING))
    want = np.stack([Ei.compose(api.RvecTvec.from6(p)).as6() for p in one[0]])
    dr = cases.dR(out[0], want); dt = float(np.abs(out[0][:, 3:] - want[:, 3:]).max())
    dc = float(np.abs(out[5] / one[5] - 1).max())
    print(f"E^-1 o single-camera result: dR {dr:.2e} dt {dt:.2e} cost {dc:.2e}; iters {out[2].tolist()}")
    assert out[1].tolist() == one[1].tolist() and out[3].tolist() == one[3].tolist()
    assert dr <= single.NOISY_DIFF_R and dt <= single.NOISY_DIFF_T, (dr, dt)
    assert dc <= 1e-9, dc


# ---- 4. noisy data with outliers, against the yardstick --------------------------------------------------------------------------
def test_noisy_against_the_yardstick(gpu_ctx):
    rig, slots, start, gt = cases.noisy()
    poses, status, iters, used, cost0, cost = _run(gpu_ctx, rig, slots, start, _tight(_TO_ROUNDING))
    y = cases.yardstick_noisy()
    own_r = max(cases.dR(r[2], r[3]) for r in y); own_t = max(np.abs(r[2][3:] - r[3][3:]).max() for r in y)
    worst_r = max(cases.dR(poses[s], y[s][0]) for s in range(24))
    worst_t = max(np.abs(poses[s, 3:] - y[s][0][3:]).max() for s in range(24))
    worst_c = max(cost[s] / y[s][1] - 1 for s in range(24))
    print(f"rig A: kernel - yardstick dR {worst_r:.2e} dt {worst_t:.2e}, cost / yardstick cost - 1 <= {worst_c:.2e}; "
          f"yardstick's two starts differ by dR {own_r:.2e} dt {own_t:.2e}; iters {iters.min()}..{iters.max()}")
    assert (status == OK_).all(), status                 # no slot is left out
    assert (used == [_total(s) for s in slots]).all()
    assert worst_r <= NOISY_DIFF_R, worst_r
    assert worst_t <= NOISY_DIFF_T, worst_t
    assert worst_c <= 1e-9, worst_c


# ---- 5. first-order optimality, independent of the kernel's Jacobian ---------------------------------------------------------------
def test_first_order_optimality(gpu_ctx):
    rig, slots, start, gt = cases.noisy()
    poses, status, *_ = _run(gpu_ctx, rig, slots, start, _tight(_TO_ROUNDING))
    y = cases.yardstick_noisy()
    worst = worst_ref = 0.0
    for s in range(24):
        g0 = np.linalg.norm(ref.gradient(rig, slots[s], start[s], 1.0))
        worst = max(worst, np.linalg.norm(ref.gradient(rig, slots[s], poses[s], 1.0)) / g0)
        worst_ref = max(worst_ref, np.linalg.norm(ref.gradient(rig, slots[s], y[s][0], 1.0)) / g0)
    print(f"rig A: |grad| / |grad at the start| kernel {worst:.2e}, yardstick {worst_ref:.2e}")
    assert worst <= GRAD_REL, worst


# ---- 6. shapes -------------------------------------------------------------------------------------------------------------------
# (camera, corners) of every segment: all the segment sizes around the 64 lanes, slots of 1, 2 and 3 segments, an empty segment
# between two full ones, and a slot that only both cameras together can place (2 + 2 points)
SHAPES = [[(0, 4)], [(1, 5)], [(0, 63), (2, 64)], [(1, 65), (2, 128)], [(0, 129), (1, 300), (2, 4)], [(0, 64), (1, 0), (2, 65)],
          [(0, 2), (2, 2)], [(2, 300)], [(0, 5), (1, 63), (2, 129)]]
_SHAPE_CACHE = {}


def _shape_slots():
    """Rig B looking at a 20 x 15 board: per segment the first `count` corners of a random order, projected in f64 at the true
    T_c_0 o T_0_b, 0.1 px noise; the start is 0.008 rad / 0.004 m off."""
    if "v" in _SHAPE_CACHE:
        return _SHAPE_CACHE["v"]
    models, extr = cases.RIGS["B"]
    ms = [synth.MODEL_NAMES[m] for m in models]
    extr = np.asarray(extr, dtype=np.float64)
    rig = (ms, [np.asarray(synth.GT_PARAMS[m], dtype=np.float64) for m in ms], extr)
    bx, by = np.meshgrid(np.arange(20) * 0.035, -np.arange(15) * 0.035)
    board = np.stack([bx.ravel(), by.ravel(), np.zeros(300)], axis=1).astype(np.float32).astype(np.float64)
    R, t = synth._gen_poses(0x5A4E, len(SHAPES), (0.75, 1.3), 0.12)
    gt = np.concatenate([synth.rotmat_to_rvec(R), t], axis=-1)
    slots = []
    for s, segs in enumerate(SHAPES):
        out = []
        for j, (cam, count) in enumerate(segs):
            order = np.argsort(synth.uniform01(0x5A4E + 31 * s + j, 300, stream=3))[:count]
            X = board[order]
            pc = (X @ R[s].T + t[s]) @ synth.rodrigues(extr[cam, :3]).T + extr[cam, 3:]
            uv = synth.project(ms[cam], rig[1][cam], pc) + 0.1 * synth.normal01(0x5A4E + 31 * s + j, 2 * count, stream=4).reshape(count, 2)
            assert (pc[:, 2] > 0.05).all()
            out.append((cam, X, uv))
        slots.append(out)
    dp = 2.0 * synth.uniform01(0x5A4E, len(SHAPES) * 6, stream=8).reshape(-1, 6) - 1.0
    start = gt + dp * np.array([0.008, 0.008, 0.008, 0.004, 0.004, 0.004])
    alone_ref = [ref.refine(rig, slots[s], start[s], 1.0) for s in range(len(SHAPES))]      # the yardstick from the same start
    _SHAPE_CACHE["v"] = (rig, slots, start, gt, alone_ref)
    return _SHAPE_CACHE["v"]


@pytest.mark.parametrize("n_slots", [1, 3, 4, 5, 9])
def test_shapes_and_batch_sizes(gpu_ctx, n_slots):
    rig, slots, start, gt, yard = _shape_slots()
    alone = [_run(gpu_ctx, rig, [slots[s]], start[s:s + 1], _tight(), with_errors=True) for s in range(9)]
    # the batch takes the slots from the far end, so that every shape appears in some batch size
    sel = list(range(9))[::-1][:n_slots] if n_slots < 9 else list(range(9))
    out = _run(gpu_ctx, rig, [slots[s] for s in sel], start[sel], _tight(), with_errors=True)
    for k, s in enumerate(sel):
        for i in range(6):
            assert np.asarray(out[i][k]).tobytes() == np.asarray(alone[s][i][0]).tobytes(), (s, i)
        assert out[6][k].tobytes() == alone[s][6][0].tobytes()
        assert out[1][k] == OK_ and out[3][k] == _total(slots[s]), (s, out[1][k], out[3][k])
        # the refined pose is the minimum of the numpy cost: no lower cost at the yardstick's result, to rounding
        assert out[5][k] <= yard[s][1] * (1 + 1e-9), (s, out[5][k], yard[s][1])
        assert len(out[6][k]) == _total(slots[s])
        np.testing.assert_allclose(out[6][k], ref.pixel_errors(rig, slots[s], out[0][k]), rtol=0, atol=1e-9)


def test_two_cameras_place_a_slot_that_neither_could_alone(gpu_ctx):
    rig, slots, start, gt, yard = _shape_slots()
    s = SHAPES.index([(0, 2), (2, 2)])
    out = _run(gpu_ctx, rig, [slots[s]], start[s:s + 1], _tight(), min_points=4)
    assert out[1][0] == OK_ and out[3][0] == 4
    assert out[5][0] <= yard[s][1] * (1 + 1e-9), (out[5][0], yard[s][1])
    for seg in slots[s]:                                  # neither camera alone
        o = _run(gpu_ctx, rig, [[seg]], start[s:s + 1], _tight(), min_points=4)
        assert o[1][0] == _ffi.NO_RESULT and o[0][0].tobytes() == start[s].tobytes()


# ---- 7. empty and invalid rows ---------------------------------------------------------------------------------------------------
def test_empty_slots_nan_rows_and_too_few_points(gpu_ctx):
    rig, slots, start, gt, _ = _shape_slots()
    start = start.copy()
    # 0: full; 1: no segments; 2: NaN / inf rows in two segments; 3: below min_points (5 + 0 + ... < 7); 4: full
    s2 = [(c, x.copy(), u.copy()) for c, x, u in slots[4]]
    s2[0][2][[0, 70, 128], 0] = np.nan; s2[1][1][[5, 299], 2] = np.inf; s2[2][2][3, 1] = -np.inf
    batch = [slots[3], [], s2, slots[1], slots[8]]
    st = start[[3, 0, 4, 1, 8]]
    poses, status, iters, used, cost0, cost, err = _run(gpu_ctx, rig, batch, st, _tight(), min_points=7, with_errors=True)
    assert status.tolist() == [OK_, _ffi.NO_RESULT, OK_, _ffi.NO_RESULT, OK_], status
    assert used.tolist() == [193, 0, 433 - 6, 0, 197]
    for k in (1, 3):                                      # no segments / below min_points: untouched
        assert poses[k].tobytes() == st[k].tobytes() and iters[k] == 0 and cost0[k] == 0.0 and cost[k] == 0.0
        assert np.isnan(err[k]).all()
    assert len(err[1]) == 0 and len(err[3]) == 5
    bad = np.zeros(433, dtype=bool); bad[[0, 70, 128, 129 + 5, 129 + 299, 429 + 3]] = True
    assert np.isnan(err[2][bad]).all() and np.isfinite(err[2][~bad]).all()
    # the rows that are not finite are left out: the same result as the slot without them
    keep = [np.ones(129, dtype=bool), np.ones(300, dtype=bool), np.ones(4, dtype=bool)]
    keep[0][[0, 70, 128]] = False; keep[1][[5, 299]] = False; keep[2][3] = False
    clean = [(c, x[k], u[k]) for (c, x, u), k in zip(slots[4], keep)]
    o = _run(gpu_ctx, rig, [clean], st[2:3], _tight(), min_points=7)
    np.testing.assert_allclose(poses[2], o[0][0], rtol=0, atol=1e-12)
    # a start that is not finite: no result either
    nf = st.copy(); nf[0, 2] = np.nan
    o = _run(gpu_ctx, rig, batch, nf, _tight(), min_points=7, with_errors=True)
    assert o[1][0] == _ffi.NO_RESULT and o[0][0].tobytes() == nf[0].tobytes() and np.isnan(o[6][0]).all()
    assert o[1][4] == OK_ and o[0][4].tobytes() == poses[4].tobytes()
    # n_slots == 0
    o = _run(gpu_ctx, rig, [], np.zeros((0, 6)), with_errors=True)
    assert all(len(v) == 0 for v in o)


# ---- 8. independence and determinism -----------------------------------------------------------------------------------------------
def test_independence_and_determinism(gpu_ctx):
    rig, slots, start, gt = cases.noisy()
    slots, start = slots[:9], start[:9].copy()
    probe = (slots[4], start[4:5])
    alone = _run(gpu_ctx, rig, [probe[0]], probe[1], _tight(), with_errors=True)
    for pos in (0, 4, 8):
        sb, pb = list(slots), start.copy()
        sb[pos], pb[pos] = probe[0], probe[1][0]
        out = _run(gpu_ctx, rig, sb, pb, _tight(), with_errors=True)
        for i in range(6):
            assert np.asarray(out[i][pos]).tobytes() == np.asarray(alone[i][0]).tobytes(), (pos, i)
        assert out[6][pos].tobytes() == alone[6][0].tobytes()
    a = _run(gpu_ctx, rig, slots, start, _tight(), with_errors=True)
    b = _run(gpu_ctx, rig, slots, start, _tight(), with_errors=True)
    for i in range(6):
        assert a[i].tobytes() == b[i].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[6], b[6]))
    # a slot that starts 0.4 rad off beside slots that start at the optimum: each stops by its own rule
    at_opt = a[0].copy()
    at_opt[3, :3] += 0.4 / np.sqrt(3.0)
    mixed = _run(gpu_ctx, rig, slots, at_opt, _tight())
    own = [_run(gpu_ctx, rig, [slots[s]], at_opt[s:s + 1], _tight())[2][0] for s in range(9)]
    print("iterations in the batch", mixed[2].tolist(), "alone", own)
    assert mixed[2].tolist() == own
    assert mixed[2][3] > np.delete(mixed[2], 3).max()


# ---- 9. arguments ------------------------------------------------------------------------------------------------------------------
def test_arguments(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
    rig, slots, start, gt, _ = _shape_slots()
    segs = slots[1] + slots[8]                            # slot 0: one segment of 5; slot 1: 5 + 63 + 129
    Xa = np.ascontiguousarray(np.concatenate([x for _, x, _ in segs])); Ua = np.ascontiguousarray(np.concatenate([u for _, _, u in segs]))
    model = np.array(rig[0], dtype=np.int32)
    params = np.zeros((3, synth.PMAX))
    for c, p in enumerate(rig[1]):
        params[c, :len(p)] = p
    extr = np.ascontiguousarray(rig[2])
    so = np.array([0, 1, 4], dtype=np.int64); sc = np.array([1, 0, 1, 2], dtype=np.int32); po = np.array([0, 5, 10, 73, 202], dtype=np.int64)
    first = start[[1, 8]].copy()
    poses = first.copy(); st = np.full(2, -7, dtype=np.int32); it = np.full(2, -7, dtype=np.int32); nu = np.full(2, -7, dtype=np.int32)
    c0 = np.full(2, -7.0); c1 = np.full(2, -7.0); err = np.full(202, -7.0)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    i32 = lambda *v: np.array(v, dtype=np.int32)

    def call(n_cams=3, model=model, params=params, extr=extr, n=2, so=so, sc=sc, po=po, X=Xa, U=Ua, pose=poses, status=st):
        return lib.ccal_refine_rig_poses_batch(h, n_cams, ip(model), dp(params), dp(extr), 1.0, n, lp(so), ip(sc), lp(po), dp(X), dp(U),
                                               4, None, dp(pose), ip(status), ip(it), ip(nu), dp(c0), dp(c1), dp(err))
    bad = _ffi.ERR_INVALID_ARG
    assert call(n_cams=0) == bad and call(n_cams=-1) == bad and call(n_cams=9) == bad
    assert call(model=i32(1, 17, 1)) == bad and call(model=i32(-1, 3, 1)) == bad
    assert call(model=i32(0, api.MODEL_EUCMT, 1)) == _ffi.ERR_UNSUPPORTED
    assert call(sc=i32(1, 0, 3, 2)) == bad and call(sc=i32(1, -1, 1, 2)) == bad
    assert call(n_cams=2) == bad                          # camera 2 of the segments is out of range for two cameras
    assert call(so=i64(1, 1, 4)) == bad and call(so=i64(0, 4, 1)) == bad
    assert call(po=i64(1, 5, 10, 73, 202)) == bad and call(po=i64(0, 5, 10, 9, 202)) == bad
    assert call(po=i64(0, 5, 10, 73, (1 << 24) + 80)) == bad      # more than 2^24 points in a slot
    assert call(n=-1) == bad
    for k in ("model", "params", "extr", "so", "sc", "po", "X", "U", "pose", "status"):
        assert call(**{k: None}) == bad, k
    assert poses.tobytes() == first.tobytes()
    assert (st == -7).all() and (it == -7).all() and (nu == -7).all() and (c0 == -7).all() and (c1 == -7).all() and (err == -7).all()
    assert call() == _ffi.OK and (st == OK_).all() and (err >= 0).all() and nu.tolist() == [5, 197]
    with pytest.raises(api.CcalError):
        api.refine_rig_poses([[None]], [api.GenericModel("eucmt", [1.0] * 8, 512, 512)], [api.RvecTvec.from6(np.zeros(6))])


# ---- 10. the api level ---------------------------------------------------------------------------------------------------------------
def test_api_refine_rig_poses_and_validation_holdout_rig(gpu_ctx):
    models, extr_gt = cases.RIGS["A"]
    sp = synth.make_rig(48, models, extr_gt, seed=1, noise_px=0.1, drop_frac=0.3)
    frames = [api.frames_from_synth(sp, c) for c in range(2)]
    even = [[f if i % 2 == 0 else None for i, f in enumerate(fr)] for fr in frames]
    held = [[f if i % 2 == 1 else None for i, f in enumerate(fr)] for fr in frames]
    P = [synth.MODEL_NPARAMS[int(m)] for m in sp.model]
    cams0 = [api.GenericModel(models[c], sp.intr0[c, :P[c]], 512, 512) for c in range(2)]
    t0 = [api.RvecTvec.from6(sp.extr0[c]) for c in range(2)]
    rt0 = [{i: t0[c].compose(api.RvecTvec.from6(sp.poses0[i])) for i, f in enumerate(even[c]) if f is not None} for c in range(2)]
    fit = api.calib_all_camera_with_extrinsics(cams0, t0, rt0, even, False, 0, False, ctx=gpu_ctx)
    assert fit is not None
    fit_cams, fit_t, _ = fit
    odd_seen = sorted(i for i in range(1, 48, 2) if any(fr[i] is not None for fr in frames))
    n_seen = [sum(fr[i] is not None for fr in frames) for i in range(1, 48, 2)]
    assert set(n_seen) == {0, 1, 2}                       # held-out slots that no camera, one camera and both cameras saw
    start = {i: api.RvecTvec.from6(sp.poses0[i]) for i in range(48)}
    refined = api.refine_rig_poses(held, fit_cams, fit_t, start, ctx=gpu_ctx)
    assert sorted(refined) == odd_seen
    assert sorted(api.refine_rig_poses(held, fit_cams, fit_t, ctx=gpu_ctx)) == odd_seen       # starts from init_frame_poses
    got = api.validation_holdout_rig(fit_cams, fit_t, held, ctx=gpu_ctx)
    own = api.refine_rig_poses(held, fit_cams, fit_t, ctx=gpu_ctx)
    want = [api.validation(c, fit_cams[c], {k: fit_t[c].compose(t) for k, t in own.items()}, held[c], ctx=gpu_ctx) for c in range(2)]
    assert got == want
    # True intrinsics and extrinsics, both sides at the rounding of the objective.  The joint minimum is not either camera's own, so
    # the bound is the yardstick's excess - plus `reach`: the most a median can move when the poses move by the margins that case 4
    # holds the kernel to (sum_k |d e_i / d pose_k| x margin, central differences of the yardstick's errors; about 1e-6 px).
    true_cams = [api.GenericModel(models[c], sp.intr_gt[c, :P[c]], 512, 512) for c in range(2)]
    true_t = [api.RvecTvec.from6(sp.extr_gt[c]) for c in range(2)]
    res = api.validation_holdout_rig(true_cams, true_t, held, ctx=gpu_ctx, opts=_tight(_TO_ROUNDING))
    res_default = api.validation_holdout_rig(true_cams, true_t, held, ctx=gpu_ctx)
    rig = cases.rig_of(sp)
    slots = cases.slots_of(sp)
    yard = {i: ref.solve(rig, slots[i], sp.poses0[i], sp.poses_gt[i], 1.0)[0] for i in odd_seen}
    margin = np.array([NOISY_DIFF_R] * 3 + [NOISY_DIFF_T] * 3)
    for c in range(2):
        mine = [i for i in odd_seen if held[c][i] is not None]
        seg = {i: [s for s in slots[i] if s[0] == c] for i in mine}
        e_y = np.concatenate([ref.pixel_errors(rig, seg[i], yard[i]) for i in mine])
        e_gt = np.concatenate([ref.pixel_errors(rig, seg[i], sp.poses_gt[i]) for i in mine])
        excess = float(np.median(e_y) - np.median(e_gt))
        reach = 0.0
        for i in mine:
            e = ref.pixel_errors(rig, seg[i], ref._stencil(yard[i], 1e-6))               # [12, n]
            reach = max(reach, float((np.abs(e[:6] - e[6:]) / 2e-6 * margin[:, None]).sum(axis=0).max()))
        _, med_gt = api.validation(c, true_cams[c], {i: true_t[c].compose(api.RvecTvec.from6(sp.poses_gt[i])) for i in mine}, held[c], ctx=gpu_ctx)
        print(f"camera {c}: held-out median {res[c][1]:.9f} px (default stop rules {res_default[c][1]:.9f}), at the ground-truth poses "
              f"{med_gt:.9f} px, the yardstick's excess {excess:+.3e} px, reach of case 4's margins {reach:.2e} px; "
              f"held-out excess - yardstick's excess {res[c][1] - med_gt - excess:+.3e} px (default stop rules "
              f"{res_default[c][1] - med_gt - excess:+.3e}); fitted rig {got[c]}")
        assert reach <= 1e-5, reach
        assert res[c][1] - med_gt <= excess + reach, (c, res[c][1], med_gt, excess, reach)


# ---- 11. poisoned memory -----------------------------------------------------------------------------------------------------------
def _run_rig_noisy(ctx):
    rig, slots, start, gt = cases.noisy()
    out = _run(ctx, rig, slots, start, _tight(_TO_ROUNDING), with_errors=True)
    res = {k: out[i] for i, k in enumerate(["poses", "status", "iters", "used", "cost0", "cost"])}
    res["err"] = np.concatenate(out[6])
    return res


def test_poisoned_memory(gpu_ctx):
    """Case 4 on a context of the second library with every block of doubles pre-filled with NaN, in a fresh process, against the
    same run without the hook (the harness of tests/test_gpu_poison.py, imported as it is) and against this process's run."""
    import test_gpu_poison as tp
    res = tp._poisoned_and_clean(_run_rig_noisy)
    assert (res["status"] == OK_).all()
    here = _run_rig_noisy(gpu_ctx)
    for k in here:
        assert np.asarray(here[k]).tobytes() == np.asarray(res[k]).tobytes(), k
