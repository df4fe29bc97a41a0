"""GPU: the two small dense solves at the end of every step - k_solve (all three paths: rows in registers to K = 32, the LDS loop
to 63, two wavefronts with a run-time row stride from 64; the prefetch form to K = 24; the strided copy of the parameter sets),
head_wave in k_head (chol_solve_reg<4..9>) and k_backsub - on the named systems of tests/camera_solve_cases.py, against the mpmath
reference of tests/camera_solve_ref.py.

The systems go in through ccal_test_camera_solve and ccal_test_backsub, entry points of the second library only
(csrc/ccal_legacy_test_hooks.hip): the kernels as they are, one launch per case, on a state as launch_state_eval leaves it with the
case's `cur`.  Every in / out array carries the NaN pattern of test_gpu_eval_forms in front, behind and in its unused tail.

EXACT, no tolerance: dc == 0 on fixed columns and their candidates are the current values bit for bit; every free candidate is
fl(x + dc) of the device's OWN dc, clamped, and mirrored into dst2; a candidate the reference says is clamped sits on its bound; every
parameter that is no column's is copied from the current set; the current set, the guards and the tails are untouched;
lambda_solve == lambda; two runs give the same bits; a system that is not positive definite is reported (flags[1] / cam_failed /
done), with dc == 0, mc_cam == 0 and no NaN in the candidate set; a slot with R[0] == 0 keeps its pose bits.

ACCURACY: the device's error in dc (camera_solve_ref.dc_error: scaled by sqrt(S_ii)), mc_cam, dp and mc_slot (relative), per (form,
family, K) over the cell's seeds, against 16 x max(yardstick's worst error over the same seeds, K 2^-52).  The yardstick is the same
algorithm in f64 in another operation order, with division where the device multiplies by a <= 2-ulp reciprocal square root: small
constant factors; a wrong index, mask, stride or damping term costs orders of magnitude.  The floor is under the YARDSTICK: where its
few roundings happen to cancel (mc at K = 1 is three operations) its error says nothing about an algorithm whose bound is K u.
Each test prints one line per family: the worst ratio device / max(yardstick, floor) and the K it is at.

In the stiff family (condition 1e6 .. 1e8) the yardstick is the worst of its four operation orders (camera_solve_ref.ORDERS): the error of
one order is a single draw of (rounding noise along the weakest direction) / (smallest eigenvalue), and with one order 2 of 254 stiff cells
came out at 23 and 19 (mc at K = 66 and 103) although the device's error lay inside the span of the four orders; margin and floor unchanged.

CPU time of the reference for the whole file: about 28 s single-threaded (measured; seeds are thinned above K = 40 to stay there)."""
import ctypes as C

import numpy as np
import pytest

import camera_solve_cases as cases
import camera_solve_ref as ref
from camera_intrinsic_calibration_rs_amd import _ffi

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
GUARD, TAIL = 64, 8
PATTERN = np.uint64(0x7FF8C0DEC0DE0BAD)                 # tests/test_gpu_eval_forms.py: a quiet NaN no computation produces
FORM = {"k_solve": 0, "k_head": 1}
MARGIN = 16.0
DONE_NOT_PD = _ffi.ERR_NOT_PD + 1


def _fn_solve(ctx):
    fn = ctx.lib.ccal_test_camera_solve                         # not in _ffi.SYMBOLS: the second library's own
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp,
                   C.c_double, C.c_double, C.c_double, C.c_int, _dp, _dp]
    return fn


def _fn_backsub(ctx):
    fn = ctx.lib.ccal_test_backsub
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_int, _dp]
    return fn


def _buf(n, payload=None, tail=0):
    """[guard | n (+ tail) | guard] of the pattern, `payload` in front of the tail"""
    b = np.full(2 * GUARD + n + tail, PATTERN, dtype=np.uint64)
    if payload is not None:
        b[GUARD:GUARD + n] = np.ascontiguousarray(payload, dtype=np.float64).view(np.uint64)
    return b


def _p(b):
    return b.ctypes.data_as(_dp)


def _run_solve(ctx, case, decoy=False):
    """one launch: the four parameter buffers, dc and the state as uint64, guards included"""
    cand_i = 777.0 + np.arange(case.n_intr) if decoy else None
    cand_e = 555.0 + np.arange(case.n_extr) if decoy else None
    sets = [[_buf(case.n_intr, case.intr, TAIL), _buf(case.n_extr, case.extr, TAIL)],
            [_buf(case.n_intr, cand_i, TAIL), _buf(case.n_extr, cand_e, TAIL)]]
    if case.cur:
        sets.reverse()
    sent = [[a.copy() for a in s] for s in sets]
    dc, state = _buf(ref.KMAX), np.full(8, PATTERN, dtype=np.uint64)
    red, cols = np.ascontiguousarray(case.red), np.ascontiguousarray(case.cols)
    rc = _fn_solve(ctx)(ctx.handle, FORM[case.form], case.K, _p(red), cols.ctypes.data, cols.dtype.itemsize, case.n_intr, case.n_extr, GUARD,
                        TAIL, _p(sets[0][0]), _p(sets[1][0]), _p(sets[0][1]), _p(sets[1][1]), case.lam, case.min_diag, case.max_diag,
                        case.cur, _p(dc), _p(state))
    assert rc == _ffi.OK, (case.name, rc, ctx.last_error())
    return {"sets": sets, "sent": sent, "dc": dc, "state": state}


def _state(out):
    s = out["state"].view(np.float64)
    return dict(mc_cam=s[0], lambda_solve=s[1], done=s[2], cam_failed=s[3], cur=s[4], first=s[5], flag=s[6], scal_mc=s[7])


def _same_bits(a, b):
    return all((x == y).all() for x, y in zip(a["sets"][0] + a["sets"][1] + [a["dc"], a["state"]],
                                              b["sets"][0] + b["sets"][1] + [b["dc"], b["state"]]))


def _check_frame(case, out):
    """guards, tails and the current set; returns (current, candidate) payloads as [intr, extr] of uint64"""
    name = case.name
    for s in (0, 1):
        for a, n in zip(out["sets"][s], (case.n_intr, case.n_extr)):
            assert (a[:GUARD] == PATTERN).all() and (a[GUARD + n:] == PATTERN).all(), (name, "guard or tail of a parameter set", s)
    dc = out["dc"]
    assert (dc[:GUARD] == PATTERN).all() and (dc[GUARD + case.K:] == PATTERN).all(), (name, "guard or tail of dc")
    cur = case.cur
    for a, b in zip(out["sets"][cur], out["sent"][cur]):
        assert (a == b).all(), (name, "the current set was written")
    pay = lambda s: [a[GUARD:GUARD + n] for a, n in zip(out["sets"][s], (case.n_intr, case.n_extr))]
    return pay(cur), pay(cur ^ 1)


def _check_solved(case, out, tr):
    """the exact claims of a case that solves; returns (dc, mc_cam) of the device"""
    name, K, cols = case.name, case.K, case.cols
    cur_p, cand_p = _check_frame(case, out)
    st = _state(out)
    assert st["done"] == 0 and st["cam_failed"] == 0 and st["cur"] == case.cur and st["first"] == 0, (name, st)
    assert st["lambda_solve"] == case.lam, (name, st)
    if case.form == "k_solve":
        assert st["flag"] == 0 and np.float64(st["scal_mc"]).view(np.uint64) == np.float64(st["mc_cam"]).view(np.uint64), (name, st)
    dc = out["dc"][GUARD:GUARD + K].view(np.float64)
    assert np.isfinite(dc).all() and np.isfinite(st["mc_cam"]), (name, dc, st)
    want = [a.copy() for a in cur_p]                            # the candidate set: the current one ...
    for i in range(K):
        e = int(cols["is_extr"][i])
        if cols["fixed"][i]:
            assert dc[i] == 0.0, (name, i, dc[i])
            continue
        x = cur_p[e][cols["dst"][i]:cols["dst"][i] + 1].view(np.float64)[0]
        v = x + dc[i]                                           # ... with fl(x + dc) of the device's own step, clamped
        if cols["has_bound"][i]:
            v = min(max(v, cols["lo"][i]), cols["hi"][i])
            c = tr["clamped"][i]
            if c:
                assert v == (cols["hi"][i] if c > 0 else cols["lo"][i]), (name, i, "the reference clamps this column", v)
            else:
                assert cols["lo"][i] < v < cols["hi"][i], (name, i, "the reference leaves this column inside", v)
        want[e][cols["dst"][i]] = np.float64(v).view(np.uint64)
        if cols["dst2"][i] >= 0:
            want[e][cols["dst2"][i]] = np.float64(v).view(np.uint64)
    for e in (0, 1):
        bad = np.nonzero(cand_p[e] != want[e])[0]
        assert bad.size == 0, (name, "extr" if e else "intr", bad.tolist(), cand_p[e][bad].view(np.float64), want[e][bad].view(np.float64))
    return dc, float(st["mc_cam"])


_TRUTH: dict = {}


def _truth(case):
    if case.name not in _TRUTH:
        tr = ref.truth(case)
        ys = [ref.yardstick(case, o) for o in range(ref.ORDERS if case.family == "stiff" else 1)]
        _TRUTH[case.name] = (tr, max(ref.dc_error(y["dc"], tr) for y in ys), max(ref.rel_error(y["mc"], tr["mc"]) for y in ys))
    return _TRUTH[case.name]


def _cells(ctx, cells, label=None):
    """cells: (K, [cases]); runs every case twice, checks the exact claims, returns the worst ratios and the cells over the margin"""
    worst = {"dc": (0.0, None), "mc": (0.0, None)}
    over = []
    for K, cs in cells:
        floor = K * 2.0 ** -52
        dev, yard = {"dc": 0.0, "mc": 0.0}, {"dc": 0.0, "mc": 0.0}
        for case in cs:
            tr, y_dc, y_mc = _truth(case)
            out = _run_solve(ctx, case)
            assert _same_bits(out, _run_solve(ctx, case)), (case.name, "two runs differ")
            dc, mc = _check_solved(case, out, tr)
            dev["dc"], dev["mc"] = max(dev["dc"], ref.dc_error(dc, tr)), max(dev["mc"], ref.rel_error(mc, tr["mc"]))
            yard["dc"], yard["mc"] = max(yard["dc"], y_dc), max(yard["mc"], y_mc)
        for q in ("dc", "mc"):
            ratio = dev[q] / max(yard[q], floor)
            if ratio >= worst[q][0]:
                worst[q] = (ratio, K)
            if ratio > MARGIN:
                over.append((q, cs[0].name, dev[q], yard[q]))
    if label:
        print(f"{label}: {sum(len(c) for _, c in cells)} cases  worst dc ratio {worst['dc'][0]:.3f} at K = {worst['dc'][1]}  "
              f"worst mc ratio {worst['mc'][0]:.3f} at K = {worst['mc'][1]}  (margin {MARGIN:g})")
    return worst, over


def _steps(ratios):
    """the ratio on either side of the sizes where k_solve changes its path"""
    return "  ".join(f"{a}/{b}: {ratios.get(a, 0):.2f}/{ratios.get(b, 0):.2f}" for a, b in ((24, 25), (32, 33), (63, 64)))


@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("form", list(cases.SOLVE_SIZES))
def test_family_against_the_reference(dev_ctx, form, family):
    per_k, per_k_mc, over, n = {}, {}, [], 0
    for K in cases.SOLVE_SIZES[form]:
        cs = cases.cell(form, family, K)
        w, o = _cells(dev_ctx, [(K, cs)])
        per_k[K], per_k_mc[K] = w["dc"][0], w["mc"][0]
        over += o
        n += len(cs)
    peak, peak_mc = max(per_k, key=per_k.get), max(per_k_mc, key=per_k_mc.get)
    print(f"{form} {family}: {n} cases  worst dc ratio {per_k[peak]:.3f} at K = {peak}  worst mc ratio {per_k_mc[peak_mc]:.3f} at K = "
          f"{peak_mc}  (margin {MARGIN:g})" + (f"  dc ratio across the path changes {_steps(per_k)}" if form == "k_solve" else ""))
    assert not over, over


def test_layouts_against_the_reference(dev_ctx):
    """the product's parameter layouts for 2 .. 8 cameras and n_intr = 70 at K = 40: the strided copy of the sets"""
    lay = cases.layout_cases()
    strided = [c for c in lay if "strided" in c.name]
    assert len(strided) == 2 and all(c.n_intr > 64 and c.K < 64 for c in strided)
    cells = {}
    for c in lay:
        cells.setdefault((c.K, "strided" in c.name), []).append(c)
    w, over = _cells(dev_ctx, [(k[0], cs) for k, cs in sorted(cells.items())], "k_solve layout")
    assert not over, over


@pytest.mark.parametrize("form", list(cases.SOLVE_SIZES))
def test_not_positive_definite_is_reported(dev_ctx, form):
    n = 0
    for K in cases.SOLVE_SIZES[form]:
        for case in cases.not_pd_cases(form, K):
            out = _run_solve(dev_ctx, case, decoy=True)
            assert _same_bits(out, _run_solve(dev_ctx, case, decoy=True)), (case.name, "two runs differ")
            cur_p, cand_p = _check_frame(case, out)
            st, lm = _state(out), case.claims["lm"]
            dc = out["dc"][GUARD:GUARD + K].view(np.float64)
            assert (dc == 0.0).all(), (case.name, dc)
            assert st["mc_cam"] == 0.0 and st["lambda_solve"] == case.lam and st["cur"] == case.cur, (case.name, st)
            if form == "k_solve":
                assert st["flag"] == 1, (case.name, st)
            assert st["cam_failed"] == (1 if lm else 0) and st["done"] == (0 if lm else DONE_NOT_PD), (case.name, st)
            for e in (0, 1):
                assert not np.isnan(cand_p[e].view(np.float64)).any(), (case.name, "NaN in the candidate set")
                if form == "k_solve" or lm:                    # the candidate is the current point: LM rejects it at the next decision
                    assert (cand_p[e] == cur_p[e]).all(), (case.name, "the candidate set is not the current one")
                else:                                           # k_head under Gauss-Newton: the solve has ended, no candidate is written
                    assert (cand_p[e] == out["sent"][case.cur ^ 1][e][GUARD:GUARD + len(cand_p[e])]).all(), case.name
            n += 1
    print(f"{form} not_pd: {n} cases reported")


def _run_backsub(ctx, case):
    n = case.n_slots
    sets = [_buf(6 * n, case.poses.ravel()), _buf(6 * n)]
    if case.cur:
        sets.reverse()
    sent = [a.copy() for a in sets]
    mc = _buf(n)
    pf, dc = np.ascontiguousarray(case.pf), np.ascontiguousarray(case.dc)
    rc = _fn_backsub(ctx)(ctx.handle, n, case.K, _p(pf), _p(dc), GUARD, _p(sets[0]), _p(sets[1]), case.lam, case.min_diag, case.max_diag,
                          case.cur, _p(mc))
    assert rc == _ffi.OK, (case.name, rc, ctx.last_error())
    return {"sets": sets, "sent": sent, "mc": mc}


def test_backsub_against_the_reference(dev_ctx):
    over = []
    for K in cases.BACKSUB_K:
        worst = {"dp": (0.0, None), "mc": (0.0, None)}
        for n in cases.BACKSUB_SLOTS:
            dev, yard = {"dp": 0.0, "mc": 0.0}, {"dp": 0.0, "mc": 0.0}
            for case in (c for c in cases.backsub_cases() if c.K == K and c.n_slots == n):
                out = _run_backsub(dev_ctx, case)
                again = _run_backsub(dev_ctx, case)
                assert all((a == b).all() for a, b in zip(out["sets"] + [out["mc"]], again["sets"] + [again["mc"]])), (case.name, "two runs differ")
                for a in out["sets"] + [out["mc"]]:
                    assert (a[:GUARD] == PATTERN).all() and (a[-GUARD:] == PATTERN).all(), (case.name, "guard")
                assert (out["sets"][case.cur] == out["sent"][case.cur]).all(), (case.name, "the current poses were written")
                cur = out["sets"][case.cur][GUARD:-GUARD].reshape(n, 6)
                cand = out["sets"][case.cur ^ 1][GUARD:-GUARD].reshape(n, 6)
                mc = out["mc"][GUARD:-GUARD].view(np.float64)
                tr, ya = ref.backsub_truth(case), ref.backsub_yardstick(case)
                assert tr[case.claims["unobserved"]] is None if "unobserved" in case.claims else True
                for s in range(n):
                    if tr[s] is None:                           # R[0] == 0: the slot keeps its pose bits, mc 0
                        assert (cand[s] == cur[s]).all() and mc[s] == 0.0, (case.name, s)
                        continue
                    x, xc = cur[s].view(np.float64), cand[s].view(np.float64)
                    assert np.isfinite(xc).all() and np.isfinite(mc[s]), (case.name, s)
                    dev["dp"] = max(dev["dp"], ref.pose_error(xc, x, tr[s][0]))
                    dev["mc"] = max(dev["mc"], ref.rel_error(mc[s], tr[s][1]))
                    yard["dp"] = max(yard["dp"], ref.pose_error(ya[s][0], x, tr[s][0]))
                    yard["mc"] = max(yard["mc"], ref.rel_error(ya[s][1], tr[s][1]))
            floor = K * 2.0 ** -52
            for q in ("dp", "mc"):
                ratio = dev[q] / max(yard[q], floor)
                if ratio > worst[q][0]:
                    worst[q] = (ratio, n)
                if ratio > MARGIN:
                    over.append((q, K, n, dev[q], yard[q]))
        print(f"backsub K {K}: worst dp ratio {worst['dp'][0]:.3f} at n_slots = {worst['dp'][1]}  worst mc ratio {worst['mc'][0]:.3f} "
              f"at n_slots = {worst['mc'][1]}  (margin {MARGIN:g})")
    assert not over, over


def test_bad_arguments_are_refused(dev_ctx):
    """nothing is launched, nothing is written: K, n_intr, n_extr, dst, dst2, n_slots - and form, cur, the record size, the guard"""
    case = cases.solve_case("k_solve", "scaled", 6, 0)
    head = cases.solve_case("k_head", "scaled", 6, 0)
    fn = _fn_solve(dev_ctx)

    def call(c, **kw):
        a = dict(form=FORM[c.form], K=c.K, col_bytes=c.cols.dtype.itemsize, n_intr=c.n_intr, n_extr=c.n_extr, guard=GUARD, tail=TAIL,
                 lam=c.lam, cur=c.cur, cols=c.cols, ctx=dev_ctx.handle)
        a.update(kw)
        bufs = [_buf(max(c.n_intr, 0)+ 16, None, TAIL) for _ in range(4)] + [_buf(ref.KMAX), np.full(8, PATTERN, dtype=np.uint64)]
        sent = [b.copy() for b in bufs]
        red, cols = np.ascontiguousarray(c.red), np.ascontiguousarray(a["cols"])
        rc = fn(a["ctx"], a["form"], a["K"], _p(red), cols.ctypes.data, a["col_bytes"], a["n_intr"], a["n_extr"], a["guard"], a["tail"],
                _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(bufs[3]), a["lam"], c.min_diag, c.max_diag, a["cur"], _p(bufs[4]), _p(bufs[5]))
        assert all((x == y).all() for x, y in zip(bufs, sent)), kw
        return rc

    def cols_with(c, field, i, v):
        cols = c.cols.copy()
        cols[field][i] = v
        return cols

    e_col = int(np.nonzero(case.cols["is_extr"])[0][0])
    i_col = int(np.nonzero(case.cols["is_extr"] == 0)[0][0])
    bad = [dict(K=0), dict(K=-1), dict(K=ref.KMAX), dict(K=1 << 20), dict(form=2), dict(form=-1), dict(cur=2), dict(cur=-1),
           dict(col_bytes=36), dict(n_intr=0), dict(n_intr=-5), dict(n_intr=1 << 20), dict(n_extr=-1), dict(n_extr=1 << 20),
           dict(guard=-1), dict(tail=-1), dict(guard=1 << 20), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")),
           dict(cols=cols_with(case, "dst", i_col, case.n_intr)), dict(cols=cols_with(case, "dst", i_col, -1)),
           dict(cols=cols_with(case, "dst", e_col, case.n_extr)), dict(cols=cols_with(case, "dst2", i_col, case.n_intr)),
           dict(cols=cols_with(case, "dst2", i_col, -2)), dict(cols=cols_with(case, "is_extr", i_col, 2)),
           dict(n_intr=int(case.cols["dst"][i_col])), dict(n_extr=int(case.cols["dst"][e_col]))]
    for kw in bad:
        assert call(case, **kw) == _ffi.ERR_INVALID_ARG, kw
        assert "ccal_test_camera_solve" in dev_ctx.last_error()
    for kw in (dict(K=3), dict(K=10), dict(n_intr=9), dict(n_intr=11), dict(n_extr=6), dict(cols=cols_with(head, "dst", 0, ref.PMAX)),
               dict(cols=cols_with(head, "is_extr", 0, 1))):
        assert call(head, **kw) == _ffi.ERR_INVALID_ARG, kw
    assert call(case, ctx=None) == _ffi.ERR_INVALID_ARG
    bs = next(c for c in cases.backsub_cases() if c.K == 4 and c.n_slots == 15)
    fb = _fn_backsub(dev_ctx)
    for kw in (dict(n=0), dict(n=-1), dict(n=1 << 20), dict(K=0), dict(K=ref.KMAX), dict(guard=-1), dict(cur=2), dict(lam=-1.0)):
        a = dict(n=bs.n_slots, K=bs.K, guard=GUARD, cur=bs.cur, lam=bs.lam)
        a.update(kw)
        bufs = [_buf(6 * bs.n_slots), _buf(6 * bs.n_slots), _buf(bs.n_slots)]
        sent = [b.copy() for b in bufs]
        pf, dc = np.ascontiguousarray(bs.pf), np.ascontiguousarray(bs.dc)
        rc = fb(dev_ctx.handle, a["n"], a["K"], _p(pf), _p(dc), a["guard"], _p(bufs[0]), _p(bufs[1]), a["lam"], bs.min_diag, bs.max_diag,
                a["cur"], _p(bufs[2]))
        assert rc == _ffi.ERR_INVALID_ARG and "ccal_test_backsub" in dev_ctx.last_error(), kw
        assert all((x == y).all() for x, y in zip(bufs, sent)), kw
    _check_solved(case, _run_solve(dev_ctx, case), _truth(case)[0])      # and a good call still goes through
