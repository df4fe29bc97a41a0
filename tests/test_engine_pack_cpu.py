"""CPU: what the four batched Context methods (rdh_batch, pnp_batch, refine_poses_batch, refine_rig_poses_batch) hand to the
library and what they make of its answer, through a stub in the library's place: the offsets, the concatenated rows, the padded and
poisoned output arrays, NULL for outputs not asked for, and the slicing of what comes back.  Every expected value is written out
here; the stub copies what the pointers address during the call and fills the outputs with numbers that name their position."""
import ctypes as C

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import _ffi
from camera_intrinsic_calibration_rs_amd.engine import Context

NAN = np.nan


def _rd(ptr, count):
    """A copy of `count` elements behind a ctypes pointer (its dtype is the pointer's), or None for NULL."""
    return None if ptr is None else np.ctypeslib.as_array(ptr, shape=(max(count, 1),))[:count].copy()


def _wr(ptr, count, first):
    """The output behind ptr: a copy of its `count` elements as they came in, then first, first + 1, ... written over them."""
    if ptr is None:
        return None
    a = np.ctypeslib.as_array(ptr, shape=(max(count, 1),))[:count]
    seen = a.copy()
    a[:] = first + np.arange(count)
    return seen


class _Stub:
    """Stands in for the loaded library: every ccal_*_batch records its arguments under .got and returns OK."""

    def __init__(self):
        self.got = {}

    def ccal_ctx_create(self, device, stream, handle):
        return _ffi.OK

    def ccal_rdh_batch(self, h, n, offs, pairs, seeds, n_hyp, lam, H, score, best, n_valid, h_sample, h_lam, h_H, h_score):
        m, o = max(n, 1), _rd(offs, n + 1)
        self.got = dict(n=n, offs=o, pairs=_rd(pairs, max(int(o[-1]), 1) * 4), seeds=_rd(seeds, n), n_hyp=n_hyp,
                        lam=_wr(lam, m, 100.0), H=_wr(H, m * 9, 200.0), score=_wr(score, m, 300.0), best=_wr(best, m, 400),
                        n_valid=_wr(n_valid, m, 500), h_sample=_wr(h_sample, m * n_hyp * 6, 600), h_lam=_wr(h_lam, m * n_hyp, 700.0),
                        h_H=_wr(h_H, m * n_hyp * 9, 800.0), h_score=_wr(h_score, m * n_hyp, 900.0))
        return _ffi.OK

    def ccal_pnp_batch(self, h, n, offs, xyz, xn, min_points, poses, used, cost):
        m, o = max(n, 1), _rd(offs, n + 1)
        self.got = dict(n=n, offs=o, xyz=_rd(xyz, int(o[-1]) * 3), xn=_rd(xn, int(o[-1]) * 2), min_points=min_points,
                        poses=_wr(poses, m * 6, 100.0), used=_wr(used, m, 200), cost=_wr(cost, m, 300.0))
        return _ffi.OK

    def _results(self, n, tot, poses, status, iters, used, cost0, cost, err):
        m = max(n, 1)
        return dict(poses=_wr(poses, m * 6, 100.0), status=_wr(status, m, 200), iters=_wr(iters, m, 300), used=_wr(used, m, 400),
                    cost0=_wr(cost0, m, 500.0), cost=_wr(cost, m, 600.0), err=_wr(err, max(tot, 1), 700.0))

    def ccal_refine_poses_batch(self, h, model, par, delta, n, offs, xyz, uv, min_points, opts, poses, status, iters, used, cost0,
                                cost, err):
        o = _rd(offs, n + 1)
        tot = int(o[-1])
        self.got = dict(model=model, par=_rd(par, _ffi.PMAX), delta=delta, n=n, offs=o, xyz=_rd(xyz, tot * 3), uv=_rd(uv, tot * 2),
                        min_points=min_points, opts=opts, **self._results(n, tot, poses, status, iters, used, cost0, cost, err))
        return _ffi.OK

    def ccal_refine_rig_poses_batch(self, h, n_cams, model, par, extr, delta, n, seg_offs, seg_cam, pt_offs, xyz, uv, min_points, opts,
                                    poses, status, iters, used, cost0, cost, err):
        so = _rd(seg_offs, n + 1)
        n_seg = int(so[-1])
        po = _rd(pt_offs, n_seg + 1)
        tot = int(po[-1])
        self.got = dict(n_cams=n_cams, model=_rd(model, n_cams), par=_rd(par, n_cams * _ffi.PMAX), extr=_rd(extr, n_cams * 6),
                        delta=delta, n=n, seg_offs=so, seg_cam=_rd(seg_cam, n_seg + 1), pt_offs=po, xyz=_rd(xyz, tot * 3),
                        uv=_rd(uv, tot * 2), min_points=min_points, opts=opts,
                        **self._results(n, tot, poses, status, iters, used, cost0, cost, err))
        return _ffi.OK


@pytest.fixture
def ctx():
    return Context(lib=_Stub())


def _same(a, dtype, values):
    """a is an array of exactly this dtype and these values (NaN equal to NaN)."""
    assert a is not None and a.dtype == dtype, (a, dtype)
    np.testing.assert_array_equal(a, np.asarray(values, dtype=dtype))


def _padded(a, shape):
    """A returned array is a leading slice of the padded array that the library wrote into."""
    assert a.base is not None and a.base.shape == shape, (a.base, shape)


# three problems of 3, 0 and 5 points: rows 1, 2, ... so that a row out of place shows
X3 = [[[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.zeros((0, 3)), [[10, 11, 12], [13, 14, 15], [16, 17, 18], [19, 20, 21], [22, 23, 24]]]
U3 = [[[1, 2], [3, 4], [5, 6]], [], [[7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]]


def test_pnp_batch(ctx):
    g = lambda: ctx.lib.got
    poses, used, cost = ctx.pnp_batch([], [])
    _same(g()["offs"], np.int64, [0]); assert g()["n"] == 0 and g()["xyz"].size == 0 and g()["xn"].size == 0
    _same(g()["poses"], np.float64, [NAN] * 6); _same(g()["used"], np.int32, [-2]); _same(g()["cost"], np.float64, [NAN])
    assert poses.shape == (0, 6) and used.shape == (0,) and cost.shape == (0,)
    _padded(poses, (1, 6)); _padded(used, (1,)); _padded(cost, (1,))

    poses, used, cost = ctx.pnp_batch([np.zeros((0, 3))], [np.zeros((0, 2))], min_points=5, with_cost=False)
    _same(g()["offs"], np.int64, [0, 0]); assert g()["xyz"].size == 0 and g()["min_points"] == 5
    assert g()["cost"] is None and cost is None
    _same(poses, np.float64, [[100, 101, 102, 103, 104, 105]]); _same(used, np.int32, [200])

    poses, used, cost = ctx.pnp_batch(X3, U3)
    _same(g()["offs"], np.int64, [0, 3, 3, 8])
    _same(g()["xyz"], np.float64, np.arange(1.0, 25.0)); _same(g()["xn"], np.float64, np.arange(1.0, 17.0))
    _same(g()["poses"], np.float64, [NAN] * 18); _same(g()["used"], np.int32, [-2] * 3); _same(g()["cost"], np.float64, [NAN] * 3)
    assert g()["min_points"] == 4
    _same(poses, np.float64, 100.0 + np.arange(18).reshape(3, 6)); _same(used, np.int32, [200, 201, 202])
    _same(cost, np.float64, [300, 301, 302])

    with pytest.raises(ValueError):
        ctx.pnp_batch(X3, U3[:2])
    with pytest.raises(ValueError):
        ctx.pnp_batch(X3, [U3[0], [[0, 0]], U3[2]])


def test_rdh_batch(ctx):
    g = lambda: ctx.lib.got
    out = ctx.rdh_batch([], [], n_hyp=2)
    _same(g()["offs"], np.int64, [0]); _same(g()["pairs"], np.float64, [0] * 4)        # no pairs at all: one row of zeros
    assert g()["n"] == 0 and g()["n_hyp"] == 2 and g()["seeds"].size == 0 and g()["seeds"].dtype == np.uint64
    _same(g()["lam"], np.float64, [NAN]); _same(g()["H"], np.float64, [NAN] * 9); _same(g()["score"], np.float64, [NAN])
    _same(g()["best"], np.int32, [-2]); _same(g()["n_valid"], np.int32, [-2])
    assert all(g()[k] is None for k in ("h_sample", "h_lam", "h_H", "h_score"))
    assert sorted(out) == ["H", "best", "lambda", "n_valid", "score"]
    assert out["lambda"].shape == (0,) and out["H"].shape == (0, 3, 3) and out["best"].shape == (0,)
    _padded(out["H"], (1, 3, 3))

    out = ctx.rdh_batch([np.zeros((0, 4))], [-1], n_hyp=2)
    _same(g()["offs"], np.int64, [0, 0]); _same(g()["pairs"], np.float64, [0] * 4); _same(g()["seeds"], np.uint64, [2**64 - 1])
    _same(out["lambda"], np.float64, [100]); _same(out["H"], np.float64, 200.0 + np.arange(9).reshape(1, 3, 3))

    P = [np.arange(1.0, 13.0).reshape(3, 4), np.zeros((0, 4)), np.arange(13.0, 33.0).reshape(5, 4)]
    out = ctx.rdh_batch(P, [1, 2, 3], n_hyp=2, per_hypothesis=True)
    _same(g()["offs"], np.int64, [0, 3, 3, 8]); _same(g()["pairs"], np.float64, np.arange(1.0, 33.0))
    _same(g()["seeds"], np.uint64, [1, 2, 3])
    _same(g()["lam"], np.float64, [NAN] * 3); _same(g()["H"], np.float64, [NAN] * 27); _same(g()["best"], np.int32, [-2] * 3)
    _same(g()["h_sample"], np.int32, [-2] * 36); _same(g()["h_lam"], np.float64, [NAN] * 6)
    _same(g()["h_H"], np.float64, [NAN] * 54); _same(g()["h_score"], np.float64, [NAN] * 6)
    _same(out["score"], np.float64, [300, 301, 302]); _same(out["best"], np.int32, [400, 401, 402])
    _same(out["n_valid"], np.int32, [500, 501, 502])
    _same(out["hyp_sample"], np.int32, 600 + np.arange(36).reshape(3, 2, 6))
    _same(out["hyp_lambda"], np.float64, 700.0 + np.arange(6).reshape(3, 2))
    _same(out["hyp_H"], np.float64, 800.0 + np.arange(54).reshape(3, 2, 9))
    _same(out["hyp_score"], np.float64, 900.0 + np.arange(6).reshape(3, 2))

    with pytest.raises(ValueError):
        ctx.rdh_batch(P, [1, 2])


def _check_results(got, out, n, tot, with_errors):
    """The seven result arrays of a refine call: poisoned and padded going in, sliced coming out."""
    m = max(n, 1)
    for k in ("status", "iters", "used"):
        _same(got[k], np.int32, [-2] * m)
    _same(got["cost0"], np.float64, [NAN] * m); _same(got["cost"], np.float64, [NAN] * m)
    assert len(out) == (7 if with_errors else 6)
    _same(out[0], np.float64, 100.0 + np.arange(n * 6).reshape(n, 6)); _padded(out[0], (m, 6))
    for i, (dt, first) in enumerate([(np.int32, 200), (np.int32, 300), (np.int32, 400), (np.float64, 500), (np.float64, 600)]):
        _same(out[1 + i], dt, first + np.arange(n)); _padded(out[1 + i], (m,))
    if with_errors:
        _same(got["err"], np.float64, [NAN] * max(tot, 1))
    else:
        assert got["err"] is None


def test_refine_poses_batch(ctx):
    g = lambda: ctx.lib.got
    out = ctx.refine_poses_batch(2, [1.0, 2.0, 3.0], [], [], np.zeros((0, 6)))
    _same(g()["offs"], np.int64, [0]); assert g()["n"] == 0 and g()["xyz"].size == 0 and g()["uv"].size == 0
    _same(g()["par"], np.float64, [1, 2, 3] + [0] * (_ffi.PMAX - 3)); _same(g()["poses"], np.float64, [NAN] * 6)
    assert (g()["model"], g()["delta"], g()["min_points"], g()["opts"]) == (2, 1.0, 4, None)
    _check_results(g(), out, 0, 0, False)

    out = ctx.refine_poses_batch(1, [5.0], [np.zeros((0, 3))], [np.zeros((0, 2))], [[1, 2, 3, 4, 5, 6]], huber_delta=0.5, min_points=6,
                                 with_errors=True)
    _same(g()["offs"], np.int64, [0, 0]); _same(g()["poses"], np.float64, [1, 2, 3, 4, 5, 6])
    assert (g()["model"], g()["delta"], g()["min_points"]) == (1, 0.5, 6)
    _check_results(g(), out, 1, 0, True)
    assert len(out[6]) == 1 and out[6][0].shape == (0,)

    start = np.arange(18.0).reshape(3, 6)
    for with_errors in (False, True):
        out = ctx.refine_poses_batch(3, np.arange(1.0, 7.0), X3, U3, start, with_errors=with_errors)
        _same(g()["offs"], np.int64, [0, 3, 3, 8])
        _same(g()["xyz"], np.float64, np.arange(1.0, 25.0)); _same(g()["uv"], np.float64, np.arange(1.0, 17.0))
        _same(g()["poses"], np.float64, np.arange(18.0))
        _check_results(g(), out, 3, 8, with_errors)
    assert [e.tolist() for e in out[6]] == [[700, 701, 702], [], [703, 704, 705, 706, 707]]

    with pytest.raises(ValueError):
        ctx.refine_poses_batch(3, [1.0], X3, U3[:2], start)
    with pytest.raises(ValueError):
        ctx.refine_poses_batch(3, [1.0], X3, [U3[0], [[0, 0]], U3[2]], start)


def test_refine_rig_poses_batch(ctx):
    g = lambda: ctx.lib.got
    models, params, extr = [1, 3], [[1.0, 2.0], [3.0, 4.0, 5.0]], np.arange(12.0).reshape(2, 6)
    par = [1, 2] + [0] * (_ffi.PMAX - 2) + [3, 4, 5] + [0] * (_ffi.PMAX - 3)
    out = ctx.refine_rig_poses_batch(models, params, extr, [], np.zeros((0, 6)))
    assert (g()["n_cams"], g()["n"], g()["delta"], g()["min_points"], g()["opts"]) == (2, 0, 1.0, 4, None)
    _same(g()["model"], np.int32, [1, 3]); _same(g()["par"], np.float64, par); _same(g()["extr"], np.float64, np.arange(12.0))
    _same(g()["seg_offs"], np.int64, [0]); _same(g()["seg_cam"], np.int32, [0]); _same(g()["pt_offs"], np.int64, [0])
    assert g()["xyz"].size == 0 and g()["uv"].size == 0
    _same(g()["poses"], np.float64, [NAN] * 6)
    _check_results(g(), out, 0, 0, False)

    # three slots: two segments (2 and 3 points, cameras 0 and 1), no segment, one segment of 0 points (camera 1)
    slots = [[(0, [[1, 2, 3], [4, 5, 6]], [[1, 2], [3, 4]]), (1, [[7, 8, 9], [10, 11, 12], [13, 14, 15]], [[5, 6], [7, 8], [9, 10]])],
             [], [(1, np.zeros((0, 3)), np.zeros((0, 2)))]]
    start = np.arange(18.0).reshape(3, 6)
    for with_errors in (False, True):
        out = ctx.refine_rig_poses_batch(models, params, extr, slots, start, huber_delta=2.0, min_points=5, with_errors=with_errors)
        assert (g()["n_cams"], g()["n"], g()["delta"], g()["min_points"]) == (2, 3, 2.0, 5)
        _same(g()["seg_offs"], np.int64, [0, 2, 2, 3]); _same(g()["seg_cam"], np.int32, [0, 1, 1, 0])
        _same(g()["pt_offs"], np.int64, [0, 2, 5, 5])
        _same(g()["xyz"], np.float64, np.arange(1.0, 16.0)); _same(g()["uv"], np.float64, np.arange(1.0, 11.0))
        _same(g()["poses"], np.float64, np.arange(18.0))
        _check_results(g(), out, 3, 5, with_errors)
    assert [e.tolist() for e in out[6]] == [[700, 701, 702, 703, 704], [], []]

    with pytest.raises(ValueError):
        ctx.refine_rig_poses_batch(models, params, extr, [[(0, [[1, 2, 3], [4, 5, 6]], [[1, 2]])]], start[:1])
    with pytest.raises(ValueError):
        ctx.refine_rig_poses_batch(models, params[:1], extr, slots, start)
