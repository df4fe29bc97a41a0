"""CPU: what every wrapper of engine.py outside tests/test_engine_pack_cpu.py hands to the library and what it makes of the answer,
through a stub in the library's place.  The stub records the argument list of every call - scalars with their Python types, what the
pointers address on entry, the fields of the option structs, NULL - and writes numbers that name their position (100 * the
argument's index, counting up) into every output it knows the size of.  Every expected value is written out here.  The error texts,
the public signatures (tests/golden/engine_signatures.json) and the order of the destroy calls are held the same way."""
import ctypes as C
import functools
import inspect
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import _ffi, engine
from camera_intrinsic_calibration_rs_amd.engine import (CcalError, Context, MultiContext, MultiProblem, Problem, aprilgrid_target,
                                                        checkerboard_target, grey_opts, make_desc, normalize_opts, partition_slots,
                                                        photo_tables, render_opts, solve_sharded)

NAN = np.nan
PMAX = _ffi.PMAX

# what the stub's functions that are no status calls return
RETURNS = {"ccal_last_error": b"ctx detail", "ccal_multi_last_error": b"multi detail", "ccal_create_last_error": b"create detail",
           "ccal_num_corners": 7, "ccal_reduced_dim": 5, "ccal_jacobian_len": 11, "ccal_block_dim": 4, "ccal_eff_num_params": 6,
           "ccal_multi_problem_num_shards": 2, "ccal_multi_transport": 2, "ccal_multi_rccl_ranks": 0, "ccal_multi_problem_shard": 0x5000,
           "ccal_rccl_available": 1, "ccal_rccl_comm_count": 3}
DESTROYS = ("ccal_ctx_destroy", "ccal_undistort_map_destroy", "ccal_multi_destroy", "ccal_multi_problem_destroy", "ccal_problem_destroy",
            "ccal_rccl_comm_destroy")
# the fields a call of the library sets in a struct: name -> (argument index, fields)
SETS = {"ccal_render_set_defaults": (1, dict(supersample=4, black=40.0, white=215.0, background=0.0, margin=0.03)),
        "ccal_normalize_set_defaults": (0, dict(radius=16, min_sigma=4.0, amp=64.0)),
        "ccal_grey_set_defaults": (0, dict(bin=1, w_r=19595, w_g=38470, w_b=7471)),
        "ccal_set_defaults": (0, dict(method=0, max_iterations=100)),
        "ccal_solve": (5, dict(iterations=3)), "ccal_solve_dev": (2, dict(iterations=4)), "ccal_multi_solve": (5, dict(iterations=5)),
        "ccal_solve_sharded": (6, dict(iterations=6)), "ccal_covariance": (8, dict(bad_slot=1))}


def _offs(ptr, n):
    return np.ctypeslib.as_array(ptr, shape=(n + 1,)).copy()


def _sz_points(in_w, out_w):
    return lambda s, a: {2: s.n_par, 4: a[3] * in_w, 5: max(a[3], 1) * out_w, 6: max(a[3], 1)}


def _sz_corners(s, a):
    n = int(_offs(a[6], a[4])[-1]); m = max(n, 1)
    return {6: a[4] + 1, 7: m * 2, 11: m, 12: m, 13: m}


def _sz_detect(s, a):
    m, rows = max(a[4], 1), max(a[10], 1)
    return {11: m, 12: m * rows * 2, 13: m * rows * 3, 14: m * rows}


def _sz_tags(s, a):
    n = int(_offs(a[6], a[4])[-1]); m = max(n, 1)
    return {6: a[4] + 1, 7: n * 8, 10: a[11], 16: m, 17: m, 18: m, 19: m, 20: m * 8, 21: m, 22: m}


def _sz_quads(s, a):
    n = int(_offs(a[6], a[4])[-1]); m, rows = max(a[4], 1), max(a[14], 1)
    return {6: a[4] + 1, 7: n * 2, 15: m, 16: m, 17: m * rows * 4, 18: m * rows * 8}


def _sz_detect_tags(s, a):
    m, rows = max(a[4], 1), max(a[9]._obj.tag_cap, 1)
    return {7: a[8], 10: m, 11: m * rows, 12: m * rows, 13: m * rows, 14: m * rows * 8, 15: m * rows, 16: m, 17: m * 4}


def _sz_assemble(s, a):
    n = int(_offs(a[2], a[1])[-1]); m, nw = max(a[1], 1), max(a[5] * a[6], 1)
    return {2: a[1] + 1, 3: n * 2, 4: n * 3, 7: m, 8: m * nw * 2, 9: m * nw, 10: m, 11: m * 4}


def _sz_detect_boards(s, a):
    m, nw = max(a[4], 1), max(a[6]._obj.cols * a[6]._obj.rows, 1)
    return {7: m, 8: m * nw * 2, 9: m, 10: m * 4}


def _sz_params(first):
    return lambda s, a: {first: s.n_cams * PMAX, first + 1: s.n_slots * 6, first + 2: s.n_cams * 6}


def _sz_init(first):
    return lambda s, a: {first: max(s.n_obs, 1) * 6, first + 1: max(s.n_obs, 1)}


# the number of elements behind every pointer argument the stub reads or writes: name -> f(stub, arguments) -> {index: count}
SIZES = {
    "ccal_project_points": _sz_points(3, 2), "ccal_unproject_points": _sz_points(2, 3),
    "ccal_estimate_new_camera_matrix": lambda s, a: {2: s.n_par, 8: 9},
    "ccal_undistort_map_create": lambda s, a: {2: s.n_par, 3: 9, 4: 9},
    "ccal_undistort_map_from_host": lambda s, a: {1: a[3] * a[4], 2: a[3] * a[4]},
    "ccal_undistort_map_download": lambda s, a: {1: 6, 2: 6},
    "ccal_refine_corners_batch": _sz_corners, "ccal_refine_corners_dev": _sz_corners,
    "ccal_detect_corners_batch": _sz_detect, "ccal_detect_corners_dev": _sz_detect,
    "ccal_decode_tags_batch": _sz_tags, "ccal_decode_tags_dev": _sz_tags,
    "ccal_propose_quads_batch": _sz_quads, "ccal_propose_quads_dev": _sz_quads,
    "ccal_detect_tags_batch": _sz_detect_tags, "ccal_detect_tags_dev": _sz_detect_tags,
    "ccal_assemble_checkerboards_batch": _sz_assemble,
    "ccal_detect_checkerboards_batch": _sz_detect_boards, "ccal_detect_checkerboards_dev": _sz_detect_boards,
    "ccal_render_targets_batch": lambda s, a: {2: s.n_par, 7: a[6] * 6}, "ccal_render_targets_dev": lambda s, a: {2: s.n_par, 7: a[6] * 6},
    "ccal_render_photo_targets": lambda s, a: {2: s.n_par, 7: a[6] * 6}, "ccal_render_photo_targets_dev": lambda s, a: {2: s.n_par, 7: a[6] * 6},
    "ccal_photo_tables": lambda s, a: {2: 17, 3: 256},
    "ccal_partition_slots": lambda s, a: {2: a[1] + 1},
    "ccal_multi_create_transport": lambda s, a: {0: a[1]},
    "ccal_disable_distortions": lambda s, a: {2: s.n_cams * PMAX}, "ccal_multi_disable_distortions": lambda s, a: {2: s.n_cams * PMAX},
    "ccal_upload_params": _sz_params(1), "ccal_multi_upload_params": _sz_params(1),
    "ccal_download_params": _sz_params(1),
    "ccal_init_poses": lambda s, a: {1: s.n_cams * PMAX, **_sz_init(3)(s, a)},
    "ccal_multi_init_poses": lambda s, a: {1: s.n_cams * PMAX, **_sz_init(3)(s, a)},
    "ccal_init_poses_division": _sz_init(3),
    "ccal_validation": _sz_params(2), "ccal_multi_validation": _sz_params(2),
    "ccal_reprojection_errors": lambda s, a: {**_sz_params(1)(s, a), 4: 7},
    "ccal_multi_reprojection_errors": lambda s, a: {**_sz_params(1)(s, a), 4: 7, 5: s.n_obs + 1},
    "ccal_eval": lambda s, a: {**_sz_params(1)(s, a), 5: 14, 6: 11},
    "ccal_build_normal": lambda s, a: {**_sz_params(1)(s, a), 5: 25, 6: 5},
    "ccal_solve": _sz_params(2), "ccal_multi_solve": _sz_params(2),
    "ccal_solve_sharded": lambda s, a: {3: s.n_cams * PMAX, 4: s.n_slots * 6, 5: s.n_cams * 6},
    "ccal_solve_batch": lambda s, a: {3: s.n_cams * PMAX, 4: s.n_slots * 6, 5: s.n_cams * 6},
    "ccal_covariance": lambda s, a: {**_sz_params(1)(s, a), 4: 25, 5: max(s.n_slots, 1) * 36, 6: 7, 7: max(s.n_slots, 1)},
}


_r = lambda a, b: set(range(a, b + 1))
# which of those pointers are outputs: the stub writes into them and into nothing else
OUTS = {"ccal_project_points": {5, 6}, "ccal_unproject_points": {5, 6}, "ccal_estimate_new_camera_matrix": {8},
        "ccal_undistort_map_download": {1, 2}, "ccal_refine_corners_batch": {7, 11, 12, 13}, "ccal_refine_corners_dev": {7, 11, 12, 13},
        "ccal_detect_corners_batch": _r(11, 14), "ccal_detect_corners_dev": _r(11, 14), "ccal_decode_tags_batch": _r(16, 22),
        "ccal_decode_tags_dev": _r(16, 22), "ccal_propose_quads_batch": _r(15, 18), "ccal_propose_quads_dev": _r(15, 18),
        "ccal_detect_tags_batch": _r(10, 17), "ccal_detect_tags_dev": _r(10, 17), "ccal_assemble_checkerboards_batch": _r(7, 11),
        "ccal_detect_checkerboards_batch": _r(7, 10), "ccal_detect_checkerboards_dev": _r(7, 10), "ccal_photo_tables": {2, 3},
        "ccal_partition_slots": {2}, "ccal_download_params": {1, 2, 3}, "ccal_init_poses": {3, 4}, "ccal_multi_init_poses": {3, 4},
        "ccal_init_poses_division": {3, 4}, "ccal_reprojection_errors": {4}, "ccal_multi_reprojection_errors": {4}, "ccal_eval": {5, 6},
        "ccal_build_normal": {5, 6}, "ccal_solve": {2, 3, 4}, "ccal_multi_solve": {2, 3, 4}, "ccal_solve_sharded": {3, 5},
        "ccal_covariance": _r(4, 7)}


class _Stub:
    """Stands in for the loaded library.  .calls: (name, recorded arguments) of every status call and destroy call in order;
    .rc[name]: the status a call returns (OK otherwise); .fill[name][index]: what to write into an output instead of the default
    100 * index, 100 * index + 1, ...; .void[name][index] = (count, dtype, fill or None): what a void pointer addresses."""

    def __init__(self):
        self.calls, self.rc, self.fill, self.void = [], {}, {}, {}
        self.next_handle = 0
        self.n_par, self.n_cams, self.n_slots, self.n_obs = 4, 1, 2, 2

    def __getattr__(self, name):
        if not name.startswith("ccal_"):
            raise AttributeError(name)
        if name in RETURNS:
            return lambda *a: RETURNS[name]
        return functools.partial(self._call, name)

    def last(self, name=None):
        got = self.calls[-1]
        assert name is None or got[0] == name, got[0]
        return got[1]

    def _mem(self, name, i, arr, fill):
        seen = arr.copy()
        fill = self.fill.get(name, {}).get(i, fill)
        if fill is not None and arr.size:
            arr[:] = (fill + np.arange(arr.size)) if np.isscalar(fill) else np.asarray(fill).ravel()
        return seen

    def _arg(self, name, i, a, sizes):
        if a is None or isinstance(a, (int, float, bytes, str)):
            return a
        if isinstance(a, C.c_void_p):
            if i in self.void.get(name, {}):
                count, dtype, fill = self.void[name][i]
                p = C.cast(a, C.POINTER(np.ctypeslib.as_ctypes_type(dtype)))
                return ("mem", self._mem(name, i, np.ctypeslib.as_array(p, shape=(max(count, 1),))[:count], fill))
            return ("vp", a.value)
        if isinstance(a, C._Pointer):
            if i not in sizes:
                return ("ptr", type(a)._type_.__name__)
            return self._mem(name, i, np.ctypeslib.as_array(a, shape=(max(sizes[i], 1),))[:sizes[i]], 100 * i if i in OUTS.get(name, ()) else None)
        if isinstance(a, C._CFuncPtr):
            return ("fn", bool(a))
        if isinstance(a, C.Array):
            if a._type_ is C.c_char:
                raw = a.raw
                C.memset(a, 7, len(raw))
                return raw
            if a._type_ is C.c_void_p:
                return ("vps", list(a))
            if issubclass(a._type_, C.Structure):
                return ("structs", a._type_.__name__, len(a))
            return ("ptrs", [self._mem(name, i, np.ctypeslib.as_array(p, shape=(max(sizes[i], 1),))[:sizes[i]], None) for p in a])
        o = a._obj                                              # byref(o)
        if isinstance(o, C.c_void_p):
            self.next_handle += 0x1000
            o.value = self.next_handle
            return ("new", o.value)
        if isinstance(o, C.c_double):
            o.value = i + 0.5
            return "f64*"
        if isinstance(o, C.c_int32):
            o.value = 10 * i
            return "i32*"
        seen = {f: getattr(o, f) for f, _ in o._fields_ if isinstance(getattr(o, f), (int, float)) and f != "reserved_"}
        if name in SETS and SETS[name][0] == i:
            for f, v in SETS[name][1].items():
                setattr(o, f, v)
        return (type(o).__name__, seen)

    def _call(self, name, *args):
        sizes = SIZES[name](self, args) if name in SIZES else {}
        self.calls.append((name, [self._arg(name, i, a, sizes) for i, a in enumerate(args)]))
        return None if name in DESTROYS else self.rc.get(name, _ffi.OK)


class Some:
    """An array of this dtype and size whose content is not looked at: np.empty."""

    def __init__(self, dtype, size):
        self.dtype, self.size = np.dtype(dtype), size


def _eq(got, want, path="arg"):
    """got is want: the same Python type, for arrays the same dtype and values (NaN equal to NaN), element by element."""
    if isinstance(want, Some):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.size == want.size, (path, got, want.dtype, want.size)
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (path, got, want)
        np.testing.assert_array_equal(got, want, err_msg=path)
    elif isinstance(want, (tuple, list)):
        assert type(got) is type(want) and len(got) == len(want), (path, got, want)
        for k, (g, w) in enumerate(zip(got, want)):
            _eq(g, w, f"{path}[{k}]")
    elif isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (path, got, want)
        for k in want:
            _eq(got[k], want[k], f"{path}[{k!r}]")
    else:
        assert type(got) is type(want) and got == want, (path, got, want)


def f8(*v): return np.asarray(v, dtype=np.float64).reshape(-1)
def f4(*v): return np.asarray(v, dtype=np.float32).reshape(-1)
def i4(*v): return np.asarray(v, dtype=np.int32).reshape(-1)
def i8(*v): return np.asarray(v, dtype=np.int64).reshape(-1)
def u8(*v): return np.asarray(v, dtype=np.uint64).reshape(-1)
def u1(*v): return np.asarray(v, dtype=np.uint8).reshape(-1)
def up(first, count, dtype=np.float64): return (first + np.arange(count)).astype(dtype)


def H(k):
    """The k-th handle the stub gave out, as the library gets it back."""
    return ("vp", 0x1000 * k)


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(_ffi, "load", lambda: s)          # the free functions without a lib argument
    return s


@pytest.fixture
def ctx(stub):
    c = Context(lib=stub)
    _eq(stub.last("ccal_ctx_create"), [0, None, ("new", 0x1000)])
    return c


PAR = [1.0, 2.0, 3.0, 4.0]
IMG2 = np.arange(40, dtype=np.uint8).reshape(2, 4, 5)
IMG3 = np.arange(60, dtype=np.uint16).reshape(3, 4, 5)
DEV = 0xABC0


# ---------------------------------------------------------------------------------------------------------------------------------
# Context: the small calls
def test_context_create_sync_pin(stub, ctx):
    assert ctx.device == 0 and ctx.handle.value == 0x1000 and ctx.last_error() == "ctx detail"
    c2 = Context(3, stream=0x77, lib=stub)
    _eq(stub.last("ccal_ctx_create"), [3, ("vp", 0x77), ("new", 0x2000)])
    assert c2.device == 3
    assert ctx.sync() is None
    _eq(stub.last("ccal_sync"), [H(1)])
    a = np.arange(6.0).reshape(2, 3)
    assert ctx.pin(a) is a
    _eq(stub.last("ccal_pin_buffer"), [H(1), ("vp", a.ctypes.data), 48])
    assert ctx.unpin(a) is None
    _eq(stub.last("ccal_unpin_buffer"), [H(1), ("vp", a.ctypes.data)])
    with pytest.raises(ValueError, match="^pin: a C-contiguous array$"):
        ctx.pin(a.T)


def test_model_conventions_and_rccl(stub, ctx):
    cv = ctx.model_conventions()
    assert isinstance(cv, _ffi.ModelConventions)
    _eq(stub.last("ccal_get_model_conventions"), [H(1), ("ModelConventions", dict(kb4_small_radius=0.0, unproject_small_radius=0.0))])
    cv.kb4_small_radius = 0.25
    assert ctx.set_model_conventions(cv) is None
    _eq(stub.last("ccal_set_model_conventions"), [H(1), ("ModelConventions", dict(kb4_small_radius=0.25, unproject_small_radius=0.0))])
    ctx.set_model_conventions(None)
    _eq(stub.last("ccal_set_model_conventions"), [H(1), None])
    uid = bytes(range(128))
    assert ctx.rccl_comm_create(2, 1, uid) == 0x2000
    _eq(stub.last("ccal_rccl_comm_create"), [H(1), 2, 1, uid, ("new", 0x2000)])
    with pytest.raises(ValueError, match="^an RCCL unique id is 128 bytes$"):
        ctx.rccl_comm_create(2, 1, b"short")
    assert engine.rccl_unique_id() == b"\x07" * 128
    _eq(stub.last("ccal_rccl_unique_id"), [bytes(128)])
    assert engine.rccl_available() is True and engine.rccl_comm_count(0x2000) == 3
    engine.rccl_comm_destroy(0x2000)
    _eq(stub.last("ccal_rccl_comm_destroy"), [("vp", 0x2000)])


def test_points(stub, ctx):
    stub.fill = {"ccal_project_points": {6: [0, 1]}}
    uv, valid = ctx.project_points(3, PAR, [[1, 2, 3], [4, 5, 6]])
    _eq(stub.last("ccal_project_points"), [H(1), 3, f8(*PAR), 2, f8(1, 2, 3, 4, 5, 6), f8(*[NAN] * 4), u1(0, 0)])
    _eq(uv, up(500, 4).reshape(2, 2)); _eq(valid, np.array([False, True]))
    stub.fill = {}
    uv, valid = ctx.project_points(3, PAR, np.zeros((0, 3)))
    _eq(stub.last("ccal_project_points"), [H(1), 3, f8(*PAR), 0, f8(), f8(NAN, NAN), u1(0)])
    assert uv.shape == (0, 2) and valid.shape == (0,) and valid.dtype == bool
    rays, valid = ctx.unproject_points(1, PAR, [[7, 8]])
    _eq(stub.last("ccal_unproject_points"), [H(1), 1, f8(*PAR), 1, f8(7, 8), f8(NAN, NAN, NAN), u1(0)])
    _eq(rays, f8(500, 501, 502).reshape(1, 3)); _eq(valid, np.array([True]))
    with pytest.raises(ValueError, match=r"^ccal_project_points: an \[n, 3\] array$"):
        ctx.project_points(3, PAR, [[1, 2]])
    with pytest.raises(ValueError, match=r"^ccal_unproject_points: an \[n, 2\] array$"):
        ctx.unproject_points(3, PAR, [1, 2])


def test_new_camera_matrix_and_maps(stub, ctx):
    K = ctx.estimate_new_camera_matrix(2, PAR, 640, 480, 0.5)
    _eq(stub.last("ccal_estimate_new_camera_matrix"), [H(1), 2, f8(*PAR), 640, 480, 0.5, 0, 0, f8(*[NAN] * 9)])
    _eq(K, up(800, 9).reshape(3, 3))
    ctx.estimate_new_camera_matrix(2, PAR, 640, 480, 1, new_w_h=(320.0, 240))
    _eq(stub.last("ccal_estimate_new_camera_matrix"), [H(1), 2, f8(*PAR), 640, 480, 1.0, 320, 240, f8(*[NAN] * 9)])
    stub.rc["ccal_estimate_new_camera_matrix"] = _ffi.NO_RESULT
    assert ctx.estimate_new_camera_matrix(2, PAR, 640, 480, 0.5) is None

    m = ctx.undistort_map(2, PAR, np.arange(9.0).reshape(3, 3), (3, 2))
    _eq(stub.last("ccal_undistort_map_create"), [H(1), 2, f8(*PAR), up(0, 9), None, 3, 2, ("new", 0x2000)])
    assert (m.w, m.h, m.handle.value, m.ctx, m.lib) == (3, 2, 0x2000, ctx, stub)
    m3 = ctx.undistort_map(2, PAR, np.arange(9.0), (3.0, 2.0), rotation=np.arange(10.0, 19.0).reshape(3, 3))     # (held: a dropped map is destroyed)
    _eq(stub.last("ccal_undistort_map_create"), [H(1), 2, f8(*PAR), up(0, 9), up(10, 9), 3, 2, ("new", 0x3000)])

    xm, ym = np.arange(6, dtype=np.float32).reshape(2, 3), np.arange(6, 12, dtype=np.float32).reshape(2, 3)
    m2 = ctx.undistort_map_from_arrays(xm, ym)
    _eq(stub.last("ccal_undistort_map_from_host"), [H(1), f4(0, 1, 2, 3, 4, 5), f4(6, 7, 8, 9, 10, 11), 3, 2, ("new", 0x4000)])
    assert (m2.w, m2.h, m2.handle.value) == (3, 2, 0x4000)
    with pytest.raises(ValueError, match="^maps: float32 arrays$"):
        ctx.undistort_map_from_arrays(xm.astype(np.float64), ym)
    with pytest.raises(ValueError, match="^maps: two non-empty"):
        ctx.undistort_map_from_arrays(xm, ym[:1])

    x, y = m2.download()
    _eq(stub.last("ccal_undistort_map_download"), [H(4), Some(np.float32, 6), Some(np.float32, 6)])
    _eq(x, up(100, 6, np.float32).reshape(2, 3)); _eq(y, up(200, 6, np.float32).reshape(2, 3))
    stub.void = {"ccal_remap": {6: (40, np.uint8, None), 7: (12, np.uint8, 50)}}
    out = m2.remap(IMG2)
    _eq(stub.last("ccal_remap"), [H(4), 0, 1, 5, 4, 2, ("mem", up(0, 40, np.uint8)), ("mem", Some(np.uint8, 12))])
    _eq(out, up(50, 12, np.uint8).reshape(2, 2, 3))
    rgb = np.arange(24, dtype=np.uint8).reshape(1, 2, 4, 3)
    stub.void = {}
    out = m2.remap(rgb)
    _eq(stub.last("ccal_remap"), [H(4), 0, 3, 4, 2, 1, ("vp", rgb.ctypes.data), ("vp", out.ctypes.data)])
    assert out.shape == (1, 2, 3, 3) and out.dtype == np.uint8
    assert m2.remap_dev(DEV, DEV + 64, 1.0, 1, 5, 4, 2) is None
    _eq(stub.last("ccal_remap_dev"), [H(4), 1, 1, 5, 4, 2, ("vp", DEV), ("vp", DEV + 64)])
    with pytest.raises(ValueError, match="^remap: uint8 or uint16 images$"):
        m2.remap(IMG2.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# Context: the seven image stages, _batch and _dev
XY3 = [[[1, 2], [3, 4]], np.zeros((0, 2)), [[5, 6]]]           # a ragged batch: 2, 0 and 1 points


def test_refine_corners(stub, ctx):
    stub.void = {"ccal_refine_corners_batch": {5: (60, np.uint16, None)}}
    xy, status, iters, lam = ctx.refine_corners_batch(IMG3, XY3)
    _eq(stub.last("ccal_refine_corners_batch"),
        [H(1), 1, 5, 4, 3, ("mem", up(0, 60, np.uint16)), i8(0, 2, 2, 3), f8(1, 2, 3, 4, 5, 6), 5, 30, 1e-3, i4(-2, -2, -2), i4(-2, -2, -2),
         f8(NAN, NAN, NAN)])
    _eq(xy, [up(700, 4).reshape(2, 2), np.zeros((0, 2)), f8(704, 705).reshape(1, 2)])
    _eq(status, [i4(1100, 1101), i4(), i4(1102)]); _eq(iters, [i4(1200, 1201), i4(), i4(1202)])
    _eq(lam, [f8(1300, 1301), f8(), f8(1302)])
    assert xy[0].base is not None                              # views of the flat outputs
    stub.void = {}
    ctx.refine_corners_batch(IMG2[:1], [[]], half_win=3.0, max_iterations=7, eps=1)
    _eq(stub.last("ccal_refine_corners_batch"),
        [H(1), 0, 5, 4, 1, ("vp", IMG2.ctypes.data), i8(0, 0), f8(NAN, NAN), 3, 7, 1.0, i4(-2), i4(-2), f8(NAN)])
    out = ctx.refine_corners_dev(DEV, 1.0, 5.0, 4, 0, [])
    _eq(stub.last("ccal_refine_corners_dev"), [H(1), 1, 5, 4, 0, ("vp", DEV), i8(0), f8(NAN, NAN), 5, 30, 1e-3, i4(-2), i4(-2), f8(NAN)])
    _eq(out, ([], [], [], []))
    xy, status, iters, lam = ctx.refine_corners_dev(DEV, 0, 5, 4, 1, [[[9, 8]]], 2, 3, 0.5)
    _eq(stub.last("ccal_refine_corners_dev"), [H(1), 0, 5, 4, 1, ("vp", DEV), i8(0, 1), f8(9, 8), 2, 3, 0.5, i4(-2), i4(-2), f8(NAN)])
    _eq(xy, [f8(700, 701).reshape(1, 2)]); _eq(status, [i4(1100)]); _eq(iters, [i4(1200)]); _eq(lam, [f8(1300)])
    with pytest.raises(ValueError, match="^ccal_refine_corners_batch: one array of corners per image$"):
        ctx.refine_corners_batch(IMG2, [[]])
    with pytest.raises(ValueError, match="^ccal_refine_corners_dev: one array of corners per image$"):
        ctx.refine_corners_dev(DEV, 0, 5, 4, 2, [[]])
    with pytest.raises(ValueError, match=r"^refine_corners_batch: single-channel images \[n\]\[H\]\[W\]$"):
        ctx.refine_corners_batch(np.zeros((1, 4, 5, 3), dtype=np.uint8), [[]])
    with pytest.raises(ValueError, match="^remap: uint8 or uint16 images$"):
        ctx.refine_corners_batch(IMG2.astype(np.int32), [[], []])


def test_detect_corners(stub, ctx):
    # 20 x 16, step 1, radius 2: (r + 1) = 3, a domain of 14 x 10 -> 5 x 4 = 20 blocks
    stub.fill = {"ccal_detect_corners_dev": {11: [5, 2]}}
    out = ctx.detect_corners_dev(DEV, 0, 20, 16, 2, nms_radius=2, max_per_image=3)          # below the bound; count 5 > 3 rows
    _eq(stub.last("ccal_detect_corners_dev"),
        [H(1), 0, 20, 16, 2, ("vp", DEV), 1, 2, 1, 102, 3, i4(0, 0), Some(np.int32, 12), Some(np.int32, 18), Some(np.int64, 6)])
    _eq(out, [(up(1200, 6, np.int32).reshape(3, 2), up(1300, 9, np.int32).reshape(3, 3), up(1400, 3, np.int64), 5),
              (up(1206, 4, np.int32).reshape(2, 2), up(1309, 6, np.int32).reshape(2, 3), up(1403, 2, np.int64), 2)])
    assert out[0][0].base is not None and out[0][0].base is out[1][0].base          # one compact copy, views of it
    stub.fill = {"ccal_detect_corners_dev": {11: [1]}}
    out = ctx.detect_corners_dev(DEV, 1, 20, 16, 1, 1, 2, 7, 0.5)                            # above: 4096 -> 20
    _eq(stub.last("ccal_detect_corners_dev"),
        [H(1), 1, 20, 16, 1, ("vp", DEV), 1, 2, 7, 512, 20, i4(0), Some(np.int32, 40), Some(np.int32, 60), Some(np.int64, 20)])
    _eq(out, [(i4(1200, 1201).reshape(1, 2), i4(1300, 1301, 1302).reshape(1, 3), i8(1400), 1)])
    out = ctx.detect_corners_dev(DEV, 1, 20, 16, 0, max_per_image=0)                         # no image, no room asked for
    _eq(stub.last("ccal_detect_corners_dev"),
        [H(1), 1, 20, 16, 0, ("vp", DEV), 1, 5, 1, 102, 0, i4(0), Some(np.int32, 2), Some(np.int32, 3), Some(np.int64, 1)])
    assert out == []
    stub.void = {"ccal_detect_corners_batch": {5: (40, np.uint8, None)}}
    stub.fill = {"ccal_detect_corners_batch": {11: [0, 3]}}
    out = ctx.detect_corners_batch(IMG2)                                                     # 5 x 4: no block at all, one row
    _eq(stub.last("ccal_detect_corners_batch"),
        [H(1), 0, 5, 4, 2, ("mem", up(0, 40, np.uint8)), 1, 5, 1, 102, 1, i4(0, 0), Some(np.int32, 4), Some(np.int32, 6), Some(np.int64, 2)])
    _eq(out, [(np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32), i8(), 0),
              (i4(1202, 1203).reshape(1, 2), i4(1303, 1304, 1305).reshape(1, 3), i8(1401), 3)])
    with pytest.raises(ValueError, match="^ccal_detect_corners_dev: rel_threshold is not finite$"):
        ctx.detect_corners_dev(DEV, 0, 20, 16, 1, rel_threshold=NAN)
    with pytest.raises(ValueError, match="^ccal_detect_corners_batch: rel_threshold is not finite$"):
        ctx.detect_corners_batch(IMG2, rel_threshold=np.inf)
    with pytest.raises(ValueError, match=r"^detect_corners_batch: single-channel images \[n\]\[H\]\[W\]$"):
        ctx.detect_corners_batch(np.zeros((1, 4, 5, 3), dtype=np.uint8))


Q3 = [np.arange(16.0).reshape(2, 4, 2), np.zeros((0, 4, 2)), np.arange(16.0, 24.0).reshape(1, 4, 2)]


def test_decode_tags(stub, ctx):
    stub.void = {"ccal_decode_tags_batch": {5: (60, np.uint16, None)}}
    out = ctx.decode_tags_batch(IMG3, Q3, 16, [1, 2, 3])
    _eq(stub.last("ccal_decode_tags_batch"),
        [H(1), 1, 5, 4, 3, ("mem", up(0, 60, np.uint16)), i8(0, 2, 2, 3), up(0, 24), 4, 1, u8(1, 2, 3), 3, 3, 20.0, 0, 2,
         i4(-2, -2, -2), i4(-2, -2, -2), i4(-2, -2, -2), i4(-2, -2, -2), f8(*[NAN] * 24), u8(0, 0, 0), f8(NAN, NAN, NAN)])
    reason, tag_id, rot, ham, corners, code, margin = out
    _eq(reason, [i4(1600, 1601), i4(), i4(1602)]); _eq(tag_id, [i4(1700, 1701), i4(), i4(1702)])
    _eq(rot, [i4(1800, 1801), i4(), i4(1802)]); _eq(ham, [i4(1900, 1901), i4(), i4(1902)])
    _eq(corners, [up(2000, 16).reshape(2, 4, 2), np.zeros((0, 4, 2)), up(2016, 8).reshape(1, 4, 2)])
    _eq(code, [u8(2100, 2101), u8(), u8(2102)]); _eq(margin, [f8(2200, 2201), f8(), f8(2202)])
    out = ctx.decode_tags_dev(DEV, 0, 5, 4, 0, [], 9, [], 2, 4, 5, 1, 3)
    _eq(stub.last("ccal_decode_tags_dev"),
        [H(1), 0, 5, 4, 0, ("vp", DEV), i8(0), f8(), 3, 2, u8(), 0, 4, 5.0, 1, 3, i4(-2), i4(-2), i4(-2), i4(-2), f8(*[NAN] * 8), u8(0),
         f8(NAN)])
    _eq(out, ([], [], [], [], [], [], []))
    ctx.decode_tags_dev(DEV, 0, 5, 4, 1, [Q3[2]], 16, [2 ** 63])
    _eq(stub.last("ccal_decode_tags_dev"),
        [H(1), 0, 5, 4, 1, ("vp", DEV), i8(0, 1), up(16, 8), 4, 1, u8(2 ** 63), 1, 3, 20.0, 0, 2, i4(-2), i4(-2), i4(-2), i4(-2),
         f8(*[NAN] * 8), u8(0), f8(NAN)])
    with pytest.raises(ValueError, match="^ccal_decode_tags_batch: family_bits is not a square$"):
        ctx.decode_tags_batch(IMG3, Q3, 15, [1])
    with pytest.raises(ValueError, match="^ccal_decode_tags_dev: one array of quads per image$"):
        ctx.decode_tags_dev(DEV, 0, 5, 4, 2, [Q3[0]], 16, [1])
    with pytest.raises(ValueError, match=r"^decode_tags_batch: single-channel images \[n\]\[H\]\[W\]$"):
        ctx.decode_tags_batch(np.zeros((1, 4, 5, 3), dtype=np.uint8), Q3[:1], 16, [1])


def test_propose_quads(stub, ctx):
    stub.void = {"ccal_propose_quads_batch": {5: (60, np.uint16, None)}}
    stub.fill = {"ccal_propose_quads_batch": {15: [3, 0, 1], 16: [1, 0, 0]}}
    out = ctx.propose_quads_batch(IMG3, XY3, max_per_image=2)                # below the bound 8^3 * 2; count 3 > 2 rows
    _eq(stub.last("ccal_propose_quads_batch"),
        [H(1), 1, 5, 4, 3, ("mem", up(0, 60, np.uint16)), i8(0, 2, 2, 3), f8(1, 2, 3, 4, 5, 6), 20.0, 2.5, 2.0, 0.0625, 8, 40.0, 2,
         i4(0, 0, 0), i4(0, 0, 0), Some(np.int32, 24), Some(np.float64, 48)])
    _eq(out, [(up(1700, 8, np.int32).reshape(2, 4), up(1800, 16).reshape(2, 4, 2), 3, 1),
              (np.zeros((0, 4), np.int32), np.zeros((0, 4, 2)), 0, 0),
              (up(1716, 4, np.int32).reshape(1, 4), up(1832, 8).reshape(1, 4, 2), 1, 0)])
    assert out[0][0].flags.owndata and out[0][1].flags.owndata                # copies
    ctx.propose_quads_dev(DEV, 0, 5, 9, 3, XY3, 10, 30, 3, 0.125, 4, 5, 2000)     # above: 2000 -> 8^3 * 2
    _eq(stub.last("ccal_propose_quads_dev"),
        [H(1), 0, 5, 9, 3, ("vp", DEV), i8(0, 2, 2, 3), f8(1, 2, 3, 4, 5, 6), 10.0, 30.0, 3.0, 0.125, 4, 5.0, 1024, i4(0, 0, 0), i4(0, 0, 0),
         Some(np.int32, 3 * 1024 * 4), Some(np.float64, 3 * 1024 * 8)])
    out = ctx.propose_quads_dev(DEV, 0, 5, 9, 0, [])                             # no image: max_side from the sides, one row
    _eq(stub.last("ccal_propose_quads_dev"),
        [H(1), 0, 5, 9, 0, ("vp", DEV), i8(0), f8(), 20.0, 4.5, 2.0, 0.0625, 8, 40.0, 1, i4(0), i4(0), Some(np.int32, 4),
         Some(np.float64, 8)])
    assert out == []
    ctx.propose_quads_dev(DEV, 0, 5, 9, 1, [[]], max_per_image=0)                # no points, no room asked for
    _eq(stub.last("ccal_propose_quads_dev"),
        [H(1), 0, 5, 9, 1, ("vp", DEV), i8(0, 0), f8(), 20.0, 4.5, 2.0, 0.0625, 8, 40.0, 0, i4(0), i4(0), Some(np.int32, 4),
         Some(np.float64, 8)])
    with pytest.raises(ValueError, match="^ccal_propose_quads_dev: one array of points per image$"):
        ctx.propose_quads_dev(DEV, 0, 5, 9, 2, [[]])
    with pytest.raises(ValueError, match=r"^propose_quads_batch: single-channel images \[n\]\[H\]\[W\]$"):
        ctx.propose_quads_batch(np.zeros((1, 4, 5, 3), dtype=np.uint8), [[]])


FRONT = dict(step=1, nms_radius=5, min_response=1, rel_q10=102, cand_cap=4096, max_iterations=30, eps=1e-3)


def test_detect_tags(stub, ctx):
    stub.void = {"ccal_detect_tags_batch": {5: (40, np.uint8, None)}}
    stub.fill = {"ccal_detect_tags_batch": {10: [4, 1], 16: [8, 0]}}
    out = ctx.detect_tags_batch(IMG2, 16, [5, 6, 7])                           # max_side, offset, max_tags None; count 4 > 3 rows
    opts = dict(FRONT, half_win=4, merge_radius=1.0, min_side=20.0, max_side=2.5, max_side_ratio=2.0, offset=1.0 / 12.0,
                edge_min_contrast=40.0, edge_samples=8, quad_cap=1024, border=1, cell_samples=3, tag_min_contrast=40.0,
                max_border_errors=0, max_hamming=2, tag_cap=3)
    _eq(stub.last("ccal_detect_tags_batch"),
        [H(1), 0, 5, 4, 2, ("mem", up(0, 40, np.uint8)), 4, u8(5, 6, 7), 3, ("DetectTagsOpts", opts), i4(0, 0), i4(*[-2] * 6), i4(*[-2] * 6),
         i4(*[-2] * 6), f8(*[NAN] * 48), f8(*[NAN] * 6), i4(0, 0), i4(*[0] * 8)])
    _eq(out, [(i4(1100, 1101, 1102), i4(1200, 1201, 1202), i4(1300, 1301, 1302), up(1400, 24).reshape(3, 4, 2), f8(1500, 1501, 1502), 4, 8,
               i4(1700, 1701, 1702, 1703)),
              (i4(1103), i4(1203), i4(1303), up(1424, 8).reshape(1, 4, 2), f8(1503), 1, 0, i4(1704, 1705, 1706, 1707))])
    assert all(a.flags.owndata for a in out[0][:5]) and out[0][7].flags.owndata
    out = ctx.detect_tags_dev(DEV, 1, 5, 4, 0, 9, [5], 2, 3, 4, 0.25, 100, 6, 7, 0.5, 1.5, 11, 12, 3, 0.2, 5, 13, 50, 2, 4, 14, 1, 3, 2)
    opts = dict(step=2, nms_radius=3, min_response=4, rel_q10=256, cand_cap=100, half_win=6, max_iterations=7, eps=0.5, merge_radius=1.5,
                min_side=11.0, max_side=12.0, max_side_ratio=3.0, offset=0.2, edge_min_contrast=13.0, edge_samples=5, quad_cap=50,
                border=2, cell_samples=4, tag_min_contrast=14.0, max_border_errors=1, max_hamming=3, tag_cap=2)
    _eq(stub.last("ccal_detect_tags_dev"),
        [H(1), 1, 5, 4, 0, ("vp", DEV), 3, u8(5), 1, ("DetectTagsOpts", opts), i4(0), i4(-2, -2), i4(-2, -2), i4(-2, -2), f8(*[NAN] * 16),
         f8(NAN, NAN), i4(0), i4(0, 0, 0, 0)])
    assert out == []
    ctx.detect_tags_dev(DEV, 0, 8, 6, 1, 9, [], border=2)                      # an empty family: one row; offset from d and the border
    got = stub.last("ccal_detect_tags_dev")
    _eq(got[:9], [H(1), 0, 8, 6, 1, ("vp", DEV), 3, u8(), 0])
    _eq({k: got[9][1][k] for k in ("max_side", "offset", "tag_cap", "border")}, dict(max_side=4.0, offset=1.0 / 14.0, tag_cap=1, border=2))
    _eq(got[10:], [i4(0), i4(-2), i4(-2), i4(-2), f8(*[NAN] * 8), f8(NAN), i4(0), i4(0, 0, 0, 0)])
    with pytest.raises(ValueError, match="^ccal_detect_tags_dev: rel_threshold is not finite$"):
        ctx.detect_tags_dev(DEV, 0, 8, 6, 1, 9, [], rel_threshold=NAN)
    with pytest.raises(ValueError, match="^ccal_detect_tags_batch: family_bits is not a square$"):
        ctx.detect_tags_batch(IMG2, 10, [])
    with pytest.raises(ValueError, match=r"^detect_tags_batch: single-channel images \[n\]\[H\]\[W\]$"):
        ctx.detect_tags_batch(np.zeros((1, 4, 5, 3), dtype=np.uint8), 16, [])


def test_checkerboards(stub, ctx):
    hess = [[[1, 2, 3], [4, 5, 6]], np.zeros((0, 3)), [[7, 8, 9]]]
    stub.fill = {"ccal_assemble_checkerboards_batch": {7: [1, 0, 1]}}
    out = ctx.assemble_checkerboards_batch(XY3, hess, 2, 1.0)
    _eq(stub.last("ccal_assemble_checkerboards_batch"),
        [H(1), 3, i8(0, 2, 2, 3), f8(1, 2, 3, 4, 5, 6), f8(1, 2, 3, 4, 5, 6, 7, 8, 9), 2, 1, i4(-2, -2, -2), f8(*[NAN] * 12), i4(*[-2] * 6),
         i4(-2, -2, -2), i4(*[-2] * 12)])
    _eq(out, [(1, up(800, 4).reshape(2, 2), i4(900, 901), 1000, up(1100, 4, np.int32)), (0, None, None, 1001, up(1104, 4, np.int32)),
              (1, up(808, 4).reshape(2, 2), i4(904, 905), 1002, up(1108, 4, np.int32))])
    assert out[0][1].flags.owndata and out[0][2].flags.owndata and out[0][4].flags.owndata
    stub.fill = {}
    out = ctx.assemble_checkerboards_batch([], [], 0, 3)
    _eq(stub.last("ccal_assemble_checkerboards_batch"),
        [H(1), 0, i8(0), f8(), f8(), 0, 3, i4(-2), f8(NAN, NAN), i4(-2), i4(-2), i4(-2, -2, -2, -2)])
    assert out == []
    with pytest.raises(ValueError, match="^ccal_assemble_checkerboards_batch: one array of Hessians per array of positions$"):
        ctx.assemble_checkerboards_batch(XY3, hess[:2], 2, 1)
    with pytest.raises(ValueError, match="^ccal_assemble_checkerboards_batch: one Hessian per position$"):
        ctx.assemble_checkerboards_batch(XY3, [hess[0], hess[2], hess[1]], 2, 1)

    stub.void = {"ccal_detect_checkerboards_batch": {5: (40, np.uint8, None)}}
    stub.fill = {"ccal_detect_checkerboards_batch": {7: [0, 2]}}
    out = ctx.detect_checkerboards_batch(IMG2, 2, 1)
    _eq(stub.last("ccal_detect_checkerboards_batch"),
        [H(1), 0, 5, 4, 2, ("mem", up(0, 40, np.uint8)), ("DetectCheckerboardsOpts", dict(FRONT, half_win=5, cols=2, rows=1)), i4(0, 0),
         f8(*[NAN] * 8), i4(0, 0), i4(*[0] * 8)])
    _eq(out, [(0, None, 900, up(1000, 4, np.int32)), (2, up(804, 4).reshape(2, 2), 901, up(1004, 4, np.int32))])
    assert out[1][1].flags.owndata
    out = ctx.detect_checkerboards_dev(DEV, 1, 5, 4, 0, 3.0, 0, 2, 3, 4, 0.25, 100, 6, 7, 0.5)
    _eq(stub.last("ccal_detect_checkerboards_dev"),
        [H(1), 1, 5, 4, 0, ("vp", DEV),
         ("DetectCheckerboardsOpts", dict(step=2, nms_radius=3, min_response=4, rel_q10=256, cand_cap=100, half_win=6, max_iterations=7,
                                          eps=0.5, cols=3, rows=0)), i4(0), f8(NAN, NAN), i4(0), i4(0, 0, 0, 0)])
    assert out == []
    with pytest.raises(ValueError, match="^ccal_detect_checkerboards_dev: rel_threshold is not finite$"):
        ctx.detect_checkerboards_dev(DEV, 1, 5, 4, 1, 3, 2, rel_threshold=NAN)
    with pytest.raises(ValueError, match=r"^detect_checkerboards_batch: single-channel images \[n\]\[H\]\[W\]$"):
        ctx.detect_checkerboards_batch(np.zeros((1, 4, 5, 3), dtype=np.uint8), 2, 1)


BOARD = dict(kind=0, cols=3, rows=2, square=0.05, tag_size=0.0, tag_spacing=0.0, tag_rows=0, tag_cols=0, first_id=0, family_bits=0,
             n_codes=0, border=0)
RDEF = dict(supersample=0, black=0.0, white=0.0, background=0.0, margin=0.0)          # a fresh ccal_render_opts going into set_defaults
PHOTO = NS(blur_sigma=1, vignette=0.5, gain=2, noise_read=3, noise_shot=4, seed=-1, first_index=5.0)
PHOTO_F = dict(blur_sigma=1.0, vignette=0.5, gain=2.0, noise_read=3.0, noise_shot=4.0, seed=2 ** 64 - 1, first_index=5)


def test_render(stub, ctx):
    target = checkerboard_target(3.0, 2, 0.05)
    poses = np.arange(12.0).reshape(2, 6)
    stub.void = {"ccal_render_targets_batch": {10: (24, np.uint8, 9)}}
    out = ctx.render_targets_batch(2, PAR, 4, 3, poses, target)
    _eq(stub.calls[-2], ("ccal_render_set_defaults", [("RenderTarget", BOARD), ("RenderOpts", RDEF)]))
    _eq(stub.last("ccal_render_targets_batch"),
        [H(1), 2, f8(*PAR), 0, 4, 3, 2, up(0, 12), ("RenderTarget", BOARD),
         ("RenderOpts", dict(supersample=4, black=40.0, white=215.0, background=0.0, margin=0.03)), ("mem", Some(np.uint8, 24))])
    _eq(out, up(9, 24, np.uint8).reshape(2, 3, 4))
    stub.void = {"ccal_render_photo_targets": {11: (12, np.uint16, 9)}}
    out = ctx.render_targets_batch(2, PAR, 4, 3, poses[:1], target, np.uint16, 2.0, 1, 2, 3, 0.5, PHOTO)
    _eq(stub.last("ccal_render_photo_targets"),
        [H(1), 2, f8(*PAR), 1, 4, 3, 1, up(0, 6), ("RenderTarget", BOARD),
         ("RenderOpts", dict(supersample=2, black=1.0, white=2.0, background=3.0, margin=0.5)), ("PhotoOpts", PHOTO_F),
         ("mem", Some(np.uint16, 12))])
    _eq(out, up(9, 12, np.uint16).reshape(1, 3, 4))
    out = ctx.render_targets_batch(2, PAR, 4, 3, np.zeros((0, 6)), target)                  # no pose: a NULL block
    _eq(stub.last("ccal_render_targets_batch")[6:8] + stub.last()[10:], [0, f8(), ("vp", None)])
    assert out.shape == (0, 3, 4) and out.dtype == np.uint8
    assert ctx.render_targets_dev(DEV, 2, PAR, 1.0, 4.0, 3, poses, target, white=100) is None
    _eq(stub.last("ccal_render_targets_dev"),
        [H(1), 2, f8(*PAR), 1, 4, 3, 2, up(0, 12), ("RenderTarget", BOARD),
         ("RenderOpts", dict(supersample=4, black=40.0, white=100.0, background=0.0, margin=0.03)), ("vp", DEV)])
    ph = _ffi.PhotoOpts(gain=1.5)
    ctx.render_targets_dev(DEV, 2, PAR, 1, 4, 3, poses, target, photo=ph)
    got = stub.last("ccal_render_photo_targets_dev")
    _eq(got[10:], [("PhotoOpts", dict(blur_sigma=0.0, vignette=0.0, gain=1.5, noise_read=0.0, noise_shot=0.0, seed=0, first_index=0)),
                   ("vp", DEV)])
    with pytest.raises(ValueError, match="^render_targets_batch: uint8 or uint16 images$"):
        ctx.render_targets_batch(2, PAR, 4, 3, poses, target, np.int16)
    with pytest.raises(ValueError, match=r"^ccal_render_targets_batch: poses is an \[n, 6\] array of rvec, tvec$"):
        ctx.render_targets_batch(2, PAR, 4, 3, np.zeros(6), target)
    with pytest.raises(ValueError, match=r"^ccal_render_photo_targets: poses is an \[n, 6\] array of rvec, tvec$"):
        ctx.render_targets_batch(2, PAR, 4, 3, np.zeros(6), target, photo=ph)
    with pytest.raises(ValueError, match=r"^ccal_render_photo_targets_dev: poses is an \[n, 6\] array of rvec, tvec$"):
        ctx.render_targets_dev(DEV, 2, PAR, 1, 4, 3, np.zeros((2, 5)), target, photo=ph)


def test_pixel_stages(stub, ctx):
    assert ctx.photo_apply_dev(DEV, DEV + 64, 0, 1.0, 5, 4, 2, PHOTO) is None
    _eq(stub.last("ccal_photo_apply_dev"), [H(1), 0, 1, 5, 4, 2, ("vp", DEV), ("vp", DEV + 64), ("PhotoOpts", PHOTO_F)])
    assert ctx.normalize_dev(DEV, DEV + 64, 0, 1.0, 5, 4, 2) is None
    _eq(stub.calls[-2], ("ccal_normalize_set_defaults", [("NormalizeOpts", dict(radius=0, min_sigma=0.0, amp=0.0))]))
    _eq(stub.last("ccal_normalize_dev"),
        [H(1), 0, 1, 5, 4, 2, ("vp", DEV), ("vp", DEV + 64), ("NormalizeOpts", dict(radius=16, min_sigma=4.0, amp=64.0))])
    ctx.normalize_dev(DEV, DEV + 64, 0, 1, 5, 4, 2, NS(radius=3.0, min_sigma=1, amp=2))
    _eq(stub.last("ccal_normalize_dev")[8], ("NormalizeOpts", dict(radius=3, min_sigma=1.0, amp=2.0)))
    n = len(stub.calls)
    ctx.normalize_dev(DEV, DEV + 64, 0, 1, 5, 4, 2, _ffi.NormalizeOpts(radius=9))         # a ready struct: no set_defaults
    assert len(stub.calls) == n + 1
    _eq(stub.last("ccal_normalize_dev")[8], ("NormalizeOpts", dict(radius=9, min_sigma=0.0, amp=0.0)))
    assert ctx.grey_dev(DEV, DEV + 64, 5.0, 0, 1, 6, 4, 2) is None
    _eq(stub.calls[-2], ("ccal_grey_set_defaults", [("GreyOpts", dict(bin=0, w_r=0, w_g=0, w_b=0))]))
    _eq(stub.last("ccal_grey_dev"),
        [H(1), 5, 0, 1, 6, 4, 2, ("vp", DEV), ("vp", DEV + 64), ("GreyOpts", dict(bin=1, w_r=19595, w_g=38470, w_b=7471))])
    ctx.grey_dev(DEV, DEV + 64, 1, 0, 1, 6, 4, 2, NS(bin=2.0, w_r=1, w_g=2, w_b=3))
    _eq(stub.last("ccal_grey_dev")[9], ("GreyOpts", dict(bin=2, w_r=1, w_g=2, w_b=3)))
    n = len(stub.calls)
    ctx.grey_dev(DEV, DEV + 64, 1, 0, 1, 6, 4, 2, _ffi.GreyOpts(bin=4))
    assert len(stub.calls) == n + 1
    _eq(stub.last("ccal_grey_dev")[9], ("GreyOpts", dict(bin=4, w_r=0, w_g=0, w_b=0)))


def test_option_builders(stub):
    """The free builders: a ready struct passes through, None takes the library's defaults, anything else overrides them."""
    target = aprilgrid_target(0.1, 0.3, 2.0, 3, 4, 16, [1, 2], border=2)
    april = dict(kind=1, cols=0, rows=0, square=0.0, tag_size=0.1, tag_spacing=0.3, tag_rows=2, tag_cols=3, first_id=4, family_bits=16,
                 n_codes=2, border=2)
    _eq(np.ctypeslib.as_array(target.codes, shape=(2,)).copy(), u8(1, 2))
    o = render_opts(target, lib=stub)
    _eq(stub.last("ccal_render_set_defaults"), [("RenderTarget", april), ("RenderOpts", RDEF)])
    assert isinstance(o, _ffi.RenderOpts) and (o.supersample, o.black, o.white, o.background, o.margin) == (4, 40.0, 215.0, 0.0, 0.03)
    o = render_opts(target, 3.0, 1, 2, 3, 4)                                                # lib None: the loaded library
    assert (o.supersample, o.black, o.white, o.background, o.margin) == (3, 1.0, 2.0, 3.0, 4.0)
    assert not aprilgrid_target(0.1, 0.3, 2, 3, 4, 16, []).codes                            # no code: NULL

    ready = _ffi.NormalizeOpts(radius=2)
    assert normalize_opts(ready, lib=stub) is ready
    o = normalize_opts(lib=stub)
    assert isinstance(o, _ffi.NormalizeOpts) and (o.radius, o.min_sigma, o.amp) == (16, 4.0, 64.0)
    o = normalize_opts(NS(radius=5.0, min_sigma=2, amp=3))
    assert (o.radius, o.min_sigma, o.amp) == (5, 2.0, 3.0) and type(o.radius) is int

    ready = _ffi.GreyOpts(bin=2)
    assert grey_opts(ready, lib=stub) is ready
    o = grey_opts(lib=stub)
    assert isinstance(o, _ffi.GreyOpts) and (o.bin, o.w_r, o.w_g, o.w_b) == (1, 19595, 38470, 7471)
    o = grey_opts(NS(bin=2.0, w_r=3, w_g=4, w_b=5))
    assert (o.bin, o.w_r, o.w_g, o.w_b) == (2, 3, 4, 5)
    assert engine.grey_out_size(11, 7.0, 2) == (5, 3)

    ph = _ffi.PhotoOpts()
    assert engine.photo_opts(ph) is ph
    radius, taps, sigma = photo_tables(PHOTO, lib=stub)
    _eq(stub.last("ccal_photo_tables"), [("PhotoOpts", PHOTO_F), "i32*", f8(*[0] * 17), f8(*[0] * 256)])
    assert radius == 10 and type(radius) is int
    _eq(taps, up(200, 17)); _eq(sigma, up(300, 256))
    stub.rc["ccal_photo_tables"] = _ffi.ERR_INVALID_ARG
    with pytest.raises(ValueError, match=r"^photo_tables: an option is out of range \(include/ccal.h, the photometric stage\)$"):
        photo_tables(PHOTO)

    o = engine.default_opts(_ffi.METHOD_LM, max_iterations=7)
    _eq(stub.last("ccal_set_defaults")[0][0], "SolverOpts")
    assert (o.method, o.max_iterations) == (1, 7)


# ---------------------------------------------------------------------------------------------------------------------------------
# Problem, MultiContext / MultiProblem, the sharded solve
def _desc(n_slots=2):
    """One camera, n_slots frame slots with an observation each: 3 and 4 corners (or none at all)."""
    offs = [0, 3, 7][:n_slots + 1]
    c = np.arange(float(offs[-1]))
    return make_desc(1, [2], [640], [480], False, n_slots, [0] * n_slots, list(range(n_slots)), offs, c, c + 10, c + 20, c + 30, c + 40, 1.5)


DESC_F = dict(n_cams=1, xy_same_focal=0, n_slots=2, n_obs=2, huber_delta=1.5)
INTR = np.arange(1.0, 11.0).reshape(1, 10)
POSES = np.arange(12.0).reshape(2, 6)
EXTR = np.arange(20.0, 26.0).reshape(1, 6)
PARAMS3 = [up(1, 10), up(0, 12), up(20, 6)]
ZEXTR = [up(1, 10), up(0, 12), f8(*[0] * 6)]
OPTS_F = dict(method=0, max_iterations=100, min_abs_error_decrease=0.0, min_rel_error_decrease=0.0, min_error=0.0, lm_initial_radius=0.0,
              lm_min_diagonal=0.0, lm_max_diagonal=0.0, verbose=0, timeout_s=0, error_metric=0)
REP0 = dict(status=0, iterations=0, lm_accepted=0, lm_rejected=0, initial_cost=0.0, final_cost=0.0, solve_ms=0.0, lm_spec_hits=0,
            lm_spec_misses=0)


def test_make_desc():
    d, keep = _desc()
    assert {f: getattr(d, f) for f in DESC_F} == DESC_F
    _eq(keep["model"], i4(2)); _eq(keep["width"], f8(640)); _eq(keep["obs_offsets"], i8(0, 3, 7)); _eq(keep["obs_slot"], i4(0, 1))
    _eq(keep["x"], up(0, 7, np.float32)); _eq(keep["v"], up(40, 7, np.float32))
    for field, key in (("model", "model"), ("width", "width"), ("height", "height"), ("obs_cam", "obs_cam"), ("obs_slot", "obs_slot"),
                       ("obs_offsets", "obs_offsets"), ("p3d_x", "x"), ("p3d_y", "y"), ("p3d_z", "z"), ("p2d_u", "u"), ("p2d_v", "v")):
        assert C.addressof(getattr(d, field).contents) == keep[key].ctypes.data, field
    _eq(partition_slots(d, 2, lib=_Stub()), [200, 201, 202])


def _problem_common(stub, p, pre, h):
    """The eleven methods Problem and MultiProblem share, under the C prefix `pre`; h: the problem's handle as the library sees it."""
    assert (p.n_cams, p.n_slots, p.n_obs) == (1, 2, 2)
    assert p.set_bounds(0, 1, 0.5, 2) is None
    _eq(stub.last(pre + "set_bounds"), [h, 0, 1, 0.5, 2])
    p.fix_param(0, 3); _eq(stub.last(pre + "fix_param"), [h, 0, 3])
    p.unfix_param(0, 3); _eq(stub.last(pre + "unfix_param"), [h, 0, 3])
    p.apply_reference_bounds(); _eq(stub.last(pre + "apply_reference_bounds"), [h])
    assert p.disable_distortions(2, INTR) is None
    _eq(stub.last(pre + "disable_distortions"), [h, 2, up(1, 10)])
    assert p.upload_params(INTR, POSES) is None
    _eq(stub.last(pre + "upload_params"), [h] + ZEXTR)
    p.upload_params(INTR.ravel().tolist(), POSES.ravel(), EXTR)
    _eq(stub.last(pre + "upload_params"), [h] + PARAMS3)
    with pytest.raises(ValueError):
        p.upload_params(INTR, POSES[:1])
    poses, used = p.init_poses(INTR, 12.0)
    _eq(stub.last(pre + "init_poses"), [h, up(1, 10), 12, f8(*[0] * 12), i4(0, 0)])
    _eq(poses, up(300, 12).reshape(2, 6)); _eq(used, i4(400, 401))
    poses, used = p.init_poses(INTR)
    assert stub.last(pre + "init_poses")[2] == 10
    _eq(p.validation(0, INTR, POSES), (5.5, 6.5))
    _eq(stub.last(pre + "validation"), [h, 0] + ZEXTR + ["f64*", "f64*"])
    p.validation(0, INTR, POSES, EXTR)
    _eq(stub.last(pre + "validation"), [h, 0] + PARAMS3 + ["f64*", "f64*"])
    _eq(list(p._params(INTR, POSES, None)), [INTR, POSES, np.zeros((1, 6))])


def test_problem(stub, ctx, monkeypatch):
    d, keep = _desc()
    p = Problem(ctx, d, keep)
    _eq(stub.last("ccal_problem_create"), [H(1), ("ProblemDesc", DESC_F), ("new", 0x2000)])
    assert (p.ctx, p.lib, p._keep, p.n_corners, p.K, p.j_len, p.block_dim(), p.eff_num_params(1)) == (ctx, stub, keep, 7, 5, 11, 4, 6)
    assert p in ctx._problems
    h = H(2)
    _problem_common(stub, p, "ccal_", h)

    p.set_allreduce(None); _eq(stub.last("ccal_set_allreduce"), [h, ("fn", False), None]); assert p._cb is None
    p.set_allreduce(lambda ptr, count, stream: 0); _eq(stub.last("ccal_set_allreduce"), [h, ("fn", True), None]); assert p._cb is not None
    p.set_rccl_comm(0x9000); _eq(stub.last("ccal_set_rccl_comm"), [h, ("vp", 0x9000)])
    p.set_rccl_comm(None); _eq(stub.last("ccal_set_rccl_comm"), [h, None])

    r, J = p.eval(INTR, POSES, apply_loss=True)
    _eq(stub.last("ccal_eval"), [h] + ZEXTR + [1, Some(np.float64, 14), Some(np.float64, 11)])
    _eq(r, up(500, 14).reshape(7, 2)); _eq(J, up(600, 11))
    p.eval(INTR, POSES, EXTR); _eq(stub.last("ccal_eval")[:5], [h] + PARAMS3 + [0])
    _eq(p.download_params(), (up(100, 10).reshape(1, 10), up(200, 12).reshape(2, 6), up(300, 6).reshape(1, 6)))
    _eq(stub.last("ccal_download_params"), [h, f8(*[0] * 10), f8(*[0] * 12), f8(*[0] * 6)])
    p.eval_dev(DEV, DEV + 64); _eq(stub.last("ccal_eval_dev"), [h, 0, ("vp", DEV), ("vp", DEV + 64)])
    p.eval_dev(DEV, DEV + 64, True); _eq(stub.last("ccal_eval_dev"), [h, 1, ("vp", DEV), ("vp", DEV + 64)])
    S, b, cost = p.build_normal(INTR, POSES, EXTR, lam=2)
    _eq(stub.last("ccal_build_normal"), [h] + PARAMS3 + [2.0, Some(np.float64, 25), Some(np.float64, 5), "f64*"])
    _eq(S, up(500, 25).reshape(5, 5)); _eq(b, up(600, 5)); assert cost == 7.5
    p.build_normal_dev(); _eq(stub.last("ccal_build_normal_dev"), [h, 0.0])
    p.build_normal_dev(3); _eq(stub.last("ccal_build_normal_dev"), [h, 3.0])
    poses, used = p.init_poses_division(-0.5, 12.0)
    _eq(stub.last("ccal_init_poses_division"), [h, -0.5, 12, f8(*[0] * 12), i4(0, 0)])
    _eq(poses, up(300, 12).reshape(2, 6)); _eq(used, i4(400, 401))
    _eq(p.reprojection_errors(INTR, POSES), up(400, 7))
    _eq(stub.last("ccal_reprojection_errors"), [h] + ZEXTR + [Some(np.float64, 7)])

    # the solve forms
    intr, poses, extr, rep = p.solve(INTR, POSES)                              # opts None: default_opts() of the loaded library
    _eq(stub.last("ccal_solve"), [h, ("SolverOpts", OPTS_F)] + ZEXTR + [("Report", REP0)])
    _eq([intr, poses, extr], [up(200, 10).reshape(1, 10), up(300, 12).reshape(2, 6), up(400, 6).reshape(1, 6)])
    assert rep.iterations == 3 and INTR[0, 0] == 1.0 and POSES[0, 1] == 1.0    # copies went to the library
    opts = _ffi.SolverOpts(method=1, max_iterations=9)
    p.solve(INTR, POSES, EXTR, opts)
    _eq(stub.last("ccal_solve"), [h, ("SolverOpts", dict(OPTS_F, method=1, max_iterations=9))] + PARAMS3 + [("Report", REP0)])
    intr, poses, extr, rep = p.solve(INTR, POSES, opts=opts, pinned=True)
    pin = p._pin_poses
    assert pin.shape == (2, 6) and poses.base is pin
    assert [c[0] for c in stub.calls[-2:]] == ["ccal_pin_buffer", "ccal_solve"]
    _eq(stub.calls[-2][1], [H(1), ("vp", pin.ctypes.data), 96])
    _eq(stub.last("ccal_solve")[2:5], ZEXTR)
    n = len(stub.calls)
    p.solve(INTR, POSES, opts=opts, pinned=True)                               # pinned once per problem
    assert len(stub.calls) == n + 1 and p._pin_poses is pin
    rep = p.solve_dev(opts)
    _eq(stub.last("ccal_solve_dev"), [h, ("SolverOpts", dict(OPTS_F, method=1, max_iterations=9)), ("Report", REP0)])
    assert isinstance(rep, _ffi.Report) and rep.iterations == 4
    p.solve_dev(); _eq(stub.last("ccal_solve_dev")[1], ("SolverOpts", OPTS_F))

    reps, results = Problem.solve_batch([p, p], opts)
    _eq(stub.last("ccal_solve_batch"), [("vps", [0x2000, 0x2000]), 2, ("SolverOpts", dict(OPTS_F, method=1, max_iterations=9)), None, None,
                                        None, ("structs", "Report", 2)])
    assert results is None and len(reps) == 2 and isinstance(reps[0], _ffi.Report)
    reps, results = Problem.solve_batch([p], starts=[(INTR, POSES, None)])
    _eq(stub.last("ccal_solve_batch"), [("vps", [0x2000]), 1, ("SolverOpts", OPTS_F), ("ptrs", [up(1, 10)]), ("ptrs", [up(0, 12)]),
                                        ("ptrs", [f8(*[0] * 6)]), ("structs", "Report", 1)])
    _eq(results, [(INTR, POSES, np.zeros((1, 6)))])
    reps, results = Problem.solve_batch([])
    _eq(stub.last("ccal_solve_batch"), [("vps", [None]), 0, ("SolverOpts", OPTS_F), None, None, None, ("structs", "Report", 1)])
    assert reps == [] and results is None

    # the sharded solve over problems of the caller's
    intr, poses, extr, rep = solve_sharded([p, p], INTR, [POSES, POSES + 1], opts=opts)
    _eq(stub.last("ccal_solve_sharded"),
        [("vps", [0x2000, 0x2000]), 2, ("SolverOpts", dict(OPTS_F, method=1, max_iterations=9)), up(1, 10), ("ptrs", [up(0, 12), up(1, 12)]),
         f8(*[0] * 6), ("Report", REP0)])
    _eq(intr, up(300, 10).reshape(1, 10)); _eq(poses, [POSES, POSES + 1]); _eq(extr, up(500, 6).reshape(1, 6)); assert rep.iterations == 6
    solve_sharded([p], INTR, [POSES], EXTR)
    _eq(stub.last("ccal_solve_sharded")[2:6], [("SolverOpts", OPTS_F), up(1, 10), ("ptrs", [up(0, 12)]), up(20, 6)])


def test_covariance(stub, ctx):
    d, keep = _desc()
    p = Problem(ctx, d, keep)
    h = H(2)
    c = p.covariance()
    _eq(stub.last("ccal_covariance"),
        [h, None, None, None, f8(*[NAN] * 25), f8(*[NAN] * 72), f8(*[NAN] * 7), i4(-2, -2),
         ("CovReport", dict(status=0, bad_slot=0, dof=0, n_free=0, n_posed=0, cost=0.0, sigma2=0.0, leverage_sum=0.0))])
    _eq(c.cov_cam, up(400, 25).reshape(5, 5)); _eq(c.cov_poses, up(500, 72).reshape(2, 6, 6)); _eq(c.leverage, up(600, 7))
    _eq(c.slot_status, i4(700, 701)); assert isinstance(c.report, _ffi.CovReport) and c.report.bad_slot == 1
    c = p.covariance(INTR, POSES, poses_cov=False)
    _eq(stub.last("ccal_covariance")[:8], [h] + ZEXTR + [f8(*[NAN] * 25), None, f8(*[NAN] * 7), i4(-2, -2)])
    assert c.cov_poses is None and c.leverage is not None
    c = p.covariance(INTR, POSES, EXTR, leverage=False)
    _eq(stub.last("ccal_covariance")[:8], [h] + PARAMS3 + [f8(*[NAN] * 25), f8(*[NAN] * 72), None, i4(-2, -2)])
    assert c.leverage is None and c.cov_poses.shape == (2, 6, 6)
    with pytest.raises(ValueError, match=r"^covariance: poses / extr without intr \(intr None means the point on the device\)$"):
        p.covariance(poses=POSES)
    with pytest.raises(ValueError, match="^covariance: poses is missing$"):
        p.covariance(INTR)
    # no slot at all: the outputs padded to one slot, and cut back to none
    stub.n_slots = stub.n_obs = 0
    d0, keep0 = _desc(0)
    p0 = Problem(ctx, d0, keep0)
    c = p0.covariance(INTR)
    _eq(stub.last("ccal_covariance")[:8], [H(3), up(1, 10), f8(), f8(*[0] * 6), f8(*[NAN] * 25), f8(*[NAN] * 36), f8(*[NAN] * 7), i4(-2)])
    assert c.cov_poses.shape == (0, 6, 6) and c.slot_status.shape == (0,)
    poses, used = p0.init_poses(INTR)
    _eq(stub.last("ccal_init_poses")[3:], [f8(*[0] * 6), i4(0)])
    assert poses.shape == (0, 6) and used.shape == (0,)
    # CCAL_ERR_NOT_PD passes only where the caller asks for it; every other code raises either way
    stub.rc["ccal_covariance"] = _ffi.ERR_NOT_PD
    assert p0.covariance(INTR, raise_on_error=False).report.bad_slot == 1
    with pytest.raises(CcalError) as e:
        p0.covariance(INTR)
    assert e.value.code == _ffi.ERR_NOT_PD and str(e.value) == "ccal_covariance: CCAL_ERR_NOT_PD (ctx detail)"
    stub.rc["ccal_covariance"] = _ffi.ERR_HIP
    with pytest.raises(CcalError) as e:
        p0.covariance(INTR, raise_on_error=False)
    assert e.value.code == _ffi.ERR_HIP and str(e.value) == "ccal_covariance: CCAL_ERR_HIP (ctx detail)"


def test_multi(stub):
    m = MultiContext([0, 0.0, 1], lib=stub)
    _eq(stub.last("ccal_multi_create_transport"), [i4(0, 0, 1), 3, -1, ("new", 0x1000)])
    assert m.devices == [0, 0, 1] and type(m.devices[1]) is int and m.transport == 2 and m.rccl_ranks == 0 and m.last_error() == "multi detail"
    m1 = MultiContext([2], transport=1.0, lib=stub)          # (held: a dropped set is destroyed)
    _eq(stub.last("ccal_multi_create_transport"), [i4(2), 1, 1, ("new", 0x2000)])
    m.sync(); _eq(stub.last("ccal_multi_sync"), [H(1)])
    m.set_model_conventions(None); _eq(stub.last("ccal_multi_set_model_conventions"), [H(1), None])
    m.set_model_conventions(_ffi.ModelConventions(kb4_small_radius=0.5))
    _eq(stub.last("ccal_multi_set_model_conventions"), [H(1), ("ModelConventions", dict(kb4_small_radius=0.5, unproject_small_radius=0.0))])

    d, keep = _desc()
    p = MultiProblem(m, d, keep)
    _eq(stub.last("ccal_multi_problem_create"), [H(1), ("ProblemDesc", DESC_F), ("new", 0x3000)])
    assert (p.mctx, p.lib, p._keep, p.n_shards) == (m, stub, keep, 2) and p in m._problems
    h = H(3)
    _problem_common(stub, p, "ccal_multi_", h)
    _eq(p.slot_range(1), (20, 30)); _eq(stub.last("ccal_multi_problem_slot_range"), [h, 1, "i32*", "i32*"])
    assert p.shard_handle(1).value == 0x5000 and p.shard_sizes(0) == (7, 11)
    p.eval_dev([DEV, DEV + 8], [DEV + 16, DEV + 24])
    _eq(stub.last("ccal_multi_eval_dev"), [h, 0, ("vps", [DEV, DEV + 8]), ("vps", [DEV + 16, DEV + 24])])
    p.eval_dev([DEV, DEV + 8], [DEV + 16, DEV + 24], apply_loss=1)
    assert stub.last("ccal_multi_eval_dev")[1] == 1
    _eq(p.reprojection_errors(INTR, POSES), up(400, 7))
    _eq(stub.last("ccal_multi_reprojection_errors"), [h] + ZEXTR + [Some(np.float64, 7), i8(0, 3, 7)])
    intr, poses, extr, rep = p.solve(INTR, POSES, EXTR)
    _eq(stub.last("ccal_multi_solve"), [h, ("SolverOpts", OPTS_F)] + PARAMS3 + [("Report", REP0)])
    _eq([intr, poses, extr], [up(200, 10).reshape(1, 10), up(300, 12).reshape(2, 6), up(400, 6).reshape(1, 6)])
    assert rep.iterations == 5 and INTR[0, 0] == 1.0


def test_from_synth(stub, ctx):
    sp = NS(n_cams=1, model=[2], width=[640], height=[480], xy_same_focal=True, n_slots=2, obs_cam=[0, 0], obs_slot=[0, 1],
            obs_offsets=[0, 3, 7], huber_delta=2.0, soa=lambda: tuple(np.arange(7.0) + k for k in range(5)))
    p = Problem.from_synth(ctx, sp)
    _eq(stub.last("ccal_problem_create")[1], ("ProblemDesc", dict(DESC_F, xy_same_focal=1, huber_delta=2.0)))
    assert type(p) is Problem and sorted(p._keep) == sorted(["model", "width", "height", "obs_cam", "obs_slot", "obs_offsets", "x", "y", "z",
                                                              "u", "v"])
    m = MultiContext([0], lib=stub)
    mp = MultiProblem.from_synth(m, sp)
    _eq(stub.last("ccal_multi_problem_create")[1], ("ProblemDesc", dict(DESC_F, xy_same_focal=1, huber_delta=2.0)))
    assert type(mp) is MultiProblem and mp._keep["obs_offsets"].tolist() == [0, 3, 7]


# ---------------------------------------------------------------------------------------------------------------------------------
# errors: the `where` of every wrapped entry point and which of them carry a detail
def _error_cases():
    """(the library function that fails, the CcalError text after the status name, the call) for every wrapped entry point."""
    c, m = " (ctx detail)", " (multi detail)"
    t = checkerboard_target(3, 2, 0.05)
    xm = np.zeros((2, 3), dtype=np.float32)
    opts = _ffi.SolverOpts()
    E = lambda fn, call, tail=c, where=None: (fn, (where or fn), tail, call)
    return [
        E("ccal_sync", lambda e: e.ctx.sync()),
        E("ccal_pin_buffer", lambda e: e.ctx.pin(np.zeros(3))),
        E("ccal_unpin_buffer", lambda e: e.ctx.unpin(np.zeros(3))),
        E("ccal_get_model_conventions", lambda e: e.ctx.model_conventions(), ""),
        E("ccal_set_model_conventions", lambda e: e.ctx.set_model_conventions(None), ""),
        E("ccal_rccl_comm_create", lambda e: e.ctx.rccl_comm_create(1, 0, bytes(128))),
        E("ccal_rdh_batch", lambda e: e.ctx.rdh_batch([], [])),
        E("ccal_pnp_batch", lambda e: e.ctx.pnp_batch([], [])),
        E("ccal_refine_poses_batch", lambda e: e.ctx.refine_poses_batch(1, PAR, [], [], np.zeros((0, 6)))),
        E("ccal_refine_rig_poses_batch", lambda e: e.ctx.refine_rig_poses_batch([1], [PAR], np.zeros((1, 6)), [], np.zeros((0, 6)))),
        E("ccal_project_points", lambda e: e.ctx.project_points(1, PAR, np.zeros((0, 3)))),
        E("ccal_unproject_points", lambda e: e.ctx.unproject_points(1, PAR, np.zeros((0, 2)))),
        E("ccal_estimate_new_camera_matrix", lambda e: e.ctx.estimate_new_camera_matrix(1, PAR, 4, 3, 0.0)),
        E("ccal_undistort_map_create", lambda e: e.ctx.undistort_map(1, PAR, np.eye(3), (4, 3))),
        E("ccal_undistort_map_from_host", lambda e: e.ctx.undistort_map_from_arrays(xm, xm)),
        E("ccal_refine_corners_batch", lambda e: e.ctx.refine_corners_batch(IMG2, [[], []])),
        E("ccal_refine_corners_dev", lambda e: e.ctx.refine_corners_dev(DEV, 0, 5, 4, 0, [])),
        E("ccal_detect_corners_batch", lambda e: e.ctx.detect_corners_batch(IMG2)),
        E("ccal_detect_corners_dev", lambda e: e.ctx.detect_corners_dev(DEV, 0, 5, 4, 0)),
        E("ccal_decode_tags_batch", lambda e: e.ctx.decode_tags_batch(IMG2, [[], []], 16, [1])),
        E("ccal_decode_tags_dev", lambda e: e.ctx.decode_tags_dev(DEV, 0, 5, 4, 0, [], 16, [1])),
        E("ccal_propose_quads_batch", lambda e: e.ctx.propose_quads_batch(IMG2, [[], []])),
        E("ccal_propose_quads_dev", lambda e: e.ctx.propose_quads_dev(DEV, 0, 5, 4, 0, [])),
        E("ccal_detect_tags_batch", lambda e: e.ctx.detect_tags_batch(IMG2, 16, [1])),
        E("ccal_detect_tags_dev", lambda e: e.ctx.detect_tags_dev(DEV, 0, 5, 4, 0, 16, [1])),
        E("ccal_assemble_checkerboards_batch", lambda e: e.ctx.assemble_checkerboards_batch([], [], 2, 2)),
        E("ccal_detect_checkerboards_batch", lambda e: e.ctx.detect_checkerboards_batch(IMG2, 2, 2)),
        E("ccal_detect_checkerboards_dev", lambda e: e.ctx.detect_checkerboards_dev(DEV, 0, 5, 4, 0, 2, 2)),
        E("ccal_render_set_defaults", lambda e: e.ctx.render_targets_dev(DEV, 1, PAR, 0, 4, 3, np.zeros((0, 6)), t), ""),
        E("ccal_render_targets_batch", lambda e: e.ctx.render_targets_batch(1, PAR, 4, 3, np.zeros((0, 6)), t)),
        E("ccal_render_targets_dev", lambda e: e.ctx.render_targets_dev(DEV, 1, PAR, 0, 4, 3, np.zeros((0, 6)), t)),
        E("ccal_render_photo_targets", lambda e: e.ctx.render_targets_batch(1, PAR, 4, 3, np.zeros((0, 6)), t, photo=PHOTO)),
        E("ccal_render_photo_targets_dev", lambda e: e.ctx.render_targets_dev(DEV, 1, PAR, 0, 4, 3, np.zeros((0, 6)), t, photo=PHOTO)),
        E("ccal_photo_apply_dev", lambda e: e.ctx.photo_apply_dev(DEV, DEV, 0, 0, 5, 4, 1, PHOTO)),
        E("ccal_normalize_dev", lambda e: e.ctx.normalize_dev(DEV, DEV, 0, 0, 5, 4, 1)),
        E("ccal_normalize_set_defaults", lambda e: e.ctx.normalize_dev(DEV, DEV, 0, 0, 5, 4, 1), ""),
        E("ccal_grey_dev", lambda e: e.ctx.grey_dev(DEV, DEV, 1, 0, 0, 5, 4, 1)),
        E("ccal_grey_set_defaults", lambda e: e.ctx.grey_dev(DEV, DEV, 1, 0, 0, 5, 4, 1), ""),
        E("ccal_render_set_defaults", lambda e: render_opts(t), ""),
        E("ccal_normalize_set_defaults", lambda e: normalize_opts(), ""),
        E("ccal_grey_set_defaults", lambda e: grey_opts(), ""),
        E("ccal_partition_slots", lambda e: partition_slots(e.desc, 2), ""),
        E("ccal_rccl_unique_id", lambda e: engine.rccl_unique_id(), ""),
        E("ccal_undistort_map_download", lambda e: e.map.download()),
        E("ccal_remap", lambda e: e.map.remap(IMG2)),
        E("ccal_remap_dev", lambda e: e.map.remap_dev(DEV, DEV, 0, 1, 5, 4, 1)),
        E("ccal_problem_create", lambda e: Problem(e.ctx, e.desc)),
        E("ccal_set_bounds", lambda e: e.p.set_bounds(0, 0, 0.0, 1.0)),
        E("ccal_fix_param", lambda e: e.p.fix_param(0, 0)),
        E("ccal_unfix_param", lambda e: e.p.unfix_param(0, 0)),
        E("ccal_apply_reference_bounds", lambda e: e.p.apply_reference_bounds()),
        E("ccal_disable_distortions", lambda e: e.p.disable_distortions(1, INTR)),
        E("ccal_set_allreduce", lambda e: e.p.set_allreduce(None)),
        E("ccal_set_allreduce", lambda e: e.p.set_allreduce(lambda *a: 0)),
        E("ccal_set_rccl_comm", lambda e: e.p.set_rccl_comm(None)),
        E("ccal_eval", lambda e: e.p.eval(INTR, POSES)),
        E("ccal_upload_params", lambda e: e.p.upload_params(INTR, POSES)),
        E("ccal_download_params", lambda e: e.p.download_params()),
        E("ccal_eval_dev", lambda e: e.p.eval_dev(DEV, DEV)),
        E("ccal_build_normal", lambda e: e.p.build_normal(INTR, POSES)),
        E("ccal_build_normal_dev", lambda e: e.p.build_normal_dev()),
        E("ccal_solve", lambda e: e.p.solve(INTR, POSES, opts=opts)),
        E("ccal_pin_buffer", lambda e: e.p.solve(INTR, POSES, opts=opts, pinned=True)),
        E("ccal_solve_dev", lambda e: e.p.solve_dev(opts)),
        E("ccal_solve_batch", lambda e: Problem.solve_batch([e.p], opts)),
        E("ccal_solve_batch", lambda e: Problem.solve_batch([], opts), ""),
        E("ccal_solve_sharded", lambda e: solve_sharded([e.p], INTR, [POSES], opts=opts)),
        E("ccal_init_poses", lambda e: e.p.init_poses(INTR)),
        E("ccal_init_poses_division", lambda e: e.p.init_poses_division(0.0)),
        E("ccal_reprojection_errors", lambda e: e.p.reprojection_errors(INTR, POSES)),
        E("ccal_validation", lambda e: e.p.validation(0, INTR, POSES)),
        E("ccal_covariance", lambda e: e.p.covariance()),
        E("ccal_multi_create_transport", lambda e: MultiContext([0], lib=e.stub), " (create detail)", "ccal_multi_create"),
        E("ccal_multi_set_model_conventions", lambda e: e.m.set_model_conventions(None), ""),
        E("ccal_multi_sync", lambda e: e.m.sync(), m),
        E("ccal_multi_problem_create", lambda e: MultiProblem(e.m, e.desc), m),
        E("ccal_multi_problem_slot_range", lambda e: e.mp.slot_range(0), m),
        E("ccal_multi_set_bounds", lambda e: e.mp.set_bounds(0, 0, 0.0, 1.0), m),
        E("ccal_multi_fix_param", lambda e: e.mp.fix_param(0, 0), m),
        E("ccal_multi_unfix_param", lambda e: e.mp.unfix_param(0, 0), m),
        E("ccal_multi_apply_reference_bounds", lambda e: e.mp.apply_reference_bounds(), m),
        E("ccal_multi_disable_distortions", lambda e: e.mp.disable_distortions(1, INTR), m),
        E("ccal_multi_upload_params", lambda e: e.mp.upload_params(INTR, POSES), m),
        E("ccal_multi_eval_dev", lambda e: e.mp.eval_dev([DEV, DEV], [DEV, DEV]), m),
        E("ccal_multi_init_poses", lambda e: e.mp.init_poses(INTR), m),
        E("ccal_multi_validation", lambda e: e.mp.validation(0, INTR, POSES), m),
        E("ccal_multi_reprojection_errors", lambda e: e.mp.reprojection_errors(INTR, POSES), m),
        E("ccal_multi_solve", lambda e: e.mp.solve(INTR, POSES, opts=opts), m),
    ]


ERROR_CASES = _error_cases()


@pytest.fixture
def env(stub):
    e = NS(stub=stub, ctx=Context(lib=stub), m=MultiContext([0, 1], lib=stub))
    e.desc, e.keep = _desc()
    e.p, e.mp = Problem(e.ctx, e.desc, e.keep), MultiProblem(e.m, e.desc, e.keep)
    e.map = e.ctx.undistort_map_from_arrays(np.zeros((2, 3), dtype=np.float32), np.zeros((2, 3), dtype=np.float32))
    return e


@pytest.mark.parametrize("k", range(len(ERROR_CASES)), ids=[f"{c[0]}-{k}" for k, c in enumerate(ERROR_CASES)])
def test_error_text(env, k):
    fn, where, tail, call = ERROR_CASES[k]
    env.stub.rc[fn] = _ffi.ERR_INVALID_ARG
    with pytest.raises(CcalError) as e:
        call(env)
    assert e.value.code == _ffi.ERR_INVALID_ARG and str(e.value) == f"{where}: CCAL_ERR_INVALID_ARG{tail}"
    env.stub.rc[fn] = 77                                                       # a code without a name
    with pytest.raises(CcalError) as e:
        call(env)
    assert e.value.code == 77 and str(e.value) == f"{where}: 77{tail}"


def test_ctx_create_error(stub):
    stub.rc["ccal_ctx_create"] = _ffi.ERR_HIP
    with pytest.raises(CcalError) as e:
        Context(lib=stub)
    assert e.value.code == _ffi.ERR_HIP and str(e.value) == "ccal_ctx_create: CCAL_ERR_HIP (no usable HIP device)"
    stub.rc["ccal_ctx_create"] = _ffi.ERR_NO_MEMORY
    with pytest.raises(CcalError) as e:
        Context(lib=stub)
    assert e.value.code == _ffi.ERR_NO_MEMORY and str(e.value) == "ccal_ctx_create: CCAL_ERR_NO_MEMORY"


SOLVES = [("ccal_solve", " (ctx detail)", lambda e, **kw: e.p.solve(INTR, POSES, opts=_ffi.SolverOpts(), **kw)),
          ("ccal_solve_dev", " (ctx detail)", lambda e, **kw: e.p.solve_dev(_ffi.SolverOpts(), **kw)),
          ("ccal_multi_solve", " (multi detail)", lambda e, **kw: e.mp.solve(INTR, POSES, opts=_ffi.SolverOpts(), **kw)),
          ("ccal_solve_sharded", " (ctx detail)", lambda e, **kw: solve_sharded([e.p], INTR, [POSES], opts=_ffi.SolverOpts(), **kw))]


@pytest.mark.parametrize("fn, tail, call", SOLVES, ids=[s[0] for s in SOLVES])
def test_solve_forms_status(env, fn, tail, call):
    """CCAL_ERR_NO_CONVERGENCE always comes back as a result; every other code only with raise_on_error=False."""
    env.stub.rc[fn] = _ffi.ERR_NO_CONVERGENCE
    rep = call(env)
    assert isinstance(rep if fn == "ccal_solve_dev" else rep[3], _ffi.Report)
    call(env, raise_on_error=False)
    env.stub.rc[fn] = _ffi.ERR_NONFINITE
    with pytest.raises(CcalError) as e:
        call(env)
    assert e.value.code == _ffi.ERR_NONFINITE and str(e.value) == f"{fn}: CCAL_ERR_NONFINITE{tail}"
    rep = call(env, raise_on_error=False)
    assert isinstance(rep if fn == "ccal_solve_dev" else rep[3], _ffi.Report)


# ---------------------------------------------------------------------------------------------------------------------------------
# lifetime
def _destroys(stub):
    return [(n, a[0][1]) for n, a in stub.calls if n in DESTROYS or n == "ccal_unpin_buffer"]


def test_context_closes_children_first(env):
    stub, ctx = env.stub, env.ctx
    p2 = Problem(ctx, env.desc, env.keep)
    handles = {"p": env.p.handle.value, "p2": p2.handle.value, "map": env.map.handle.value, "ctx": ctx.handle.value}
    p2.close()
    assert _destroys(stub) == [("ccal_problem_destroy", handles["p2"])] and p2.handle is None
    p2.close()                                                                 # twice is one destroy
    assert len(_destroys(stub)) == 1
    ctx.close()
    d = _destroys(stub)[1:]
    assert sorted(d[:2]) == [("ccal_problem_destroy", handles["p"]), ("ccal_undistort_map_destroy", handles["map"])]
    assert d[2:] == [("ccal_ctx_destroy", handles["ctx"])]
    assert ctx.handle is None and env.p.handle is None and env.map.handle is None
    ctx.close(); env.p.close(); env.map.close()
    assert len(_destroys(stub)) == 4
    del p2


def test_multi_context_closes_children_first(env):
    stub, m = env.stub, env.m
    handles = (env.mp.handle.value, m.handle.value)
    m.close()
    assert _destroys(stub) == [("ccal_multi_problem_destroy", handles[0]), ("ccal_multi_destroy", handles[1])]
    assert m.handle is None and env.mp.handle is None
    m.close(); env.mp.close()
    assert len(_destroys(stub)) == 2
    m2 = MultiContext([0], lib=stub)
    mp2 = MultiProblem(m2, env.desc)
    h = mp2.handle.value
    mp2.close(); mp2.close()
    assert _destroys(stub)[2:] == [("ccal_multi_problem_destroy", h)]


def test_problem_close_unpins_first(env):
    stub, p = env.stub, env.p
    p.solve(INTR, POSES, opts=_ffi.SolverOpts(), pinned=True)
    pin, h = p._pin_poses, p.handle.value
    p.close()
    assert _destroys(stub) == [("ccal_unpin_buffer", env.ctx.handle.value), ("ccal_problem_destroy", h)]
    unpin = [a for n, a in stub.calls if n == "ccal_unpin_buffer"][0]
    _eq(unpin, [("vp", env.ctx.handle.value), ("vp", pin.ctypes.data)])
    assert p._pin_poses is None and p.handle is None
    # a failing unpin still ends in the destroy, and the error comes out of close()
    p2 = Problem(env.ctx, env.desc)
    p2.solve(INTR, POSES, opts=_ffi.SolverOpts(), pinned=True)
    stub.rc["ccal_unpin_buffer"] = _ffi.ERR_HIP
    with pytest.raises(CcalError, match=r"^ccal_unpin_buffer: CCAL_ERR_HIP \(ctx detail\)$"):
        p2.close()
    assert p2._pin_poses is None and p2.handle is not None
    del stub.rc["ccal_unpin_buffer"]
    # only while the context still has a handle
    p3 = Problem(env.ctx, env.desc)
    p3.solve(INTR, POSES, opts=_ffi.SolverOpts(), pinned=True)
    h3 = p3.handle.value
    env.map.close()
    n = len(_destroys(stub))
    env.ctx._problems.discard(p3); env.ctx._problems.discard(p2)
    env.ctx.close()
    p3.close()
    assert _destroys(stub)[n:] == [("ccal_ctx_destroy", 0x1000), ("ccal_problem_destroy", h3)]


def test_del_swallows_exceptions(stub):
    class Boom(_Stub):
        def __getattr__(self, name):
            if name in DESTROYS:
                raise RuntimeError("boom")
            return super().__getattr__(name)
    lib = Boom()
    ctx = Context(lib=lib)
    d, keep = _desc()
    objs = [ctx, Problem(ctx, d, keep), ctx.undistort_map_from_arrays(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)),
            MultiContext([0], lib=lib)]
    objs.append(MultiProblem(objs[3], d, keep))
    for o in objs:
        with pytest.raises(RuntimeError, match="boom"):
            o.close()
        o.__del__()                                                            # the same failure, swallowed
    # an object whose constructor failed has no handle: close() and __del__ do nothing
    stub.rc["ccal_ctx_create"] = _ffi.ERR_HIP
    for cls in (Context, MultiContext, Problem, MultiProblem, engine.UndistortMap):
        o = object.__new__(cls)
        o.close(); o.__del__()
    assert [n for n, _ in stub.calls if n in DESTROYS] == []


# ---------------------------------------------------------------------------------------------------------------------------------
# signatures
def _signatures():
    """name -> [[parameter, kind, repr(default) or None]] of every public callable of engine and every public method of its classes
    (the constructors included)."""
    out = {}

    def add(name, fn):
        out[name] = [[p.name, p.kind.name, None if p.default is p.empty else repr(p.default)] for p in inspect.signature(fn).parameters.values()]
    for name, obj in sorted(vars(engine).items()):
        if name.startswith("_") or getattr(obj, "__module__", None) != engine.__name__:
            continue
        if inspect.isclass(obj):
            for mname, _ in inspect.getmembers(obj, predicate=lambda x: inspect.isfunction(x) or inspect.ismethod(x)):
                if mname == "__init__" or not mname.startswith("_"):
                    kind = type(inspect.getattr_static(obj, mname)).__name__
                    add(f"{name}.{mname}", getattr(obj, mname))
                    out[f"{name}.{mname}"].insert(0, kind)
            for mname, member in inspect.getmembers(obj, predicate=lambda x: isinstance(x, property)):
                out[f"{name}.{mname}"] = ["property"]
        elif inspect.isfunction(obj):
            add(name, obj)
    return out


def test_public_signatures(golden_dir):
    with open(os.path.join(golden_dir, "engine_signatures.json")) as f:
        want = json.load(f)
    got = _signatures()
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    for name in want:
        assert got[name] == want[name], name
    assert len(want) > 100 and "Context.detect_tags_dev" in want and "Problem.solve" in want and "MultiProblem.validation" in want
