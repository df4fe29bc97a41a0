"""Thin object wrappers over the C ABI (include/ccal.h): Context, Problem and UndistortMap.

Nothing here computes; every method forwards to the HIP library through ctypes.  Three pieces carry the plumbing: _check (with
_Handle._call, the one way a method reaches the library) turns a status into a CcalError, _Handle owns a library handle and its
close(), _ProblemBase holds what Problem and MultiProblem share.
"""
from __future__ import annotations

import ctypes as C
import weakref
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

from . import _ffi
from ._ffi import PMAX


class CcalError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        name = _ffi.STATUS_NAMES[code] if 0 <= code < len(_ffi.STATUS_NAMES) else str(code)
        super().__init__(f"{where}: {name}" + (f" ({detail})" if detail else ""))


_OK = (_ffi.OK,)
_ANY = range(-2 ** 31, 2 ** 31)                # every status: the caller reads it from the report


def _check(rc: int, where: str, detail="", ok=_OK) -> int:
    """rc where it is one of `ok`, else CcalError.  detail: the text, or a function that fetches it (called on failure only)."""
    if rc not in ok:
        raise CcalError(rc, where, detail() if callable(detail) else detail)
    return rc


def _solve_ok(raise_on_error: bool):
    """The statuses a solve form hands back as a result: not converging is one, always."""
    return (_ffi.OK, _ffi.ERR_NO_CONVERGENCE) if raise_on_error else _ANY


def _f64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


_POINTER = {np.dtype(t).char: C.POINTER(c) for t, c in ((np.float64, C.c_double), (np.float32, C.c_float), (np.int32, C.c_int32),
                                                        (np.int64, C.c_int64), (np.uint8, C.c_uint8), (np.uint64, C.c_uint64))}


def _ptr(a: Optional[np.ndarray]):
    """The array as the C pointer of its dtype; None is NULL."""
    return None if a is None else a.ctypes.data_as(_POINTER[a.dtype.char])


def _out(n: int, *tail, dtype=np.float64) -> np.ndarray:
    """A poisoned output array [max(n, 1), *tail]: -2 for an integer type, NaN for a float."""
    return np.full((max(n, 1), *tail), -2 if np.issubdtype(dtype, np.integer) else np.nan, dtype=dtype)


def _u64(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray([int(c) for c in values], dtype=np.uint64))


def _pack(arrays, width: int):
    """The arrays [n_i, width] of a batch one after the other: (offsets int64 [n + 1], rows [total, width] f64, C-contiguous)."""
    arrs = [_f64(a).reshape(-1, width) for a in arrays]
    offs = np.zeros(len(arrs) + 1, dtype=np.int64)
    np.cumsum([len(a) for a in arrs], out=offs[1:])
    return offs, (np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros((0, width)))


class _RefineOut:
    """The outputs of a refine call for n problems of n_points points in all: poisoned, padded to one element at least."""

    def __init__(self, n: int, poses0, n_points: int, with_errors: bool):
        self.poses = _out(n, 6)
        self.poses[:n] = _f64(poses0).reshape(n, 6)
        self.ints = [_out(n, dtype=np.int32) for _ in range(3)]                     # status, iterations, n_used
        self.costs = [_out(n), _out(n)]                                             # cost0, cost
        self.err = _out(n_points) if with_errors else None

    def args(self):
        return tuple(map(_ptr, (self.poses, *self.ints, *self.costs, self.err)))     # the tail of the C call

    def result(self, n: int, err_bounds):
        """The returned tuple; err_bounds: per problem the (first, last) of its points in err."""
        out = tuple(a[:n] for a in (self.poses, *self.ints, *self.costs))
        return out + ([self.err[a:b] for a, b in err_bounds],) if self.err is not None else out


class _Handle:
    """One handle of the library and the library it came from: the checked call on it, close() and __del__."""
    handle = None               # (an object whose constructor failed has none)
    _destroy = ""               # the library function that frees the handle
    _problems = ()              # what holds this handle and is closed before it

    def _detail(self) -> str:
        return self.last_error()

    def _call(self, where: str, *args, ok=_OK) -> int:
        """The library's `where` on this handle; a status outside `ok` raises with the owner's last error."""
        return _check(getattr(self.lib, where)(self.handle, *args), where, self._detail, ok)

    def _release(self):
        for p in list(self._problems):         # whatever order the garbage collector picks: problems first
            p.close()

    def close(self):
        if self.handle:
            self._release()
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Block(NamedTuple):
    """The grey images of an image stage's call: a host or device pointer to [n_img][height][width] of dtype PIX_U8 / PIX_U16."""
    ptr: int
    dtype: int
    width: int
    height: int
    n_img: int

    def args(self):
        return int(self.dtype), int(self.width), int(self.height), int(self.n_img), C.c_void_p(self.ptr)


class Context(_Handle):
    """One GPU + one HIP stream (ccal_ctx)."""
    _destroy = "ccal_ctx_destroy"

    def __init__(self, device: int = 0, stream: int | None = None, lib=None):
        self.lib = lib if lib is not None else _ffi.load()      # lib: another build of the library (tests: _ffi.load_legacy())
        h = C.c_void_p()
        rc = self.lib.ccal_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        _check(rc, "ccal_ctx_create", "no usable HIP device" if rc == _ffi.ERR_HIP else "")
        self.handle = h
        self.device = device
        self._problems = weakref.WeakSet()        # closed before the context: a ccal_problem holds its ccal_ctx

    def last_error(self) -> str:
        return (self.lib.ccal_last_error(self.handle) or b"").decode()

    def sync(self):
        self._call("ccal_sync")

    # -- pinned caller memory (ccal_pin_buffer): arrays the library reads and writes in place, no staging copy -----
    def pin(self, a: np.ndarray) -> np.ndarray:
        """Page-lock a C-contiguous array for the GPU (hipHostRegister through the library); it must outlive the pinning."""
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("pin: a C-contiguous array")
        self._call("ccal_pin_buffer", C.c_void_p(a.ctypes.data), a.nbytes)
        return a

    def unpin(self, a: np.ndarray):
        self._call("ccal_unpin_buffer", C.c_void_p(a.ctypes.data))

    # -- model conventions (what this build assumes about the absent camera-intrinsic-model crate) -----------
    def model_conventions(self) -> _ffi.ModelConventions:
        cv = _ffi.ModelConventions()
        _check(self.lib.ccal_get_model_conventions(self.handle, C.byref(cv)), "ccal_get_model_conventions")
        return cv

    def set_model_conventions(self, cv: "_ffi.ModelConventions | None"):
        _check(self.lib.ccal_set_model_conventions(self.handle, C.byref(cv) if cv is not None else None), "ccal_set_model_conventions")

    # -- native RCCL communicator of this context's GPU (frame-sharded solves) --------------------------------
    def rccl_comm_create(self, world: int, rank: int, unique_id: bytes) -> int:
        if len(unique_id) != 128:
            raise ValueError("an RCCL unique id is 128 bytes")
        h = C.c_void_p()
        self._call("ccal_rccl_comm_create", int(world), int(rank), C.create_string_buffer(unique_id, 128), C.byref(h))
        return h.value

    # -- RANSAC radial-distortion homography (ccal_rdh_batch) -------------------------------------------------
    def rdh_batch(self, pairs_list, seeds, n_hyp: int = 1000, per_hypothesis: bool = False):
        """n independent problems in one launch.  pairs_list: arrays [n_i, 4] of normalised (x, y, x', y'); seeds: one uint64
        each.  Returns a dict of per-problem arrays `lambda` [n], `H` [n, 3, 3], `score` [n], `best` [n] (-1: none), `n_valid` [n]
        and, with per_hypothesis, `hyp_sample` [n, n_hyp, 6], `hyp_lambda`, `hyp_H` [n, n_hyp, 9], `hyp_score` (+inf: none)."""
        n = len(pairs_list)
        offs, allp = _pack(pairs_list, 4)
        if allp.size == 0:
            allp = np.zeros((1, 4))
        sd = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)
        if len(sd) != n:
            raise ValueError("one seed per problem")
        out = {"lambda": _out(n), "H": _out(n, 3, 3), "score": _out(n), "best": _out(n, dtype=np.int32), "n_valid": _out(n, dtype=np.int32)}
        hyp = {"hyp_sample": None, "hyp_lambda": None, "hyp_H": None, "hyp_score": None}
        if per_hypothesis:
            hyp = {"hyp_sample": _out(n, n_hyp, 6, dtype=np.int32), "hyp_lambda": _out(n, n_hyp), "hyp_H": _out(n, n_hyp, 9),
                   "hyp_score": _out(n, n_hyp)}
        self._call("ccal_rdh_batch", n, _ptr(offs), _ptr(allp), _ptr(sd), int(n_hyp), *map(_ptr, out.values()), *map(_ptr, hyp.values()))
        out = {k: v[:n] for k, v in out.items()}
        if per_hypothesis:
            out.update({k: v[:n] for k, v in hyp.items()})
        return out

    # -- general PnP, batched (ccal_pnp_batch, ccal_kernels_pnp.hip) ------------------------------------------------------------
    def pnp_batch(self, xyz_list, xn_list, min_points: int = 4, with_cost: bool = True):
        """n independent PnP problems in one launch.  xyz_list: arrays [n_i, 3] of 3-D points (any point set); xn_list: arrays
        [n_i, 2] of their normalised image points.  Returns (poses [n, 6] rvec,tvec, n_used [n] int32 - 0: no pose, six zeros -,
        cost [n] = E at the result, or None without with_cost)."""
        n = len(xyz_list)
        if len(xn_list) != n:
            raise ValueError("pnp_batch: one array of image points per array of points")
        (offs, allx), (offs_u, allu) = _pack(xyz_list, 3), _pack(xn_list, 2)
        if not np.array_equal(offs, offs_u):
            raise ValueError("pnp_batch: a problem's points and image points differ in number")
        poses, used, cost = _out(n, 6), _out(n, dtype=np.int32), (_out(n) if with_cost else None)
        self._call("ccal_pnp_batch", n, _ptr(offs), _ptr(allx), _ptr(allu), int(min_points), _ptr(poses), _ptr(used), _ptr(cost))
        return poses[:n], used[:n], (cost[:n] if with_cost else None)

    # -- pose refinement under fixed intrinsics, batched (ccal_refine_poses_batch, ccal_kernels_refine.hip) -----------------------
    def refine_poses_batch(self, model: int, params, xyz_list, uv_list, poses0, huber_delta: float = 1.0, min_points: int = 4,
                           opts: "_ffi.SolverOpts | None" = None, with_errors: bool = False):
        """n independent frames in one launch: the pose of each that minimises the Huber cost of the pixel reprojection error
        through the model `model` with the params() vector `params`, which stays fixed.  xyz_list: arrays [n_i, 3] of board
        points; uv_list: arrays [n_i, 2] of detections in pixels; poses0 [n, 6]: the starting rvec, tvec.  Returns (poses [n, 6],
        status [n] int32 - _ffi.OK, ERR_NO_CONVERGENCE, ERR_NONFINITE, NO_RESULT: pose as given -, iterations [n], n_used [n],
        cost0 [n], cost [n]) and, with_errors, a list of per-frame arrays of pixel errors at the result (NaN: point left out)."""
        n = len(xyz_list)
        if len(uv_list) != n:
            raise ValueError("refine_poses_batch: one array of detections per array of points")
        (offs, allx), (offs_u, allu) = _pack(xyz_list, 3), _pack(uv_list, 2)
        if not np.array_equal(offs, offs_u):
            raise ValueError("refine_poses_batch: a frame's points and detections differ in number")
        out = _RefineOut(n, poses0, int(offs[-1]), with_errors)
        par = np.zeros(PMAX)
        p = _f64(params).ravel()
        par[:len(p)] = p
        self._call("ccal_refine_poses_batch", int(model), _ptr(par), float(huber_delta), n, _ptr(offs), _ptr(allx), _ptr(allu),
                   int(min_points), C.byref(opts) if opts is not None else None, *out.args())
        return out.result(n, [(int(offs[i]), int(offs[i + 1])) for i in range(n)])

    # -- board poses of a rig under fixed intrinsics and extrinsics, batched (ccal_refine_rig_poses_batch, ccal_kernels_rig_refine.hip) --
    def refine_rig_poses_batch(self, models, params, extr, slots, poses0, huber_delta: float = 1.0, min_points: int = 4,
                               opts: "_ffi.SolverOpts | None" = None, with_errors: bool = False):
        """n independent frame slots of one rig in one launch: the board pose T_0_b of each that minimises the Huber cost of the pixel
        reprojection error summed over every camera that saw the slot.  models [n_cams], params (one params() vector per camera)
        and extr [n_cams, 6] (rvec, tvec of T_c_0, every row used as given) stay fixed.  slots: one list per slot of segments
        (cam, xyz [n_j, 3], uv [n_j, 2]); poses0 [n, 6]: the starting rvec, tvec.  Returns the tuple of refine_poses_batch with
        "frame" read as "slot": (poses [n, 6], status [n], iterations [n], n_used [n] - over all the slot's cameras -, cost0 [n],
        cost [n]) and, with_errors, a list of per-slot arrays of pixel errors at the result, the slot's segments one after the other."""
        n = len(slots)
        n_cams = len(models)
        if len(params) != n_cams:
            raise ValueError("refine_rig_poses_batch: one parameter vector per camera")
        mod = np.ascontiguousarray(models, dtype=np.int32).reshape(n_cams)
        par = np.zeros((max(n_cams, 1), PMAX))
        for c, p in enumerate(params):
            p = _f64(p).ravel()[:PMAX]
            par[c, :len(p)] = p
        ex = _f64(extr).reshape(n_cams, 6)
        segs = [seg for slot in slots for seg in slot]
        seg_offs = np.zeros(n + 1, dtype=np.int64)
        seg_offs[1:] = np.add.accumulate([len(slot) for slot in slots], dtype=np.int64)
        (pt_offs, allx), (offs_u, allu) = _pack([x for _, x, _ in segs], 3), _pack([u for _, _, u in segs], 2)
        if not np.array_equal(pt_offs, offs_u):
            raise ValueError("refine_rig_poses_batch: a segment's points and detections differ in number")
        seg_cam = np.asarray([int(cam) for cam, _, _ in segs] + [0], dtype=np.int32)
        out = _RefineOut(n, poses0, int(pt_offs[-1]), with_errors)
        self._call("ccal_refine_rig_poses_batch", n_cams, _ptr(mod), _ptr(par), _ptr(ex), float(huber_delta), n, _ptr(seg_offs),
                   _ptr(seg_cam), _ptr(pt_offs), _ptr(allx), _ptr(allu), int(min_points), C.byref(opts) if opts is not None else None,
                   *out.args())
        return out.result(n, [(int(pt_offs[seg_offs[s]]), int(pt_offs[seg_offs[s + 1]])) for s in range(n)])

    # -- applying a calibration: points, the new camera matrix, undistortion maps (ccal_kernels_undistort.hip) ---------------
    def _points(self, where, model: int, params, pts, in_w: int, out_w: int):
        pts = _f64(pts)
        if pts.ndim != 2 or pts.shape[1] != in_w:
            raise ValueError(f"{where}: an [n, {in_w}] array")
        n = pts.shape[0]
        out = _out(n, out_w)
        valid = np.zeros(max(n, 1), dtype=np.uint8)
        self._call(where, int(model), _ptr(_f64(params)), n, _ptr(pts), _ptr(out), _ptr(valid))
        return out[:n], valid[:n].astype(bool)

    def project_points(self, model: int, params, xyz):
        """GenericModel::project over xyz [n, 3]: (uv [n, 2], valid [n]); invalid rows are NaN."""
        return self._points("ccal_project_points", model, params, xyz, 3, 2)

    def unproject_points(self, model: int, params, uv):
        """GenericModel::unproject over uv [n, 2]: (rays [n, 3], valid [n]); invalid rows are NaN."""
        return self._points("ccal_unproject_points", model, params, uv, 2, 3)

    def estimate_new_camera_matrix(self, model: int, params, width: int, height: int, balance: float, new_w_h=None):
        """estimate_new_camera_matrix_for_undistort: K [3, 3], or None where an edge midpoint has no ray (CCAL_NO_RESULT)."""
        nw, nh = (0, 0) if new_w_h is None else (int(new_w_h[0]), int(new_w_h[1]))
        K = np.full(9, np.nan)
        rc = self._call("ccal_estimate_new_camera_matrix", int(model), _ptr(_f64(params)), int(width), int(height), float(balance), nw, nh,
                        _ptr(K), ok=(_ffi.OK, _ffi.NO_RESULT))
        return None if rc == _ffi.NO_RESULT else K.reshape(3, 3)

    def undistort_map(self, model: int, params, K, new_w_h, rotation=None) -> "UndistortMap":
        """init_undistort_map on the device: the maps of a new_w x new_h pinhole image K (3 x 3), optionally rotated."""
        K = _f64(K, 9)
        R = None if rotation is None else _f64(rotation, 9)
        h = C.c_void_p()
        self._call("ccal_undistort_map_create", int(model), _ptr(_f64(params)), _ptr(K), _ptr(R), int(new_w_h[0]), int(new_w_h[1]),
                   C.byref(h))
        return UndistortMap(self, h, int(new_w_h[0]), int(new_w_h[1]))

    def undistort_map_from_arrays(self, xmap, ymap) -> "UndistortMap":
        """A device-resident map from caller-made f32 arrays [h, w]."""
        xmap, ymap = check_maps(xmap, ymap)
        h = C.c_void_p()
        self._call("ccal_undistort_map_from_host", _ptr(xmap), _ptr(ymap), xmap.shape[1], xmap.shape[0], C.byref(h))
        return UndistortMap(self, h, xmap.shape[1], xmap.shape[0])

    # -- from pixels to detections: sub-pixel corner refinement, batched (ccal_refine_corners_batch, ccal_kernels_corners.hip) --------
    def _corners(self, suffix, blk, xy_list, half_win, max_iterations, eps):
        where = "ccal_refine_corners_" + suffix
        if len(xy_list) != blk.n_img:
            raise ValueError(f"{where}: one array of corners per image")
        offs, xy = _pack(xy_list, 2)
        n = int(offs[-1])
        out_xy = _out(n, 2)
        out_xy[:n] = xy
        status, iters, lam = _out(n, dtype=np.int32), _out(n, dtype=np.int32), _out(n)
        self._call(where, *blk.args(), _ptr(offs), _ptr(out_xy), int(half_win), int(max_iterations), float(eps), _ptr(status), _ptr(iters),
                   _ptr(lam))
        return _per_image(offs, blk.n_img, (out_xy, status, iters, lam))

    def refine_corners_batch(self, images, xy_list, half_win: int = 5, max_iterations: int = 30, eps: float = 1e-3):
        """Every coarse corner of a batch of grey images moved onto the grey-level saddle, all in one launch.  images: [n][H][W],
        uint8 or uint16; xy_list: one array [n_i, 2] of (x, y) starts per image.  Returns (xy_list, status_list, iters_list,
        lambda_min_list), per image: positions [n_i, 2], status [n_i] int32 - _ffi.OK, ERR_NO_CONVERGENCE (the last iterate),
        ERR_NOT_PD or NO_RESULT (the position as given) -, updates made [n_i], corner strength [n_i] (NaN: nothing evaluated)."""
        images, blk = _grey_batch(images, "refine_corners_batch")
        return self._corners("batch", blk, xy_list, half_win, max_iterations, eps)

    def refine_corners_dev(self, images_ptr: int, dtype: int, width: int, height: int, n_img: int, xy_list, half_win: int = 5,
                           max_iterations: int = 30, eps: float = 1e-3):
        """refine_corners_batch over an image block that is already on the device (a device pointer to [n_img][height][width] of
        dtype _ffi.PIX_U8 / PIX_U16, its writes complete or enqueued on the context's stream); corners and results are host arrays."""
        return self._corners("dev", _Block(images_ptr, dtype, width, height, n_img), xy_list, half_win, max_iterations, eps)

    # -- from pixels to detections: checkerboard-corner candidates of whole images (ccal_detect_corners_batch, ccal_kernels_detect.hip) --
    def _detect(self, suffix, blk, step, nms_radius, min_response, rel_threshold, max_per_image):
        where = "ccal_detect_corners_" + suffix
        rel_q10 = _rel_q10(where, rel_threshold)
        n_img = int(blk.n_img)
        cap, m = int(max_per_image), max(n_img, 1)
        # an image holds at most one candidate per (r + 1) x (r + 1) block of its domain: no room beyond that is needed
        r1, d = max(int(nms_radius), 0) + 1, 2 * (int(step) + 2)
        blocks = max(-(-(int(blk.width) - d) // r1), 0) * max(-(-(int(blk.height) - d) // r1), 0)
        if cap >= 1:
            cap = max(min(cap, blocks), 1)
        rows = max(cap, 1)
        count = np.zeros(m, dtype=np.int32)
        xy = np.empty((m, rows, 2), dtype=np.int32); hess = np.empty((m, rows, 3), dtype=np.int32)
        resp = np.empty((m, rows), dtype=np.int64)
        self._call(where, *blk.args(), int(step), int(nms_radius), int(min_response), rel_q10, cap, _ptr(count), _ptr(xy), _ptr(hess),
                   _ptr(resp))
        # one compact copy of the stored rows of all images; the per-image results are views of it
        kept = np.minimum(count[:n_img], rows).astype(np.int64)
        ends = np.cumsum(kept)
        flat = np.arange(int(ends[-1]) if n_img else 0) + np.repeat(np.arange(n_img) * rows - (ends - kept), kept)
        cxy, chess, cresp = xy.reshape(-1, 2).take(flat, axis=0), hess.reshape(-1, 3).take(flat, axis=0), resp.reshape(-1).take(flat)
        lo, hi, cnt = (ends - kept).tolist(), ends.tolist(), count.tolist()
        return [(cxy[a:b], chess[a:b], cresp[a:b], c) for a, b, c in zip(lo, hi, cnt)]

    def detect_corners_batch(self, images, step: int = 1, nms_radius: int = 5, min_response: int = 1, rel_threshold: float = 0.1,
                             max_per_image: int = 4096):
        """Checkerboard-corner candidates (grey-level saddles) of every image of a batch, by the integer rule stated at
        ccal_detect_corners_batch in include/ccal.h.  images: [n][H][W], uint8 or uint16.  rel_threshold is the fraction of the image's
        largest response a candidate must reach (rel_q10 = round(1024 rel_threshold), 0 .. 1).  Returns one tuple per image:
        (xy int32 [k, 2], hess int32 [k, 3] = (hxx, hyy, hxy), response int64 [k], count) in row-major order of (y, x), with
        k = min(count, max_per_image).  min_response scales with the square of the image contrast; no useful value has been measured
        (as for refine_corners_batch's lambda_min), the default 1 screens only flat and edge-only neighbourhoods."""
        images, blk = _grey_batch(images, "detect_corners_batch")
        return self._detect("batch", blk, step, nms_radius, min_response, rel_threshold, max_per_image)

    def detect_corners_dev(self, images_ptr: int, dtype: int, width: int, height: int, n_img: int, step: int = 1, nms_radius: int = 5,
                           min_response: int = 1, rel_threshold: float = 0.1, max_per_image: int = 4096):
        """detect_corners_batch over an image block that is already on the device (a device pointer to [n_img][height][width] of
        dtype _ffi.PIX_U8 / PIX_U16, its writes complete or enqueued on the context's stream); results are host arrays."""
        return self._detect("dev", _Block(images_ptr, dtype, width, height, n_img), step, nms_radius, min_response, rel_threshold,
                            max_per_image)

    # -- from pixels to detections: decoding tags in candidate quads (ccal_decode_tags_batch, ccal_kernels_tags.hip) ------------------
    def _tags(self, suffix, blk, quads_list, family_bits, codes, border, samples, min_contrast, max_border_errors, max_hamming):
        where = "ccal_decode_tags_" + suffix
        if len(quads_list) != blk.n_img:
            raise ValueError(f"{where}: one array of quads per image")
        d, codes = _family(where, family_bits, codes)
        offs, quads = _pack(quads_list, 8)
        n = int(offs[-1])
        reason, tag_id, rot, hamming = (_out(n, dtype=np.int32) for _ in range(4))
        corners, margin = _out(n, 4, 2), _out(n)
        code = np.zeros(max(n, 1), dtype=np.uint64)
        self._call(where, *blk.args(), _ptr(offs), _ptr(quads), d, int(border), _ptr(codes), len(codes), int(samples), float(min_contrast),
                   int(max_border_errors), int(max_hamming), *map(_ptr, (reason, tag_id, rot, hamming, corners, code, margin)))
        return _per_image(offs, blk.n_img, (reason, tag_id, rot, hamming, corners, code, margin))

    def decode_tags_batch(self, images, quads_list, family_bits: int, codes, border: int = 1, samples: int = 3,
                          min_contrast: float = 20.0, max_border_errors: int = 0, max_hamming: int = 2):
        """Every candidate quad of a batch of grey images decoded against a tag family, all in one launch, by the rule stated at
        ccal_decode_tags_batch in include/ccal.h.  images: [n][H][W], uint8 or uint16; quads_list: one array [n_i, 4, 2] of (x, y)
        corners per image, each quad in order around the tag's outer border edge; family_bits = d * d with d in 3 .. 8 and codes the
        family's table (integers < 2^family_bits), which the caller supplies.  min_contrast is in grey levels of the images' type.
        Returns (reason, id, rot, hamming, corners, code, margin), each a list with one array per image: reason [n_i] int32
        (_ffi.TAG_OK, TAG_OUTSIDE, TAG_LOW_CONTRAST, TAG_BORDER, TAG_NO_CODE), id / rot / hamming [n_i] int32 (-1 unless TAG_OK),
        corners [n_i, 4, 2] in the tag's canonical order (NaN unless TAG_OK), code [n_i] uint64 as read, margin [n_i]."""
        images, blk = _grey_batch(images, "decode_tags_batch")
        return self._tags("batch", blk, quads_list, family_bits, codes, border, samples, min_contrast, max_border_errors, max_hamming)

    def decode_tags_dev(self, images_ptr: int, dtype: int, width: int, height: int, n_img: int, quads_list, family_bits: int, codes,
                        border: int = 1, samples: int = 3, min_contrast: float = 20.0, max_border_errors: int = 0, max_hamming: int = 2):
        """decode_tags_batch over an image block that is already on the device (a device pointer to [n_img][height][width] of
        dtype _ffi.PIX_U8 / PIX_U16, its writes complete or enqueued on the context's stream); quads, codes and results are host arrays."""
        return self._tags("dev", _Block(images_ptr, dtype, width, height, n_img), quads_list, family_bits, codes, border, samples,
                          min_contrast, max_border_errors, max_hamming)

    # -- from pixels to detections: proposing tag quads from corner candidates (ccal_propose_quads_batch, ccal_kernels_quads.hip) ------
    def _quads(self, suffix, blk, xy_list, min_side, max_side, max_side_ratio, offset, samples, min_contrast, max_per_image):
        where = "ccal_propose_quads_" + suffix
        if len(xy_list) != blk.n_img:
            raise ValueError(f"{where}: one array of points per image")
        if max_side is None:
            max_side = max(int(blk.width), int(blk.height)) / 2.0
        offs, xy = _pack(xy_list, 2)
        n_img = int(blk.n_img)
        cap, m = int(max_per_image), max(n_img, 1)
        # a point starts at most 8^3 chains: no room beyond that is needed
        most = max((int(offs[k + 1] - offs[k]) for k in range(n_img)), default=0)
        if cap >= 1:
            cap = max(min(cap, _ffi.QUAD_MAX_OUT_EDGES ** 3 * most), 1)
        rows = max(cap, 1)
        count = np.zeros(m, dtype=np.int32); flags = np.zeros(m, dtype=np.int32)
        # NOT pre-filled with a poison value as the neighbouring wrappers' outputs are: at 1024 images and cap 1024 the two arrays are
        # 80 MB, and filling them cost 1.1 of a call's 8.07 ms (6.95 ms without).  Rows past min(count, cap) are never read below;
        # the price is that only a caller of the C entry point with its own sentinels (tests/test_gpu_quads.py: raw_propose) can
        # see a stored row the library failed to write
        idx = np.empty((m, rows, 4), dtype=np.int32); quads = np.empty((m, rows, 4, 2))
        self._call(where, *blk.args(), _ptr(offs), _ptr(xy), float(min_side), float(max_side), float(max_side_ratio), float(offset),
                   int(samples), float(min_contrast), cap, _ptr(count), _ptr(flags), _ptr(idx), _ptr(quads))
        return [(idx[k, :min(int(count[k]), rows)].copy(), quads[k, :min(int(count[k]), rows)].copy(), int(count[k]), int(flags[k]))
                for k in range(n_img)]

    def propose_quads_batch(self, images, xy_list, min_side: float = 20.0, max_side: Optional[float] = None, max_side_ratio: float = 2.0,
                            offset: float = 1.0 / 16.0, samples: int = 8, min_contrast: float = 40.0, max_per_image: int = 1024):
        """Candidate tag outlines of an AprilGrid from the refined saddle points of every image of a batch, by the rule stated at
        ccal_propose_quads_batch in include/ccal.h.  images: [n][H][W], uint8 or uint16; xy_list: one array [n_i, 2] of (x, y) points
        per image, in any order.  max_side None: half the larger image side.  offset: half a cell of the tag as a fraction of its
        side, 1 / (2 (d + 2 border)); min_contrast is in grey levels of the images' type.  Returns one tuple per image:
        (idx int32 [m, 4] - the corners' indices into the image's points -, quads f64 [m, 4, 2] - their coordinates, ready for
        decode_tags_batch -, count, flags) in lexicographic order of the indices, with m = min(count, max_per_image); bit 0 of flags
        (_ffi.QUAD_FLAG_CUT): a point had more than 8 out-edges, proposals may be missing."""
        images, blk = _grey_batch(images, "propose_quads_batch")
        return self._quads("batch", blk, xy_list, min_side, max_side, max_side_ratio, offset, samples, min_contrast, max_per_image)

    def propose_quads_dev(self, images_ptr: int, dtype: int, width: int, height: int, n_img: int, xy_list, min_side: float = 20.0,
                          max_side: Optional[float] = None, max_side_ratio: float = 2.0, offset: float = 1.0 / 16.0, samples: int = 8,
                          min_contrast: float = 40.0, max_per_image: int = 1024):
        """propose_quads_batch over an image block that is already on the device (a device pointer to [n_img][height][width] of
        dtype _ffi.PIX_U8 / PIX_U16, its writes complete or enqueued on the context's stream); points and results are host arrays."""
        return self._quads("dev", _Block(images_ptr, dtype, width, height, n_img), xy_list, min_side, max_side, max_side_ratio, offset,
                           samples, min_contrast, max_per_image)

    # -- from pixels to detections: the four stages in one device-resident call (ccal_detect_tags_batch, ccal_kernels_tagchain.hip) ----
    def _detect_tags(self, suffix, blk, family_bits, codes, step, nms_radius, min_response, rel_threshold, max_candidates, half_win,
                     max_iterations, eps, merge_radius, min_side, max_side, max_side_ratio, offset, edge_samples, edge_min_contrast,
                     max_quads, border, cell_samples, tag_min_contrast, max_border_errors, max_hamming, max_tags):
        where = "ccal_detect_tags_" + suffix
        front = _front_opts(where, step, nms_radius, min_response, rel_threshold, max_candidates, half_win, max_iterations, eps)
        d, codes = _family(where, family_bits, codes)
        if max_side is None:
            max_side = max(int(blk.width), int(blk.height)) / 2.0
        if offset is None:
            offset = 1.0 / (2.0 * (d + 2 * int(border)))
        if max_tags is None:
            max_tags = max(len(codes), 1)              # an image's tags have distinct ids
        o = _ffi.DetectTagsOpts(
            **front, merge_radius=float(merge_radius), min_side=float(min_side), max_side=float(max_side), max_side_ratio=float(max_side_ratio),
            offset=float(offset), edge_min_contrast=float(edge_min_contrast), edge_samples=int(edge_samples), quad_cap=int(max_quads),
            border=int(border), cell_samples=int(cell_samples), tag_min_contrast=float(tag_min_contrast),
            max_border_errors=int(max_border_errors), max_hamming=int(max_hamming), tag_cap=int(max_tags))
        n_img, rows = int(blk.n_img), max(int(max_tags), 1)
        m = max(n_img, 1)
        count = np.zeros(m, dtype=np.int32); flags = np.zeros(m, dtype=np.int32); stats = np.zeros((m, 4), dtype=np.int32)
        tag_id, rot, hamming = (_out(n_img, rows, dtype=np.int32) for _ in range(3))
        corners, margin = _out(n_img, rows, 4, 2), _out(n_img, rows)
        self._call(where, *blk.args(), d, _ptr(codes), len(codes), C.byref(o),
                   *map(_ptr, (count, tag_id, rot, hamming, corners, margin, flags, stats)))
        out = []
        for k in range(n_img):
            n = min(int(count[k]), rows)
            out.append((tag_id[k, :n].copy(), rot[k, :n].copy(), hamming[k, :n].copy(), corners[k, :n].copy(), margin[k, :n].copy(),
                        int(count[k]), int(flags[k]), stats[k].copy()))
        return out

    def detect_tags_batch(self, images, family_bits: int, codes, step: int = 1, nms_radius: int = 5, min_response: int = 1,
                          rel_threshold: float = 0.1, max_candidates: int = 4096, half_win: int = 4, max_iterations: int = 30,
                          eps: float = 1e-3, merge_radius: float = 1.0, min_side: float = 20.0, max_side: Optional[float] = None,
                          max_side_ratio: float = 2.0, offset: Optional[float] = None, edge_samples: int = 8,
                          edge_min_contrast: float = 40.0, max_quads: int = 1024, border: int = 1, cell_samples: int = 3,
                          tag_min_contrast: float = 40.0, max_border_errors: int = 0, max_hamming: int = 2, max_tags: Optional[int] = None):
        """From a batch of grey images to the tags of a family in each, in ONE call that keeps every intermediate on the device:
        detector, refinement, merge, proposer, decoder and the best quad per id, by the rule stated at ccal_detect_tags_batch in
        include/ccal.h.  images: [n][H][W], uint8 or uint16; family_bits = d * d and codes as for decode_tags_batch.  The other
        parameters are the stages' (detect_corners_batch, refine_corners_batch, api.merge_points, propose_quads_batch,
        decode_tags_batch); max_side None: half the larger image side; offset None: half a cell, 1 / (2 (d + 2 border)); max_tags
        None: the family's size.  The contrasts are in grey levels of the images' type.  Returns one tuple per image: (id int32 [m],
        rot [m], hamming [m], corners f64 [m, 4, 2] in the tag's canonical order, margin [m], count, flags, stats int32 [4]) in
        ascending id, m = min(count, max_tags); flags: _ffi.TAGS_FLAG_*; stats = candidates found, points after the merge, quads
        found, decodable quads before the selection."""
        images, blk = _grey_batch(images, "detect_tags_batch")
        return self._detect_tags("batch", blk, family_bits, codes, step, nms_radius, min_response, rel_threshold, max_candidates, half_win,
                                 max_iterations, eps, merge_radius, min_side, max_side, max_side_ratio, offset, edge_samples,
                                 edge_min_contrast, max_quads, border, cell_samples, tag_min_contrast, max_border_errors, max_hamming,
                                 max_tags)

    def detect_tags_dev(self, images_ptr: int, dtype: int, width: int, height: int, n_img: int, family_bits: int, codes, step: int = 1,
                        nms_radius: int = 5, min_response: int = 1, rel_threshold: float = 0.1, max_candidates: int = 4096,
                        half_win: int = 4, max_iterations: int = 30, eps: float = 1e-3, merge_radius: float = 1.0, min_side: float = 20.0,
                        max_side: Optional[float] = None, max_side_ratio: float = 2.0, offset: Optional[float] = None,
                        edge_samples: int = 8, edge_min_contrast: float = 40.0, max_quads: int = 1024, border: int = 1,
                        cell_samples: int = 3, tag_min_contrast: float = 40.0, max_border_errors: int = 0, max_hamming: int = 2,
                        max_tags: Optional[int] = None):
        """detect_tags_batch over an image block that is already on the device (a device pointer to [n_img][height][width] of
        dtype _ffi.PIX_U8 / PIX_U16, its writes complete or enqueued on the context's stream); the family and the results are host arrays."""
        return self._detect_tags("dev", _Block(images_ptr, dtype, width, height, n_img), family_bits, codes, step, nms_radius,
                                 min_response, rel_threshold, max_candidates, half_win, max_iterations, eps, merge_radius, min_side,
                                 max_side, max_side_ratio, offset, edge_samples, edge_min_contrast, max_quads, border, cell_samples,
                                 tag_min_contrast, max_border_errors, max_hamming, max_tags)

    # -- from pixels to detections: complete checkerboards (ccal_assemble_checkerboards_batch, ccal_kernels_board.hip) ---------------
    def assemble_checkerboards_batch(self, xy_list, hess_list, cols: int, rows: int):
        """The corner candidates of every image of a batch ordered into a complete cols x rows checkerboard, all images in one call,
        by the rule stated at ccal_assemble_checkerboards_batch in include/ccal.h.  xy_list: one array [n_i, 2] of refined (x, y)
        per image; hess_list: one array [n_i, 3] of (hxx, hyy, hxy) per image as the detector returns them.  Returns one tuple per
        image: (found, xy f64 [cols * rows, 2] in id order, idx int32 [cols * rows] - the image's row of each corner -, flags,
        stats int32 [4] = rows kept, attempts that found a board, the winner's seed rank and pair); xy and idx are None without a
        board.  flags: _ffi.BOARD_FLAG_KEPT_LIMIT - more than 512 rows kept after the screen, no board."""
        where = "ccal_assemble_checkerboards_batch"
        if len(xy_list) != len(hess_list):
            raise ValueError(f"{where}: one array of Hessians per array of positions")
        n_img = len(xy_list)
        (offs, xy), (offs_h, hess) = _pack(xy_list, 2), _pack(hess_list, 3)
        if not np.array_equal(offs, offs_h):
            raise ValueError(f"{where}: one Hessian per position")
        nw = max(int(cols) * int(rows), 1)
        found, flags, stats = _out(n_img, dtype=np.int32), _out(n_img, dtype=np.int32), _out(n_img, 4, dtype=np.int32)
        oxy, idx = _out(n_img, nw, 2), _out(n_img, nw, dtype=np.int32)
        self._call(where, n_img, _ptr(offs), _ptr(xy), _ptr(hess), int(cols), int(rows), _ptr(found), _ptr(oxy), _ptr(idx), _ptr(flags),
                   _ptr(stats))
        return [(int(found[k]), oxy[k].copy() if found[k] else None, idx[k].copy() if found[k] else None, int(flags[k]), stats[k].copy())
                for k in range(n_img)]

    def _detect_boards(self, suffix, blk, cols, rows, step, nms_radius, min_response, rel_threshold, max_candidates, half_win,
                       max_iterations, eps):
        where = "ccal_detect_checkerboards_" + suffix
        o = _ffi.DetectCheckerboardsOpts(
            **_front_opts(where, step, nms_radius, min_response, rel_threshold, max_candidates, half_win, max_iterations, eps),
            cols=int(cols), rows=int(rows))
        n_img, nw = int(blk.n_img), max(int(cols) * int(rows), 1)
        m = max(n_img, 1)
        found = np.zeros(m, dtype=np.int32); flags = np.zeros(m, dtype=np.int32); stats = np.zeros((m, 4), dtype=np.int32)
        oxy = _out(n_img, nw, 2)
        self._call(where, *blk.args(), C.byref(o), _ptr(found), _ptr(oxy), _ptr(flags), _ptr(stats))
        return [(int(found[k]), oxy[k].copy() if found[k] else None, int(flags[k]), stats[k].copy()) for k in range(n_img)]

    def detect_checkerboards_batch(self, images, cols: int, rows: int, step: int = 1, nms_radius: int = 5, min_response: int = 1,
                                   rel_threshold: float = 0.1, max_candidates: int = 4096, half_win: int = 5, max_iterations: int = 30,
                                   eps: float = 1e-3):
        """From a batch of grey images to the complete cols x rows checkerboard in each, in ONE call that keeps every intermediate
        on the device: detector, refinement, the CCAL_OK corners with their Hessians, assembly - by the rule stated at
        ccal_detect_checkerboards_batch in include/ccal.h.  images: [n][H][W], uint8 or uint16; the other parameters are the stages'
        (detect_corners_batch, refine_corners_batch; max_candidates at most 4096).  Returns one tuple per image: (found, xy f64
        [cols * rows, 2] in id order or None, flags, stats int32 [4] as assemble_checkerboards_batch); flags:
        _ffi.BOARD_FLAG_CAND_CAP, _ffi.BOARD_FLAG_KEPT_LIMIT."""
        images, blk = _grey_batch(images, "detect_checkerboards_batch")
        return self._detect_boards("batch", blk, cols, rows, step, nms_radius, min_response, rel_threshold, max_candidates, half_win,
                                   max_iterations, eps)

    def detect_checkerboards_dev(self, images_ptr: int, dtype: int, width: int, height: int, n_img: int, cols: int, rows: int,
                                 step: int = 1, nms_radius: int = 5, min_response: int = 1, rel_threshold: float = 0.1,
                                 max_candidates: int = 4096, half_win: int = 5, max_iterations: int = 30, eps: float = 1e-3):
        """detect_checkerboards_batch over an image block that is already on the device (a device pointer to [n_img][height][width]
        of dtype _ffi.PIX_U8 / PIX_U16, its writes complete or enqueued on the context's stream); the results are host arrays."""
        return self._detect_boards("dev", _Block(images_ptr, dtype, width, height, n_img), cols, rows, step, nms_radius, min_response,
                                   rel_threshold, max_candidates, half_win, max_iterations, eps)

    # -- rendering calibration targets through the camera models (ccal_render_targets_batch, ccal_kernels_render.hip) ----------------
    def _render(self, suffix, out_ptr, model, params, dtype, width, height, poses, target, supersample, black, white, background,
                margin, photo=None):
        """suffix: batch / dev; with photo the call is the ccal_render_photo_targets form of ccal_render_targets_<suffix>."""
        where = "ccal_render_targets_" + suffix if photo is None else "ccal_render_photo_targets" + ("_dev" if suffix == "dev" else "")
        poses = _f64(poses)
        if poses.ndim != 2 or poses.shape[1] != 6:
            raise ValueError(f"{where}: poses is an [n, 6] array of rvec, tvec")
        o = render_opts(target, supersample, black, white, background, margin, lib=self.lib)
        tail = (C.c_void_p(out_ptr),) if photo is None else (C.byref(photo_opts(photo)), C.c_void_p(out_ptr))
        self._call(where, int(model), _ptr(_f64(params)), int(dtype), int(width), int(height), poses.shape[0], _ptr(poses), C.byref(target),
                   C.byref(o), *tail)

    def render_targets_batch(self, model: int, params, width: int, height: int, poses, target: "_ffi.RenderTarget", dtype=np.uint8,
                             supersample: Optional[int] = None, black: Optional[float] = None, white: Optional[float] = None,
                             background: Optional[float] = None, margin: Optional[float] = None, photo=None) -> np.ndarray:
        """Grey images [n][height][width] (uint8 or uint16) of `target` (checkerboard_target / aprilgrid_target) as the camera
        (model, params) sees it at poses [n, 6] (rvec, tvec: board -> camera), by the rule stated at ccal_render_targets_batch in
        include/ccal.h: every pixel the mean of supersample x supersample rays.  An option left at None takes
        ccal_render_set_defaults' value (4; 40, 215, 0 grey levels; a margin of one square or one tag pitch).  photo (an
        api.PhotoOpts or a _ffi.PhotoOpts; None: ideal images, the call above): the ideal images at uint16 go through the
        photometric stage - lens blur, vignetting, exposure, sensor noise - on the device (ccal_render_photo_targets)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise ValueError("render_targets_batch: uint8 or uint16 images")
        n = _f64(poses).shape[0] if np.ndim(poses) == 2 else 0
        out = np.empty((n, max(int(height), 0), max(int(width), 0)), dtype=dt)
        self._render("batch", out.ctypes.data if out.size else 0, model, params, _ffi.PIX_U8 if dt == np.uint8 else _ffi.PIX_U16, width,
                     height, poses, target, supersample, black, white, background, margin, photo)
        return out

    def render_targets_dev(self, out_ptr: int, model: int, params, dtype: int, width: int, height: int, poses, target: "_ffi.RenderTarget",
                           supersample: Optional[int] = None, black: Optional[float] = None, white: Optional[float] = None,
                           background: Optional[float] = None, margin: Optional[float] = None, photo=None) -> None:
        """render_targets_batch into a device block (a device pointer to [n][height][width] of dtype _ffi.PIX_U8 / PIX_U16) on the
        context's stream: the block goes straight into detect_checkerboards_dev, detect_tags_dev or UndistortMap.remap_dev."""
        self._render("dev", out_ptr, model, params, dtype, width, height, poses, target, supersample, black, white, background, margin, photo)

    def _pixels(self, where, head, src_dtype, dst_dtype, width, height, n_img, src_ptr, dst_ptr, opts):
        """A pixel-writing stage from one device block to another: where(handle, *head, the two types, the size, the blocks, opts)."""
        self._call(where, *head, int(src_dtype), int(dst_dtype), int(width), int(height), int(n_img), C.c_void_p(src_ptr), C.c_void_p(dst_ptr),
                   C.byref(opts))

    # -- the photometric stage (ccal_photo_apply_dev, ccal_kernels_photo.hip) -------------------------------------------------------
    def photo_apply_dev(self, src_ptr: int, dst_ptr: int, src_dtype: int, dst_dtype: int, width: int, height: int, n_img: int,
                        photo) -> None:
        """Lens blur, vignetting, exposure and sensor noise (photo: an api.PhotoOpts or a _ffi.PhotoOpts) from the device block
        src_ptr to the device block dst_ptr, [n_img][height][width] of _ffi.PIX_U8 / PIX_U16 each, by the rule stated at
        ccal_photo_apply_dev in include/ccal.h.  Only enqueued on the context's stream; the blocks must not overlap."""
        self._pixels("ccal_photo_apply_dev", (), src_dtype, dst_dtype, width, height, n_img, src_ptr, dst_ptr, photo_opts(photo))

    # -- local contrast normalisation (ccal_normalize_dev, ccal_kernels_normalize.hip) ------------------------------------------------
    def normalize_dev(self, src_ptr: int, dst_ptr: int, src_dtype: int, dst_dtype: int, width: int, height: int, n_img: int,
                      norm=None) -> None:
        """Every pixel's distance from the mean of the (2 r + 1)^2 window around it in units of the window's standard deviation
        (norm: an api.NormalizeOpts or a _ffi.NormalizeOpts; None: ccal_normalize_set_defaults) from the device block src_ptr to
        the device block dst_ptr, [n_img][height][width] of _ffi.PIX_U8 / PIX_U16 each, by the rule stated at ccal_normalize_dev in
        include/ccal.h; dst_ptr then goes into detect_checkerboards_dev / detect_tags_dev.  Only enqueued on the context's stream;
        the blocks must not overlap."""
        self._pixels("ccal_normalize_dev", (), src_dtype, dst_dtype, width, height, n_img, src_ptr, dst_ptr,
                     normalize_opts(norm, lib=self.lib))

    # -- grey frames from colour and raw Bayer frames (ccal_grey_dev, ccal_kernels_grey.hip) -------------------------------------------
    def grey_dev(self, src_ptr: int, dst_ptr: int, layout: int, src_dtype: int, dst_dtype: int, width: int, height: int, n_img: int,
                 opts=None) -> None:
        """The grey frames of the device block src_ptr - [n_img][height][width][c] for the interleaved layouts (_ffi.LAYOUT_RGB, _BGR,
        _RGBA, _BGRA), [n_img][height][width] for _ffi.LAYOUT_GREY and the four _ffi.LAYOUT_BAYER_* mosaics, of _ffi.PIX_U8 / PIX_U16 -
        into the device block dst_ptr, [n_img][height // bin][width // bin] of dst_dtype (grey_out_size), by the rule stated at
        ccal_grey_dev in include/ccal.h (opts: an api.GreyOpts or a _ffi.GreyOpts; None: ccal_grey_set_defaults); dst_ptr then goes
        into normalize_dev, detect_checkerboards_dev or detect_tags_dev.  Only enqueued on the context's stream; the blocks must not
        overlap."""
        self._pixels("ccal_grey_dev", (int(layout),), src_dtype, dst_dtype, width, height, n_img, src_ptr, dst_ptr,
                     grey_opts(opts, lib=self.lib))


def _grey_batch(images, who: str):
    """The image arguments of an image stage's host call: the checked array (the caller keeps it alive over the call) and its
    _Block as the stage's private method takes it."""
    images, dtype, channels = check_images(images, True)
    if channels != 1:
        raise ValueError(f"{who}: single-channel images [n][H][W]")
    n_img, H, W = images.shape[:3]
    return images, _Block(images.ctypes.data, dtype, W, H, n_img)


def _rel_q10(where: str, rel_threshold) -> int:
    """rel_threshold as the detector takes it: round(1024 rel_threshold); ValueError when it is not finite."""
    if not np.isfinite(rel_threshold):
        raise ValueError(f"{where}: rel_threshold is not finite")
    return int(round(1024.0 * float(rel_threshold)))


def _front_opts(where: str, step, nms_radius, min_response, rel_threshold, max_candidates, half_win, max_iterations, eps) -> dict:
    """The detector's and the refinement's fields, with which the options of both image chains begin."""
    return dict(step=int(step), nms_radius=int(nms_radius), min_response=int(min_response), rel_q10=_rel_q10(where, rel_threshold),
                cand_cap=int(max_candidates), half_win=int(half_win), max_iterations=int(max_iterations), eps=float(eps))


def _family(where: str, family_bits, codes):
    """(d, the code table as a contiguous uint64 array) of a tag family of family_bits = d * d bits."""
    d = int(round(max(float(family_bits), 0.0) ** 0.5))
    if d * d != int(family_bits):
        raise ValueError(f"{where}: family_bits is not a square")
    return d, _u64(codes)


def checkerboard_target(cols: int, rows: int, square: float) -> "_ffi.RenderTarget":
    """The ccal_render_target of a checkerboard of cols x rows inner corners and squares of `square` metres."""
    return _ffi.RenderTarget(kind=_ffi.TARGET_CHECKERBOARD, cols=int(cols), rows=int(rows), square=float(square))


def aprilgrid_target(tag_size: float, tag_spacing: float, tag_rows: int, tag_cols: int, first_id: int, family_bits: int, codes,
                     border: int = 1) -> "_ffi.RenderTarget":
    """The ccal_render_target of an AprilGrid; it keeps the code table it points to alive."""
    table = _u64(codes)
    t = _ffi.RenderTarget(kind=_ffi.TARGET_APRILGRID, tag_size=float(tag_size), tag_spacing=float(tag_spacing), tag_rows=int(tag_rows),
                          tag_cols=int(tag_cols), first_id=int(first_id), family_bits=int(family_bits), n_codes=len(table),
                          border=int(border), codes=_ptr(table) if len(table) else None)
    t._table = table
    return t


def _opts(struct, set_defaults: str, src, fields, lib, *head):
    """The option struct of `src`: a ready `struct` as it is; else the library's set_defaults(*head, the struct), then every field
    of src (None: no field) that is not None, cast to the struct's type of it."""
    if isinstance(src, struct):
        return src
    o = struct()
    _check(getattr(lib or _ffi.load(), set_defaults)(*head, C.byref(o)), set_defaults)
    types = dict(struct._fields_)
    for name in (fields if src is not None else ()):
        v = getattr(src, name)
        if v is not None:
            setattr(o, name, float(v) if types[name] is C.c_double else int(v))
    return o


def render_opts(target: "_ffi.RenderTarget", supersample=None, black=None, white=None, background=None, margin=None,
                lib=None) -> "_ffi.RenderOpts":
    """ccal_render_set_defaults for `target`, then every option that is not None."""
    given = SimpleNamespace(supersample=supersample, black=black, white=white, background=background, margin=margin)
    return _opts(_ffi.RenderOpts, "ccal_render_set_defaults", given, vars(given), lib, C.byref(target))


def photo_opts(photo) -> "_ffi.PhotoOpts":
    """The ccal_photo_opts of `photo`: a _ffi.PhotoOpts as it is, else anything with the seven fields (api.PhotoOpts)."""
    if isinstance(photo, _ffi.PhotoOpts):
        return photo
    return _ffi.PhotoOpts(blur_sigma=float(photo.blur_sigma), vignette=float(photo.vignette), gain=float(photo.gain),
                          noise_read=float(photo.noise_read), noise_shot=float(photo.noise_shot),
                          seed=int(photo.seed) & 0xFFFFFFFFFFFFFFFF, first_index=int(photo.first_index))


def photo_tables(photo, lib=None):
    """(radius, taps f64 [17], sigma f64 [256]) of ccal_photo_tables: exactly what the photometric kernel uses for `photo`.  Host
    only.  ValueError when an option is out of range."""
    radius, taps, sigma = C.c_int32(0), np.zeros(_ffi.PHOTO_MAX_RADIUS + 1), np.zeros(256)
    try:
        _check((lib or _ffi.load()).ccal_photo_tables(C.byref(photo_opts(photo)), C.byref(radius), _ptr(taps), _ptr(sigma)), "photo_tables")
    except CcalError:
        raise ValueError("photo_tables: an option is out of range (include/ccal.h, the photometric stage)") from None
    return int(radius.value), taps, sigma


def normalize_opts(norm=None, lib=None) -> "_ffi.NormalizeOpts":
    """The ccal_normalize_opts of `norm`: a _ffi.NormalizeOpts as it is; None: ccal_normalize_set_defaults; else anything with the
    fields radius, min_sigma and amp (api.NormalizeOpts)."""
    return _opts(_ffi.NormalizeOpts, "ccal_normalize_set_defaults", norm, ("radius", "min_sigma", "amp"), lib)


def grey_opts(opts=None, lib=None) -> "_ffi.GreyOpts":
    """The ccal_grey_opts of `opts`: a _ffi.GreyOpts as it is; None: ccal_grey_set_defaults; else anything with the fields bin, w_r,
    w_g and w_b (api.GreyOpts)."""
    return _opts(_ffi.GreyOpts, "ccal_grey_set_defaults", opts, ("bin", "w_r", "w_g", "w_b"), lib)


def grey_out_size(width: int, height: int, bin: int):
    """(width, height) of the frames Context.grey_dev writes for sources of width x height at `bin`: the rows and columns of an
    incomplete last block are dropped."""
    return int(width) // int(bin), int(height) // int(bin)


def _per_image(offs, n_img: int, arrays):
    """Flat outputs cut back per image: for each array the list of its n_img views."""
    cut = [(int(offs[k]), int(offs[k + 1])) for k in range(n_img)]
    return tuple([arr[a:b] for a, b in cut] for arr in arrays)


def check_maps(xmap, ymap):
    """Two f32 arrays [h, w] of one shape (ValueError otherwise), C-contiguous."""
    xmap, ymap = np.asarray(xmap), np.asarray(ymap)
    if xmap.dtype != np.float32 or ymap.dtype != np.float32:
        raise ValueError("maps: float32 arrays")
    if xmap.ndim != 2 or xmap.shape != ymap.shape or xmap.size == 0:
        raise ValueError("maps: two non-empty [h, w] arrays of the same shape")
    return np.ascontiguousarray(xmap), np.ascontiguousarray(ymap)


def check_images(images, batched: bool):
    """uint8 [..][H][W], uint8 [..][H][W][3] or uint16 [..][H][W] (ValueError otherwise): (array, dtype code, channels)."""
    images = np.asarray(images)
    lead = 1 if batched else 0
    if images.dtype not in (np.uint8, np.uint16):
        raise ValueError("remap: uint8 or uint16 images")
    if images.ndim not in (lead + 2, lead + 3) or images.size == 0:
        raise ValueError("remap: images [n][H][W] or [n][H][W][3]" if batched else "remap: an image [H][W] or [H][W][3]")
    channels = images.shape[lead + 2] if images.ndim == lead + 3 else 1
    if (images.dtype == np.uint8 and channels not in (1, 3)) or (images.dtype == np.uint16 and channels != 1) or \
            (images.ndim == lead + 3 and channels == 1):
        raise ValueError("remap: one channel ([H][W]) of uint8 or uint16, or three interleaved channels of uint8")
    return np.ascontiguousarray(images), (_ffi.PIX_U8 if images.dtype == np.uint8 else _ffi.PIX_U16), int(channels)


class UndistortMap(_Handle):
    """A device-resident pair of undistortion maps (ccal_undistort_map): build once, remap every frame of a session."""
    _destroy = "ccal_undistort_map_destroy"

    def __init__(self, ctx: Context, handle, w: int, h: int):
        self.ctx = ctx
        self.lib = ctx.lib
        self.handle = handle
        self.w, self.h = int(w), int(h)
        ctx._problems.add(self)               # closed before the context, like a problem

    def _detail(self) -> str:
        return self.ctx.last_error()

    def download(self):
        """(xmap, ymap), f32 [h, w]."""
        xmap = np.empty((self.h, self.w), dtype=np.float32); ymap = np.empty((self.h, self.w), dtype=np.float32)
        self._call("ccal_undistort_map_download", _ptr(xmap), _ptr(ymap))
        return xmap, ymap

    def remap(self, images) -> np.ndarray:
        """Bilinear resampling of a batch [n][H][W] (uint8 / uint16) or [n][H][W][3] (uint8) -> [n][h][w](, 3), same dtype."""
        images, dtype, channels = check_images(images, True)
        n, H, W = images.shape[:3]
        out = np.empty((n, self.h, self.w) + images.shape[3:], dtype=images.dtype)
        self._call("ccal_remap", dtype, channels, W, H, n, C.c_void_p(images.ctypes.data), C.c_void_p(out.ctypes.data))
        return out

    def remap_dev(self, src_ptr: int, dst_ptr: int, dtype: int, channels: int, src_w: int, src_h: int, n_img: int):
        """Device pointers; only enqueues on the context's stream (Context.sync waits)."""
        self._call("ccal_remap_dev", int(dtype), int(channels), int(src_w), int(src_h), int(n_img), C.c_void_p(src_ptr), C.c_void_p(dst_ptr))


def rccl_available() -> bool:
    return bool(_ffi.load().ccal_rccl_available())


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls this and hands the 128 bytes to every rank)."""
    buf = C.create_string_buffer(128)
    _check(_ffi.load().ccal_rccl_unique_id(buf), "ccal_rccl_unique_id")
    return buf.raw


def rccl_comm_destroy(comm: int) -> None:
    _ffi.load().ccal_rccl_comm_destroy(C.c_void_p(comm))


def rccl_comm_count(comm: int) -> int:
    """ncclCommCount of a communicator made by Context.rccl_comm_create (-1 on error)."""
    return int(_ffi.load().ccal_rccl_comm_count(C.c_void_p(comm)))


def partition_slots(desc: "_ffi.ProblemDesc", n_shards: int, lib=None) -> list:
    """ccal_partition_slots (host only, no GPU): the n_shards + 1 slot boundaries ccal_multi_problem_create cuts `desc` at -
    contiguous frame-slot ranges balanced by corner count."""
    first = np.zeros(n_shards + 1, dtype=np.int32)
    _check((lib or _ffi.load()).ccal_partition_slots(C.byref(desc), int(n_shards), _ptr(first)), "ccal_partition_slots")
    return [int(x) for x in first]


def make_desc(n_cams, model, width, height, xy_same_focal, n_slots, obs_cam, obs_slot, obs_offsets,
              x, y, z, u, v, huber_delta):
    """Build a ccal_problem_desc and return (desc, keepalive-list-of-arrays)."""
    keep = dict(
        model=np.ascontiguousarray(model, dtype=np.int32), width=_f64(width), height=_f64(height),
        obs_cam=np.ascontiguousarray(obs_cam, dtype=np.int32), obs_slot=np.ascontiguousarray(obs_slot, dtype=np.int32),
        obs_offsets=np.ascontiguousarray(obs_offsets, dtype=np.int64),
        x=np.ascontiguousarray(x, dtype=np.float32), y=np.ascontiguousarray(y, dtype=np.float32),
        z=np.ascontiguousarray(z, dtype=np.float32), u=np.ascontiguousarray(u, dtype=np.float32),
        v=np.ascontiguousarray(v, dtype=np.float32))
    d = _ffi.ProblemDesc()
    d.n_cams = int(n_cams)
    d.xy_same_focal = 1 if xy_same_focal else 0
    d.n_slots = int(n_slots); d.n_obs = int(len(keep["obs_cam"]))
    for name, key in (("model", "model"), ("width", "width"), ("height", "height"), ("obs_cam", "obs_cam"), ("obs_slot", "obs_slot"),
                      ("obs_offsets", "obs_offsets"), ("p3d_x", "x"), ("p3d_y", "y"), ("p3d_z", "z"), ("p2d_u", "u"), ("p2d_v", "v")):
        setattr(d, name, _ptr(keep[key]))
    d.huber_delta = float(huber_delta)
    return d, keep


def desc_from_synth(sp):
    x, y, z, u, v = sp.soa()
    return make_desc(sp.n_cams, sp.model, sp.width, sp.height, sp.xy_same_focal, sp.n_slots,
                     sp.obs_cam, sp.obs_slot, sp.obs_offsets, x, y, z, u, v, sp.huber_delta)


def default_opts(method: int = _ffi.METHOD_GN, **kw) -> _ffi.SolverOpts:
    o = _ffi.SolverOpts()
    _ffi.load().ccal_set_defaults(C.byref(o))
    o.method = method
    for k, val in kw.items():
        setattr(o, k, val)
    return o


class MultiContext(_Handle):
    """A set of GPUs driven from THIS process (ccal_multi): one context per listed device plus the transport of the step's
    all-reduce - RCCL when the devices differ, the library's in-process transport when a device is listed more than once."""
    _destroy = "ccal_multi_destroy"

    def __init__(self, devices, transport: int | None = None, lib=None):
        """transport: None = automatic, _ffi.TRANSPORT_RCCL / TRANSPORT_INPROC = that one or an error (ccal_multi_create_transport).
        lib: another build of the library (tests: _ffi.load_legacy(), which carries the fault-injection hook)."""
        self.lib = lib if lib is not None else _ffi.load()
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        _check(self.lib.ccal_multi_create_transport(_ptr(devs), len(devs), -1 if transport is None else int(transport), C.byref(h)),
               "ccal_multi_create", lambda: (self.lib.ccal_create_last_error() or b"").decode())
        self.handle = h
        self.devices = [int(d) for d in devs]
        self._problems = weakref.WeakSet()

    @property
    def transport(self) -> int:
        return int(self.lib.ccal_multi_transport(self.handle))

    @property
    def rccl_ranks(self) -> int:
        """Ranks RCCL itself counts in this set's communicators (ncclCommCount); 0 when the transport is not RCCL."""
        return int(self.lib.ccal_multi_rccl_ranks(self.handle))

    def last_error(self) -> str:
        return (self.lib.ccal_multi_last_error(self.handle) or b"").decode()

    def set_model_conventions(self, cv):
        _check(self.lib.ccal_multi_set_model_conventions(self.handle, C.byref(cv) if cv is not None else None),
               "ccal_multi_set_model_conventions")

    def sync(self):
        self._call("ccal_multi_sync")


class _ProblemBase(_Handle):
    """What Problem and MultiProblem share: a ccal_problem or ccal_multi_problem made from a description in `owner` (a Context or
    a MultiContext), and the calls that differ only in the prefix `_pre` of their C names."""
    _pre = ""

    def __init__(self, owner, desc: _ffi.ProblemDesc, keep=None):
        self._owner = owner
        self.lib = owner.lib
        self._keep = keep
        h = C.c_void_p()
        where = self._pre + "problem_create"
        _check(getattr(self.lib, where)(owner.handle, C.byref(desc), C.byref(h)), where, owner.last_error)
        self.handle = h
        owner._problems.add(self)
        self.n_cams = desc.n_cams
        self.n_slots = desc.n_slots
        self.n_obs = int(desc.n_obs)               # from the description the library holds, not from the keep-alive arrays

    @classmethod
    def from_synth(cls, ctx, sp):
        d, keep = desc_from_synth(sp)
        return cls(ctx, d, keep)

    def _detail(self) -> str:
        return self._owner.last_error()

    # -- constraints (tiny_solver::Problem::set_variable_bounds / fix_variable) -------------------
    def set_bounds(self, cam, idx, lo, hi):
        self._call(self._pre + "set_bounds", cam, idx, lo, hi)

    def fix_param(self, cam, idx):
        self._call(self._pre + "fix_param", cam, idx)

    def unfix_param(self, cam, idx):
        self._call(self._pre + "unfix_param", cam, idx)

    def apply_reference_bounds(self):
        self._call(self._pre + "apply_reference_bounds")

    def disable_distortions(self, n: int, intr: np.ndarray):
        self._call(self._pre + "disable_distortions", n, _ptr(intr))

    def _params(self, intr, poses, extr):
        intr = _f64(intr, (self.n_cams, PMAX))
        poses = _f64(poses, (self.n_slots, 6))
        extr = _f64(np.zeros((self.n_cams, 6)) if extr is None else extr, (self.n_cams, 6))
        return intr, poses, extr

    def _param_ptrs(self, intr, poses, extr):
        return tuple(map(_ptr, self._params(intr, poses, extr)))

    def upload_params(self, intr, poses, extr=None):
        self._call(self._pre + "upload_params", *self._param_ptrs(intr, poses, extr))

    # -- pose initialisation (src/util.rs:418-436) ---------------------------------------------------
    def _init_poses(self, where, *args):
        poses = np.zeros((max(self.n_obs, 1), 6)); used = np.zeros(max(self.n_obs, 1), dtype=np.int32)
        self._call(where, *args, _ptr(poses), _ptr(used))
        return poses[:self.n_obs], used[:self.n_obs]

    def init_poses(self, intr, min_points: int = 10):
        """T_cam_board per observation frame [n_obs, 6] and the number of corners used (0 = no pose)."""
        return self._init_poses(self._pre + "init_poses", _ptr(_f64(intr, (self.n_cams, PMAX))), int(min_points))

    # -- validation ---------------------------------------------------------------------------------
    def validation(self, cam, intr, poses, extr=None):
        """validation() statistics (avg of the lowest 99 %, median); a MultiProblem's, over the shards, are bit-identical to
        Problem.validation."""
        a = C.c_double(); m = C.c_double()
        self._call(self._pre + "validation", cam, *self._param_ptrs(intr, poses, extr), C.byref(a), C.byref(m))
        return a.value, m.value

    def _solve(self, intr, poses, extr, opts, raise_on_error):
        """The solve call on host arrays the library updates in place: (intr, poses, extr, report)."""
        rep = _ffi.Report()
        self._call(self._pre + "solve", C.byref(opts or default_opts()), _ptr(intr), _ptr(poses), _ptr(extr), C.byref(rep),
                   ok=_solve_ok(raise_on_error))
        return intr, poses, extr, rep


class MultiProblem(_ProblemBase):
    """One problem whose frame slots the library shards over the GPUs of a MultiContext (ccal_multi_problem)."""
    _pre = "ccal_multi_"
    _destroy = "ccal_multi_problem_destroy"

    def __init__(self, mctx: MultiContext, desc: _ffi.ProblemDesc, keep=None):
        self.mctx = mctx
        super().__init__(mctx, desc, keep)
        self.n_shards = int(self.lib.ccal_multi_problem_num_shards(self.handle))

    @classmethod
    def from_synth(cls, mctx: MultiContext, sp) -> "MultiProblem":
        return super().from_synth(mctx, sp)

    def slot_range(self, i: int):
        a = C.c_int32(); b = C.c_int32()
        self._call("ccal_multi_problem_slot_range", i, C.byref(a), C.byref(b))
        return a.value, b.value

    def shard_handle(self, i: int):
        return C.c_void_p(self.lib.ccal_multi_problem_shard(self.handle, i))

    def shard_sizes(self, i: int):
        """(corners, doubles of J_out) of shard i: the sizes of its mode-E output buffers."""
        h = self.shard_handle(i)
        return int(self.lib.ccal_num_corners(h)), int(self.lib.ccal_jacobian_len(h))

    def eval_dev(self, r_dev_ptrs, J_dev_ptrs, apply_loss=False):
        """ccal_multi_eval_dev: mode E on every shard (device buffers on the shard's own GPU); enqueues only - MultiContext.sync()."""
        n = self.n_shards
        ra = (C.c_void_p * n)(*[C.c_void_p(int(x)) for x in r_dev_ptrs]); ja = (C.c_void_p * n)(*[C.c_void_p(int(x)) for x in J_dev_ptrs])
        self._call("ccal_multi_eval_dev", 1 if apply_loss else 0, ra, ja)

    def reprojection_errors(self, intr, poses, extr=None):
        """Per-corner Euclidean reprojection errors in the corner order of the description this problem was made from."""
        offs = self._keep["obs_offsets"]
        e = np.empty(int(offs[-1]))
        self._call("ccal_multi_reprojection_errors", *self._param_ptrs(intr, poses, extr), _ptr(e), _ptr(offs))
        return e

    def solve(self, intr, poses, extr=None, opts: _ffi.SolverOpts | None = None, raise_on_error=True):
        """ccal_multi_solve: ONE call, every GPU of the set; poses in the caller's slot order."""
        return self._solve(*(a.copy() for a in self._params(intr, poses, extr)), opts, raise_on_error)


def solve_sharded(problems, intr, poses_list, extr=None, opts: _ffi.SolverOpts | None = None, raise_on_error=True):
    """ccal_solve_sharded: shards built by the caller (one Problem per context), solved as ONE problem from this thread."""
    n = len(problems)
    lib = problems[0].lib
    n_cams = problems[0].n_cams
    intr = _f64(intr, (n_cams, PMAX)).copy()
    extr = _f64(np.zeros((n_cams, 6)) if extr is None else extr, (n_cams, 6)).copy()
    poses = [_f64(p, (q.n_slots, 6)).copy() for p, q in zip(poses_list, problems)]
    opts = opts or default_opts()
    hs = (C.c_void_p * n)(*[p.handle for p in problems])
    pa = (C.POINTER(C.c_double) * n)(*[_ptr(p) for p in poses])
    rep = _ffi.Report()
    _check(lib.ccal_solve_sharded(hs, n, C.byref(opts), _ptr(intr), pa, _ptr(extr), C.byref(rep)), "ccal_solve_sharded",
           problems[0].ctx.last_error, _solve_ok(raise_on_error))
    return intr, poses, extr, rep


class Covariance:
    """What Problem.covariance returns: cov_cam [K, K], cov_poses [n_slots, 6, 6] (NaN blocks for empty slots) or None, leverage
    [n_corners] or None, slot_status [n_slots] int32 (1: no corner, no pose) and the call's report (_ffi.CovReport)."""
    __slots__ = ("cov_cam", "cov_poses", "leverage", "slot_status", "report")

    def __init__(self, cov_cam, cov_poses, leverage, slot_status, report):
        self.cov_cam, self.cov_poses, self.leverage, self.slot_status, self.report = cov_cam, cov_poses, leverage, slot_status, report


class Problem(_ProblemBase):
    """Calib-frame inputs resident in HBM (ccal_problem)."""
    _pre = "ccal_"
    _destroy = "ccal_problem_destroy"
    _pin_poses = None

    def __init__(self, ctx: Context, desc: _ffi.ProblemDesc, keep=None):
        self.ctx = ctx
        super().__init__(ctx, desc, keep)
        self.n_corners = int(self.lib.ccal_num_corners(self.handle))
        self.K = int(self.lib.ccal_reduced_dim(self.handle))
        self.j_len = int(self.lib.ccal_jacobian_len(self.handle))
        self._cb = None

    def block_dim(self, cam: int = 0) -> int:
        return int(self.lib.ccal_block_dim(self.handle, cam))

    def eff_num_params(self, cam: int = 0) -> int:
        return int(self.lib.ccal_eff_num_params(self.handle, cam))

    def set_allreduce(self, fn):
        """fn(device_ptr:int, count:int, stream:int) -> int; kept alive on the object."""
        if fn is None:
            self._cb = None
            self._call("ccal_set_allreduce", C.cast(None, _ffi.ALLREDUCE_FN), None)
            return
        def tramp(user, ptr, count, stream):
            try:
                return int(fn(ptr or 0, int(count), stream or 0) or 0)
            except Exception:   # never unwind through C
                import traceback; traceback.print_exc()
                return 1
        self._cb = _ffi.ALLREDUCE_FN(tramp)
        self._call("ccal_set_allreduce", self._cb, None)

    def set_rccl_comm(self, comm: "int | None"):
        """ncclComm_t (from Context.rccl_comm_create or the host's own RCCL): the library issues the step's all-reduce itself."""
        self._call("ccal_set_rccl_comm", C.c_void_p(comm) if comm else None)

    # -- mode E -----------------------------------------------------------------------------------
    def eval(self, intr, poses, extr=None, apply_loss=False):
        r = np.empty((self.n_corners, 2)); J = np.empty(self.j_len)
        self._call("ccal_eval", *self._param_ptrs(intr, poses, extr), 1 if apply_loss else 0, _ptr(r), _ptr(J))
        return r, J

    def download_params(self):
        intr = np.zeros((self.n_cams, PMAX)); poses = np.zeros((self.n_slots, 6)); extr = np.zeros((self.n_cams, 6))
        self._call("ccal_download_params", _ptr(intr), _ptr(poses), _ptr(extr))
        return intr, poses, extr

    def eval_dev(self, r_dev_ptr: int, J_dev_ptr: int, apply_loss=False):
        self._call("ccal_eval_dev", 1 if apply_loss else 0, C.c_void_p(r_dev_ptr), C.c_void_p(J_dev_ptr))

    # -- mode N -----------------------------------------------------------------------------------
    def build_normal(self, intr, poses, extr=None, lam=0.0):
        S = np.empty((self.K, self.K)); b = np.empty(self.K); cost = C.c_double()
        self._call("ccal_build_normal", *self._param_ptrs(intr, poses, extr), float(lam), _ptr(S), _ptr(b), C.byref(cost))
        return S, b, cost.value

    def build_normal_dev(self, lam=0.0):
        self._call("ccal_build_normal_dev", float(lam))

    def solve(self, intr, poses, extr=None, opts: _ffi.SolverOpts | None = None, raise_on_error=True, pinned=False):
        intr, poses, extr = self._params(intr, poses, extr)
        if pinned:
            # the host keeps its pose array pinned (ccal_pin_buffer, once per problem): the library reads the start from it and
            # writes the result into it, no staging copy either way.  The arrays returned are that buffer (valid until the next call)
            if self._pin_poses is None:
                self._pin_poses = self.ctx.pin(np.zeros((max(self.n_slots, 1), 6)))
            np.copyto(self._pin_poses[:self.n_slots], poses)
            poses = self._pin_poses[:self.n_slots]
        else:
            poses = poses.copy()
        return self._solve(intr.copy(), poses, extr.copy(), opts, raise_on_error)

    def solve_dev(self, opts: _ffi.SolverOpts | None = None, raise_on_error=True) -> _ffi.Report:
        """ccal_solve_dev: start from the parameters on the device (upload_params / a previous solve), leave the result
        there (download_params fetches it)."""
        rep = _ffi.Report()
        self._call("ccal_solve_dev", C.byref(opts or default_opts()), C.byref(rep), ok=_solve_ok(raise_on_error))
        return rep

    @staticmethod
    def solve_batch(problems, opts: _ffi.SolverOpts | None = None, starts=None):
        """ccal_solve_batch: independent problems (ideally one context each) solved side by side from this thread.
        starts = None: device-resident (every problem starts from what upload_params / a previous solve left on the device,
        download_params fetches the results); else a list of (intr, poses, extr) per problem, returned updated.
        Returns (reports, results-or-None); a problem's own verdict is in its report."""
        n = len(problems)
        lib = problems[0].lib if n else _ffi.load()
        opts = opts or default_opts()
        hs = (C.c_void_p * max(n, 1))(*[p.handle for p in problems])
        reps = (_ffi.Report * max(n, 1))()
        results, arrays = None, (None, None, None)
        if starts is not None:
            results = [tuple(a.copy() for a in p._params(*start)) for p, start in zip(problems, starts)]
            arrays = [(C.POINTER(C.c_double) * max(n, 1))(*[_ptr(r[k]) for r in results]) for k in range(3)]
        _check(lib.ccal_solve_batch(hs, n, C.byref(opts), *arrays, reps), "ccal_solve_batch", problems[0].ctx.last_error if n else "")
        return [reps[i] for i in range(n)], results

    def init_poses_division(self, lam: float, min_points: int = 10):
        """init_pose (src/optimization/linear.rs:5-21) of every observation frame: division-model bearings + planar PnP."""
        return self._init_poses("ccal_init_poses_division", float(lam), int(min_points))

    def reprojection_errors(self, intr, poses, extr=None):
        e = np.empty(self.n_corners)
        self._call("ccal_reprojection_errors", *self._param_ptrs(intr, poses, extr), _ptr(e))
        return e

    # -- calibration uncertainty (ccal_covariance, ccal_kernels_cov.hip) -----------------------------------------------------------
    def covariance(self, intr=None, poses=None, extr=None, poses_cov=True, leverage=True, raise_on_error=True) -> "Covariance":
        """The covariance of the camera block and of every board pose and the leverage of every corner at a solved point, by the
        rule stated at ccal_covariance in include/ccal.h.  intr None: the point on the device (upload_params / a device-resident
        solve); else intr, poses (and extr for a rig) as for eval.  poses_cov / leverage False: that output is not fetched (None
        in the result).  CCAL_ERR_NOT_PD raises unless raise_on_error is False: the report then names the slot."""
        if intr is None:
            if poses is not None or extr is not None:
                raise ValueError("covariance: poses / extr without intr (intr None means the point on the device)")
            point = (None, None, None)
        else:
            if poses is None and self.n_slots:
                raise ValueError("covariance: poses is missing")
            if extr is None and self.n_cams > 1:
                raise ValueError("covariance: extr is missing (a rig)")
            point = self._param_ptrs(intr, np.zeros((0, 6)) if poses is None else poses, extr)
        cov_cam = np.full((self.K, self.K), np.nan)
        cov_p = _out(self.n_slots, 6, 6) if poses_cov else None
        lev = _out(self.n_corners) if leverage else None
        status = _out(self.n_slots, dtype=np.int32)
        rep = _ffi.CovReport()
        self._call("ccal_covariance", *point, _ptr(cov_cam), _ptr(cov_p), _ptr(lev), _ptr(status), C.byref(rep),
                   ok=_OK if raise_on_error else (_ffi.OK, _ffi.ERR_NOT_PD))
        return Covariance(cov_cam, None if cov_p is None else cov_p[:self.n_slots], None if lev is None else lev[:self.n_corners],
                          status[:self.n_slots], rep)

    def _release(self):
        if self._pin_poses is not None and self.ctx.handle:
            try:
                self.ctx.unpin(self._pin_poses)          # (before the array goes: the registration must not outlive the memory)
            finally:
                self._pin_poses = None
