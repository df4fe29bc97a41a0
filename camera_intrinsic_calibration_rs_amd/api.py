"""Host-side mirror of the reference's calib-frame API for the hot path (same names, argument
meaning and error behaviour), driving the HIP engine through the C ABI.

  reference (Rust)                                             here
  ---------------------------------------------------------   ------------------------------------------
  detected_points::FeaturePoint / FrameFeature                 FeaturePoint / FrameFeature
  types::RvecTvec (+ to_na_isometry3 / to_rvec_tvec)            RvecTvec
  camera_intrinsic_model::GenericModel<f64>                     GenericModel
  optimization::factors::ReprojectionFactor::residual_func      ReprojectionFactor.residual_func
  optimization::factors::OtherCamReprojectionFactor             OtherCamReprojectionFactor.residual_func
  util::calib_camera                (src/util.rs:384-490)       calib_camera
  util::calib_all_camera_with_extrinsics (src/util.rs:567-715)  calib_all_camera_with_extrinsics
  util::validation                  (src/util.rs:721-795)       validation
  io::write_report / object_to_json (src/io.rs)                 write_report / model_to_json / poses_to_json / ...
  types::CalibParams                (src/types.rs:6-10)         CalibParams
  util::find_best_two_frames_idx    (src/util.rs:168-219)       find_best_two_frames_idx
  optimization::homography::radial_distortion_homography        radial_distortion_homography (+ rdh_sample_indices)
  optimization::homography::homography_to_focal                 homography_to_focal
  optimization::linear::init_pose   (linear.rs:5-21)            init_pose
  GenericModel::project / unproject, estimate_new_camera_matrix_for_undistort, init_undistort_map
                                    (examples/convert_model.rs:27-29)   GenericModel methods of the same names
  remap                             (examples/test_pnp.rs:80)           remap (+ engine.UndistortMap for batches)
  the sub-pixel step that ends image_to_option_feature_frame
                                    (src/data_loader.rs:36-70)          refine_corners, redetect_corners (no tag detector here)
  board::BoardConfig / Board::init_aprilgrid (src/board.rs:7-95)        AprilGridBoard
  image_to_option_feature_frame's corner naming id = tag_id * 4 + i     frames_from_tags
  what tag_detector.detect decides for a quad (the absent aprilgrid crate; this project's rule, the family supplied by the
  caller, quads not proposed here)                                      decode_tags, TagFamily
  what tag_detector.detect does for an AprilGrid image as a whole (this project's rules: saddles, their refinement, tag
  outlines from the saddles, the decoder)                               detect_aprilgrid, propose_quads, merge_points
  the same up to the tags, in one device-resident call                  detect_tags (detect_aprilgrid(fused=True))
  a detector for plain checkerboards (the reference's tag detector is in the absent aprilgrid crate)
                                                                        detect_checkerboard, assemble_checkerboard
  the same in one device-resident call                                  detect_checkerboard(fused=True)
  (util::try_init_camera / init_and_calibrate_one_camera, src/util.rs:107-159, 831-911: the glue over these pieces is
   not here yet - see README, "From detections alone")

Differences, on purpose: (1) `calib_camera` takes the per-frame initial poses as an argument (the
reference computes them inside with sqpnp, src/util.rs:418-436, which is outside the hot path); frames
without an initial pose are rejected up front instead of reproducing the reference's latent bug of
adding residual blocks that have no initial value (src/util.rs:431-433 vs 407-414).  (2) corner order
inside a frame is by corner id, not HashMap order (the reference is not reproducible with itself,
SURVEY 0.5); results agree at the converged optimum.  `None` is returned where the reference returns
`None` (solver failure); nothing here falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from .engine import (CcalError, Context, MultiContext, MultiProblem, Problem, UndistortMap, aprilgrid_target, check_images, check_maps,
                     checkerboard_target, default_opts, make_desc)
from .synth import MODEL_NAMES, MODEL_NPARAMS, PMAX, rodrigues, rotmat_to_rvec, splitmix64

_MODEL_KEYS = {
    "ucm": ["fx", "fy", "cx", "cy", "alpha"],
    "eucm": ["fx", "fy", "cx", "cy", "alpha", "beta"],
    "kb4": ["fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4"],
    "opencv5": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"],
}
# serde tags of GenericModel's variants.  UCM / EUCM / KannalaBrandt4 appear in the reference (data/eucm.json,
# examples/convert_model.rs:14,19); "OpenCVModel5" is this build's ASSUMPTION about the absent crate (one string to flip).
_JSON_NAMES = {"ucm": "UCM", "eucm": "EUCM", "kb4": "KannalaBrandt4", "opencv5": "OpenCVModel5"}
# EUCMT ("Extended Unified with Tangential", README.md:78): a PARAMETER CONTAINER here - target of the closed-form
# UCM -> EUCMT conversion (src/util.rs:236-243).  Its projection and its JSON field names live only in the absent crate.
MODEL_EUCMT = 4
_CONTAINER_KINDS = {"eucmt": (MODEL_EUCMT, 8)}


@dataclasses.dataclass
class FeaturePoint:                      # src/detected_points.rs:6-9 (f32 in the reference)
    p2d: Tuple[float, float]
    p3d: Tuple[float, float, float]


@dataclasses.dataclass
class FrameFeature:                      # src/detected_points.rs:13-17
    time_ns: int
    img_w_h: Tuple[int, int]
    features: Dict[int, FeaturePoint]


@dataclasses.dataclass
class RvecTvec:                          # src/types.rs:13-36
    rvec: Tuple[float, float, float]
    tvec: Tuple[float, float, float]

    def as6(self) -> np.ndarray:
        return np.array(list(self.rvec) + list(self.tvec), dtype=np.float64)

    @staticmethod
    def from6(v) -> "RvecTvec":
        v = [float(x) for x in v]
        return RvecTvec((v[0], v[1], v[2]), (v[3], v[4], v[5]))

    # Isometry algebra used by the problem set-up / result mapping (host side, a handful of poses)
    def matrix(self) -> Tuple[np.ndarray, np.ndarray]:
        return rodrigues(np.array(self.rvec)), np.array(self.tvec, dtype=np.float64)

    def inverse(self) -> "RvecTvec":
        R, t = self.matrix()
        return RvecTvec.from6(np.concatenate([rotmat_to_rvec(R.T), -R.T @ t]))

    def compose(self, other: "RvecTvec") -> "RvecTvec":      # self * other
        R1, t1 = self.matrix(); R2, t2 = other.matrix()
        return RvecTvec.from6(np.concatenate([rotmat_to_rvec(R1 @ R2), R1 @ t2 + t1]))


class GenericModel:
    """camera_intrinsic_model::GenericModel<f64> for the four models on the hot path."""

    def __init__(self, kind: str, params: Sequence[float], width: float, height: float):
        kind = kind.lower()
        if kind not in MODEL_NAMES and kind not in _CONTAINER_KINDS:
            raise ValueError(f"unsupported model {kind}")
        if len(params) != (_CONTAINER_KINDS[kind][1] if kind in _CONTAINER_KINDS else MODEL_NPARAMS[MODEL_NAMES[kind]]):
            raise ValueError("wrong number of parameters")
        self.kind = kind
        self._params = np.asarray(params, dtype=np.float64).copy()
        self._w, self._h = float(width), float(height)

    @property
    def model_id(self) -> int:
        return _CONTAINER_KINDS[self.kind][0] if self.kind in _CONTAINER_KINDS else MODEL_NAMES[self.kind]

    def params(self) -> np.ndarray:
        return self._params.copy()

    def set_params(self, p) -> None:
        self._params = np.asarray(p, dtype=np.float64).copy()

    def width(self) -> float:
        return self._w

    def height(self) -> float:
        return self._h

    def set_w_h(self, w: int, h: int) -> None:
        self._w, self._h = float(w), float(h)

    def copy(self) -> "GenericModel":
        return GenericModel(self.kind, self._params, self._w, self._h)

    # -- applying the model (the tail of examples/convert_model.rs and examples/test_pnp.rs) --------------------------------------
    def _usable(self, what: str) -> None:
        if self.kind in _CONTAINER_KINDS:
            raise CcalError(_ffi.ERR_UNSUPPORTED, what, f"{self.kind} is a parameter container: its projection lives only in the absent crate")

    def project(self, p3ds, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
        """GenericModel::project: camera-frame points [n, 3] -> (uv [n, 2], valid [n]); rows where it is undefined are NaN."""
        self._usable("project")
        p3ds = np.asarray(p3ds, dtype=np.float64)
        if p3ds.ndim != 2 or p3ds.shape[1] != 3:
            raise ValueError("project: an [n, 3] array of points")
        return _ctx(ctx).project_points(self.model_id, self._params, p3ds)

    def unproject(self, p2ds, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
        """GenericModel::unproject: pixels [n, 2] -> (rays [n, 3], valid [n]); a unit ray, NaN where there is none."""
        self._usable("unproject")
        p2ds = np.asarray(p2ds, dtype=np.float64)
        if p2ds.ndim != 2 or p2ds.shape[1] != 2:
            raise ValueError("unproject: an [n, 2] array of pixels")
        return _ctx(ctx).unproject_points(self.model_id, self._params, p2ds)

    def estimate_new_camera_matrix_for_undistort(self, balance: float, new_w_h: Optional[Tuple[int, int]] = None,
                                                 ctx: Optional[Context] = None) -> Optional[np.ndarray]:
        """The pinhole matrix [3, 3] whose image holds the four edge midpoints' rays; balance 0 keeps every output pixel inside
        the source image along the tighter axis, 1 keeps the whole source along the wider one.  None where an edge midpoint has
        no ray in front of the camera."""
        self._usable("estimate_new_camera_matrix_for_undistort")
        if not (0.0 <= float(balance) <= 1.0):                      # also refuses NaN
            raise ValueError("balance must lie in [0, 1]")
        if new_w_h is not None and (len(new_w_h) != 2 or int(new_w_h[0]) <= 0 or int(new_w_h[1]) <= 0):
            raise ValueError("new_w_h: a positive (width, height)")
        return _ctx(ctx).estimate_new_camera_matrix(self.model_id, self._params, int(round(self._w)), int(round(self._h)),
                                                    float(balance), new_w_h)

    def init_undistort_map(self, projection_mat, new_w_h: Tuple[int, int], rotation=None,
                           ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(xmap, ymap), f32 [h, w]: for every pixel of the new pinhole image `projection_mat` (3 x 3; `rotation` 3 x 3 from the
        camera frame to the new one, None = identity) the source pixel it is sampled from, NaN where the model has none."""
        self._usable("init_undistort_map")
        K = np.asarray(projection_mat, dtype=np.float64)
        if K.shape != (3, 3):
            raise ValueError("projection_mat: a 3 x 3 matrix")
        if rotation is not None and np.asarray(rotation).shape != (3, 3):
            raise ValueError("rotation: a 3 x 3 matrix")
        if len(new_w_h) != 2 or int(new_w_h[0]) <= 0 or int(new_w_h[1]) <= 0:
            raise ValueError("new_w_h: a positive (width, height)")
        m = _ctx(ctx).undistort_map(self.model_id, self._params, K, new_w_h, rotation)
        try:
            return m.download()
        finally:
            m.close()

    # cam{i}.json: {"EUCM": {"fx":..,"fy":..,"cx":..,"cy":..,"alpha":..,"beta":..,"width":..,"height":..}} (data/eucm.json)
    def to_json_obj(self) -> dict:
        if self.kind in _CONTAINER_KINDS:
            raise NotImplementedError(f"{self.kind}: the JSON field names are defined only in the absent camera-intrinsic-model crate")
        d = {k: float(v) for k, v in zip(_MODEL_KEYS[self.kind], self._params)}
        d["width"] = int(round(self._w)); d["height"] = int(round(self._h))
        return {_JSON_NAMES[self.kind]: d}

    @staticmethod
    def from_json_obj(obj: dict) -> "GenericModel":
        (name, d), = obj.items()
        kind = {v: k for k, v in _JSON_NAMES.items()}[name]
        return GenericModel(kind, [d[k] for k in _MODEL_KEYS[kind]], d["width"], d["height"])


def model_to_json(path: str, model: GenericModel) -> None:
    with open(path, "w") as f:
        json.dump(model.to_json_obj(), f, indent=2)


def model_from_json(path: str) -> GenericModel:
    with open(path) as f:
        return GenericModel.from_json_obj(json.load(f))


def poses_to_json(path: str, poses: Dict[int, RvecTvec]) -> None:
    """cam{i}_poses.json: BTreeMap frame-index -> {"rvec":[3],"tvec":[3]} (src/bin/camera_calibration.rs:288-293)."""
    with open(path, "w") as f:
        json.dump({str(k): {"rvec": list(v.rvec), "tvec": list(v.tvec)} for k, v in sorted(poses.items())}, f, indent=2)


def poses_from_json(path: str) -> Dict[int, RvecTvec]:
    with open(path) as f:
        return {int(k): RvecTvec(tuple(v["rvec"]), tuple(v["tvec"])) for k, v in json.load(f).items()}


def extrinsics_to_json(path: str, rtvecs: Sequence[RvecTvec]) -> None:
    """extrinsics.json: {"rtvecs":[{"rvec":..,"tvec":..},..]} (src/types.rs:41-44)."""
    with open(path, "w") as f:
        json.dump({"rtvecs": [{"rvec": list(r.rvec), "tvec": list(r.tvec)} for r in rtvecs]}, f, indent=2)


def extrinsics_from_json(path: str) -> List[RvecTvec]:
    with open(path) as f:
        return [RvecTvec(tuple(v["rvec"]), tuple(v["tvec"])) for v in json.load(f)["rtvecs"]]


def write_report(path: str, with_extrinsic: bool, rep_rms: Sequence[Tuple[float, float]]) -> None:
    """src/io.rs:21-31, byte for byte."""
    s = f"Calibrate with extrinsics: {'true' if with_extrinsic else 'false'}\n\n"
    for i, (avg, med) in enumerate(rep_rms):
        s += f"cam{i}:\n    average reprojection error: {avg:.5f} px\n    median  reprojection error: {med:.5f} px\n\n"
    with open(path, "w") as f:
        f.write(s)


_default_ctx: Optional[Context] = None


def _ctx(ctx: Optional[Context]) -> Context:
    global _default_ctx
    if ctx is not None:
        return ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def remap(img, xmap, ymap, ctx: Optional[Context] = None) -> np.ndarray:
    """remap: one image [H][W] (uint8 / uint16) or [H][W][3] (uint8) resampled bilinearly through the maps -> the maps' shape, same
    dtype; 0 where the map points outside the image or is NaN.  For many frames through one map keep an engine.UndistortMap."""
    xmap, ymap = check_maps(xmap, ymap)
    img, _, _ = check_images(img, False)
    m = _ctx(ctx).undistort_map_from_arrays(xmap, ymap)
    try:
        return m.remap(img[None])[0]
    finally:
        m.close()


class _Opened:
    """A problem on one context, or - `devices` given - sharded by the library over a device set of this process
    (ccal_multi_*: one call, every listed GPU; a device listed twice = two shards on it)."""

    def __init__(self, ctx: Optional[Context], devices: Optional[Sequence[int]], d, keep):
        self.mctx = None
        if devices is not None:
            self.mctx = MultiContext(list(devices))
            try:
                self.prob = MultiProblem(self.mctx, d, keep)
            except Exception:
                self.mctx.close()
                raise
        else:
            self.prob = Problem(_ctx(ctx), d, keep)

    def __enter__(self):
        return self.prob

    def __exit__(self, *exc):
        self.prob.close()
        if self.mctx is not None:
            self.mctx.close()
        return False


def _points_f32(ff: FrameFeature):
    """(ids, p3d [n, 3], p2d [n, 2]) of a frame in the order of its sorted feature ids, f64 values of the f32 numbers that the
    reference holds detections and board points in (src/detected_points.rs:6-9)."""
    ids = sorted(ff.features.keys())
    return (ids, np.asarray([ff.features[k].p3d for k in ids], dtype=np.float32).astype(np.float64).reshape(-1, 3),
            np.asarray([ff.features[k].p2d for k in ids], dtype=np.float32).astype(np.float64).reshape(-1, 2))


def _flatten(cams_frames: Sequence[Sequence[Optional[FrameFeature]]], use: Sequence[Sequence[int]]):
    """(cam, frame index) observation frames -> CSR + SoA arrays; slots = sorted union of frame indices."""
    slots = sorted({i for idxs in use for i in idxs})
    slot_of = {fi: s for s, fi in enumerate(slots)}
    obs_cam, obs_slot, offs, X, U = [], [], [0], [], []
    for fi in slots:                                     # a slot's observations stay adjacent
        for c, idxs in enumerate(use):
            if fi not in idxs:
                continue
            ff = cams_frames[c][fi]
            ids = sorted(ff.features.keys())
            X += [ff.features[k].p3d for k in ids]
            U += [ff.features[k].p2d for k in ids]
            obs_cam.append(c); obs_slot.append(slot_of[fi]); offs.append(offs[-1] + len(ids))
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3); U = np.asarray(U, dtype=np.float32).reshape(-1, 2)
    return slots, obs_cam, obs_slot, offs, X, U


def _intr_matrix(cameras: Sequence[GenericModel]) -> np.ndarray:
    intr = np.zeros((len(cameras), PMAX))
    for c, m in enumerate(cameras):
        intr[c, :len(m._params)] = m._params
    return intr


def init_frame_poses(frame_feature_list: Sequence[Optional[FrameFeature]], generic_camera: GenericModel,
                     min_points: int = 10, ctx: Optional[Context] = None, devices: Optional[Sequence[int]] = None) -> Dict[int, RvecTvec]:
    """The pose initialisation inside calib_camera (src/util.rs:418-436): `unproject` the detections with
    the current model, keep the valid ones, normalise by z, PnP -- one wavefront per frame (the planar homography for frames at
    z = 0, the general PnP of ccal_pnp_batch for any other target)."""
    valid = [i for i, f in enumerate(frame_feature_list) if f is not None]
    if not valid:
        return {}
    slots, obs_cam, obs_slot, offs, X, U = _flatten([frame_feature_list], [valid])
    d, keep = make_desc(1, [generic_camera.model_id], [generic_camera.width()], [generic_camera.height()], False,
                        len(slots), obs_cam, obs_slot, offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    with _Opened(ctx, devices, d, keep) as prob:
        poses, used = prob.init_poses(_intr_matrix([generic_camera]), min_points)
    return {fi: RvecTvec.from6(poses[s]) for s, fi in enumerate(slots) if used[s] > 0}


def calib_camera(frame_feature_list: Sequence[Optional[FrameFeature]], generic_camera: GenericModel,
                 xy_same_focal: bool, disabled_distortions: int, fixed_focal: bool,
                 initial_poses: Optional[Dict[int, RvecTvec]] = None, ctx: Optional[Context] = None,
                 opts: Optional[_ffi.SolverOpts] = None, devices: Optional[Sequence[int]] = None
                 ) -> Optional[Tuple[GenericModel, Dict[int, RvecTvec]]]:
    """util::calib_camera (src/util.rs:384-490): single-camera bundle adjustment, Gauss-Newton.
    `initial_poses=None` reproduces the reference's in-function initialisation (unproject + planar PnP
    per frame on the GPU, frames with fewer than 10 valid points are skipped, src/util.rs:418-436).
    `devices`: still ONE call of ONE process, like the reference's - the library shards the frames over the listed GPUs
    (ccal_multi_*), one all-reduce per Gauss-Newton step."""
    if initial_poses is None:
        initial_poses = init_frame_poses(frame_feature_list, generic_camera, ctx=ctx, devices=devices)
    valid = [i for i, f in enumerate(frame_feature_list) if f is not None and i in initial_poses]
    if not valid:
        return None
    slots, obs_cam, obs_slot, offs, X, U = _flatten([frame_feature_list], [valid])
    d, keep = make_desc(1, [generic_camera.model_id], [generic_camera.width()], [generic_camera.height()],
                        xy_same_focal, len(slots), obs_cam, obs_slot, offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    with _Opened(ctx, devices, d, keep) as prob:
        intr = _intr_matrix([generic_camera])
        poses = np.stack([initial_poses[i].as6() for i in slots])
        prob.apply_reference_bounds()                                  # src/util.rs:446
        prob.disable_distortions(disabled_distortions, intr)           # src/util.rs:447-454
        try:
            intr, poses, _, rep = prob.solve(intr, poses, None, opts or default_opts())      # :455
        except CcalError:
            return None                                                # result_option.as_ref()?  -> None
        if fixed_focal:                                                # :459-464 "set focal and opt again."
            prob.fix_param(0, 0)
            intr[0, 0] = generic_camera.params()[0]
            if xy_same_focal:
                intr[0, 1] = intr[0, 0]
            intr, poses, _, rep = prob.solve(intr, poses, None, opts or default_opts())      # .unwrap()
        out = generic_camera.copy()
        out.set_params(intr[0, :len(generic_camera._params)])          # fy = f re-inserted by the engine (:467-470)
        return out, {fi: RvecTvec.from6(poses[s]) for s, fi in enumerate(slots)}


def calib_cameras(cams_frame_feature_lists: Sequence[Sequence[Optional[FrameFeature]]], generic_cameras: Sequence[GenericModel],
                  xy_same_focal: bool, disabled_distortions: int, fixed_focal: bool, device: int = 0,
                  opts: Optional[_ffi.SolverOpts] = None, devices: Optional[Sequence[int]] = None
                  ) -> List[Optional[Tuple[GenericModel, Dict[int, RvecTvec]]]]:
    """The per-camera loop of the tool - `for cam in 0..cam_num { calib_camera(...) }` (src/bin/camera_calibration.rs:255-265) -
    as ONE ccal_solve_batch: every camera's single-camera problem on a context of its own, solved side by side (a session-
    sized problem leaves the GPU almost idle).  `devices`: the cameras' contexts are placed round-robin on the listed GPUs
    (independent sessions are the path's most natural multi-GPU split at session size: no collective at all); default: all on
    `device`.  Entry i equals calib_camera(cams_frame_feature_lists[i], generic_cameras[i], ...) - same verdict and iteration
    count, results to the order of summation (ccal_solve_batch sizes every problem's launches for its share of its GPU)."""
    n = len(generic_cameras)
    devs = [int(d) for d in devices] if devices else [int(device)]
    ctxs = [Context(devs[c % len(devs)]) for c in range(n)]
    out: List[Optional[Tuple[GenericModel, Dict[int, RvecTvec]]]] = [None] * n
    jobs = []                                       # (camera, problem, slots, intr, poses)
    try:
        for c in range(n):
            frames, cam = cams_frame_feature_lists[c], generic_cameras[c]
            init = init_frame_poses(frames, cam, ctx=ctxs[c])
            valid = [i for i, f in enumerate(frames) if f is not None and i in init]
            if not valid:
                continue
            slots, obs_cam, obs_slot, offs, X, U = _flatten([frames], [valid])
            d, keep = make_desc(1, [cam.model_id], [cam.width()], [cam.height()], xy_same_focal, len(slots), obs_cam, obs_slot, offs,
                                X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
            prob = Problem(ctxs[c], d, keep)
            intr = _intr_matrix([cam])
            prob.apply_reference_bounds()
            prob.disable_distortions(disabled_distortions, intr)
            jobs.append([c, prob, slots, intr, np.stack([init[i].as6() for i in slots])])
        o = opts or default_opts()
        reps, res = Problem.solve_batch([j[1] for j in jobs], o, starts=[(j[3], j[4], None) for j in jobs])
        alive = []
        for j, rep, r in zip(jobs, reps, res):
            if rep.status not in (_ffi.OK, _ffi.ERR_NO_CONVERGENCE):
                continue                                                # result_option.as_ref()?  -> None
            j[3], j[4] = r[0], r[1]
            alive.append(j)
        if fixed_focal and alive:                                       # src/util.rs:459-464 "set focal and opt again."
            for j in alive:
                j[1].fix_param(0, 0)
                j[3][0, 0] = generic_cameras[j[0]].params()[0]
                if xy_same_focal:
                    j[3][0, 1] = j[3][0, 0]
            reps, res = Problem.solve_batch([j[1] for j in alive], o, starts=[(j[3], j[4], None) for j in alive])
            for j, rep, r in zip(alive, reps, res):
                if rep.status not in (_ffi.OK, _ffi.ERR_NO_CONVERGENCE):     # calib_camera's second solve is `.unwrap()`ed (src/util.rs:463)
                    raise CcalError(rep.status, "ccal_solve_batch", f"camera {j[0]}: the fixed-focal re-optimisation failed")
                j[3], j[4] = r[0], r[1]
        for c, prob, slots, intr, poses in alive:
            m = generic_cameras[c].copy()
            m.set_params(intr[0, :len(m._params)])
            out[c] = (m, {fi: RvecTvec.from6(poses[s]) for s, fi in enumerate(slots)})
        return out
    finally:
        for j in jobs:
            j[1].close()
        for cx in ctxs:
            cx.close()


def _joint_problem_inputs(cameras, t_cam_i_0, cam_rtvecs, cams_detected_feature_frames, xy_same_focal):
    """Problem description and starting point of the joint problem exactly as src/util.rs:576-651 lays it out (the tests
    hand the same arrays to the oracle): slots = sorted union of the frame indices with a pose, T_0_b per slot = cam0's
    pose when it saw the frame, else T_c0^-1 * T_cb of the first camera that did (`.entry().or_insert()` in camera order)."""
    n_cams = len(cameras)
    use = [sorted(cam_rtvecs[c].keys()) for c in range(n_cams)]
    slots, obs_cam, obs_slot, offs, X, U = _flatten(cams_detected_feature_frames, use)
    if not slots:
        return None
    d, keep = make_desc(n_cams, [m.model_id for m in cameras], [m.width() for m in cameras],
                        [m.height() for m in cameras], xy_same_focal, len(slots), obs_cam, obs_slot, offs,
                        X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    intr = _intr_matrix(cameras)
    extr = np.zeros((n_cams, 6))
    for c in range(1, n_cams):
        extr[c] = t_cam_i_0[c].as6()
    poses = np.zeros((len(slots), 6))
    for s, fi in enumerate(slots):
        for c in range(n_cams):
            if fi in cam_rtvecs[c]:
                rt = cam_rtvecs[c][fi]
                poses[s] = (rt if c == 0 else t_cam_i_0[c].inverse().compose(rt)).as6()
                break
    return d, keep, slots, intr, poses, extr


def calib_all_camera_with_extrinsics(cameras: Sequence[GenericModel], t_cam_i_0: Sequence[RvecTvec],
                                     cam_rtvecs: Sequence[Dict[int, RvecTvec]],
                                     cams_detected_feature_frames: Sequence[Sequence[Optional[FrameFeature]]],
                                     xy_same_focal: bool, disabled_distortions: int, cam0_fixed_focal: bool,
                                     ctx: Optional[Context] = None, opts: Optional[_ffi.SolverOpts] = None,
                                     devices: Optional[Sequence[int]] = None
                                     ) -> Optional[Tuple[List[GenericModel], List[RvecTvec], Dict[int, RvecTvec]]]:
    """util::calib_all_camera_with_extrinsics (src/util.rs:567-715): joint intrinsics + extrinsics.
    `devices`: one call, the frame slots sharded over the listed GPUs (ccal_multi_*)."""
    n_cams = len(cameras)
    built = _joint_problem_inputs(cameras, t_cam_i_0, cam_rtvecs, cams_detected_feature_frames, xy_same_focal)
    if built is None:
        return None
    d, keep, slots, intr, poses, extr = built
    with _Opened(ctx, devices, d, keep) as prob:
        prob.apply_reference_bounds()
        prob.disable_distortions(disabled_distortions, intr)
        if cam0_fixed_focal:
            prob.fix_param(0, 0)                                       # src/util.rs:664-667
        try:
            intr, poses, extr, rep = prob.solve(intr, poses, extr, opts or default_opts())
        except CcalError:
            return None
        out_models = []
        for c, m in enumerate(cameras):
            mm = m.copy(); mm.set_params(intr[c, :len(m._params)]); out_models.append(mm)
        t_i_0 = [RvecTvec((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))] + [RvecTvec.from6(extr[c]) for c in range(1, n_cams)]
        return out_models, t_i_0, {fi: RvecTvec.from6(poses[s]) for s, fi in enumerate(slots)}


def init_camera_extrinsic(cam_rtvecs: Sequence[Dict[int, RvecTvec]], opts=None) -> List[RvecTvec]:
    """util::init_camera_extrinsic (src/util.rs:511-561): T_i_0 of every camera from the frames both it and
    camera 0 have a board pose for (SE3Factor + HuberLoss(0.5) + Gauss-Newton, in the library's host code).
    opts: the optimizer's stop rules (None = GaussNewtonOptimizer::default(), as the reference)."""
    lib = _ffi.load()
    out = [RvecTvec((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]
    for cam_i in range(1, len(cam_rtvecs)):
        keys = sorted(set(cam_rtvecs[0].keys()) & set(cam_rtvecs[cam_i].keys()))
        if not keys:
            raise ValueError(f"camera {cam_i} shares no frame with camera 0")       # the reference indexes [0] and panics
        p0 = np.ascontiguousarray(np.stack([cam_rtvecs[0][k].as6() for k in keys]))
        pi = np.ascontiguousarray(np.stack([cam_rtvecs[cam_i][k].as6() for k in keys]))
        x = np.zeros(6)
        rep = _ffi.Report()
        rc = lib.ccal_init_camera_extrinsic_opts(p0.ctypes.data_as(C.POINTER(C.c_double)), pi.ctypes.data_as(C.POINTER(C.c_double)),
                                                 len(keys), x.ctypes.data_as(C.POINTER(C.c_double)), 0,
                                                 C.byref(opts) if opts is not None else None, C.byref(rep))
        if rc != _ffi.OK:
            raise CcalError(rc, "ccal_init_camera_extrinsic")                        # `.unwrap()` in the reference
        out.append(RvecTvec.from6(x))
    return out


def convert_model(source_model: GenericModel, target_model: GenericModel, disabled_distortions: int = 0,
                  ctx: Optional[Context] = None) -> GenericModel:
    """util::convert_model (src/util.rs:224-282).  UCM -> EUCM is the closed form beta = 1 (:229-235, pinned by
    tests/util_test.rs:77-110); everything else fits the target over the reference's pixel grid with
    ModelConvertFactor (src/optimization/factors.rs:10-76) through `ccal_convert_model` on the device.  The
    reference mutates `target_model`; here the fitted model is also returned."""
    if round(source_model.width()) != round(target_model.width()):
        raise ValueError("source width and target width are not the same.")          # factors.rs:29-33: panic!
    if round(source_model.height()) != round(target_model.height()):
        raise ValueError("source height and target height are not the same.")
    if source_model.kind == "ucm" and target_model.kind == "eucm":                   # closed form: no device needed
        target_model.set_params(list(source_model.params()) + [1.0])
        return target_model
    if source_model.kind == "ucm" and target_model.kind == "eucmt":                  # src/util.rs:236-243
        target_model.set_params(list(source_model.params()) + [1.0, 0.0, 0.0])
        return target_model
    if source_model.kind in _CONTAINER_KINDS or target_model.kind in _CONTAINER_KINDS:
        raise CcalError(_ffi.ERR_UNSUPPORTED, "convert_model", "EUCMT can only be the target of the closed-form UCM conversion")
    lib = _ffi.load()
    c = _ctx(ctx)
    src = np.ascontiguousarray(source_model.params(), dtype=np.float64)
    tgt = np.ascontiguousarray(target_model.params(), dtype=np.float64).copy()
    rep = _ffi.Report()
    rc = lib.ccal_convert_model(c.handle, source_model.model_id, src.ctypes.data_as(C.POINTER(C.c_double)),
                                target_model.model_id, tgt.ctypes.data_as(C.POINTER(C.c_double)),
                                float(source_model.width()), float(source_model.height()), int(disabled_distortions),
                                None, C.byref(rep))
    if rc not in (_ffi.OK, _ffi.ERR_NO_CONVERGENCE):                                 # max_iterations: the reference keeps the result
        raise CcalError(rc, "ccal_convert_model: " + c.last_error())                 # `.unwrap()` in the reference (:276)
    target_model.set_params(tgt)
    return target_model


def init_ucm(frame_feature0: FrameFeature, frame_feature1: FrameFeature, rtvec0: RvecTvec, rtvec1: RvecTvec,
             init_f: float, init_alpha: float, fixed_focal: bool, ctx: Optional[Context] = None) -> Optional[GenericModel]:
    """util::init_ucm (src/util.rs:287-378).  UCMInitFocalAlphaFactor (factors.rs:82-120) is the reprojection
    factor of a UCM whose only free intrinsics are f = fx = fy and alpha with the principal point pinned at the
    image centre, i.e. the engine's UCM + xy_same_focal problem with cx, cy fixed; bounds f in [f0/3, 3 f0],
    alpha in [1e-6, 1] (:345-346).  Then calib_camera on the two frames with xy_same_focal = true (:365-371)."""
    w, h = frame_feature0.img_w_h
    ucm0 = GenericModel("ucm", [init_f, init_f, w / 2.0, h / 2.0, init_alpha], w, h)
    frames = [frame_feature0, frame_feature1]
    slots, obs_cam, obs_slot, offs, X, U = _flatten([frames], [[0, 1]])
    d, keep = make_desc(1, [ucm0.model_id], [w], [h], True, 2, obs_cam, obs_slot, offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    prob = Problem(_ctx(ctx), d, keep)
    try:
        prob.fix_param(0, 1); prob.fix_param(0, 2)                      # cx, cy (eff indices with fy removed)
        if fixed_focal:
            prob.fix_param(0, 0)
        prob.set_bounds(0, 0, init_f / 3.0, init_f * 3.0)
        prob.set_bounds(0, 3, 1e-6, 1.0)
        try:
            intr, _, _, _ = prob.solve(_intr_matrix([ucm0]), np.stack([rtvec0.as6(), rtvec1.as6()]), None, default_opts())
        except CcalError:
            return None
    finally:
        prob.close()
    ucm1 = GenericModel("ucm", [intr[0, 0], intr[0, 0], w / 2.0, h / 2.0, intr[0, 4]], w, h)
    res = calib_camera(frames, ucm1, True, 0, fixed_focal, None, ctx=ctx)
    if res is None:
        raise RuntimeError("The initial UCM model fitting failed. Might be wrong board configuration.")   # .expect(...)
    return res[0]


def validation(cam_idx: int, final_result: GenericModel, rtvec_list: Dict[int, RvecTvec],
               detected_feature_frames: Sequence[Optional[FrameFeature]], ctx: Optional[Context] = None,
               devices: Optional[Sequence[int]] = None) -> Tuple[float, float]:
    """util::validation (src/util.rs:721-795): (avg of the lowest 99 %, median) reprojection error in px.
    `devices`: the errors are evaluated shard by shard on the listed GPUs, the statistics are the same bits."""
    valid = [i for i in sorted(rtvec_list.keys()) if detected_feature_frames[i] is not None]
    slots, obs_cam, obs_slot, offs, X, U = _flatten([detected_feature_frames], [valid])
    d, keep = make_desc(1, [final_result.model_id], [final_result.width()], [final_result.height()], False,
                        len(slots), obs_cam, obs_slot, offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    with _Opened(ctx, devices, d, keep) as prob:
        poses = np.stack([rtvec_list[i].as6() for i in slots])
        return prob.validation(0, _intr_matrix([final_result]), poses, None)


@dataclasses.dataclass
class Uncertainty:
    """How far to trust a finished calibration (engine.Problem.covariance, the rule at ccal_covariance in include/ccal.h).
    calibration_uncertainty: param_names / param_std / param_corr are the camera's; rig_uncertainty: lists with one entry per
    camera, and extr_std [n_cams, 6] (row 0 zeros) beside them.  Standard deviations are in the parameters' own units (px, rad, m);
    a fixed parameter has 0 (and a NaN-free 0 correlation row).  pose_std / pose_cov: per frame, rvec | tvec as the solver steps
    in them.  leverage: {frame: {feature id: h}} - rig_uncertainty: one such dict per camera - h in [0, 2], their sum over all
    corners = report.n_free.  cov_cam: the reduced system's whole covariance [K, K] in the order of ccal_build_normal."""
    sigma: float
    param_names: list
    param_std: object
    param_corr: object
    pose_std: Dict[int, np.ndarray]
    pose_cov: Dict[int, np.ndarray]
    leverage: object
    report: object
    cov_cam: np.ndarray
    extr_std: Optional[np.ndarray] = None


def _corr(cov: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(standard deviations, correlation matrix) of a covariance; rows and columns of zero variance are 0."""
    std = np.sqrt(np.maximum(np.diag(cov), 0.0))
    inv = np.divide(1.0, std, out=np.zeros_like(std), where=std > 0)
    return std, cov * inv[:, None] * inv[None, :]


def _camera_block(model: GenericModel, cov_cam: np.ndarray, col: int, xy_same_focal: bool):
    """(names, std, corr) of one camera's params() vector out of the reduced system's covariance, whose block starts at column
    `col`; under one focal fy repeats fx's column."""
    names = list(_MODEL_KEYS[model.kind])
    idx = [col + (0 if i == 0 else i - 1) for i in range(len(names))] if xy_same_focal else [col + i for i in range(len(names))]
    std, corr = _corr(cov_cam[np.ix_(idx, idx)])
    return names, std, corr


def _uncertainty(prob, cams, slots, use, frames, xy_same_focal, intr, poses, extr) -> Uncertainty:
    res = prob.covariance(intr, poses, extr)
    rep = res.report
    col, blocks, extr_std = 0, [], np.zeros((len(cams), 6))
    for c, m in enumerate(cams):
        blocks.append(_camera_block(m, res.cov_cam, col, xy_same_focal))
        col += len(m._params) - (1 if xy_same_focal else 0)
        if c > 0:
            extr_std[c] = np.sqrt(np.maximum(np.diag(res.cov_cam)[col:col + 6], 0.0))
            col += 6
    posed = [s for s in range(len(slots)) if res.slot_status[s] == 0]
    pose_cov = {slots[s]: res.cov_poses[s].copy() for s in posed}
    pose_std = {fi: np.sqrt(np.maximum(np.diag(c), 0.0)) for fi, c in pose_cov.items()}
    lev = [dict() for _ in cams]
    at = 0
    for fi in slots:                                     # the corner order of _flatten: slot, camera, sorted feature ids
        for c, idxs in enumerate(use):
            if fi not in idxs:
                continue
            ids = sorted(frames[c][fi].features.keys())
            lev[c][fi] = {k: float(res.leverage[at + j]) for j, k in enumerate(ids)}
            at += len(ids)
    one = len(cams) == 1
    return Uncertainty(sigma=float(np.sqrt(rep.sigma2)), param_names=blocks[0][0] if one else [b[0] for b in blocks],
                       param_std=blocks[0][1] if one else [b[1] for b in blocks],
                       param_corr=blocks[0][2] if one else [b[2] for b in blocks], pose_std=pose_std, pose_cov=pose_cov,
                       leverage=lev[0] if one else lev, report=rep, cov_cam=res.cov_cam, extr_std=None if one else extr_std)


def calibration_uncertainty(frame_feature_list: Sequence[Optional[FrameFeature]], model: GenericModel,
                            rtvec_map: Dict[int, RvecTvec], xy_same_focal: bool = False, disabled_distortions: int = 0,
                            fixed_focal: bool = False, ctx: Optional[Context] = None) -> Uncertainty:
    """The uncertainty of a finished single-camera calibration (model, rtvec_map: what calib_camera returned, with the same
    xy_same_focal / disabled_distortions / fixed_focal): standard deviations and correlations of the camera parameters, the
    covariance of every frame's pose and the leverage of every detection, evaluated on the device at that point."""
    valid = [i for i in sorted(rtvec_map.keys()) if i < len(frame_feature_list) and frame_feature_list[i] is not None]
    if not valid:
        raise ValueError("calibration_uncertainty: no frame with both detections and a pose")
    slots, obs_cam, obs_slot, offs, X, U = _flatten([frame_feature_list], [valid])
    d, keep = make_desc(1, [model.model_id], [model.width()], [model.height()], xy_same_focal, len(slots), obs_cam, obs_slot, offs,
                        X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    with _Opened(ctx, None, d, keep) as prob:
        intr = _intr_matrix([model])
        prob.disable_distortions(disabled_distortions, intr)
        if fixed_focal:
            prob.fix_param(0, 0)
        poses = np.stack([rtvec_map[i].as6() for i in slots])
        return _uncertainty(prob, [model], slots, [valid], [frame_feature_list], xy_same_focal, intr, poses, None)


def rig_uncertainty(cameras: Sequence[GenericModel], t_cam_i_0: Sequence[RvecTvec], board_rtvecs: Dict[int, RvecTvec],
                    cams_detected_feature_frames: Sequence[Sequence[Optional[FrameFeature]]], xy_same_focal: bool = False,
                    disabled_distortions: int = 0, fixed_focal: bool = False, ctx: Optional[Context] = None) -> Uncertainty:
    """calibration_uncertainty for the joint problem of a rig (cameras, t_cam_i_0, board_rtvecs: what
    calib_all_camera_with_extrinsics returned - board_rtvecs the poses T_0_b): per-camera parameter blocks, the extrinsics'
    standard deviations, every board pose's covariance and per-camera leverages."""
    n_cams = len(cameras)
    cam_rtvecs = [{fi: rt for fi, rt in board_rtvecs.items() if fi < len(cams_detected_feature_frames[c])
                   and cams_detected_feature_frames[c][fi] is not None} for c in range(n_cams)]
    # (_joint_problem_inputs derives T_0_b from per-camera poses; here the board poses themselves are given and replace what it derives)
    built = _joint_problem_inputs(cameras, t_cam_i_0, cam_rtvecs, cams_detected_feature_frames, xy_same_focal)
    if built is None:
        raise ValueError("rig_uncertainty: no frame with both detections and a pose")
    d, keep, slots, intr, poses, extr = built
    poses = np.stack([board_rtvecs[fi].as6() for fi in slots])
    with _Opened(ctx, None, d, keep) as prob:
        prob.disable_distortions(disabled_distortions, intr)
        if fixed_focal:
            prob.fix_param(0, 0)
        use = [sorted(cam_rtvecs[c].keys()) for c in range(n_cams)]
        return _uncertainty(prob, list(cameras), slots, use, cams_detected_feature_frames, xy_same_focal, intr, poses, extr)


_REFINE_MIN_POINTS = 4


def _accepted(cand, poses, status) -> Dict[int, RvecTvec]:
    """{frame: pose} of the problems with a result: converged, or stopped at max_iterations (the reference keeps that result)."""
    return {fi: RvecTvec.from6(poses[k]) for k, fi in enumerate(cand) if status[k] in (_ffi.OK, _ffi.ERR_NO_CONVERGENCE)}


def refine_poses(frame_feature_list: Sequence[Optional[FrameFeature]], model: GenericModel,
                 rtvec_map: Optional[Dict[int, RvecTvec]] = None, huber_delta: float = 1.0,
                 ctx: Optional[Context] = None) -> Dict[int, RvecTvec]:
    """The board pose of every frame under the FIXED model `model`: the minimiser of the Huber cost of the pixel reprojection
    error (the ReprojectionFactor of the joint solve over rvec | tvec alone), one wavefront per frame, all frames in one launch
    (ccal_refine_poses_batch).  Starts from rtvec_map where one is given, otherwise from init_frame_poses.  Frames that are None,
    have fewer than 4 points, no starting pose or no result are absent from the returned map, as in calib_camera."""
    model._usable("refine_poses")
    cand = [i for i, f in enumerate(frame_feature_list) if f is not None and len(f.features) >= _REFINE_MIN_POINTS]
    if rtvec_map is not None:
        cand = [i for i in cand if i in rtvec_map]
    if not cand:
        return {}
    if rtvec_map is None:
        only = [f if i in set(cand) else None for i, f in enumerate(frame_feature_list)]
        rtvec_map = init_frame_poses(only, model, ctx=ctx)
        cand = [i for i in cand if i in rtvec_map]
        if not cand:
            return {}
    _, X, U = zip(*(_points_f32(frame_feature_list[i]) for i in cand))
    poses0 = np.stack([rtvec_map[i].as6() for i in cand])
    poses, status, _, _, _, _ = _ctx(ctx).refine_poses_batch(model.model_id, model._params, X, U, poses0, huber_delta,
                                                             _REFINE_MIN_POINTS)
    return _accepted(cand, poses, status)


def validation_holdout(cam_idx: int, model: GenericModel, frame_feature_list: Sequence[Optional[FrameFeature]],
                       ctx: Optional[Context] = None) -> Tuple[float, float]:
    """util::validation (src/util.rs:721-795) on frames the fit did not see: their poses are fitted with the model fixed
    (refine_poses), then the same statistics - (avg of the lowest 99 %, median) reprojection error in px."""
    return validation(cam_idx, model, refine_poses(frame_feature_list, model, ctx=ctx), frame_feature_list, ctx=ctx)


def refine_rig_poses(cams_detected_feature_frames: Sequence[Sequence[Optional[FrameFeature]]], cameras: Sequence[GenericModel],
                     t_cam_i_0: Sequence[RvecTvec], board_rtvecs: Optional[Dict[int, RvecTvec]] = None, huber_delta: float = 1.0,
                     ctx: Optional[Context] = None, opts: "Optional[_ffi.SolverOpts]" = None) -> Dict[int, RvecTvec]:
    """The board pose T_0_b of every frame index under the FIXED rig `cameras`, `t_cam_i_0`: the minimiser of the Huber cost of the
    pixel reprojection error over ALL cameras that saw the frame (the OtherCamReprojectionFactor of the joint solve over rvec_0_b |
    tvec_0_b alone), one wavefront per frame, all frames in one launch (ccal_refine_rig_poses_batch).  A frame seen by several
    cameras gets one pose.  Every entry of t_cam_i_0 is used as given (the reference's camera 0 is the identity).  Starts from
    board_rtvecs where given, otherwise by the rule of the joint solve (src/util.rs:576-651): T_c_0^-1 o T_c_b with the
    init_frame_poses result T_c_b of the first camera that has one (camera 0's own result where t_cam_i_0[0] is the identity).
    Frames without a start or without a result are absent from the returned map.  `opts`: the stop rules of the solve (None: the
    library's defaults)."""
    n_cams = len(cameras)
    if len(t_cam_i_0) != n_cams or len(cams_detected_feature_frames) != n_cams:
        raise ValueError("refine_rig_poses: one frame list and one T_c_0 per camera")
    for m in cameras:
        m._usable("refine_rig_poses")
    n_frames = max((len(f) for f in cams_detected_feature_frames), default=0)
    seen = [[c for c in range(n_cams) if fi < len(cams_detected_feature_frames[c]) and cams_detected_feature_frames[c][fi] is not None]
            for fi in range(n_frames)]
    if board_rtvecs is None:
        board_rtvecs = {}
        cam_rtvecs = [init_frame_poses(cams_detected_feature_frames[c], cameras[c], ctx=ctx) for c in range(n_cams)]
        for fi in range(n_frames):
            for c in range(n_cams):
                if fi in cam_rtvecs[c]:
                    board_rtvecs[fi] = t_cam_i_0[c].inverse().compose(cam_rtvecs[c][fi])
                    break
    cand = [fi for fi in range(n_frames) if seen[fi] and fi in board_rtvecs]
    if not cand:
        return {}
    slots = [[(c,) + _points_f32(cams_detected_feature_frames[c][fi])[1:] for c in seen[fi]] for fi in cand]
    poses0 = np.stack([board_rtvecs[fi].as6() for fi in cand])
    poses, status, _, _, _, _ = _ctx(ctx).refine_rig_poses_batch([m.model_id for m in cameras], [m._params for m in cameras],
                                                                 np.stack([t.as6() for t in t_cam_i_0]), slots, poses0, huber_delta,
                                                                 _REFINE_MIN_POINTS, opts)
    return _accepted(cand, poses, status)


def validation_holdout_rig(cameras: Sequence[GenericModel], t_cam_i_0: Sequence[RvecTvec],
                           cams_detected_feature_frames: Sequence[Sequence[Optional[FrameFeature]]],
                           ctx: Optional[Context] = None, opts: "Optional[_ffi.SolverOpts]" = None) -> List[Tuple[float, float]]:
    """The with-extrinsics branch of save_and_validate_results (src/bin/camera_calibration.rs:277-307) on frames the fit did not
    see: the board poses T_0_b are fitted with the whole rig fixed (refine_rig_poses), then per camera util::validation at
    T_i_0 o T_0_b - (avg of the lowest 99 %, median) reprojection error in px for every camera.  `opts` as in refine_rig_poses."""
    t_0_b = refine_rig_poses(cams_detected_feature_frames, cameras, t_cam_i_0, ctx=ctx, opts=opts)
    return [validation(c, cameras[c], {k: t_cam_i_0[c].compose(t) for k, t in t_0_b.items() if k < len(cams_detected_feature_frames[c])},
                       cams_detected_feature_frames[c], ctx=ctx) for c in range(len(cameras))]


# ----------------------------------------------------------------------------- from pixels to detections
def _corner_args(where: str, images, live: Sequence[int], half_win, max_iterations, eps, min_lambda) -> Optional[np.ndarray]:
    """The argument checks of refine_corners / redetect_corners that need no device, and the images of the frames `live`
    stacked [n][H][W] (None when there is none); images of other frames are not read."""
    if not 1 <= int(half_win) <= 15:
        raise ValueError(f"{where}: half_win 1 .. 15")
    if int(max_iterations) < 1:
        raise ValueError(f"{where}: max_iterations >= 1")
    if not (np.isfinite(eps) and float(eps) >= 0.0):
        raise ValueError(f"{where}: eps >= 0 and finite")
    if np.isnan(min_lambda):
        raise ValueError(f"{where}: min_lambda is NaN")
    if not live:
        return None
    imgs = [np.asarray(images[i]) for i in live]
    if any(im.ndim != 2 or im.shape != imgs[0].shape or im.dtype != imgs[0].dtype for im in imgs):
        raise ValueError(f"{where}: single-channel images [H][W] of one size and type")
    stack, _, _ = check_images(np.stack(imgs), True)
    return stack


def _kept_frames(n_frames: int, live, ids, p3ds, img_w_h, times, xy, status, lam, min_lambda) -> List[Optional[FrameFeature]]:
    out: List[Optional[FrameFeature]] = [None] * n_frames
    for k, fi in enumerate(live):
        keep = (status[k] == _ffi.OK) & (lam[k] >= min_lambda)
        feats = {ids[k][j]: FeaturePoint((float(np.float32(xy[k][j, 0])), float(np.float32(xy[k][j, 1]))), p3ds[k][j])
                 for j in np.flatnonzero(keep)}
        if feats:
            out[fi] = FrameFeature(times[k], img_w_h, feats)
    return out


def refine_corners(images, frame_feature_list: Sequence[Optional[FrameFeature]], half_win: int = 5, max_iterations: int = 30,
                   eps: float = 1e-3, min_lambda: float = 0.0, ctx: Optional[Context] = None) -> List[Optional[FrameFeature]]:
    """The sub-pixel step at the end of a target detector: every corner of every frame moved onto the grey-level saddle of its
    image (ccal_refine_corners_batch: one wavefront per corner, all frames in one launch).  images: one grey image [H][W] (uint8 or
    uint16, all of one size) per entry of frame_feature_list; the image of a frame that is None is not read.  Returns a new list:
    kept corners carry the refined p2d, stored as the f32 the reference's FeaturePoint holds; corners whose status is not CCAL_OK
    (no convergence, a flat patch or a single edge, a window that leaves the image or slides off its start by more than half_win)
    or whose lambda_min is below min_lambda are dropped; a frame left without a corner becomes None.
    min_lambda screens by corner strength (the smaller eigenvalue of the weighted gradient matrix).  It scales with the square of
    the image contrast; no useful value has been measured here, so the default 0 screens nothing."""
    if len(images) != len(frame_feature_list):
        raise ValueError("refine_corners: one image per frame")
    live = [i for i, f in enumerate(frame_feature_list) if f is not None and f.features]
    stack = _corner_args("refine_corners", images, live, half_win, max_iterations, eps, min_lambda)
    if stack is None:
        return [None] * len(frame_feature_list)
    ids, _, starts = zip(*(_points_f32(frame_feature_list[i]) for i in live))
    p3ds = [[frame_feature_list[i].features[k].p3d for k in ids_k] for i, ids_k in zip(live, ids)]
    xy, status, _, lam = _ctx(ctx).refine_corners_batch(stack, starts, half_win, max_iterations, eps)
    return _kept_frames(len(frame_feature_list), live, ids, p3ds, (stack.shape[2], stack.shape[1]),
                        [frame_feature_list[i].time_ns for i in live], xy, status, lam, min_lambda)


def redetect_corners(images, model: GenericModel, rtvec_map: Dict[int, RvecTvec], board_points: Dict[int, Tuple[float, float, float]],
                     half_win: int = 5, max_iterations: int = 30, eps: float = 1e-3, min_lambda: float = 0.0,
                     ctx: Optional[Context] = None) -> List[Optional[FrameFeature]]:
    """Guided re-detection after a first calibration: for every frame in rtvec_map (frame index -> board pose) every board point
    (board_points: id -> p3d) is taken into the camera frame, projected through `model`, and - where the projection is valid and its
    window lies in the image - refined onto the grey-level saddle of that frame's image (refine_corners' rule and parameters).
    Returns one entry per image: a FrameFeature (time_ns 0) of the corners that end CCAL_OK with lambda_min >= min_lambda, None for
    a frame without a pose or without such a corner.  This finds corners the detector missed, at the image edge above all.
    min_lambda: as in refine_corners - no useful value has been measured, 0 screens nothing."""
    model._usable("redetect_corners")
    if any(not 0 <= int(fi) < len(images) for fi in rtvec_map):
        raise ValueError("redetect_corners: a pose for a frame that has no image")
    live = sorted(int(fi) for fi in rtvec_map) if board_points else []
    stack = _corner_args("redetect_corners", images, live, half_win, max_iterations, eps, min_lambda)
    if stack is None:
        return [None] * len(images)
    H, W = stack.shape[1:]
    all_ids = sorted(board_points.keys())
    X = np.asarray([board_points[k] for k in all_ids], dtype=np.float32).astype(np.float64).reshape(-1, 3)
    cam = []
    for fi in live:
        R, t = rtvec_map[fi].matrix()
        cam.append(X @ R.T + t)
    uv, valid = model.project(np.concatenate(cam), ctx=ctx)
    m = int(half_win) + 1
    with np.errstate(invalid="ignore"):
        valid = valid & (uv[:, 0] >= m) & (uv[:, 0] <= W - 1 - m) & (uv[:, 1] >= m) & (uv[:, 1] <= H - 1 - m)
    uv, valid = uv.reshape(len(live), -1, 2), valid.reshape(len(live), -1)
    ids = [[all_ids[j] for j in np.flatnonzero(v)] for v in valid]
    p3ds = [[tuple(board_points[k]) for k in ids_k] for ids_k in ids]
    xy, status, _, lam = _ctx(ctx).refine_corners_batch(stack, [u[v] for u, v in zip(uv, valid)], half_win, max_iterations, eps)
    return _kept_frames(len(images), live, ids, p3ds, (W, H), [0] * len(live), xy, status, lam, min_lambda)


def _edge_directions(hess: np.ndarray) -> np.ndarray:
    """Per candidate the two unit zero-curvature directions of its Hessian [[hxx, hxy / 4], [hxy / 4, hyy]] - the two edges that
    cross at a checkerboard corner: [k, 2, 2].  (hxy of the detector is four times the mixed derivative.)"""
    h = np.asarray(hess, dtype=np.float64).reshape(-1, 3)
    M = np.empty((len(h), 2, 2))
    M[:, 0, 0], M[:, 1, 1], M[:, 0, 1], M[:, 1, 0] = h[:, 0], h[:, 1], h[:, 2] / 4.0, h[:, 2] / 4.0
    lam, vec = np.linalg.eigh(M)                                    # lam[:, 0] <= lam[:, 1]
    a, b = np.sqrt(np.maximum(lam[:, 1], 0.0))[:, None], np.sqrt(np.maximum(-lam[:, 0], 0.0))[:, None]
    d = np.stack([b * vec[:, :, 1] + a * vec[:, :, 0], b * vec[:, :, 1] - a * vec[:, :, 0]], axis=1)
    return d / np.maximum(np.linalg.norm(d, axis=2, keepdims=True), 1e-300)


_CONE_COS = 0.9            # a neighbour lies within about 25 degrees of an edge direction, seen from both ends
_WEAK = 0.5                # candidates below this fraction of the (cols * rows)-th strongest response are set aside


def assemble_checkerboard(xy, hess, pattern: Tuple[int, int], square_size: float) -> Optional[Dict[int, Tuple[float, float]]]:
    """Corner candidates of ONE image ordered into a complete checkerboard: xy [k, 2] (refined positions, f64) and hess [k, 3] =
    (hxx, hyy, hxy) as the detector returns them; pattern = (cols, rows) inner corners.  Returns {id: (x, y)} with
    id = r * cols + c for all cols * rows corners - the board point of id is (c * square_size, r * square_size, 0) - or None.

    Method: candidates whose response hxy^2 - 16 hxx hyy is below half of the (cols * rows)-th strongest are set aside (the
    L-corners of the outer squares: on the rendered boards of tests/detect_ref.py they respond at 0.18 .. 0.28 of the strongest
    candidate, the inner corners at 0.64 .. 1).  Each corner's two edge directions are the zero-curvature directions of its
    Hessian; along each of the four its neighbour is the nearest corner that lies in a cone around that direction, sees this
    corner in one of its own cones and has the opposite saddle polarity (the Hessians' inner product is negative: black and white
    swap from one corner to the next).  Every corner, the strongest first, seeds a lattice with a neighbour along each of its two
    edges; the lattice grows cell by cell: a free cell is predicted from the cells around it (2 p1 - p2 along a row or column,
    p1 + p2 - p3 across a square) and takes the nearest unused corner of the right polarity within 0.3 of the local spacing.  Then
    every cell is predicted once more from the finished lattice and takes the corner nearest to that - which puts a true corner
    back where a stray next to it had been picked.  The first lattice in which exactly one cols x rows (or rows x cols) window is
    completely filled is the board; cells outside the window are left out.  A partial board therefore returns None: without tags
    its offset in the pattern cannot be known.

    Stray candidates.  Weak ones are set aside by strength.  Strong ones (tests: six per frame, anywhere in the image, with a true
    corner's Hessian at 0.64 to 1.5 of its strength, over a range of seeds) do not change the result as long as each is farther
    than 5 px in x or y from every other candidate - what the detector guarantees at its default nms_radius.  A stray closer to
    a true corner than that can be taken in its place.  When no board is found every corner has been tried as a seed: about half
    a second for 60 candidates.

    Labelling: right-handed in the image (c towards r turns like +x towards +y).  That leaves two rotations of the board, four
    when cols == rows; the one whose id 0 is smallest in (y, x) is chosen.  The choice is a valid pose of a symmetric point set, so
    intrinsics are unaffected - but two cameras of a rig may choose differently for the same board, and a board that turns through
    the symmetry between frames changes its labelling with it."""
    cols, rows = int(pattern[0]), int(pattern[1])
    if cols < 2 or rows < 2 or not float(square_size) > 0.0:
        raise ValueError("assemble_checkerboard: pattern (cols, rows) >= 2 each, square_size > 0")
    P = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    Hs = np.asarray(hess, dtype=np.float64).reshape(-1, 3)
    if len(P) != len(Hs):
        raise ValueError("assemble_checkerboard: one Hessian per position")
    n_want = cols * rows
    resp = Hs[:, 2] ** 2 - 16.0 * Hs[:, 0] * Hs[:, 1]
    ok = np.isfinite(P).all(axis=1) & (resp > 0.0)
    if np.count_nonzero(ok) < n_want:
        return None
    ok &= resp >= _WEAK * np.sort(resp[ok])[-n_want]
    keep = np.flatnonzero(ok)
    keep = keep[np.lexsort((P[keep, 0], P[keep, 1]))]               # a fixed order, whatever the caller's
    P, Hs, resp = P[keep], Hs[keep], resp[keep]
    n = len(P)
    d2 = _edge_directions(Hs)
    dirs = np.concatenate([d2, -d2], axis=1)                        # [n, 4, 2]: d1, d2, -d1, -d2
    diff = P[None, :, :] - P[:, None, :]                            # diff[a, b] = b - a
    dist = np.linalg.norm(diff, axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = diff / dist[:, :, None]
    cosd = np.einsum("akc,abc->akb", dirs, np.nan_to_num(unit))     # [a, k, b]: b seen from a against a's direction k
    in_cone = cosd > _CONE_COS
    seen_back = in_cone.any(axis=1).T                               # [a, b]: a lies in one of b's cones
    M = np.stack([Hs[:, 0], Hs[:, 1], Hs[:, 2] / 4.0], axis=1)
    opposite = (M[:, 0:1] * M[None, :, 0] + M[:, 1:2] * M[None, :, 1] + 2.0 * M[:, 2:3] * M[None, :, 2]) < 0.0
    cand = in_cone & (seen_back & opposite & (dist > 0.0))[:, None, :]
    link = np.where(cand, dist[:, None, :], np.inf).argmin(axis=2)  # [a, k]
    link = np.where(cand.any(axis=2), link, -1)
    seen = np.zeros(n, dtype=bool)
    for start in np.argsort(-resp, kind="stable"):                  # seeds in the order of their strength
        if seen[start]:
            continue
        for kb, kc in ((0, 1), (0, 3), (2, 1), (2, 3)):             # a neighbour along each of the seed's two edges
            b, c = int(link[start, kb]), int(link[start, kc])
            if b < 0 or c < 0 or b == c:
                continue
            cell = _grow_lattice(P, opposite, int(start), b, c, cols + rows)
            G = _full_window(cell, cols, rows)
            if G is None:
                continue
            e_c, e_r = P[G[0, 1]] - P[G[0, 0]], P[G[1, 0]] - P[G[0, 0]]
            if e_c[0] * e_r[1] - e_c[1] * e_r[0] < 0.0:             # left-handed: mirror c
                G = G[:, ::-1]
            best = None
            for q in range(4):                                      # rotations keep the handedness
                A = np.rot90(G, q)
                if A.shape != (rows, cols):
                    continue
                key = (P[A[0, 0], 1], P[A[0, 0], 0])
                if best is None or key < best[0]:
                    best = (key, A)
            A = best[1]
            return {r * cols + c: (float(P[A[r, c], 0]), float(P[A[r, c], 1])) for r in range(rows) for c in range(cols)}
        seen[start] = True
    return None


_REACH = 0.3               # a corner is taken for a lattice cell within this fraction of the local spacing of the cell's prediction
_STEPS = ((1, 0), (0, 1), (-1, 0), (0, -1))


def _predict_cell(cell: Dict[Tuple[int, int], int], P: np.ndarray, i: int, j: int):
    """Where cell (i, j) should lie, from the other cells: 2 p1 - p2 along a row or column, p1 + p2 - p3 across a square, the mean
    of all that apply, and the smallest spacing among them; None when no stencil applies."""
    preds, spans = [], []
    for di, dj in _STEPS:
        p1, p2 = cell.get((i - di, j - dj)), cell.get((i - 2 * di, j - 2 * dj))
        if p1 is not None and p2 is not None:
            preds.append(2.0 * P[p1] - P[p2]); spans.append(np.linalg.norm(P[p1] - P[p2]))
    for di in (1, -1):
        for dj in (1, -1):
            p1, p2, p3 = cell.get((i - di, j)), cell.get((i, j - dj)), cell.get((i - di, j - dj))
            if p1 is not None and p2 is not None and p3 is not None:
                preds.append(P[p1] + P[p2] - P[p3]); spans.append(min(np.linalg.norm(P[p1] - P[p3]), np.linalg.norm(P[p2] - P[p3])))
    return (np.mean(preds, axis=0), min(spans)) if preds else None


def _best_for_cell(cell, P, opposite, free, i, j) -> int:
    """The corner for cell (i, j): the nearest to the cell's prediction among `free` within _REACH of the local spacing whose
    polarity is opposite to that of every neighbouring cell; -1: none."""
    pred = _predict_cell(cell, P, i, j)
    if pred is None:
        return -1
    d = np.linalg.norm(P - pred[0], axis=1)
    ok = (d <= _REACH * pred[1]) & free
    for di, dj in _STEPS:
        nb = cell.get((i + di, j + dj))
        if nb is not None:
            ok &= opposite[nb]
    return int(np.argmin(np.where(ok, d, np.inf))) if ok.any() else -1


def _grow_lattice(P: np.ndarray, opposite: np.ndarray, a: int, b: int, c: int, limit: int) -> Dict[Tuple[int, int], int]:
    """The lattice grown from corner a at cell (0, 0) with b at (1, 0) and c at (0, 1): {cell: corner}.  A free cell next to the
    lattice takes _best_for_cell among the unused corners; repeated until nothing is added, |i|, |j| <= limit.  Then every cell is
    settled: predicted from the finished lattice around it, it takes the best corner among the unused ones and its own - which puts
    the true corner back where the seed's nearest neighbour, or an early prediction, had picked a stray next to it."""
    cell = {(0, 0): a, (1, 0): b, (0, 1): c}
    used = np.zeros(len(P), dtype=bool)
    used[[a, b, c]] = True
    grown = True
    while grown:
        grown = False
        for i, j in sorted({(i + di, j + dj) for i, j in cell for di, dj in _STEPS} - set(cell)):
            if abs(i) > limit or abs(j) > limit:
                continue
            q = _best_for_cell(cell, P, opposite, ~used, i, j)
            if q >= 0:
                cell[(i, j)] = q
                used[q] = True
                grown = True
    for _ in range(3):
        moved = False
        for i, j in sorted(cell):
            own = cell.pop((i, j))
            used[own] = False
            q = _best_for_cell(cell, P, opposite, ~used, i, j)
            q = own if q < 0 else q
            cell[(i, j)] = q
            used[q] = True
            moved |= q != own
        if not moved:
            break
    return cell


def _full_window(cell: Dict[Tuple[int, int], int], cols: int, rows: int) -> Optional[np.ndarray]:
    """The one cols x rows (or rows x cols) window of a grown lattice in which every cell holds a corner, as an array [j][i] of
    corner indices; None when there is none or more than one."""
    ij = np.array(sorted(cell)); idx = np.array([cell[tuple(c)] for c in ij])
    ij -= ij.min(axis=0)
    ni, nj = ij.max(axis=0) + 1
    G = np.full((nj, ni), -1)
    G[ij[:, 1], ij[:, 0]] = idx
    found = []
    for w, h in sorted({(cols, rows), (rows, cols)}):
        for j0 in range(nj - h + 1):
            for i0 in range(ni - w + 1):
                if (G[j0:j0 + h, i0:i0 + w] >= 0).all():
                    found.append(G[j0:j0 + h, i0:i0 + w])
    return found[0] if len(found) == 1 else None


def detect_checkerboard_points(images, pattern: Tuple[int, int], square_size: float, step: int = 1, nms_radius: int = 5,
                               rel_threshold: float = 0.1, half_win: int = 5, max_iterations: int = 30, eps: float = 1e-3,
                               min_response: int = 1, max_per_image: int = 4096, ctx: Optional[Context] = None,
                               fused: bool = False) -> List[Optional[Dict[int, Tuple[float, float]]]]:
    """detect_checkerboard without the FrameFeature wrapping: per image {id: (x, y)} in f64, or None.
    fused=True: detector, refinement and assembly as ONE device-resident call (ccal_detect_checkerboards_batch; pattern sides
    2 .. 20, max_per_image at most 4096); the assembly follows the rule stated in include/ccal.h, which is assemble_checkerboard's
    method with every operation spelled out.  An image that keeps more than 512 candidates after the strength screen is beyond the
    device rule's limit and goes through the staged chain alone, so the limit does not show here."""
    if len(images) == 0:
        return []
    imgs = [np.asarray(im) for im in images]
    if any(im.ndim != 2 or im.shape != imgs[0].shape or im.dtype != imgs[0].dtype for im in imgs):
        raise ValueError("detect_checkerboard: single-channel images [H][W] of one size and type")
    stack, _, _ = check_images(np.stack(imgs), True)
    cols, rows = int(pattern[0]), int(pattern[1])
    if fused and (not (_ffi.BOARD_MIN_SIDE <= cols <= _ffi.BOARD_MAX_SIDE and _ffi.BOARD_MIN_SIDE <= rows <= _ffi.BOARD_MAX_SIDE)
                  or not float(square_size) > 0.0):
        raise ValueError("detect_checkerboard: fused: pattern (cols, rows) in 2 .. 20 each, square_size > 0")
    if fused and not 1 <= int(max_per_image) <= _ffi.BOARD_MAX_ROWS:
        raise ValueError("detect_checkerboard: fused: max_per_image in 1 .. 4096")
    c = _ctx(ctx)
    if fused:
        got = c.detect_checkerboards_batch(stack, cols, rows, step, nms_radius, min_response, rel_threshold, max_per_image, half_win,
                                           max_iterations, eps)
        out = [{i: (float(x), float(y)) for i, (x, y) in enumerate(xy)} if found else None for found, xy, _, _ in got]
        for k, (_, _, flags, _) in enumerate(got):
            if flags & _ffi.BOARD_FLAG_KEPT_LIMIT:
                out[k] = detect_checkerboard_points([stack[k]], pattern, square_size, step, nms_radius, rel_threshold, half_win,
                                                    max_iterations, eps, min_response, max_per_image, c)[0]
        return out
    found = c.detect_corners_batch(stack, step, nms_radius, min_response, rel_threshold, max_per_image)
    xy, status, _, _ = c.refine_corners_batch(stack, [f[0].astype(np.float64) for f in found], half_win, max_iterations, eps)
    out: List[Optional[Dict[int, Tuple[float, float]]]] = []
    for k, f in enumerate(found):
        good = status[k] == _ffi.OK
        out.append(assemble_checkerboard(xy[k][good], f[1][good], pattern, square_size))
    return out


def detect_checkerboard(images, pattern: Tuple[int, int], square_size: float, step: int = 1, nms_radius: int = 5,
                        rel_threshold: float = 0.1, half_win: int = 5, max_iterations: int = 30, eps: float = 1e-3,
                        min_response: int = 1, max_per_image: int = 4096, ctx: Optional[Context] = None,
                        fused: bool = False) -> List[Optional[FrameFeature]]:
    """From images alone to detections of a plain checkerboard of pattern = (cols, rows) inner corners: the integer saddle detector
    over all images in one call (ccal_detect_corners_batch), the sub-pixel refinement of its candidates (refine_corners' rule;
    corners whose status is not CCAL_OK are dropped), then assemble_checkerboard per image.  images: grey [H][W] each, uint8 or
    uint16, of one size.  Returns one entry per image: a FrameFeature with time_ns = the image's index, all cols * rows corners
    (p2d stored as f32 like the reference's FeaturePoint, p3d = (c * square_size, r * square_size, 0) for id = r * cols + c), or
    None where no complete board was found - partial boards are not returned.  The labelling's symmetry: assemble_checkerboard.
    min_response scales with the square of the image contrast; as for refine_corners' min_lambda no useful value has been measured
    here, and the default 1 screens only flat and edge-only neighbourhoods (rel_threshold does the work).
    fused=True runs the same chain as ONE call that keeps every intermediate on the device (detect_checkerboard_points states its
    limits); the positions are the same refined corners, and the assembly's decisions are the host function's on every input of
    the tests (its closed forms can round differently from the host's eigen-solver in the last bit).  The default is the staged
    chain above."""
    cols = int(pattern[0])
    pts = detect_checkerboard_points(images, pattern, square_size, step, nms_radius, rel_threshold, half_win, max_iterations, eps,
                                     min_response, max_per_image, ctx, fused)
    out: List[Optional[FrameFeature]] = []
    for k, found in enumerate(pts):
        if found is None:
            out.append(None)
            continue
        H, W = np.asarray(images[k]).shape
        sq = float(square_size)
        out.append(FrameFeature(k, (W, H), {i: FeaturePoint((float(np.float32(x)), float(np.float32(y))),
                                                            ((i % cols) * sq, (i // cols) * sq, 0.0)) for i, (x, y) in found.items()}))
    return out


@dataclasses.dataclass(frozen=True)
class TagFamily:
    """A tag family as data: bits = d * d data cells per tag (d in 3 .. 8) and the table of codes, code m being the tag of id m.
    A code is the d x d bit image in row-major order from the top-left cell, the first cell in the highest bit (the rule at
    ccal_decode_tags_batch in include/ccal.h).  NO family table ships with this project: the caller supplies the table of the
    family the board was printed from (tag36h11 for the usual AprilGrid: bits = 36, 587 codes), taken from the library that
    printed it.  JSON form: {"name": ..., "bits": ..., "codes": [...]}."""
    name: str
    bits: int
    codes: Tuple[int, ...]

    def __post_init__(self):
        bits = int(self.bits)
        if bits not in (9, 16, 25, 36, 49, 64):
            raise ValueError("TagFamily: bits is the square of 3 .. 8")
        codes = tuple(int(c) for c in self.codes)
        if not codes or any(not 0 <= c < (1 << bits) for c in codes):
            raise ValueError("TagFamily: at least one code, each 0 <= code < 2^bits")
        object.__setattr__(self, "bits", bits)
        object.__setattr__(self, "codes", codes)

    @property
    def d(self) -> int:
        return int(round(self.bits ** 0.5))

    @staticmethod
    def from_json_obj(obj) -> "TagFamily":
        return TagFamily(str(obj["name"]), int(obj["bits"]), tuple(int(c) for c in obj["codes"]))

    def to_json_obj(self):
        return {"name": self.name, "bits": self.bits, "codes": list(self.codes)}


class AprilGridBoard:
    """board::Board::init_aprilgrid (src/board.rs:46-95) with BoardConfig's fields and defaults (src/board.rs:7-25): id_to_3d maps
    corner id = tag_id * 4 + i to the corner's board point, in the reference's f32 arithmetic and order of operations.  Tag
    (r, c) starts at x = c * size * (1 + spacing), y = -r * size * (1 + spacing); its corners i = 0 .. 3 are (x, y), (x + s, y),
    (x + s, y - s), (x, y - s); ids count from first_id * 4, row by row."""

    def __init__(self, tag_size_meter: float = 0.088, tag_spacing: float = 0.3, tag_rows: int = 6, tag_cols: int = 6, first_id: int = 0):
        self.tag_size_meter, self.tag_spacing = float(tag_size_meter), float(tag_spacing)
        self.tag_rows, self.tag_cols, self.first_id = int(tag_rows), int(tag_cols), int(first_id)
        if self.tag_rows < 0 or self.tag_cols < 0 or self.first_id < 0:
            raise ValueError("AprilGridBoard: tag_rows, tag_cols and first_id are not negative")
        f32 = np.float32
        size, pitch = f32(self.tag_size_meter), f32(1.0) + f32(self.tag_spacing)
        self.id_to_3d: Dict[int, Tuple[float, float, float]] = {}
        count_id = self.first_id * 4
        for r in range(self.tag_rows):
            for c in range(self.tag_cols):
                start_x = f32(c) * size * pitch
                start_y = -f32(r) * size * pitch
                for i, (x, y) in enumerate(((start_x, start_y), (start_x + size, start_y), (start_x + size, start_y - size),
                                            (start_x, start_y - size))):
                    self.id_to_3d[count_id + i] = (float(x), float(y), 0.0)
                count_id += 4

    @staticmethod
    def from_json_obj(obj) -> "AprilGridBoard":
        """From the reference's BoardConfig as serde writes it: tag_size_meter, tag_spacing, tag_rows, tag_cols, first_id."""
        return AprilGridBoard(obj["tag_size_meter"], obj["tag_spacing"], obj["tag_rows"], obj["tag_cols"], obj["first_id"])


def decode_tags(images, quads_list, family: TagFamily, border: int = 1, samples: int = 3, min_contrast: float = 20.0,
                max_border_errors: int = 0, max_hamming: int = 2, ctx: Optional[Context] = None
                ) -> List[List[Tuple[int, int, int, np.ndarray]]]:
    """Candidate quads decoded against a tag family (ccal_decode_tags_batch: one wavefront per quad, all images in one call).
    images: one grey image [H][W] per entry (uint8 or uint16, all of one size); quads_list: per image an array [n_i, 4, 2] of quads,
    each in order around the tag's outer border edge, starting anywhere.  Returns per image the list of (tag_id, rot, hamming,
    corners [4, 2]) of the quads that decode (CCAL_TAG_OK), ascending in tag_id; corners are in the tag's canonical order (top-left,
    top-right, bottom-right, bottom-left of the code image), whatever corner the quad started at.  When two quads of one image
    decode to the same id the one with the smaller (hamming, -margin) is kept.  Proposing the quads is not part of this call."""
    if len(images) != len(quads_list):
        raise ValueError("decode_tags: one array of quads per image")
    if not len(images):
        return []
    imgs = [np.asarray(im) for im in images]
    if any(im.ndim != 2 or im.shape != imgs[0].shape or im.dtype != imgs[0].dtype for im in imgs):
        raise ValueError("decode_tags: single-channel images [H][W] of one size and type")
    reason, tag_id, rot, ham, corners, _, margin = _ctx(ctx).decode_tags_batch(
        np.stack(imgs), [np.asarray(q, dtype=np.float64).reshape(-1, 4, 2) for q in quads_list], family.bits, family.codes, border,
        samples, min_contrast, max_border_errors, max_hamming)
    out = []
    for k in range(len(imgs)):
        best: Dict[int, int] = {}
        for j in np.flatnonzero(reason[k] == _ffi.TAG_OK):
            t = int(tag_id[k][j])
            if t not in best or (ham[k][j], -margin[k][j]) < (ham[k][best[t]], -margin[k][best[t]]):
                best[t] = int(j)
        out.append([(t, int(rot[k][j]), int(ham[k][j]), corners[k][j].copy()) for t, j in sorted(best.items())])
    return out


def frames_from_tags(decoded, board: AprilGridBoard, img_w_h: Tuple[int, int], times: Optional[Sequence[int]] = None,
                     min_corners: int = 24) -> List[Optional[FrameFeature]]:
    """image_to_option_feature_frame (src/data_loader.rs:36-70) over decode_tags' output: corner i of tag tag_id gets
    id = tag_id * 4 + i and the board's point of that id; ids the board does not hold are dropped; a frame with fewer than
    min_corners corners (the reference's MIN_CORNERS = 24) is None.  p2d is stored as the f32 the reference's FeaturePoint holds.
    times: time_ns per frame (default: the frame's index)."""
    if times is not None and len(times) != len(decoded):
        raise ValueError("frames_from_tags: one time per frame")
    out: List[Optional[FrameFeature]] = []
    for k, tags in enumerate(decoded):
        feats: Dict[int, FeaturePoint] = {}
        for tag in tags:
            tag_id, corners = int(tag[0]), np.asarray(tag[3], dtype=np.float64).reshape(4, 2)
            for i in range(4):
                p3d = board.id_to_3d.get(tag_id * 4 + i)
                if p3d is not None:
                    feats[tag_id * 4 + i] = FeaturePoint((float(np.float32(corners[i, 0])), float(np.float32(corners[i, 1]))), p3d)
        if len(feats) < int(min_corners):
            out.append(None)
        else:
            out.append(FrameFeature(int(times[k]) if times is not None else k, (int(img_w_h[0]), int(img_w_h[1])), feats))
    return out


def merge_points(xy, radius: float = 1.0) -> np.ndarray:
    """The points [n, 2] without near-duplicates: in the given order, a point within `radius` px in BOTH coordinates of a point
    kept before it is dropped.  Two detector candidates can refine onto one saddle, to the last bit or nearly; as separate points
    they would multiply every outline they belong to."""
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    kept = np.zeros((len(pts), 2))
    n = 0
    for p in pts:
        if not (np.abs(kept[:n] - p) <= radius).all(axis=1).any():
            kept[n] = p
            n += 1
    return kept[:n].copy()


def _same_images(where: str, images) -> np.ndarray:
    imgs = [np.asarray(im) for im in images]
    if any(im.ndim != 2 or im.shape != imgs[0].shape or im.dtype != imgs[0].dtype for im in imgs):
        raise ValueError(f"{where}: single-channel images [H][W] of one size and type")
    stack, _, _ = check_images(np.stack(imgs), True)
    return stack


def propose_quads(images, xy_list, family: Optional[TagFamily] = None, border: int = 1, min_side: float = 20.0,
                  max_side: Optional[float] = None, max_side_ratio: float = 2.0, offset: Optional[float] = None, samples: int = 8,
                  min_contrast: float = 40.0, max_per_image: int = 1024, ctx: Optional[Context] = None
                  ) -> List[Tuple[np.ndarray, int, int]]:
    """Candidate tag outlines of an AprilGrid from refined saddle points (ccal_propose_quads_batch: one wavefront per point, all
    images in one call; the rule is stated in include/ccal.h).  images: one grey image [H][W] per entry (uint8 or uint16, all of one
    size); xy_list: per image the refined corner candidates [n_i, 2], in any order - merge_points is applied to them first.
    offset None: half a cell of the family's tags, 1 / (2 (family.d + 2 border)); without a family 1/16 (36 bits, one border cell).
    max_side None: half the larger image side.  min_contrast is in grey levels of the images' type (scale it by 257 for uint16
    images that span the 16 bits).  Returns per image (quads [m, 4, 2] - clockwise in the image, ready for decode_tags -, count,
    flags): m = min(count, max_per_image); bit 0 of flags says a point had more than 8 out-edges and proposals may be missing."""
    if len(images) != len(xy_list):
        raise ValueError("propose_quads: one array of points per image")
    if not len(images):
        return []
    if offset is None:
        offset = 1.0 / (2.0 * (family.d + 2 * int(border))) if family is not None else 1.0 / 16.0
    stack = _same_images("propose_quads", images)
    got = _ctx(ctx).propose_quads_batch(stack, [merge_points(xy) for xy in xy_list], min_side, max_side, max_side_ratio, offset,
                                        samples, min_contrast, max_per_image)
    return [(quads, count, flags) for _, quads, count, flags in got]


def detect_tags(images, family: TagFamily, step: int = 1, nms_radius: int = 5, rel_threshold: float = 0.1, half_win: int = 4,
                min_side: float = 20.0, max_side: Optional[float] = None, min_contrast: float = 40.0, border: int = 1,
                max_hamming: int = 2, ctx: Optional[Context] = None) -> List[List[Tuple[int, int, int, np.ndarray]]]:
    """From images alone to the tags of `family` in each, in one device-resident call (ccal_detect_tags_batch: the image block is
    uploaded once, no candidate, point or quad comes back to the host).  The parameters are detect_aprilgrid's and mean the same.
    Returns what decode_tags returns for the quads of the staged chain, to the bit: per image the list of (tag_id, rot, hamming,
    corners [4, 2]), ascending in tag_id."""
    if not len(images):
        return []
    stack = _same_images("detect_tags", images)
    got = _ctx(ctx).detect_tags_batch(stack, family.bits, family.codes, step, nms_radius, 1, rel_threshold, half_win=half_win,
                                      min_side=min_side, max_side=max_side, edge_min_contrast=min_contrast, border=border,
                                      tag_min_contrast=min_contrast, max_hamming=max_hamming)
    return [[(int(t), int(r), int(h), c.copy()) for t, r, h, c in zip(ids, rot, ham, corners)] for ids, rot, ham, corners, *_ in got]


def detect_aprilgrid(images, family: TagFamily, board: AprilGridBoard, step: int = 1, nms_radius: int = 5, rel_threshold: float = 0.1,
                     half_win: int = 4, min_side: float = 20.0, max_side: Optional[float] = None, min_contrast: float = 40.0,
                     border: int = 1, max_hamming: int = 2, times: Optional[Sequence[int]] = None, min_corners: int = 24,
                     ctx: Optional[Context] = None, fused: bool = False) -> List[Optional[FrameFeature]]:
    """From images alone to detections of an AprilGrid: the integer saddle detector over all images (ccal_detect_corners_batch), the
    sub-pixel refinement of its candidates (ccal_refine_corners_batch; candidates whose status is not CCAL_OK are dropped, the rest
    rounded through the f32 a FeaturePoint holds), merge_points, the quad proposer (ccal_propose_quads_batch, offset from the
    family's bit count and `border`), the decoder (decode_tags) and frames_from_tags.  images: grey [H][W] each, uint8 or uint16, of
    one size.  family: the table the board was printed from - none ships with this project.  Returns one entry per image: a
    FrameFeature (corner id = tag_id * 4 + i, p3d from `board`, time_ns from `times` or the image's index) or None for an image with
    fewer than min_corners corners.
    half_win 4 suits tags whose cells are 5 to 6 px: the window around a tag's outer corner has to hold the border cell and the
    gap square and little of the data cells.  min_contrast goes to BOTH the proposer (bright - dark along an edge) and the decoder
    (hi - lo over a tag's cells) and is in grey levels of the images' type: for uint16 images the caller scales it (by 257 when
    they span the 16 bits); nothing here guesses the range from the pixels.
    fused=True runs the same chain as ONE call that keeps every intermediate on the device (detect_tags) and gives the same
    FrameFeatures; the default is the staged chain above."""
    if not len(images):
        return []
    stack = _same_images("detect_aprilgrid", images)
    H, W = stack.shape[1:]
    c = _ctx(ctx)
    if fused:
        decoded = detect_tags(list(stack), family, step, nms_radius, rel_threshold, half_win, min_side, max_side, min_contrast, border,
                              max_hamming, ctx=c)
        return frames_from_tags(decoded, board, (W, H), times, min_corners)
    found = c.detect_corners_batch(stack, step, nms_radius, 1, rel_threshold)
    xy, status, _, _ = c.refine_corners_batch(stack, [f[0].astype(np.float64) for f in found], half_win)
    points = [merge_points(np.float32(xy[k][status[k] == _ffi.OK]).astype(np.float64)) for k in range(len(stack))]
    offset = 1.0 / (2.0 * (family.d + 2 * int(border)))
    proposed = c.propose_quads_batch(stack, points, min_side, max_side, 2.0, offset, 8, min_contrast)
    decoded = decode_tags(list(stack), [p[1] for p in proposed], family, border, 3, min_contrast, 0, max_hamming, ctx=c)
    return frames_from_tags(decoded, board, (W, H), times, min_corners)


def _render_args(where: str, model: GenericModel, poses, dtype) -> Tuple[np.ndarray, np.dtype]:
    """The checks of the two renderers that need no device: (poses [n, 6], the images' dtype)."""
    model._usable(where)
    if np.dtype(dtype) not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise ValueError(f"{where}: dtype is uint8 or uint16")
    if len(poses) and all(isinstance(p, RvecTvec) for p in poses):
        poses = [p.as6() for p in poses]
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 2 or poses.shape[1] != 6:
        raise ValueError(f"{where}: poses is a sequence of RvecTvec or an [n, 6] array of rvec, tvec")
    w, h = int(model.width()), int(model.height())
    if w != model.width() or h != model.height() or w <= 0 or h <= 0:
        raise ValueError(f"{where}: the model's width and height are positive whole numbers of pixels")
    return np.ascontiguousarray(poses), np.dtype(dtype)


@dataclasses.dataclass
class PhotoOpts:
    """The photometric stage between ideal irradiance and pixels (ccal_photo_opts in include/ccal.h states the rule): a Gaussian lens
    blur of blur_sigma px (0 .. 16/3), vignetting with the gain 1 / (1 + vignette)^2 at the corners, the exposure `gain`, read noise
    of noise_read grey levels (8-bit scale) and shot noise of variance noise_shot per grey level; image k of a call draws from the
    stream seed + first_index + k.  The defaults switch everything off."""
    blur_sigma: float = 0.0
    vignette: float = 0.0
    gain: float = 1.0
    noise_read: float = 0.0
    noise_shot: float = 0.0
    seed: int = 0
    first_index: int = 0


@dataclasses.dataclass
class NormalizeOpts:
    """Local contrast normalisation ahead of the detectors (ccal_normalize_opts in include/ccal.h states the rule;
    Context.normalize_dev): every pixel minus the mean of the (2 radius + 1)^2 window around it (radius 1 .. 32) over the window's
    standard deviation, which is held above min_sigma grey levels (8-bit scale, 0 .. 255), times `amp` grey levels, around 128.
    For frames whose contrast falls towards the edge or that are under-exposed; on a clean frame it costs accuracy (README)."""
    radius: int = 16
    min_sigma: float = 4.0
    amp: float = 64.0


@dataclasses.dataclass
class GreyOpts:
    """The grey stage ahead of every image stage (ccal_grey_opts in include/ccal.h states the rule; Context.grey_dev): colour and raw
    Bayer frames to grey ones, `bin` x `bin` source pixels (1, 2 or 4) to an output pixel, with the channel weights w_r, w_g, w_b in
    units of 1 / 65536 (they sum to 65536; the defaults are 0.299 / 0.587 / 0.114).  Output pixel X has its centre at source
    coordinate bin X + (bin - 1) / 2."""
    bin: int = 1
    w_r: int = 19595
    w_g: int = 38470
    w_b: int = 7471


# ccal_pixel_layout by name: what a source pixel of Context.grey_dev is
LAYOUTS = {"grey": _ffi.LAYOUT_GREY, "rgb": _ffi.LAYOUT_RGB, "bgr": _ffi.LAYOUT_BGR, "rgba": _ffi.LAYOUT_RGBA, "bgra": _ffi.LAYOUT_BGRA,
           "bayer_rggb": _ffi.LAYOUT_BAYER_RGGB, "bayer_bggr": _ffi.LAYOUT_BAYER_BGGR, "bayer_grbg": _ffi.LAYOUT_BAYER_GRBG,
           "bayer_gbrg": _ffi.LAYOUT_BAYER_GBRG}


def render_checkerboard(model: GenericModel, poses, pattern: Tuple[int, int], square_size: float, dtype=np.uint8, supersample: int = 4,
                        black: float = 40, white: float = 215, background: float = 0, margin: Optional[float] = None,
                        ctx: Optional[Context] = None, photo: Optional[PhotoOpts] = None) -> np.ndarray:
    """Images [n, H, W] of a checkerboard of pattern = (cols, rows) inner corners and squares of square_size metres as `model` sees
    it at `poses` (board -> camera; a sequence of RvecTvec or an [n, 6] array), rendered on the GPU by the rule stated at
    ccal_render_targets_batch in include/ccal.h: every pixel the mean of supersample x supersample rays through the model, black
    and white squares at the given 8-bit grey levels (times 257 for uint16), `background` beyond the white sheet, which extends
    `margin` metres (default: one square; inf: a white plane) beyond the squares.  Inner corner (c, r) is the board point
    (c square_size, r square_size, 0), the labelling of detect_checkerboard.  H, W are the model's.  photo None: ideal images;
    a PhotoOpts: lens blur, vignetting, exposure and sensor noise on the device, in the same call."""
    poses, dt = _render_args("render_checkerboard", model, poses, dtype)
    target = checkerboard_target(int(pattern[0]), int(pattern[1]), square_size)
    return _ctx(ctx).render_targets_batch(model.model_id, model.params(), int(model.width()), int(model.height()), poses, target, dt,
                                          supersample, black, white, background, margin, photo=photo)


def render_aprilgrid(model: GenericModel, poses, board: AprilGridBoard, family: TagFamily, border: int = 1, dtype=np.uint8,
                     supersample: int = 4, black: float = 40, white: float = 215, background: float = 0,
                     margin: Optional[float] = None, ctx: Optional[Context] = None, photo: Optional[PhotoOpts] = None) -> np.ndarray:
    """Images [n, H, W] of the AprilGrid `board` printed from `family` (tag (r, c) shows the code of id first_id + r tag_cols + c,
    `border` black cells around its data cells, black squares in the gaps at the tag corners) as `model` sees it at `poses`,
    rendered on the GPU like render_checkerboard.  The geometry is board.id_to_3d's and the decoder's corner order; margin
    defaults to one tag pitch; photo as there."""
    poses, dt = _render_args("render_aprilgrid", model, poses, dtype)
    target = aprilgrid_target(board.tag_size_meter, board.tag_spacing, board.tag_rows, board.tag_cols, board.first_id, family.bits,
                              family.codes, border)
    return _ctx(ctx).render_targets_batch(model.model_id, model.params(), int(model.width()), int(model.height()), poses, target, dt,
                                          supersample, black, white, background, margin, photo=photo)


class ReprojectionFactor:
    """optimization::factors::ReprojectionFactor (src/optimization/factors.rs:126-173).
    residual_func(params) with params = [intrinsics (P_eff), rvec, tvec] evaluates the block on the GPU;
    `jacobian=True` also returns the 2 x D block Jacobian tiny-solver would obtain with dual numbers."""

    other = False

    def __init__(self, target: GenericModel, p3d, p2d, xy_same_focal: bool, ctx: Optional[Context] = None):
        self.target = target
        self.p3d = np.asarray(p3d, dtype=np.float32)          # glam::Vec3 (f32) widened later, factors.rs:141-143
        self.p2d = np.asarray(p2d, dtype=np.float32)
        self.xy_same_focal = bool(xy_same_focal)
        self._ctx = ctx

    @classmethod
    def new(cls, target, p3d, p2d, xy_same_focal, ctx=None):
        return cls(target, p3d, p2d, xy_same_focal, ctx)

    def residual_func(self, params: Sequence[np.ndarray], jacobian: bool = False):
        n_cams = 2 if self.other else 1
        m = self.target.model_id
        p0 = np.asarray(params[0], dtype=np.float64)
        full = np.insert(p0, 1, p0[0]) if self.xy_same_focal else p0          # factors.rs:155-158
        intr = np.zeros((n_cams, PMAX)); intr[:, :len(full)] = full
        pose = np.concatenate([np.asarray(params[1], float), np.asarray(params[2], float)])[None, :]
        extr = np.zeros((n_cams, 6))
        if self.other:
            extr[1] = np.concatenate([np.asarray(params[3], float), np.asarray(params[4], float)])
        d, keep = make_desc(n_cams, [m] * n_cams, [self.target.width()] * n_cams, [self.target.height()] * n_cams,
                            self.xy_same_focal, 1, [n_cams - 1], [0], [0, 1],
                            [self.p3d[0]], [self.p3d[1]], [self.p3d[2]], [self.p2d[0]], [self.p2d[1]], 1.0)
        prob = Problem(_ctx(self._ctx), d, keep)
        try:
            r, J = prob.eval(intr, pose, extr)
        finally:
            prob.close()
        return (r[0], J.reshape(2, -1)) if jacobian else r[0]


class OtherCamReprojectionFactor(ReprojectionFactor):
    """optimization::factors::OtherCamReprojectionFactor (factors.rs:179-228);
    params = [intrinsics, rvec_0_b, tvec_0_b, rvec_i_0, tvec_i_0]."""
    other = True


def frames_from_synth(sp, cam: int = 0) -> List[Optional[FrameFeature]]:
    """SynthProblem -> the reference's `Vec<Option<FrameFeature>>` for one camera (ids = row order)."""
    out: List[Optional[FrameFeature]] = [None] * sp.n_slots
    for o in range(sp.n_obs):
        if sp.obs_cam[o] != cam:
            continue
        a, b = int(sp.obs_offsets[o]), int(sp.obs_offsets[o + 1])
        feats = {k: FeaturePoint(tuple(sp.p2d[a + k]), tuple(sp.p3d[a + k])) for k in range(b - a)}
        out[int(sp.obs_slot[o])] = FrameFeature(0, (int(sp.width[cam]), int(sp.height[cam])), feats)
    return out


# ----------------------------------------------------------------------------- calibration from detections alone
@dataclasses.dataclass
class CalibParams:                       # src/types.rs:6-10
    fixed_focal: Optional[float] = None
    disabled_distortion_num: int = 0
    one_focal: bool = False

    def to_json_obj(self) -> dict:
        return {"fixed_focal": self.fixed_focal, "disabled_distortion_num": int(self.disabled_distortion_num),
                "one_focal": bool(self.one_focal)}

    @staticmethod
    def from_json_obj(d: dict) -> "CalibParams":
        ff = d.get("fixed_focal")
        return CalibParams(None if ff is None else float(ff), int(d.get("disabled_distortion_num", 0)), bool(d.get("one_focal", False)))


def find_best_two_frames_idx(detected_feature_frames: Sequence[Optional[FrameFeature]], random_pick: bool,
                             seed: Optional[int] = None) -> Tuple[int, int]:
    """util::find_best_two_frames_idx (src/util.rs:168-219).  Among the frames with the maximal corner count: the one whose
    detections cover the largest bounding box, and the one whose centroid lies farthest from the mean centroid (ties: the
    later frame, as a stable ascending sort's last element).  `random_pick`: two of them at random - reproducible under `seed`
    (the reference's generator is unseeded)."""
    best, idxs = 0, []
    for i, f in enumerate(detected_feature_frames):
        if f is None:
            continue
        n = len(f.features)
        if n > best:
            best, idxs = n, [i]
        elif n == best:
            idxs.append(i)
    if random_pick:
        pick = np.random.default_rng(seed).permutation(len(idxs))
        return idxs[int(pick[0])], idxs[int(pick[1])]                  # IndexError with one candidate: the reference panics
    pts = {i: np.array([fp.p2d for fp in detected_feature_frames[i].features.values()], dtype=np.float32) for i in idxs}
    centre = {i: pts[i].mean(axis=0) for i in idxs}
    mean_centre = np.mean([centre[i] for i in idxs], axis=0)
    by_distance = sorted(idxs, key=lambda i: float(((centre[i] - mean_centre) ** 2).sum()))
    by_area = sorted(idxs, key=lambda i: float(np.prod(pts[i].max(axis=0) - pts[i].min(axis=0))))
    return by_area[-1], by_distance[-1]


def rdh_sample_indices(seed: int, n_pairs: int, n_hyp: int) -> np.ndarray:
    """Host twin of the RANSAC kernel's sampler: [n_hyp, 6] distinct pair indices - hypothesis h runs a partial Fisher-Yates
    shuffle of 0 .. n_pairs-1 on splitmix64(seed, 6, stream=h): draw k swaps position k with k + z_k mod (n_pairs - k)."""
    if n_pairs < 6:
        raise ValueError("six distinct indices need at least six pairs")
    out = np.empty((n_hyp, 6), dtype=np.int32)
    for h in range(n_hyp):
        z = splitmix64(int(seed), 6, stream=h)
        a = np.arange(n_pairs)
        for k in range(6):
            j = k + int(z[k] % np.uint64(n_pairs - k))
            a[k], a[j] = a[j], a[k]
        out[h] = a[:6]
    return out


def _normalised_pairs(frame_feature0: FrameFeature, frame_feature1: FrameFeature) -> np.ndarray:
    """Corners whose ids both frames hold (ids ascending), (p - (w/2, h/2)) / max(w/2, h/2) with the FIRST frame's size
    (src/optimization/homography.rs:223-238)."""
    w, h = frame_feature0.img_w_h
    c = np.array([w / 2.0, h / 2.0]); half = max(w / 2.0, h / 2.0)
    ids = sorted(set(frame_feature0.features) & set(frame_feature1.features))
    p0 = np.array([frame_feature0.features[i].p2d for i in ids], dtype=np.float64).reshape(-1, 2)
    p1 = np.array([frame_feature1.features[i].p2d for i in ids], dtype=np.float64).reshape(-1, 2)
    return np.concatenate([(p0 - c) / half, (p1 - c) / half], axis=1)


def radial_distortion_homography(frame_feature0: FrameFeature, frame_feature1: FrameFeature, seed: int = 0, n_hyp: int = 1000,
                                 ctx: Optional[Context] = None) -> Tuple[float, np.ndarray]:
    """optimization::homography::radial_distortion_homography (homography.rs:218-271) on the GPU: (lambda, H [3, 3]).
    Without one valid hypothesis the reference returns its initial (0, zeros): so does this."""
    r = _ctx(ctx).rdh_batch([_normalised_pairs(frame_feature0, frame_feature1)], [seed], n_hyp)
    return float(r["lambda"][0]), r["H"][0].copy()


def homography_to_focal(h_mat) -> Optional[float]:
    """optimization::homography::homography_to_focal (homography.rs:274-325); None where the reference returns None."""
    H = np.ascontiguousarray(h_mat, dtype=np.float64).reshape(9)
    f = C.c_double()
    rc = _ffi.load().ccal_homography_to_focal(H.ctypes.data_as(C.POINTER(C.c_double)), C.byref(f))
    if rc == _ffi.NO_RESULT:
        return None
    if rc != _ffi.OK:
        raise CcalError(rc, "ccal_homography_to_focal")
    return float(f.value)


def solve_pnp(p3ds, p2ds_z, ctx: Optional[Context] = None
              ) -> Optional[Tuple[Tuple[float, float, float], Tuple[float, float, float]]]:
    """sqpnp_simple::sqpnp_solve_glam(&p3ds, &p2ds_z) as the reference calls it (src/util.rs:431, examples/test_pnp.rs:61): 3-D points
    [n, 3] - any point set - and their normalised image points [n, 2] -> (rvec, tvec), None without a pose."""
    poses, used, _ = _ctx(ctx).pnp_batch([p3ds], [p2ds_z], 4, with_cost=False)
    if used[0] == 0:
        return None
    return tuple(float(v) for v in poses[0, :3]), tuple(float(v) for v in poses[0, 3:])


def init_pose(frame_feature: FrameFeature, lam: float, ctx: Optional[Context] = None
              ) -> Tuple[Tuple[float, float, float], Tuple[float, float, float]]:
    """optimization::linear::init_pose (linear.rs:5-21): division-model undistortion, planar PnP -> (rvec, tvec)."""
    slots, obs_cam, obs_slot, offs, X, U = _flatten([[frame_feature]], [[0]])
    w, h = frame_feature.img_w_h
    d, keep = make_desc(1, [MODEL_NAMES["ucm"]], [w], [h], False, 1, obs_cam, obs_slot, offs, X[:, 0], X[:, 1], X[:, 2], U[:, 0], U[:, 1], 1.0)
    prob = Problem(_ctx(ctx), d, keep)
    try:
        poses, used = prob.init_poses_division(lam, 4)
    finally:
        prob.close()
    if used[0] == 0:
        raise RuntimeError("init_pose: no pose from these detections")            # sqpnp_solve_glam(..).unwrap()
    return tuple(float(v) for v in poses[0, :3]), tuple(float(v) for v in poses[0, 3:])
