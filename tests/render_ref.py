"""The yardstick of the target renderer: a numpy f64 statement of the rule that include/ccal.h states at ccal_render_targets_batch,
written from that text (whole-array arithmetic over all sub-pixel rays of an image: no lanes, no tiles, no packed words), for the
four models; the cases the GPU parity tests run, shared with the CPU test that holds every one of them to the near cap; and the
round-trip poses with the corner errors the numpy detector chains reach on them.

Rays: closed forms for UCM and EUCM (Usenko et al. 2018); for KB4 and OPENCV5 undistort_ref.unproject_newton on oracle.project.
That Newton iteration parametrises a ray as (a, b, 1), so it serves rays in front of the camera; KB4 pixels whose image-plane radius
is 1.2 or more (polar angles from about 69 degrees on - the rim of the 512 x 512 fisheye, nothing in the small parity cases) take
a one-dimensional Newton iteration on the polar angle instead, and every such ray is held to oracle.project within 1e-9 px.

A sub-pixel ray is NEAR when its class at one of (u +- 1e-8, v +- 1e-8) differs from its class at (u, v); a pixel is near when one
of its rays is.  1e-8 px is ten times the 1e-9 px round-trip bound the suite holds `unproject` to (tests/test_gpu_undistort.py):
two correct inverses cannot disagree on a ray's class outside that band.  numpy rounds every product and sum on its own, and so does
the library's render unit.  It depends on no GPU and on nothing outside this repository."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref  # noqa: E402
import tag_ref  # noqa: E402
import undistort_ref  # noqa: E402

UCM, EUCM, KB4, OPENCV5 = 0, 1, 2, 3
B, W, G = 0, 1, 2
NEAR_PX = 1e-8
NEAR_CAP = 1e-3             # near pixels may make up at most 0.1 % of a case
KB4_WIDE = 1.2              # image-plane radius from which a KB4 pixel takes the polar-angle iteration


# ---- poses ------------------------------------------------------------------------------------------------------------------------
def pose_rt(pose):
    """(R [3, 3], tb = R^T t) of rvec, tvec as the header states them: Rodrigues' formula, then the three sums written out."""
    rx, ry, rz, tx, ty, tz = [float(x) for x in pose]
    a = math.sqrt(rx * rx + ry * ry + rz * rz)
    R = np.eye(3)
    if not a < 1e-12:
        K = np.array([[0.0, -rz / a, ry / a], [rz / a, 0.0, -rx / a], [-ry / a, rx / a, 0.0]])
        s, c1 = math.sin(a), 1.0 - math.cos(a)
        for i in range(3):
            for j in range(3):
                kk = K[i, 0] * K[0, j] + K[i, 1] * K[1, j] + K[i, 2] * K[2, j]
                R[i, j] = (1.0 if i == j else 0.0) + s * K[i, j] + c1 * kk
    tb = np.array([R[0, j] * tx + R[1, j] * ty + R[2, j] * tz for j in range(3)])
    return R, tb


def pose6(R, t):
    """rvec, tvec of a rotation matrix and a translation (the angle in [0, pi], through the quaternion with w >= 0)."""
    from camera_intrinsic_calibration_rs_amd.synth import rotmat_to_rvec
    return np.concatenate([rotmat_to_rvec(np.asarray(R, dtype=np.float64)), np.asarray(t, dtype=np.float64)])


# ---- targets ----------------------------------------------------------------------------------------------------------------------
def board_target(cols, rows, square, margin=None):
    return {"kind": "board", "cols": int(cols), "rows": int(rows), "square": float(square),
            "margin": float(square if margin is None else margin)}


def grid_target(board, family, border=1, margin=None):
    """board: anything with tag_ref.Board's fields; family: anything with .bits and .codes."""
    pitch = board.tag_size_meter * (1.0 + board.tag_spacing)
    return {"kind": "grid", "board": board, "bits": int(family.bits), "codes": tuple(int(c) for c in family.codes), "border": int(border),
            "margin": float(pitch if margin is None else margin)}


def classify(target, X, Y):
    """Step 5: the class of the plane points (X, Y), arrays of one shape."""
    m = target["margin"]
    with np.errstate(invalid="ignore", divide="ignore"):
        if target["kind"] == "board":
            cols, rows, sq = target["cols"], target["rows"], target["square"]
            sheet = (X >= -sq - m) & (X <= cols * sq + m) & (Y >= -sq - m) & (Y <= rows * sq + m)
            i, j = np.floor(X / sq) + 1.0, np.floor(Y / sq) + 1.0
            on = (i >= 0) & (i <= cols) & (j >= 0) & (j <= rows)
            dark = on & (np.mod(i + j, 2.0) == 0.0)
            return np.where(sheet, np.where(dark, B, W), G)
        bd, border = target["board"], target["border"]
        d = int(round(target["bits"] ** 0.5))
        n = d + 2 * border
        size, pitch = bd.tag_size_meter, bd.tag_size_meter * (1.0 + bd.tag_spacing)
        gap_w = bd.tag_spacing * bd.tag_size_meter
        Yd = -Y
        sheet = (X >= -gap_w - m) & (X <= bd.tag_cols * pitch + m) & (Yd >= -gap_w - m) & (Yd <= bd.tag_rows * pitch + m)
        cells = np.zeros((bd.tag_rows, bd.tag_cols, n, n), dtype=bool)
        for r in range(bd.tag_rows):
            for c in range(bd.tag_cols):
                cells[r, c, border:border + d, border:border + d] = tag_ref.code_to_bits(target["codes"][bd.first_id + r * bd.tag_cols + c], d) == 1
        c, r = np.floor(X / pitch), np.floor(Yd / pitch)
        u, v = (X - c * pitch) / size, (Yd - r * pitch) / size
        tag = (c >= 0) & (c < bd.tag_cols) & (r >= 0) & (r < bd.tag_rows) & (u < 1.0) & (v < 1.0)
        gap = (u >= 1.0) & (v >= 1.0) & (c >= -1) & (c < bd.tag_cols) & (r >= -1) & (r < bd.tag_rows)
        ok = np.isfinite(X) & np.isfinite(Yd)
        ci = np.clip(np.where(ok, c, 0.0), 0, bd.tag_cols - 1).astype(np.int64)
        ri = np.clip(np.where(ok, r, 0.0), 0, bd.tag_rows - 1).astype(np.int64)
        cu = np.clip(np.floor(np.where(tag, u, 0.0) * n), 0, n - 1).astype(np.int64)
        cv = np.clip(np.floor(np.where(tag, v, 0.0) * n), 0, n - 1).astype(np.int64)
        white = np.where(tag, cells[ri, ci, cv, cu], ~gap)
        return np.where(sheet, np.where(white, W, B), G)


# ---- rays -------------------------------------------------------------------------------------------------------------------------
def _newton_ab(oracle, model, p, uv, ab, iters):
    """undistort_ref.unproject_newton's iteration from the start ab: rays (a, b, 1) with oracle.project(ray) == uv."""
    f = lambda q: oracle.project(model, p, np.concatenate([q, np.ones((len(q), 1))], axis=1))
    e = 1e-6
    for _ in range(iters):
        r = f(ab) - uv
        Ja = (f(ab + [e, 0.0]) - f(ab - [e, 0.0])) / (2 * e)
        Jb = (f(ab + [0.0, e]) - f(ab - [0.0, e])) / (2 * e)
        det = Ja[:, 0] * Jb[:, 1] - Jb[:, 0] * Ja[:, 1]
        da = (r[:, 0] * Jb[:, 1] - Jb[:, 0] * r[:, 1]) / det
        db = (Ja[:, 0] * r[:, 1] - r[:, 0] * Ja[:, 1]) / det
        ab = ab - np.stack([da, db], axis=1)
    return ab


def _kb4_wide(oracle, p, uv):
    """KB4 rays of pixels far from the centre: Newton on the polar angle t of r = t + k1 t^3 + k2 t^5 + k3 t^7 + k4 t^9."""
    mx, my = (uv[:, 0] - p[2]) / p[0], (uv[:, 1] - p[3]) / p[1]
    r = np.sqrt(mx * mx + my * my)
    t = r.copy()
    for _ in range(30):
        t2 = t * t
        f = t * (1.0 + t2 * (p[4] + t2 * (p[5] + t2 * (p[6] + t2 * p[7])))) - r
        fp = 1.0 + t2 * (3.0 * p[4] + t2 * (5.0 * p[5] + t2 * (7.0 * p[6] + t2 * 9.0 * p[7])))
        t = t - f / fp
    ok = (t > 0.0) & (t < math.pi)
    ray = np.stack([np.sin(t) * mx / r, np.sin(t) * my / r, np.cos(t)], axis=1)
    if ok.any():
        assert np.abs(oracle.project(KB4, p, ray[ok]) - uv[ok]).max() <= 1e-9
    return ray, ok


def rays(oracle, model, params, u, v, start=None, iters=14):
    """Step 2 over arrays of pixels: (rays [n, 3], ok [n], what `start` takes for pixels that lie within a few 1e-8 px of these)."""
    p = np.asarray(params, dtype=np.float64)
    u, v = np.asarray(u, dtype=np.float64).reshape(-1), np.asarray(v, dtype=np.float64).reshape(-1)
    mx, my = (u - p[2]) / p[0], (v - p[3]) / p[1]
    r2 = mx * mx + my * my
    if model in (UCM, EUCM):
        alpha, beta = p[4], (p[5] if model == EUCM else 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            t1 = 1.0 - (2.0 * alpha - 1.0) * beta * r2
            ok = t1 >= 0.0
            if alpha > 0.5:
                ok &= ~(r2 > 1.0 / (beta * (2.0 * alpha - 1.0)))
            mz = (1.0 - beta * alpha * alpha * r2) / (alpha * np.sqrt(np.where(ok, t1, 0.0)) + (1.0 - alpha))
            nrm = np.sqrt(r2 + mz * mz)
        return np.stack([mx / nrm, my / nrm, mz / nrm], axis=1), ok, None
    uv = np.stack([u, v], axis=1)
    wide = (np.sqrt(r2) >= KB4_WIDE) if model == KB4 else np.zeros(len(u), dtype=bool)
    ray, ok = np.zeros((len(u), 3)), np.zeros(len(u), dtype=bool)
    ab = np.zeros((len(u), 2))
    if wide.any():
        ray[wide], ok[wide] = _kb4_wide(oracle, p, uv[wide])
    front = ~wide
    if front.any():
        if start is None:
            rr = undistort_ref.unproject_newton(oracle, model, p, uv[front], iters=iters)
            ab[front] = rr[:, :2] / rr[:, 2:3]
        else:
            ab[front] = _newton_ab(oracle, model, p, uv[front], start[front], 2)
        q = np.concatenate([ab[front], np.ones((int(front.sum()), 1))], axis=1)
        with np.errstate(invalid="ignore"):
            good = np.isfinite(q).all(axis=1)
            back = np.full((len(q), 2), np.inf)
            if good.any():
                back[good] = oracle.project(model, p, q[good])
            good &= np.abs(back - uv[front]).sum(axis=1) < 1e-9
        ray[front] = q / np.linalg.norm(q, axis=1, keepdims=True)
        ok[front] = good
    return ray, ok, ab


def ray_classes(oracle, model, params, R, tb, target, u, v, start=None):
    """Steps 2 to 5 over arrays of sub-pixel positions: (class [n], the start for positions next to these)."""
    ray, ok, ab = rays(oracle, model, params, u, v, start)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = [R[0, j] * ray[:, 0] + R[1, j] * ray[:, 1] + R[2, j] * ray[:, 2] for j in range(3)]
        k = tb[2] / d[2]
        front = ok & np.isfinite(k) & (k > 0)
        X, Y = k * d[0] - tb[0], k * d[1] - tb[1]
        cls = np.where(front, classify(target, np.where(front, X, np.nan), np.where(front, Y, np.nan)), G)
    return cls, ab


def render(oracle, model, params, width, height, pose, target, dtype=np.uint8, ss=4, black=40.0, white=215.0, background=0.0, near=True):
    """One image by the rule: (image [H, W], counts [H, W, 3] of B, W, G rays, near rays per pixel [H, W] - None with near=False)."""
    R, tb = pose_rt(pose)
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    us = (np.arange(width, dtype=np.float64)[:, None] + sub[None, :]).reshape(-1)
    vs = (np.arange(height, dtype=np.float64)[:, None] + sub[None, :]).reshape(-1)
    U, V = np.meshgrid(us, vs)
    U, V = U.reshape(-1), V.reshape(-1)
    cls, ab = ray_classes(oracle, model, params, R, tb, target, U, V)
    per_pixel = lambda a: a.reshape(height, ss, width, ss).sum(axis=(1, 3))
    counts = np.stack([per_pixel(cls == c) for c in (B, W, G)], axis=-1)
    lum = ((counts[..., 0] * float(black) + counts[..., 1] * float(white)) + counts[..., 2] * float(background)) / float(ss * ss)
    dt = np.dtype(dtype)
    img = np.clip(np.rint(lum * (257.0 if dt == np.uint16 else 1.0)), 0, np.iinfo(dt).max).astype(dt)
    if not near:
        return img, counts, None
    is_near = np.zeros(len(U), dtype=bool)
    for du in (-NEAR_PX, NEAR_PX):
        for dv in (-NEAR_PX, NEAR_PX):
            is_near |= ray_classes(oracle, model, params, R, tb, target, U + du, V + dv, ab)[0] != cls
    return img, counts, per_pixel(is_near)


def allowed_difference(n_near, ss, dtype, black=40.0, white=215.0, background=0.0):
    """What a pixel with n_near near rays may differ by: the contribution of those rays plus one level."""
    step = max(abs(white - black), abs(white - background), abs(black - background)) / float(ss * ss)
    return np.ceil(n_near * step * (257.0 if np.dtype(dtype) == np.uint16 else 1.0)) + 1.0


# ---- the cases of the GPU parity tests --------------------------------------------------------------------------------------------
SMALL = {UCM: [30.0, 30.5, 33.2, 21.7, 0.6], EUCM: [30.0, 30.5, 33.2, 21.7, 0.6, 1.1],
         KB4: [45.0, 45.5, 33.2, 21.7, 0.003, 0.0007, -0.002, 0.0002], OPENCV5: [60.0, 60.5, 33.2, 21.7, -0.2, 0.05, 0.001, -0.0005, 0.01]}
BOARD = (7, 5, 0.03)
GRID = tag_ref.Board(0.03, 0.3, 2, 3)
GRID_FROM_4 = tag_ref.Board(0.03, 0.3, 2, 3, first_id=4)


def family():
    return tag_ref.grid_family()


def _board_pose(rot, tilt, axis, centre):
    return pose6(*detect_ref.board_pose(BOARD[0], BOARD[1], BOARD[2], rot, tilt, axis, centre))


def _grid_pose(rot, tilt, axis, centre, board=GRID):
    return pose6(*tag_ref.grid_pose(board, rot, tilt, axis, centre))


def _case(name, model, params, width, height, poses, target, ss=4, dtype=np.uint8, **opts):
    return {"name": name, "model": model, "params": np.asarray(params, dtype=np.float64), "width": width, "height": height,
            "poses": np.asarray(poses, dtype=np.float64).reshape(-1, 6), "target": target, "ss": ss, "dtype": np.dtype(dtype), "opts": opts}


@functools.lru_cache(maxsize=None)
def parity_cases():
    out = []
    names = {UCM: "ucm", EUCM: "eucm", KB4: "kb4", OPENCV5: "opencv5"}
    # both targets through all four models on 67 x 45 (a width that is no multiple of 4), three images: the target in front, tilted
    # and turned, and seen from behind (the mirror image); finite default margins, so the background shows
    for m in (UCM, EUCM, KB4, OPENCV5):
        z = 0.25 if m != OPENCV5 else 0.5
        bp = [_board_pose(12.0, 10.0, 30.0, (0.004, -0.003, z)), _board_pose(-33.0, 35.0, 80.0, (-0.02, 0.03, 0.9 * z)),
              _board_pose(20.0, 170.0, 40.0, (0.01, 0.0, z))]
        out.append(_case(f"board {names[m]}", m, SMALL[m], 67, 45, bp, board_target(*BOARD), 4, np.uint8 if m % 2 == 0 else np.uint16))
        gp = [_grid_pose(15.0, 10.0, 30.0, (0.002, -0.003, 0.6 * z)), _grid_pose(100.0, 30.0, 80.0, (0.01, 0.01, 0.5 * z)),
              _grid_pose(15.0, 160.0, 30.0, (0.0, 0.0, 0.6 * z))]
        out.append(_case(f"grid {names[m]}", m, SMALL[m], 67, 45, gp, grid_target(GRID, family()), 4, np.uint16 if m % 2 == 0 else np.uint8))
    # supersampling 1 and 3; 130 x 67 (more than one workgroup each way); a white plane (margin inf); first_id > 0; other grey levels
    out.append(_case("board ucm 130 x 67 s 3", UCM, [55.0, 55.0, 64.0, 33.0, 0.6], 130, 67, [_board_pose(5.0, 20.0, 10.0, (0.0, 0.0, 0.3))],
                     board_target(*BOARD, margin=np.inf), 3, np.uint8, black=10.0, white=250.0, background=128.0))
    out.append(_case("grid opencv5 130 x 67 s 1 first_id 4", OPENCV5, [110.0, 110.0, 64.0, 33.0, -0.2, 0.05, 0.001, -0.0005, 0.01], 130, 67,
                     [_grid_pose(-20.0, 25.0, 60.0, (0.0, 0.0, 0.12), GRID_FROM_4)], grid_target(GRID_FROM_4, family(), margin=np.inf), 1, np.uint16))
    # a pose whose horizon crosses the image: KB4, the board tilted 80 degrees, a white plane out to the horizon
    out.append(_case("board kb4 horizon", KB4, [60.0, 60.0, 64.5, 33.0, 0.003, 0.0007, -0.002, 0.0002], 130, 67,
                     [_board_pose(10.0, 80.0, 0.0, (0.0, 0.02, 0.15))], board_target(*BOARD, margin=np.inf), 3, np.uint8))
    # a camera whose domain ends inside the image: alpha 0.63, f = 20 px on 67 x 45 - the corners have no ray
    out.append(_case("board ucm domain", UCM, [20.0, 20.0, 33.0, 22.0, 0.63], 67, 45, [_board_pose(0.0, 15.0, 45.0, (0.0, 0.0, 0.08))],
                     board_target(*BOARD, margin=np.inf), 4, np.uint8, background=77.0))
    out.append(_case("grid eucm domain", EUCM, [20.0, 20.0, 33.0, 22.0, 0.63, 1.0], 67, 45, [_grid_pose(0.0, 15.0, 45.0, (0.0, 0.0, 0.05))],
                     grid_target(GRID, family(), margin=np.inf), 4, np.uint8, background=77.0))
    # a board entirely off screen (behind the camera's side): all background; and one pixel
    out.append(_case("board eucm off screen", EUCM, SMALL[EUCM], 67, 45, [_board_pose(0.0, 0.0, 0.0, (3.0, 0.0, 0.2))], board_target(*BOARD), 4,
                     np.uint8, background=9.0))
    out.append(_case("board kb4 1 x 1", KB4, [45.0, 45.0, 0.2, -0.1, 0.003, 0.0007, -0.002, 0.0002], 1, 1,
                     [_board_pose(0.0, 5.0, 0.0, (0.0002, 0.0001, 0.2))], board_target(*BOARD), 3, np.uint16))
    # 65 images: the grid turning in steps through a full circle, in front of the EUCM camera
    turn = [_grid_pose(360.0 * k / 65.0, 20.0, 7.0 * k, (0.001 * (k % 5), -0.002, 0.15)) for k in range(65)]
    out.append(_case("grid eucm 65 images s 1", EUCM, SMALL[EUCM], 67, 45, turn, grid_target(GRID, family()), 1, np.uint8))
    return tuple(out)


_YARD = {}


def yardstick(oracle, case):
    """render() over every pose of a case: (images [n, H, W], near rays per pixel [n, H, W]); computed once per case and shared."""
    if case["name"] not in _YARD:
        res = [render(oracle, case["model"], case["params"], case["width"], case["height"], pose, case["target"], case["dtype"], case["ss"],
                      **case["opts"]) for pose in case["poses"]]
        _YARD[case["name"]] = (np.stack([r[0] for r in res]), np.stack([r[2] for r in res]))
    return _YARD[case["name"]]


# ---- round trips at 512 x 512 under the four GT lenses (synth.GT_PARAMS) --------------------------------------------------------------
# Per model the poses - (in-plane rotation, tilt, tilt axis in degrees, the target's middle in the camera frame) - on which the
# numpy chains below find the whole target: the board through detect_ref.detect -> corner_ref.refine -> api.assemble_checkerboard,
# the grid through tagchain_ref.chain.  RT_*_WORST: the worst distance (px) from model.project of the posed corner over all of a
# model's poses, measured on render()'s uint8 images; the bound the GPU round trips are held to is 1.5 x that (the project's
# convention, detect_ref.BOARD_BOUND).  `python tests/render_ref.py` measures them again.
RT_SIZE = 512
RT_BOARD_POSES = {
    UCM: ((12.0, 10.0, 30.0, (0.004, -0.003, 0.18)), (-20.0, 40.0, 90.0, (0.13, 0.005, 0.13))),
    EUCM: ((12.0, 10.0, 30.0, (0.004, -0.003, 0.18)), (-20.0, 40.0, 90.0, (0.13, 0.005, 0.13))),
    KB4: ((12.0, 10.0, 30.0, (0.004, -0.003, 0.18)), (-20.0, 40.0, 90.0, (0.13, 0.005, 0.13))),
    OPENCV5: ((12.0, 10.0, 30.0, (0.004, -0.003, 0.40)), (-20.0, 25.0, 90.0, (0.12, 0.005, 0.38))),
}
RT_GRID_POSES = {
    UCM: ((15.0, 10.0, 30.0, (0.002, -0.003, 0.12)), (100.0, 25.0, 60.0, (0.05, 0.01, 0.10))),
    EUCM: ((15.0, 10.0, 30.0, (0.002, -0.003, 0.12)), (100.0, 25.0, 60.0, (0.05, 0.01, 0.10))),
    KB4: ((15.0, 10.0, 30.0, (0.002, -0.003, 0.12)), (100.0, 25.0, 60.0, (0.05, 0.01, 0.10))),
    OPENCV5: ((15.0, 10.0, 30.0, (0.002, -0.003, 0.25)), (100.0, 25.0, 60.0, (0.06, 0.01, 0.24))),
}
RT_BOARD_WORST = {UCM: 0.09222, EUCM: 0.08224, KB4: 0.08842, OPENCV5: 0.08522}
RT_GRID_WORST = {UCM: 0.12025, EUCM: 0.09628, KB4: 0.10658, OPENCV5: 0.09859}
RT_BOARD_HALF_WIN, RT_GRID_HALF_WIN = detect_ref.BOARD_HALF_WIN, tag_ref.GRID_HALF_WIN


def rt_bound(worst):
    return 1.5 * worst


def gt_params(model):
    from camera_intrinsic_calibration_rs_amd import synth
    return np.asarray(synth.GT_PARAMS[model], dtype=np.float64)


def rt_board_poses(model):
    return np.stack([_board_pose(*p) for p in RT_BOARD_POSES[model]])


def rt_grid_poses(model):
    return np.stack([_grid_pose(*p) for p in RT_GRID_POSES[model]])


def board_truth(oracle, model, params, pose):
    """model.project of the posed inner corners, id = r cols + c: [rows cols, 2]."""
    cols, rows, sq = BOARD
    R, _ = pose_rt(pose)
    cr = np.stack(np.meshgrid(np.arange(cols), np.arange(rows)), axis=-1).reshape(-1, 2).astype(np.float64)
    Xb = np.concatenate([cr * sq, np.zeros((len(cr), 1))], axis=1)
    return oracle.project(model, params, Xb @ R.T + np.asarray(pose[3:], dtype=np.float64))


def grid_truth(oracle, model, params, pose, board=GRID):
    """model.project of every tag's outer corners in the decoder's order: [tag_rows tag_cols, 4, 2], tag (r, c) at r tag_cols + c."""
    s, pitch = board.tag_size_meter, board.tag_size_meter * (1.0 + board.tag_spacing)
    R, _ = pose_rt(pose)
    P = []
    for r in range(board.tag_rows):
        for c in range(board.tag_cols):
            x, y = c * pitch, -r * pitch
            P += [(x, y, 0.0), (x + s, y, 0.0), (x + s, y - s, 0.0), (x, y - s, 0.0)]
    return oracle.project(model, params, np.array(P) @ R.T + np.asarray(pose[3:], dtype=np.float64)).reshape(-1, 4, 2)


def board_error(found_xy, truth):
    """The worst corner distance under the labelling rule's admissible rotation: the labelling fixes the board up to the half turn
    (id -> n - 1 - id), which a plain checkerboard cannot tell apart."""
    found_xy = np.asarray(found_xy, dtype=np.float64).reshape(-1, 2)
    return min(float(np.linalg.norm(found_xy - t, axis=1).max()) for t in (truth, truth[::-1]))


def chain_board(img):
    """The numpy board chain on one image: the corners [rows cols, 2] in id order, or None."""
    import corner_ref
    from camera_intrinsic_calibration_rs_amd import api
    cols, rows, sq = BOARD
    cand = detect_ref.detect(img)
    r = corner_ref.refine(img, cand["xy"].astype(np.float64), RT_BOARD_HALF_WIN, 30, 1e-3)
    keep = np.asarray(r["status"]) == 0
    res = api.assemble_checkerboard(np.asarray(r["xy"])[keep], cand["hess"][keep].astype(np.float64), (cols, rows), sq)
    if res is None:
        return None
    return np.array([res[i] for i in range(cols * rows)])


def chain_grid(img):
    """The numpy tag chain on one 512 x 512 uint8 image: tagchain_ref.chain's result with the options detect_tags_dev defaults to."""
    import tagchain_ref
    return tagchain_ref.chain(img, 6, family().codes, tagchain_ref.opts(np.uint8, RT_SIZE, RT_SIZE))


def measure_board(oracle, model):
    """The worst corner error of the board chain over the model's round-trip poses; every board must be found."""
    p, worst = gt_params(model), 0.0
    for pose in rt_board_poses(model):
        img = render(oracle, model, p, RT_SIZE, RT_SIZE, pose, board_target(*BOARD), near=False)[0]
        xy = chain_board(img)
        assert xy is not None
        worst = max(worst, board_error(xy, board_truth(oracle, model, p, pose)))
    return worst


def measure_grid(oracle, model):
    """The same for the tag chain; every tag must decode at Hamming distance 0."""
    p, worst = gt_params(model), 0.0
    for pose in rt_grid_poses(model):
        img = render(oracle, model, p, RT_SIZE, RT_SIZE, pose, grid_target(GRID, family()), near=False)[0]
        res = chain_grid(img)
        assert list(res["id"]) == list(range(6)) and not np.any(res["hamming"])
        truth = grid_truth(oracle, model, p, pose)
        worst = max(worst, max(float(np.linalg.norm(res["corners"][i] - truth[t], axis=1).max()) for i, t in enumerate(res["id"])))
    return worst


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import binding
    binding.load()
    for m, name in ((UCM, "ucm"), (EUCM, "eucm"), (KB4, "kb4"), (OPENCV5, "opencv5")):
        print(f"{name}: board worst {measure_board(binding, m):.5f} px (recorded {RT_BOARD_WORST[m]}), "
              f"grid worst {measure_grid(binding, m):.5f} px (recorded {RT_GRID_WORST[m]})", flush=True)
