"""The yardstick of the saddle detector: an independent numpy int64 restatement of the rule that include/ccal.h states at
ccal_detect_corners_batch, written from that text (whole-array arithmetic, non-maximum suppression by explicit comparison with
every shifted copy of the response: no tiles, no slots, no scan), and the renderer of the checkerboard fixture the tests share.
It depends on no GPU, on no oracle and on nothing outside this repository."""
import functools

import numpy as np

B5 = np.array([1, 4, 6, 4, 1], dtype=np.int64)
NONE = np.iinfo(np.int64).min


def smooth(img):
    """S over the pixels 2 <= x <= W - 3, 2 <= y <= H - 3: int64 [H - 4][W - 4] (S[y - 2][x - 2] = S(x, y))."""
    im = np.asarray(img).astype(np.int64)
    H, W = im.shape
    rows = sum(int(B5[i]) * im[:, i:W - 4 + i] for i in range(5))
    return sum(int(B5[j]) * rows[j:H - 4 + j, :] for j in range(5))


def response(img, step):
    """(R, hxx, hyy, hxy) over the domain, int64 [dh][dw] with [y - d0][x - d0], d0 = step + 2; None when the image has no domain."""
    H, W = np.asarray(img).shape
    s, d0 = int(step), int(step) + 2
    dw, dh = W - 2 * d0, H - 2 * d0
    if dw <= 0 or dh <= 0:
        return None
    S = smooth(img)                                     # index (y - 2, x - 2)
    at = lambda ox, oy: S[d0 - 2 + oy:d0 - 2 + oy + dh, d0 - 2 + ox:d0 - 2 + ox + dw]      # noqa: E731  S(x + ox, y + oy) over the domain
    hxx = at(s, 0) - 2 * at(0, 0) + at(-s, 0)
    hyy = at(0, s) - 2 * at(0, 0) + at(0, -s)
    hxy = at(s, s) - at(s, -s) - at(-s, s) + at(-s, -s)
    return hxy * hxy - 16 * hxx * hyy, hxx, hyy, hxy


def local_maxima(R, r, min_response):
    """The boolean map of the local maxima of R [dh][dw] (the whole array is the domain)."""
    dh, dw = R.shape
    pad = np.full((dh + 2 * r, dw + 2 * r), NONE, dtype=np.int64)
    pad[r:r + dh, r:r + dw] = R
    ok = R >= min_response
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            q = pad[r + dy:r + dy + dh, r + dx:r + dx + dw]
            ok &= (R > q) if (dy < 0 or (dy == 0 and dx < 0)) else (R >= q)
    return ok


def detect(img, step=1, nms_radius=5, min_response=1, rel_q10=102, cap=4096):
    """One image (any integer dtype, [H][W]): {"count", "xy" int32 [k, 2], "hess" int32 [k, 3], "response" int64 [k], "rmax",
    "threshold"} with k = min(count, cap), the candidates in row-major order of (y, x)."""
    empty = {"count": 0, "xy": np.zeros((0, 2), np.int32), "hess": np.zeros((0, 3), np.int32), "response": np.zeros(0, np.int64),
             "rmax": None, "threshold": None}
    res = response(img, step)
    if res is None:
        return empty
    R, hxx, hyy, hxy = res
    rmax = int(R.max())
    if rmax <= 0:
        return dict(empty, rmax=rmax)
    T = max(int(min_response), (rmax >> 10) * int(rel_q10))
    ys, xs = np.nonzero(local_maxima(R, int(nms_radius), int(min_response)) & (R >= T))           # nonzero: row-major order
    count = len(ys)
    k = min(count, int(cap))
    ys, xs = ys[:k], xs[:k]
    d0 = int(step) + 2
    return {"count": count,
            "xy": np.stack([xs + d0, ys + d0], axis=1).astype(np.int32),
            "hess": np.stack([hxx[ys, xs], hyy[ys, xs], hxy[ys, xs]], axis=1).astype(np.int32),
            "response": R[ys, xs].astype(np.int64), "rmax": rmax, "threshold": T}


# ---- the checkerboard fixture -----------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float64)


class Camera:
    """A pinhole (f, cx, cy) with the one-parameter division model: with (xd, yd) = ((u - cx) / f, (v - cy) / f) and
    rd^2 = xd^2 + yd^2 the ray of pixel (u, v) is (xd, yd, 1 + lam rd^2).  Both ways are closed forms."""

    def __init__(self, f, cx, cy, lam):
        self.f, self.cx, self.cy, self.lam = float(f), float(cx), float(cy), float(lam)

    def rays(self, u, v):
        xd, yd = np.broadcast_arrays((u - self.cx) / self.f, (v - self.cy) / self.f)
        return np.stack([xd, yd, 1.0 + self.lam * (xd * xd + yd * yd)], axis=-1)

    def project(self, X):
        xu, yu = X[..., 0] / X[..., 2], X[..., 1] / X[..., 2]
        ru = np.hypot(xu, yu)
        if self.lam == 0.0:
            k = np.ones_like(ru)
        else:                                           # rd = ru (1 + lam rd^2): the root that tends to ru as lam -> 0
            with np.errstate(invalid="ignore", divide="ignore"):
                rd = (1.0 - np.sqrt(1.0 - 4.0 * self.lam * ru * ru)) / (2.0 * self.lam * ru)
                k = np.where(ru > 1e-12, rd / ru, 1.0)
        return np.stack([self.f * xu * k + self.cx, self.f * yu * k + self.cy], axis=-1)


def board_pose(cols, rows, square, rot_deg, tilt_deg, tilt_axis_deg, centre_xyz):
    """Board -> camera: the board's middle goes to centre_xyz, the board is turned by rot_deg in its plane and tilted by tilt_deg
    about the in-plane axis at tilt_axis_deg: (R, t)."""
    ax = np.deg2rad(tilt_axis_deg)
    R = _rot("z", ax) @ _rot("x", np.deg2rad(tilt_deg)) @ _rot("z", -ax) @ _rot("z", np.deg2rad(rot_deg))
    mid = np.array([(cols - 1) * square / 2.0, (rows - 1) * square / 2.0, 0.0])
    return R, np.asarray(centre_xyz, dtype=np.float64) - R @ mid


def render_board(width, height, cam, R, t, cols, rows, square, dtype=np.uint8, black=40.0, white=215.0, ss=4):
    """A cols x rows inner-corner checkerboard ((cols + 1) x (rows + 1) squares, white beyond them) seen by `cam` at pose (R, t):
    every pixel the mean of ss x ss rays, each intersected with the board plane.  Returns (image, true corner pixels [rows*cols, 2]
    in the order id = r * cols + c)."""
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    u = (np.arange(width, dtype=np.float64)[:, None] + sub[None, :]).reshape(-1)
    v = (np.arange(height, dtype=np.float64)[:, None] + sub[None, :]).reshape(-1)
    d = cam.rays(u[None, :], v[:, None])                # [H ss][W ss][3]
    dn, tn = d @ R, R.T @ t                             # R^T d, R^T t
    with np.errstate(divide="ignore", invalid="ignore"):
        k = tn[2] / dn[..., 2]
        bx, by = k * dn[..., 0] - tn[0], k * dn[..., 1] - tn[1]
        i, j = np.floor(bx / square) + 1.0, np.floor(by / square) + 1.0
        on = (k > 0) & (i >= 0) & (i <= cols) & (j >= 0) & (j <= rows)
    dark = on & (np.mod(i + j, 2.0) == 0.0)
    lum = np.where(dark, black, white).reshape(height, ss, width, ss).mean(axis=(1, 3))
    cr = np.stack(np.meshgrid(np.arange(cols), np.arange(rows)), axis=-1).reshape(-1, 2).astype(np.float64)
    Xb = np.concatenate([cr * square, np.zeros((len(cr), 1))], axis=1)
    true = cam.project(Xb @ R.T + t)
    if dtype == np.uint16:
        return np.rint(lum * 257.0).astype(np.uint16), true
    return np.rint(lum).astype(np.uint8), true


# The board fixture: a 7 x 5 inner-corner board of 30 mm squares in 320 x 240 images, f = 400 px, at 0.37 .. 0.40 m: 21 .. 38 px
# between neighbouring corners (30 px head-on; the 35 degree tilt spreads them most).  Per frame: (lam of the division model, in-plane
# rotation, tilt, tilt axis - degrees -, the board's middle in the camera frame).  Every corner lies at least 12 px inside the image.
BOARD_COLS, BOARD_ROWS, BOARD_SQUARE = 7, 5, 0.03
BOARD_W, BOARD_H, BOARD_F = 320, 240, 400.0
BOARD_FRAMES = (
    (0.0, 12.0, 10.0, 30.0, (0.004, -0.003, 0.40)),
    (-0.35, -33.0, 35.0, 80.0, (-0.006, 0.009, 0.37)),
    (-0.35, 100.0, 25.0, -20.0, (0.003, 0.005, 0.40)),
)
BOARD_HALF_WIN = 5
# The worst distance (px) from the true corner pixel that detect() -> corner_ref.refine() (half_win 5, eps 1e-3, 30 iterations) ->
# api.assemble_checkerboard measured over the three uint8 frames, and the bound the tests hold results to: 1.5 x that (the
# rendering and the quantisation are the only noise, nothing is random).
BOARD_WORST = 0.09115
BOARD_BOUND = 1.5 * BOARD_WORST


@functools.lru_cache(maxsize=None)
def board_frames(dtype=np.uint8):
    """The fixture's frames: (images [3][240][320], true corner pixels [3][35][2])."""
    imgs, truth = [], []
    for lam, rot, tilt, axis, centre in BOARD_FRAMES:
        cam = Camera(BOARD_F, (BOARD_W - 1) / 2.0, (BOARD_H - 1) / 2.0, lam)
        R, t = board_pose(BOARD_COLS, BOARD_ROWS, BOARD_SQUARE, rot, tilt, axis, centre)
        im, tr = render_board(BOARD_W, BOARD_H, cam, R, t, BOARD_COLS, BOARD_ROWS, BOARD_SQUARE, dtype)
        imgs.append(im); truth.append(tr)
    out = np.stack(imgs), np.stack(truth)
    out[0].setflags(write=False); out[1].setflags(write=False)
    return out


# ---- the images of the GPU parity tests -----------------------------------------------------------------------------------------
def extreme_blocks(width=64, height=48, block=3):
    """uint16, 0 / 65535 alternating in block x block squares: the largest magnitudes S, the Hessian and R can take."""
    yy, xx = np.mgrid[0:height, 0:width]
    return np.where(((xx // block) + (yy // block)) % 2 == 0, 0, 65535).astype(np.uint16)


def periodic8(width=96, height=80, dtype=np.uint8):
    """A pattern that repeats exactly with period 8 in x and y (one blurred saddle-like cell): equal maxima 8 px apart everywhere,
    across every tile border, so with nms_radius 8 the tie rule alone decides."""
    cell = np.array([[(37 * i * i + 91 * j * j + 53 * i * j + 11 * i + 7 * j) % 251 for i in range(8)] for j in range(8)])
    img = np.tile(cell, (height // 8 + 1, width // 8 + 1))[:height, :width]
    return (img * 257).astype(np.uint16) if dtype == np.uint16 else img.astype(np.uint8)
