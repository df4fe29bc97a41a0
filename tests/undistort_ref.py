"""Independent numpy f64 yardstick of the undistortion path (ccal_kernels_undistort.hip).  The kernels are never compared with
themselves: projection VALUES come from oracle.project; this file restates, from the definitions,

  * where `project` is defined (the domains of oracle/ccal_oracle.hpp:334-343) and the UCM / EUCM unprojection domain,
  * the rays of an undistortion map, R^T ((x - cx) / fx, (y - cy) / fy, 1),
  * estimate_new_camera_matrix_for_undistort from four unprojected edge midpoints,
  * an unprojection by Newton's method on oracle.project (rays in front of the camera; used for the edge midpoints),
  * bilinear resampling in f64 with the semantics include/ccal.h fixes for ccal_remap.

`near` masks mark inputs whose validity margin is within 1e-12 relative of the domain boundary: a last-bit difference in the
arithmetic may put them on either side, the tests leave them out (and cap how many there may be)."""
import numpy as np

UCM, EUCM, KB4, OPENCV5 = 0, 1, 2, 3
BOUNDARY_REL = 1e-12


def project_valid(model, params, xyz):
    """(valid, near) of GenericModel::project for camera-frame points [n, 3]."""
    p = np.asarray(params, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if model in (UCM, EUCM):
        alpha, beta = p[4], (p[5] if model == EUCM else 1.0)
        d = np.sqrt(beta * (x * x + y * y) + z * z)
        w = alpha / (1.0 - alpha) if alpha <= 0.5 else (1.0 - alpha) / alpha
        margin = z + w * d
        return margin > 0.0, np.abs(margin) <= BOUNDARY_REL * np.maximum(d, np.abs(z))
    if model == KB4:
        n2 = x * x + y * y + z * z
        return n2 > 0.0, np.zeros(len(z), dtype=bool)
    return z > 1e-9, np.abs(z - 1e-9) <= BOUNDARY_REL * 1e-9


def unproject_domain(model, params, uv):
    """UCM / EUCM only: (valid, near) of the closed-form unprojection domain, invalid iff alpha > 1/2 and r^2 > 1 / (beta (2 alpha - 1))."""
    assert model in (UCM, EUCM)
    p = np.asarray(params, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    mx, my = (uv[:, 0] - p[2]) / p[0], (uv[:, 1] - p[3]) / p[1]
    r2 = mx * mx + my * my
    alpha, beta = p[4], (p[5] if model == EUCM else 1.0)
    if alpha <= 0.5:
        return np.ones(len(r2), dtype=bool), np.zeros(len(r2), dtype=bool)
    lim = 1.0 / (beta * (2.0 * alpha - 1.0))
    return ~(r2 > lim), np.abs(r2 - lim) <= BOUNDARY_REL * lim


def map_rays(K, R, w, h):
    """Camera-frame ray of every pixel of the new w x h pinhole image: [h * w, 3], row-major over (y, x)."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    v = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1).reshape(-1, 3)
    return v @ R          # row form of R^T v


def undistort_map(oracle, model, params, K, R, w, h):
    """(xmap, ymap) f64 [h, w] with NaN where project is undefined, and the `near` mask [h, w]."""
    rays = map_rays(K, R, w, h)
    valid, near = project_valid(model, params, rays)
    uv = np.full((w * h, 2), np.nan)
    if valid.any():
        uv[valid] = oracle.project(model, params, rays[valid])
    return uv[:, 0].reshape(h, w), uv[:, 1].reshape(h, w), near.reshape(h, w)


def edge_midpoints(params, width, height):
    cx, cy = float(params[2]), float(params[3])
    return np.array([[cx, 0.0], [width - 1.0, cy], [cx, height - 1.0], [0.0, cy]])


def new_camera_matrix(rays4, balance, new_w, new_h):
    """The formula of estimate_new_camera_matrix_for_undistort on four unprojected edge midpoints [4, 3]; None where one of
    them is not finite or not in front of the camera."""
    rays4 = np.asarray(rays4, dtype=np.float64).reshape(4, 3)
    if not np.isfinite(rays4).all() or not (rays4[:, 2] > 0.0).all():
        return None
    x, y = rays4[:, 0] / rays4[:, 2], rays4[:, 1] / rays4[:, 2]
    min_x, max_x, min_y, max_y = abs(x.min()), x.max(), abs(y.min()), y.max()
    ra, rb = new_w / (min_x + max_x), new_h / (min_y + max_y)
    f = balance * max(ra, rb) + (1.0 - balance) * min(ra, rb)
    return np.array([[f, 0.0, new_w * min_x / (min_x + max_x)], [0.0, f, new_h * min_y / (min_y + max_y)], [0.0, 0.0, 1.0]])


def unproject_newton(oracle, model, params, uv, iters=40):
    """Unit rays (a, b, 1) / |.| with oracle.project(ray) == uv, by Newton's method with central differences from the pinhole
    guess.  Only for pixels whose ray lies well in front of the camera (the edge midpoints of the tests' models)."""
    p = np.asarray(params, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    ab = np.stack([(uv[:, 0] - p[2]) / p[0], (uv[:, 1] - p[3]) / p[1]], axis=1)
    f = lambda q: oracle.project(model, p, np.concatenate([q, np.ones((len(q), 1))], axis=1))
    for _ in range(iters):
        r = f(ab) - uv
        e = 1e-6
        Ja = (f(ab + [e, 0.0]) - f(ab - [e, 0.0])) / (2 * e)
        Jb = (f(ab + [0.0, e]) - f(ab - [0.0, e])) / (2 * e)
        det = Ja[:, 0] * Jb[:, 1] - Jb[:, 0] * Ja[:, 1]
        da = (r[:, 0] * Jb[:, 1] - Jb[:, 0] * r[:, 1]) / det
        db = (Ja[:, 0] * r[:, 1] - r[:, 0] * Ja[:, 1]) / det
        ab = ab - np.stack([da, db], axis=1)
    rays = np.concatenate([ab, np.ones((len(ab), 1))], axis=1)
    return rays / np.linalg.norm(rays, axis=1, keepdims=True)


def remap(img, xmap, ymap):
    """Bilinear resampling in f64.  img [H][W] or [H][W][C] (uint8 / uint16), maps [h][w] -> [h][w](C), same dtype.  Returns
    (out, valid [h][w])."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    src = img.reshape(H, W, -1).astype(np.float64)
    mx, my = np.asarray(xmap, dtype=np.float64), np.asarray(ymap, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(mx) & np.isfinite(my) & (mx >= 0.0) & (mx <= W - 1) & (my >= 0.0) & (my <= H - 1)
    sx, sy = np.where(valid, mx, 0.0), np.where(valid, my, 0.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = (sx - x0)[..., None], (sy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    val = (1 - ay) * ((1 - ax) * src[y0, x0] + ax * src[y0, x1]) + ay * ((1 - ax) * src[y1, x0] + ax * src[y1, x1])
    out = np.clip(np.floor(val + 0.5), 0, np.iinfo(img.dtype).max)
    out = np.where(valid[..., None], out, 0.0).astype(img.dtype)
    return out.reshape(mx.shape + img.shape[2:]), valid


# ---- the seeded inputs the GPU tests use (the CPU tests hold them to the boundary caps) ------------------------------------------
def seeded_rays(model, n, seed=7):
    """n unit rays with polar angles up to 170 degrees: behind the camera (z < 0) and beyond the UCM / EUCM cone included.  OPENCV5:
    rays between 60 and 90 degrees off the axis are mirrored behind the camera - close to the z = 0 plane that model's pixel values
    grow without bound and no absolute pixel tolerance can hold.  From n = 63 on, the first two rays are the optical axis and its
    opposite."""
    rng = np.random.default_rng(seed + 1000 * model + n)
    theta = rng.uniform(0.0, np.deg2rad(170.0), n)
    phi = rng.uniform(-np.pi, np.pi, n)
    rays = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
    rays *= rng.uniform(0.2, 5.0, n)[:, None]
    if model == OPENCV5:
        flip = (theta > np.deg2rad(60.0)) & (theta <= np.deg2rad(90.0))
        rays[flip, 2] *= -1.0
    if n >= 63:
        rays[0] = [0.0, 0.0, 1.0]
        rays[1] = [0.0, 0.0, -1.0]
    return rays


def seeded_pixels(params, n, width, height, ring=40.0, seed=11):
    """n pixels over the image and a ring of `ring` px around it; from n = 63 on, the first is the principal point."""
    rng = np.random.default_rng(seed + n)
    uv = np.stack([rng.uniform(-ring, width + ring, n), rng.uniform(-ring, height + ring, n)], axis=1)
    if n >= 63:
        uv[0] = [params[2], params[3]]
    return uv
