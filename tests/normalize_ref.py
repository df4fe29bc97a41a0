"""The numpy yardstick of local contrast normalisation (include/ccal.h, "local contrast normalisation"; ccal_kernels_normalize.hip):
the window sums, the variance term and the exact integer square root in int64, the last two steps in IEEE f64 with every operation
rounded on its own.  The GPU tests hold the device to normalize() by exact equality.

Also the degraded frames on which the plain numpy chains lose the target and the normalised ones find it (tests/test_normalize_cpu.py,
tests/test_gpu_normalize.py), with the worst corner errors the numpy chains reach on the normalised frames recorded below.
`python tests/normalize_ref.py` measures them again (CPU, minutes) and prints them beside the recorded constants, with the variant
"detect on the normalised frame, refine on the original" (EXPERIMENTS.md)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MAX_RADIUS = 32
DEFAULTS = dict(radius=16, min_sigma=4.0, amp=64.0)


def opts(**kw):
    o = dict(DEFAULTS)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


def isqrt(v):
    """The largest s with s s <= v over an int64 array (0 <= v < 2^62): seeded from the f64 square root, corrected in integers both
    ways, so that the result does not depend on how the seed rounds."""
    v = np.asarray(v, dtype=np.int64)
    s = np.sqrt(v.astype(np.float64)).astype(np.int64)
    while True:
        high = s * s > v
        if not high.any():
            break
        s = s - high
    while True:
        low = (s + 1) * (s + 1) <= v
        if not low.any():
            break
        s = s + low
    return s


def _window_sums(I, r, axis):
    """The sum over -r .. r along `axis` with clamped borders, int64."""
    pad = [(0, 0)] * I.ndim
    pad[axis] = (r + 1, r)
    c = np.cumsum(np.pad(I, pad, mode="edge"), axis=axis, dtype=np.int64)
    n = I.shape[axis]
    return np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis) - np.take(c, np.arange(0, n), axis=axis)


def terms(src, radius, min_sigma):
    """(d, s) int64 [n, H, W] of the rule: d = N I - S1, s = max(isqrt(N S2 - S1 S1), N F)."""
    src = np.asarray(src)
    assert src.ndim == 3 and src.dtype in (np.dtype(np.uint8), np.dtype(np.uint16))
    r = int(radius)
    assert 1 <= r <= MAX_RADIUS
    I = src.astype(np.int64) * (257 if src.dtype == np.uint8 else 1)
    N = (2 * r + 1) * (2 * r + 1)
    S1 = _window_sums(_window_sums(I, r, 2), r, 1)
    S2 = _window_sums(_window_sums(I * I, r, 2), r, 1)
    v = N * S2 - S1 * S1
    assert (v >= 0).all()
    F = max(1, int(np.rint(257.0 * float(min_sigma))))
    return N * I - S1, np.maximum(isqrt(v), N * F)


def normalize(src, dst_dtype, o):
    """src [n, H, W] (uint8 or uint16) by the rule with the options o (radius, min_sigma, amp): the images [n, H, W] of dst_dtype."""
    d, s = terms(src, o["radius"], o["min_sigma"])
    q = d.astype(np.float64) / s.astype(np.float64)
    Y = 128.0 + float(o["amp"]) * q
    if np.dtype(dst_dtype) == np.uint8:
        return np.rint(np.minimum(np.maximum(Y, 0.0), 255.0)).astype(np.uint8)
    return np.rint(np.minimum(np.maximum(Y * 257.0, 0.0), 65535.0)).astype(np.uint16)


# ---- the cases of tests/test_gpu_normalize.py: blocks through ccal_normalize_dev -------------------------------------------------------
def _case(name, src, dst, n, height, width, kind="random", **o):
    return {"name": name, "src": np.dtype(src), "dst": np.dtype(dst), "n": n, "height": height, "width": width, "kind": kind, "opts": opts(**o)}


@functools.lru_cache(maxsize=None)
def parity_cases():
    """Every u8 / u16 source and destination pair; radii 1, 5, 16, 32; one pixel, an image inside the halo, a column, 67 x 45 (an odd
    u16 width, a u8 width that is no multiple of 4), 130 x 67 (three tiles across, three down),
    65 images, 70 000 images (more than the grid's image axis holds); 0 / 65535 halves at r = 32 (v above 2^53); a constant image;
    min_sigma 0 and 255; amp 0 and 1000."""
    u8, u16 = np.uint8, np.uint16
    return (
        _case("1 x 1", u8, u8, 1, 1, 1),
        _case("1 x 1 u16 r 1", u16, u16, 1, 1, 1, radius=1),
        _case("3 x 2 r 32", u16, u8, 2, 2, 3, radius=32),
        _case("1 x 40 column r 5", u8, u16, 1, 40, 1, radius=5),
        _case("67 x 45 r 1", u16, u16, 2, 45, 67, radius=1, min_sigma=0.0),
        _case("67 x 45 r 5", u8, u8, 2, 45, 67, radius=5),
        _case("67 x 45 r 16 u8 to u16", u8, u16, 1, 45, 67),
        _case("67 x 45 r 32 u16 to u8", u16, u8, 1, 45, 67, radius=32),
        _case("67 x 45 min_sigma 0", u8, u8, 1, 45, 67, radius=5, min_sigma=0.0),
        _case("67 x 45 min_sigma 255", u16, u16, 1, 45, 67, radius=5, min_sigma=255.0),
        _case("67 x 45 amp 0", u16, u8, 1, 45, 67, amp=0.0),
        _case("67 x 45 amp 1000", u8, u16, 1, 45, 67, radius=5, amp=1000.0),
        _case("130 x 67 r 16 u16", u16, u16, 2, 67, 130),
        _case("130 x 67 r 32 u8", u8, u8, 2, 67, 130, radius=32),
        _case("130 x 67 r 5 u16 to u8", u16, u8, 1, 67, 130, radius=5),
        _case("130 x 67 r 1 u8 to u16", u8, u16, 1, 67, 130, radius=1),
        _case("halves r 32", u16, u16, 1, 67, 130, kind="halves", radius=32, min_sigma=0.0),
        _case("halves r 32 to u8", u16, u8, 1, 45, 67, kind="halves", radius=32),
        _case("constant u16", u16, u16, 1, 45, 67, kind="constant", min_sigma=0.0),
        _case("constant u8", u8, u8, 1, 45, 67, kind="constant", radius=32),
        _case("65 images 9 x 5", u8, u16, 65, 5, 9, radius=5),
        _case("70000 images 3 x 2", u8, u8, 70000, 2, 3, radius=1, min_sigma=0.0),
    )


def source(case):
    """The source block of a case: random over the whole range of its type, 0 / 65535 halves, or a constant."""
    n, H, W = case["n"], case["height"], case["width"]
    hi = np.iinfo(case["src"]).max
    if case["kind"] == "halves":
        return np.broadcast_to(np.where(np.arange(W) < W // 2, 0, hi).astype(case["src"]), (n, H, W)).copy()
    if case["kind"] == "constant":
        return np.full((n, H, W), 0x5B if case["src"] == np.uint8 else 0x5B17, dtype=case["src"])
    rng = np.random.default_rng(sum(map(ord, case["name"])))
    return rng.integers(0, hi + 1, (n, H, W)).astype(case["src"])


# ---- round trips: degraded frames that the plain chains lose --------------------------------------------------------------------------
# Boards: the 7 x 5 board of detect_ref in 320 x 240 images under Camera(400, 159.5, 119.5, -0.35) at board_pose(7, 5, 0.03, 12, 10, 30,
# centre); the uint16 render through photo_ref.apply (numpy tables) to uint8, every image on its own (the noise stream is the seed's).
# Grids: tag_ref.GRID_FRAMES[0] and [1] at tag_ref's pose, the same way.  Per case: (vignette, gain, the board's centre / the frame).
# The plain numpy chains (detect_ref.detect -> corner_ref.refine -> api.assemble_checkerboard; tagchain_ref.chain) find no board and
# fewer than six tags on them; on normalize(..., DEFAULTS) they find every board and all six tags at Hamming distance 0.
# RT_NORM_*_WORST: the worst distance (px) from the true corner that the numpy chains reach on the normalised uint8 frames; the GPU
# round trips are held to 1.5 x that (rt_bound; the project's convention, detect_ref.BOARD_BOUND).
RT_BOARD_PHOTO = dict(blur_sigma=1.2, noise_read=2.0, noise_shot=0.05, seed=2024)
RT_GRID_PHOTO = dict(blur_sigma=0.8, noise_read=2.0, noise_shot=0.05, seed=2024)
RT_BOARD_CASES = (
    (1.0, 1.0, (0.045, 0.03, 0.40)),
    (2.0, 1.0, (0.045, 0.03, 0.40)),
    (2.0, 1.0, (-0.05, 0.035, 0.42)),
    (4.0, 1.0, (0.004, -0.003, 0.40)),
)
RT_GRID_CASES = ((4.0, 1.0, 0), (4.0, 1.0, 1), (0.5, 0.3, 0), (0.5, 0.3, 1))
RT_NORM_BOARD_WORST = (0.23164, 0.35482, 0.24377, 0.42054)
RT_NORM_GRID_WORST = (0.27236, 0.27285, 0.33154, 0.37128)
# normalised at radius 8 and 32 (boards), and the variant "detect on the normalised frame, refine the found corners on the original"
# are measured by the script only (EXPERIMENTS.md).


def rt_bound(worst):
    return 1.5 * worst


def _degrade(ideal_u16, photo):
    import photo_ref as pr
    o = pr.opts(**photo)
    return pr.apply(ideal_u16[None], np.uint8, pr.tables(o), o)[0]


@functools.lru_cache(maxsize=None)
def rt_board(k):
    """Board case k: (the degraded uint8 frame [240, 320], the true corner pixels [35, 2])."""
    import detect_ref as dr
    vignette, gain, centre = RT_BOARD_CASES[k]
    cam = dr.Camera(dr.BOARD_F, (dr.BOARD_W - 1) / 2.0, (dr.BOARD_H - 1) / 2.0, -0.35)
    R, t = dr.board_pose(dr.BOARD_COLS, dr.BOARD_ROWS, dr.BOARD_SQUARE, 12.0, 10.0, 30.0, centre)
    ideal, truth = dr.render_board(dr.BOARD_W, dr.BOARD_H, cam, R, t, dr.BOARD_COLS, dr.BOARD_ROWS, dr.BOARD_SQUARE, np.uint16)
    img = _degrade(ideal, dict(RT_BOARD_PHOTO, vignette=vignette, gain=gain))
    img.setflags(write=False)
    return img, truth


def rt_grid(k):
    """Grid case k: (the degraded uint8 frame [240, 320], the true quads [6, 4, 2])."""
    return grid_frame(*RT_GRID_CASES[k])


@functools.lru_cache(maxsize=None)
def grid_frame(vignette, gain, frame):
    """tag_ref's grid frame `frame` through RT_GRID_PHOTO at the given vignetting and gain: (the uint8 frame, the true quads)."""
    import detect_ref as dr
    import tag_ref as tr
    lam, rot, tilt, axis = tr.GRID_FRAMES[frame]
    cam = dr.Camera(tr.GRID_F, (tr.GRID_W - 1) / 2.0, (tr.GRID_H - 1) / 2.0, lam)
    R, t = tr.grid_pose(tr.GRID, rot, tilt, axis, (0.002, -0.003, 0.40))
    ideal = tr.render_aprilgrid(tr.GRID_W, tr.GRID_H, cam, R, t, tr.GRID, tr.grid_family(), tr.GRID_BORDER, np.uint16)
    img = _degrade(ideal, dict(RT_GRID_PHOTO, vignette=vignette, gain=gain))
    img.setflags(write=False)
    return img, tr.true_quads(cam, R, t, tr.GRID)


def chain_board(img, refine_on=None):
    """The numpy board chain on one image: the corners [35, 2] in id order, or None.  refine_on: the image the found candidates are
    refined on (None: img)."""
    import corner_ref
    import detect_ref as dr
    from camera_intrinsic_calibration_rs_amd import api
    cand = dr.detect(img)
    r = corner_ref.refine(img if refine_on is None else refine_on, cand["xy"].astype(np.float64), dr.BOARD_HALF_WIN, 30, 1e-3)
    keep = np.asarray(r["status"]) == 0
    res = api.assemble_checkerboard(np.asarray(r["xy"])[keep], cand["hess"][keep].astype(np.float64), (dr.BOARD_COLS, dr.BOARD_ROWS), dr.BOARD_SQUARE)
    if res is None:
        return None
    return np.array([res[i] for i in range(dr.BOARD_COLS * dr.BOARD_ROWS)])


def board_error(found_xy, truth):
    """The worst corner distance under the labelling's half turn (render_ref.board_error)."""
    found_xy = np.asarray(found_xy, dtype=np.float64).reshape(-1, 2)
    return min(float(np.linalg.norm(found_xy - t, axis=1).max()) for t in (truth, truth[::-1]))


def chain_grid(img):
    import tag_ref as tr
    import tagchain_ref as tc
    return tc.chain(img, tr.GRID_D, tr.grid_family().codes, tc.opts(img.dtype, img.shape[1], img.shape[0]))


def grid_complete(res):
    return [int(t) for t in res["id"]] == list(range(6)) and not np.any(res["hamming"])


def grid_error(res, quads):
    return max(float(np.linalg.norm(res["corners"][i] - quads[int(t)], axis=1).max()) for i, t in enumerate(res["id"]))


def norm1(img, dst_dtype=np.uint8, **o):
    return normalize(img[None], dst_dtype, opts(**o))[0]


def _refine_on_original(norm_img, img, quads):
    """The tag chain on the normalised frame, its corners refined again on the original: the worst corner error."""
    import corner_ref
    import tag_ref as tr
    res = chain_grid(norm_img)
    if not grid_complete(res):
        return None
    xy = res["corners"].reshape(-1, 2)
    r = corner_ref.refine(img, xy, tr.GRID_HALF_WIN, 30, 1e-3)
    ok = np.asarray(r["status"]).reshape(-1) == 0
    xy2 = np.where(ok[:, None], np.asarray(r["xy"]).reshape(-1, 2), xy).reshape(-1, 4, 2)
    return max(float(np.linalg.norm(xy2[i] - quads[int(t)], axis=1).max()) for i, t in enumerate(res["id"])), int((~ok).sum())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import detect_ref as dr
    import tag_ref as tr
    fmt = lambda e: "None" if e is None else f"{e:.5f}"
    for k in range(len(RT_BOARD_CASES)):
        img, truth = rt_board(k)
        plain = chain_board(img)
        row = []
        for r in (16, 8, 32):
            xy = chain_board(norm1(img, radius=r))
            row.append(None if xy is None else board_error(xy, truth))
        xy16 = chain_board(norm1(img, np.uint16))
        mixed = chain_board(norm1(img), refine_on=img)
        print(f"board {k} {RT_BOARD_CASES[k]}: plain {'None' if plain is None else 'found'}; normalised r 16 {fmt(row[0])} px (recorded "
              f"{RT_NORM_BOARD_WORST[k]}), r 8 {fmt(row[1])}, r 32 {fmt(row[2])}, u16 out {fmt(None if xy16 is None else board_error(xy16, truth))}; "
              f"detect normalised, refine original {fmt(None if mixed is None else board_error(mixed, truth))}", flush=True)
    for k in range(len(RT_GRID_CASES)):
        img, quads = rt_grid(k)
        plain, res = chain_grid(img), chain_grid(norm1(img))
        print(f"grid {k} {RT_GRID_CASES[k]}: plain ids {[int(t) for t in plain['id']]}; normalised complete {grid_complete(res)}, "
              f"{fmt(grid_error(res, quads) if len(res['id']) else None)} px (recorded {RT_NORM_GRID_WORST[k]}); "
              f"detect normalised, refine original {_refine_on_original(norm1(img), img, quads)}", flush=True)
    imgs, truth = dr.board_frames()
    for k in range(len(imgs)):
        plain, normed, mixed = chain_board(imgs[k]), chain_board(norm1(imgs[k])), chain_board(norm1(imgs[k]), refine_on=imgs[k])
        print(f"clean board {k}: plain {fmt(board_error(plain, truth[k]))} px, normalised {fmt(None if normed is None else board_error(normed, truth[k]))}, "
              f"detect normalised, refine original {fmt(None if mixed is None else board_error(mixed, truth[k]))} (bound {dr.BOARD_BOUND:.5f})", flush=True)
    for k in (0, 1):
        img, quads = grid_frame(0.0, 1.0, k)
        plain, res = chain_grid(img), chain_grid(norm1(img))
        print(f"un-vignetted grid {k} (blur and noise only): plain complete {grid_complete(plain)} {fmt(grid_error(plain, quads))} px, normalised complete "
              f"{grid_complete(res)} {fmt(grid_error(res, quads))}; detect normalised, refine original {_refine_on_original(norm1(img), img, quads)}", flush=True)
    gimgs, gquads = tr.grid_frames()
    for k in (0, 1):
        plain, res = chain_grid(gimgs[k]), chain_grid(norm1(gimgs[k]))
        print(f"clean grid {k}: plain {fmt(grid_error(plain, gquads[k]))} px, normalised complete {grid_complete(res)} {fmt(grid_error(res, gquads[k]))}; "
              f"detect normalised, refine original {_refine_on_original(norm1(gimgs[k]), gimgs[k], gquads[k])}", flush=True)
