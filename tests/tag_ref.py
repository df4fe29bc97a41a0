"""The yardstick of the tag decoder: an independent numpy f64 restatement of the rule that include/ccal.h states at
ccal_decode_tags_batch, written from that text step by step (whole-array arithmetic over the n x n cells, plain Python ints for
codes: no lanes, no ballots, no packed keys), a seeded generator of tag families, the renderer of the AprilGrid fixture and the
cases the GPU parity tests run - shared with the CPU test that holds every one of them to the margin condition.
numpy rounds every product and sum on its own (no fused multiply-add), and so does the library's tag unit.
It depends on no GPU, on no oracle and on nothing outside this repository."""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ref  # noqa: E402

OK, OUTSIDE, LOW_CONTRAST, BORDER, NO_CODE = range(5)
REASONS = ("OK", "OUTSIDE", "LOW_CONTRAST", "BORDER", "NO_CODE")
MARGIN_FLOOR = 0.5          # grey levels: every quad of a parity fixture is at least this far from its threshold, or OUTSIDE


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def quad_map(quad):
    """Step 1: the coefficients (a, b, c, d_, e, f, g, h) of the map of the unit square onto the quad, np.float64 scalars."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(np.float64(p[0]), np.float64(p[1])) for p in np.asarray(quad, dtype=np.float64).reshape(4, 2)]
    with np.errstate(all="ignore"):
        sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
        d1x, d1y, d2x, d2y = x1 - x2, y1 - y2, x3 - x2, y3 - y2
        den = d1x * d2y - d2x * d1y
        g = (sx * d2y - d2x * sy) / den
        h = (d1x * sy - sx * d1y) / den
        a, b, c = x1 - x0 + g * x1, x3 - x0 + h * x3, x0
        d_, e, f = y1 - y0 + g * y1, y3 - y0 + h * y3, y0
    return a, b, c, d_, e, f, g, h


def map_point(coef, u, v):
    """(x, y, w) of the unit-square point (u, v); arrays broadcast."""
    a, b, c, d_, e, f, g, h = coef
    with np.errstate(all="ignore"):
        w = g * u + h * v + 1.0
        return (a * u + b * v + c) / w, (d_ * u + e * v + f) / w, w


def bilinear(img, x, y):
    """The header's I(x, y), in differences, over arrays of points that lie in the image."""
    H, W = img.shape
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    im = img.astype(np.float64)
    p00, p01, p10, p11 = im[y0, x0], im[y0, x1], im[y1, x0], im[y1, x1]
    top, bot = p00 + ax * (p01 - p00), p10 + ax * (p11 - p10)
    return top + ay * (bot - top)


def popcount(x):
    return bin(int(x)).count("1")


def bits_to_code(B):
    """Step 6 on a d x d 0 / 1 array."""
    d = len(B)
    return sum(int(B[r][c]) << (d * d - 1 - (r * d + c)) for r in range(d) for c in range(d))


def code_to_bits(code, d):
    return np.array([[(int(code) >> (d * d - 1 - (r * d + c))) & 1 for c in range(d)] for r in range(d)], dtype=np.int64)


def turn(B):
    """Step 7: T(B)(r, c) = B(d - 1 - c, r), one quarter turn clockwise."""
    d = len(B)
    return np.array([[B[d - 1 - c][r] for c in range(d)] for r in range(d)], dtype=np.int64)


def turn_code(code, d, k=1):
    B = code_to_bits(code, d)
    for _ in range(k % 4):
        B = turn(B)
    return bits_to_code(B)


def cell_values(img, quad, n, samples):
    """Steps 2 and 3: the n x n cell means [row j][col i], or None when a sample point is not inside."""
    img = np.asarray(img)
    H, W = img.shape
    coef = quad_map(quad)
    S = int(samples)
    ii, jj = np.arange(n, dtype=np.float64)[None, :], np.arange(n, dtype=np.float64)[:, None]
    acc = np.zeros((n, n))
    for q in range(S):
        v = (jj + (2 * q + 1) / (2 * S)) / n
        for p in range(S):
            u = (ii + (2 * p + 1) / (2 * S)) / n
            x, y, w = map_point(coef, u, v)
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(w) & (w > 0.0) & (x >= 0.0) & (x <= W - 1) & (y >= 0.0) & (y <= H - 1)
            if not ok.all():
                return None
            acc = acc + bilinear(img, x, y)
    return acc / (S * S)


def decode_one(img, quad, d, border, codes, samples, min_contrast, max_border_errors, max_hamming):
    """One quad by the header's steps: {"reason", "id", "rot", "hamming", "corners" [4][2], "code", "margin"}."""
    quad = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    out = {"reason": OUTSIDE, "id": -1, "rot": -1, "hamming": -1, "corners": np.full((4, 2), np.nan), "code": 0, "margin": np.nan}
    n = d + 2 * border
    val = cell_values(img, quad, n, samples)
    if val is None:
        return out
    lo, hi = val.min(), val.max()
    t = lo + (hi - lo) / 2.0
    out["margin"] = float(np.abs(val - t).min())
    if not (hi - lo >= min_contrast):
        return dict(out, reason=LOW_CONTRAST)
    white = (val > t).astype(np.int64)
    B = white[border:border + d, border:border + d]
    out["code"] = bits_to_code(B)
    if int(white.sum() - B.sum()) > max_border_errors:
        return dict(out, reason=BORDER)
    code_k, Bk = [], B
    for _ in range(4):
        code_k.append(bits_to_code(Bk))
        Bk = turn(Bk)
    best = min((popcount(code_k[k] ^ int(codes[m])), m, k) for m in range(len(codes)) for k in range(4))
    if best[0] > max_hamming:
        return dict(out, reason=NO_CODE)
    rot = best[2]
    return dict(out, reason=OK, id=best[1], rot=rot, hamming=best[0], corners=np.array([quad[(i + 3 * rot) % 4] for i in range(4)]))


# ---- families ---------------------------------------------------------------------------------------------------------------------
Family = collections.namedtuple("Family", "bits codes")


def _popcounts(arr):
    return np.unpackbits(np.ascontiguousarray(arr, dtype="<u8").view(np.uint8)).reshape(len(arr), 64).sum(axis=1)


@functools.lru_cache(maxsize=None)
def make_family(d, n_codes, min_dist, seed):
    """n_codes codes of d * d bits, drawn from a seeded generator and accepted greedily: a code is at Hamming distance >= min_dist
    from every turn of every code accepted before it and from its own three non-trivial turns.  A tuple of Python ints."""
    rng = np.random.default_rng(seed)
    dd = d * d
    codes, turns = [], np.zeros(0, dtype=np.uint64)
    for _ in range(200000):
        if len(codes) == n_codes:
            return tuple(codes)
        c = int(rng.integers(0, 1 << 63, dtype=np.uint64)) << 1 | int(rng.integers(0, 2))
        c &= (1 << dd) - 1
        own = [turn_code(c, d, k) for k in range(4)]
        if any(popcount(c ^ own[k]) < min_dist for k in (1, 2, 3)):
            continue
        if len(turns) and int(_popcounts(turns ^ np.uint64(c)).min()) < min_dist:
            continue
        codes.append(c)
        turns = np.concatenate([turns, np.array(own, dtype=np.uint64)])
    raise RuntimeError("make_family: no family of that size at that distance")


def symmetric_code(d, seed):
    """A code that equals all of its turns: a random pattern OR-ed with its three turns."""
    rng = np.random.default_rng(seed)
    B = (rng.random((d, d)) < 0.25).astype(np.int64)
    S = B.copy()
    for _ in range(3):
        B = turn(B)
        S |= B
    return bits_to_code(S)


# ---- painted tags: whole pixels per cell, so that a cell's samples all read the same grey level -----------------------------------------
def paint_tag(img, x0, y0, cell, code, d, border, black, white, turns=0, flips=(), white_border_cells=()):
    """A tag of n = d + 2 border cells of cell x cell pixels with its top-left pixel at (x0, y0), shown turned COUNTER-clockwise by
    `turns` quarter turns - `turns` clockwise turns of what is shown give the code back, so a quad that starts at the shown top-left
    decodes with rot = turns; flips: data bit numbers (0 = the first cell) inverted; white_border_cells: (j, i) border cells painted white.
    Pixels outside the image are left out.  Returns the outer quad [4][2] in the rule's order, starting at the SHOWN top-left: the
    tag's edge runs half a pixel outside its outermost pixel centres."""
    n = d + 2 * border
    B = code_to_bits(code, d)
    for b in flips:
        B[b // d][b % d] ^= 1
    for _ in range((-turns) % 4):
        B = turn(B)
    cells = np.zeros((n, n), dtype=np.int64)
    cells[border:border + d, border:border + d] = B
    for j, i in white_border_cells:
        cells[j][i] = 1
    H, W = img.shape
    for j in range(n):
        for i in range(n):
            ya, yb = max(y0 + j * cell, 0), min(y0 + (j + 1) * cell, H)
            xa, xb = max(x0 + i * cell, 0), min(x0 + (i + 1) * cell, W)
            if ya < yb and xa < xb:
                img[ya:yb, xa:xb] = white if cells[j][i] else black
    s = n * cell
    return np.array([[x0 - 0.5, y0 - 0.5], [x0 - 0.5 + s, y0 - 0.5], [x0 - 0.5 + s, y0 - 0.5 + s], [x0 - 0.5, y0 - 0.5 + s]])


# ---- the AprilGrid fixture ----------------------------------------------------------------------------------------------------------
class Board:
    """The reference's BoardConfig as plain numbers (f64 here: the renderer's geometry, not the library's f32 board points)."""

    def __init__(self, tag_size_meter, tag_spacing, tag_rows, tag_cols, first_id=0):
        self.tag_size_meter, self.tag_spacing = float(tag_size_meter), float(tag_spacing)
        self.tag_rows, self.tag_cols, self.first_id = int(tag_rows), int(tag_cols), int(first_id)


def grid_pose(board, rot_deg, tilt_deg, tilt_axis_deg, centre_xyz):
    """Board -> camera for a camera that looks at the PRINTED side: the board's x goes right, its y up and its z towards the
    viewer, so a half turn about x comes first; then detect_ref.board_pose's in-plane rotation and tilt; the grid's middle goes
    to centre_xyz."""
    R0, centre = detect_ref.board_pose(1, 1, 0.0, rot_deg, tilt_deg, tilt_axis_deg, centre_xyz)
    R = R0 @ np.diag([1.0, -1.0, -1.0])
    s, pitch = board.tag_size_meter, board.tag_size_meter * (1.0 + board.tag_spacing)
    mid = np.array([((board.tag_cols - 1) * pitch + s) / 2.0, -((board.tag_rows - 1) * pitch + s) / 2.0, 0.0])
    return R, centre - R @ mid


def render_aprilgrid(width, height, cam, R, t, board, family, border, dtype=np.uint8, black=40.0, white=215.0, ss=4):
    """The AprilGrid seen by `cam` at pose (R, t): every pixel the mean of ss x ss rays.  Per ray: the point (X, Y) of the plane
    z = 0, the tag (r, c) it falls in, u = (X - start_x) / size, v = (start_y - Y) / size, the cell, black or white.  Outside the
    tags everything is white but the black squares of side spacing * size at the tag corners.  Tag (r, c) shows the code of id
    first_id + r * tag_cols + c of `family` (anything with .bits and .codes: Family below, api.TagFamily)."""
    d = int(round(family.bits ** 0.5))
    n = d + 2 * border
    size, pitch = board.tag_size_meter, board.tag_size_meter * (1.0 + board.tag_spacing)
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    px = (np.arange(width, dtype=np.float64)[:, None] + sub[None, :]).reshape(-1)
    py = (np.arange(height, dtype=np.float64)[:, None] + sub[None, :]).reshape(-1)
    ray = cam.rays(px[None, :], py[:, None])
    dn, tn = ray @ R, R.T @ t
    cells = np.zeros((board.tag_rows, board.tag_cols, n, n), dtype=bool)
    for r in range(board.tag_rows):
        for c in range(board.tag_cols):
            cells[r, c, border:border + d, border:border + d] = code_to_bits(family.codes[board.first_id + r * board.tag_cols + c], d) == 1
    with np.errstate(divide="ignore", invalid="ignore"):
        k = tn[2] / dn[..., 2]
        X, Y = k * dn[..., 0] - tn[0], -(k * dn[..., 1] - tn[1])            # Y counted downwards from the first row's top edge
        c, r = np.floor(X / pitch), np.floor(Y / pitch)
        u, v = (X - c * pitch) / size, (Y - r * pitch) / size
    front = np.isfinite(k) & (k > 0)
    in_c, in_r = front & (c >= 0) & (c < board.tag_cols), front & (r >= 0) & (r < board.tag_rows)
    tag = in_c & in_r & (u < 1.0) & (v < 1.0)
    gap = front & (u >= 1.0) & (v >= 1.0) & (c >= -1) & (c < board.tag_cols) & (r >= -1) & (r < board.tag_rows)
    ci = np.clip(c, 0, board.tag_cols - 1).astype(np.int64); ri = np.clip(r, 0, board.tag_rows - 1).astype(np.int64)
    cu = np.clip(np.floor(np.where(tag, u, 0.0) * n), 0, n - 1).astype(np.int64)
    cv = np.clip(np.floor(np.where(tag, v, 0.0) * n), 0, n - 1).astype(np.int64)
    is_white = np.where(tag, cells[ri, ci, cv, cu], ~gap)
    lum = np.where(is_white, white, black).reshape(height, ss, width, ss).mean(axis=(1, 3))
    if dtype == np.uint16:
        return np.rint(lum * 257.0).astype(np.uint16)
    return np.rint(lum).astype(np.uint8)


def true_quads(cam, R, t, board):
    """The projected outer corners of every tag in the rule's order - (x, y), (x + s, y), (x + s, y - s), (x, y - s) of the
    board, which the camera sees as top-left, top-right, bottom-right, bottom-left: [tag_rows * tag_cols][4][2], row by row."""
    s, pitch = board.tag_size_meter, board.tag_size_meter * (1.0 + board.tag_spacing)
    P = []
    for r in range(board.tag_rows):
        for c in range(board.tag_cols):
            x, y = c * pitch, -r * pitch
            P += [(x, y, 0.0), (x + s, y, 0.0), (x + s, y - s, 0.0), (x, y - s, 0.0)]
    return cam.project(np.array(P) @ R.T + t).reshape(-1, 4, 2)


# The end-to-end fixture: a 3 x 2 AprilGrid (3 columns, 2 rows) of 30 mm tags, d = 6, one border cell, in 320 x 240 images at
# f = 600 px and 0.40 m: a tag is about 45 px wide, a cell 5.6 px.  Per frame: (lam of the division model, in-plane rotation, tilt,
# tilt axis - degrees).
GRID = Board(0.03, 0.3, 2, 3)
GRID_D, GRID_BORDER, GRID_W, GRID_H, GRID_F = 6, 1, 320, 240, 600.0
# The refinement window of the end-to-end test: half_win 4 - the 9 x 9 window around a tag's outer corner then holds the black
# border cell (5.6 px) and the black gap square diagonally across, and keeps the data cells beyond the border cell at its rim.
GRID_HALF_WIN = 4
GRID_FRAMES = ((0.0, 15.0, 10.0, 30.0), (-0.35, 100.0, 30.0, 80.0), (-0.35, 15.0, 30.0, -20.0), (0.0, 100.0, 10.0, 60.0))


def grid_family():
    return Family(36, make_family(6, 40, 10, 11))


@functools.lru_cache(maxsize=None)
def grid_frames(dtype=np.uint8):
    """(images [4][240][320], true quads [4][6][4][2])."""
    imgs, quads = [], []
    for lam, rot, tilt, axis in GRID_FRAMES:
        cam = detect_ref.Camera(GRID_F, (GRID_W - 1) / 2.0, (GRID_H - 1) / 2.0, lam)
        R, t = grid_pose(GRID, rot, tilt, axis, (0.002, -0.003, 0.40))
        imgs.append(render_aprilgrid(GRID_W, GRID_H, cam, R, t, GRID, grid_family(), GRID_BORDER, dtype))
        quads.append(true_quads(cam, R, t, GRID))
    out = np.stack(imgs), np.stack(quads)
    out[0].setflags(write=False); out[1].setflags(write=False)
    return out


# ---- the cases of the GPU parity tests ----------------------------------------------------------------------------------------------
def _grey(dtype, level):
    return int(level) * (257 if np.dtype(dtype) == np.uint16 else 1)


def _case(name, images, quads_list, d, border, codes, samples=3, min_contrast=20.0, max_border_errors=0, max_hamming=2):
    return {"name": name, "images": np.ascontiguousarray(images), "quads_list": [np.asarray(q, dtype=np.float64).reshape(-1, 4, 2) for q in quads_list],
            "d": d, "border": border, "codes": tuple(int(c) for c in codes), "samples": samples, "min_contrast": float(min_contrast),
            "max_border_errors": max_border_errors, "max_hamming": max_hamming}


def _painted_sheet(d, border, codes, dtype, seed, cell=6, black=40, white=215):
    """One image of painted tags - code k % len(codes) shown at turn k % 4, every third one with a flipped data bit - and per tag
    two quads: the exact outline, and the outline with every corner moved by up to 0.4 px (a general projective map)."""
    rng = np.random.default_rng(seed)
    n = d + 2 * border
    side, gap = n * cell, 8
    per_row, rows = (320 - gap) // (side + gap), (240 - gap) // (side + gap)
    img = np.full((240, 320), _grey(dtype, white), dtype=dtype)
    quads = []
    for k in range(per_row * rows):
        x0, y0 = gap + (k % per_row) * (side + gap), gap + (k // per_row) * (side + gap)
        q = paint_tag(img, x0, y0, cell, codes[k % len(codes)], d, border, _grey(dtype, black), _grey(dtype, white), turns=k % 4,
                      flips=(int(rng.integers(0, d * d)),) if k % 3 == 2 else ())
        quads += [q, q + rng.uniform(-0.4, 0.4, (4, 2)), np.roll(q, -(k % 3), axis=0)]
    return img, np.array(quads)


SHEET_SHAPES = ((6, 1, 64), (6, 2, 100), (8, 2, 144), (3, 1, 25), (8, 1, 100))       # (d, border, cells): 1, 2, 3 chunks, idle lanes, 64 bits


def small_family(d):
    return {3: lambda: make_family(3, 3, 3, 5), 6: lambda: make_family(6, 8, 10, 6), 8: lambda: make_family(8, 8, 20, 8)}[d]()


@functools.lru_cache(maxsize=None)
def sheet_cases():
    out = []
    for d, border, _ in SHEET_SHAPES:
        for samples in (1, 4):
            for dtype in (np.uint8, np.uint16):
                img, quads = _painted_sheet(d, border, small_family(d), dtype, 100 * d + border)
                out.append(_case(f"sheet d {d} border {border} S {samples} {np.dtype(dtype).name}", img[None], [quads], d, border,
                                 small_family(d), samples, 20.0, 0, 1 if d > 3 else 0))
    return out


TABLE_SIZES = (1, 63, 64, 65, 587)


def big_family():
    return make_family(6, 587, 8, 3)


@functools.lru_cache(maxsize=None)
def table_cases():
    """The matching code first, last and at index 64 of tables of 1 .. 587 codes (strides of the lanes and of the staged chunks);
    each tag carries one flipped bit, and a fourth tag shows a code that is not in the table at all."""
    out = []
    for n_codes in TABLE_SIZES:
        codes = big_family()[:n_codes]
        img = np.full((80, 320), 215, dtype=np.uint8)
        want = [0, n_codes - 1, min(64, n_codes - 1)]
        quads = [paint_tag(img, 8 + 60 * i, 8, 6, codes[m], 6, 1, 40, 215, turns=i + 1, flips=(7 * i + 3,)) for i, m in enumerate(want)]
        # five flipped bits: 5 from its own code and, the family's distance being 8, at least 3 from every other - NO_CODE at 2
        quads.append(paint_tag(img, 8 + 60 * 3, 8, 6, codes[min(300, n_codes - 1)] ^ 0x2A5, 6, 1, 40, 215))
        out.append(dict(_case(f"table of {n_codes}", img[None], [np.array(quads)], 6, 1, codes, 3, 20.0, 0, 2), want=want))
    return out


@functools.lru_cache(maxsize=None)
def bounds_case():
    """d 6, border 1, S 1 on a 64 x 100 image: the quad (-4, 39) .. (60, 103) has cells of 8 px whose centres - the sample points -
    are the pixels (8 i, 43 + 8 j): column 0 at x = 0 and row 7 at y = 99 = height - 1 exactly, all in exact arithmetic (the quad
    is a square, g = h = 0).  Then the same quad 1e-9 to the left, 1e-9 down, and - inside again - 1e-9 right and up."""
    code = small_family(6)[2]
    img = np.full((100, 64), 215, dtype=np.uint8)
    paint_tag(img, -4 + 1, 39 + 1, 8, code, 6, 1, 40, 215)        # the pixels 8 i - 3 .. 8 i + 4 of column i: the sample pixel among them
    q = np.array([[-4.0, 39.0], [60.0, 39.0], [60.0, 103.0], [-4.0, 103.0]])
    quads = [q, q + [-1e-9, 0.0], q + [0.0, 1e-9], q + [1e-9, -1e-9]]
    return dict(_case("image bounds", img[None], [np.array(quads)], 6, 1, small_family(6), 1, 20.0, 0, 0),
                want_reasons=[OK, OUTSIDE, OUTSIDE, OK])


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """Quads that are no quads, over a painted tag: repeated corners (q2 = q1, which makes den 0, and all four equal), three
    collinear corners (q1 on the diagonal q0 q2, at 0.4 of it: a valid map of a triangle, which the border test rejects), a crossed
    quad, a NaN corner, an Inf corner.  The yardstick decides each; the repeated, NaN and Inf ones are OUTSIDE by the rule.
    (q1 = q0 is left out on purpose: its map sends the whole square to q0, every cell reads the same point, and the margin is
    rounding noise - against the margin condition of the fixtures.)"""
    code = small_family(6)[1]
    img = np.full((80, 80), 215, dtype=np.uint8)
    q = paint_tag(img, 16, 16, 6, code, 6, 1, 40, 215)
    two = q.copy(); two[2] = two[1]
    point = np.repeat(q[:1], 4, axis=0)
    line = q.copy(); line[1] = q[0] + (q[2] - q[0]) * 0.4
    crossed = q[[0, 2, 1, 3]]
    nan = q.copy(); nan[2, 0] = np.nan
    inf = q.copy(); inf[3, 1] = np.inf
    ninf = q.copy(); ninf[0, 0] = -np.inf
    return dict(_case("degenerate corners", img[None], [np.array([q, two, point, line, crossed, nan, inf, ninf])], 6, 1, small_family(6), 3,
                      20.0, 0, 2), must_be_outside=[1, 2, 5, 6, 7])


@functools.lru_cache(maxsize=None)
def threshold_cases():
    """Contrast 21 grey levels against min_contrast 20 (just above) and 60 (well below); one white border cell against
    max_border_errors 1 (equal) and 0 (one more)."""
    codes = small_family(6)
    low = np.full((64, 64), 121, dtype=np.uint8)
    q_low = paint_tag(low, 8, 8, 6, codes[3], 6, 1, 100, 121)
    nick = np.full((64, 64), 215, dtype=np.uint8)
    q_nick = paint_tag(nick, 8, 8, 6, codes[4], 6, 1, 40, 215, white_border_cells=((0, 3),))
    return [dict(_case("contrast 21 >= 20", low[None], [q_low[None]], 6, 1, codes, 3, 20.0, 0, 0), want_reasons=[OK]),
            dict(_case("contrast 21 < 60", low[None], [q_low[None]], 6, 1, codes, 3, 60.0, 0, 0), want_reasons=[LOW_CONTRAST]),
            dict(_case("border errors 1 <= 1", nick[None], [q_nick[None]], 6, 1, codes, 3, 20.0, 1, 0), want_reasons=[OK]),
            dict(_case("border errors 1 > 0", nick[None], [q_nick[None]], 6, 1, codes, 3, 20.0, 0, 0), want_reasons=[BORDER])]


@functools.lru_cache(maxsize=None)
def tie_cases():
    """Two equal codes: the smaller m.  A code equal to all its turns: k = 0."""
    c = small_family(6)[5]
    img = np.full((64, 64), 215, dtype=np.uint8)
    q = paint_tag(img, 8, 8, 6, c, 6, 1, 40, 215, turns=2)
    sym = symmetric_code(6, 4)
    img2 = np.full((64, 64), 215, dtype=np.uint8)
    q2 = paint_tag(img2, 8, 8, 6, sym, 6, 1, 40, 215, flips=(9,))
    return [dict(_case("equal codes", img[None], [q[None]], 6, 1, (small_family(6)[0], c, c), 3, 20.0, 0, 0), want=(1, 2, 0)),
            dict(_case("symmetric code", img2[None], [q2[None]], 6, 1, (sym,), 3, 20.0, 0, 1), want=(0, 0, 1))]


@functools.lru_cache(maxsize=None)
def batch_case():
    """Three images: a sheet with its quads, an image without quads, and a sheet whose quads are repeated until the quad of the
    one-image call below is quad 130 of image 2."""
    codes = small_family(6)
    a, qa = _painted_sheet(6, 1, codes, np.uint8, 41)
    b, qb = _painted_sheet(6, 1, codes, np.uint8, 42)
    reps = np.concatenate([qb] * (131 // len(qb) + 1))[:140]
    return _case("three images", np.stack([a, np.full_like(a, 9), b]), [qa, np.zeros((0, 4, 2)), reps], 6, 1, codes, 3, 20.0, 0, 1)


# tests/test_gpu_tags.py::test_a_batch_cut_into_chunks on batch_case() (three 76 800-byte images with 60, 0 and 140 quads): the chunk
# limits for the host call (pixels count) and the _dev call (they do not) - 1 byte: an image per chunk; the second: the images (0, 1)
# and (2) - the first two together, the third alone.  tests/test_quads_plan_cpu.py holds the library's planner to exactly these groupings.
CHUNK_LIMITS_HOST, CHUNK_LIMITS_DEV, CHUNK_GROUPS = (1, 200000), (1, 20000), (0, 2, 3)


@functools.lru_cache(maxsize=None)
def rendered_cases():
    """The end-to-end frames with their true quads moved by up to 0.3 px per coordinate: general projective maps over antialiased,
    distorted tags."""
    out = []
    for dtype in (np.uint8, np.uint16):
        imgs, quads = grid_frames(dtype)
        rng = np.random.default_rng(77)
        moved = [q + rng.uniform(-0.3, 0.3, q.shape) for q in quads]
        for samples in (1, 3):
            out.append(_case(f"rendered grid S {samples} {np.dtype(dtype).name}", imgs, moved, GRID_D, GRID_BORDER, grid_family().codes, samples,
                             20.0 * (257 if dtype == np.uint16 else 1), 0, 2))
    return out


def parity_cases():
    """Every case the GPU parity tests compare quad by quad with decode_one."""
    return (sheet_cases() + table_cases() + [bounds_case(), degenerate_case()] + threshold_cases() + tie_cases() + [batch_case()]
            + rendered_cases())


_YARD = {}


def yardstick(case):
    """decode_one over every quad of a case, per image: computed once per case and shared."""
    if case["name"] not in _YARD:
        _YARD[case["name"]] = [[decode_one(case["images"][k], q, case["d"], case["border"], case["codes"], case["samples"], case["min_contrast"],
                                           case["max_border_errors"], case["max_hamming"]) for q in quads]
                               for k, quads in enumerate(case["quads_list"])]
    return _YARD[case["name"]]
