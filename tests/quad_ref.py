"""The yardstick of the quad proposer: an independent numpy f64 restatement of the rule that include/ccal.h states at
ccal_propose_quads_batch, written from that text step by step (whole-array arithmetic over all point pairs, Python lists and loops
for the out-edge lists and the chains: no lanes, no ballots, no scans), and the cases the GPU parity tests run.
numpy rounds every product and sum on its own (no fused multiply-add), and so does the library's quad unit.

Every case builder holds its case to the margin condition on the CPU (check_margins): every pair that passes the length and
inside tests has |bright - dark - min_contrast| >= 1e-3 grey levels, and every comparison of a cross product, of a side limit and
of the side ratio is at least 1e-6 relative from equality - so no decision rides on the last bits of a sum.
It depends on no GPU, on no oracle and on nothing outside this repository."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_ref  # noqa: E402
import detect_ref  # noqa: E402
import tag_ref  # noqa: E402

MAX_OUT_EDGES = 8           # CCAL_QUAD_MAX_OUT_EDGES
FLAG_CUT = 1                # bit 0 of flags: an out-edge list of the image was cut
EDGE_MARGIN = 1e-3          # grey levels
REL_MARGIN = 1e-6
DEFAULTS = dict(min_side=20.0, max_side=120.0, max_side_ratio=2.0, offset=1.0 / 16.0, samples=8, min_contrast=40.0, cap=1024)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    """|a - b| relative to the larger magnitude (1 when both are 0 and equal: nothing can move them)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = np.maximum(np.abs(a), np.abs(b))
        return np.where(m > 0, np.abs(a - b) / np.where(m > 0, m, 1.0), 1.0)


def edges(img, xy, min_side, max_side, offset, samples, min_contrast):
    """Step 1 over all ordered pairs: (edge [n][n] bool with edge[A][B] = "A -> B is an edge", the smallest
    |bright - dark - min_contrast| over the pairs that pass the length and inside tests, the smallest relative distance of an
    L2 from a side limit over all pairs A != B with a finite L2); inf where there is no such pair."""
    img = np.asarray(img)
    H, W = img.shape
    P = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n, K = len(P), int(samples)
    edge = np.zeros((n, n), dtype=bool)
    if n < 2:
        return edge, np.inf, np.inf
    min_side, max_side, offset, min_contrast = np.float64(min_side), np.float64(max_side), np.float64(offset), np.float64(min_contrast)
    with np.errstate(all="ignore"):
        ex, ey = P[None, :, 0] - P[:, None, 0], P[None, :, 1] - P[:, None, 1]              # e[A][B] = B - A
        L2 = ex * ex + ey * ey
        lo, hi = min_side * min_side, max_side * max_side
        ok = (L2 >= lo) & (L2 <= hi)
    np.fill_diagonal(ok, False)
    off_diag = ~np.eye(n, dtype=bool) & np.isfinite(L2)
    side_margin = float(min(_rel(L2[off_diag], lo).min(), _rel(L2[off_diag], hi).min())) if off_diag.any() else np.inf
    A, B = np.nonzero(ok)
    if not len(A):
        return edge, np.inf, side_margin
    ax, ay, ex, ey = P[A, 0], P[A, 1], ex[A, B], ey[A, B]
    nx, ny = -offset * ey, offset * ex
    dark, bright = np.full(len(A), -np.inf), np.full(len(A), np.inf)
    inside = np.ones(len(A), dtype=bool)
    for k in range(K):
        t = np.float64(k + 1) / np.float64(K + 1)
        px, py = ax + t * ex, ay + t * ey
        for sign in (1, -1):
            x, y = (px + nx, py + ny) if sign > 0 else (px - nx, py - ny)
            with np.errstate(invalid="ignore"):
                here = (x >= 0.0) & (x <= W - 1) & (y >= 0.0) & (y <= H - 1)
            inside &= here
            v = tag_ref.bilinear(img, np.where(here, x, 0.0), np.where(here, y, 0.0))
            if sign > 0:
                dark = np.maximum(dark, v)
            else:
                bright = np.minimum(bright, v)
    contrast = bright - dark
    is_edge = inside & (contrast >= min_contrast)
    edge[A[is_edge], B[is_edge]] = True
    margin = float(np.abs(contrast[inside] - min_contrast).min()) if inside.any() else np.inf
    return edge, margin, side_margin


def _cross(e1, e2):
    return e1[0] * e2[1] - e1[1] * e2[0]


def propose(img, xy, min_side=20.0, max_side=120.0, max_side_ratio=2.0, offset=1.0 / 16.0, samples=8, min_contrast=40.0, cap=1024):
    """One image (any integer dtype, [H][W]) and its points [n, 2]: {"count", "idx" int32 [m, 4], "quads" f64 [m, 4, 2] with
    m = min(count, cap), "flags", "deg" (the full out-degrees), "edge_margin", "rel_margin"}."""
    P = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(P)
    edge, edge_margin, rel_margin = edges(img, P, min_side, max_side, offset, samples, min_contrast)
    # step 2: the out-edge lists in increasing index order, cut to the first MAX_OUT_EDGES
    full = [np.flatnonzero(edge[a]).tolist() for a in range(n)]
    out = [lst[:MAX_OUT_EDGES] for lst in full]
    flags = FLAG_CUT if any(len(lst) > MAX_OUT_EDGES for lst in full) else 0
    # step 3
    ratio2 = np.float64(max_side_ratio) * np.float64(max_side_ratio)
    found = []
    for a in range(n):
        for b in out[a]:
            for c in out[b]:
                for d in out[c]:
                    if a not in out[d] or len({a, b, c, d}) != 4 or a != min(a, b, c, d):
                        continue
                    q = P[[a, b, c, d]]
                    e = [q[(i + 1) % 4] - q[i] for i in range(4)]
                    cr = [_cross(e[i], e[(i + 1) % 4]) for i in range(4)]
                    for i in range(4):
                        rel_margin = min(rel_margin, float(_rel(e[i][0] * e[(i + 1) % 4][1], e[i][1] * e[(i + 1) % 4][0])))
                    if not all(x > 0.0 for x in cr):
                        continue
                    s2 = [v[0] * v[0] + v[1] * v[1] for v in e]
                    rel_margin = min(rel_margin, float(_rel(max(s2), ratio2 * min(s2))))
                    if max(s2) <= ratio2 * min(s2):
                        found.append((a, b, c, d))
    found.sort()
    m = min(len(found), int(cap))
    idx = np.array(found[:m], dtype=np.int32).reshape(m, 4)
    return {"count": len(found), "idx": idx, "quads": P[idx.reshape(-1)].reshape(m, 4, 2), "flags": flags,
            "deg": np.array([len(lst) for lst in full], dtype=np.int32), "edge_margin": edge_margin, "rel_margin": rel_margin}


def merge_points(xy, radius=1.0):
    """What api.propose_quads does first: a point within `radius` px, in both coordinates, of an earlier kept point is dropped."""
    kept = []
    for p in np.asarray(xy, dtype=np.float64).reshape(-1, 2):
        if not any(abs(p[0] - q[0]) <= radius and abs(p[1] - q[1]) <= radius for q in kept):
            kept.append(p)
    return np.array(kept, dtype=np.float64).reshape(-1, 2)


def same_outline(q, truth, tol):
    """q [4][2] equals truth [4][2] up to a cyclic shift, every corner within tol px."""
    return any(np.linalg.norm(np.roll(q, -s, axis=0) - truth, axis=1).max() <= tol for s in range(4))


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _case(name, images, xy_list, **params):
    p = dict(DEFAULTS)
    p.update(params)
    case = dict(p, name=name, images=np.ascontiguousarray(images), xy_list=[np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in xy_list])
    assert len(case["images"]) == len(case["xy_list"])
    check_margins(case)
    return case


_YARD = {}


def yardstick(case):
    """propose() over every image of a case: computed once per case and shared."""
    if case["name"] not in _YARD:
        _YARD[case["name"]] = [propose(case["images"][k], xy, case["min_side"], case["max_side"], case["max_side_ratio"], case["offset"],
                                       case["samples"], case["min_contrast"], case["cap"]) for k, xy in enumerate(case["xy_list"])]
    return _YARD[case["name"]]


def check_margins(case):
    for k, r in enumerate(yardstick(case)):
        assert r["edge_margin"] >= EDGE_MARGIN, (case["name"], k, r["edge_margin"])
        assert r["rel_margin"] >= REL_MARGIN, (case["name"], k, r["rel_margin"])


def _scale(dtype):
    return 257 if np.dtype(dtype) == np.uint16 else 1


@functools.lru_cache(maxsize=None)
def fixture_points(dtype=np.uint8, nms_radius=5):
    """The end-to-end fixture (tag_ref.grid_frames) through the CPU chain in front of the proposer: detect_ref.detect at the given
    nms_radius, corner_ref.refine at half_win 4 keeping status OK, rounded through f32 as a FeaturePoint is, merged.  Per frame
    (refined [n, 2] with its duplicates, merged [m, 2])."""
    imgs, _ = tag_ref.grid_frames(dtype)
    out = []
    for img in imgs:
        cand = detect_ref.detect(img, 1, nms_radius, 1, 102, 4096)["xy"].astype(np.float64)
        r = corner_ref.refine(img, cand, tag_ref.GRID_HALF_WIN, 30, 1e-3)
        xy = np.float32(r["xy"][r["status"] == 0]).astype(np.float64)
        out.append((xy, merge_points(xy)))
    return tuple(out)


def fixture_params(dtype, **change):
    return dict(dict(max_side=max(tag_ref.GRID_W, tag_ref.GRID_H) / 2.0, min_contrast=40.0 * _scale(dtype)), **change)


def _fixture_name(dtype, min_side):
    return f"fixture {np.dtype(dtype).name} min_side {min_side:g}"


@functools.lru_cache(maxsize=None)
def fixture_case(dtype=np.uint8, min_side=20.0):
    imgs, _ = tag_ref.grid_frames(dtype)
    return _case(_fixture_name(dtype, min_side), imgs, [m for _, m in fixture_points(dtype)], **fixture_params(dtype, min_side=min_side))


def painted(width, height, cell, n_points, seed, dtype=np.uint8, d=6, border=1, shuffle=True, jitter=0.0):
    """An image of painted tags (tag_ref.paint_tag, cells of cell x cell pixels, 8 px apart) and n_points points: the exact outer
    corners of as many whole tags as the count allows, then seeded stray points, all in a seeded order; jitter: every corner moved by up to that many
    pixels per coordinate (off the lattice the exact corners lie on, where three of them are collinear exactly).  Returns (image,
    points, the outlines [tags][4][2] among the points)."""
    rng = np.random.default_rng(seed)
    codes = tag_ref.small_family(d)
    n = d + 2 * border
    side, gap = n * cell, 8
    per_row, rows = (width - gap) // (side + gap), (height - gap) // (side + gap)
    s = _scale(dtype)
    img = np.full((height, width), 215 * s, dtype=dtype)
    outlines = []
    for k in range(per_row * rows):
        q = tag_ref.paint_tag(img, gap + (k % per_row) * (side + gap), gap + (k // per_row) * (side + gap), cell, codes[k % len(codes)], d,
                              border, 40 * s, 215 * s, turns=k % 4)
        if 4 * (len(outlines) + 1) <= n_points:
            outlines.append(q + rng.uniform(-jitter, jitter, (4, 2)) if jitter else q)
    pts = np.concatenate([np.array(outlines).reshape(-1, 2), rng.uniform([0.0, 0.0], [width - 1.0, height - 1.0], (n_points - 4 * len(outlines), 2))])
    if shuffle:
        pts = pts[rng.permutation(len(pts))]
    return img, pts, np.array(outlines).reshape(-1, 4, 2)


SHEET_COUNTS = (0, 1, 3, 4, 63, 64, 65, 130)         # partial, full and several passes of the 64-lane stride over B
SHEET_SIZES = ((67, 45, 3), (67, 45, 3), (67, 45, 3), (67, 45, 3), (200, 160, 3), (160, 200, 3), (200, 160, 3), (200, 160, 3))


SHEET_KINDS = ((np.uint8, 8), (np.uint16, 8), (np.uint8, 1), (np.uint8, 16))          # (dtype, K)


def _sheet_name(dtype, samples, size):
    return f"sheets {size[0]} x {size[1]} K {samples} {np.dtype(dtype).name}"


@functools.lru_cache(maxsize=None)
def sheet_case(dtype, samples, size):
    """The point counts of SHEET_COUNTS that go with one image size, as the images of one call.  max_side 100: the corners lie on a
    lattice of 8 px, where 120^2 is a distance that occurs exactly.  At K = 1 and 16 the corners are jittered: one sample per edge
    accepts many chains across tags, among them exactly collinear ones on the lattice."""
    built = [painted(size[0], size[1], size[2], cnt, 1000 + 7 * cnt + samples, dtype, jitter=0.0 if samples == 8 else 0.3)
             for cnt, sz in zip(SHEET_COUNTS, SHEET_SIZES) if sz == size]
    return _case(_sheet_name(dtype, samples, size), np.stack([b[0] for b in built]), [b[1] for b in built], samples=samples,
                 max_side=100.0, min_contrast=40.0 * _scale(dtype))


def sheet_cases():
    """One case per dtype, K and image size: the eight point counts as eight images of three sizes - so three calls per kind."""
    return [parity_case(name) for name in parity_case_names() if name.startswith("sheets ")]


@functools.lru_cache(maxsize=None)
def overflow_case():
    """A straight boundary, white above and black below, with 12 points on it 8 px apart: walking in +x the dark side is to the
    right, so every point has an edge to every point ahead of it (min_side 6): out-degrees 11, 10, .. 0.  The lists are cut, and
    there is no quad: no edge leads back."""
    img = np.full((32, 100), 215, dtype=np.uint8)
    img[16:] = 40
    pts = np.array([[6.0 + 8.0 * i, 15.5] for i in range(12)])
    return _case("out-edge overflow", img[None], [pts], min_side=6.0)


@functools.lru_cache(maxsize=None)
def outside_case():
    """Two tags of 24 px in a 67 x 45 image: one whose outline runs 0.5 px from the left image border - the outer samples of its left
    side fall at x < 0, so that side is no edge and the tag no quad - and one well inside; plus a NaN and an Inf point."""
    img = np.full((45, 67), 215, dtype=np.uint8)
    code = tag_ref.small_family(6)[0]
    a = tag_ref.paint_tag(img, 1, 10, 3, code, 6, 1, 40, 215)
    b = tag_ref.paint_tag(img, 35, 10, 3, code, 6, 1, 40, 215)
    pts = np.concatenate([a, [[np.nan, 20.0]], b, [[30.0, np.inf]]])
    return _case("sample points outside", img[None], [pts])


@functools.lru_cache(maxsize=None)
def cap_case():
    img, pts, _ = painted(200, 160, 3, 65, 31)
    return _case("cap 1", img[None], [pts], max_side=100.0, cap=1)


@functools.lru_cache(maxsize=None)
def batch_case():
    """Five images of one size: sheets with 130, 0, 65 and 4 points and the 130 again in another order."""
    built = [painted(200, 160, 3, cnt, 500 + cnt) for cnt in (130, 0, 65, 4)] + [painted(200, 160, 3, 130, 501)]
    return _case("five images", np.stack([b[0] for b in built]), [b[1] for b in built], max_side=100.0)


# tests/test_gpu_quads.py::test_a_batch_cut_into_chunks on batch_case() (five 32 000-byte images with 130, 0, 65, 4, 130 points): the
# chunk limits for the host call (pixels count) and the _dev call (they do not) - 1 byte: an image per chunk; the second: the images
# (0, 1), (2, 3), (4) - a chunk of two images with points that is not the first.  tests/test_quads_plan_cpu.py holds the library's
# planner to exactly these groupings.
CHUNK_LIMITS_HOST, CHUNK_LIMITS_DEV, CHUNK_GROUPS = (1, 80000), (1, 8000), (0, 2, 4, 5)


# The cases the GPU parity tests compare with propose(): ONE table of (name, builder), in the tests' order.  Making the table builds
# no case; the names come from the same helpers the builders use.
PARITY = tuple([(_fixture_name(dtype, min_side), functools.partial(fixture_case, dtype, min_side))
                for dtype, min_side in ((np.uint8, 20.0), (np.uint16, 20.0), (np.uint8, 6.0))]
               + [(_sheet_name(dtype, samples, size), functools.partial(sheet_case, dtype, samples, size))
                  for dtype, samples in SHEET_KINDS for size in sorted(set(SHEET_SIZES))]
               + [("out-edge overflow", overflow_case), ("sample points outside", outside_case), ("cap 1", cap_case),
                  ("five images", batch_case)])


def parity_case_names():
    return [name for name, _ in PARITY]


def parity_case(name):
    case = dict(PARITY)[name]()
    assert case["name"] == name
    return case


def parity_cases():
    return [parity_case(name) for name in parity_case_names()]
