"""The yardstick of the checkerboard assembly: a numpy f64 restatement of the rule that include/ccal.h states at
ccal_assemble_checkerboards_batch, written from that text step by step (whole-array arithmetic over all candidates and candidate
pairs, a Python dict for the lattice and Python loops for its growth: no lanes, no ballots, no scans).  The rule is the method of
api.assemble_checkerboard with every operation spelled out as IEEE + - * / sqrt in a fixed order: the closed form of a 2 x 2
symmetric matrix's zero-curvature directions instead of an eigen-solver, sqrt(x x + y y) instead of a norm routine, products and
sums written one by one instead of einsum, and the stencil mean as a running sum in stencil order divided by the count.
numpy rounds every product and sum on its own (no fused multiply-add), and so does the library's board unit.
It depends on no GPU, on no oracle and on nothing outside this repository."""
import math

import numpy as np

MAX_ROWS = 4096             # CCAL_BOARD_MAX_ROWS: input rows per image
MAX_KEPT = 512              # CCAL_BOARD_MAX_KEPT: rows kept after the screen
MIN_SIDE, MAX_SIDE = 2, 20  # cols, rows
FLAG_KEPT_LIMIT = 2         # bit 1 of flags: more than MAX_KEPT rows kept - no board, nothing else written
CONE_COS = 0.9
WEAK = 0.5
REACH = 0.3
PAIRS = ((0, 1), (0, 3), (2, 1), (2, 3))
STEPS = ((1, 0), (0, 1), (-1, 0), (0, -1))
DIAGS = ((1, 1), (1, -1), (-1, 1), (-1, -1))
SETTLE_ROUNDS = 3


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def response(hess):
    h = np.asarray(hess, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return h[:, 2] * h[:, 2] - (16.0 * h[:, 0]) * h[:, 1]


def screen(xy, hess, n_want):
    """The rows kept, as input indices in the order (y, x, input index), and the number of usable rows; when fewer than n_want
    rows are usable none is kept."""
    P = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    R = response(hess)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(P[:, 0]) & np.isfinite(P[:, 1]) & (R > 0.0) & np.isfinite(R)
    usable = int(np.count_nonzero(ok))
    if usable < n_want:
        return np.zeros(0, dtype=np.int64), usable
    idx = np.flatnonzero(ok)
    # rank among the usable rows: stronger rows first, ties by input index; the row of rank n_want - 1 sets the threshold
    r = R[idx]
    rank = ((r[None, :] > r[:, None]) | ((r[None, :] == r[:, None]) & (idx[None, :] < idx[:, None]))).sum(axis=1)
    t = WEAK * r[rank == n_want - 1][0]
    keep = idx[r >= t]
    x, y = P[keep, 0], P[keep, 1]
    before = (y[None, :] < y[:, None]) | ((y[None, :] == y[:, None]) & ((x[None, :] < x[:, None]) |
                                                                       ((x[None, :] == x[:, None]) & (keep[None, :] < keep[:, None]))))
    order = np.empty(len(keep), dtype=np.int64)
    order[before.sum(axis=1)] = np.arange(len(keep))
    return keep[order], usable


def edge_directions(H):
    """d1, d2 [n, 2] each: the unit zero-curvature directions of [[hxx, b], [b, hyy]], b = hxy / 4."""
    a, c, b = H[:, 0], H[:, 1], H[:, 2] / 4.0
    with np.errstate(all="ignore"):
        m, dl = 0.5 * (a + c), 0.5 * (a - c)
        r = np.sqrt(dl * dl + b * b)
        l1, l0 = m + r, m - r
        pos = dl >= 0.0
        vx, vy = np.where(pos, dl + r, b), np.where(pos, b, r - dl)         # the eigenvector of l1, the larger component formed by a sum
        nv = np.sqrt(vx * vx + vy * vy)
        zero = ~(nv > 0.0)
        vx, vy = np.where(zero, 1.0, vx / nv), np.where(zero, 0.0, vy / nv)
        wx, wy = -vy, vx                                                     # the eigenvector of l0
        A, B = np.sqrt(np.maximum(l1, 0.0)), np.sqrt(np.maximum(-l0, 0.0))
        out = []
        for s in (1.0, -1.0):
            dx, dy = B * vx + (s * A) * wx, B * vy + (s * A) * wy
            nd = np.maximum(np.sqrt(dx * dx + dy * dy), 1e-300)
            out.append(np.stack([dx / nd, dy / nd], axis=1))
    return out[0], out[1]


def opposite_matrix(H):
    a, c, b = H[:, 0], H[:, 1], H[:, 2] / 4.0
    with np.errstate(all="ignore"):
        return ((a[:, None] * a[None, :] + c[:, None] * c[None, :]) + (2.0 * b[:, None]) * b[None, :]) < 0.0


def links(P, H):
    """link [n, 4]: along each of d1, d2, -d1, -d2 the nearest candidate b at distance > 0 that lies in the cone, sees the corner
    back in one of its own four cones and has the opposite polarity; ties to the lower index; -1: none."""
    n = len(P)
    d1, d2 = edge_directions(H)
    with np.errstate(all="ignore"):
        ex, ey = P[None, :, 0] - P[:, None, 0], P[None, :, 1] - P[:, None, 1]          # e[a][b] = b - a
        dist = np.sqrt(ex * ex + ey * ey)
        far = dist > 0.0
        ux, uy = ex / dist, ey / dist
        c1 = d1[:, None, 0] * ux + d1[:, None, 1] * uy                                 # [a][b]: b against a's d1
        c2 = d2[:, None, 0] * ux + d2[:, None, 1] * uy
        cones = np.stack([c1 > CONE_COS, c2 > CONE_COS, -c1 > CONE_COS, -c2 > CONE_COS], axis=1) & far[:, None, :]      # [a][k][b]
    seen_back = cones.any(axis=1).T                                                    # [a][b]: a lies in one of b's cones
    cand = cones & (seen_back & opposite_matrix(H))[:, None, :]
    link = np.full((n, 4), -1, dtype=np.int64)
    if n:
        best = np.where(cand, dist[:, None, :], np.inf)
        link = np.where(cand.any(axis=2), best.argmin(axis=2), -1)
    return link


def _norm2(ax, ay, bx, by):
    dx, dy = ax - bx, ay - by
    return math.sqrt(dx * dx + dy * dy)


def predict(cell, L, i, j):
    """(x, y, span) of cell (i, j) from the cells around it, or None: the stencils in the fixed order, their running sum divided
    by their number, the smallest span (a later span replaces the smallest only when it is smaller).  L: the positions as a list
    of pairs of Python floats - the same IEEE doubles, without numpy's per-scalar cost."""
    sx = sy = 0.0
    span = None
    k = 0
    get = cell.get
    for di, dj in STEPS:
        p1, p2 = get((i - di, j - dj)), get((i - 2 * di, j - 2 * dj))
        if p1 is not None and p2 is not None:
            (ax, ay), (bx, by) = L[p1], L[p2]
            px, py, s = 2.0 * ax - bx, 2.0 * ay - by, _norm2(ax, ay, bx, by)
            sx, sy = (px, py) if k == 0 else (sx + px, sy + py)
            span = s if span is None or s < span else span
            k += 1
    for di, dj in DIAGS:
        p1, p2, p3 = get((i - di, j)), get((i, j - dj)), get((i - di, j - dj))
        if p1 is not None and p2 is not None and p3 is not None:
            (ax, ay), (bx, by), (cx, cy) = L[p1], L[p2], L[p3]
            s1, s2 = _norm2(ax, ay, cx, cy), _norm2(bx, by, cx, cy)
            px, py, s = (ax + bx) - cx, (ay + by) - cy, (s2 if s2 < s1 else s1)
            sx, sy = (px, py) if k == 0 else (sx + px, sy + py)
            span = s if span is None or s < span else span
            k += 1
    if k == 0:
        return None
    return sx / float(k), sy / float(k), span


def best_for_cell(cell, P, L, opposite, free, i, j):
    pred = predict(cell, L, i, j)
    if pred is None:
        return -1
    dx, dy = P[:, 0] - pred[0], P[:, 1] - pred[1]
    d = np.sqrt(dx * dx + dy * dy)
    ok = (d <= REACH * pred[2]) & free
    if not ok.any():
        return -1
    for di, dj in STEPS:
        nb = cell.get((i + di, j + dj))
        if nb is not None:
            ok = ok & opposite[nb]
    idx = np.flatnonzero(ok)
    return int(idx[np.argmin(d[idx])]) if len(idx) else -1                # the first of equal distances: the lower index


def grow(P, opposite, a, b, c, limit):
    with np.errstate(all="ignore"):
        return _grow(P, opposite, a, b, c, limit)


def _grow(P, opposite, a, b, c, limit):
    L = [(float(x), float(y)) for x, y in P]
    cell = {(0, 0): a, (1, 0): b, (0, 1): c}
    used = np.zeros(len(P), dtype=bool)
    used[[a, b, c]] = True
    grown = True
    while grown:
        grown = False
        frontier = sorted({(i + di, j + dj) for i, j in cell for di, dj in STEPS} - set(cell))      # as the sweep starts
        for i, j in frontier:
            if abs(i) > limit or abs(j) > limit:
                continue
            q = best_for_cell(cell, P, L, opposite, ~used, i, j)
            if q >= 0:
                cell[(i, j)] = q
                used[q] = True
                grown = True
    for _ in range(SETTLE_ROUNDS):
        moved = False
        for i, j in sorted(cell):
            own = cell.pop((i, j))
            used[own] = False
            q = best_for_cell(cell, P, L, opposite, ~used, i, j)
            q = own if q < 0 else q
            cell[(i, j)] = q
            used[q] = True
            moved = moved or q != own
        if not moved:
            break
    return cell


def full_window(cell, cols, rows):
    """The one completely filled cols x rows or rows x cols window as G[j][i], or None when there is none or more than one."""
    ij = np.array(sorted(cell))
    lo = ij.min(axis=0)
    ni, nj = ij.max(axis=0) - lo + 1
    G = np.full((nj, ni), -1, dtype=np.int64)
    for (i, j), q in cell.items():
        G[j - lo[1], i - lo[0]] = q
    found = []
    for w, h in sorted({(cols, rows), (rows, cols)}):
        for j0 in range(nj - h + 1):
            for i0 in range(ni - w + 1):
                if (G[j0:j0 + h, i0:i0 + w] >= 0).all():
                    found.append(G[j0:j0 + h, i0:i0 + w])
    return found[0] if len(found) == 1 else None


def label(G, P, cols, rows):
    """The window G[j][i] as A[r][c]: right-handed, and of the admissible rotations the one whose A[0][0] is smallest in (y, x), the
    earlier rotation on a tie.  The four rotations by index: A[r][c] = G[r][c], G[c][w-1-r], G[h-1-r][w-1-c], G[h-1-c][r]."""
    h, w = G.shape
    o, ec, er = P[G[0, 0]], P[G[0, 1]], P[G[1, 0]]
    if (ec[0] - o[0]) * (er[1] - o[1]) - (ec[1] - o[1]) * (er[0] - o[0]) < 0.0:
        G = G[:, ::-1]
    best = None
    for q in range(4):
        if ((h, w) if q % 2 == 0 else (w, h)) != (rows, cols):
            continue
        if q == 0:
            A = np.array([[G[r, c] for c in range(cols)] for r in range(rows)])
        elif q == 1:
            A = np.array([[G[c, w - 1 - r] for c in range(cols)] for r in range(rows)])
        elif q == 2:
            A = np.array([[G[h - 1 - r, w - 1 - c] for c in range(cols)] for r in range(rows)])
        else:
            A = np.array([[G[h - 1 - c, r] for c in range(cols)] for r in range(rows)])
        y, x = P[A[0, 0], 1], P[A[0, 0], 0]
        if best is None or y < best[0] or (y == best[0] and x < best[1]):
            best = (y, x, A)
    return best[2]


def assemble(xy, hess, cols, rows, every_attempt=True):
    """One image.  Returns a dict: found (0 / 1), flags, stats = [rows kept, attempts that found a window, the winner's seed rank,
    its edge pair] (-1, -1 without a winner), idx [cols * rows] = the input row of every board corner in id order (id = r * cols + c)
    and xy [cols * rows, 2] = those rows' positions; idx and xy are None without a board.  Every attempt is run, so that the
    count does not depend on where the winner stands; every_attempt=False stops at the winner and leaves the count at 1."""
    cols, rows = int(cols), int(rows)
    assert MIN_SIDE <= cols <= MAX_SIDE and MIN_SIDE <= rows <= MAX_SIDE
    Pin = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    Hin = np.asarray(hess, dtype=np.float64).reshape(-1, 3)
    assert len(Pin) == len(Hin) and len(Pin) <= MAX_ROWS
    keep, usable = screen(Pin, Hin, cols * rows)
    out = dict(found=0, flags=0, stats=[len(keep), 0, -1, -1], idx=None, xy=None)
    if not len(keep):
        return out
    if len(keep) > MAX_KEPT:
        out["flags"] = FLAG_KEPT_LIMIT
        return out
    P, H = Pin[keep], Hin[keep]
    R = response(H)
    link = links(P, H)
    opposite = opposite_matrix(H)
    seeds = np.argsort(-R, kind="stable")
    winner = None
    for rank, s in enumerate(seeds):
        for pair, (kb, kc) in enumerate(PAIRS):
            b, c = int(link[s, kb]), int(link[s, kc])
            if b < 0 or c < 0 or b == c:
                continue
            G = full_window(grow(P, opposite, int(s), b, c, cols + rows), cols, rows)
            if G is None:
                continue
            out["stats"][1] += 1
            if winner is None:
                winner = (rank, pair, G)
            if not every_attempt:
                break
        if winner is not None and not every_attempt:
            break
    if winner is None:
        return out
    A = label(winner[2], P, cols, rows)
    out["found"] = 1
    out["stats"][2], out["stats"][3] = winner[0], winner[1]
    out["idx"] = keep[A.reshape(-1)].astype(np.int32)
    out["xy"] = Pin[out["idx"]].copy()
    return out


def as_dict(res):
    """The result in api.assemble_checkerboard's form: {id: (x, y)} or None."""
    if not res["found"]:
        return None
    return {i: (float(x), float(y)) for i, (x, y) in enumerate(res["xy"])}


def first_winner(xy, hess, cols, rows):
    """assemble() stopped at the first attempt that finds a window, as api.assemble_checkerboard stops, in its form: {id: (x, y)} or
    None - for comparisons that do not need the count of the other attempts."""
    return as_dict(assemble(xy, hess, cols, rows, every_attempt=False))
