// Corner candidates ordered into complete checkerboards (ccal_assemble_checkerboards_batch) and the chain from images to boards in
// one device-resident call (ccal_detect_checkerboards_batch / _dev), by the rule stated at those entry points in include/ccal.h;
// tests/board_ref.py is its numpy yardstick.  Compiled with -ffp-contract=off (csrc/Makefile): every product and sum rounds on its
// own, as numpy's do.  Wave64 code; every kernel is a grid of single wavefronts that share nothing but read-only inputs.
//   k_board_screen  one wavefront per image: responses, the usable rows, the threshold (a rank count over index order), the kept rows
//                   compacted by the wavefront's scan, their (y, x, index) order and the seeds' order by rank counts, the two edge
//                   directions of every kept corner.  O(m^2 / 64) comparisons for m input rows.
//   k_board_link    one lane per kept corner a, all b in index order: the four links.  No cross-lane traffic at all.
//   k_board_grow    one wavefront per (image, seed rank, edge pair): the lattice as an int16 grid in LDS, the positions beside it; the
//                   cells of a sweep are visited one after another in (i, j) order, the lanes divide the candidates of a cell's
//                   distance test and a butterfly takes the nearest (ties: the lower index).  It records ONE bit: exactly one full
//                   window or not.
//   k_board_final   one wavefront per image: the first recorded bit in (seed rank, pair) order and their number, then that attempt
//                   once more, its window made right-handed and turned, the board written.
// No atomics and no workgroup barrier inside divergent control flow; every loop's bound comes from n and the lattice size: a sweep
// that fills nothing ends the growth, a fill consumes a candidate (at most n - 3 fills, so at most n sweeps), three settle rounds.
// An attempt never looks at another attempt's bit, so nothing depends on the order in which the wavefronts run.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "ccal_chain_front.hpp"
#include "ccal_image_device.hpp"

namespace ccal {

constexpr int kBoardMaxRows = CCAL_BOARD_MAX_ROWS;     // kBoardMaxKept and the bytes per row: ccal_tagchain_plan.hpp
constexpr int kBoardMinSide = CCAL_BOARD_MIN_SIDE, kBoardMaxSide = CCAL_BOARD_MAX_SIDE;
constexpr double kBoardCone = 0.9, kBoardWeak = 0.5, kBoardReach = 0.3;
constexpr int kBoardNew = 0x4000, kBoardNone = 0x7fffffff;
static_assert(kBoardMaxKept <= 512, "a lane's candidates are the bits of one byte; an index and the sweep's mark share an int16");

struct BoardArgs {
    const int64_t* off;                 // [n_img + 1]: image k owns the rows [off[k], off[k + 1]) of xy, hess / hess_i, status, resp, kidx
    const double* xy;                   // [.][2]
    const double* hess;                 // [.][3] (hxx, hyy, hxy), or
    const int32_t* hess_i;              // [.][3] as the detector stores them
    const int32_t* status;              // [.] only CCAL_OK rows are usable; NULL: every row is
    double* resp;                       // [.] work: the response of a usable row, -1 otherwise
    int32_t* kidx;                      // [.] work: the kept rows of the image in input order
    // per image K slots, in the (y, x, input row) order of the kept rows
    double* P;                          // [n_img][K][2]
    double* M;                          // [n_img][K][3]: hxx, hyy, hxy / 4
    double* R;                          // [n_img][K]
    double* D;                          // [n_img][K][4]: d1, d2
    int32_t* orig;                      // [n_img][K]: the input row
    int32_t* link;                      // [n_img][K][4]
    int32_t* seed;                      // [n_img][K]: the slot of each seed rank
    uint8_t* hit;                       // [n_img][4 K]: the attempt found exactly one window
    int32_t* kept;                      // [n_img]
    int32_t* found; int32_t* flags; int32_t* stats;      // [n_img], [n_img], [n_img][4]
    double* oxy; int32_t* oidx;         // [n_img][cols rows][2], [n_img][cols rows] or NULL
    int32_t n_img, cols, rows, row_cap, K;
    int32_t per;                        // blocks per image of the launch (k_board_link, k_board_grow)
};

__device__ __forceinline__ void board_hess(const BoardArgs& a, int64_t row, double& hxx, double& hyy, double& hxy) {
    if (a.hess) { hxx = a.hess[3 * row]; hyy = a.hess[3 * row + 1]; hxy = a.hess[3 * row + 2]; }
    else { hxx = (double)a.hess_i[3 * row]; hyy = (double)a.hess_i[3 * row + 1]; hxy = (double)a.hess_i[3 * row + 2]; }
}

// the two unit zero-curvature directions of [[a, b], [b, c]]: d[0 .. 1] = d1, d[2 .. 3] = d2
__device__ __forceinline__ void board_directions(double a, double c, double b, double* d) {
    const double m = 0.5 * (a + c), dl = 0.5 * (a - c);
    const double r = sqrt(dl * dl + b * b);
    const double l1 = m + r, l0 = m - r;
    const bool pos = dl >= 0.0;
    double vx = pos ? dl + r : b, vy = pos ? b : r - dl;
    const double nv = sqrt(vx * vx + vy * vy);
    if (nv > 0.0) { vx = vx / nv; vy = vy / nv; } else { vx = 1.0; vy = 0.0; }
    const double wx = -vy, wy = vx;
    const double A = sqrt(fmax(l1, 0.0)), B = sqrt(fmax(-l0, 0.0));
    for (int s = 0; s < 2; ++s) {
        const double sa = s ? -A : A;
        const double dx = B * vx + sa * wx, dy = B * vy + sa * wy;
        const double nd = fmax(sqrt(dx * dx + dy * dy), 1e-300);
        d[2 * s] = dx / nd; d[2 * s + 1] = dy / nd;
    }
}

__global__ __launch_bounds__(64) void k_board_screen(const BoardArgs a) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int64_t first = a.off[k];
    const int m = csr_span(a.off, k, a.row_cap);
    const int n_want = a.cols * a.rows;
    const double* xy = a.xy + 2 * first;
    double* resp = a.resp + first;
    int32_t* kidx = a.kidx + first;
    int usable = 0;
    for (int b0 = 0; b0 < m; b0 += 64) {
        const int i = b0 + lane;
        bool ok = false;
        if (i < m) {
            double hxx, hyy, hxy;
            board_hess(a, first + i, hxx, hyy, hxy);
            const double r = hxy * hxy - (16.0 * hxx) * hyy;
            ok = (!a.status || a.status[first + i] == CCAL_OK) && isfinite(xy[2 * i]) && isfinite(xy[2 * i + 1]) && r > 0.0 && isfinite(r);
            resp[i] = ok ? r : -1.0;
        }
        usable += __popcll(__ballot(ok));
    }
    int n = 0;
    if (usable >= n_want) {
        wave_handoff();
        double t = 0.0;                                    // half the response of the usable row of rank n_want - 1
        for (int b0 = 0; b0 < m; b0 += 64) {
            const int i = b0 + lane;
            const double ri = i < m ? resp[i] : -1.0;
            int rank = 0;
            for (int j = 0; j < m; ++j) {                  // wave-uniform
                const double rj = resp[j];
                rank += (rj > ri || (rj == ri && j < i)) ? 1 : 0;
            }
            const unsigned long long is = __ballot(ri > 0.0 && rank == n_want - 1);
            if (is) t = kBoardWeak * __shfl(ri, __ffsll((long long)is) - 1, 64);
        }
        for (int b0 = 0; b0 < m; b0 += 64) {
            const int i = b0 + lane;
            const bool keep = i < m && resp[i] > 0.0 && resp[i] >= t;
            const int32_t inc = wave_scan_inclusive(keep ? 1 : 0, lane);
            const int pos = n + inc - 1;
            if (keep && pos < m) kidx[pos] = i;
            n += __shfl(inc, 63, 64);
        }
    }
    if (lane == 0) {
        a.kept[k] = n;
        a.found[k] = 0;
        a.flags[k] = n > kBoardMaxKept ? CCAL_BOARD_FLAG_KEPT_LIMIT : 0;
        a.stats[4 * k] = n; a.stats[4 * k + 1] = 0; a.stats[4 * k + 2] = -1; a.stats[4 * k + 3] = -1;
    }
    if (n < 1 || n > a.K) return;
    wave_handoff();
    const size_t s0 = (size_t)k * a.K;
    double* P = a.P + 2 * s0; double* M = a.M + 3 * s0; double* R = a.R + s0; double* D = a.D + 4 * s0;
    int32_t* orig = a.orig + s0; int32_t* seed = a.seed + s0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        const int i = e < n ? kidx[e] : 0;
        const double x = e < n ? xy[2 * i] : 0.0, y = e < n ? xy[2 * i + 1] : 0.0;
        int rank = 0;
        for (int f = 0; f < n; ++f) {                      // wave-uniform
            const int j = kidx[f];
            const double xj = xy[2 * j], yj = xy[2 * j + 1];
            rank += (yj < y || (yj == y && (xj < x || (xj == x && j < i)))) ? 1 : 0;
        }
        if (e < n && rank < n) {
            double hxx, hyy, hxy;
            board_hess(a, first + i, hxx, hyy, hxy);
            const double b = hxy / 4.0;
            P[2 * rank] = x; P[2 * rank + 1] = y;
            M[3 * rank] = hxx; M[3 * rank + 1] = hyy; M[3 * rank + 2] = b;
            R[rank] = resp[i];
            orig[rank] = i;
            board_directions(hxx, hyy, b, D + 4 * rank);
        }
    }
    wave_handoff();
    for (int e0 = 0; e0 < n; e0 += 64) {                   // seeds: stronger first, ties by slot
        const int e = e0 + lane;
        const double re = e < n ? R[e] : 0.0;
        int rank = 0;
        for (int f = 0; f < n; ++f) {
            const double rf = R[f];
            rank += (rf > re || (rf == re && f < e)) ? 1 : 0;
        }
        if (e < n && rank < n) seed[rank] = e;
    }
}

__global__ __launch_bounds__(64) void k_board_link(const BoardArgs a) {
    const int k = blockIdx.x / a.per, lane = threadIdx.x;
    const int n = a.kept[k];
    if (n < 1 || n > a.K) return;
    const int i = (blockIdx.x % a.per) * 64 + lane;
    if (i >= n) return;
    const size_t s0 = (size_t)k * a.K;
    const double* P = a.P + 2 * s0; const double* M = a.M + 3 * s0; const double* D = a.D + 4 * s0;
    const double ax = P[2 * i], ay = P[2 * i + 1];
    const double d1x = D[4 * i], d1y = D[4 * i + 1], d2x = D[4 * i + 2], d2y = D[4 * i + 3];
    const double m0 = M[3 * i], m1 = M[3 * i + 1], m2 = M[3 * i + 2];
    double best[4];
    int32_t to[4] = { -1, -1, -1, -1 };
    for (int b = 0; b < n; ++b) {
        const double ex = P[2 * b] - ax, ey = P[2 * b + 1] - ay;
        const double dist = sqrt(ex * ex + ey * ey);
        if (!(dist > 0.0)) continue;
        const double ux = ex / dist, uy = ey / dist;
        // a against b's directions: the unit vector from b to a is (-ux, -uy) exactly, so b's four cosines are +- these two
        const double b1 = D[4 * b] * ux + D[4 * b + 1] * uy, b2 = D[4 * b + 2] * ux + D[4 * b + 3] * uy;
        if (!(fabs(b1) > kBoardCone || fabs(b2) > kBoardCone)) continue;
        if (!((m0 * M[3 * b] + m1 * M[3 * b + 1]) + (2.0 * m2) * M[3 * b + 2] < 0.0)) continue;
        const double c1 = d1x * ux + d1y * uy, c2 = d2x * ux + d2y * uy;
        const bool in[4] = { c1 > kBoardCone, c2 > kBoardCone, -c1 > kBoardCone, -c2 > kBoardCone };
        for (int q = 0; q < 4; ++q)
            if (in[q] && (to[q] < 0 || dist < best[q])) { best[q] = dist; to[q] = b; }
    }
    for (int q = 0; q < 4; ++q) a.link[4 * (s0 + i) + q] = to[q];
}

// One attempt's lattice.  lat: S x S int16 cells, cell (i, j) at (i + o) S + (j + o) with o = L + 2, so that the stencils' reads two
// cells beyond |i|, |j| <= L stay inside; -1: empty, else the slot, with kBoardNew set while the sweep that filled it runs.
struct BoardLattice {
    const double* Pl;                   // LDS: the image's positions
    const double* M;                    // global
    int16_t* lat;
    int S, o, n, lane;
    unsigned used;                      // bit t: slot 64 t + lane is in the lattice
    int imin, imax, jmin, jmax;         // the filled cells' box
};

__device__ __forceinline__ int board_raw(const BoardLattice& g, int i, int j) { return g.lat[(i + g.o) * g.S + (j + g.o)]; }
__device__ __forceinline__ int board_cell(const BoardLattice& g, int i, int j) {
    const int v = board_raw(g, i, j);
    return v < 0 ? -1 : (v & (kBoardNew - 1));
}
__device__ __forceinline__ void board_put(BoardLattice& g, int i, int j, int v) {        // all lanes call it; lane 0 writes
    if (g.lane == 0) g.lat[(i + g.o) * g.S + (j + g.o)] = (int16_t)v;
    wave_handoff();
}
__device__ __forceinline__ void board_use(BoardLattice& g, int q, bool on) {
    if ((q & 63) == g.lane) g.used = on ? (g.used | (1u << (q >> 6))) : (g.used & ~(1u << (q >> 6)));
}

__device__ __forceinline__ void board_stencil(double px, double py, double s, double& sx, double& sy, double& span, int& cnt) {
    if (cnt == 0) { sx = px; sy = py; span = s; }
    else { sx = sx + px; sy = sy + py; span = s < span ? s : span; }
    ++cnt;
}

// the slot for cell (i, j), or -1: the same value in every lane
__device__ int board_best(const BoardLattice& g, int i, int j) {
    constexpr int di4[4] = { 1, 0, -1, 0 }, dj4[4] = { 0, 1, 0, -1 };
    constexpr int ddi[4] = { 1, 1, -1, -1 }, ddj[4] = { 1, -1, 1, -1 };
    const double* P = g.Pl;
    double sx = 0.0, sy = 0.0, span = 0.0;
    int cnt = 0;
    int nb[4];
    for (int s = 0; s < 4; ++s) {
        const int p1 = board_cell(g, i - di4[s], j - dj4[s]), p2 = board_cell(g, i - 2 * di4[s], j - 2 * dj4[s]);
        nb[(s + 2) & 3] = p1;                              // the cell at (i + di, j + dj) of step s + 2
        if (p1 >= 0 && p2 >= 0) {
            const double ax = P[2 * p1], ay = P[2 * p1 + 1], bx = P[2 * p2], by = P[2 * p2 + 1];
            const double dx = ax - bx, dy = ay - by;
            board_stencil(2.0 * ax - bx, 2.0 * ay - by, sqrt(dx * dx + dy * dy), sx, sy, span, cnt);
        }
    }
    for (int s = 0; s < 4; ++s) {
        const int p1 = board_cell(g, i - ddi[s], j), p2 = board_cell(g, i, j - ddj[s]), p3 = board_cell(g, i - ddi[s], j - ddj[s]);
        if (p1 >= 0 && p2 >= 0 && p3 >= 0) {
            const double ax = P[2 * p1], ay = P[2 * p1 + 1], bx = P[2 * p2], by = P[2 * p2 + 1], cx = P[2 * p3], cy = P[2 * p3 + 1];
            const double d1x = ax - cx, d1y = ay - cy, d2x = bx - cx, d2y = by - cy;
            const double s1 = sqrt(d1x * d1x + d1y * d1y), s2 = sqrt(d2x * d2x + d2y * d2y);
            board_stencil((ax + bx) - cx, (ay + by) - cy, s2 < s1 ? s2 : s1, sx, sy, span, cnt);
        }
    }
    if (cnt == 0) return -1;
    const double mx = sx / (double)cnt, my = sy / (double)cnt, reach = kBoardReach * span;
    double bd = 0.0;
    int bq = kBoardNone;
    for (int t = 0, q = g.lane; q < g.n; ++t, q += 64) {
        if ((g.used >> t) & 1u) continue;
        const double dx = P[2 * q] - mx, dy = P[2 * q + 1] - my;
        const double d = sqrt(dx * dx + dy * dy);
        if (!(d <= reach)) continue;
        bool ok = true;
        for (int s = 0; s < 4; ++s)
            if (nb[s] >= 0) {
                const double* mq = g.M + 3 * q; const double* mn = g.M + 3 * nb[s];
                ok = ok && ((mn[0] * mq[0] + mn[1] * mq[1]) + (2.0 * mn[2]) * mq[2] < 0.0);
            }
        if (ok && (bq == kBoardNone || d < bd)) { bd = d; bq = q; }
    }
    for (int w = 32; w >= 1; w >>= 1) {
        const double od = __shfl_xor(bd, w, 64);
        const int oq = __shfl_xor(bq, w, 64);
        if (oq != kBoardNone && (bq == kBoardNone || od < bd || (od == bd && oq < bq))) { bd = od; bq = oq; }
    }
    return bq == kBoardNone ? -1 : bq;
}

struct BoardWindow { int i0, j0, w, h; };

// The lattice grown from slot s0 at (0, 0), b at (1, 0), c at (0, 1), settled; true: exactly one full window, in win.
__device__ bool board_attempt(BoardLattice& g, int s0, int b, int c, int L, int cols, int rows, BoardWindow& win) {
    const int lane = g.lane;
    for (int t = lane; t < g.S * g.S; t += 64) g.lat[t] = -1;
    wave_handoff();
    g.used = 0;
    board_put(g, 0, 0, s0); board_put(g, 1, 0, b); board_put(g, 0, 1, c);
    board_use(g, s0, true); board_use(g, b, true); board_use(g, c, true);
    g.imin = 0; g.imax = 1; g.jmin = 0; g.jmax = 1;
    int filled = 3;
    for (int sweep = 0; sweep < g.n; ++sweep) {
        bool grown = false;
        const int i0 = max(g.imin - 1, -L), i1 = min(g.imax + 1, L), j0 = max(g.jmin - 1, -L), j1 = min(g.jmax + 1, L);
        for (int i = i0; i <= i1; ++i)
            for (int jb = j0; jb <= j1; jb += 64) {
                const int jl = jb + lane;
                bool fr = false;
                if (jl <= j1 && board_raw(g, i, jl) < 0) {                 // empty, next to a cell filled before this sweep
                    const int v0 = board_raw(g, i + 1, jl), v1 = board_raw(g, i - 1, jl), v2 = board_raw(g, i, jl + 1), v3 = board_raw(g, i, jl - 1);
                    fr = (v0 >= 0 && v0 < kBoardNew) || (v1 >= 0 && v1 < kBoardNew) || (v2 >= 0 && v2 < kBoardNew) || (v3 >= 0 && v3 < kBoardNew);
                }
                unsigned long long todo = __ballot(fr);
                while (todo) {                                             // wave-uniform: the row's frontier cells in order
                    const int j = jb + __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const int q = board_best(g, i, j);
                    if (q < 0 || filled >= g.n) continue;
                    board_put(g, i, j, q | kBoardNew);
                    board_use(g, q, true);
                    g.imin = min(g.imin, i); g.imax = max(g.imax, i); g.jmin = min(g.jmin, j); g.jmax = max(g.jmax, j);
                    ++filled;
                    grown = true;
                }
            }
        if (!grown) break;
        for (int i = g.imin; i <= g.imax; ++i)                              // the sweep is over: its cells count as filled
            for (int jb = g.jmin; jb <= g.jmax; jb += 64) {
                const int jl = jb + lane;
                if (jl <= g.jmax) {
                    const int v = board_raw(g, i, jl);
                    if (v >= kBoardNew) g.lat[(i + g.o) * g.S + (jl + g.o)] = (int16_t)(v & (kBoardNew - 1));
                }
            }
        wave_handoff();
    }
    for (int round = 0; round < 3; ++round) {
        bool moved = false;
        for (int i = g.imin; i <= g.imax; ++i)
            for (int jb = g.jmin; jb <= g.jmax; jb += 64) {
                const int jl = jb + lane;
                unsigned long long todo = __ballot(jl <= g.jmax && board_raw(g, i, jl) >= 0);
                while (todo) {
                    const int j = jb + __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const int own = board_cell(g, i, j);
                    board_put(g, i, j, -1);
                    board_use(g, own, false);
                    int q = board_best(g, i, j);
                    q = q < 0 ? own : q;
                    board_put(g, i, j, q);
                    board_use(g, q, true);
                    moved = moved || q != own;
                }
            }
        if (!moved) break;
    }
    if (filled < cols * rows) return false;
    const int ni = g.imax - g.imin + 1, nj = g.jmax - g.jmin + 1;
    int count = 0;
    win = BoardWindow{ 0, 0, 0, 0 };
    for (int o = 0; o < (cols == rows ? 1 : 2) && count < 2; ++o) {
        const int w = o ? rows : cols, h = o ? cols : rows;
        const int nio = ni - w + 1, njo = nj - h + 1;
        if (nio <= 0 || njo <= 0) continue;
        const int total = nio * njo;
        for (int t0 = 0; t0 < total && count < 2; t0 += 64) {
            const int t = t0 + lane;
            const int wi = g.imin + (t % nio), wj = g.jmin + (t / nio);
            bool full = t < total;
            for (int jj = 0; jj < h && full; ++jj)
                for (int ii = 0; ii < w && full; ++ii) full = board_raw(g, wi + ii, wj + jj) >= 0;
            const unsigned long long hits = __ballot(full);
            if (hits && count == 0) {
                const int src = __ffsll((long long)hits) - 1;
                win = BoardWindow{ __shfl(wi, src, 64), __shfl(wj, src, 64), w, h };
            }
            count += __popcll(hits);
        }
    }
    return count == 1;
}

// the attempt's three slots, or false: the seed has no neighbour along one of the two edges, or the same along both
__device__ __forceinline__ bool board_seeds(const BoardArgs& a, int k, int n, int attempt, int& s0, int& b, int& c) {
    const size_t base = (size_t)k * a.K;
    const int rank = attempt >> 2, pair = attempt & 3;
    if (rank >= n) return false;
    s0 = a.seed[base + rank];
    if (s0 < 0 || s0 >= n) return false;
    b = a.link[4 * (base + s0) + (pair & 2)];              // pairs (0, 1), (0, 3), (2, 1), (2, 3)
    c = a.link[4 * (base + s0) + ((pair & 1) ? 3 : 1)];
    return b >= 0 && c >= 0 && b != c && b < n && c < n;
}

__device__ __forceinline__ void board_lattice(const BoardArgs& a, int k, int n, int lane, char* smem, BoardLattice& g) {
    const int L = a.cols + a.rows;
    double* Pl = reinterpret_cast<double*>(smem);
    const double* P = a.P + 2 * (size_t)k * a.K;
    for (int t = lane; t < 2 * n; t += 64) Pl[t] = P[t];
    g.Pl = Pl; g.M = a.M + 3 * (size_t)k * a.K;
    g.lat = reinterpret_cast<int16_t*>(smem + 16 * (size_t)a.K);
    g.S = 2 * L + 5; g.o = L + 2; g.n = n; g.lane = lane;
}

static size_t board_lds_bytes(int K, int cols, int rows) {
    const size_t S = 2 * (size_t)(cols + rows) + 5;
    return (16 * (size_t)K + 2 * S * S + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(64) void k_board_grow(const BoardArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int k = blockIdx.x / a.per, attempt = blockIdx.x % a.per, lane = threadIdx.x;
    const int n = a.kept[k];
    if (n < 1 || n > a.K || attempt >= 4 * n) return;
    int s0, b, c;
    bool one = false;
    if (board_seeds(a, k, n, attempt, s0, b, c)) {         // wave-uniform
        BoardLattice g;
        BoardWindow win;
        board_lattice(a, k, n, lane, smem, g);
        one = board_attempt(g, s0, b, c, a.cols + a.rows, a.cols, a.rows, win);
    }
    if (lane == 0) a.hit[4 * (size_t)k * a.K + attempt] = one ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_board_final(const BoardArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int n = a.kept[k];
    if (n < 1 || n > a.K) return;
    const uint8_t* hit = a.hit + 4 * (size_t)k * a.K;
    int wins = 0, winner = -1;
    for (int t0 = 0; t0 < 4 * n; t0 += 64) {
        const int t = t0 + lane;
        const unsigned long long h = __ballot(t < 4 * n && hit[t] != 0);
        if (h && winner < 0) winner = t0 + __ffsll((long long)h) - 1;
        wins += __popcll(h);
    }
    if (lane == 0) { a.stats[4 * k + 1] = wins; a.stats[4 * k + 2] = winner < 0 ? -1 : winner >> 2; a.stats[4 * k + 3] = winner < 0 ? -1 : winner & 3; }
    int s0, b, c;
    if (winner < 0 || !board_seeds(a, k, n, winner, s0, b, c)) return;
    BoardLattice g;
    BoardWindow win;
    board_lattice(a, k, n, lane, smem, g);
    if (!board_attempt(g, s0, b, c, a.cols + a.rows, a.cols, a.rows, win)) return;
    // G[jj][ii] = the window's cell (i0 + ii, j0 + jj), h x w; mirrored in ii when left-handed
    const double* P = g.Pl;
    const int w = win.w, h = win.h;
    const int g00 = board_cell(g, win.i0, win.j0), g01 = board_cell(g, win.i0 + 1, win.j0), g10 = board_cell(g, win.i0, win.j0 + 1);
    const double ecx = P[2 * g01] - P[2 * g00], ecy = P[2 * g01 + 1] - P[2 * g00 + 1];
    const double erx = P[2 * g10] - P[2 * g00], ery = P[2 * g10 + 1] - P[2 * g00 + 1];
    const bool mirror = ecx * ery - ecy * erx < 0.0;
    auto G = [&](int jj, int ii) { return board_cell(g, win.i0 + (mirror ? w - 1 - ii : ii), win.j0 + jj); };
    // the rotations A[r][c] = G[r][c], G[c][w-1-r], G[h-1-r][w-1-c], G[h-1-c][r]; the first of the smallest (y, x) of A[0][0]
    int turn = -1;
    double ty = 0.0, tx = 0.0;
    for (int q = 0; q < 4; ++q) {
        if (((q & 1) ? w : h) != a.rows || ((q & 1) ? h : w) != a.cols) continue;
        const int s = q == 0 ? G(0, 0) : q == 1 ? G(0, w - 1) : q == 2 ? G(h - 1, w - 1) : G(h - 1, 0);
        const double y = P[2 * s + 1], x = P[2 * s];
        if (turn < 0 || y < ty || (y == ty && x < tx)) { turn = q; ty = y; tx = x; }
    }
    if (turn < 0) return;
    const int n_want = a.cols * a.rows;
    const int32_t* orig = a.orig + (size_t)k * a.K;
    for (int id = lane; id < n_want; id += 64) {
        const int r = id / a.cols, cc = id % a.cols;
        const int s = turn == 0 ? G(r, cc) : turn == 1 ? G(cc, w - 1 - r) : turn == 2 ? G(h - 1 - r, w - 1 - cc) : G(h - 1 - cc, r);
        a.oxy[2 * ((size_t)k * n_want + id)] = P[2 * s]; a.oxy[2 * ((size_t)k * n_want + id) + 1] = P[2 * s + 1];
        if (a.oidx) a.oidx[(size_t)k * n_want + id] = orig[s];
    }
    if (lane == 0) a.found[k] = 1;
}

namespace {

// The assembly's slices of a call's block, added as ints | doubles like the front's (ccal_chain_front.hpp) so that the doubles the kernels
// write before they read lie together, resp .. oxy; rows: a chunk's input rows, mi: its images.  h_*: the host's side of a chunk.
struct BoardSlices {
    Slice<int32_t> kidx, orig, link, seed; Slice<uint8_t> hit; Slice<int32_t> kept, found, flags, stats, oidx;
    Slice<double> resp, P, M, R, D, oxy;
    size_t rows = 0, K = 0, mi = 0, nw = 0;
    std::vector<int32_t> h_kept, h_found, h_flags, h_stats, h_idx; std::vector<double> h_xy;
    void add_ints(CallBlock& blk, size_t rows_, size_t K_, size_t mi_, size_t nw_, bool with_idx) {
        rows = rows_; K = K_; mi = mi_; nw = nw_;
        kidx = blk.add<int32_t>(rows);
        orig = blk.add<int32_t>(K * mi); link = blk.add<int32_t>(4 * K * mi); seed = blk.add<int32_t>(K * mi); hit = blk.add<uint8_t>(4 * K * mi);
        kept = blk.add<int32_t>(mi); found = blk.add<int32_t>(mi); flags = blk.add<int32_t>(mi); stats = blk.add<int32_t>(4 * mi);
        if (with_idx) oidx = blk.add<int32_t>(nw * mi);
        h_kept.resize(mi); h_found.resize(mi); h_flags.resize(mi); h_stats.resize(4 * mi); h_idx.resize(with_idx ? nw * mi : 0); h_xy.resize(2 * nw * mi);
    }
    void add_doubles(CallBlock& blk) {
        resp = blk.add<double>(rows);
        P = blk.add<double>(2 * K * mi); M = blk.add<double>(3 * K * mi); R = blk.add<double>(K * mi); D = blk.add<double>(4 * K * mi);
        oxy = blk.add<double>(2 * nw * mi);
    }
    BoardArgs args(const CallBlock& blk, int cols, int rows_) const {       // the caller sets off, xy, hess or hess_i, status, row_cap, n_img
        BoardArgs a = {};
        a.resp = blk.at(resp); a.kidx = blk.at(kidx);
        a.P = blk.at(P); a.M = blk.at(M); a.R = blk.at(R); a.D = blk.at(D); a.orig = blk.at(orig); a.link = blk.at(link);
        a.seed = blk.at(seed); a.hit = blk.at(hit); a.kept = blk.at(kept); a.found = blk.at(found); a.flags = blk.at(flags);
        a.stats = blk.at(stats); a.oxy = blk.at(oxy); a.oidx = blk.at(oidx);
        a.cols = cols; a.rows = rows_; a.K = (int32_t)K;
        return a;
    }
};

struct BoardsOut { int32_t* found; double* xy; int32_t* idx; int32_t* flags; int32_t* stats; };       // idx, stats: or NULL

// screen; the host learns the kept counts; links, attempts, the board - sized by the largest kept count within the limit
// h_kept: room for a.n_img counts.  Leaves the stream synchronised after the screen only.
void board_run(CallBlock& blk, hipStream_t st, BoardArgs& a, std::vector<int32_t>& h_kept) {
    const size_t m = (size_t)a.n_img;
    hipLaunchKernelGGL(k_board_screen, dim3((unsigned)m), dim3(64), 0, st, a);
    blk.launched();
    blk.download(h_kept.data(), a.kept, m);
    if (blk.ok()) blk.note(hipStreamSynchronize(st));
    if (!blk.ok()) return;
    int most = 0;
    for (size_t i = 0; i < m; ++i)
        if (h_kept[i] <= a.K) most = std::max(most, h_kept[i]);
    if (most < 1) return;
    const size_t lds = board_lds_bytes(a.K, a.cols, a.rows);
    a.per = (most + 63) / 64;
    hipLaunchKernelGGL(k_board_link, dim3((unsigned)(m * (size_t)a.per)), dim3(64), 0, st, a);
    blk.launched();
    a.per = 4 * most;
    if (blk.ok()) { hipLaunchKernelGGL(k_board_grow, dim3((unsigned)(m * (size_t)a.per)), dim3(64), lds, st, a); blk.launched(); }
    if (blk.ok()) { hipLaunchKernelGGL(k_board_final, dim3((unsigned)m), dim3(64), lds, st, a); blk.launched(); }
}

// The boards of the chunk's images, which are the caller's k0 ..: down, the stream synchronised, and found, stats, xy and idx into
// the caller's arrays - xy and idx only where there is a board.  The flags stay in h.h_flags: the caller decides how they go out.
bool board_fetch(CallBlock& blk, hipStream_t st, const BoardArgs& a, BoardSlices& h, size_t k0, const BoardsOut& out) {
    const size_t m = (size_t)a.n_img, nw = (size_t)a.cols * (size_t)a.rows;
    blk.download(h.h_found.data(), a.found, m);
    blk.download(h.h_flags.data(), a.flags, m);
    blk.download(h.h_stats.data(), a.stats, 4 * m);
    blk.download(h.h_xy.data(), a.oxy, 2 * nw * m);
    blk.download(a.oidx ? h.h_idx.data() : nullptr, a.oidx, nw * m);
    if (blk.ok()) blk.note(hipStreamSynchronize(st));
    if (!blk.ok()) return false;
    for (size_t i = 0; i < m; ++i) {
        const size_t k = k0 + i;
        out.found[k] = h.h_found[i];
        if (out.stats) std::memcpy(out.stats + 4 * k, h.h_stats.data() + 4 * i, 4 * sizeof(int32_t));
        if (!h.h_found[i]) continue;
        std::memcpy(out.xy + 2 * nw * k, h.h_xy.data() + 2 * nw * i, 2 * nw * sizeof(double));
        if (out.idx) std::memcpy(out.idx + nw * k, h.h_idx.data() + nw * i, nw * sizeof(int32_t));
    }
    return true;
}

const char* board_bad_pattern(int cols, int rows) {
    const bool bad = cols < kBoardMinSide || cols > kBoardMaxSide || rows < kBoardMinSide || rows > kBoardMaxSide;
    return bad ? "cols, rows outside 2 .. 20" : nullptr;
}

int assemble_call(ccal_ctx* ctx, const char* where, int n_img, const int64_t* offsets, const double* xy, const double* hess, int cols,
                  int rows, const BoardsOut& out) {
    const BadArg bad{ ctx, where };
    if (const char* what = board_bad_pattern(cols, rows)) return bad(what);
    if (n_img < 0) return bad("n_img < 0");
    if (n_img == 0) return CCAL_OK;
    if (!offsets || !out.found || !out.xy || !out.flags) return bad("NULL argument");
    if (check_offsets(ctx, where, "offsets", offsets, (size_t)n_img, 0)) return CCAL_ERR_INVALID_ARG;
    size_t most = 0;
    for (int k = 0; k < n_img; ++k) most = std::max(most, (size_t)(offsets[k + 1] - offsets[k]));
    if (most > (size_t)kBoardMaxRows) return bad("more than 4096 rows in an image");
    if (offsets[n_img] > 0 && (!xy || !hess)) return bad("NULL argument");

    const size_t ni = (size_t)n_img, nw = (size_t)cols * (size_t)rows;
    const size_t K = std::max<size_t>(std::min(most, (size_t)kBoardMaxKept), 1);
    const ImageChunks plan = image_chunks(offsets, ni, K * kBoardPerKeptBytes + nw * 20 + kBoardPerImageBytes, kBoardPerRowBytes,
                                          test_chunk_bytes("CCAL_TEST_BOARD_CHUNK_BYTES", kChainChunkBytes));
    const size_t mi = plan.max_img, mr = plan.max_rows;

    CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(mi + 1);
    const auto s_hess = blk.add<double>(3 * mr);           // uploaded, like s_xy: not poisoned
    const auto s_xy = blk.add<double>(2 * mr);
    BoardSlices bs;
    bs.add_ints(blk, mr, K, mi, nw, true);
    bs.add_doubles(blk);                                   // the doubles the kernels write before they read
    if (!blk.alloc()) return blk.finish(where);

    BoardArgs a = bs.args(blk, cols, rows);
    a.off = blk.at(s_off); a.xy = blk.at(s_xy); a.hess = blk.at(s_hess); a.row_cap = kBoardMaxRows;
    hipStream_t st = ctx->stream;
    std::vector<int64_t> h_off(mi + 1);
    for (size_t c = 0; c + 1 < plan.cut.size() && blk.ok(); ++c) {
        const size_t k0 = plan.cut[c], m = plan.cut[c + 1] - k0;
        const size_t at = (size_t)offsets[k0], nr = (size_t)(offsets[k0 + m] - offsets[k0]);
        for (size_t i = 0; i <= m; ++i) h_off[i] = offsets[k0 + i] - offsets[k0];
        a.n_img = (int32_t)m;
        blk.poison(bs.resp, bs.oxy);
        blk.upload(s_off, h_off.data(), m + 1);
        blk.upload(s_xy, xy + 2 * at, 2 * nr);
        blk.upload(s_hess, hess + 3 * at, 3 * nr);
        if (!blk.ok()) break;
        board_run(blk, st, a, bs.h_kept);
        if (!board_fetch(blk, st, a, bs, k0, out)) break;
        std::copy(bs.h_flags.begin(), bs.h_flags.begin() + m, out.flags + k0);          // the assembly's flags are the image's
    }
    return blk.finish(where);
}

int detect_boards_call(ccal_ctx* ctx, const char* where, const GreyBatch& b, const ccal_detect_checkerboards_opts* o, const BoardsOut& out) {
    const BadArg bad{ ctx, where };
    char buf[40];
    if (!o) return bad("NULL options");
    const FrontParams fp = FrontParams::of(*o);
    if (const char* what = front_bad_params(fp, kBoardMaxRows, buf)) return bad(what);
    if (const char* what = board_bad_pattern(o->cols, o->rows)) return bad(what);
    if (const char* what = b.bad()) return bad(what);
    if (b.n_img == 0) return CCAL_OK;
    if (!b.images || !out.found || !out.xy || !out.flags) return bad("NULL argument");

    const size_t ni = (size_t)b.n_img, nw = (size_t)o->cols * (size_t)o->rows;
    std::fill(out.found, out.found + ni, 0);
    std::fill(out.flags, out.flags + ni, 0);
    if (out.stats)                                        // what an image that never reaches the assembly reports
        for (size_t k = 0; k < ni; ++k) { out.stats[4 * k] = out.stats[4 * k + 1] = 0; out.stats[4 * k + 2] = out.stats[4 * k + 3] = -1; }
    const ChainShape sh = chain_shape((size_t)b.width, (size_t)b.height, b.dtype == CCAL_PIX_U16 ? 2 : 1, (size_t)o->step,
                                      (size_t)o->nms_radius, (size_t)o->cand_cap, 1, 1, 1);
    if (!sh.slots) return CCAL_OK;                        // no domain: nothing to launch
    const size_t C = sh.cand, K = std::min(C, (size_t)kBoardMaxKept);
    const size_t nc = chain_images_per_chunk(ni, board_chain_per_image_bytes(b.on_device, sh, nw),
                                             test_chunk_bytes("CCAL_TEST_BOARD_CHUNK_BYTES", kChainChunkBytes));

    CallBlock blk(ctx);
    ChainFront front; BoardSlices bs;
    front.add_ints(blk, b, sh.dom, C, nc);
    bs.add_ints(blk, C * nc, K, nc, nw, false);
    front.add_doubles(blk);                               // the doubles the kernels write before they read, from here on
    bs.add_doubles(blk);
    if (!blk.alloc()) return blk.finish(where);

    front.bind(blk, b, sh.dom, fp);
    BoardArgs a = bs.args(blk, o->cols, o->rows);
    a.off = front.ca.off; a.xy = front.ca.xy; a.hess_i = front.da.ohess; a.status = front.ca.status; a.row_cap = (int32_t)C;
    hipStream_t st = ctx->stream;
    std::vector<int32_t> h_count(nc);
    for (size_t k0 = 0; k0 < ni && blk.ok(); k0 += nc) {
        const size_t m = std::min(nc, ni - k0);
        a.n_img = (int32_t)m;
        blk.poison(front.xy, bs.oxy);                     // the test hook's NaN over the doubles the kernels write before they read
        // 1. - 3. candidates and their counts, starts, refinement; 4. - 5. the CCAL_OK corners with their Hessians into the assembly
        const size_t n_cand = front.run(blk, st, b, k0, m, h_count);
        if (!blk.ok()) break;
        for (size_t i = 0; i < m; ++i) out.flags[k0 + i] = h_count[i] > o->cand_cap ? CCAL_BOARD_FLAG_CAND_CAP : 0;
        if (!n_cand) continue;
        board_run(blk, st, a, bs.h_kept);
        if (!board_fetch(blk, st, a, bs, k0, out)) break;
        for (size_t i = 0; i < m; ++i) out.flags[k0 + i] |= bs.h_flags[i];          // the assembly's flags beside the chain's own
    }
    return blk.finish(where);
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_assemble_checkerboards_batch(ccal_ctx* ctx, int n_img, const int64_t* offsets, const double* xy, const double* hess, int cols,
                                      int rows, int32_t* found_out, double* xy_out, int32_t* idx_out, int32_t* flags_out,
                                      int32_t* stats_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return assemble_call(ctx, "ccal_assemble_checkerboards_batch", n_img, offsets, xy, hess, cols, rows,
                         BoardsOut{ found_out, xy_out, idx_out, flags_out, stats_out });
    CCAL_API_CATCH(ctx)
}

int ccal_detect_checkerboards_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images,
                                    const ccal_detect_checkerboards_opts* opts, int32_t* found_out, double* xy_out, int32_t* flags_out,
                                    int32_t* stats_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return detect_boards_call(ctx, "ccal_detect_checkerboards_batch", GreyBatch{ dtype, width, height, n_img, images, false }, opts,
                              BoardsOut{ found_out, xy_out, nullptr, flags_out, stats_out });
    CCAL_API_CATCH(ctx)
}

int ccal_detect_checkerboards_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev,
                                  const ccal_detect_checkerboards_opts* opts, int32_t* found_out, double* xy_out, int32_t* flags_out,
                                  int32_t* stats_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return detect_boards_call(ctx, "ccal_detect_checkerboards_dev", GreyBatch{ dtype, width, height, n_img, images_dev, true }, opts,
                              BoardsOut{ found_out, xy_out, nullptr, flags_out, stats_out });
    CCAL_API_CATCH(ctx)
}

}  // extern "C"
