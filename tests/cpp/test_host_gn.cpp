// The host Gauss-Newton kit of the small factors (csrc/ccal_host_gn.hpp) on the host alone - plain C++, no HIP call; run under the
// host's address and undefined-behaviour sanitizers by tests/test_host_gn_cpu.py.
//   Cholesky     A = L L^T from small integer L and b = A x from integer x: every intermediate is an integer, so factor and solution
//                are exact in doubles and compared for equality; pivots that are zero, negative, NaN or +inf give false; a 9 x 9
//                system with identity rows 7 and 8 and rhs 0 there (convert's fixed mask) gives exactly 0 for those unknowns
//   huber_weight exactly 1 up to s == delta^2, delta / sqrt(s) above
//   stop rule    a table of (last, cur, options) rows with the outcome worked out by hand, against gn_decide AND against a verbatim
//                copy of the if-ladder both loops carried before the kit
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_host_gn.hpp"

using namespace ccal;

static int bad(const char* what, int i = -1) { std::printf("GN-FAIL %s %d\n", what, i); return 1; }

static std::vector<double> int_lower(int n) {
    std::vector<double> L((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < i; ++j) L[i * n + j] = (double)((i * 7 + j * 3) % 5 - 2);
        L[i * n + i] = (double)(1 + i % 3);
    }
    return L;
}
static std::vector<double> llt(const std::vector<double>& L, int n) {
    std::vector<double> A((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) for (int k = 0; k < n; ++k) A[i * n + j] += L[i * n + k] * L[j * n + k];
    return A;
}
static bool exact_case(int n) {
    const std::vector<double> L = int_lower(n);
    std::vector<double> A = llt(L, n), x((size_t)n), b((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) x[i] = (double)(i % 4 - 1);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) b[i] += A[i * n + j] * x[j];
    if (!chol_factor(A.data(), n)) return false;
    for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) if (A[i * n + j] != L[i * n + j]) return false;
    chol_solve(A.data(), n, b.data());
    for (int i = 0; i < n; ++i) if (b[i] != x[i]) return false;
    return true;
}
static bool masked_case() {
    const int m = 7, n = 9;
    const std::vector<double> A7 = llt(int_lower(m), m);
    std::vector<double> A((size_t)n * n, 0.0), b((size_t)n, 0.0), x((size_t)m);
    for (int i = 0; i < m; ++i) { x[i] = (double)(2 - i % 5); for (int j = 0; j < m; ++j) A[i * n + j] = A7[i * m + j]; }
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) b[i] += A7[i * m + j] * x[j];
    A[7 * n + 7] = 1.0; A[8 * n + 8] = 1.0;
    if (!chol_factor(A.data(), n)) return false;
    chol_solve(A.data(), n, b.data());
    for (int i = 0; i < m; ++i) if (b[i] != x[i]) return false;
    return b[7] == 0.0 && b[8] == 0.0;
}

// the ladder as ccal_convert_model and ccal_init_camera_extrinsic_opts each had it: 0 continue, 1 stop (break), 2 non-finite
static int parent_ladder(double last, double cur, int em, double min_err, double min_abs, double min_rel) {
    const double le = em ? std::sqrt(std::max(last, 0.0)) : last, ce = em ? std::sqrt(std::max(cur, 0.0)) : cur;
    if (ce < min_err) return 1;
    if (std::isnan(cur)) return 2;
    if (std::fabs(le - ce) < min_abs) return 1;
    if (std::fabs(le - ce) / le < min_rel) return 1;
    return 0;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int n : { 1, 6, 9 }) if (!exact_case(n)) return bad("exact factor and solve", n);
    if (!masked_case()) return bad("fixed mask");
    {
        double z1[1] = { 0.0 }, z2[4] = { 1, 1, 1, 1 }, neg1[1] = { -4.0 }, neg2[4] = { 1, 2, 2, 1 }, nan1[1] = { nan }, nan2[4] = { 1, nan, nan, 1 },
               inf1[1] = { inf }, inf2[4] = { 1, 0, 0, inf }, ninf[1] = { -inf };
        if (chol_factor(z1, 1) || chol_factor(z2, 2)) return bad("zero pivot");
        if (chol_factor(neg1, 1) || chol_factor(neg2, 2) || chol_factor(ninf, 1)) return bad("negative pivot");
        if (chol_factor(nan1, 1) || chol_factor(nan2, 2)) return bad("NaN entry");
        if (chol_factor(inf1, 1) || chol_factor(inf2, 2)) return bad("+inf pivot");
    }
    for (double delta : { 0.5, 1.0 }) {
        const double d2 = delta * delta;
        if (huber_weight(0.0, delta) != 1.0 || huber_weight(0.5 * d2, delta) != 1.0 || huber_weight(d2, delta) != 1.0) return bad("huber_weight inside");
        // (just above delta^2 the quotient may round to 1: the formula is what is held there, the value below 1 from 2 delta^2 on)
        for (double s : { std::nextafter(d2, 2.0), 2.0 * d2, 9.0, 1e300 })
            if (huber_weight(s, delta) != delta / std::sqrt(s) || (s >= 2.0 * d2 && !(huber_weight(s, delta) < 1.0))) return bad("huber_weight outside");
    }
    // tiny-solver's defaults: min_error 1e-10, min_abs 1e-5, min_rel 1e-5
    struct Row { double last, cur; int em; double min_err, min_abs, min_rel; int want; };
    const Row rows[] = {
        { 10.0, 5.0, 0, 1e-10, 1e-5, 1e-5, 0 },            // a plain decrease: continue
        { 10.0, 5.0, 1, 1e-10, 1e-5, 1e-5, 0 },
        { 10.0, 1e-11, 0, 1e-10, 1e-5, 1e-5, 1 },          // below min_error
        { 10.0, 1e-11, 1, 1e-10, 1e-5, 1e-5, 0 },          // ... whose norm, 3.2e-6, is not
        { 10.0, 1e-21, 1, 1e-10, 1e-5, 1e-5, 1 },
        { 10.0, nan, 0, 1e-10, 1e-5, 1e-5, 2 },            // cur NaN
        { 10.0, nan, 1, 1e-10, 1e-5, 1e-5, 2 },
        { nan, 5.0, 0, 1e-10, 1e-5, 1e-5, 0 },             // last NaN: every comparison is false
        { nan, 1e-12, 0, 1e-10, 1e-5, 1e-5, 1 },
        { 10.0, 10.0 - 1e-6, 0, 1e-10, 1e-5, 1e-5, 1 },    // absolute decrease
        { 1e6, 1e6 - 1.0, 0, 1e-10, 1e-5, 1e-5, 1 },       // relative decrease 1e-6 (absolute 1: not that test)
        { 1e6, 1e6 - 1.0, 0, 1e-10, 1e-5, 1e-7, 0 },
        { 1e6, 1e6 - 1.0, 1, 1e-10, 1e-5, 1e-5, 1 },       // norms 1000 and 999.9995: relative 5e-7
        { 1e6, 1e6 - 100.0, 1, 1e-10, 1e-5, 1e-5, 0 },     // norms differ by 0.05: relative 5e-5
        { 4.0, 4.0 - 2e-5, 1, 1e-10, 1e-5, 1e-5, 1 },      // norms differ by 5e-6: absolute
        { 4.0, 4.0 - 2e-5, 0, 1e-10, 1e-5, 1e-5, 1 },      // squared: 2e-5 is not below 1e-5, relative 5e-6 is
        { 10.0, 20.0, 0, 1e-10, 1e-5, 1e-5, 0 },           // an increase is a change like any other
        { 10.0, inf, 0, 1e-10, 1e-5, 1e-5, 0 },            // inf is not NaN: the ladder goes on
        { 0.0, 0.5, 0, 1e-10, 1e-5, 1e-5, 0 },             // last == 0: 0.5 / 0 = inf
        { 0.0, 0.5, 1, 1e-10, 1e-5, 1e-5, 0 },
        { 0.0, 0.0, 0, 0.0, 0.0, 1e-5, 0 },                // last == 0 == cur with the first tests off: 0 / 0 = NaN falls through
        { 0.0, 0.0, 0, 1e-10, 1e-5, 1e-5, 1 },
        { -1.0, -4.0, 1, 1e-10, 1e-5, 1e-5, 1 },           // negative costs under the norm: both read 0
        { -1.0, -4.0, 1, 0.0, 1e-5, 1e-5, 1 },             // ... min_error off: the absolute test, |0 - 0|
        { -1.0, -4.0, 1, 0.0, 0.0, 1e-5, 0 },              // ... that off too: 0 / 0
        { -1.0, -4.0, 0, 0.0, 0.0, 1e-5, 1 },              // squared norm: -4 < 0 = min_error
        { 9.0, -4.0, 1, 0.0, 1e-5, 1e-5, 0 },              // norm 3 -> 0
        { -1.0, 4.0, 1, 1e-10, 1e-5, 1e-5, 0 },            // norm 0 -> 2: 2 / 0 = inf
    };
    int i = 0;
    for (const Row& r : rows) {
        const int ref = parent_ladder(r.last, r.cur, r.em, r.min_err, r.min_abs, r.min_rel);
        const GnNext got = gn_decide(r.last, r.cur, r.em, r.min_err, r.min_abs, r.min_rel);
        const int g = got == GnNext::go_on ? 0 : got == GnNext::stop ? 1 : 2;
        if (ref != r.want) return bad("stop rule: the table's outcome against the ladder", i);
        if (g != ref) return bad("stop rule: gn_decide against the ladder", i);
        ++i;
    }
    std::printf("GN-OK %d\n", i);
    return 0;
}
