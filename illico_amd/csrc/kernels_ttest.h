// Welch's t-test from per-group moments -- illico_ttest_from_moments / illico_student_t_pvalues (group_moments.hip).
//
// From a group's (n1, S1 = sum x, Q1 = sum x^2) and its reference's (n2, S2, Q2) -- the reference group's row in one-versus-one, the
// rest planes in one-versus-rest -- every step ONE IEEE float64 operation, in this order (the build is -ffp-contract=off, a numpy
// restatement gives the same bits):
//     m1 = S1 / n1                  m2 = S2 / n2
//     q1 = Q1 - S1 * m1             q2 = Q2 - S2 * m2        (q < 0 -> 0; NaN stays NaN)
//     v1 = q1 / (n1 - 1)            v2 = q2 / (n2 - 1)        (n = 1: 0 / 0 -> NaN)
//     n2' = n1 for ILLICO_TT_OVERESTIM_VAR, else n2
//     a = v1 / n1                   b = v2 / n2'
//     t  = (m1 - m2) / sqrt(a + b)
//     df = ((a + b) * (a + b)) / (a * a / (n1 - 1) + b * b / (n2' - 1));   NaN -> 1   (as scipy)
// This is scanpy's form; the variance carries a relative error of about 2^-52 (1 + mean^2 / var).  A NaN t (0 / 0, n = 1, NaN input)
// gives (t, p) = (0, 1); t = +-inf (no variance on either side, different means) is kept and p follows from it.
//
// Student's t tail in float64: the two-sided tail is I_x(a, 1/2), a = df / 2, x = df / (df + t^2), by the continued fraction of the
// incomplete beta function (modified Lentz), on the side where it converges fast: directly while y = 1 - x = t^2 / (df + t^2) is
// beyond 1.5 / (a + 2.5), as 1 - I_y(1/2, a) below.  Three roundings are designed out:
//   * the prefactor x^a y^(1/2) / B(a, 1/2) takes ln x as -log1p(t^2 / df) and Gamma(a + 1/2) / Gamma(a) from its asymptotic series
//     (a >= 30; below, the series at a + N and N exact ratio steps): no difference of two lgamma values;
//   * on the direct side x is close to 1 for large df and every odd coefficient of the fraction close to -1; the coefficients are held
//     as -1 + eps with eps = delta_m + y - delta_m y formed from y, and the recurrences are written in eps and in the even steps'
//     small terms, so that 1 - x is never formed by subtraction (tt_cf_direct);
//   * nothing takes log(1 - y) with y near 1.
// An evaluation that has not converged after TT_CF_CAP steps returns NaN.
#pragma once
#include "common.h"

#define TT_NT 256
#define TT_N_OUT 7
#define TT_CF_CAP 2000 // steps of the continued fraction at most: df = 4.2e6 at the switch between its two sides takes about 40
#define TT_TINY 1e-300

struct TtParams {
    const double *S, *Q, *SR, *QR; // [G][in_ld]; SR / QR: one-versus-rest
    long long in_ld;
    double *out[TT_N_OUT];         // p, t, df, mean, var, mean_ref, var_ref: [G][out_ld] or null
    long long out_ld;
    const int *counts;             // [G]
    long long n_cells;
    int G, W, ref, variant, alternative;
};

__device__ __forceinline__ double tt_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double tt_guard(double v) { return fabs(v) < TT_TINY ? TT_TINY : v; }

// I_y(1/2, a) / (prefactor / (1/2)): Lentz on the coefficients of the incomplete beta function with first parameter 1/2
__device__ inline double tt_cf_complement(double a, double y) {
    const double p = 0.5, qab = p + a, qap = p + 1.0, qam = p - 1.0;
    double c = 1.0, d = 1.0 / tt_guard(1.0 - qab * y / qap), h = d;
    for (int m = 1; m <= TT_CF_CAP; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (a - m) * y / ((qam + m2) * (p + m2));
        d = 1.0 / tt_guard(1.0 + aa * d);
        c = tt_guard(1.0 + aa / c);
        h *= d * c;
        aa = -(p + m) * (qab + m) * y / ((p + m2) * (qap + m2));
        d = 1.0 / tt_guard(1.0 + aa * d);
        c = tt_guard(1.0 + aa / c);
        const double de = d * c;
        h *= de;
        if (fabs(de - 1.0) < 2e-16) return h;
    }
    return tt_nan();
}
// I_x(a, 1/2) / (prefactor / a), x = 1 - y: the odd coefficients as -1 + eps (see above)
__device__ inline double tt_cf_direct(double a, double x, double y) {
    double e = 0.5 / (a + 1.0);
    e = e + y - e * y;
    double d = 1.0 / e, c = 1.0, h = d;
    for (int m = 1; m <= TT_CF_CAP; ++m) {
        const double m2 = 2.0 * m;
        const double ae = m * (0.5 - m) * x / ((a - 1.0 + m2) * (a + m2));
        const double nd = ae * d, nc = ae / c;
        h *= (1.0 + nc) / (1.0 + nd);
        const double dl = (a * (m2 + 0.5) + (3.0 * m * m + 1.5 * m)) / ((a + m2) * (a + 1.0 + m2));
        e = dl + y - dl * y;
        d = (1.0 + nd) / (nd + e);
        c = (nc + e) / (1.0 + nc);
        const double de = d * c;
        h *= de;
        if (fabs(de - 1.0) < 2e-16) return h;
    }
    return tt_nan();
}
// the two-sided tail P(|T| > |t|) of Student's t with df degrees of freedom (df > 0, finite)
__device__ inline double tt_two_sided(double t, double df) {
    t = fabs(t);
    if (!(t < __longlong_as_double(0x7FF0000000000000ll))) return t != t ? tt_nan() : 0.0;
    const double t2 = t * t, a = 0.5 * df, s = df + t2, y = t2 / s, x = df / s;
    if (!(t2 < __longlong_as_double(0x7FF0000000000000ll))) return 0.0;
    // Gamma(a + 1/2) / Gamma(a) = sqrt(A) exp(series(A)) prod_{k < N} (a + k) / (a + k + 1/2), A = a + N >= 30
    double num = 1.0, den = 1.0, A = a;
    while (A < 30.0) { num *= A; den *= A + 0.5; A += 1.0; }
    const double i = 1.0 / A, i2 = i * i;
    const double ser = i * (-1.0 / 8.0 + i2 * (1.0 / 192.0 + i2 * (-1.0 / 640.0 + i2 * (17.0 / 14336.0))));
    const double pre = exp(ser - a * log1p(t2 / df)) * sqrt(A * y / 3.141592653589793) * (num / den); // x^a y^(1/2) / B(a, 1/2)
    if (x < (a + 1.0) / (a + 2.5)) return pre * tt_cf_direct(a, x, y) / a;
    return 1.0 - pre * tt_cf_complement(a, y) / 0.5;
}
// scipy.stats.t.sf-based p of an alternative: two-sided 2 sf(|t|), greater sf(t), less sf(-t)
__device__ inline double tt_pvalue(double t, double df, int alternative) {
    const double p2 = tt_two_sided(t, df);
    if (alternative == ILLICO_ALT_TWO_SIDED) return p2;
    const double u = alternative == ILLICO_ALT_GREATER ? t : -t;
    return u >= 0.0 ? 0.5 * p2 : 1.0 - 0.5 * p2;
}

// grid (ceil(W / 256), groups): thread = one gene of the groups blockIdx.y, blockIdx.y + gridDim.y, ...
static __global__ __launch_bounds__(TT_NT) void k_ttest_from_moments(TtParams P) {
    const int j = blockIdx.x * TT_NT + threadIdx.x;
    if (j >= P.W) return;
    const bool ovr = P.ref < 0;
    for (int g = blockIdx.y; g < P.G; g += gridDim.y) {
        const size_t o = (size_t)g * P.in_ld + j, r = ovr ? o : (size_t)P.ref * P.in_ld + j;
        const double n1 = (double)P.counts[g], n2 = ovr ? (double)(P.n_cells - P.counts[g]) : (double)P.counts[P.ref];
        const double S1 = P.S[o], Q1 = P.Q[o], S2 = ovr ? P.SR[r] : P.S[r], Q2 = ovr ? P.QR[r] : P.Q[r];
        const double m1 = S1 / n1, m2 = S2 / n2;
        double q1 = Q1 - S1 * m1, q2 = Q2 - S2 * m2;
        if (q1 < 0.0) q1 = 0.0;
        if (q2 < 0.0) q2 = 0.0;
        const double v1 = q1 / (n1 - 1.0), v2 = q2 / (n2 - 1.0);
        const double n2p = P.variant == ILLICO_TT_OVERESTIM_VAR ? n1 : n2;
        const double a = v1 / n1, b = v2 / n2p;
        double t = (m1 - m2) / sqrt(a + b);
        double df = ((a + b) * (a + b)) / (a * a / (n1 - 1.0) + b * b / (n2p - 1.0));
        if (df != df) df = 1.0;
        double p;
        if (t != t || (!ovr && g == P.ref)) { t = 0.0; p = 1.0; }
        else p = tt_pvalue(t, df, P.alternative);
        const size_t q = (size_t)g * P.out_ld + j;
        const double vals[TT_N_OUT] = {p, t, df, m1, v1, m2, v2};
#pragma unroll
        for (int k = 0; k < TT_N_OUT; ++k)
            if (P.out[k]) P.out[k][q] = vals[k];
    }
}

static __global__ __launch_bounds__(TT_NT) void k_student_t_pvalues(const double *__restrict__ t, const double *__restrict__ df, long long n, int alternative,
                                                                   double *__restrict__ out_p) {
    const long long i = (long long)blockIdx.x * TT_NT + threadIdx.x;
    if (i < n) out_p[i] = tt_pvalue(t[i], df[i], alternative);
}
