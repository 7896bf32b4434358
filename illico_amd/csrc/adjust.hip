// illico_adjust_pvalues: per-row Benjamini-Hochberg / Benjamini-Yekutieli / Bonferroni adjustment of a p-value plane and the row's
// top-n columns (kernels_adjust.h).  A translation unit of its own: the kernels depend on nothing the Wilcoxon routes use.
#include "engine.h"
#include "kernels_adjust.h"

static int64_t next_pow2(int64_t x) {
    int64_t n = 1;
    while (n < x) n <<= 1;
    return n;
}

// c_m = sum_{i <= m} 1 / i summed as numpy sums a float64 array (scipy's np.sum(1 / i)): pairwise within blocks of 8192 elements (its
// reduction buffer), eight accumulators below 128 elements, the block sums added in order
static double pairwise_inv(int64_t lo, int64_t n) {
    if (n < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < n; ++i) r += 1.0 / (double)(lo + i);
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = 1.0 / (double)(lo + j);
        int64_t i = 8;
        for (; i < n - n % 8; i += 8)
            for (int j = 0; j < 8; ++j) r[j] += 1.0 / (double)(lo + i + j);
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += 1.0 / (double)(lo + i);
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_inv(lo, n2) + pairwise_inv(lo + n2, n - n2);
}
static double harmonic(int64_t m) {
    double acc = 0.0;
    for (int64_t s = 0; s < m; s += 8192) {
        const double v = pairwise_inv(1 + s, std::min<int64_t>(8192, m - s));
        acc = s == 0 ? v : acc + v;
    }
    return acc;
}

// the first invalid p of rows [row0, row0 + nb) (p points at row row0): ILLICO_ERR_ARG naming it, or OK.  score: the first NaN of a
// score plane (illico_top_by_score)
static int adj_validate(illico_ctx *c, const double *p, int64_t ld, int64_t nb, int64_t m, int64_t row0, u64 *d_err, const double *host_p,
                        int64_t host_ld, bool score = false) {
    HIPCHK(c, hipMemsetAsync(d_err, 0xFF, 8, c->stream));
    {
        ProfScope ps(c, score ? KID_TOP_VALIDATE : KID_ADJ_VALIDATE);
        const int gx = (int)std::min<int64_t>((m + 255) / 256, 64);
        for (int64_t r = 0; r < nb; r += 65535) {
            const int ny = (int)std::min<int64_t>(65535, nb - r);
            KERNELCHK(c, score ? k_top_validate : k_adj_validate, dim3(gx, ny), dim3(256), 0, p + r * ld, (long long)ld, (int)m, (long long)(row0 + r), d_err);
        }
    }
    u64 err = 0;
    HIPCHK(c, hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (err == ~0ull) return ILLICO_OK;
    const int64_t r = (int64_t)(err / (u64)m), col = (int64_t)(err % (u64)m);
    double v = 0.0;
    if (host_p) v = host_p[r * host_ld + col];
    else HIPCHK(c, hipMemcpy(&v, p + (r - row0) * ld + col, 8, hipMemcpyDeviceToHost));
    if (score) return fail(c, ILLICO_ERR_ARG, "score at (row %lld, column %lld) is NaN", (long long)r, (long long)col);
    return fail(c, ILLICO_ERR_ARG, "p-value at (row %lld, column %lld) is %.17g: p-values must lie in [0, 1]", (long long)r, (long long)col, v);
}

// illico_adjust_pvalues, and (score) illico_top_by_score: the same batches, sorts and merges on the keys of -x, top-n only
static int adjust_or_top(illico_ctx *c, const double *p, int64_t n_rows, int64_t n_cols, int64_t in_ld, int method, int flags,
                         double *out_adj, int64_t out_ld, int64_t n_top, int64_t *out_top, int64_t top_ld, bool score) {
    if (!c) return ILLICO_ERR_ARG;
    CTX_LOCK(c);
    if (!p) return fail(c, ILLICO_ERR_ARG, score ? "null x" : "null p");
    if (n_rows < 0 || n_cols < 0) return fail(c, ILLICO_ERR_ARG, "negative shape (%lld, %lld)", (long long)n_rows, (long long)n_cols);
    if (in_ld < n_cols) return fail(c, ILLICO_ERR_ARG, "in_ld %lld smaller than n_cols %lld", (long long)in_ld, (long long)n_cols);
    if (method != ILLICO_ADJ_BH && method != ILLICO_ADJ_BY && method != ILLICO_ADJ_BONFERRONI)
        return fail(c, ILLICO_ERR_ARG, "unknown adjustment method %d", method);
    if (n_top < 0 || n_top > n_cols) return fail(c, ILLICO_ERR_ARG, "n_top %lld outside [0, n_cols = %lld]", (long long)n_top, (long long)n_cols);
    if (!out_adj && n_top == 0) return fail(c, ILLICO_ERR_ARG, "null out_adj and n_top == 0: nothing to compute");
    if (out_adj && out_ld < n_cols) return fail(c, ILLICO_ERR_ARG, "out_ld %lld smaller than n_cols %lld", (long long)out_ld, (long long)n_cols);
    if (out_adj == p && out_ld != in_ld) return fail(c, ILLICO_ERR_ARG, "in-place adjustment needs out_ld == in_ld");
    if (n_top > 0 && (!out_top || top_ld < n_top)) return fail(c, ILLICO_ERR_ARG, "null out_top or top_ld smaller than n_top");
    if (n_cols > (int64_t)INT32_MAX - 2 * ADJ_LDS_COLS)
        return fail(c, ILLICO_ERR_UNSUPPORTED, "%lld columns: rows of up to 2^31 - %d p-values are supported", (long long)n_cols, 2 * ADJ_LDS_COLS);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = resolve_pending(c); // a plane written under ILLICO_FLAG_DEFER is complete only after its leftover genes
    if (rc) return rc;
    if (n_rows == 0 || n_cols == 0) return ILLICO_OK;

    const bool in_dev = flags & ILLICO_FLAG_INPUT_DEVICE, out_dev = flags & ILLICO_FLAG_OUTPUT_DEVICE;
    const int64_t m = n_cols;
    const bool sort = method != ILLICO_ADJ_BONFERRONI || n_top > 0, big = m > ADJ_LDS_COLS;
    // device bytes per row of a batch: the staged input / outputs of host planes, the two run buffers of rows beyond LDS
    const size_t b_in = in_dev ? 0 : (size_t)m * 8, b_out = (out_dev || !out_adj) ? 0 : (size_t)m * 8,
                 b_top = (out_dev || !n_top) ? 0 : (size_t)n_top * 8, b_runs = (sort && big) ? (size_t)m * 24 : 0;
    const size_t per_row = b_in + b_out + b_top + b_runs;
    int64_t rows_b = std::min<int64_t>(n_rows, 65535);
    if (per_row) rows_b = std::max<int64_t>(1, std::min<int64_t>(rows_b, (int64_t)((size_t)std::max<int64_t>(c->scratch_bytes, 1) / per_row)));
    u64 *d_err;
    if ((rc = scratch(c, "adj_err", 2, &d_err))) return rc;
    unsigned char *work = nullptr;
    if (per_row && (rc = scratch(c, "adj_work", per_row * (size_t)rows_b, &work))) return rc;
    double *d_in = (double *)work;
    double *d_out = (double *)(work + b_in * rows_b);
    long long *d_top = (long long *)(work + (b_in + b_out) * rows_b);
    u64 *run_k[2] = {(u64 *)(work + (b_in + b_out + b_top) * rows_b), (u64 *)(work + (b_in + b_out + b_top) * rows_b + (size_t)m * 8 * rows_b)};
    u32 *run_i[2] = {(u32 *)(work + (b_in + b_out + b_top) * rows_b + (size_t)m * 16 * rows_b),
                     (u32 *)(work + (b_in + b_out + b_top) * rows_b + (size_t)m * 20 * rows_b)};

    // device input is looked at whole before anything is written (in place or not, an invalid plane leaves every output untouched);
    // host input batch by batch, as it arrives (a plane larger than the scratch cap may then have earlier batches written)
    if (in_dev && (rc = adj_validate(c, p, in_ld, n_rows, m, 0, d_err, nullptr, 0, score))) return rc;
    const double cm = method == ILLICO_ADJ_BY ? harmonic(m) : 0.0;
    const int gx = (int)std::min<int64_t>((m + 255) / 256, 64);

    for (int64_t r0 = 0; r0 < n_rows; r0 += rows_b) {
        const int64_t nb = std::min<int64_t>(rows_b, n_rows - r0);
        const double *dp = p + r0 * in_ld;
        int64_t dld = in_ld;
        if (!in_dev) {
            HIPCHK(c, hipMemcpy2DAsync(d_in, (size_t)m * 8, dp, (size_t)in_ld * 8, (size_t)m * 8, (size_t)nb, hipMemcpyHostToDevice, c->stream));
            dp = d_in;
            dld = m;
            if ((rc = adj_validate(c, dp, dld, nb, m, r0, d_err, p, in_ld, score))) return rc;
        }
        double *dout = out_adj ? (out_dev ? out_adj + r0 * out_ld : d_out) : nullptr;
        const int64_t dold = out_dev ? out_ld : m;
        long long *dtop = n_top ? (out_dev ? (long long *)out_top + r0 * top_ld : d_top) : nullptr;
        const int64_t dtld = out_dev ? top_ld : n_top;

        if (sort) {
            AdjParams P{};
            P.p = dp;
            P.in_ld = dld;
            P.m = (int)m;
            P.method = method == ILLICO_ADJ_BONFERRONI || !dout ? ADJ_M_NONE : method == ILLICO_ADJ_BY ? ADJ_M_BY : ADJ_M_BH;
            P.cm = cm;
            P.out = P.method == ADJ_M_NONE ? nullptr : dout;
            P.out_ld = dold;
            P.top = dtop;
            P.top_ld = dtld;
            P.n_top = (int)n_top;
            if (!big) {
                P.n2 = (int)std::max<int64_t>(128, next_pow2(m));
                const int nt = std::min(1024, P.n2 / 2);
                const size_t lds = (size_t)P.n2 * 12 + 16 * 8;
                ProfScope ps(c, score ? KID_TOP_SORT : KID_ADJ_SORT);
                KERNELCHK(c, score ? k_top_sort_lds<true> : k_adj_sort_lds<true>, dim3(1, (int)nb), dim3(nt), lds, P);
            } else {
                // runs of ADJ_LDS_COLS sorted in LDS, merged pairwise through HBM, then scanned row by row
                P.n2 = ADJ_LDS_COLS;
                P.skey = run_k[0];
                P.sidx = run_i[0];
                const size_t lds = (size_t)P.n2 * 12 + 16 * 8;
                {
                    ProfScope ps(c, score ? KID_TOP_SORT : KID_ADJ_SORT);
                    KERNELCHK(c, score ? k_top_sort_lds<false> : k_adj_sort_lds<false>, dim3((int)((m + ADJ_LDS_COLS - 1) / ADJ_LDS_COLS), (int)nb), dim3(1024), lds, P);
                }
                int cur = 0;
                for (int64_t w = ADJ_LDS_COLS; w < m; w *= 2, cur ^= 1) {
                    ProfScope ps(c, score ? KID_TOP_MERGE : KID_ADJ_MERGE);
                    KERNELCHK(c, k_adj_merge, dim3((int)((m + 255) / 256), (int)nb), dim3(256), 0, run_k[cur], run_i[cur], run_k[cur ^ 1], run_i[cur ^ 1], (int)m, (int)w);
                }
                P.skey = run_k[cur];
                P.sidx = run_i[cur];
                ProfScope ps(c, score ? KID_TOP_SCAN : KID_ADJ_SCAN);
                KERNELCHK(c, k_adj_scan, dim3(1, (int)nb), dim3(ADJ_SCAN_NT), 0, P);
            }
        }
        if (method == ILLICO_ADJ_BONFERRONI && dout) { // (after the sort, which reads the input: in place, this overwrites it)
            ProfScope ps(c, KID_ADJ_BONF);
            KERNELCHK(c, k_adj_bonferroni, dim3(gx, (int)nb), dim3(256), 0, dp, (long long)dld, (int)m, dout, (long long)dold);
        }
        if (!out_dev) {
            if (out_adj)
                HIPCHK(c, hipMemcpy2DAsync(out_adj + r0 * out_ld, (size_t)out_ld * 8, d_out, (size_t)m * 8, (size_t)m * 8, (size_t)nb,
                                           hipMemcpyDeviceToHost, c->stream));
            if (n_top)
                HIPCHK(c, hipMemcpy2DAsync(out_top + r0 * top_ld, (size_t)top_ld * 8, d_top, (size_t)n_top * 8, (size_t)n_top * 8, (size_t)nb,
                                           hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream)); // (the staging buffers are reused by the next batch)
        }
    }
    return ILLICO_OK;
}

extern "C" int illico_adjust_pvalues(illico_ctx *c, const double *p, int64_t n_rows, int64_t n_cols, int64_t in_ld, int method, int flags,
                                     double *out_adj, int64_t out_ld, int64_t n_top, int64_t *out_top, int64_t top_ld) {
    return adjust_or_top(c, p, n_rows, n_cols, in_ld, method, flags, out_adj, out_ld, n_top, out_top, top_ld, false);
}

extern "C" int illico_top_by_score(illico_ctx *c, const double *x, int64_t n_rows, int64_t n_cols, int64_t in_ld, int flags, int64_t n_top,
                                   int64_t *out_top, int64_t top_ld) {
    if (!c) return ILLICO_ERR_ARG;
    if (n_top < 1 && n_rows > 0 && n_cols > 0) return fail(c, ILLICO_ERR_ARG, "n_top %lld: at least 1 is needed", (long long)n_top);
    // method ADJ_M_NONE through "no out_adj": only the order and the top-n are formed (the sort kernels' FINAL path and k_adj_scan)
    return adjust_or_top(c, x, n_rows, n_cols, in_ld, ILLICO_ADJ_BH, flags, nullptr, 0, n_top, out_top, top_ld, true);
}
