// Welch's t-test of every ordered pair of K selected groups from the per-group moment planes -- illico_pair_ttest_from_moments
// (pair_ttest.hip; include/illico_hip_pair_ttest.h).
//
// Cell [r][g][j] of a [K][K][out_ld] plane is group sel[g] against reference sel[r] in column j.  t, df and p of a cell are the bits
// k_ttest_from_moments (kernels_ttest.h, whose head states the formula) writes for group sel[g] with ref = sel[r]: the same operations
// in the same order, the tail through tt_pvalue.  The effect planes, each step one float64 operation:
//     fold_change = (F1 / n1) / (F2 / n2)              inf where F2 / n2 == 0          (F: fsum, or S without it)
//     cohen_d     = (m1 - m2) / sqrt(0.5 * (v1 + v2))  NaN -> 0, +-inf kept, 0 on the diagonal
// The diagonal is that kernel's reference row: (t, p) = (0, 1), df what the formula gives for a group against itself.
//
// A group's m = S / n, v = q / (n - 1), a = v / n and fold mean F / n are formed ONCE per (group, gene) of a workgroup and held in LDS:
// a workgroup takes PT_TILE genes and the pairs between two tiles of PT_GT groups (I <= J), its PT_NT / 64 wavefronts the pairs of
// that block in turn (those of index z, z + Z, ... with the launch's split Z = gridDim.z * wavefronts); a lane is one gene, so that
// the loads of S / Q and the stores of a plane row are contiguous.
//
// ILLICO_TT_WELCH evaluates the tail once per unordered pair {g, r} and writes both cells from it: a + b and the denominator of df are
// commutative sums, so sqrt(a + b), df and the two-sided tail are the bits of a direct evaluation of the mirrored cell.  Its t is
// (m2 - m1) / sqrt(a + b), formed by its own subtraction and division (not -t: for equal means both differences are +0), and its
// one-sided p follows from the same two-sided tail through the last line of tt_pvalue.  ILLICO_TT_OVERESTIM_VAR divides the reference's
// variance by the GROUP's size: it is not symmetric and evaluates every ordered pair.
#pragma once
#include "kernels_ttest.h"

#define PT_NT 256   // threads of a workgroup: four wavefronts
#define PT_TILE 64  // genes of a workgroup: one per lane
#define PT_GT 8     // groups of a tile
#define PT_N_OUT 5
#define PT_MAX_SPLIT 16 // gridDim.z at most: 4 * 16 = PT_GT * PT_GT wavefronts, one pair each

struct PtParams {
    const double *S, *Q, *F; // [G][in_ld]; F null: the fold change from S
    long long in_ld;
    double *out[PT_N_OUT];   // p, t, df, fold_change, cohen_d: [K][K][out_ld] or null
    long long out_ld;
    const int *counts;       // [G]
    const int *sel;          // [K]
    int K, W, n_tiles, variant, alternative;
};

enum { PT_M, PT_V, PT_A, PT_FM, PT_FIELDS };

// one cell from the shared quantities of its two groups; `tail` false: the diagonal, or the mirrored Welch cell whose two-sided tail p2
// is given
struct PtCell { double p, t, df, fc, d; };

__device__ __forceinline__ double pt_side(double p2, double t, int alternative) { // tt_pvalue's last line, from a tail that is known
    if (alternative == ILLICO_ALT_TWO_SIDED) return p2;
    const double u = alternative == ILLICO_ALT_GREATER ? t : -t;
    return u >= 0.0 ? 0.5 * p2 : 1.0 - 0.5 * p2;
}

__device__ __forceinline__ void pt_store(const PtParams &P, int r, int g, int j, const PtCell &c) {
    const size_t q = ((size_t)r * P.K + g) * (size_t)P.out_ld + j;
    const double vals[PT_N_OUT] = {c.p, c.t, c.df, c.fc, c.d};
#pragma unroll
    for (int k = 0; k < PT_N_OUT; ++k)
        if (P.out[k]) P.out[k][q] = vals[k];
}

// grid (ceil(W / PT_TILE), n_tiles (n_tiles + 1) / 2, split)
static __global__ __launch_bounds__(PT_NT) void k_pair_ttest(PtParams P) {
    __shared__ double sh[2][PT_FIELDS][PT_GT][PT_TILE];
    __shared__ double sh_n[2][PT_GT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * PT_TILE + lane;
    const bool live = j < P.W;
    // the tile pair (I, J), I <= J, of blockIdx.y: row I of the upper triangle holds n_tiles - I of them
    int I = 0, J = (int)blockIdx.y;
    while (J >= P.n_tiles - I) { J -= P.n_tiles - I; ++I; }
    J += I;
    const int nI = min(PT_GT, P.K - I * PT_GT), nJ = min(PT_GT, P.K - J * PT_GT);
    const bool same = I == J;

    // ---- a group's quantities, once per (group, gene): slot s = side * PT_GT + local group
    for (int s = wave; s < (same ? PT_GT : 2 * PT_GT); s += PT_NT / 64) {
        const int side = s / PT_GT, l = s % PT_GT;
        if (l >= (side ? nJ : nI)) continue;
        const int grp = P.sel[(side ? J : I) * PT_GT + l];
        const double n = (double)P.counts[grp];
        if (lane == 0) sh_n[side][l] = n;
        if (!live) continue;
        const size_t o = (size_t)grp * P.in_ld + j;
        const double S1 = P.S[o], Q1 = P.Q[o];
        const double m = S1 / n;
        double q = Q1 - S1 * m;
        if (q < 0.0) q = 0.0;
        const double v = q / (n - 1.0);
        sh[side][PT_M][l][lane] = m;
        sh[side][PT_V][l][lane] = v;
        sh[side][PT_A][l][lane] = v / n;
        sh[side][PT_FM][l][lane] = P.F ? P.F[o] / n : m;
    }
    __syncthreads();
    if (!live) return;

    const int sj = same ? 0 : 1;
    const int slot = (int)blockIdx.z * (PT_NT / 64) + wave, n_slots = (int)gridDim.z * (PT_NT / 64);
    const bool welch = P.variant != ILLICO_TT_OVERESTIM_VAR;
    const bool want_d = P.out[4] != nullptr, want_fc = P.out[3] != nullptr;
    int turn = 0; // the block's pairs in order, dealt to the wavefronts of the split
    for (int gi = 0; gi < nI; ++gi) {
        for (int rj = same ? gi : 0; rj < nJ; ++rj, ++turn) {
            if (turn % n_slots != slot) continue;
            const int g = I * PT_GT + gi, r = J * PT_GT + rj;
            const bool diag = same && gi == rj;
            const double n1 = sh_n[0][gi], n2 = sh_n[sj][rj];
            const double m1 = sh[0][PT_M][gi][lane], m2 = sh[sj][PT_M][rj][lane];
            const double a1 = sh[0][PT_A][gi][lane], a2 = sh[sj][PT_A][rj][lane];
            double d12 = 0.0, d21 = 0.0, fc12 = 0.0, fc21 = 0.0;
            if (want_d && !diag) {
                const double sd = sqrt(0.5 * (sh[0][PT_V][gi][lane] + sh[sj][PT_V][rj][lane]));
                d12 = (m1 - m2) / sd;
                d21 = (m2 - m1) / sd;
                if (d12 != d12) d12 = 0.0;
                if (d21 != d21) d21 = 0.0;
            }
            if (want_fc) {
                const double f1 = sh[0][PT_FM][gi][lane], f2 = sh[sj][PT_FM][rj][lane];
                fc12 = f2 == 0.0 ? __longlong_as_double(0x7FF0000000000000ll) : f1 / f2;
                fc21 = f1 == 0.0 ? __longlong_as_double(0x7FF0000000000000ll) : f2 / f1;
            }
            // cell [r][g]: group g against reference r
            PtCell c;
            double a = a1, b = welch ? a2 : sh[sj][PT_V][rj][lane] / n1;
            const double n2p = welch ? n2 : n1;
            double s = sqrt(a + b);
            c.t = (m1 - m2) / s;
            c.df = ((a + b) * (a + b)) / (a * a / (n1 - 1.0) + b * b / (n2p - 1.0));
            if (c.df != c.df) c.df = 1.0;
            const bool dead = c.t != c.t || diag;
            double p2 = 1.0;
            if (dead) { c.t = 0.0; c.p = 1.0; }
            else if (welch) { p2 = tt_pvalue(c.t, c.df, ILLICO_ALT_TWO_SIDED); c.p = pt_side(p2, c.t, P.alternative); }
            else c.p = tt_pvalue(c.t, c.df, P.alternative);
            c.fc = fc12; c.d = d12;
            pt_store(P, r, g, j, c);
            if (diag) continue;
            // cell [g][r]: group r against reference g
            PtCell e;
            if (welch) {
                e.t = (m2 - m1) / s;
                e.df = c.df;
                if (dead) { e.t = 0.0; e.p = 1.0; }
                else e.p = pt_side(p2, e.t, P.alternative);
            } else {
                a = a2; b = sh[0][PT_V][gi][lane] / n2;
                s = sqrt(a + b);
                e.t = (m2 - m1) / s;
                e.df = ((a + b) * (a + b)) / (a * a / (n2 - 1.0) + b * b / (n2 - 1.0));
                if (e.df != e.df) e.df = 1.0;
                if (e.t != e.t) { e.t = 0.0; e.p = 1.0; }
                else e.p = tt_pvalue(e.t, e.df, P.alternative);
            }
            e.fc = fc21; e.d = d21;
            pt_store(P, g, r, j, e);
        }
    }
}
