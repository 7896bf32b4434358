// Microbenchmark: HBM read rate of the fused kernels' access shape, by cache policy.
//  1. k_read: a wavefront owns a column slice of SEG bytes (64 lanes x 4 / 8 / 16 B) and walks rows with UU row segments in
//     flight; the row pitch is 32000 B (8000 floats).  EVERY row is read -- the remainder of a wavefront's range (150 = 4 x 32 + 22)
//     goes in chunks of 16 and 8, the last one with the row index clamped -- so the rate is the whole matrix over the time whatever the rows per wavefront.
//     (Until round 6 the remainder was skipped but counted: the 150-row lines read 128 of every 150 rows and printed 7.1 TB/s for 6.1.)
//     Loads: default policy or non-temporal.
//  2. k_groups: the geometry of k_ovo_fused at C2 -- grid (125 tiles, 250 group chunks), 4 wavefronts, 2 groups of 145 rows each per
//     wavefront (128 + 16 + a clamped chunk of 8), lane = gene -- and after every group the wavefront writes three 512-B pieces into
//     three [2000][8000] float64 planes where the fused kernel would.  Stores: none / 8 B per lane plain / 8 B nt / 16 B per lane plain
//     / 16 B write-through (sc0 sc1); the 16-B forms pair neighbouring lanes (even lanes: planes 0 and 2, odd lanes: plane 1).
// Build: hipcc --offload-arch=gfx950 -O3 -o seg_bw seg_bw.hip ; run: ./seg_bw
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
template <bool NT, typename T> __device__ __forceinline__ T ld(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <int VEC, bool NT> __device__ __forceinline__ float ld_sum(const float *p) {
    if constexpr (VEC == 1) return ld<NT>(p);
    else if constexpr (VEC == 2) { const f32x2 t = ld<NT>((const f32x2 *)p); return t.x + t.y; }
    else { const f32x4 t = ld<NT>((const f32x4 *)p); return (t.x + t.y) + (t.z + t.w); }
}
// UU rows from r on; CLAMP: rows at or past r1 re-read row r1 - 1 (a cache hit)
template <int VEC, int UU, bool NT, bool CLAMP> __device__ __forceinline__ float rows(const float *X, long long ld_, long long col, int r, int r1) {
    float v[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) v[u] = ld_sum<VEC, NT>(X + (long long)(CLAMP ? min(r + u, r1 - 1) : r + u) * ld_ + col);
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < UU; ++u) acc += v[u];
    return acc;
}
template <int VEC, int UU, bool NT> __device__ __forceinline__ float row_range(const float *X, long long ld_, long long col, int r0, int r1) {
    float acc = 0.f;
    int r = r0;
    for (; r + UU <= r1; r += UU) acc += rows<VEC, UU, NT, false>(X, ld_, col, r, r1);
    if constexpr (UU > 16) { if (r + 16 <= r1) { acc += rows<VEC, 16, NT, false>(X, ld_, col, r, r1); r += 16; } }
    for (; r + 8 <= r1; r += 8) acc += rows<VEC, 8, NT, false>(X, ld_, col, r, r1);
    if (r < r1) acc += rows<VEC, 8, NT, true>(X, ld_, col, r, r1);
    return acc;
}
template <int VEC, int UU, bool NT>
__global__ __launch_bounds__(256) void k_read(const float *__restrict__ X, long long ld_, int n_rows, int rows_per_wave, float *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long col = ((long long)blockIdx.x * 64 + lane) * VEC; // column slice
    const int chunk = blockIdx.y * 4 + wave;                         // row range of this wavefront
    const int r0 = min(chunk * rows_per_wave, n_rows), r1 = min(r0 + rows_per_wave, n_rows);
    const float acc = row_range<VEC, UU, NT>(X, ld_, col, r0, r1);
    if (acc == 12345.678f) out[0] = acc;
}

enum { ST_NONE, ST_8, ST_8NT, ST_16, ST_16WT };
static const char *kStoreNames[] = {"no stores", "8 B plain", "8 B nt", "16 B plain", "16 B write-through"};
template <bool WT> __device__ __forceinline__ void store16(double *p, double x, double y) {
    f64x2 v; v.x = x; v.y = y;
    if constexpr (WT) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else *(f64x2 *)p = v;
}
template <bool NT, int ST>
__global__ __launch_bounds__(256) void k_groups(const float *__restrict__ X, long long ld_, int rows_per_group, int G, int groups_per_wg,
                                                double *p0, double *p1, double *p2, long long out_ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gene = blockIdx.x * 64 + lane;
    const int gbeg = blockIdx.y * groups_per_wg, gend = min(gbeg + groups_per_wg, G);
    for (int g = gbeg + wave; g < gend; g += 4) {
        const int r0 = g * rows_per_group;
        const float acc = row_range<1, 32, NT>(X, ld_, gene, r0, r0 + rows_per_group);
        const double a = (double)acc, b = a + 1.0, c = a + 2.0;
        const size_t o = (size_t)g * out_ld + gene;
        if constexpr (ST == ST_8) { p0[o] = a; p1[o] = b; p2[o] = c; }
        else if constexpr (ST == ST_8NT) {
            __builtin_nontemporal_store(a, p0 + o); __builtin_nontemporal_store(b, p1 + o); __builtin_nontemporal_store(c, p2 + o);
        } else if constexpr (ST == ST_16 || ST == ST_16WT) {
            const bool odd = lane & 1;
            const double r = __shfl_xor(odd ? a : b, 1), r2 = __shfl_xor(c, 1);
            if (!odd) store16<ST == ST_16WT>(p0 + o, a, r); else store16<ST == ST_16WT>(p1 + o - 1, r, b);
            if (!odd) store16<ST == ST_16WT>(p2 + o, c, r2);
        } else if (acc == 12345.678f) p0[o] = a;
    }
}

template <typename F> static float time_ms(F launch) {
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    launch();
    hipDeviceSynchronize();
    hipEventRecord(a);
    for (int i = 0; i < 5; ++i) launch();
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    hipEventDestroy(a); hipEventDestroy(b);
    return ms / 5;
}
template <int VEC, int UU, bool NT> void run(const float *X, long long ld_, int N, int M, float *out, int rows_per_wave) {
    dim3 grid(M / (64 * VEC), (N + rows_per_wave * 4 - 1) / (rows_per_wave * 4));
    const float ms = time_ms([&] { k_read<VEC, UU, NT><<<grid, 256>>>(X, ld_, N, rows_per_wave, out); });
    printf("read   segment %4d B, %2d rows in flight, %5d rows per wavefront, %-7s loads: %.3f ms  %.2f TB/s\n", VEC * 256, UU, rows_per_wave,
           NT ? "nt" : "default", ms, (double)N * M * 4 / ms / 1e9);
}
template <bool NT, int ST> void run_groups(const float *X, long long ld_, int M, double *const *pl, int G, int rpg) {
    const int gpw = 8;
    dim3 grid(M / 64, (G + gpw - 1) / gpw);
    const float ms = time_ms([&] { k_groups<NT, ST><<<grid, 256>>>(X, ld_, rpg, G, gpw, pl[0], pl[1], pl[2], (long long)M); });
    const double rd = (double)G * rpg * M * 4, wr = ST == ST_NONE ? 0.0 : 3.0 * G * M * 8;
    printf("groups %4d x %3d rows, %-7s loads, %-18s: %.3f ms  read %.2f TB/s  read + written %.2f TB/s\n", G, rpg, NT ? "nt" : "default",
           kStoreNames[ST], ms, rd / ms / 1e9, (rd + wr) / ms / 1e9);
}
template <bool NT> void run_groups_all(const float *X, long long ld_, int M, double *const *pl, int G, int rpg) {
    run_groups<NT, ST_NONE>(X, ld_, M, pl, G, rpg);
    run_groups<NT, ST_8>(X, ld_, M, pl, G, rpg);
    run_groups<NT, ST_8NT>(X, ld_, M, pl, G, rpg);
    run_groups<NT, ST_16>(X, ld_, M, pl, G, rpg);
    run_groups<NT, ST_16WT>(X, ld_, M, pl, G, rpg);
}
int main() {
    const int N = 300000, M = 8000, G = 2000, RPG = 145; const long long ld_ = M; // G x RPG = 290 000 rows of the matrix
    float *X, *out;
    double *pl[3];
    if (hipMalloc(&X, (size_t)N * M * 4) != hipSuccess || hipMalloc(&out, 4) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    for (auto &p : pl) if (hipMalloc(&p, (size_t)G * M * 8) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    hipMemset(X, 0, (size_t)N * M * 4);
    for (int rpw : {150, 1200}) {
        run<1, 32, false>(X, ld_, N, M - M % 64, out, rpw);
        run<1, 32, true>(X, ld_, N, M - M % 64, out, rpw);
        run<2, 32, false>(X, ld_, N, M - M % 128, out, rpw);
        run<2, 16, false>(X, ld_, N, M - M % 128, out, rpw);
        run<4, 16, false>(X, ld_, N, M - M % 256, out, rpw);
        run<4, 16, true>(X, ld_, N, M - M % 256, out, rpw);
        run<4, 8, false>(X, ld_, N, M - M % 256, out, rpw);
    }
    for (int rep = 0; rep < 2; ++rep) { // twice: the second block shows how steady a line is
        run_groups_all<false>(X, ld_, M, pl, G, RPG);
        run_groups_all<true>(X, ld_, M, pl, G, RPG);
    }
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "a kernel failed\n"); return 1; }
    return 0;
}
