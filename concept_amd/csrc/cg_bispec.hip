// cg_bispec.hip — the two hot loops of the bispectrum (Scoccimarro estimator).
//   k_bispec_shell   the loop of get_bispec_grid              analysis.py:2739-2778
//                    over fourier_shell_loop(skip_origin)     mesh.py:3186-3296
//                    with get_bispec_overlap_cellshell        analysis.py:2803-2982 (cg_bispec.h)
//   k_bispec_sums    the three cases of compute_bispec_value  analysis.py:2621-2689
//   k_reduce_columns the sum of the workgroups' partial sums, in a fixed tree (cg_wave.h)
// k_bispec_shell ASSIGNS the whole Fourier view of the destination (cg_ctx::four, the view
// k_powerspec_bin walks): one thread per complex element, frac x source (or frac + 0i) inside
// the reference's visited set and 0 everywhere else, so the nullified slab the reference
// starts from (get_fftw_slab(nullify=True)) needs no pass of its own.
// k_bispec_sums walks the real cells of the domain (owned layers, no padding): a workgroup
// takes rows in turn, a thread two neighbouring cells of a row at a time.  Deterministic: no
// floating-point atomics; lanes by a fixed butterfly (wave_sum_xor), waves in wave order,
// workgroups by k_reduce_columns in a fixed tree.  Compiled with -ffp-contract=off; FP64 throughout.
#include "cg_bispec.h"
#include "cg_internal.h"
#include "cg_wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 256 * 8;  // 8 workgroups per CU

__global__ __launch_bounds__(kThreads) void k_bispec_shell(
    double2 *__restrict__ dst, const double2 *__restrict__ src, int N, i64 dst_si, i64 src_si,
    i64 cp, int j0, int nj, double k_inner, double k_outer, int antialias,
    BispecShellBounds bounds) {
#pragma clang fp contract(off)
    const i64 e = (i64)blockIdx.x * kThreads + threadIdx.x;
    const i64 row = e / cp;
    if (row >= (i64)N * nj) return;
    const int kk = (int)(e - row * cp);
    const int a = (int)(row / nj), bl = (int)(row - (i64)a * nj), b = j0 + bl;
    const int nyq = N / 2;
    const i64 ki = a - (a >= nyq ? N : 0), kj = b - (b >= nyq ? N : 0);
    double2 out = make_double2(0.0, 0.0);
    i64 kk_bgn, kk_end;
    // (a == nyq gives ki = -nyq, b == nyq gives kj = -nyq: beyond k_max_1D <= nyq - 1)
    if (bispec_shell_row(bounds, ki, kj, &kk_bgn, &kk_end) && kk >= kk_bgn && kk <= kk_end) {
        double frac;
        if (antialias) {
            // the loop evaluates the overlap at (ki >= 0, kj, kk) and mirrors it to -ki
            frac = bispec_overlap_cellshell(ki < 0 ? -ki : ki, kj, kk, k_inner, k_outer);
        } else {
            const double k2 = (double)((kj * kj + ki * ki) + (i64)kk * kk);
            frac = (bounds.k2_min < k2 && k2 <= bounds.k2_max) ? 1.0 : 0.0;
        }
        if (src) {
            const double2 z = src[(i64)a * src_si + (i64)bl * cp + kk];
            out = make_double2(frac * z.x, frac * z.y);
        } else {
            out = make_double2(frac, 0.0);
        }
    }
    dst[(i64)a * dst_si + (i64)bl * cp + kk] = out;
}

// kUnique grids: 3 sums g0 g1 g2, 2 sums g0 g1^2, 1 sums g0^3; bit q of power_mask adds the
// sum of gq^2.  partial: double[gridDim.x][4] = (value, power 0, power 1, power 2).
template <int kUnique>
__global__ __launch_bounds__(kThreads) void k_bispec_sums(
    const double *__restrict__ g0, const double *__restrict__ g1, const double *__restrict__ g2,
    int N, int nrows, i64 ny, i64 pad, int power_mask, double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double red[kWaves][4];
    const int half = N / 2;  // pairs of cells per row (N is even)
    double v = 0, p0 = 0, p1 = 0, p2 = 0;
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int layer = row / N, j = row - layer * N;
        const i64 off = ((i64)layer * ny + j) * pad;
        for (int p = threadIdx.x; p < half; p += kThreads) {
            const double2 x0 = *(const double2 *)(g0 + off + 2 * p);
            double2 x1 = x0, x2 = x0;
            if (kUnique >= 2) x1 = *(const double2 *)(g1 + off + 2 * p);
            if (kUnique >= 3) x2 = *(const double2 *)(g2 + off + 2 * p);
            if (kUnique == 3) {
                v += x0.x * x1.x * x2.x;
                v += x0.y * x1.y * x2.y;
            } else if (kUnique == 2) {
                v += x0.x * (x1.x * x1.x);
                v += x0.y * (x1.y * x1.y);
            } else {
                v += x0.x * x0.x * x0.x;
                v += x0.y * x0.y * x0.y;
            }
            if (power_mask & 1) {
                p0 += x0.x * x0.x;
                p0 += x0.y * x0.y;
            }
            if (kUnique >= 2 && (power_mask & 2)) {
                p1 += x1.x * x1.x;
                p1 += x1.y * x1.y;
            }
            if (kUnique >= 3 && (power_mask & 4)) {
                p2 += x2.x * x2.x;
                p2 += x2.y * x2.y;
            }
        }
    }
    v = wave_sum_xor(v);
    p0 = wave_sum_xor(p0);
    p1 = wave_sum_xor(p1);
    p2 = wave_sum_xor(p2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = v;
        red[wave][1] = p0;
        red[wave][2] = p1;
        red[wave][3] = p2;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < kWaves; w++) s = s + red[w][threadIdx.x];
        partial[(i64)blockIdx.x * 4 + threadIdx.x] = s;
    }
}

bool same_geometry(const cg_ctx *a, const cg_ctx *b) {
    return a->N == b->N && a->pad == b->pad && a->ny == b->ny && a->xmap.nxl == b->xmap.nxl &&
           a->xmap.x0 == b->xmap.x0 && a->f_si == b->f_si && a->f_j0 == b->f_j0 &&
           a->f_nj == b->f_nj;
}

}  // namespace

extern "C" int cg_bispec_shell(cg_ctx *dst, cg_ctx *src, double k_inner, double k_outer,
                               int antialias) {
    CG_CHECK(dst, "cg_bispec_shell: null destination context");
    CG_CHECK(dst->four != nullptr,
             "cg_bispec_shell: no Fourier buffer bound to the destination (cg_dist_bind_fourier)");
    CG_CHECK(dst->N >= 2 && dst->N % 2 == 0, "cg_bispec_shell: grid size %lld is not even",
             (long long)dst->N);
    CG_CHECK(0 <= k_inner && k_inner <= k_outer,
             "cg_bispec_shell: shell (%g, %g) is not 0 <= k_inner <= k_outer", k_inner, k_outer);
    if (src) {
        CG_CHECK(src != dst, "cg_bispec_shell: source and destination are one context");
        CG_CHECK(src->four != nullptr,
                 "cg_bispec_shell: no Fourier buffer bound to the source (cg_dist_bind_fourier)");
        CG_CHECK(same_geometry(dst, src),
                 "cg_bispec_shell: source and destination differ in grid size or domain");
    }
    const i64 cp = dst->pad / 2;
    const i64 n = dst->N * (i64)dst->f_nj * cp;
    const BispecShellBounds bounds = bispec_shell_bounds(dst->N, k_inner, k_outer);
    hipLaunchKernelGGL(k_bispec_shell, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, dst->stream, dst->four,
                       src ? (const double2 *)src->four : (const double2 *)nullptr, (int)dst->N,
                       dst->f_si, src ? src->f_si : (i64)0, cp, dst->f_j0, dst->f_nj, k_inner,
                       k_outer, antialias, bounds);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_bispec_sums(cg_ctx *c0, cg_ctx *c1, cg_ctx *c2, int n_unique,
                              int want_power_mask, double *out) {
    CG_CHECK(c0 && out, "cg_bispec_sums: null argument");
    CG_CHECK(n_unique >= 1 && n_unique <= 3, "cg_bispec_sums: n_unique = %d outside 1..3",
             n_unique);
    CG_CHECK(want_power_mask >= 0 && want_power_mask < (1 << n_unique),
             "cg_bispec_sums: power mask %d names a grid beyond the %d unique ones",
             want_power_mask, n_unique);
    cg_ctx *cs[3] = {c0, c1, c2};
    for (int q = 1; q < n_unique; q++) {
        CG_CHECK(cs[q], "cg_bispec_sums: context %d is null with %d unique grids", q, n_unique);
        CG_CHECK(same_geometry(c0, cs[q]),
                 "cg_bispec_sums: context %d differs from context 0 in grid size or domain", q);
        for (int r = 0; r < q; r++)
            CG_CHECK(cs[q] != cs[r], "cg_bispec_sums: contexts %d and %d are one", r, q);
    }
    CG_CHECK(c0->N % 2 == 0, "cg_bispec_sums: grid size %lld is not even", (long long)c0->N);
    const i64 rows = c0->xmap.nxl * c0->N;
    CG_CHECK(rows >= 1 && rows < ((i64)1 << 31), "cg_bispec_sums: %lld rows", (long long)rows);
    const int blocks = (int)(rows < kMaxBlocks ? rows : kMaxBlocks);
    if (c0->bispec_partial.reserve(c0, sizeof(double) * 4 * kMaxBlocks)) return 1;
    double *partial = c0->bispec_partial;
    const double *g0 = c0->mesh0, *g1 = n_unique >= 2 ? c1->mesh0 : nullptr,
                 *g2 = n_unique >= 3 ? c2->mesh0 : nullptr;
#define CG_BISPEC_SUMS(U)                                                                     \
    hipLaunchKernelGGL(k_bispec_sums<U>, dim3((unsigned)blocks), dim3(kThreads), 0, c0->stream, \
                       g0, g1, g2, (int)c0->N, (int)rows, c0->ny, c0->pad, want_power_mask,   \
                       partial)
    if (n_unique == 3) CG_BISPEC_SUMS(3);
    else if (n_unique == 2) CG_BISPEC_SUMS(2);
    else CG_BISPEC_SUMS(1);
#undef CG_BISPEC_SUMS
    CG_LAUNCH_CHECK();
    // out[q] = the sum of the workgroups' partial q
    hipLaunchKernelGGL(k_reduce_columns<OpPlus>, dim3(4), dim3(256), 0, c0->stream,
                       (const double *)partial, (i64)blocks, (i64)4, out);
    CG_LAUNCH_CHECK();
    return 0;
}
