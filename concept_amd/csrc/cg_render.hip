// cg_render.hip — the real-space reductions of the 2D render (graphics).
//   k_project_along_z    project_render2D, axis 'z'              graphics.py:1374-1532
//   k_project_across     project_render2D, axes 'x' and 'y'      graphics.py:1374-1532
//   k_image_minmax       np.min / np.max of enhance_render2D and rescale_render2D
//                                                                 graphics.py:1619-1620, 1745-1746
//   k_image_histogram    np.histogram(projection**exponent, n_bins) of the exponent search and
//                        of the colour truncation                 graphics.py:1634, 1686
//   k_image_apply        projection **= exponent, the colour limits and the rescaling to [0, 1]
//                                                                 graphics.py:1683-1685, 1713-1717,
//                                                                 1747-1755
// The projection reads the context's real-space mesh (cell (x, j, k) of the owned layers at
// mesh0[((x - x0)*ny + j)*pad + k]) and only the planes of the extent.  The image leaves the
// kernels in its final orientation: the transpose and the vertical flip of graphics.py:1524-1531
// take pixel (d0, d1) of the projection to image[(N - 1 - d1)*N + d0], with (d0, d1) = (y, z),
// (x, z), (x, y) for the axes x, y, z.
//
// Deterministic: no floating-point atomics.  A pixel is summed by one wave (axis z: the lanes
// walk the contiguous row, then a fixed butterfly: wave_sum_xor) or by one thread (axes x and y: the lanes run
// along z, every thread adds its planes in ascending order).  The histogram counts are integers
// (LDS and global integer atomics).  Compiled with -ffp-contract=off; FP64 throughout.
#include "cg_internal.h"
#include "cg_wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMinmaxBlocks = 256;          // partial (min, max) pairs of k_image_minmax
constexpr int kLdsMaxBins = 12288;          // 48 KB of 32-bit counts per workgroup
constexpr int kTileD = 16;                  // pixels along d0 per workgroup of k_project_across

// the planes [s0, s1) of the summed axis with the weight of the first and of the last one
// (frac_bgn, frac_end of graphics.py:1399-1400, 1482-1490); every plane between counts once
struct Planes {
    int s0, s1;
    double w_first, w_last;
};

__device__ inline double plane_weight(const Planes &pl, int s) {
    return s == pl.s0 ? pl.w_first : (s == pl.s1 - 1 ? pl.w_last : 1.0);
}

// Axis z: the row (layer, j) is contiguous.  A wave takes 64 consecutive rows j of one layer in
// turn; its lanes walk the planes of a row 64 at a time, a butterfly sums them, and lane t keeps
// the sum of row jb + t.  The wave's 64 pixels lie in one image column, N doubles apart, so its
// store is not coalesced (8 N^2 bytes in all, against 8 N^2 per plane read).  Every row costs
// one six-step butterfly; reducing the partial sums of several rows together is left undone.
__global__ __launch_bounds__(kThreads) void k_project_along_z(
    const double *__restrict__ mesh0, int N, i64 ny, i64 pad, int nxl, int x0, Planes pl,
    double factor, double *__restrict__ image) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const i64 wave = (i64)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int jblocks = (N + 63) / 64;
    if (wave >= (i64)nxl * jblocks) return;
    const int l = (int)(wave / jblocks), jb = (int)(wave - (i64)l * jblocks) * 64;
    double mine = 0;
    for (int t = 0; t < 64 && jb + t < N; t++) {
        const double *row = mesh0 + ((i64)l * ny + (jb + t)) * pad;
        double acc = 0;
        for (int k = pl.s0 + lane; k < pl.s1; k += 64) acc = acc + plane_weight(pl, k) * row[k];
        const double s = wave_sum_xor(acc);
        if (lane == t) mine = s;
    }
    const int j = jb + lane;
    if (j < N) image[(i64)(N - 1 - j) * N + (x0 + l)] = mine * factor;
}

// Axes x and y: the lanes run along z (k), so every load is a coalesced row segment, and a
// thread adds the planes s of its pixels in ascending order.  Cell (d0, s, k) is at
// mesh0[d0*stride_d + s*stride_s + k]: d0 the layer and s the row for axis y, d0 the row and s
// the layer for axis x.  A workgroup owns a tile of 64 k by kTileD d0 (four pixels per thread)
// and turns it in LDS, so that the image rows (fixed k) are stored in segments of kTileD
// pixels.
__global__ __launch_bounds__(kThreads) void k_project_across(
    const double *__restrict__ mesh0, int N, i64 stride_d, i64 stride_s, int nd, int col0,
    Planes pl, double factor, double *__restrict__ image) {
#pragma clang fp contract(off)
    __shared__ double tile[kTileD][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane, d_base = blockIdx.y * kTileD;
    constexpr int kPer = kTileD / 4;
    double acc[kPer];
    const double *src[kPer];
    bool on[kPer];
#pragma unroll
    for (int i = 0; i < kPer; i++) {
        const int d = d_base + wave + 4 * i;
        on[i] = k < N && d < nd;
        src[i] = mesh0 + (i64)(on[i] ? d : 0) * stride_d + (on[i] ? k : 0);
        acc[i] = 0;
    }
    for (int s = pl.s0; s < pl.s1; s++) {
        const double w = plane_weight(pl, s);
#pragma unroll
        for (int i = 0; i < kPer; i++)
            if (on[i]) acc[i] = acc[i] + w * src[i][(i64)s * stride_s];
    }
#pragma unroll
    for (int i = 0; i < kPer; i++) tile[wave + 4 * i][lane] = acc[i] * factor;
    __syncthreads();
    for (int t = threadIdx.x; t < 64 * kTileD; t += kThreads) {
        const int kk = t / kTileD, dd = t - kk * kTileD;
        const int ko = blockIdx.x * 64 + kk, d = d_base + dd;
        if (ko < N && d < nd) image[(i64)(N - 1 - ko) * N + (col0 + d)] = tile[dd][kk];
    }
}

// projection**exponent; an exponent of 1 leaves the value as it is
__device__ inline double powered(double v, double exponent) {
    return exponent == 1.0 ? v : pow(v, exponent);
}

// (min, max) of image**exponent: a pair per workgroup, then one workgroup over the pairs
__global__ __launch_bounds__(kThreads) void k_image_minmax(const double *__restrict__ image, i64 n,
                                                          double exponent, i64 npairs,
                                                          double *__restrict__ pairs) {
    __shared__ double lo_s[kThreads], hi_s[kThreads];
    double lo = INFINITY, hi = -INFINITY;
    if (npairs == 0) {  // the values themselves, one per thread and grid step
        for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads) {
            const double v = powered(image[i], exponent);
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
    } else {            // the pairs of the first pass
        for (i64 i = threadIdx.x; i < npairs; i += kThreads) {
            lo = fmin(lo, image[2 * i]);
            hi = fmax(hi, image[2 * i + 1]);
        }
    }
    lo = block_tree<OpFmin>(lo_s, lo);
    hi = block_tree<OpFmax>(hi_s, hi);
    if (threadIdx.x == 0) {
        pairs[2 * blockIdx.x] = lo;
        pairs[2 * blockIdx.x + 1] = hi;
    }
}

// numpy's bin of x among n_bins uniform bins (numpy/lib/_histograms_impl.py, the equal-width
// path): the index from (x - first)/(last - first)*n_bins, moved down or up by one against the
// edges linspace(first, last, n_bins + 1) gave; the last bin is closed on the right
__device__ inline int uniform_bin(double x, const double *__restrict__ edges, int n_bins) {
#pragma clang fp contract(off)
    const double first = edges[0], last = edges[n_bins];
    if (!(x >= first && x <= last)) return -1;
    const double f = (x - first) / (last - first) * (double)n_bins;
    int idx = (int)f;
    if (idx >= n_bins) idx = n_bins - 1;
    if (idx < 0) idx = 0;
    if (x < edges[idx] && idx > 0) idx--;
    if (x >= edges[idx + 1] && idx != n_bins - 1) idx++;
    return idx;
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void k_image_histogram(
    const double *__restrict__ image, i64 n, double exponent, const double *__restrict__ edges,
    int n_bins, unsigned long long *__restrict__ counts) {
    extern __shared__ unsigned lds_counts[];
    if (kLds) {
        for (int b = threadIdx.x; b < n_bins; b += kThreads) lds_counts[b] = 0;
        __syncthreads();
    }
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads) {
        const int bin = uniform_bin(powered(image[i], exponent), edges, n_bins);
        if (bin < 0) continue;
        if (kLds) atomicAdd(&lds_counts[bin], 1u);
        else atomicAdd(&counts[bin], 1ull);
    }
    if (kLds) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += kThreads) {
            const unsigned cnt = lds_counts[b];
            if (cnt) atomicAdd(&counts[b], (unsigned long long)cnt);
        }
    }
}

// v -> (min(max(v**exponent, lo), hi) - shift)*scale, or `fill` for every pixel (fill >= 0)
__global__ __launch_bounds__(kThreads) void k_image_apply(double *__restrict__ image, i64 n,
                                                         double exponent, double lo, double hi,
                                                         double shift, double scale, double fill) {
#pragma clang fp contract(off)
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads) {
        if (fill >= 0) {
            image[i] = fill;
            continue;
        }
        double v = powered(image[i], exponent);
        v = v > lo ? v : lo;   // pairmax(value, vmin)
        v = v < hi ? v : hi;   // pairmin(value, vmax)
        image[i] = (v - shift) * scale;
    }
}

unsigned grid_for(i64 n, i64 cap) {
    i64 blocks = (n + kThreads - 1) / kThreads;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

extern "C" int cg_render2d_project(cg_ctx *c, int axis, int64_t plane_bgn, int64_t plane_end,
                                   double frac_bgn, double frac_end, double factor,
                                   double *image) {
    CG_CHECK(c && image, "cg_render2d_project: null argument");
    CG_CHECK(axis >= 0 && axis < 3, "cg_render2d_project: axis %d not in {0, 1, 2}", axis);
    const i64 N = c->N;
    CG_CHECK(plane_bgn >= 0 && plane_bgn < plane_end && plane_end <= N,
             "cg_render2d_project: planes [%lld, %lld) outside the grid of size %lld",
             (long long)plane_bgn, (long long)plane_end, (long long)N);
    const i64 x0 = c->xmap.x0, nxl = c->xmap.nxl;
    if (c->p.nprocs > 1)  // the other domains' pixels: zero here, summed over the ranks later
        CG_HIP(hipMemsetAsync(image, 0, sizeof(double) * N * N, c->stream));
    // this domain's planes of the range, with the fractions on the planes that end the range
    i64 s0 = plane_bgn, s1 = plane_end;
    if (axis == 0) {
        s0 = (plane_bgn > x0 ? plane_bgn : x0) - x0;
        s1 = (plane_end < x0 + nxl ? plane_end : x0 + nxl) - x0;
        if (s0 >= s1) {  // none of the planes are here (graphics.py:1415-1440)
            if (c->p.nprocs == 1) CG_HIP(hipMemsetAsync(image, 0, sizeof(double) * N * N, c->stream));
            return 0;
        }
    }
    const i64 g0 = axis == 0 ? s0 + x0 : s0, g1 = axis == 0 ? s1 + x0 : s1;
    Planes pl{(int)s0, (int)s1, g0 == plane_bgn ? frac_bgn : 1.0,
              g1 == plane_end ? frac_end : 1.0};
    // one plane here is counted once: as the first of the range if it is that, else as the last
    if (s1 - s0 == 1 && g0 != plane_bgn) pl.w_first = pl.w_last;
    const i64 layer = c->ny * c->pad;
    if (axis == 2) {
        const i64 waves = nxl * ((N + 63) / 64);
        hipLaunchKernelGGL(k_project_along_z, dim3((unsigned)((waves + 3) / 4)), dim3(kThreads), 0,
                           c->stream, (const double *)c->mesh0, (int)N, c->ny, c->pad, (int)nxl,
                           (int)x0, pl, factor, image);
    } else {
        // axis y: pixels (x, z) of the own layers, summed over the rows; axis x: pixels (y, z),
        // summed over the own layers
        const i64 nd = axis == 1 ? nxl : N;
        const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((nd + kTileD - 1) / kTileD));
        hipLaunchKernelGGL(k_project_across, grid, dim3(kThreads), 0, c->stream,
                           (const double *)c->mesh0, (int)N, axis == 1 ? layer : c->pad,
                           axis == 1 ? c->pad : layer, (int)nd, axis == 1 ? (int)x0 : 0, pl,
                           factor, image);
    }
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t cg_render2d_workspace(void) { return 2 * kMinmaxBlocks; }

extern "C" int cg_render2d_minmax(cg_ctx *c, const double *image, int64_t n, double exponent,
                                  double *minmax_out, double *workspace) {
    CG_CHECK(c && image && minmax_out && workspace, "cg_render2d_minmax: null argument");
    CG_CHECK(n >= 1, "cg_render2d_minmax: an image of %lld pixels", (long long)n);
    const unsigned blocks = grid_for(n, kMinmaxBlocks);
    hipLaunchKernelGGL(k_image_minmax, dim3(blocks), dim3(kThreads), 0, c->stream, image, (i64)n,
                       exponent, (i64)0, workspace);
    CG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_image_minmax, dim3(1), dim3(kThreads), 0, c->stream,
                       (const double *)workspace, (i64)0, 1.0, (i64)blocks, minmax_out);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_render2d_histogram(cg_ctx *c, const double *image, int64_t n, double exponent,
                                     const double *bin_edges, int32_t n_bins,
                                     int64_t *counts_out) {
    CG_CHECK(c && image && bin_edges && counts_out, "cg_render2d_histogram: null argument");
    CG_CHECK(n >= 1 && n_bins >= 1, "cg_render2d_histogram: %lld pixels, %d bins", (long long)n,
             (int)n_bins);
    CG_HIP(hipMemsetAsync(counts_out, 0, sizeof(int64_t) * n_bins, c->stream));
    if (n_bins <= kLdsMaxBins) {
        // a workgroup adds its n_bins counts to the global ones at the end: give it at least
        // eight pixels per bin, so that this costs less than counting in global memory
        i64 blocks = n / (8 * (i64)n_bins);
        blocks = blocks > 1024 ? 1024 : (blocks < 1 ? 1 : blocks);
        hipLaunchKernelGGL(k_image_histogram<true>, dim3((unsigned)blocks), dim3(kThreads),
                           sizeof(unsigned) * n_bins, c->stream, image, (i64)n, exponent,
                           bin_edges, (int)n_bins, (unsigned long long *)counts_out);
    } else {
        hipLaunchKernelGGL(k_image_histogram<false>, dim3(grid_for(n, 2048)), dim3(kThreads), 0,
                           c->stream, image, (i64)n, exponent, bin_edges, (int)n_bins,
                           (unsigned long long *)counts_out);
    }
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_render2d_apply(cg_ctx *c, double *image, int64_t n, double exponent, double vmin,
                                 double vmax, double shift, double scale, double fill) {
    CG_CHECK(c && image, "cg_render2d_apply: null argument");
    CG_CHECK(n >= 1, "cg_render2d_apply: an image of %lld pixels", (long long)n);
    hipLaunchKernelGGL(k_image_apply, dim3(grid_for(n, 2048)), dim3(kThreads), 0, c->stream, image,
                       (i64)n, exponent, vmin, vmax, shift, scale, fill);
    CG_LAUNCH_CHECK();
    return 0;
}
