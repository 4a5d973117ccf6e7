// cg_measure.hip — the reductions of analysis.measure() (analysis.py:3860-4230):
//   k_measure_sums     Σx and Σx² in double-double, min x and max |x| of up to three columns of a
//                      strided array ('momentum', 'ϱ', 'mass': analysis.py:4032-4143), and with
//                      another loader of the fluid's squared velocity        analysis.py:4005-4012
//   k_discontinuity    max |fwd − bwd| and max(|fwd|, |bwd|) of the order-1 differences of a
//                      fluid grid along the three dimensions  analysis.py:4171-4213, mesh.py:4961-4965
// Every reduction has a fixed shape: a thread folds its elements in index order, the 64 lanes of a
// wave by xor butterfly, the four waves of a workgroup as (w0 + w1) + (w2 + w3), one partial per
// workgroup, and one last workgroup folds the partials the same way.  No atomics: the same input
// gives the same bits.
//
// The sums (cg_wave.h, dd): a thread adds x to Σx with DWPlusFP (error <= 2u² of the partial sum,
// u = 2^-53) and the exact square fma(x, x, -x*x) + x*x to Σx² with AccurateDWPlusDW (<= 3u² +
// 13u³); every later step is an AccurateDWPlusDW.  A sum of n values passes through n additions in
// the threads and fewer than n in the trees, each with an error of at most 3.001u² Σ|x|: the result
// is within 2n·3.001u² Σ|x| < n 2^-100 Σ|x| of the exact sum (2^-100 = 64u²).
#include "cg_wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSumBlocks = 1024;   // at most this many partials per launch
constexpr int kMaxCols = 3;
constexpr int kBatch = 4;          // rows a thread has in flight
constexpr int kPerCol = 6;         // Σx hi, lo, Σx² hi, lo, min x, max |x|

template <int kCols>
struct Acc {
    dd s[kCols], s2[kCols];
    double mn[kCols], mx[kCols];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < kCols; q++) {
            s[q] = s2[q] = dd{0.0, 0.0};
            mn[q] = OpMinNan::identity();
            mx[q] = OpMaxNan::identity();
        }
    }
    __device__ __forceinline__ void take(const double (&x)[kCols]) {
#pragma unroll
        for (int q = 0; q < kCols; q++) {
            s[q] = dd_add_double(s[q], x[q]);
            s2[q] = dd_add(s2[q], dd_square(x[q]));
            mn[q] = OpMinNan()(mn[q], x[q]);
            mx[q] = OpMaxNan()(mx[q], fabs(x[q]));
        }
    }
    // the kPerCol numbers of every column as a workgroup wrote them
    __device__ __forceinline__ void merge(const double *p) {
#pragma unroll
        for (int q = 0; q < kCols; q++, p += kPerCol) {
            s[q] = dd_add(s[q], dd{p[0], p[1]});
            s2[q] = dd_add(s2[q], dd{p[2], p[3]});
            mn[q] = OpMinNan()(mn[q], p[4]);
            mx[q] = OpMaxNan()(mx[q], p[5]);
        }
    }
};

// The workgroup's 256 accumulators as one, stored by thread 0 as kPerCol numbers per column:
// lanes by xor butterfly, then the four wave leaders' values through LDS as (w0 + w1) + (w2 + w3).
template <int kCols>
__device__ __forceinline__ void block_acc_store(Acc<kCols> a, double *out) {
    __shared__ double lds[4][kCols * kPerCol];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kCols; q++) {
        const dd s = wave_sum_xor_dd(a.s[q]), s2 = wave_sum_xor_dd(a.s2[q]);
        const double mn = wave_fold_xor<OpMinNan>(a.mn[q]), mx = wave_fold_xor<OpMaxNan>(a.mx[q]);
        if ((threadIdx.x & 63) == 0) {
            double *l = lds[w] + q * kPerCol;
            l[0] = s.hi, l[1] = s.lo, l[2] = s2.hi, l[3] = s2.lo, l[4] = mn, l[5] = mx;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kCols; q++) {
            const double *l0 = lds[0] + q * kPerCol, *l1 = lds[1] + q * kPerCol,
                         *l2 = lds[2] + q * kPerCol, *l3 = lds[3] + q * kPerCol;
            const dd s = dd_add(dd_add(dd{l0[0], l0[1]}, dd{l1[0], l1[1]}),
                                dd_add(dd{l2[0], l2[1]}, dd{l3[0], l3[1]}));
            const dd s2 = dd_add(dd_add(dd{l0[2], l0[3]}, dd{l1[2], l1[3]}),
                                 dd_add(dd{l2[2], l2[3]}, dd{l3[2], l3[3]}));
            double *o = out + q * kPerCol;
            o[0] = s.hi, o[1] = s.lo, o[2] = s2.hi, o[3] = s2.lo;
            o[4] = OpMinNan()(OpMinNan()(l0[4], l1[4]), OpMinNan()(l2[4], l3[4]));
            o[5] = OpMaxNan()(OpMaxNan()(l0[5], l1[5]), OpMaxNan()(l2[5], l3[5]));
        }
    }
}

// what a row holds: kCols neighbouring elements of a strided array ...
struct LoadStrided {
    const double *x;   // the first column of row 0
    i64 stride;
    template <int kCols>
    __device__ __forceinline__ void operator()(i64 row, double (&v)[kCols]) const {
#pragma unroll
        for (int q = 0; q < kCols; q++) v[q] = x[row * stride + q];
    }
};
// ... or the squared velocity of a fluid cell, in the reference's expression order (k_vmax has
// the maximum of the same term)
struct LoadFluidVelocity {
    const double *rho, *P, *Jx, *Jy, *Jz;
    double inv_c2;
    __device__ __forceinline__ void operator()(i64 i, double (&v)[1]) const {
#pragma clang fp contract(off)
        const double jx = Jx[i], jy = Jy[i], jz = Jz[i];
        const double den = rho[i] + inv_c2 * P[i];
        v[0] = (jx * jx + jy * jy + jz * jz) / (den * den);
    }
};

// rows [p0, p1) by the workgroup's threads, thread t taking p0 + t, p0 + t + 256, ... in turn,
// kBatch of them loaded before they are added
template <int kCols, class Load>
__device__ __forceinline__ void take_rows(Acc<kCols> &a, const Load &load, i64 p0, i64 p1) {
    for (i64 p = p0 + threadIdx.x; p < p1; p += (i64)kBatch * kThreads) {
        double v[kBatch][kCols];
#pragma unroll
        for (int u = 0; u < kBatch; u++)
            if (p + (i64)u * kThreads < p1) load(p + (i64)u * kThreads, v[u]);
#pragma unroll
        for (int u = 0; u < kBatch; u++)
            if (p + (i64)u * kThreads < p1) a.take(v[u]);
    }
}

// start == nullptr: workgroup b takes the rows [b per, (b + 1) per) of n, per = ceil(n / workgroups).
// Else the regions [b per, (b + 1) per) of nregions, region r holding the rows
// [start[r], start[r] + count[r]) (count == nullptr: up to start[r + 1]); rows between the regions
// are not read.
template <int kCols, class Load>
__global__ __launch_bounds__(kThreads) void k_measure_sums(Load load, i64 n,
                                                          const unsigned *__restrict__ start,
                                                          const unsigned *__restrict__ count,
                                                          i64 nregions,
                                                          double *__restrict__ partial) {
    Acc<kCols> a;
    a.clear();
    const i64 total = start ? nregions : n;
    const i64 per = (total + gridDim.x - 1) / gridDim.x;
    const i64 b0 = (i64)blockIdx.x * per, b1 = b0 + per < total ? b0 + per : total;
    if (!start) {
        take_rows(a, load, b0, b1);
    } else {
        for (i64 r = b0; r < b1; r++) {
            const i64 p0 = start[r], m = count ? count[r] : start[r + 1] - start[r];
            take_rows(a, load, p0, p0 + m);
        }
    }
    block_acc_store(a, partial + (i64)blockIdx.x * kCols * kPerCol);
}

// the partials of nb workgroups as one result: thread t merges the partials t, t + 256, ... in turn
template <int kCols>
__global__ __launch_bounds__(kThreads) void k_measure_sums_final(const double *__restrict__ partial,
                                                                int nb, double *__restrict__ out) {
    Acc<kCols> a;
    a.clear();
    for (int b = threadIdx.x; b < nb; b += kThreads) a.merge(partial + (i64)b * kCols * kPerCol);
    block_acc_store(a, out);
}

template <int kCols, class Load>
int launch_sums(cg_ctx *c, const Load &load, i64 n, const unsigned *start, const unsigned *count,
                i64 nregions, double *out) {
    if (c->measure_partial.reserve(c, sizeof(double) * kSumBlocks * kMaxCols * kPerCol)) return 1;
    // a workgroup per 256 rows (per region), at most kSumBlocks
    i64 nb = start ? nregions : (n + kThreads - 1) / kThreads;
    nb = nb < 1 ? 1 : (nb > kSumBlocks ? kSumBlocks : nb);
    double *partial = c->measure_partial;
    hipLaunchKernelGGL((k_measure_sums<kCols, Load>), dim3((unsigned)nb), dim3(kThreads), 0,
                       c->stream, load, n, start, count, nregions, partial);
    CG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_measure_sums_final<kCols>, dim3(1), dim3(kThreads), 0, c->stream,
                       (const double *)partial, (int)nb, out);
    CG_LAUNCH_CHECK();
    return 0;
}

__device__ __forceinline__ int wrap(int a, int g) { return a < 0 ? a + g : (a >= g ? a - g : a); }

// A thread per cell, grid stride.  lo / hi: the layer below the first and above the last own one
// (null: the own layers wrap around).  out[b*6 + d] = max |fwd − bwd| along d, out[b*6 + 3 + d] =
// max(|fwd|, |bwd|), under the reference's compare (value > maximum, from 0).
__global__ __launch_bounds__(kThreads) void k_discontinuity(const double *__restrict__ own,
                                                           const double *__restrict__ lo,
                                                           const double *__restrict__ hi, int g,
                                                           int nxl, double inv_h,
                                                           double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double lds[4][6];
    const OpGreaterFrom0 greater;
    const i64 g2 = (i64)g * g, n = (i64)nxl * g2;
    double best[6];
#pragma unroll
    for (int q = 0; q < 6; q++) best[q] = OpGreaterFrom0::identity();
    for (i64 idx = (i64)blockIdx.x * kThreads + threadIdx.x; idx < n;
         idx += (i64)gridDim.x * kThreads) {
        const int i = (int)(idx / g2);
        const i64 r = idx - (i64)i * g2;
        const int j = (int)(r / g), k = (int)(r - (i64)j * g);
        const double *layer = own + (i64)i * g2;
        const double *below = i > 0 ? layer - g2 : (lo ? lo : own + (i64)(nxl - 1) * g2);
        const double *above = i + 1 < nxl ? layer + g2 : (hi ? hi : own);
        const double f0 = layer[r];
        const double up[3] = {above[r], layer[(i64)wrap(j + 1, g) * g + k],
                              layer[(i64)j * g + wrap(k + 1, g)]};
        const double dn[3] = {below[r], layer[(i64)wrap(j - 1, g) * g + k],
                              layer[(i64)j * g + wrap(k - 1, g)]};
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double fwd = inv_h * (up[d] - f0), bwd = inv_h * (f0 - dn[d]);
            best[d] = greater(best[d], fabs(fwd - bwd));
            best[3 + d] = greater(greater(best[3 + d], fabs(fwd)), fabs(bwd));
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const double v = wave_fold_xor<OpGreaterFrom0>(best[q]);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int q = threadIdx.x;
        partial[(i64)blockIdx.x * 6 + q] =
            greater(greater(lds[0][q], lds[1][q]), greater(lds[2][q], lds[3][q]));
    }
}

}  // namespace

extern "C" int cg_measure_sums(cg_ctx *c, const double *x, int64_t n, int64_t stride,
                               int64_t offset, int ncols, const uint32_t *start,
                               const uint32_t *count, int64_t nregions, double *out) {
    CG_READS_PARTICLES(c);
    CG_CHECK(c && out, "cg_measure_sums: null argument");
    CG_CHECK(ncols >= 1 && ncols <= kMaxCols, "cg_measure_sums: %d columns (1 to %d)", ncols,
             kMaxCols);
    CG_CHECK(stride >= 1 && offset >= 0 && offset + ncols <= stride,
             "cg_measure_sums: columns [%lld, %lld) of rows of %lld elements", (long long)offset,
             (long long)(offset + ncols), (long long)stride);
    if (start) {
        CG_CHECK(x && nregions >= 0, "cg_measure_sums: null array or %lld regions",
                 (long long)nregions);
    } else {
        CG_CHECK(n >= 0 && (x || n == 0) && !count, "cg_measure_sums: n out of range, null array "
                 "or populations without regions");
        nregions = 0;
    }
    const LoadStrided load{x ? x + offset : x, stride};
    return with_case<kMaxCols>(ncols - 1, [&](auto k) {
        return launch_sums<decltype(k)::value + 1>(c, load, (i64)n, start, count, (i64)nregions,
                                                   out);
    });
}

extern "C" int cg_measure_fluid_velocity(cg_ctx *c, const double *rho, const double *P,
                                         const void *const *J, int64_t n, double inv_c2,
                                         double *out) {
    CG_CHECK(c && rho && P && J && out && n >= 0, "cg_measure_fluid_velocity: null argument");
    CG_CHECK(J[0] && J[1] && J[2], "cg_measure_fluid_velocity: null grid");
    const LoadFluidVelocity load{rho, P, (const double *)J[0], (const double *)J[1],
                                 (const double *)J[2], inv_c2};
    return launch_sums<1>(c, load, (i64)n, nullptr, nullptr, 0, out);
}

extern "C" int cg_measure_discontinuity(cg_ctx *c, const double *f, const double *f_lo,
                                        const double *f_hi, int64_t gridsize, int64_t nxl,
                                        double inv_h, double *out) {
    CG_CHECK(c && f && out, "cg_measure_discontinuity: null argument");
    CG_CHECK((f_lo == nullptr) == (f_hi == nullptr),
             "cg_measure_discontinuity: give both neighbouring layers or neither");
    CG_CHECK(gridsize >= 1 && gridsize <= 32768, "cg_measure_discontinuity: grid size %lld",
             (long long)gridsize);
    CG_CHECK(nxl >= 1 && nxl <= gridsize && (f_lo || nxl == gridsize),
             "cg_measure_discontinuity: %lld of %lld layers%s", (long long)nxl,
             (long long)gridsize, f_lo ? "" : " and no layers of the neighbouring domains");
    if (c->measure_partial.reserve(c, sizeof(double) * kSumBlocks * kMaxCols * kPerCol)) return 1;
    const i64 n = nxl * gridsize * gridsize;
    i64 nb = (n + kThreads - 1) / kThreads;
    nb = nb > kSumBlocks ? kSumBlocks : nb;
    double *partial = c->measure_partial;
    hipLaunchKernelGGL(k_discontinuity, dim3((unsigned)nb), dim3(kThreads), 0, c->stream, f, f_lo,
                       f_hi, (int)gridsize, (int)nxl, inv_h, partial);
    CG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_reduce_columns<OpGreaterFrom0>, dim3(6), dim3(kThreads), 0, c->stream,
                       (const double *)partial, nb, (i64)6, out);
    CG_LAUNCH_CHECK();
    return 0;
}
