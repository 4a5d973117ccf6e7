// cg_analysis.hip — the k-space reduction of the power spectrum (analysis).
//   k_powerspec_bin      the binning loop of compute_powerspec   analysis.py:544-560
//                        over fourier_loop(sparse=True, skip_origin=True, k2_max)
//                                                                 mesh.py:2748-2838
//   k_reduce_columns     the Reduce(op=MPI.SUM) of the partial bins, in a fixed order
//   (cg_wave.h)                                                   analysis.py:562-566
// The walk is over the context's current Fourier view (cg_ctx::four, the view
// k_fourier_operate walks): mode (ki, kj, kk) with array indices (a, b, kk) at
// four[a*f_si + (b - f_j0)*cp + kk].  Visited are the modes of the reference's sparse loop:
// no Nyquist planes, no origin, ki² + kj² + kk² <= k2_max, and in the kk = 0 plane one of each
// conjugate pair (ki > 0 and ki == 0 && kj > 0 are skipped, mesh.py:2815-2827).
//
// Deterministic: no floating-point atomics.  A wave owns a row (a, b) at a time and walks it in
// chunks of 64 modes, one per lane.  Along kk the bin index never decreases, so a chunk whose
// modes all fall into the bin of the wave's pending run is added lane-wise into per-lane
// accumulators; a change of bin closes the run: wave_sum_xor sums it over the lanes, and
// lane 0 adds the sum into the wave's private histogram.  The waves of a workgroup are
// combined in wave order into one partial histogram per workgroup (LDS histograms), or every
// wave keeps its partial histogram in global memory (bins beyond the LDS budget);
// k_reduce_columns then sums the partials of every bin in a fixed tree order (cg_wave.h).
// Compiled with -ffp-contract=off; FP64 throughout, k² as an integer.
#include "cg_internal.h"
#include "cg_wave.h"

namespace {

constexpr int kWaves = 4;                 // waves per workgroup of k_powerspec_bin
constexpr int kThreads = 64 * kWaves;
constexpr int kLdsMaxBins = 1024;         // 4 waves x 1024 bins x 8 B = 32 KB of LDS
constexpr i64 kGlobalPartialDoubles = (i64)32 << 20;  // 256 MB for the global-memory path

// floor(sqrt(n)) for 0 <= n < 2^52, exact
__device__ __host__ inline i64 isqrt64(i64 n) {
    i64 r = (i64)sqrt((double)n);
    while (r * r > n) r--;
    while ((r + 1) * (r + 1) <= n) r++;
    return r;
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void k_powerspec_bin(
    const double2 *__restrict__ four, int N, i64 si, i64 cp, int j0, int nj,
    const int32_t *__restrict__ k_bin_indices, i64 k2_max, int nbins,
    double *__restrict__ partial) {
#pragma clang fp contract(off)
    extern __shared__ double lds_hist[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nyq = N / 2;
    double *hist = kLds ? lds_hist + (i64)wave * nbins
                        : partial + ((i64)blockIdx.x * kWaves + wave) * nbins;
    if (kLds) {
        for (int b = threadIdx.x; b < kWaves * nbins; b += kThreads) lds_hist[b] = 0;
        __syncthreads();
    }
    const i64 rows = (i64)N * nj;
    const i64 wave_id = (i64)blockIdx.x * kWaves + wave, nwaves = (i64)gridDim.x * kWaves;
    for (i64 row = wave_id; row < rows; row += nwaves) {
        const int a = (int)(row / nj), bl = (int)(row - (i64)a * nj), b = j0 + bl;
        if (a == nyq || b == nyq) continue;  // Nyquist planes
        const i64 ki = a - (a >= nyq ? N : 0), kj = b - (b >= nyq ? N : 0);
        const i64 r2 = ki * ki + kj * kj;
        if (r2 > k2_max) continue;  // the row lies outside the sphere: nothing is read
        i64 kk_end = isqrt64(k2_max - r2) + 1;
        if (kk_end > nyq) kk_end = nyq;  // kk = nyq is the Nyquist plane
        // origin and the conjugate half of the kk = 0 plane (mesh.py:2800-2827)
        const int kk_bgn = (ki > 0 || (ki == 0 && kj >= 0)) ? 1 : 0;
        const double2 *src = four + (i64)a * si + (i64)bl * cp;
        double acc = 0;  // the pending run: lane-wise partial sums of bin `pending`
        int pending = -1;
        for (int c0 = 0; c0 < kk_end; c0 += 64) {
            const int kk = c0 + lane;
            const bool in = kk >= kk_bgn && kk < kk_end;
            int bin = -1;
            double pw = 0;
            if (in) {
                const i64 k2 = r2 + (i64)kk * kk;
                bin = k_bin_indices[k2];
                const double2 z = src[kk];
                pw = z.x * z.x + z.y * z.y;
            }
            const bool valid = in && bin >= 0 && bin < nbins;
            unsigned long long vmask = __ballot(valid);
            if (!vmask) continue;
            const int first = __ffsll((long long)vmask) - 1;
            const int b0 = __shfl(bin, first);
            if (__ballot(valid && bin != b0) == 0) {
                // the whole chunk falls into one bin
                if (b0 != pending) {
                    if (pending >= 0) {
                        const double s = wave_sum_xor(acc);
                        if (lane == 0) hist[pending] += s;
                    }
                    pending = b0;
                    acc = 0;
                }
                if (valid) acc += pw;
                continue;
            }
            // the chunk spans several bins: close the run, then one butterfly per bin
            if (pending >= 0) {
                const double s = wave_sum_xor(acc);
                if (lane == 0) hist[pending] += s;
            }
            pending = -1;
            acc = 0;
            while (vmask) {
                const int l = __ffsll((long long)vmask) - 1;
                const int bsel = __shfl(bin, l);
                const bool sel = valid && bin == bsel;
                const double s = wave_sum_xor(sel ? pw : 0.0);
                if (lane == 0) hist[bsel] += s;
                vmask &= ~__ballot(sel);
            }
        }
        if (pending >= 0) {
            const double s = wave_sum_xor(acc);
            if (lane == 0) hist[pending] += s;
        }
    }
    if (kLds) {
        __syncthreads();
        double *out = partial + (i64)blockIdx.x * nbins;
        for (int bb = threadIdx.x; bb < nbins; bb += kThreads) {
            double s = lds_hist[bb];
            for (int w = 1; w < kWaves; w++) s = s + lds_hist[(i64)w * nbins + bb];
            out[bb] = s;
        }
    }
}

struct BinLaunch {
    bool lds;
    i64 blocks, npartials, doubles;
};

BinLaunch bin_launch(const cg_ctx *c, int nbins) {
    BinLaunch L{};
    const i64 rows = c->N * (i64)c->f_nj;
    i64 blocks = (rows + kWaves - 1) / kWaves;
    if (blocks > 256 * 8) blocks = 256 * 8;  // 8 workgroups per CU
    if (blocks < 1) blocks = 1;
    L.lds = nbins <= kLdsMaxBins;
    if (!L.lds) {
        const i64 fit = kGlobalPartialDoubles / ((i64)kWaves * nbins);
        if (blocks > fit) blocks = fit < 1 ? 1 : fit;
    }
    L.blocks = blocks;
    L.npartials = L.lds ? blocks : blocks * kWaves;
    L.doubles = L.npartials * nbins;
    return L;
}

}  // namespace

extern "C" int64_t cg_powerspec_workspace(cg_ctx *c, int32_t nbins) {
    if (!c || nbins < 1) {
        cg_set_error("cg_powerspec_workspace: null context or nbins %d < 1", (int)nbins);
        return -1;
    }
    return bin_launch(c, nbins).doubles;
}

extern "C" int cg_powerspec_bin(cg_ctx *c, const int32_t *k_bin_indices, int64_t k2_max,
                                int32_t nbins, double *power_out, double *workspace,
                                int64_t workspace_doubles) {
    CG_CHECK(c && k_bin_indices && power_out && workspace, "cg_powerspec_bin: null argument");
    CG_CHECK(c->four != nullptr,
             "cg_powerspec_bin: no Fourier buffer bound (cg_dist_bind_fourier)");
    CG_CHECK(nbins >= 1, "cg_powerspec_bin: nbins = %d < 1", (int)nbins);
    const i64 nyq = c->N / 2;
    CG_CHECK(k2_max >= 0 && k2_max <= 3 * nyq * nyq,
             "cg_powerspec_bin: k2_max = %lld outside [0, 3*nyquist^2 = %lld]",
             (long long)k2_max, (long long)(3 * nyq * nyq));
    const BinLaunch L = bin_launch(c, nbins);
    CG_CHECK(workspace_doubles >= L.doubles,
             "cg_powerspec_bin: workspace of %lld doubles, %lld needed (cg_powerspec_workspace)",
             (long long)workspace_doubles, (long long)L.doubles);
    if (L.lds) {
        hipLaunchKernelGGL(k_powerspec_bin<true>, dim3((unsigned)L.blocks), dim3(kThreads),
                           (size_t)kWaves * nbins * sizeof(double), c->stream,
                           (const double2 *)c->four, (int)c->N, c->f_si, c->pad / 2, c->f_j0,
                           c->f_nj, k_bin_indices, (i64)k2_max, (int)nbins, workspace);
    } else {
        CG_HIP(hipMemsetAsync(workspace, 0, (size_t)L.doubles * sizeof(double), c->stream));
        hipLaunchKernelGGL(k_powerspec_bin<false>, dim3((unsigned)L.blocks), dim3(kThreads), 0,
                           c->stream, (const double2 *)c->four, (int)c->N, c->f_si, c->pad / 2,
                           c->f_j0, c->f_nj, k_bin_indices, (i64)k2_max, (int)nbins, workspace);
    }
    CG_LAUNCH_CHECK();
    // power[bin] = the sum of the partial histograms' column `bin`
    hipLaunchKernelGGL(k_reduce_columns<OpPlus>, dim3((unsigned)nbins), dim3(256), 0, c->stream,
                       (const double *)workspace, L.npartials, (i64)nbins, power_out);
    CG_LAUNCH_CHECK();
    return 0;
}
