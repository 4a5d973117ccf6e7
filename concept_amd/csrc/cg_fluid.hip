// cg_fluid.hip — the flux terms of the MacCormack scheme for a fluid with non-linear ϱ and J
// (boltzmann_order = 1, closure 'truncate'), its vacuum sweep and its v_max.
//   k_mc_step         maccormack_step, all four variables in one pass     fluid.py:841-946
//   k_mc_halve        scale_nonlinear_fluid_grids(0.5)                    fluid.py:788
//   k_vacuum_detect   the detection compare and fac_time of correct_vacuum, and the compare of
//                     check_vacuum                                        fluid.py:1241-1286, 1094-1097
//   k_vacuum_gather   the pair terms of the 3x3x3 blocks, as a gather     fluid.py:1289-1319
//   k_vacuum_apply    variable += Δ                                       fluid.py:1333-1340
//   k_vmax            max (Jx² + Jy² + Jz²)/(ϱ + c⁻²𝒫)²                   analysis.py:3940-3955
//                     (the workgroups' maxima, then k_reduce_columns of cg_wave.h)
//   k_pressure_sources  𝒫 = ϱ (c²w) and the pressure term of the Euler equation, one pass
//                                                         ic.py:503-508, fluid.py:1044-1057, mesh.py:4966-4970
//   k_realize_P       𝒫 = ϱ (c²w) alone                                   ic.py:503-508
//   k_kt_step         one Runge-Kutta step of kurganov_tadmor, all four variables and the
//                     realisation of 𝒫 in one pass, per flux limiter     fluid.py:103-673
//
// A fluid grid is this domain's layers of the global grid, double[nxl][g][g] without ghosts
// (species.Component).  y and z are periodic by index wrap.  In x a kernel reads up to H layers
// beyond the own ones: with lo = hi = NULL they are the own layers on the other side of the box
// (one domain, nxl = g); else lo holds the H layers below the first own one and hi the H layers
// above the last, each double[H][g][g] in ascending x (the caller exchanged them).
//
// The three stencil kernels (k_mc_step, k_pressure_sources, k_kt_step) share StepTile, a
// workgroup's tile of cells and its walk along x (k_kt_step spells its values out, see there), and
// stage(), the copy of a layer's tile and halo into LDS; they differ in the halo and in what stays
// resident.  On the host: tile_grid and
// launch_stride (the two launch shapes), take4 (a pack of grids from the caller's pointers),
// take_layers, check_shape and check_aliasing (no pass reads what it writes).
//
// FP64, compiled with -ffp-contract=off: every sum, product and quotient is evaluated as the
// reference writes it.  No floating-point atomics: the results do not depend on the launch.
#include "cg_internal.h"
#include "cg_wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTY = 8, kTZ = 32;   // cells of a step tile along y and z (kTY*kTZ = kThreads)
constexpr int kXC = 8;             // layers a workgroup of the step walks along x
constexpr int kPartials = 1024;    // partial maxima of k_vmax

// the layers of one grid as a kernel sees them
struct Layers {
    const double *own, *lo, *hi;
};
template <int n>
struct LayersN {
    Layers v[n];
};
struct Out4 {
    double *p[4];
};
struct In4 {
    const double *p[4];
};

// layer l in [-H, nxl + H) of a grid; g2 = g*g
template <int H>
__device__ inline const double *layer_of(const Layers &a, int l, int nxl, i64 g2) {
    if (a.lo == nullptr) {
        l = l < 0 ? l + nxl : (l >= nxl ? l - nxl : l);
        return a.own + (i64)l * g2;
    }
    if (l < 0) return a.lo + (i64)(l + H) * g2;
    if (l >= nxl) return a.hi + (i64)(l - nxl) * g2;
    return a.own + (i64)l * g2;
}

__device__ inline int wrap(int a, int g) { return a < 0 ? a + g : (a >= g ? a - g : a); }

// layer l of each of the n grids
template <int H, int n>
__device__ inline void layers_of(const LayersN<n> &a, int l, int nxl, i64 g2,
                                 const double *(&layer)[n]) {
#pragma unroll
    for (int v = 0; v < n; v++) layer[v] = layer_of<H>(a.v[v], l, nxl, g2);
}

// What a workgroup of a step kernel (k_mc_step, k_pressure_sources, k_kt_step) works on: a tile of
// kTY x kTZ cells with its first cell at (y0, z0), a thread per cell, walked over the layers
// [xa, xb) of a chunk of xc layers along x.
struct StepTile {
    int y0, z0;   // the tile's first cell
    int ty, tz;   // the thread's cell within the tile
    int xa, xb;   // the layers of the walk
    bool mine;    // the thread's cell lies within the grid (a partial tile has threads that only stage)
    i64 col;      // the thread's cell within a layer, (y0 + ty) g + (z0 + tz); 0 when not mine
    __device__ StepTile(int g, int nxl, int xc)
        : y0(blockIdx.y * kTY), z0(blockIdx.x * kTZ), ty(threadIdx.x / kTZ), tz(threadIdx.x % kTZ),
          xa(blockIdx.z * xc), xb(xa + xc < nxl ? xa + xc : nxl), mine(y0 + ty < g && z0 + tz < g),
          col(mine ? (i64)(y0 + ty) * g + (z0 + tz) : 0) {}
};

// Stage EY x EZ cells of one layer of NV grids in LDS, by the whole workgroup: local (ly, lz) is
// cell (y + ly, z + lz) of the layer, wrapped, so a tile with a halo of h cells passes its first
// cell less h.  (A partial tile's rows beyond the grid wrap as well: loaded, never used.)  The
// caller synchronises.
template <int NV, int EY, int EZ>
__device__ inline void stage(const double *(&layer)[NV], int y, int z, int g,
                             double (&tile)[NV][EY][EZ]) {
    for (int e = threadIdx.x; e < EY * EZ; e += kThreads) {
        const int ly = e / EZ, lz = e - ly * EZ;
        const i64 at = (i64)((y + ly + g) % g) * g + (z + lz + g) % g;
#pragma unroll
        for (int v = 0; v < NV; v++) tile[v][ly][lz] = layer[v][at];
    }
}

// One MacCormack step.  src: ϱ, Jx, Jy, Jz as the stencil reads them (the unstarred grids in
// step 0, the starred in step 1) and 𝒫 (always the unstarred grid); dst: the four grids the step
// writes (the starred in step 0, the unstarred in step 1).  The prologue of fluid.py:862-870
// touches only dst — dst = src in step 0, dst += src in step 1 — so it is the first term of the
// cell's own sum.  A workgroup owns a tile of kTY x kTZ cells and walks kXC layers in the direction
// of the x step: the layer it reads as the +s_x neighbour is the layer it updates next, kept in
// the other half of the LDS buffer, and the +s_y and +s_z neighbours are the tile's own cells and
// one halo row and column.  Every cell is loaded once per walk (plus the halo).
__global__ __launch_bounds__(kThreads) void k_mc_step(LayersN<5> src, Out4 dst, int g, int nxl,
                                                      int sx, int sy, int sz, double c,
                                                      double inv_c2, int mc_step, int halve) {
#pragma clang fp contract(off)
    __shared__ double tile[2][5][kTY + 1][kTZ + 1];
    const StepTile t(g, nxl, kXC);
    const i64 g2 = (i64)g * g;
    // the halo row sits on the side the step points to
    const int oy = sy < 0, oz = sz < 0;
    auto load = [&](int buf, int l) {
        const double *layer[5];
        layers_of<1>(src, l, nxl, g2, layer);
        stage(layer, t.y0 - oy, t.z0 - oz, g, tile[buf]);
    };
    const int count = t.xb - t.xa, first = sx > 0 ? t.xa : t.xb - 1;
    const int cy = t.ty + oy, cz = t.tz + oz;
    load(0, first);
    for (int n = 0; n < count; n++) {
        const int l = first + n * sx, b = n & 1;
        load(b ^ 1, l + sx);
        __syncthreads();
        if (t.mine) {
            const i64 at = (i64)l * g2 + t.col;
            // the cell itself and its +s_x, +s_y, +s_z neighbours: J and ϱ + c⁻²𝒫
            double J0[3], JN[3][3], den0, denN[3];
#pragma unroll
            for (int el = 0; el < 3; el++) {
                J0[el] = tile[b][1 + el][cy][cz];
                JN[0][el] = tile[b ^ 1][1 + el][cy][cz];
                JN[1][el] = tile[b][1 + el][cy + sy][cz];
                JN[2][el] = tile[b][1 + el][cy][cz + sz];
            }
            const double rho0 = tile[b][0][cy][cz];
            den0 = rho0 + inv_c2 * tile[b][4][cy][cz];
            denN[0] = tile[b ^ 1][0][cy][cz] + inv_c2 * tile[b ^ 1][4][cy][cz];
            denN[1] = tile[b][0][cy + sy][cz] + inv_c2 * tile[b][4][cy + sy][cz];
            denN[2] = tile[b][0][cy][cz + sz] + inv_c2 * tile[b][4][cy][cz + sz];
            const double s[3] = {(double)sx, (double)sy, (double)sz};
            // the continuity equation, fluid.py:883-894
            double out = mc_step == 0 ? rho0 : dst.p[0][at] + rho0;
#pragma unroll
            for (int d = 0; d < 3; d++) out = out + (s[d] * (JN[d][d] - J0[d])) * c;
            dst.p[0][at] = halve ? 0.5 * out : out;
            // the Euler equation, fluid.py:915-939
#pragma unroll
            for (int el = 0; el < 3; el++) {
                out = mc_step == 0 ? J0[el] : dst.p[1 + el][at] + J0[el];
#pragma unroll
                for (int d = 0; d < 3; d++)
                    out = out + (s[d] * (JN[d][el] * JN[d][d] / denN[d] - J0[el] * J0[d] / den0)) * c;
                dst.p[1 + el][at] = halve ? 0.5 * out : out;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_mc_halve(Out4 grids, i64 n) {
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads) {
#pragma unroll
        for (int v = 0; v < 4; v++) grids.p[v][i] = grids.p[v][i] * 0.5;
    }
}

// mode 0: a*k1 + b < threshold, fac_time = 0.5 (a - b)/(a - ρ_vacuum)   (first step: a = ϱ, b = ϱˣ)
// mode 1: b < threshold, fac_time = 1                                   (second step: b = ϱ)
// mode 2: a < threshold, nothing written but the flag                   (check_vacuum)
__global__ __launch_bounds__(kThreads) void k_vacuum_detect(const double *__restrict__ a,
                                                           const double *__restrict__ b, i64 n,
                                                           int mode, double k1, double threshold,
                                                           double rho_vacuum,
                                                           double *__restrict__ fac_time,
                                                           int *__restrict__ flag) {
#pragma clang fp contract(off)
    int any = 0;
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads) {
        double ft = 0;
        bool imminent;
        if (mode == 0) {
            const double r = a[i], rs = b[i];
            imminent = r * k1 + rs < threshold;
            if (imminent) ft = 0.5 * (r - rs) / (r - rho_vacuum);
        } else if (mode == 1) {
            imminent = b[i] < threshold;
            if (imminent) ft = 1;
        } else {
            imminent = a[i] < threshold;
        }
        any |= imminent;
        if (mode != 2) fac_time[i] = ft;
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(flag, 1);
}

// The sweep of fluid.py:1289-1319 seen from the cell p that receives: every vacuum centre c whose
// 3x3x3 block holds p pairs p with the 26 other cells q of that block, and each pair moves
// (v[q] - v[p]) fac_smoothing fac_time(c) / |q - p|² to p.  Centres and, within a centre, the
// cells q are walked in ascending (x, y, z) offset, the order in which the reference's loops reach
// the pairs of an interior cell.  var: the four variables with two layers beyond the own ones,
// fac_time with one.
__global__ __launch_bounds__(kThreads) void k_vacuum_gather(LayersN<4> var, Layers fac_time,
                                                           Out4 delta, int g, int nxl,
                                                           double fac_smoothing) {
#pragma clang fp contract(off)
    const i64 g2 = (i64)g * g, n = (i64)nxl * g2;
    const i64 idx = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n) return;
    const int i = (int)(idx / g2), j = (int)((idx - (i64)i * g2) / g), k = (int)(idx % g);
    double vp[4], sum[4] = {0, 0, 0, 0};
#pragma unroll
    for (int v = 0; v < 4; v++) vp[v] = var.v[v].own[idx];
    for (int di = -1; di <= 1; di++)
        for (int dj = -1; dj <= 1; dj++)
            for (int dk = -1; dk <= 1; dk++) {
                const double ft =
                    layer_of<1>(fac_time, i + di, nxl, g2)[(i64)wrap(j + dj, g) * g + wrap(k + dk, g)];
                if (ft == 0) continue;
                const double f = fac_smoothing * ft;
                for (int ei = di - 1; ei <= di + 1; ei++)
                    for (int ej = dj - 1; ej <= dj + 1; ej++)
                        for (int ek = dk - 1; ek <= dk + 1; ek++) {
                            const int dist2 = ei * ei + ej * ej + ek * ek;
                            if (dist2 == 0) continue;
                            const double w = 1.0 / (double)dist2;
                            const i64 at = (i64)wrap(j + ej, g) * g + wrap(k + ek, g);
#pragma unroll
                            for (int v = 0; v < 4; v++) {
                                const double vq = layer_of<2>(var.v[v], i + ei, nxl, g2)[at];
                                sum[v] = sum[v] + (vq - vp[v]) * f * w;
                            }
                        }
            }
#pragma unroll
    for (int v = 0; v < 4; v++) delta.p[v][idx] = sum[v];
}

__global__ __launch_bounds__(kThreads) void k_vacuum_apply(Out4 var, In4 delta, i64 n) {
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads) {
#pragma unroll
        for (int v = 0; v < 4; v++) var.p[v][i] = var.p[v][i] + delta.p[v][i];
    }
}

// partial maxima per workgroup, then k_reduce_columns over the partials (cg_wave.h); the
// reference's compare (value > maximum, from 0: OpGreaterFrom0) lets no NaN in
__global__ __launch_bounds__(kThreads) void k_vmax(const double *__restrict__ rho,
                                                  const double *__restrict__ P, In4 J, i64 n,
                                                  double inv_c2, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[kThreads];
    double best = OpGreaterFrom0::identity();
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads) {
        const double jx = J.p[0][i], jy = J.p[1][i], jz = J.p[2][i];
        const double den = rho[i] + inv_c2 * P[i];
        const double v = (jx * jx + jy * jy + jz * jz) / (den * den);
        best = OpGreaterFrom0()(best, v);
    }
    best = block_tree<OpGreaterFrom0>(red, best);
    if (threadIdx.x == 0) out[blockIdx.x] = best;
}

// The realisation 𝒫 = ϱ (c²w) of the P = wρ approximation (ic.py:503-508) and the pressure term of
// maccormack_internal_sources (fluid.py:1044-1057) in one pass:
//   J_i += minus_dt * (half_inv_dx * (𝒫[+1_i] - 𝒫[-1_i]))      diff_domaingrid, order 2 (mesh.py:4966-4970)
// A workgroup owns a tile of kTY x kTZ cells, staged with one halo cell on every side, and walks
// kXC layers upwards along x with the layer below, the own one and the layer above resident in
// LDS; every ϱ value is loaded once per walk (plus the halo).  The six neighbour values of 𝒫 are
// formed from the staged ϱ by the product that fills the 𝒫 grid, so they are the bits the
// reference reads from that grid.  The stencil reads ϱ only: J and 𝒫 are updated in place.
__global__ __launch_bounds__(kThreads) void k_pressure_sources(Layers rho, double *__restrict__ P,
                                                               Out4 J, int g, int nxl, double c2w,
                                                               double minus_dt,
                                                               double half_inv_dx) {
#pragma clang fp contract(off)
    __shared__ double tile[3][1][kTY + 2][kTZ + 2];   // [buffer][the one grid staged: ϱ]
    const StepTile t(g, nxl, kXC);
    const i64 g2 = (i64)g * g;
    auto load = [&](int buf, int l) {
        const double *layer[1] = {layer_of<1>(rho, l, nxl, g2)};
        stage(layer, t.y0 - 1, t.z0 - 1, g, tile[buf]);
    };
    const int cy = t.ty + 1, cz = t.tz + 1;
    load(0, t.xa - 1);
    load(1, t.xa);
    for (int l = t.xa, n = 0; l < t.xb; l++, n++) {
        const int below = n % 3, own = (n + 1) % 3, above = (n + 2) % 3;
        load(above, l + 1);
        __syncthreads();
        if (t.mine) {
            const i64 at = (i64)l * g2 + t.col;
            P[at] = tile[own][0][cy][cz] * c2w;
            const double up[3] = {tile[above][0][cy][cz] * c2w, tile[own][0][cy + 1][cz] * c2w,
                                  tile[own][0][cy][cz + 1] * c2w};
            const double down[3] = {tile[below][0][cy][cz] * c2w, tile[own][0][cy - 1][cz] * c2w,
                                    tile[own][0][cy][cz - 1] * c2w};
#pragma unroll
            for (int d = 0; d < 3; d++)
                J.p[d][at] = J.p[d][at] + minus_dt * (half_inv_dx * (up[d] - down[d]));
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_realize_P(const double *__restrict__ rho,
                                                        double *__restrict__ P, i64 n,
                                                        double c2w) {
#pragma clang fp contract(off)
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < n; i += (i64)gridDim.x * kThreads)
        P[i] = rho[i] * c2w;
}

// -- the Kurganov-Tadmor scheme (fluid.py:103-673) -------------------------------------------------
constexpr int kKtXC = 16;   // layers a workgroup of the Kurganov-Tadmor step walks along x
constexpr int kKtH = 2;     // cells the stencil reaches to either side

enum KtLimiter {
    kMinmod, kMonotonizedCentral, kOspre, kSuperbee, kSweby, kUmist, kVanAlbada, kVanLeer, kKoren,
    kLimiters
};

// what a step needs besides the grids, formed by the caller as the reference's ℝ[...] expressions
struct KtFactors {
    double c2w;          // light_speed**2*w
    double inv_c2;       // light_speed**(-2)
    double a_pow;        // a**(3*w_eff - 2)
    double soundspeed;   // light_speed*sqrt(w)/a
    double f_J;          // ᔑdt['a**(3*w_eff-2)']/ᔑdt['1']
    double f_P;          // ᔑdt['a**(-3*w_eff)']/ᔑdt['1']
    double to_delta;     // (1 + rk_step)/rk_order*ᔑdt['1']/Δx
};

// slope_ratio, fluid.py:516-526
__device__ inline double kt_slope_ratio(double numerator, double denominator) {
    constexpr double eps = 1e+2 * 2.220446049250313e-16;
    constexpr double inv_eps = 1 / eps;
    if (fabs(numerator) < eps) return 0;
    if (fabs(denominator) < eps) {
        if (numerator > eps) return inv_eps;
        if (numerator < -eps) return -inv_eps;
    }
    return numerator / denominator;
}

// the flux limiters, fluid.py:588-673, branch by branch
template <int LIM>
__device__ inline double kt_limiter(double r) {
    if constexpr (LIM == kMinmod) {
        if (r > 1) return 1;
        if (r > 0) return r;
        return 0;
    } else if constexpr (LIM == kMonotonizedCentral) {
        if (r > 3) return 2;
        if (r > 1. / 3.) return 0.5 * (r + 1);
        if (r > 0) return 2 * r;
        return 0;
    } else if constexpr (LIM == kOspre) {
        if (r > 0) {
            const double r2 = r * r, s = r2 + r;
            return 1.5 * s / (s + 1);
        }
        return 0;
    } else if constexpr (LIM == kSuperbee) {
        if (r > 2) return 2;
        if (r > 1) return r;
        if (r > 0.5) return 1;
        if (r > 0) return 2 * r;
        return 0;
    } else if constexpr (LIM == kSweby) {
        constexpr double beta = 1.5, inv_beta = 1 / beta;
        if (r > beta) return beta;
        if (r > 1) return r;
        if (r > inv_beta) return 1;
        if (r > 0) return beta * r;
        return 0;
    } else if constexpr (LIM == kUmist) {
        if (r > 5) return 2;
        if (r > 1) return 0.75 + 0.25 * r;
        if (r > 0.2) return 0.25 + 0.75 * r;
        if (r > 0) return 2 * r;
        return 0;
    } else if constexpr (LIM == kVanAlbada) {
        if (r > 0) {
            const double r2 = r * r;
            return (r2 + r) / (r2 + 1);
        }
        return 0;
    } else if constexpr (LIM == kVanLeer) {
        if (r > 0) return 2 * r / (1 + r);
        return 0;
    } else {
        static_assert(LIM == kKoren, "unknown flux limiter");
        if (r > 2.5) return 2;
        if (r > 0.25) return 1. / 3. * (1 + 2 * r);
        if (r > 0) return 2 * r;
        return 0;
    }
}

// at_interface, fluid.py:486-504: the left and right value at the interface between the cells m
// and c, from the cells m2, m, c, p along one direction
template <int LIM>
__device__ inline void kt_at_interface(double m2, double m, double c, double p, double &left,
                                       double &right) {
    const double dcm = c - m, dpc = p - c;
    const double r_m = kt_slope_ratio(m - m2, dcm);
    const double r_c = kt_slope_ratio(dcm, dpc);
    left = m + 0.5 * kt_limiter<LIM>(r_m) * dcm;
    right = c - (0.5 * kt_limiter<LIM>(r_c)) * dpc;
}

// The numerical fluxes of ϱ, Jx, Jy, Jz through one interface across direction D
// (fluid.py:275-297, 373-418 with kurganov_tadmor_flux, :541-554), from the four cells m2, m, c, p
// of every variable along D; q[0] = ϱ, q[1 + i] = Jⁱ.  The interface values of ϱ, 𝒫 and J_D and the
// propagation speed do not depend on the variable that flows: formed once.  𝒫 of a cell is the
// product that fills the 𝒫 grid.
template <int LIM, int D>
__device__ inline void kt_flux(const double (&q)[4][4], const KtFactors &k, double (&flux)[4]) {
    double face[4][2], P[2], den[2], v[2];
#pragma unroll
    for (int var = 0; var < 4; var++)
        kt_at_interface<LIM>(q[var][0], q[var][1], q[var][2], q[var][3], face[var][0], face[var][1]);
    kt_at_interface<LIM>(q[0][0] * k.c2w, q[0][1] * k.c2w, q[0][2] * k.c2w, q[0][3] * k.c2w, P[0],
                         P[1]);
#pragma unroll
    for (int lr = 0; lr < 2; lr++) {
        den[lr] = face[0][lr] + k.inv_c2 * P[lr];
        v[lr] = fabs(k.a_pow * face[1 + D][lr] / den[lr]) + k.soundspeed;
    }
    // pairmax (commons.py:5091-5092)
    const double speed = v[0] * (double)(v[1] <= v[0]) + v[1] * (double)(v[0] < v[1]);
    const bool use_P = k.c2w != 0;
    double f[2];
#pragma unroll
    for (int lr = 0; lr < 2; lr++) f[lr] = k.f_J * face[1 + D][lr];
    flux[0] = 0.5 * ((f[1] + f[0]) - speed * (face[0][1] - face[0][0]));
#pragma unroll
    for (int m = 0; m < 3; m++) {
#pragma unroll
        for (int lr = 0; lr < 2; lr++) {
            f[lr] = k.f_J * (face[1 + m][lr] * face[1 + D][lr] / den[lr]);
            if (m == D && use_P) f[lr] = f[lr] + k.f_P * P[lr];
        }
        flux[1 + m] = 0.5 * ((f[1] + f[0]) - speed * (face[1 + m][1] - face[1 + m][0]));
    }
}

// What the cell at (cy, cz) of a staged layer receives through its two faces across direction D
// (1: y, 2: z), the lower face first: out += Δ(-½), then out -= Δ(+½), with Δ = flux*to_delta.
// The two faces share three of their four cells: the five cells of the line are read once (read
// per face, the compiler keeps the second face's loads apart and spills more registers).
template <int LIM, int D, int EY, int EZ>
__device__ inline void kt_add_faces(const double (&tile)[4][EY][EZ], int cy, int cz,
                                    const KtFactors &k, double (&out)[4]) {
#pragma clang fp contract(off)
    static_assert(D == 1 || D == 2, "the faces along x are the walk's own");
    double line[4][5], flux[4], q[4][4];
#pragma unroll
    for (int var = 0; var < 4; var++)
#pragma unroll
        for (int o = 0; o < 5; o++)
            line[var][o] = D == 1 ? tile[var][cy - 2 + o][cz] : tile[var][cy][cz - 2 + o];
#pragma unroll
    for (int side = 0; side < 2; side++) {
#pragma unroll
        for (int var = 0; var < 4; var++)
#pragma unroll
            for (int o = 0; o < 4; o++) q[var][o] = line[var][side + o];
        kt_flux<LIM, D>(q, k, flux);
#pragma unroll
        for (int var = 0; var < 4; var++)
            out[var] = side ? out[var] - flux[var] * k.to_delta : out[var] + flux[var] * k.to_delta;
    }
}

// One Runge-Kutta step of kurganov_tadmor (fluid.py:103-464) with its finalize_rk_step
// (:565-586), as a gather.  The reference scatters Δ = flux*to_delta of every interface to the two
// cells beside it, in loops over the variable, the direction and the interfaces in ascending
// (i, j, k); a cell therefore receives, per variable, +Δ(x-½), -Δ(x+½), +Δ(y-½), -Δ(y+½),
// +Δ(z-½), -Δ(z+½) in this order, onto 0 in step 0 (the unstarred value is added last) and onto
// the unstarred value in step 1.  src: the grids the stencil reads (the unstarred in step 0, the
// starred in step 1), with kKtH layers beyond the own ones; dst: the grids written (the starred in
// step 0, the unstarred in step 1).  P receives the realisation ϱ (c²w) of the grid that is read
// (realize_if_linear(2, 'trace', use_gridˣ), fluid.py:240).
// A workgroup owns a tile of kTY x kTZ cells and walks kKtXC layers upwards.  A thread keeps the
// four x-neighbours of the next x-interface of its column in registers and hands the flux through
// x+½ to the next layer as its flux through x-½; the own layer is staged in LDS with a halo of two
// cells in y and z.
template <int LIM>
__global__ __launch_bounds__(kThreads) void k_kt_step(LayersN<4> src, Out4 dst,
                                                      double *__restrict__ P, int g, int nxl,
                                                      int rk_step, KtFactors k) {
#pragma clang fp contract(off)
    __shared__ double tile[4][kTY + 2 * kKtH][kTZ + 2 * kKtH];
    // (the StepTile of this kernel, spelt out: built through the struct, the same values reach the
    // register allocator in another order, and this kernel, at the register limit, moves more
    // values to and from the accumulation registers and runs 1 % slower)
    const int tz = threadIdx.x % kTZ, ty = threadIdx.x / kTZ;
    const int z0 = blockIdx.x * kTZ, y0 = blockIdx.y * kTY;
    const int xa = blockIdx.z * kKtXC, xb = xa + kKtXC < nxl ? xa + kKtXC : nxl;
    const i64 g2 = (i64)g * g;
    const bool mine = y0 + ty < g && z0 + tz < g;
    const int cy = ty + kKtH, cz = tz + kKtH;
    const i64 col = mine ? (i64)(y0 + ty) * g + (z0 + tz) : 0;
    // the cells xa-2 .. xa+1 of the column, and the flux through xa-½
    double w[4][4], lower[4] = {0, 0, 0, 0};
    if (mine) {
#pragma unroll
        for (int var = 0; var < 4; var++)
#pragma unroll
            for (int o = 0; o < 4; o++)
                w[var][o] = layer_of<kKtH>(src.v[var], xa - 2 + o, nxl, g2)[col];
        kt_flux<LIM, 0>(w, k, lower);
    }
    for (int l = xa; l < xb; l++) {
        const double *layer[4];
        layers_of<kKtH>(src, l, nxl, g2, layer);
        stage(layer, y0 - kKtH, z0 - kKtH, g, tile);
        __syncthreads();
        if (mine) {
            const i64 at = (i64)l * g2 + col;
            double out[4];
#pragma unroll
            for (int var = 0; var < 4; var++) {
                out[var] = rk_step == 0 ? 0.0 : dst.p[var][at];
                out[var] = out[var] + lower[var] * k.to_delta;
                // the cells l-1 .. l+2 of the column: the interface l+½
                w[var][0] = w[var][1];
                w[var][1] = w[var][2];
                w[var][2] = w[var][3];
                w[var][3] = layer_of<kKtH>(src.v[var], l + 2, nxl, g2)[col];
            }
            kt_flux<LIM, 0>(w, k, lower);
#pragma unroll
            for (int var = 0; var < 4; var++) out[var] = out[var] - lower[var] * k.to_delta;
            kt_add_faces<LIM, 1>(tile, cy, cz, k, out);
            kt_add_faces<LIM, 2>(tile, cy, cz, k, out);
            if (P) P[at] = w[0][1] * k.c2w;
#pragma unroll
            for (int var = 0; var < 4; var++)
                dst.p[var][at] = rk_step == 0 ? out[var] + w[var][1] : out[var];
        }
        __syncthreads();
    }
}

unsigned grid_for(i64 n, i64 cap) {
    i64 blocks = (n + kThreads - 1) / kThreads;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// an element-wise kernel over n elements: grid stride, at most `cap` workgroups
template <class Kernel, class... Args>
int launch_stride(cg_ctx *c, Kernel kernel, i64 n, i64 cap, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, cap)), dim3(kThreads), 0, c->stream, args...);
    CG_LAUNCH_CHECK();
    return 0;
}

// a step kernel: a workgroup per StepTile with chunks of xc layers
dim3 tile_grid(int64_t gridsize, int64_t nxl, int xc) {
    return dim3((unsigned)((gridsize + kTZ - 1) / kTZ), (unsigned)((gridsize + kTY - 1) / kTY),
                (unsigned)((nxl + xc - 1) / xc));
}

// the first `count` grids of a pack (Out4 or In4); `what` names a missing one ("null grid")
template <class Pack, class Ptr>
int take4(const char *who, const char *what, Ptr *const *ptrs, int count, Pack &out) {
    using Grid = std::remove_reference_t<decltype(*out.p)>;
    for (int v = 0; v < count; v++) {
        CG_CHECK(ptrs[v], "%s: %s %d", who, what, v);
        out.p[v] = (Grid)ptrs[v];
    }
    return 0;
}

// The stencil must not read what the pass writes, and no grid is written twice: refuses a written
// grid that is one of those read, and two written grids that are one.  `what` names a written grid.
int check_aliasing(const char *who, const char *what, const void *const *reads, int nreads,
                   const void *const *writes, int nwrites) {
    for (int v = 0; v < nwrites; v++) {
        for (int u = 0; u < nreads; u++)
            CG_CHECK(writes[v] != reads[u], "%s: %s %d is read and written", who, what, v);
        for (int u = 0; u < v; u++)
            CG_CHECK(writes[v] != writes[u], "%s: %ss %d and %d are one", who, what, u, v);
    }
    return 0;
}

// nvar grids with their layers beyond the own ones (both lists or neither)
int take_layers(const char *who, Layers *out, int nvar, const void *const *own,
                const void *const *lo, const void *const *hi) {
    CG_CHECK(own, "%s: null argument", who);
    CG_CHECK((lo == nullptr) == (hi == nullptr), "%s: give both lo and hi or neither", who);
    for (int v = 0; v < nvar; v++) {
        CG_CHECK(own[v] && (!lo || (lo[v] && hi[v])), "%s: null grid %d", who, v);
        out[v] = Layers{(const double *)own[v], lo ? (const double *)lo[v] : nullptr,
                        hi ? (const double *)hi[v] : nullptr};
    }
    return 0;
}

int check_shape(const char *who, int64_t gridsize, int64_t nxl, bool periodic, int H) {
    CG_CHECK(gridsize >= 3 && gridsize <= 32768, "%s: grid size %lld", who, (long long)gridsize);
    CG_CHECK(nxl >= H && nxl <= gridsize, "%s: %lld layers of a grid of size %lld (at least %d)",
             who, (long long)nxl, (long long)gridsize, H);
    CG_CHECK(!periodic || nxl == gridsize,
             "%s: %lld of %lld layers and no layers of the neighbouring domains", who,
             (long long)nxl, (long long)gridsize);
    return 0;
}

}  // namespace

extern "C" int cg_fluid_mc_step(cg_ctx *c, const void *const *src, const void *const *src_lo,
                                const void *const *src_hi, void *const *dst, int64_t gridsize,
                                int64_t nxl, const int *steps, double factor, double inv_c2,
                                int mc_step, int halve) {
    CG_CHECK(c && dst && steps, "cg_fluid_mc_step: null argument");
    LayersN<5> s;
    if (take_layers("cg_fluid_mc_step", s.v, 5, src, src_lo, src_hi)) return 1;
    if (check_shape("cg_fluid_mc_step", gridsize, nxl, src_lo == nullptr, 1)) return 1;
    CG_CHECK(mc_step == 0 || mc_step == 1, "cg_fluid_mc_step: mc_step %d", mc_step);
    for (int i = 0; i < 3; i++)
        CG_CHECK(steps[i] == 1 || steps[i] == -1, "cg_fluid_mc_step: step %d", steps[i]);
    Out4 d;
    if (take4("cg_fluid_mc_step", "null grid", dst, 4, d)) return 1;
    if (check_aliasing("cg_fluid_mc_step", "grid", src, 5, dst, 4)) return 1;
    hipLaunchKernelGGL(k_mc_step, tile_grid(gridsize, nxl, kXC), dim3(kThreads), 0, c->stream, s, d,
                       (int)gridsize, (int)nxl, steps[0], steps[1], steps[2], factor, inv_c2,
                       mc_step, halve);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_fluid_kt_step(cg_ctx *c, const void *const *src, const void *const *src_lo,
                                const void *const *src_hi, void *const *dst, double *P,
                                int64_t gridsize, int64_t nxl, int limiter, int rk_step, double c2w,
                                double inv_c2, double a_pow, double soundspeed, double f_J,
                                double f_P, double to_delta) {
    CG_CHECK(c && dst, "cg_fluid_kt_step: null argument");
    LayersN<4> s;
    if (take_layers("cg_fluid_kt_step", s.v, 4, src, src_lo, src_hi)) return 1;
    if (check_shape("cg_fluid_kt_step", gridsize, nxl, src_lo == nullptr, kKtH)) return 1;
    CG_CHECK(rk_step == 0 || rk_step == 1, "cg_fluid_kt_step: rk_step %d", rk_step);
    CG_CHECK(limiter >= 0 && limiter < kLimiters, "cg_fluid_kt_step: flux limiter %d", limiter);
    Out4 d;
    if (take4("cg_fluid_kt_step", "null grid", dst, 4, d)) return 1;
    if (check_aliasing("cg_fluid_kt_step", "grid", src, 4, dst, 4)) return 1;
    // (𝒫 is written as well, and may be left out)
    for (int v = 0; v < 4; v++)
        CG_CHECK(src[v] != (const void *)P && dst[v] != (void *)P,
                 "cg_fluid_kt_step: 𝒫 and grid %d are one", v);
    const KtFactors k{c2w, inv_c2, a_pow, soundspeed, f_J, f_P, to_delta};
    return with_case<kLimiters>(limiter, [=](auto lim) {
        hipLaunchKernelGGL(k_kt_step<decltype(lim)::value>, tile_grid(gridsize, nxl, kKtXC),
                           dim3(kThreads), 0, c->stream, s, d, P, (int)gridsize, (int)nxl, rk_step,
                           k);
        CG_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int cg_fluid_mc_finish(cg_ctx *c, void *const *grids, void *const *starred,
                                  void *const *delta, int64_t n, int halve) {
    CG_CHECK(c && grids && starred && n >= 1, "cg_fluid_mc_finish: null argument");
    if (halve) {
        Out4 gr;
        if (take4("cg_fluid_mc_finish", "null grid", grids, 4, gr)) return 1;
        if (launch_stride(c, k_mc_halve, n, 4096, gr, (i64)n)) return 1;
    }
    for (int v = 0; v < 4; v++) {
        CG_CHECK(starred[v], "cg_fluid_mc_finish: null starred grid %d", v);
        CG_HIP(hipMemsetAsync(starred[v], 0, sizeof(double) * n, c->stream));
        if (delta && delta[v]) CG_HIP(hipMemsetAsync(delta[v], 0, sizeof(double) * n, c->stream));
    }
    return 0;
}

extern "C" int cg_fluid_vacuum_detect(cg_ctx *c, const double *a, const double *b, int64_t n,
                                      int mode, double k1, double threshold, double rho_vacuum,
                                      double *fac_time, int *flag) {
    CG_CHECK(c && flag && n >= 1, "cg_fluid_vacuum_detect: null argument");
    CG_CHECK(mode >= 0 && mode <= 2, "cg_fluid_vacuum_detect: mode %d", mode);
    CG_CHECK((mode == 1 || a) && (mode == 2 || (b && fac_time)),
             "cg_fluid_vacuum_detect: null grid for mode %d", mode);
    CG_HIP(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    return launch_stride(c, k_vacuum_detect, n, 4096, a, b, (i64)n, mode, k1, threshold, rho_vacuum,
                         fac_time, flag);
}

extern "C" int cg_fluid_vacuum_gather(cg_ctx *c, const void *const *var, const void *const *var_lo,
                                      const void *const *var_hi, const double *fac_time,
                                      const double *fac_time_lo, const double *fac_time_hi,
                                      void *const *delta, int64_t gridsize, int64_t nxl,
                                      double fac_smoothing) {
    CG_CHECK(c && delta && fac_time, "cg_fluid_vacuum_gather: null argument");
    LayersN<4> s;
    if (take_layers("cg_fluid_vacuum_gather", s.v, 4, var, var_lo, var_hi)) return 1;
    if (check_shape("cg_fluid_vacuum_gather", gridsize, nxl, var_lo == nullptr, 2)) return 1;
    CG_CHECK((fac_time_lo == nullptr) == (var_lo == nullptr) &&
                 (fac_time_hi == nullptr) == (var_lo == nullptr),
             "cg_fluid_vacuum_gather: fac_time and the variables need the same neighbours");
    Out4 d;
    if (take4("cg_fluid_vacuum_gather", "Δ buffer", delta, 4, d)) return 1;
    const void *reads[5] = {var[0], var[1], var[2], var[3], fac_time};
    if (check_aliasing("cg_fluid_vacuum_gather", "Δ buffer", reads, 5, delta, 4)) return 1;
    const i64 n = nxl * gridsize * gridsize;
    hipLaunchKernelGGL(k_vacuum_gather, dim3((unsigned)((n + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, c->stream, s, Layers{fac_time, fac_time_lo, fac_time_hi},
                       d, (int)gridsize, (int)nxl, fac_smoothing);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_fluid_vacuum_apply(cg_ctx *c, void *const *var, const void *const *delta,
                                     int64_t n) {
    CG_CHECK(c && var && delta && n >= 1, "cg_fluid_vacuum_apply: null argument");
    Out4 o;
    In4 d;
    if (take4("cg_fluid_vacuum_apply", "null grid", var, 4, o) ||
        take4("cg_fluid_vacuum_apply", "null grid", delta, 4, d))
        return 1;
    if (check_aliasing("cg_fluid_vacuum_apply", "grid", delta, 4, var, 4)) return 1;
    return launch_stride(c, k_vacuum_apply, n, 4096, o, d, (i64)n);
}

extern "C" int cg_fluid_vmax(cg_ctx *c, const double *rho, const double *P, const void *const *J,
                             int64_t n, double inv_c2, double *out) {
    CG_CHECK(c && rho && P && J && out && n >= 1, "cg_fluid_vmax: null argument");
    In4 j{};
    if (take4("cg_fluid_vmax", "null grid", J, 3, j)) return 1;
    if (c->fluid_partial.reserve(c, sizeof(double) * kPartials)) return 1;
    if (launch_stride(c, k_vmax, n, kPartials, rho, P, j, (i64)n, inv_c2,
                      (double *)c->fluid_partial))
        return 1;
    hipLaunchKernelGGL(k_reduce_columns<OpGreaterFrom0>, dim3(1), dim3(256), 0, c->stream,
                       (const double *)c->fluid_partial, (i64)grid_for(n, kPartials), (i64)1, out);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_fluid_pressure_sources(cg_ctx *c, const double *rho, const double *rho_lo,
                                         const double *rho_hi, double *P, void *const *J,
                                         int64_t gridsize, int64_t nxl, double c2w,
                                         double minus_dt, double half_inv_dx) {
    CG_CHECK(c && P, "cg_fluid_pressure_sources: null argument");
    const void *own[1] = {rho}, *lo[1] = {rho_lo}, *hi[1] = {rho_hi};
    Layers r;
    if (take_layers("cg_fluid_pressure_sources", &r, 1, own, rho_lo ? lo : nullptr,
                    rho_hi ? hi : nullptr))
        return 1;
    // (the realisation alone reads no neighbour: any number of own layers, no lo and hi)
    if (check_shape("cg_fluid_pressure_sources", gridsize, nxl, J && rho_lo == nullptr, 1))
        return 1;
    CG_CHECK((const double *)P != rho, "cg_fluid_pressure_sources: 𝒫 and ϱ are one grid");
    if (!J) {   // the realisation alone
        const i64 n = nxl * gridsize * gridsize;
        return launch_stride(c, k_realize_P, n, 4096, rho, P, n, c2w);
    }
    Out4 j{};
    if (take4("cg_fluid_pressure_sources", "J grid", J, 3, j)) return 1;
    // (𝒫 is written as well: it counts as J grid 3)
    const void *reads[1] = {rho}, *writes[4] = {J[0], J[1], J[2], P};
    if (check_aliasing("cg_fluid_pressure_sources", "J grid", reads, 1, writes, 4)) return 1;
    hipLaunchKernelGGL(k_pressure_sources, tile_grid(gridsize, nxl, kXC), dim3(kThreads), 0,
                       c->stream, r, P, j, (int)gridsize, (int)nxl, c2w, minus_dt, half_inv_dx);
    CG_LAUNCH_CHECK();
    return 0;
}
