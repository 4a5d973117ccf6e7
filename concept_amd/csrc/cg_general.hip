// cg_general.hip — the pieces of the GENERAL particle_mesh() that the fused
// fast path does not need: several suppliers and
// receivers, particles and fluids, added together in Fourier space.
//   k_fluid_add         add_fluid_to_grid                 mesh.py:1685-1753
//   k_nullify_nyquist   nullify_modes('nyquist')          mesh.py:3591-3622
//   k_fourier_operate   fourier_operate / copy_modes      mesh.py:3327-3400, 1038-1092
//                       (equal grid sizes) over fourier_loop   mesh.py:2615-2890
//   k_fluid_kick        diff_domaingrid + the fluid branch of
//                       apply_particle_mesh_force         mesh.py:4874-5030,
//                                                         interactions.py:2388-2401
// Fluid grids are double[N][N][N] (the reference's grid_noghosts order); the
// mesh is double[N][N][pad] / complex[N][N][pad/2], un-transposed: the first
// index is x (the reference's ki), the second y (kj).
// Compiled with -ffp-contract=off; every expression keeps the reference's order.
#include "cg_chunk_box.h"
#include "cg_internal.h"

// Fluid grids of an x-slab domain are its own layers double[nxl][N][N]; `mesh` is then the
// first OWNED layer of the local buffer.
__global__ __launch_bounds__(256) void k_fluid_add(double *__restrict__ mesh,
                                                   const double *__restrict__ fluid, int N,
                                                   int nxl, i64 ny, i64 pad, double factor,
                                                   int op_add) {
    // one thread per (i, j, k-pair): rows of the fluid grid are contiguous
    const i64 total = (i64)nxl * N * N;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (i64)gridDim.x * blockDim.x) {
        i64 row = t / N;
        int k = (int)(t - row * N);
        double v = fluid[t];
        if (factor != 1) v = v * factor;  // mesh.py:1737-1751
        i64 i = row / N;
        double *dst = mesh + (i * ny + (row - i * N)) * pad + k;
        if (op_add) *dst += v;
        else *dst = v;
    }
}

__global__ __launch_bounds__(256) void k_nullify_nyquist(double2 *__restrict__ four, int N,
                                                         i64 si, i64 cp, int j0, int nj) {
    // Fourier view (cg_ctx::four): planes a == nyq, b == nyq, kk == nyq
    const int nyq = N / 2;
    const i64 rows = (i64)N * nj;
    for (i64 row = (i64)blockIdx.x; row < rows; row += gridDim.x) {
        int a = (int)(row / nj), bl = (int)(row - (i64)a * nj), b = j0 + bl;
        double2 *r = four + (i64)a * si + (i64)bl * cp;
        if (a == nyq || b == nyq) {
            for (int kk = threadIdx.x; kk <= nyq; kk += blockDim.x) r[kk] = make_double2(0, 0);
        } else if (threadIdx.x == 0) {
            r[nyq] = make_double2(0, 0);
        }
    }
}

struct FourierOp {
    const double *tab_n, *tab_s;
    int deconv_order, nlattice, diff_dim, shifted, op_add, zero_nyquist;
    double A, B, Cc;  // -2*pi/N*shift[d]
    double k_fundamental, inv_lat;
};

__global__ __launch_bounds__(256) void k_fourier_operate(const double2 *__restrict__ from,
                                                         double2 *__restrict__ onto, int N,
                                                         i64 si, i64 cp, int j0, int nj,
                                                         FourierOp P) {
#pragma clang fp contract(off)
    const int nyq = N / 2;
    const i64 rows = (i64)N * nj;
    for (i64 row = (i64)blockIdx.x; row < rows; row += gridDim.x) {
        const int a = (int)(row / nj), bl = (int)(row - (i64)a * nj), b = j0 + bl;
        const double2 *src = from + (i64)a * si + (i64)bl * cp;
        double2 *dst = onto + (i64)a * si + (i64)bl * cp;
        const bool dead_row = (a == nyq) || (b == nyq);
        const int ka = a - (a >= nyq ? N : 0), kb = b - (b >= nyq ? N : 0);
        double dab_n = 0, dab_d = 0;
        if (P.deconv_order) {
            dab_n = P.tab_n[a] * P.tab_n[b];  // mesh.py:2797-2798
            dab_d = P.tab_s[a] * P.tab_s[b];
        }
        for (int kk = threadIdx.x; kk <= nyq; kk += blockDim.x) {
            if (dead_row || kk == nyq) {
                if (P.zero_nyquist) dst[kk] = make_double2(0, 0);
                continue;
            }
            double factor = 1;
            if (P.deconv_order) {
                factor = (dab_n * P.tab_n[kk]) / (dab_d * P.tab_s[kk]);  // mesh.py:2850-2853
                double f = factor;
                for (int o = 1; o < P.deconv_order; o++) factor *= f;   // factor **= order
            }
            factor *= P.inv_lat;  // mesh.py:2856
            double re = src[kk].x, im = src[kk].y;
            if (P.shifted) {
                double theta = ((double)ka * P.A + (double)kb * P.B) + (double)kk * P.Cc;
                double c = cos(theta), s = sin(theta);
                double re2 = re * c - im * s, im2 = re * s + im * c;  // mesh.py:3376-3379
                re = re2;
                im = im2;
            }
            if (P.diff_dim >= 0) {
                int kl = P.diff_dim == 0 ? ka : (P.diff_dim == 1 ? kb : kk);
                factor *= P.k_fundamental * (double)kl;  // mesh.py:3391-3392
                double t = re;
                re = -im;
                im = t;
            }
            re *= factor;
            im *= factor;
            if (P.op_add) dst[kk] = make_double2(dst[kk].x + re, dst[kk].y + im);
            else dst[kk] = make_double2(re, im);
        }
    }
}

// copy_modes between DIFFERENT grid sizes (mesh.py:1094-1326): one workgroup per (a, b)
// row of the smaller grid, lanes over kk.  Deconvolution and lattice phase use the grid
// size of `from` (fourier_loop's gridsize_corrections, mesh.py:1245-1250); the extra
// rotation theta = (pi/N_onto - pi/N_from)*((ki + kj) + kk) re-centres the cell-centred
// grid values (mesh.py:1302).
struct CopyModes {
    const double *tab_n, *tab_s;  // of the `from` context (indexed by ITS array index)
    int deconv_order, shifted, op_add;
    double A, B, Cc, dtheta, inv_lat;
};
static CopyModes copy_modes_params(cg_ctx *onto, cg_ctx *from, int deconv_order, int nlattice,
                                    const double *shift, int op_add);
__global__ __launch_bounds__(64) void k_copy_modes(const double2 *__restrict__ from, int N_from,
                                                   i64 ny_from, i64 cp_from,
                                                   double2 *__restrict__ onto, int N_onto,
                                                   i64 ny_onto, i64 cp_onto, CopyModes P) {
#pragma clang fp contract(off)
    const int N_small = N_from < N_onto ? N_from : N_onto;
    const int nyq = N_small / 2;
    const i64 rows = (i64)N_small * N_small;
    for (i64 row = (i64)blockIdx.x; row < rows; row += gridDim.x) {
        const int as = (int)(row / N_small), bs = (int)(row - (i64)as * N_small);
        if (as == nyq || bs == nyq) continue;
        const int ka = as - (as >= nyq ? N_small : 0), kb = bs - (bs >= nyq ? N_small : 0);
        const int af = ka + (ka < 0 ? N_from : 0), bf = kb + (kb < 0 ? N_from : 0);
        const int ao = ka + (ka < 0 ? N_onto : 0), bo = kb + (kb < 0 ? N_onto : 0);
        const double2 *src = from + ((i64)af * ny_from + bf) * cp_from;
        double2 *dst = onto + ((i64)ao * ny_onto + bo) * cp_onto;
        double dab_n = 0, dab_d = 0;
        if (P.deconv_order) {
            dab_n = P.tab_n[af] * P.tab_n[bf];
            dab_d = P.tab_s[af] * P.tab_s[bf];
        }
        for (int kk = threadIdx.x; kk < nyq; kk += blockDim.x) {
            double factor = 1;
            if (P.deconv_order) {
                factor = (dab_n * P.tab_n[kk]) / (dab_d * P.tab_s[kk]);
                double f = factor;
                for (int o = 1; o < P.deconv_order; o++) factor *= f;
            }
            factor *= P.inv_lat;
            double re = src[kk].x, im = src[kk].y;
            double theta = P.dtheta * (double)((ka + kb) + kk);  // mesh.py:1302
            if (P.shifted) theta += ((double)ka * P.A + (double)kb * P.B) + (double)kk * P.Cc;
            double c = cos(theta), s = sin(theta);
            double re2 = factor * (re * c - im * s), im2 = factor * (re * s + im * c);
            if (P.op_add) dst[kk] = make_double2(dst[kk].x + re2, dst[kk].y + im2);
            else dst[kk] = make_double2(re2, im2);
        }
    }
}

// copy_modes between different grid sizes over x-slab domains (get_subslabs / the sub-slab
// exchange of mesh.py:1327-1468): a row kj of the small cube lives on different domains in
// the two grids' decompositions, so it travels.  Pack: the small-cube part of the listed
// local rows of `from`, out[r][as][kk] (as = array index of ki in the SMALL grid, kk < nyq).
// Unpack: what k_copy_modes does per row, reading the packed rows.
__global__ __launch_bounds__(64) void k_cm_pack(const double2 *__restrict__ from, int N_from,
                                                i64 si, i64 cp, const int *__restrict__ rows,
                                                i64 n_rows, int NS, double2 *__restrict__ out) {
    const int nyq = NS / 2;
    for (i64 w = blockIdx.x; w < n_rows * NS; w += gridDim.x) {
        const i64 r = w / NS;
        const int as = (int)(w - r * NS);
        if (as == nyq) continue;
        const int ka = as - (as >= nyq ? NS : 0);
        const int af = ka + (ka < 0 ? N_from : 0);
        const double2 *src = from + (i64)af * si + (i64)rows[r] * cp;
        double2 *dst = out + (r * NS + as) * nyq;
        for (int kk = threadIdx.x; kk < nyq; kk += blockDim.x) dst[kk] = src[kk];
    }
}
__global__ __launch_bounds__(64) void k_cm_unpack(const double2 *__restrict__ in, int NS,
                                                  const int *__restrict__ rows, i64 n_rows,
                                                  double2 *__restrict__ onto, int N_onto, i64 si,
                                                  i64 cp, int j0, int N_from, CopyModes P) {
#pragma clang fp contract(off)
    const int nyq = NS / 2;
    for (i64 w = blockIdx.x; w < n_rows * NS; w += gridDim.x) {
        const i64 r = w / NS;
        const int as = (int)(w - r * NS);
        if (as == nyq) continue;
        const int bo = j0 + rows[r];
        const int kb = bo - (bo >= N_onto / 2 ? N_onto : 0);
        const int ka = as - (as >= nyq ? NS : 0);
        const int af = ka + (ka < 0 ? N_from : 0), bf = kb + (kb < 0 ? N_from : 0);
        const int ao = ka + (ka < 0 ? N_onto : 0);
        const double2 *src = in + (r * NS + as) * nyq;
        double2 *dst = onto + (i64)ao * si + (i64)rows[r] * cp;
        double dab_n = 0, dab_d = 0;
        if (P.deconv_order) {
            dab_n = P.tab_n[af] * P.tab_n[bf];
            dab_d = P.tab_s[af] * P.tab_s[bf];
        }
        for (int kk = threadIdx.x; kk < nyq; kk += blockDim.x) {
            double factor = 1;
            if (P.deconv_order) {
                factor = (dab_n * P.tab_n[kk]) / (dab_d * P.tab_s[kk]);
                double f = factor;
                for (int o = 1; o < P.deconv_order; o++) factor *= f;
            }
            factor *= P.inv_lat;
            double re = src[kk].x, im = src[kk].y;
            double theta = P.dtheta * (double)((ka + kb) + kk);  // mesh.py:1302
            if (P.shifted) theta += ((double)ka * P.A + (double)kb * P.B) + (double)kk * P.Cc;
            double c = cos(theta), s = sin(theta);
            double re2 = factor * (re * c - im * s), im2 = factor * (re * s + im * c);
            if (P.op_add) dst[kk] = make_double2(dst[kk].x + re2, dst[kk].y + im2);
            else dst[kk] = make_double2(re2, im2);
        }
    }
}

#define CG_FD_SWITCH(order, KERNEL, ...)                                          \
    switch (order) {                                                              \
        case 0: hipLaunchKernelGGL(KERNEL<0>, __VA_ARGS__); break;                \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                \
        case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                \
        case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                \
        default: hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__); break;               \
    }

template <int ORDER>
__global__ __launch_bounds__(256) void k_fluid_kick(double *__restrict__ J,
                                                    const double *__restrict__ rho,
                                                    const double *__restrict__ P,
                                                    const double *__restrict__ mesh, int N,
                                                    XMap xm, i64 ny, i64 pad, int dim, FdCoef fc,
                                                    double mdt, double inv_c2) {
#pragma clang fp contract(off)
    // `mesh` is the local buffer (ghost layers included); the fluid grids hold the owned layers
    const i64 total = (i64)xm.nxl * N * N;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (i64)gridDim.x * blockDim.x) {
        i64 row = t / N;
        int k = (int)(t - row * N);
        int i = (int)(row / N), j = (int)(row - (i64)i * N);
        auto phi = [&](int s) {
            i64 ii = cg_xlayer(xm, xm.x0 + i + (dim == 0 ? s : 0), N);
            int jj = j, kk = k;
            if (dim == 1) jj = wrap(j + s, N);
            else if (dim == 2) kk = wrap(k + s, N);
            return mesh[(ii * ny + jj) * pad + kk];
        };
        const double g = fd_value<ORDER>(phi, fc);
        // Jᵢ += ℝ[-ᔑdt]*(ϱ + ℝ[c⁻²]*𝒫)*grid   (interactions.py:2397-2400)
        J[t] += mdt * (rho[t] + inv_c2 * P[t]) * g;
    }
}

// ---------------------------------------------------------------------------
// Particle interpolation of every order: deposit and scalar gather with
// the weights of set_weights_NGP / CIC / TSC / PCS and the loops over ORDER^3 grid points
// (mesh.py:5052-5283), with the coordinate map of interpolate_particles (mesh.py:1512-1636,
// lattice shift subtracted) or interpolate_domaingrid_to_particles (mesh.py:376-459, lattice
// shift added) in `geo`.  Particles in any memory order, through the chunk boxes of
// cg_chunk_box.h (the scheme and its measurements are described there); cg_deposit_cic is the
// order-2 deposit.  The tiled CIC kernels keep the default configuration's tile-sorted path.
// ---------------------------------------------------------------------------
template <int ORDER>
__global__ __launch_bounds__(kChunkLanes) void k_deposit_general(const double *__restrict__ pos,
                                                                 i64 n, double *__restrict__ mesh,
                                                                 int N, i64 ny, i64 pad, int g,
                                                                 XMap xm, CicGeom geo,
                                                                 double contribution) {
#pragma clang fp contract(off)
    __shared__ double blk[kChunkCells];
    double x[kChunkPer][3];
    int cell[kChunkPer][3];
    chunk_load<ORDER>(pos, n, geo, g, N, x, cell);
    const ChunkBox<ORDER> B = chunk_box<ORDER>(cell, n, N);
    chunk_zero(B, blk);
#pragma unroll 1
    for (int u = 0; u < kChunkPer; u++) {
        if (chunk_particle(u) >= n) continue;
        double wx[4], wy[4], wz[4];
        const int ii = set_weights<ORDER>((x[u][0] - geo.off[0]) * geo.scale, wx) - g;
        const int jj = set_weights<ORDER>((x[u][1] - geo.off[1]) * geo.scale, wy) - g;
        const int kk = set_weights<ORDER>((x[u][2] - geo.off[2]) * geo.scale, wz) - g;
        // the ORDER^3 terms, each added at(i, j, k): to the box in LDS or to the mesh
        auto deposit = [&](auto at) {
#pragma unroll
            for (int i = 0; i < ORDER; i++) {
                double weight_i = wx[i];
                weight_i *= contribution;  // apply_factor = True
#pragma unroll
                for (int j = 0; j < ORDER; j++) {
                    const double wij = weight_i * wy[j];
#pragma unroll
                    for (int k = 0; k < ORDER; k++)
                        unsafeAtomicAdd(at(i, j, k), ORDER == 1 ? weight_i : wij * wz[k]);
                }
            }
        };
        // Up to CIC the two are separate branches (ds_add_f64 and global atomics); TSC and PCS
        // choose per address (flat atomics).  Measured, 2^27 tile-sorted particles at 256^3:
        // CIC 1.31 ms per address, 1.22 in branches; PCS 8.06 ms per address, 8.35 in branches.
        double *q = blk + B.entry_of(cell[u], N);
        auto on_mesh = [&](int i, int j, int k) {
            return mesh + (cg_xlayer(xm, (i64)(ii + i), N) * ny + wrap(jj + j, N)) * pad +
                   wrap(kk + k, N);
        };
        auto in_box = [&](int i, int j, int k) { return q + (i * B.e[1] + j) * B.e[2] + k; };
        if (ORDER <= 2 && B.fits) deposit(in_box);
        else if (ORDER <= 2) deposit(on_mesh);
        else
            deposit([&](int i, int j, int k) {
                return B.fits ? in_box(i, j, k) : on_mesh(i, j, k);
            });
    }
    chunk_flush(B, blk, mesh, N, ny, pad, xm);
}

template <int ORDER>
__global__ __launch_bounds__(kChunkLanes) void k_gather_scalar(const double *__restrict__ pos,
                                                               double *__restrict__ mom, i64 n,
                                                               int dim,
                                                               const double *__restrict__ mesh,
                                                               int N, i64 ny, i64 pad, int g,
                                                               XMap xm, CicGeom geo,
                                                               double factor) {
#pragma clang fp contract(off)
    __shared__ double blk[kChunkCells];
    double x[kChunkPer][3];
    int cell[kChunkPer][3];
    chunk_load<ORDER>(pos, n, geo, g, N, x, cell);
    const ChunkBox<ORDER> B = chunk_box<ORDER>(cell, n, N);
    chunk_fill(B, blk, mesh, N, ny, pad, xm);
#pragma unroll 1
    for (int u = 0; u < kChunkPer; u++) {
        const i64 p = chunk_particle(u);
        if (p >= n) continue;
        double wx[4], wy[4], wz[4];
        const int ii = set_weights<ORDER>((x[u][0] - geo.off[0]) * geo.scale, wx) - g;
        const int jj = set_weights<ORDER>((x[u][1] - geo.off[1]) * geo.scale, wy) - g;
        const int kk = set_weights<ORDER>((x[u][2] - geo.off[2]) * geo.scale, wz) - g;
        const double *q = blk + B.entry_of(cell[u], N);
        double value = 0;
#pragma unroll
        for (int i = 0; i < ORDER; i++) {
            const i64 ri = B.fits ? 0 : cg_xlayer(xm, (i64)(ii + i), N) * ny;
#pragma unroll
            for (int j = 0; j < ORDER; j++) {
                const double wij = wx[i] * wy[j];
                const double *row = B.fits ? q + (i * B.e[1] + j) * B.e[2]
                                           : mesh + (ri + wrap(jj + j, N)) * pad;
#pragma unroll
                for (int k = 0; k < ORDER; k++)
                    value += row[B.fits ? k : wrap(kk + k, N)] * (ORDER == 1 ? 1.0 : wij * wz[k]);
            }
        }
        if (factor != 1) value *= factor;  // mesh.py:456-458
        mom[3 * p + dim] += value;
    }
}

// diff_domaingrid (mesh.py:4874-5030) of the real-space mesh of `src` into `dst`
template <int ORDER>
__global__ __launch_bounds__(256) void k_mesh_diff(double *__restrict__ dst,
                                                   const double *__restrict__ src, int N,
                                                   XMap xm, i64 ny, i64 pad, int dim, FdCoef fc) {
#pragma clang fp contract(off)
    // both are local buffers (ghost layers included); the owned layers of dst are written
    const i64 total = (i64)xm.nxl * N * N;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (i64)gridDim.x * blockDim.x) {
        i64 row = t / N;
        int k = (int)(t - row * N);
        int i = (int)(row / N), j = (int)(row - (i64)i * N);
        auto phi = [&](int s) {
            i64 ii = cg_xlayer(xm, xm.x0 + i + (dim == 0 ? s : 0), N);
            int jj = j, kk = k;
            if (dim == 1) jj = wrap(j + s, N);
            else if (dim == 2) kk = wrap(k + s, N);
            return src[(ii * ny + jj) * pad + kk];
        };
        const double gval = fd_value<ORDER>(phi, fc);
        dst[(((i64)i + xm.G) * ny + j) * pad + k] = gval;
    }
}

static unsigned blocks_for(i64 n, int per) {
    i64 b = (n + per - 1) / per;
    if (b > 256 * 64) b = 256 * 64;
    if (b < 1) b = 1;
    return (unsigned)b;
}

int cgk_fluid_add(cg_ctx *c, const double *fluid, double factor, int op_add) {
    i64 total = c->xmap.nxl * c->N * c->N;
    hipLaunchKernelGGL(k_fluid_add, dim3(blocks_for(total, 256)), dim3(256), 0, c->stream,
                       c->mesh0, fluid, (int)c->N, (int)c->xmap.nxl, c->ny, c->pad, factor, op_add);
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_nullify_nyquist(cg_ctx *c) {
    hipLaunchKernelGGL(k_nullify_nyquist, dim3(blocks_for(c->N * c->f_nj, 1)), dim3(64), 0,
                       c->stream, c->four, (int)c->N, c->f_si, c->pad / 2, c->f_j0, c->f_nj);
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_fourier_operate(cg_ctx *onto, cg_ctx *from, int deconv_order, int nlattice,
                        const double *shift, int diff_dim, int op_add) {
    const double kPiLocal = 3.141592653589793;
    FourierOp P{};
    P.tab_n = onto->ktab_n;
    P.tab_s = onto->ktab_s;
    P.deconv_order = deconv_order;
    P.nlattice = nlattice;
    P.diff_dim = diff_dim;
    P.op_add = op_add;
    P.shifted = shift && (shift[0] != 0 || shift[1] != 0 || shift[2] != 0);
    P.zero_nyquist = (from != onto) && !op_add;
    if (P.shifted) {
        // ℝ[-2*π/gridsize_corrections*interlace_lattice.shift[d]]  (mesh.py:2863-2878)
        P.A = -2 * kPiLocal / (double)onto->N * shift[0];
        P.B = -2 * kPiLocal / (double)onto->N * shift[1];
        P.Cc = -2 * kPiLocal / (double)onto->N * shift[2];
    }
    P.k_fundamental = 2 * kPiLocal / onto->p.boxsize;  // mesh.py:3362
    P.inv_lat = 1.0 / (double)nlattice;
    hipLaunchKernelGGL(k_fourier_operate, dim3(blocks_for(onto->N * onto->f_nj, 1)), dim3(256), 0,
                       onto->stream, (const double2 *)from->four, onto->four, (int)onto->N,
                       onto->f_si, onto->pad / 2, onto->f_j0, onto->f_nj, P);
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_copy_modes(cg_ctx *onto, cg_ctx *from, int deconv_order, int nlattice,
                   const double *shift, int op_add) {
    CopyModes P = copy_modes_params(onto, from, deconv_order, nlattice, shift, op_add);
    i64 ns = onto->N < from->N ? onto->N : from->N;
    hipLaunchKernelGGL(k_copy_modes, dim3(blocks_for(ns * ns, 1)), dim3(64), 0, onto->stream,
                       (const double2 *)from->mesh0, (int)from->N, from->ny, from->pad / 2,
                       (double2 *)onto->mesh0, (int)onto->N, onto->ny, onto->pad / 2, P);
    CG_LAUNCH_CHECK();
    return 0;
}

static CopyModes copy_modes_params(cg_ctx *onto, cg_ctx *from, int deconv_order, int nlattice,
                                    const double *shift, int op_add) {
    const double kPiLocal = 3.141592653589793;
    CopyModes P{};
    P.tab_n = from->ktab_n;  // kk*pi/N_from + eps by array index of the `from` grid
    P.tab_s = from->ktab_s;
    P.deconv_order = deconv_order;
    P.op_add = op_add;
    P.shifted = shift && (shift[0] != 0 || shift[1] != 0 || shift[2] != 0);
    if (P.shifted) {
        P.A = -2 * kPiLocal / (double)from->N * shift[0];
        P.B = -2 * kPiLocal / (double)from->N * shift[1];
        P.Cc = -2 * kPiLocal / (double)from->N * shift[2];
    }
    P.dtheta = kPiLocal / (double)onto->N - kPiLocal / (double)from->N;
    P.inv_lat = 1.0 / (double)nlattice;
    return P;
}

int cgk_copy_modes_pack(cg_ctx *from, i64 n_small, const int *rows_local, i64 n_rows,
                        double *out) {
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(k_cm_pack, dim3(blocks_for(n_rows * n_small, 1)), dim3(64), 0, from->stream,
                       (const double2 *)from->four, (int)from->N, from->f_si, from->pad / 2,
                       rows_local, n_rows, (int)n_small, (double2 *)out);
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_copy_modes_unpack(cg_ctx *onto, cg_ctx *from, i64 n_small, const int *rows_local,
                          i64 n_rows, const double *in, int deconv_order, int nlattice,
                          const double *shift, int op_add) {
    if (n_rows == 0) return 0;
    CopyModes P = copy_modes_params(onto, from, deconv_order, nlattice, shift, op_add);
    hipLaunchKernelGGL(k_cm_unpack, dim3(blocks_for(n_rows * n_small, 1)), dim3(64), 0,
                       onto->stream, (const double2 *)in, (int)n_small, rows_local, n_rows,
                       onto->four, (int)onto->N, onto->f_si, onto->pad / 2, onto->f_j0,
                       (int)from->N, P);
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_fluid_kick(cg_ctx *c, double *J, const double *rho, const double *P, int dim,
                   int diff_order, double minus_dt, double inv_c2) {
    i64 total = c->xmap.nxl * c->N * c->N;
    double dx = c->p.boxsize / (double)c->N;  // interactions.py:2133
    FdCoef fc;
    if (!fd_coefficients(diff_order, dx, fc)) {
        cg_set_error("cg_fluid_kick: differentiation order %d", diff_order);
        return 1;
    }
    CG_FD_SWITCH(diff_order, k_fluid_kick, dim3(blocks_for(total, 256)), dim3(256), 0, c->stream,
                 J, rho, P, c->mesh, (int)c->N, c->xmap, c->ny, c->pad, dim, fc, minus_dt, inv_c2)
    CG_LAUNCH_CHECK();
    return 0;
}

#define CG_ORDER_SWITCH(order, KERNEL, ...)                                       \
    switch (order) {                                                              \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                \
        case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                \
        default: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;               \
    }

int cgk_deposit_general(cg_ctx *c, const double *pos, i64 n, double contribution, int order,
                        const CicGeom &geo) {
    if (n == 0) return 0;
    CG_ORDER_SWITCH(order, k_deposit_general, dim3(chunk_blocks(n)), dim3(kChunkLanes), 0,
                    c->stream, pos, n, c->mesh, (int)c->N, c->ny, c->pad, c->p.nghosts, c->xmap,
                    geo, contribution)
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_gather_scalar(cg_ctx *c, const double *pos, double *mom, i64 n, int dim, int order,
                      const CicGeom &geo, double factor) {
    if (n == 0) return 0;
    CG_ORDER_SWITCH(order, k_gather_scalar, dim3(chunk_blocks(n)), dim3(kChunkLanes), 0,
                    c->stream, pos, mom, n, dim, c->mesh, (int)c->N, c->ny, c->pad, c->p.nghosts,
                    c->xmap, geo, factor)
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_mesh_diff(cg_ctx *dst, cg_ctx *src, int dim, int diff_order) {
    i64 total = src->xmap.nxl * src->N * src->N;
    double dx = src->p.boxsize / (double)src->N;
    FdCoef fc;
    if (diff_order == 0 || !fd_coefficients(diff_order, dx, fc)) {
        cg_set_error("cg_mesh_diff: differentiation order %d", diff_order);
        return 1;
    }
    CG_FD_SWITCH(diff_order, k_mesh_diff, dim3(blocks_for(total, 256)), dim3(256), 0, dst->stream,
                 dst->mesh, src->mesh, (int)src->N, src->xmap, src->ny, src->pad, dim, fc)
    CG_LAUNCH_CHECK();
    return 0;
}
