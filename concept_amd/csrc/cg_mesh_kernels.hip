// cg_mesh_kernels.hip — hand-written gfx950 kernels of the PM mesh path:
// k-space Poisson kernel (A5/A6), CIC gather + finite difference + kick
// (A9/A10) for particles in any order, slab helpers.  (The CIC deposit A1/A2
// for particles in any order, cg_deposit_cic, is the order-2 instantiation of
// k_deposit_general in cg_general.hip.)  FP64 throughout; compiled with
// -ffp-contract=off so every expression is evaluated in the reference's
// operation order (no FMA contraction).
#include "cg_chunk_box.h"
#include "cg_internal.h"
#include "cg_kspace.h"

// ---------------------------------------------------------------------------
// A5/A6 k-space kernel on rocFFT's natural output layout complex[i][j][kk]
// (not transposed: on one GPU the transposition FFTW-MPI produces is only a
// storage order; every mode (ki,kj,kk) gets the reference's factor).
//   nullify_modes('nyquist')  mesh.py:3591-3622 -> planes ki,kj = -N/2, kk = N/2
//   factor                    mesh.py:2775-2856, interactions.py:2096-2116
//   nullify_modes('origin')   interactions.py:2118
// One lane per complex mode (16 B load + 16 B store, coalesced along kk).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kspace(double2 *__restrict__ four, i64 N, i64 si,
                                                i64 pitch, int j0, int nj, KspaceParams P) {
    const i64 nk = N / 2 + 1;
    i64 row = blockIdx.x;  // i*nj + j_local over the Fourier view (cg_ctx::four)
    i64 i = row / nj, jl = row - i * nj;
    double2 *r = four + i * si + jl * pitch;
    for (i64 kk = threadIdx.x; kk < nk; kk += blockDim.x) {
        double factor = kspace_factor(P, N, i, j0 + jl, kk);
        double2 v = make_double2(0, 0);
        if (factor != 0) {
            v = r[kk];
            v.x *= factor;
            v.y *= factor;
        }
        r[kk] = v;
    }
}

int cgk_kspace(cg_ctx *c, int deconv_order, double C, int long_range, double E) {
    i64 rows = c->N * c->f_nj;
    int block = c->N / 2 + 1 >= 256 ? 256 : (c->N / 2 + 1 > 64 ? 128 : 64);
    hipLaunchKernelGGL(k_kspace, dim3((unsigned)rows), dim3(block), 0, c->stream, c->four, c->N,
                       c->f_si, c->pad / 2, c->f_j0, c->f_nj,
                       KspaceParams{c->ktab_n, c->ktab_s, c->ktab_q, deconv_order, long_range, C, E});
    CG_LAUNCH_CHECK();
    return 0;
}

// complex[i][j][kk] -> the reference's transposed double[j][i][N+2] (debug fetch)
__global__ void k_transpose_fourier(const double2 *__restrict__ src, double2 *__restrict__ dst,
                                    i64 N, i64 ny, i64 pitch) {
    i64 nk = N / 2 + 1;
    i64 row = blockIdx.x;
    i64 i = row / N, j = row - i * N;
    for (i64 kk = threadIdx.x; kk < nk; kk += blockDim.x)
        dst[(j * N + i) * nk + kk] = src[(i * ny + j) * pitch + kk];
}
int cgk_transpose_fourier(cg_ctx *c, const double *src, double *dst) {
    hipLaunchKernelGGL(k_transpose_fourier, dim3((unsigned)(c->N * c->N)), dim3(64), 0, c->stream,
                       (const double2 *)src, (double2 *)dst, c->N, c->ny, c->pad / 2);
    CG_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// A9/A10 gather + finite difference + kick (cg_gather_kick: particles in any order).  For each
// dim the 8 force-cell values are formed exactly as diff_domaingrid forms them
// (mesh.py:4966-4981, fd_value) and accumulated in the order of mesh.py:5142-5155 / :445, then
// value *= factor, mom += value (:456-459).  Through the chunk boxes of cg_chunk_box.h: the box
// of the potential a chunk needs is the box of its CIC cells with the difference's reach on
// both sides.
// ---------------------------------------------------------------------------
// phi(a, b, c): the potential at cell (a, b, c) of the particle's (2 + 2H)^3 cells
template <int ORDER, class Phi>
__device__ __forceinline__ void gather_force(const Phi &phi, const double (&wx)[2],
                                             const double (&wy)[2], const double (&wz)[2],
                                             const FdCoef &fc, double (&val)[3]) {
    constexpr int H = ORDER / 2;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const double wij = wx[i] * wy[j];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const double w = wij * wz[k];
                const int a = H + i, b = H + j, cc = H + k;
                const double fx = fd_value<ORDER>([&](int s) { return phi(a + s, b, cc); }, fc);
                const double fy = fd_value<ORDER>([&](int s) { return phi(a, b + s, cc); }, fc);
                const double fz = fd_value<ORDER>([&](int s) { return phi(a, b, cc + s); }, fc);
                val[0] += fx * w;
                val[1] += fy * w;
                val[2] += fz * w;
            }
        }
}

template <int ORDER>
__global__ __launch_bounds__(kChunkLanes) void k_gather_kick_chunks(
    const double *__restrict__ pos, double *__restrict__ mom, i64 n,
    const double *__restrict__ mesh, int N, i64 ny, i64 pad, int g, XMap xm, CicGeom geo,
    FdCoef fc, double factor) {
    constexpr int H = ORDER / 2;      // stencil half width
    constexpr int W = 2 + 2 * H;      // cells needed per dimension
    __shared__ double blk[kChunkCells];
    double x[kChunkPer][3];
    int cell[kChunkPer][3];
    chunk_load<2>(pos, n, geo, g, N, x, cell);
    const ChunkBox<W, H> B = chunk_box<W, H>(cell, n, N);
    chunk_fill(B, blk, mesh, N, ny, pad, xm);
#pragma unroll 1
    for (int u = 0; u < kChunkPer; u++) {
        const i64 p = chunk_particle(u);
        if (p >= n) continue;
        const Cic1 cx = cic1(x[u][0], geo.off[0], geo.scale),
                   cy = cic1(x[u][1], geo.off[1], geo.scale),
                   cz = cic1(x[u][2], geo.off[2], geo.scale);
        const double wx[2] = {cx.w0, cx.w1}, wy[2] = {cy.w0, cy.w1}, wz[2] = {cz.w0, cz.w1};
        double val[3] = {0, 0, 0};
        if (B.fits) {
            const double *q = blk + B.entry_of(cell[u], N);
            gather_force<ORDER>(
                [&](int a, int b, int c) { return q[(a * B.e[1] + b) * B.e[2] + c]; }, wx, wy, wz,
                fc, val);
        } else {
            i64 ix[W], iy[W], iz[W];
#pragma unroll
            for (int s = 0; s < W; s++) {
                ix[s] = cg_xlayer(xm, cx.index - g - H + s, N) * ny * pad;
                iy[s] = wrap(cy.index - g - H + s, N) * pad;
                iz[s] = wrap(cz.index - g - H + s, N);
            }
            gather_force<ORDER>([&](int a, int b, int c) { return mesh[ix[a] + iy[b] + iz[c]]; },
                                wx, wy, wz, fc, val);
        }
        if (factor != 1) {
            val[0] *= factor;
            val[1] *= factor;
            val[2] *= factor;
        }
        mom[3 * p + 0] += val[0];
        mom[3 * p + 1] += val[1];
        mom[3 * p + 2] += val[2];
    }
}

int cgk_gather_kick(cg_ctx *c, const double *pos, double *mom, i64 n, int diff_order,
                    double factor) {
    if (n <= 0) return 0;
    FdCoef fc;
    fd_coefficients(diff_order, c->p.boxsize / (double)c->N, fc);  // dx: interactions.py:2133
    if (diff_order == 2)
        hipLaunchKernelGGL(k_gather_kick_chunks<2>, dim3(chunk_blocks(n)), dim3(kChunkLanes), 0,
                           c->stream, pos, mom, n, c->mesh, (int)c->N, c->ny, c->pad,
                           c->p.nghosts, c->xmap, c->geom_gather, fc, factor);
    else
        hipLaunchKernelGGL(k_gather_kick_chunks<4>, dim3(chunk_blocks(n)), dim3(kChunkLanes), 0,
                           c->stream, pos, mom, n, c->mesh, (int)c->N, c->ny, c->pad,
                           c->p.nghosts, c->xmap, c->geom_gather, fc, factor);
    CG_LAUNCH_CHECK();
    return 0;
}

// CIC indices as set_weights_CIC returns them (parity tests: bit-exact bar)
__global__ void k_cic_indices(const double *__restrict__ pos, i64 n, CicGeom geo,
                              i64 *__restrict__ idx) {
    i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    for (int d = 0; d < 3; d++) idx[3 * p + d] = cic1(pos[3 * p + d], geo.off[d], geo.scale).index;
}
int cgk_cic_indices(cg_ctx *c, const double *pos, i64 n, int for_gather, i64 *idx) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_cic_indices, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       pos, n, for_gather ? c->geom_gather : c->geom_deposit, idx);
    CG_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// x-slab domains: halo layers.  A layer is a contiguous [N][pad] block, so the
// ghost exchange (communication.py:563-660) needs no packing: the host comm
// layer sends/receives whole layers; '+=' (deposit fold) is this add kernel,
// '=' (ghost fill) a plain copy.  layer0 is relative to the first owned layer.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_layers_add(double2 *__restrict__ dst,
                                                    const double2 *__restrict__ src, i64 n2) {
    i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x; v < n2; v += stride) {
        double2 a = dst[v], b = src[v];
        a.x += b.x;
        a.y += b.y;
        dst[v] = a;
    }
}
int cgk_layers_write(cg_ctx *c, i64 layer0, i64 nlayers, const double *src, int add) {
    i64 per = c->ny * c->pad;  // whole layers, the unused row included
    double *dst = c->mesh0 + layer0 * per;
    if (!add) {
        CG_HIP(hipMemcpyAsync(dst, src, 8 * per * nlayers, hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }
    i64 n2 = per * nlayers / 2;
    i64 blocks = (n2 + 255) / 256;
    hipLaunchKernelGGL(k_layers_add, dim3((unsigned)blocks), dim3(256), 0, c->stream,
                       (double2 *)dst, (const double2 *)src, n2);
    CG_LAUNCH_CHECK();
    return 0;
}

// Owner domain of each particle: the x-slab that holds its lower CIC cell
// (counterpart of which_domain(), communication.py:756-772, for slab domains).
__global__ void k_owner_rank(const double *__restrict__ pos, i64 n, CicGeom geo, int g, int N,
                             i64 nxl, int *__restrict__ owner) {
    i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    i64 a = wrap(cic1(pos[3 * p], geo.off[0], geo.scale).index - g, N);
    owner[p] = (int)(a / nxl);
}
// Destination domain of every listed emigrant (the rows cg_gather_kick_tiled_prepare found
// leaving the slab with the prepared drift) and the number going to each domain: what
// exchange() (communication.py:135-517) needs before it can size its messages.  *count is read
// on the device, so the host enqueues this right behind the gather-kick without waiting.
__global__ void k_emigrant_dest(const double *__restrict__ pos, const double *__restrict__ mom,
                                const i64 *__restrict__ idx, const unsigned *__restrict__ count,
                                i64 cap, double dtm, double L, CicGeom geo, int g, int N, i64 nxl,
                                int *__restrict__ dest, int *__restrict__ send_counts) {
    i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    i64 n = (i64)*count < cap ? (i64)*count : cap;
    if (t >= n) return;
    i64 p = idx[t];
    // the arithmetic of the fused drift (load_pos<true> in cg_particles.hip): x only
    double x = pos[3 * p] + mom[3 * p] * dtm;
    if (!(x > 0 && x < L)) {
        double m = fmod(x, L);
        if (m != 0) {
            if (m < 0) m += L;
        } else {
            m = 0.0;
        }
        if (m == L) m = 0;
        x = m;
    }
    int d = (int)((i64)wrap(cic1(x, geo.off[0], geo.scale).index - g, N) / nxl);
    dest[t] = d;
    atomicAdd(&send_counts[d], 1);
}
int cgk_emigrant_dest(cg_ctx *c, const double *pos, const double *mom, const i64 *idx,
                      const unsigned *count, i64 cap, double dtm, int *dest, int *send_counts) {
    CG_HIP(hipMemsetAsync(send_counts, 0, sizeof(int) * c->p.nprocs, c->stream));
    if (cap == 0) return 0;
    hipLaunchKernelGGL(k_emigrant_dest, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0,
                       c->stream, pos, mom, idx, count, cap, dtm, c->p.boxsize, c->geom_deposit,
                       c->p.nghosts, (int)c->N, c->xmap.nxl, dest, send_counts);
    CG_LAUNCH_CHECK();
    return 0;
}

int cgk_owner_rank(cg_ctx *c, const double *pos, i64 n, int *owner) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_owner_rank, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       pos, n, c->geom_deposit, c->p.nghosts, (int)c->N, c->xmap.nxl, owner);
    CG_LAUNCH_CHECK();
    return 0;
}
