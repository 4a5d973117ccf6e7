// cg_chunk_box.h — what the particle-mesh kernels share: the per-axis cell index and weights of
// every assignment order, the finite differences of diff_domaingrid, and the chunk box of the
// kernels that take particles in ANY memory order (k_deposit_general, k_gather_scalar in
// cg_general.hip; k_gather_kick_chunks in cg_mesh_kernels.hip).
//
// The chunk box.  Device-scope FP64 atomics execute memory-side on MI355X (a CIC deposit by
// direct atomics, 8 per particle: 31.7 ms for 2^27 particles), and a gather straight from the
// mesh reads 48 scattered values per particle with second-order differences.  Particles that are
// compact in space but not in THIS mesh's tile order (BASELINE configs[4]: 512^3 particles sorted
// by the tiles of their own 1024^3 P3M mesh, deposited onto and kicked from the 256^3 mesh of the
// (fluid <- particles, fluid) interaction, interactions.py:1985-2335, param/example_nonlinnu:36-45;
// tile-sorted particles under the power spectrum's, bispectrum's and renders' meshes) need
// neither.  So:
//   - a 512-lane workgroup takes 2048 consecutive particles, 4 per lane;
//   - it finds the box of the first cells of their stencils relative to the first particle's,
//     through the periodic seam (relative cells lie in [-N/2, N/2): the seam is no seam);
//   - when the box, with the stencil's width added, fits 4096 cells of LDS and no axis is longer
//     than the mesh, the workgroup works in LDS and touches the mesh once per cell: a deposit
//     accumulates there (ds_add_f64) and adds the non-zero entries to the mesh with one device
//     atomic each instead of ORDER^3 per particle; a gather copies the box of the field in first
//     (fused gather-kick: 5.5 -> 2.x ms for 2^27 particles);
//   - a chunk that is spread out (unsorted particles) takes the direct accesses.
// The stencil is W cells wide per axis and starts H cells below the particle's cell: W = ORDER,
// H = 0 for interpolation alone, W = 2 + 2*H with H = diff_order/2 for the fused gather-kick (CIC
// plus the reach of the finite difference).  Index and weight arithmetic are the reference's on
// both paths; only the order in which particles are added to a cell differs.
//
// The integer arithmetic (wrap, chunk_rel, ChunkBox) and the difference coefficients compile with
// a host compiler alone (tests/chunk_box_print.cpp); everything below `#ifdef __HIPCC__` is
// device code.
#pragma once

#ifdef __HIPCC__
#define CG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CG_HD inline
#endif

// periodic wrap of a in [-n, 2n)
CG_HD int wrap(int a, int n) {
    a = a < 0 ? a + n : a;
    return a >= n ? a - n : a;
}

// ---------------------------------------------------------------------------
// The chunk: 4 particles per lane, 512 lanes, 4096 cells of LDS
// ---------------------------------------------------------------------------
constexpr int kChunkPer = 4, kChunkLanes = 512, kChunkCells = 4096;
constexpr int kChunk = kChunkPer * kChunkLanes;

// cell relative to ref (both in [0, N)) through the periodic seam: in [-N/2, N/2)
CG_HD int chunk_rel(int cell, int ref, int N) {
    int d = cell - ref;
    d += d < -(N / 2) ? N : 0;
    d -= d >= N - N / 2 ? N : 0;
    return d;
}

// The box of a chunk whose stencils are W cells wide and start H below the particle's cell.
// Entry i = (a*e[1] + b)*e[2] + c is the cell (r + l + (a, b, c)) mod N of the mesh.
template <int W, int H = 0>
struct ChunkBox {
    int r[3];  // the first particle's cell, in [0, N)
    int l[3];  // the box's lowest cell relative to r
    int e[3];  // cells per axis
    bool fits;

    // from ref and the extremes lo <= 0 <= hi of the particles' cells relative to it
    CG_HD void set(const int (&ref)[3], const int (&lo)[3], const int (&hi)[3], int N) {
        for (int d = 0; d < 3; d++) {
            r[d] = ref[d];
            l[d] = lo[d] - H;
            e[d] = hi[d] - lo[d] + W;
        }
        fits = (long long)e[0] * e[1] * e[2] <= kChunkCells && e[0] <= N && e[1] <= N && e[2] <= N;
    }
    CG_HD int ncells() const { return fits ? e[0] * e[1] * e[2] : 0; }
    // entry -> cell of the mesh (r + l + entry is in [-N, 2N): |rel| <= N/2, H <= N/2, e <= N)
    CG_HD void cell_of(int i, int N, int (&cell)[3]) const {
        cell[0] = wrap(r[0] + l[0] + i / (e[2] * e[1]), N);
        cell[1] = wrap(r[1] + l[1] + (i / e[2]) % e[1], N);
        cell[2] = wrap(r[2] + l[2] + i % e[2], N);
    }
    // the entry of the first stencil cell of a particle in `cell` (in [0, N), inside the box)
    CG_HD int entry_of(const int (&cell)[3], int N) const {
        return ((chunk_rel(cell[0], r[0], N) - H - l[0]) * e[1] +
                (chunk_rel(cell[1], r[1], N) - H - l[1])) * e[2] +
               (chunk_rel(cell[2], r[2], N) - H - l[2]);
    }
};

// ---------------------------------------------------------------------------
// diff_domaingrid (mesh.py:4874-5030): coefficients of the differences of order 0 (none), 1, 2,
// 4, 6, 8 on cells of size dx
// ---------------------------------------------------------------------------
struct FdCoef {
    double c1, c2, c3, c4;
};
inline bool fd_coefficients(int order, double dx, FdCoef &c) {
    c = FdCoef{0, 0, 0, 0};
    switch (order) {
        case 0: return true;
        case 1: c.c1 = 1 / dx; return true;
        case 2: c.c1 = (1.0 / 2) / dx; return true;
        case 4: c.c1 = (2.0 / 3) / dx; c.c2 = (1.0 / 12) / dx; return true;
        case 6: c.c1 = (3.0 / 4) / dx; c.c2 = (3.0 / 20) / dx; c.c3 = (1.0 / 60) / dx; return true;
        case 8:
            c.c1 = (4.0 / 5) / dx; c.c2 = (1.0 / 5) / dx; c.c3 = (4.0 / 105) / dx;
            c.c4 = (1.0 / 280) / dx;
            return true;
    }
    return false;
}

#ifdef __HIPCC__
#include "cg_wave.h"

// The value of one force cell from the potential along one dimension, P(s) = the potential s
// cells away.  Coefficients and the order of the terms are the reference's; order 1 is its
// one-sided 'forward' difference.
template <int ORDER, class P>
__device__ __forceinline__ double fd_value(const P &phi, const FdCoef &c) {
#pragma clang fp contract(off)
    if (ORDER == 0) return phi(0);  // the mesh already holds the force (Fourier-space gradient)
    if (ORDER == 1) return c.c1 * (phi(1) - phi(0));                                // mesh.py:4962
    if (ORDER == 2) return c.c1 * (phi(1) - phi(-1));                               // mesh.py:4967
    if (ORDER == 4) return c.c1 * (phi(1) - phi(-1)) - c.c2 * (phi(2) - phi(-2));   // mesh.py:4973
    if (ORDER == 6)                                                                  // mesh.py:4984
        return (c.c1 * (phi(1) - phi(-1)) - c.c2 * (phi(2) - phi(-2))) + c.c3 * (phi(3) - phi(-3));
    return ((c.c1 * (phi(1) - phi(-1)) - c.c2 * (phi(2) - phi(-2))) +                // mesh.py:4999
            c.c3 * (phi(3) - phi(-3))) - c.c4 * (phi(4) - phi(-4));
}

// ---------------------------------------------------------------------------
// Cell index and weights along one axis: set_weights_NGP / CIC / TSC / PCS (mesh.py:5305-5394)
// of the grid coordinate x = (pos - off)*scale, the coordinate map of interpolate_particles
// (mesh.py:1577-1606) or interpolate_domaingrid_to_particles (mesh.py:409-432) in CicGeom.
//
// 32-bit cell arithmetic: x is positive and < gridsize + 2*nghosts + 1 (positions are in
// [0, boxsize)), so the reference's truncation to Py_ssize_t equals truncation to int —
// one v_cvt_i32_f64 instead of the ~15-instruction double -> int64 sequence, and every
// index below (N <= 2048 and change) stays in 32-bit registers.
// ---------------------------------------------------------------------------
struct Cic1 {
    int index;
    double w0, w1;
};
__device__ __forceinline__ Cic1 cic1(double pos, double off, double scale) {
    double x = (pos - off) * scale;
    Cic1 r;
    r.index = (int)x;
    double dist = x - (double)r.index;
    r.w0 = 1 - dist;
    r.w1 = dist;
    return r;
}
// every order: -> the (ghosted) index of the stencil's first cell, its ORDER weights in w
template <int ORDER>
__device__ __forceinline__ int set_weights(double x, double (&w)[4]) {
#pragma clang fp contract(off)
    if (ORDER == 1) {
        int index = (int)(x + 0.5);
        w[0] = 1;
        return index;
    }
    if (ORDER == 2) {
        int index = (int)x;
        double dist = x - (double)index;
        w[0] = 1 - dist;
        w[1] = dist;
        return index;
    }
    if (ORDER == 3) {
        int index = (int)(x + 0.5);
        double dist = x - (double)index;
        index -= 1;
        double dist2 = dist * dist;
        double weight0 = 0.125 + 0.5 * (dist2 - dist);
        double weight1 = 0.75 - dist2;
        w[0] = weight0;
        w[1] = weight1;
        w[2] = 1 - weight0 - weight1;
        return index;
    }
    int index = (int)x;
    index -= 1;
    double dist = x - (double)index;
    double tmp = 2 - dist;
    double tmp2 = tmp * tmp;
    double tmp3 = tmp * tmp2;
    double weight0 = 1. / 6. * tmp3;
    double weight2 = 2. / 3. - tmp2 + 0.5 * tmp3;
    double d1 = dist - 1;
    double weight3 = 1. / 6. * (d1 * d1 * d1);
    w[0] = weight0;
    w[1] = 1 - weight0 - weight2 - weight3;
    w[2] = weight2;
    w[3] = weight3;
    return index;
}

// ---------------------------------------------------------------------------
// The chunk on the device.  All of these are called by every lane of the workgroup.
// ---------------------------------------------------------------------------
// particle u of this lane (a row of pos; beyond n on the last chunk's tail)
__device__ __forceinline__ i64 chunk_particle(int u) {
    return (i64)blockIdx.x * kChunk + threadIdx.x + (i64)kChunkLanes * u;
}
inline unsigned chunk_blocks(i64 n) { return (unsigned)((n + kChunk - 1) / kChunk); }

// the lane's particles: positions x, and the first cells of their order-ORDER stencils on the
// mesh (two plain arrays: the kernels index them with a loop counter, and only plain arrays stay
// in registers then)
template <int ORDER>
__device__ __forceinline__ void chunk_load(const double *__restrict__ pos, i64 n,
                                           const CicGeom &geo, int g, int N,
                                           double (&x)[kChunkPer][3], int (&cell)[kChunkPer][3]) {
#pragma unroll
    for (int u = 0; u < kChunkPer; u++) {
        const i64 p = chunk_particle(u);
        double w[4];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            x[u][d] = p < n ? pos[3 * p + d] : 0.0;
            cell[u][d] = wrap(set_weights<ORDER>((x[u][d] - geo.off[d]) * geo.scale, w) - g, N);
        }
    }
}

// the chunk's box (the chunk's first particle exists: its workgroup was launched for it)
template <int W, int H = 0>
__device__ __forceinline__ ChunkBox<W, H> chunk_box(const int (&cell)[kChunkPer][3], i64 n, int N) {
    __shared__ int s_ref[3], s_lo[3], s_hi[3];
    const int tid = threadIdx.x;
    if (tid == 0) {
        for (int d = 0; d < 3; d++) {
            s_ref[d] = cell[0][d];
            s_lo[d] = 0;
            s_hi[d] = 0;
        }
    }
    __syncthreads();
    const int ref[3] = {s_ref[0], s_ref[1], s_ref[2]};
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
#pragma unroll
    for (int u = 0; u < kChunkPer; u++) {
        if (chunk_particle(u) >= n) continue;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const int v = chunk_rel(cell[u][d], ref[d], N);
            lo[d] = min(lo[d], v);
            hi[d] = max(hi[d], v);
        }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
        lo[d] = wave_min_xor(lo[d]);
        hi[d] = wave_max_xor(hi[d]);
        if ((tid & 63) == 0) {
            atomicMin(&s_lo[d], lo[d]);
            atomicMax(&s_hi[d], hi[d]);
        }
    }
    __syncthreads();
    const int blo[3] = {s_lo[0], s_lo[1], s_lo[2]}, bhi[3] = {s_hi[0], s_hi[1], s_hi[2]};
    ChunkBox<W, H> B;
    B.set(ref, blo, bhi, N);
    return B;
}

// where the mesh holds entry i of the box
template <class Box>
__device__ __forceinline__ i64 chunk_mesh_index(const Box &B, int i, int N, i64 ny, i64 pad,
                                                const XMap &xm) {
    int cell[3];
    B.cell_of(i, N, cell);
    return (cg_xlayer(xm, cell[0], N) * ny + cell[1]) * pad + cell[2];
}

// The three loops over the box (none runs when the box does not fit: ncells() is 0 then).
// zero it, for a deposit
template <class Box>
__device__ __forceinline__ void chunk_zero(const Box &B, double *blk) {
    for (int i = threadIdx.x; i < B.ncells(); i += kChunkLanes) blk[i] = 0;
    __syncthreads();
}
// fill it from the mesh, for a gather
template <class Box>
__device__ __forceinline__ void chunk_fill(const Box &B, double *blk,
                                           const double *__restrict__ mesh, int N, i64 ny, i64 pad,
                                           const XMap &xm) {
    for (int i = threadIdx.x; i < B.ncells(); i += kChunkLanes)
        blk[i] = mesh[chunk_mesh_index(B, i, N, ny, pad, xm)];
    __syncthreads();
}
// add its non-zero entries to the mesh, one device atomic each
template <class Box>
__device__ __forceinline__ void chunk_flush(const Box &B, const double *blk,
                                            double *__restrict__ mesh, int N, i64 ny, i64 pad,
                                            const XMap &xm) {
    if (!B.fits) return;  // (uniform)
    __syncthreads();
    for (int i = threadIdx.x; i < B.ncells(); i += kChunkLanes) {
        const double v = blk[i];
        if (v == 0) continue;
        unsafeAtomicAdd(mesh + chunk_mesh_index(B, i, N, ny, pad, xm), v);
    }
}
#endif  // __HIPCC__
