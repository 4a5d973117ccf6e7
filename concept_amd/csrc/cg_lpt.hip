// cg_lpt.hip — the mesh and particle passes of the realisations: particles (1LPT to 3LPT, with
// Orszag dealiasing), fluids (ϱ, Jⁱ) and the shear of closure 'class'.
//   k_lpt_potential  realize_grid (scalar case)         ic.py:711-764
//                    fused with laplacian_inverse       mesh.py:3422-3437
//   k_lpt_diff       fourier_diff                       mesh.py:3466-3510
//   k_lpt_product    the grid product and the move to the output grid of handle_lpt_term
//                                                       ic.py:2020-2057
//   k_lpt_displace   displace_particles                 ic.py:2249-2280
//   k_realize_grid   realize_grid (scalar and vector)   ic.py:708-764
//   k_fluid_from_mesh  domain_decompose and the move to ϱ or Jⁱ of realize_fluid
//                                                       ic.py:418-456
//   k_realize_grid_tensor  realize_grid (rank 2, one element)     ic.py:743-762
//   k_shear_divergence     ∂ʲςⁱⱼ of the Euler equation, formed in Fourier space
//                                                       fluid.py:1011-1043, mesh.py:4966-4970
//   k_lpt_diff_enlarge       fourier_diff + resize_grid up, of diff_ifft   ic.py:2093-2101
//   k_lpt_dealias_cube       nullify_modes('beyond cube of |k| < …')       ic.py:2025
//   k_lpt_shrink_accumulate  resize_grid down + the move to the output     ic.py:2029-2057
// All of them are streaming maps: one grid-stride loop, a thread per complex mode or per pair of
// neighbouring real cells (16-byte loads and stores), no atomics, nothing wave-level, and no LDS
// but the sine table of k_shear_divergence.  A kernel is the body of one of two walks:
//   for_each_mode / write_each_mode  the modes of a Fourier view of the contexts (cg_ctx::four,
//                    the view k_fourier_operate walks), N/2 + 1 of every row, by kspace_mode
//                    (cg_kspace.h); a mode's address comes from a Slab
//   for_each_cell_pair  the N cells of the N rows of a mesh's owned layers: the row padding and the
//                    unused row of a layer are neither read nor written
// and the bodies share wave_number, derivative (fourier_diff's rounding), rotate (the lattice
// shift and the size-change phase) and accumulate ('=', '+=', '-=' with a factor).  On the host:
// launch, with_case of cg_internal.h (a template argument from a run-time integer) and the *_checks.
// Compiled with -ffp-contract=off, and every function that rounds says so itself: every product
// and sum is rounded on its own, in the reference's order.  FP64 throughout.
#include <type_traits>

#include "cg_internal.h"
#include "cg_kspace.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;  // 8 workgroups per CU, the rest by grid stride
const double kPi = 3.141592653589793;  // float(np.pi), commons.py:1816

unsigned grid_for(i64 work) {
    i64 b = (work + kThreads - 1) / kThreads;
    return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// one thread per item of `work`, up to kMaxBlocks workgroups
template <class Kernel, class... Args>
int launch(Kernel kernel, i64 work, size_t lds_bytes, hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(work)), dim3(kThreads), lds_bytes, stream, args...);
    CG_LAUNCH_CHECK();
    return 0;
}

// ---- the Fourier view and the walk over its modes

// complex[N][nj][N/2 + 1] at p, rows `cp` and slices `si` complex numbers apart
template <class T>
struct SlabOf {
    T *p;
    i64 si, cp;
    __device__ __forceinline__ T *at_index(i64 a, i64 bl, i64 kk) const {
        return p + (a * si + bl * cp + kk);
    }
    __device__ __forceinline__ T *at(KspaceMode m) const { return at_index(m.a, m.bl, m.kk); }
    // by signed wave numbers, in a (whole) grid of size n
    __device__ __forceinline__ T *at_wave(i64 ki, i64 kj, i64 kk, int n) const {
        return at_index(ki + (ki < 0 ? n : 0), kj + (kj < 0 ? n : 0), kk);
    }
};
using Slab = SlabOf<double2>;
using ConstSlab = SlabOf<const double2>;

Slab slab(const cg_ctx *c) { return Slab{c->four, c->f_si, c->pad / 2}; }
ConstSlab const_slab(const cg_ctx *c) { return ConstSlab{c->four, c->f_si, c->pad / 2}; }
i64 mode_count(i64 N, i64 nj) { return N * nj * (N / 2 + 1); }

// body(m) for every mode of the rows j0 .. j0 + nj of a grid of size N
template <class Body>
__device__ __forceinline__ void for_each_mode(int N, int j0, int nj, Body body) {
    const i64 total = (i64)N * nj * (N / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads)
        body(kspace_mode(e, N, j0, nj));
}

// dst = value(m) at every mode: each one is written exactly once
template <class Value>
__device__ __forceinline__ void write_each_mode(Slab dst, int N, int j0, int nj, Value value) {
    for_each_mode(N, j0, nj, [=](KspaceMode m) { *dst.at(m) = value(m); });
}

__device__ __forceinline__ double2 zero2() { return make_double2(0.0, 0.0); }

__device__ __forceinline__ i64 wave_number(KspaceMode m, int dim) {
    return dim == 0 ? m.ki : (dim == 1 ? m.kj : m.kk);
}

// scale * i k_dim0 z (dim1 < 0) or scale * -k_dim0 k_dim1 z: fourier_diff
__device__ __forceinline__ double2 derivative(KspaceMode m, double2 z, int dim0, int dim1,
                                              double scale) {
#pragma clang fp contract(off)
    const i64 kl0 = wave_number(m, dim0);
    if (dim1 < 0) {
        const double amplitude = scale * (double)kl0;  // mesh.py:3496
        return make_double2(amplitude * -z.y, amplitude * z.x);
    }
    const i64 kl1 = wave_number(m, dim1);
    const double amplitude = scale * (double)kl0 * (double)kl1;  // mesh.py:3506
    return make_double2(amplitude * -z.x, amplitude * -z.y);
}

// z exp(i theta): mesh.py:2873-2888 (lattice shift), mesh.py:1310-1313 (change of size)
__device__ __forceinline__ double2 rotate(double2 z, double theta) {
#pragma clang fp contract(off)
    const double c = cos(theta), s = sin(theta);
    return make_double2(z.x * c - z.y * s, z.x * s + z.y * c);
}

// *o (= | += | -=) factor * v, factor and sum rounded in turn, a factor of 1 left out
template <int kOp>
__device__ __forceinline__ void accumulate(double2 *o, double2 v, double factor) {
#pragma clang fp contract(off)
    if (factor != 1) v = make_double2(factor * v.x, factor * v.y);  // ic.py:2042-2057
    if (kOp == 0) {
        *o = v;
    } else {
        const double2 w = *o;
        *o = kOp == 1 ? make_double2(w.x + v.x, w.y + v.y) : make_double2(w.x - v.x, w.y - v.y);
    }
}

// body(offset in the mesh, offset in a dense [nrows][N] array) for every pair of neighbouring
// real cells of the nrows = layers * N rows of a mesh's owned layers (N is even)
template <class Body>
__device__ __forceinline__ void for_each_cell_pair(int N, i64 nrows, i64 ny, i64 pad, Body body) {
    const int half = N / 2;  // pairs of cells per row
    const i64 total = nrows * half;
    for (i64 t = (i64)blockIdx.x * kThreads + threadIdx.x; t < total;
         t += (i64)gridDim.x * kThreads) {
        const i64 row = t / half;
        const int p = (int)(t - row * half);
        const i64 layer = row / N;
        body((layer * ny + (row - layer * N)) * pad + 2 * p, row * N + 2 * p);
    }
}

bool same_geometry(const cg_ctx *a, const cg_ctx *b) {
    return a->N == b->N && a->pad == b->pad && a->ny == b->ny && a->xmap.nxl == b->xmap.nxl &&
           a->xmap.x0 == b->xmap.x0 && a->f_si == b->f_si && a->f_j0 == b->f_j0 &&
           a->f_nj == b->f_nj;
}

struct LptPotential {
    const double *amp;  // amplitudes by k2 (null: the modes are taken as they are)
    int shifted;
    double A, B, Cc;    // ℝ[-2*π/gridsize*shift[d]] of fourier_loop, for the negated lattice shift
    double lap;         // ℝ[-factor/k_fundamental**2]
};

// dst = (amp[k2] * rotated src) * (lap / k2) off the origin and the Nyquist planes, 0 on them
__global__ __launch_bounds__(kThreads) void k_lpt_potential(Slab dst, ConstSlab src, int N, int j0,
                                                            int nj, LptPotential P) {
    write_each_mode(dst, N, j0, nj, [=](KspaceMode m) {
#pragma clang fp contract(off)
        if (!m.live) return zero2();  // nullify_modes(['origin', 'nyquist']), ic.py:764
        double2 z = *src.at(m);
        if (P.shifted)  // mesh.py:2873-2888, ic.py:719-726
            z = rotate(z, ((double)m.ki * P.A + (double)m.kj * P.B) + (double)m.kk * P.Cc);
        if (P.amp) {  // ic.py:715, 761-762
            const double amplitude = P.amp[m.k2];
            z = make_double2(amplitude * z.x, amplitude * z.y);
        }
        const double inv = P.lap / (double)m.k2;  // mesh.py:3434-3436
        return make_double2(z.x * inv, z.y * inv);
    });
}

// dst = i k_dim0 src (dim1 < 0) or -k_dim0 k_dim1 src, times factor; 0 on the origin and the
// Nyquist planes (the nullified output slab of mesh.py:3477)
__global__ __launch_bounds__(kThreads) void k_lpt_diff(Slab dst, ConstSlab src, int N, int j0,
                                                       int nj, int dim0, int dim1, double scale) {
    write_each_mode(dst, N, j0, nj, [=](KspaceMode m) {
        return m.live ? derivative(m, *src.at(m), dim0, dim1, scale) : zero2();
    });
}

// out (= | += | -=) factor * a * b over the real cells; the three grids may be one another:
// a thread reads its pair of cells of a, b and (for '+=', '-=') out before it writes that same
// pair of out, and no other thread touches the pair, so the in-place product base *= tmp of
// handle_lpt_term (ic.py:2020-2021) is cg_lpt_product(out = a = base, b = tmp, '=')
template <int kOp>
__global__ __launch_bounds__(kThreads) void k_lpt_product(double *out, const double *a,
                                                          const double *b, int N, i64 nrows, i64 ny,
                                                          i64 pad, double factor) {
    for_each_cell_pair(N, nrows, ny, pad, [=](i64 off, i64) {
#pragma clang fp contract(off)
        const double2 x = *(const double2 *)(a + off), y = *(const double2 *)(b + off);
        const double2 v = make_double2(x.x * y.x, x.y * y.y);  // ic.py:2020-2021
        accumulate<kOp>((double2 *)(out + off), v, factor);
    });
}

// particle p = (i*N + j)*N + k of the rows from index_bgn on takes cell (i, j, k) of psi
__global__ __launch_bounds__(kThreads) void k_lpt_displace(const double *psi, int N, i64 ny,
                                                           i64 pad, double *pos, double *mom,
                                                           int dim, double pos_factor,
                                                           double mom_factor) {
    for_each_cell_pair(N, (i64)N * N, ny, pad, [=](i64 off, i64 cell) {
#pragma clang fp contract(off)
        const double2 v = *(const double2 *)(psi + off);
        const i64 r = 3 * cell + dim;
        if (pos_factor != 0) {  // ic.py:2277-2279 (1*psi is psi: no branch for a factor of 1)
            pos[r] = pos[r] + pos_factor * v.x;
            pos[r + 3] = pos[r + 3] + pos_factor * v.y;
        }
        if (mom_factor != 0) {
            mom[r] = mom[r] + mom_factor * v.x;
            mom[r + 3] = mom[r + 3] + mom_factor * v.y;
        }
    });
}

// dst = amp[k2] * src (rank 0) or (amp[k2] * ((vec * k_index0) / k2)) * i src (rank 1) off the
// origin and the Nyquist planes, 0 on them; vec = ℝ[-boxsize/(2*π)] of ic.py:741
template <int kRank>
__global__ __launch_bounds__(kThreads) void k_realize_grid(Slab dst, ConstSlab src, int N, int j0,
                                                           int nj, const double *amp, int index0,
                                                           double vec) {
    write_each_mode(dst, N, j0, nj, [=](KspaceMode m) {
#pragma clang fp contract(off)
        if (!m.live) return zero2();  // nullify_modes(['origin', 'nyquist']), ic.py:764
        const double2 z = *src.at(m);
        double amplitude = amp[m.k2];  // ic.py:715
        double re = z.x, im = z.y;
        if (kRank == 1) {  // K(k) = -i k^l/k², ic.py:732-742
            const i64 kl = wave_number(m, index0);
            amplitude = amplitude * ((vec * (double)kl) / (double)m.k2);
            re = -z.y;
            im = z.x;
        }
        return make_double2(amplitude * re, amplitude * im);  // ic.py:761-762
    });
}

// dst = (amp[k2] * K) * src off the origin and the Nyquist planes, 0 on them;
// K = 0.5 [index0 == index1] - ((1.5 k_index0) k_index1) / k2, ic.py:744-759
__global__ __launch_bounds__(kThreads) void k_realize_grid_tensor(Slab dst, ConstSlab src, int N,
                                                                  int j0, int nj,
                                                                  const double *amp, int index0,
                                                                  int index1) {
#pragma clang fp contract(off)
    const double half_delta = 0.5 * (index0 == index1);  // ℝ[0.5*(index0 == index1)]
    write_each_mode(dst, N, j0, nj, [=](KspaceMode m) {
#pragma clang fp contract(off)
        if (!m.live) return zero2();  // nullify_modes(['origin', 'nyquist']), ic.py:764
        const double2 z = *src.at(m);
        const i64 kl = wave_number(m, index0);
        const i64 km = wave_number(m, index1);
        const double amplitude =
            amp[m.k2] * (half_delta - ((1.5 * (double)kl) * (double)km) / (double)m.k2);
        return make_double2(amplitude * z.x, amplitude * z.y);  // ic.py:761-762
    });
}

// dst = (amp[k2] * S) * i src off the origin and the Nyquist planes, 0 on them;
// S = Σ_j s_j K_dim,j = 0.5 s_dim - ((1.5 k_dim) (s_0 ki + s_1 kj + s_2 kk)) / k2 with K of
// k_realize_grid_tensor and s_j = sin(2π k_j/N)/Δx, the order-2 central difference of
// diff_domaingrid (mesh.py:4966-4970) in Fourier space.  The N sines by array index are
// tabulated once per workgroup (dynamic LDS, N doubles): a mode reads three of them.
__global__ __launch_bounds__(kThreads) void k_shear_divergence(Slab dst, ConstSlab src, int N,
                                                               int j0, int nj, const double *amp,
                                                               int dim, double inv_dx) {
#pragma clang fp contract(off)
    extern __shared__ double s_sin[];
    for (int a = threadIdx.x; a < N; a += kThreads) {
        const int k = a - (a >= N / 2 ? N : 0);
        s_sin[a] = sinpi((double)(2 * k) / (double)N) * inv_dx;
    }
    __syncthreads();
    write_each_mode(dst, N, j0, nj, [=](KspaceMode m) {
#pragma clang fp contract(off)
        if (!m.live) return zero2();
        const double2 z = *src.at(m);
        const double s0 = s_sin[m.a], s1 = s_sin[j0 + m.bl], s2 = s_sin[m.kk];
        const i64 kd = wave_number(m, dim);
        const double sd = dim == 0 ? s0 : (dim == 1 ? s1 : s2);
        const double dot = (s0 * (double)m.ki + s1 * (double)m.kj) + s2 * (double)m.kk;
        const double amplitude =
            amp[m.k2] * (0.5 * sd - ((1.5 * (double)kd) * dot) / (double)m.k2);
        return make_double2(amplitude * -z.y, amplitude * z.x);
    });
}

// out[layer][j][k] (dense) from the real cells of the mesh's owned layers.
// kVar 0: c0 * (1 + v); 1: the same after v += c1 * v²; 2: v * c0; 3: out + c0 * v
template <int kVar>
__global__ __launch_bounds__(kThreads) void k_fluid_from_mesh(const double *mesh, double *out,
                                                              int N, i64 nrows, i64 ny, i64 pad,
                                                              double c0, double c1) {
    for_each_cell_pair(N, nrows, ny, pad, [=](i64 off, i64 dense) {
#pragma clang fp contract(off)
        double2 v = *(const double2 *)(mesh + off);
        if (kVar == 1)  // ic.py:436
            v = make_double2(v.x + c1 * (v.x * v.x), v.y + c1 * (v.y * v.y));
        double2 *o = (double2 *)(out + dense);
        if (kVar == 3) {  // fluid.py:1028, 1042
            const double2 w = *o;
            v = make_double2(w.x + c0 * v.x, w.y + c0 * v.y);
        } else if (kVar == 2) {
            v = make_double2(v.x * c0, v.y * c0);  // ic.py:456
        } else {
            v = make_double2(c0 * (1 + v.x), c0 * (1 + v.y));  // ic.py:437
        }
        *o = v;
    });
}

// ---- 3LPT and Orszag dealiasing: the passes between the realisation size N and the dealiasing
// size M = 3N/2 (+1 when odd).  The size-change phase of copy_modes (mesh.py:1302) is
// theta = (pi/N_onto - pi/N_from)*((ki + kj) + kk), applied on the way up and on the way down.

// `small` is the cube of |k| < n/2 of a grid of size n inside a larger one
__device__ __forceinline__ bool in_cube(KspaceMode m, int n) {
    const int h = n / 2;
    return m.ki > -h && m.ki < h && m.kj > -h && m.kj < h && m.kk < h;
}
__device__ __forceinline__ double resize_phase(KspaceMode m, double dtheta) {
#pragma clang fp contract(off)
    return dtheta * (double)((m.ki + m.kj) + m.kk);  // mesh.py:1302
}

// fourier_diff at N (k_lpt_diff's rounding) + resize_grid to M (mesh.py:916-922) in one pass over
// dst: inside the cube the rotated derivative, everywhere else (src's Nyquist planes and all of
// dst's included) zero without a read.  Every mode of dst is written exactly once.
__global__ __launch_bounds__(kThreads) void k_lpt_diff_enlarge(Slab dst, ConstSlab src, int M,
                                                               int N, int dim0, int dim1,
                                                               double scale, double dtheta) {
    write_each_mode(dst, M, 0, M, [=](KspaceMode m) {
        if (m.k2 == 0 || !in_cube(m, N)) return zero2();
        const double2 z = *src.at_wave(m.ki, m.kj, m.kk, N);
        return rotate(derivative(m, z, dim0, dim1, scale), resize_phase(m, dtheta));
    });
}

// nullify_modes(slab, 'beyond cube of |k| < n/2') (ic.py:2025): zeros outside the cube, nothing
// read, nothing written inside
__global__ __launch_bounds__(kThreads) void k_lpt_dealias_cube(Slab mesh, int M, int n) {
    for_each_mode(M, 0, M, [=](KspaceMode m) {
        if (!in_cube(m, n)) *mesh.at(m) = zero2();
    });
}

// resize_grid down to N (nullify 'nyquist', copy_modes; mesh.py:912-922) + the move to the output
// grid (ic.py:2038-2057) in one pass over out: rotation, factor and sum rounded in turn.  On
// out's Nyquist planes the shrunk grid is zero: '=' writes it, '+=' and '-=' leave out as it is.
template <int kOp>
__global__ __launch_bounds__(kThreads) void k_lpt_shrink_accumulate(Slab out, ConstSlab src, int N,
                                                                    int M, double factor,
                                                                    double dtheta) {
    const int nyq = N / 2;
    for_each_mode(N, 0, N, [=](KspaceMode m) {
        double2 *o = out.at(m);
        if (m.a == nyq || m.bl == nyq || m.kk == nyq) {
            if (kOp == 0) *o = zero2();
            return;
        }
        const double2 z = *src.at_wave(m.ki, m.kj, m.kk, M);
        accumulate<kOp>(o, rotate(z, resize_phase(m, dtheta)), factor);
    });
}

// ---- what the entry points refuse, under the entry's name

int fourier_pair_checks(const char *name, cg_ctx *dst, cg_ctx *src) {
    CG_CHECK(dst && src, "%s: null context", name);
    CG_CHECK(dst->four != nullptr && src->four != nullptr,
             "%s: no Fourier buffer bound (cg_dist_bind_fourier)", name);
    CG_CHECK(dst->N >= 2 && dst->N % 2 == 0, "%s: grid size %lld is not even", name,
             (long long)dst->N);
    CG_CHECK(same_geometry(dst, src), "%s: the two meshes differ in grid size or domain", name);
    CG_CHECK(dst->N * (i64)dst->f_nj < ((i64)1 << 31), "%s: %lld rows", name,
             (long long)(dst->N * (i64)dst->f_nj));
    return 0;
}

// a k²-indexed table of k2_max + 1 amplitudes for the grid of c
int amplitude_count_check(const char *name, const cg_ctx *c, int64_t k2_max) {
    const i64 nyq = c->N / 2;
    CG_CHECK(k2_max == 3 * (nyq - 1) * (nyq - 1),
             "%s: %lld amplitudes for grid size %lld, which needs 3*(nyquist - 1)**2 + 1 = %lld",
             name, (long long)(k2_max + 1), (long long)c->N,
             (long long)(3 * (nyq - 1) * (nyq - 1) + 1));
    return 0;
}

// two meshes of a realisation in Fourier space and its table of amplitudes
int realize_checks(const char *name, cg_ctx *out, cg_ctx *src, const double *amplitudes,
                   int64_t k2_max) {
    if (fourier_pair_checks(name, out, src)) return 1;
    CG_CHECK(amplitudes != nullptr, "%s: no amplitudes", name);
    return amplitude_count_check(name, out, k2_max);
}

// a single-domain context `large` of size M in Fourier space and a smaller size N: that of the
// context `small` of the same box, or a bare number, with `large` itself in the place of `small`:
// the tests of `small` then repeat those of `large`, and there is no second box to compare
int resize_checks(const char *name, cg_ctx *large, cg_ctx *small, i64 N) {
    CG_CHECK(large && small, "%s: null context", name);
    CG_CHECK(large->four != nullptr && small->four != nullptr,
             "%s: no Fourier buffer bound (cg_dist_bind_fourier)", name);
    CG_CHECK(large->p.nprocs == 1 && small->p.nprocs == 1, "%s: single-domain entry point", name);
    CG_CHECK(N >= 2 && N % 2 == 0 && large->N % 2 == 0,
             "%s: grid sizes %lld and %lld are not both even", name, (long long)N,
             (long long)large->N);
    CG_CHECK(large->N > N, "%s: grid size %lld is not larger than %lld", name,
             (long long)large->N, (long long)N);
    CG_CHECK(small == large || large->p.boxsize == small->p.boxsize,
             "%s: the two meshes span different boxes", name);
    CG_CHECK(large->N * large->N < ((i64)1 << 31), "%s: %lld rows", name,
             (long long)(large->N * large->N));
    return 0;
}
int resize_pair_checks(const char *name, cg_ctx *large, cg_ctx *small) {
    return resize_checks(name, large, small, small ? small->N : 0);
}
// (pi/N_onto - pi/N_from) of the size-change phase
double resize_dtheta(const cg_ctx *onto, const cg_ctx *from) {
    return kPi / (double)onto->N - kPi / (double)from->N;  // mesh.py:1302
}

// the dimensions of a derivative, and ℝ[factor*k_fundamental] or ℝ[factor*k_fundamental**2] of
// fourier_diff in the box of c
int diff_scale(const char *name, const cg_ctx *c, int dim0, int dim1, double factor,
               double *scale) {
    CG_CHECK(dim0 >= 0 && dim0 < 3 && dim1 >= -1 && dim1 < 3,
             "%s: dimensions (%d, %d) outside 0..2 (the second may be -1)", name, dim0, dim1);
    const double k_fundamental = 2 * kPi / c->p.boxsize;
    *scale = dim1 < 0 ? factor * k_fundamental : factor * (k_fundamental * k_fundamental);
    return 0;
}

// both entries of k_fluid_from_mesh: kVar = var, none (-1) where the caller's `mode` names none
int fluid_from_mesh(const char *name, cg_ctx *mesh, double *out, int var, int mode, double c0,
                    double c1) {
    CG_CHECK(mesh && out, "%s: null %s", name, mesh ? "output grid" : "context");
    CG_CHECK(var >= 0, "%s: mode %d not in {0 ϱ, 1 J}", name, mode);
    CG_CHECK(mesh->N >= 2 && mesh->N % 2 == 0, "%s: grid size %lld is not even", name,
             (long long)mesh->N);
    CG_CHECK((uintptr_t)out % 16 == 0, "%s: the output grid is not 16-byte aligned", name);
    const i64 nrows = mesh->xmap.nxl * mesh->N;
    return with_case<4>(var, [=](auto k) {
        return launch(k_fluid_from_mesh<decltype(k)::value>, nrows * (mesh->N / 2), 0,
                      mesh->stream, (const double *)mesh->mesh0, out, (int)mesh->N, nrows,
                      mesh->ny, mesh->pad, c0, c1);
    });
}

}  // namespace

extern "C" int cg_lpt_potential(cg_ctx *dst, cg_ctx *noise_src, const double *amplitudes,
                                int64_t k2_max, const double *shift, double factor) {
    if (fourier_pair_checks("cg_lpt_potential", dst, noise_src)) return 1;
    if (amplitudes && amplitude_count_check("cg_lpt_potential", dst, k2_max)) return 1;
    LptPotential P{};
    P.amp = amplitudes;
    P.shifted = shift && (shift[0] != 0 || shift[1] != 0 || shift[2] != 0);
    if (P.shifted) {
        // the positions have been shifted by +shift, fourier_loop assumes -shift (ic.py:692-695)
        P.A = -2 * kPi / (double)dst->N * -shift[0];
        P.B = -2 * kPi / (double)dst->N * -shift[1];
        P.Cc = -2 * kPi / (double)dst->N * -shift[2];
    }
    const double k_fundamental = 2 * kPi / dst->p.boxsize;
    P.lap = -factor / (k_fundamental * k_fundamental);
    return launch(k_lpt_potential, mode_count(dst->N, dst->f_nj), 0, dst->stream, slab(dst),
                  const_slab(noise_src), (int)dst->N, dst->f_j0, dst->f_nj, P);
}

extern "C" int cg_lpt_diff(cg_ctx *dst, cg_ctx *src, int dim0, int dim1, double factor) {
    double scale;
    if (fourier_pair_checks("cg_lpt_diff", dst, src)) return 1;
    if (diff_scale("cg_lpt_diff", dst, dim0, dim1, factor, &scale)) return 1;
    // the first derivative with factor 1 into another mesh is fourier_operate(diff_dim) to the bit
    if (dim1 < 0 && factor == 1 && dst != src)
        return cgk_fourier_operate(dst, src, 0, 1, nullptr, dim0, 0);
    return launch(k_lpt_diff, mode_count(dst->N, dst->f_nj), 0, dst->stream, slab(dst),
                  const_slab(src), (int)dst->N, dst->f_j0, dst->f_nj, dim0, dim1, scale);
}

extern "C" int cg_lpt_product(cg_ctx *out, cg_ctx *a, cg_ctx *b, int op, double factor) {
    CG_CHECK(out && a && b, "cg_lpt_product: null context");
    CG_CHECK(op >= 0 && op <= 2, "cg_lpt_product: operation %d not in {0 '=', 1 '+=', 2 '-='}", op);
    CG_CHECK(out->N >= 2 && out->N % 2 == 0, "cg_lpt_product: grid size %lld is not even",
             (long long)out->N);
    CG_CHECK(same_geometry(out, a) && same_geometry(out, b),
             "cg_lpt_product: the meshes differ in grid size or domain");
    const i64 nrows = out->xmap.nxl * out->N;
    return with_case<3>(op, [=](auto k) {
        return launch(k_lpt_product<decltype(k)::value>, nrows * (out->N / 2), 0, out->stream,
                      out->mesh0, (const double *)a->mesh0, (const double *)b->mesh0, (int)out->N,
                      nrows, out->ny, out->pad, factor);
    });
}

extern "C" int cg_lpt_diff_enlarge(cg_ctx *dst, cg_ctx *src, int dim0, int dim1, double factor) {
    double scale;
    if (resize_pair_checks("cg_lpt_diff_enlarge", dst, src)) return 1;
    if (diff_scale("cg_lpt_diff_enlarge", src, dim0, dim1, factor, &scale)) return 1;
    return launch(k_lpt_diff_enlarge, mode_count(dst->N, dst->N), 0, dst->stream, slab(dst),
                  const_slab(src), (int)dst->N, (int)src->N, dim0, dim1, scale,
                  resize_dtheta(dst, src));
}

extern "C" int cg_lpt_dealias_cube(cg_ctx *mesh, int64_t n_small) {
    if (resize_checks("cg_lpt_dealias_cube", mesh, mesh, n_small)) return 1;
    return launch(k_lpt_dealias_cube, mode_count(mesh->N, mesh->N), 0, mesh->stream, slab(mesh),
                  (int)mesh->N, (int)n_small);
}

extern "C" int cg_lpt_shrink_accumulate(cg_ctx *out, cg_ctx *src, int op, double factor) {
    if (resize_pair_checks("cg_lpt_shrink_accumulate", src, out)) return 1;
    CG_CHECK(op >= 0 && op <= 2,
             "cg_lpt_shrink_accumulate: operation %d not in {0 '=', 1 '+=', 2 '-='}", op);
    return with_case<3>(op, [=](auto k) {
        return launch(k_lpt_shrink_accumulate<decltype(k)::value>, mode_count(out->N, out->N), 0,
                      out->stream, slab(out), const_slab(src), (int)out->N, (int)src->N, factor,
                      resize_dtheta(out, src));
    });
}

extern "C" int cg_lpt_displace(cg_ctx *psi, double *pos, double *mom, int64_t n,
                               int64_t index_bgn, int dim, double pos_factor, double mom_factor) {
    CG_WRITES_PARTICLES(psi);
    CG_CHECK(psi, "cg_lpt_displace: null context");
    CG_CHECK(dim >= 0 && dim < 3, "cg_lpt_displace: dim = %d not in {0, 1, 2}", dim);
    if (n == 0) return 0;
    CG_CHECK(psi->p.nprocs == 1, "cg_lpt_displace: single-domain entry point");
    CG_CHECK(psi->N % 2 == 0 && n == psi->N * psi->N * psi->N,
             "cg_lpt_displace: %lld particles for a lattice of %lld**3 cells", (long long)n,
             (long long)psi->N);
    CG_CHECK(index_bgn >= 0, "cg_lpt_displace: index_bgn = %lld < 0", (long long)index_bgn);
    CG_CHECK((pos || pos_factor == 0) && (mom || mom_factor == 0),
             "cg_lpt_displace: null particle array with a non-zero factor");
    if (pos_factor == 0 && mom_factor == 0) return 0;
    return launch(k_lpt_displace, n / 2, 0, psi->stream, (const double *)psi->mesh0, (int)psi->N,
                  psi->ny, psi->pad, pos ? pos + 3 * index_bgn : nullptr,
                  mom ? mom + 3 * index_bgn : nullptr, dim, pos_factor, mom_factor);
}

extern "C" int cg_realize_grid(cg_ctx *out, cg_ctx *noise, const double *amplitudes, int64_t k2_max,
                               int tensor_rank, int index0) {
    if (realize_checks("cg_realize_grid", out, noise, amplitudes, k2_max)) return 1;
    CG_CHECK(tensor_rank == 0 || tensor_rank == 1,
             "cg_realize_grid: tensor rank %d (0 and 1 are implemented)", tensor_rank);
    CG_CHECK(tensor_rank == 0 || (index0 >= 0 && index0 < 3),
             "cg_realize_grid: index %d not in {0, 1, 2}", index0);
    const double vec = -out->p.boxsize / (2 * kPi);  // ℝ[-boxsize/(2*π)], ic.py:741
    return with_case<2>(tensor_rank, [=](auto k) {
        return launch(k_realize_grid<decltype(k)::value>, mode_count(out->N, out->f_nj), 0,
                      out->stream, slab(out), const_slab(noise), (int)out->N, out->f_j0, out->f_nj,
                      amplitudes, index0, vec);
    });
}

extern "C" int cg_realize_grid_tensor(cg_ctx *out, cg_ctx *structure, const double *amplitudes,
                                      int64_t k2_max, int index0, int index1) {
    if (realize_checks("cg_realize_grid_tensor", out, structure, amplitudes, k2_max)) return 1;
    CG_CHECK(index0 >= 0 && index0 < 3 && index1 >= 0 && index1 < 3,
             "cg_realize_grid_tensor: indices (%d, %d) not in {0, 1, 2}", index0, index1);
    return launch(k_realize_grid_tensor, mode_count(out->N, out->f_nj), 0, out->stream, slab(out),
                  const_slab(structure), (int)out->N, out->f_j0, out->f_nj, amplitudes, index0,
                  index1);
}

extern "C" int cg_shear_divergence(cg_ctx *out, cg_ctx *structure, const double *amplitudes,
                                   int64_t k2_max, int dim) {
    if (realize_checks("cg_shear_divergence", out, structure, amplitudes, k2_max)) return 1;
    CG_CHECK(dim >= 0 && dim < 3, "cg_shear_divergence: dim = %d not in {0, 1, 2}", dim);
    CG_CHECK(out->N <= 4096, "cg_shear_divergence: grid size %lld above 4096 (the table of sines "
             "is kept in LDS)", (long long)out->N);
    const double inv_dx = (double)out->N / out->p.boxsize;
    return launch(k_shear_divergence, mode_count(out->N, out->f_nj),
                  (size_t)out->N * sizeof(double), out->stream, slab(out), const_slab(structure),
                  (int)out->N, out->f_j0, out->f_nj, amplitudes, dim, inv_dx);
}

extern "C" int cg_fluid_add_from_mesh(cg_ctx *mesh, double *out, double factor) {
    return fluid_from_mesh("cg_fluid_add_from_mesh", mesh, out, 3, 0, factor, 0.0);
}

extern "C" int cg_fluid_from_mesh(cg_ctx *mesh, double *out, int mode, double c0, double c1) {
    const int var = mode == 1 ? 2 : (mode == 0 ? (c1 != 0 ? 1 : 0) : -1);
    return fluid_from_mesh("cg_fluid_from_mesh", mesh, out, var, mode, c0, c1);
}
