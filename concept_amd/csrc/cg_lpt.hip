// cg_lpt.hip — the mesh and particle passes of the realisations: 1LPT / 2LPT particles, fluids.
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
// neighbouring real cells (16-byte loads and stores), no LDS, no atomics, nothing wave-level.
// The k-space kernels walk the Fourier view of the contexts (cg_ctx::four, the view
// k_fourier_operate walks) over the N/2 + 1 modes of every row, the real-space kernels the N
// cells of the N rows of the owned layers: the row padding and the unused row of a layer are
// neither read nor written.  Compiled with -ffp-contract=off: every product and sum is rounded
// on its own, in the reference's order.  FP64 throughout.  The k-space kernels share their walk
// over the modes: kspace_mode (cg_kspace.h).
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
__global__ __launch_bounds__(kThreads) void k_lpt_potential(double2 *dst, const double2 *src,
                                                            int N, i64 dst_si, i64 src_si, i64 cp,
                                                            int j0, int nj, LptPotential P) {
#pragma clang fp contract(off)
    const i64 total = (i64)N * nj * (N / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, N, j0, nj);
        double2 out = make_double2(0.0, 0.0);  // nullify_modes(['origin', 'nyquist']), ic.py:764
        if (m.live) {
            const double2 z = src[(i64)m.a * src_si + (i64)m.bl * cp + m.kk];
            double re = z.x, im = z.y;
            if (P.shifted) {  // mesh.py:2873-2888, ic.py:719-726
                const double theta =
                    ((double)m.ki * P.A + (double)m.kj * P.B) + (double)m.kk * P.Cc;
                const double c = cos(theta), s = sin(theta);
                const double re2 = re * c - im * s, im2 = re * s + im * c;
                re = re2;
                im = im2;
            }
            if (P.amp) {  // ic.py:715, 761-762
                const double amplitude = P.amp[m.k2];
                re = amplitude * re;
                im = amplitude * im;
            }
            const double inv = P.lap / (double)m.k2;  // mesh.py:3434-3436
            out = make_double2(re * inv, im * inv);
        }
        dst[(i64)m.a * dst_si + (i64)m.bl * cp + m.kk] = out;
    }
}

// dst = i k_dim0 src (dim1 < 0) or -k_dim0 k_dim1 src, times factor; 0 on the origin and the
// Nyquist planes (the nullified output slab of mesh.py:3477)
__global__ __launch_bounds__(kThreads) void k_lpt_diff(double2 *dst, const double2 *src, int N,
                                                       i64 dst_si, i64 src_si, i64 cp, int j0,
                                                       int nj, int dim0, int dim1, double scale) {
#pragma clang fp contract(off)
    const i64 total = (i64)N * nj * (N / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, N, j0, nj);
        double2 out = make_double2(0.0, 0.0);
        if (m.live) {
            const double2 z = src[(i64)m.a * src_si + (i64)m.bl * cp + m.kk];
            const i64 kl0 = dim0 == 0 ? m.ki : (dim0 == 1 ? m.kj : m.kk);
            if (dim1 < 0) {
                const double amplitude = scale * (double)kl0;  // mesh.py:3496
                out = make_double2(amplitude * -z.y, amplitude * z.x);
            } else {
                const i64 kl1 = dim1 == 0 ? m.ki : (dim1 == 1 ? m.kj : m.kk);
                const double amplitude = scale * (double)kl0 * (double)kl1;  // mesh.py:3506
                out = make_double2(amplitude * -z.x, amplitude * -z.y);
            }
        }
        dst[(i64)m.a * dst_si + (i64)m.bl * cp + m.kk] = out;
    }
}

// out (= | += | -=) factor * a * b over the real cells; the three grids may be one another:
// a thread reads its pair of cells of a, b and (for '+=', '-=') out before it writes that same
// pair of out, and no other thread touches the pair, so the in-place product base *= tmp of
// handle_lpt_term (ic.py:2020-2021) is cg_lpt_product(out = a = base, b = tmp, '=')
template <int kOp>
__global__ __launch_bounds__(kThreads) void k_lpt_product(double *out, const double *a,
                                                          const double *b, int N, i64 nrows, i64 ny,
                                                          i64 pad, double factor) {
#pragma clang fp contract(off)
    const int half = N / 2;  // pairs of cells per row (N is even)
    const i64 total = nrows * half;
    for (i64 t = (i64)blockIdx.x * kThreads + threadIdx.x; t < total;
         t += (i64)gridDim.x * kThreads) {
        const i64 row = t / half;
        const int p = (int)(t - row * half);
        const i64 layer = row / N;
        const i64 off = (layer * ny + (row - layer * N)) * pad + 2 * p;
        const double2 x = *(const double2 *)(a + off), y = *(const double2 *)(b + off);
        double2 v = make_double2(x.x * y.x, x.y * y.y);  // ic.py:2020-2021
        if (factor != 1) v = make_double2(factor * v.x, factor * v.y);  // ic.py:2042-2057
        double2 *o = (double2 *)(out + off);
        if (kOp == 0) {
            *o = v;
        } else {
            const double2 w = *o;
            *o = kOp == 1 ? make_double2(w.x + v.x, w.y + v.y) : make_double2(w.x - v.x, w.y - v.y);
        }
    }
}

// particle p = (i*N + j)*N + k of the rows from index_bgn on takes cell (i, j, k) of psi
__global__ __launch_bounds__(kThreads) void k_lpt_displace(const double *psi, int N, i64 ny,
                                                           i64 pad, double *pos, double *mom,
                                                           int dim, double pos_factor,
                                                           double mom_factor) {
#pragma clang fp contract(off)
    const int half = N / 2;
    const i64 total = (i64)N * N * half;
    for (i64 t = (i64)blockIdx.x * kThreads + threadIdx.x; t < total;
         t += (i64)gridDim.x * kThreads) {
        const i64 row = t / half;  // i*N + j
        const int kp = (int)(t - row * half);
        const i64 i = row / N;
        const double2 v = *(const double2 *)(psi + (i * ny + (row - i * N)) * pad + 2 * kp);
        const i64 r = 3 * (row * N + 2 * kp) + dim;
        if (pos_factor != 0) {  // ic.py:2277-2279 (1*psi is psi: no branch for a factor of 1)
            pos[r] = pos[r] + pos_factor * v.x;
            pos[r + 3] = pos[r + 3] + pos_factor * v.y;
        }
        if (mom_factor != 0) {
            mom[r] = mom[r] + mom_factor * v.x;
            mom[r + 3] = mom[r + 3] + mom_factor * v.y;
        }
    }
}

// dst = amp[k2] * src (rank 0) or (amp[k2] * ((vec * k_index0) / k2)) * i src (rank 1) off the
// origin and the Nyquist planes, 0 on them; vec = ℝ[-boxsize/(2*π)] of ic.py:741
template <int kRank>
__global__ __launch_bounds__(kThreads) void k_realize_grid(double2 *dst, const double2 *src, int N,
                                                           i64 dst_si, i64 src_si, i64 cp, int j0,
                                                           int nj, const double *amp, int index0,
                                                           double vec) {
#pragma clang fp contract(off)
    const i64 total = (i64)N * nj * (N / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, N, j0, nj);
        double2 out = make_double2(0.0, 0.0);  // nullify_modes(['origin', 'nyquist']), ic.py:764
        if (m.live) {
            const double2 z = src[(i64)m.a * src_si + (i64)m.bl * cp + m.kk];
            double amplitude = amp[m.k2];  // ic.py:715
            double re = z.x, im = z.y;
            if (kRank == 1) {  // K(k) = -i k^l/k², ic.py:732-742
                const i64 kl = index0 == 0 ? m.ki : (index0 == 1 ? m.kj : m.kk);
                amplitude = amplitude * ((vec * (double)kl) / (double)m.k2);
                re = -z.y;
                im = z.x;
            }
            out = make_double2(amplitude * re, amplitude * im);  // ic.py:761-762
        }
        dst[(i64)m.a * dst_si + (i64)m.bl * cp + m.kk] = out;
    }
}

// dst = (amp[k2] * K) * src off the origin and the Nyquist planes, 0 on them;
// K = 0.5 [index0 == index1] - ((1.5 k_index0) k_index1) / k2, ic.py:744-759
__global__ __launch_bounds__(kThreads) void k_realize_grid_tensor(double2 *dst, const double2 *src,
                                                                  int N, i64 dst_si, i64 src_si,
                                                                  i64 cp, int j0, int nj,
                                                                  const double *amp, int index0,
                                                                  int index1) {
#pragma clang fp contract(off)
    const double half_delta = 0.5 * (index0 == index1);  // ℝ[0.5*(index0 == index1)]
    const i64 total = (i64)N * nj * (N / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, N, j0, nj);
        double2 out = make_double2(0.0, 0.0);  // nullify_modes(['origin', 'nyquist']), ic.py:764
        if (m.live) {
            const double2 z = src[(i64)m.a * src_si + (i64)m.bl * cp + m.kk];
            const i64 kl = index0 == 0 ? m.ki : (index0 == 1 ? m.kj : m.kk);
            const i64 km = index1 == 0 ? m.ki : (index1 == 1 ? m.kj : m.kk);
            const double amplitude =
                amp[m.k2] * (half_delta - ((1.5 * (double)kl) * (double)km) / (double)m.k2);
            out = make_double2(amplitude * z.x, amplitude * z.y);  // ic.py:761-762
        }
        dst[(i64)m.a * dst_si + (i64)m.bl * cp + m.kk] = out;
    }
}

// dst = (amp[k2] * S) * i src off the origin and the Nyquist planes, 0 on them;
// S = Σ_j s_j K_dim,j = 0.5 s_dim - ((1.5 k_dim) (s_0 ki + s_1 kj + s_2 kk)) / k2 with K of
// k_realize_grid_tensor and s_j = sin(2π k_j/N)/Δx, the order-2 central difference of
// diff_domaingrid (mesh.py:4966-4970) in Fourier space.  The N sines by array index are
// tabulated once per workgroup (dynamic LDS, N doubles): a mode reads three of them.
__global__ __launch_bounds__(kThreads) void k_shear_divergence(double2 *dst, const double2 *src,
                                                               int N, i64 dst_si, i64 src_si,
                                                               i64 cp, int j0, int nj,
                                                               const double *amp, int dim,
                                                               double inv_dx) {
#pragma clang fp contract(off)
    extern __shared__ double s_sin[];
    for (int a = threadIdx.x; a < N; a += kThreads) {
        const int k = a - (a >= N / 2 ? N : 0);
        s_sin[a] = sinpi((double)(2 * k) / (double)N) * inv_dx;
    }
    __syncthreads();
    const i64 total = (i64)N * nj * (N / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, N, j0, nj);
        double2 out = make_double2(0.0, 0.0);
        if (m.live) {
            const double2 z = src[(i64)m.a * src_si + (i64)m.bl * cp + m.kk];
            const double s0 = s_sin[m.a], s1 = s_sin[j0 + m.bl], s2 = s_sin[m.kk];
            const i64 kd = dim == 0 ? m.ki : (dim == 1 ? m.kj : m.kk);
            const double sd = dim == 0 ? s0 : (dim == 1 ? s1 : s2);
            const double dot = (s0 * (double)m.ki + s1 * (double)m.kj) + s2 * (double)m.kk;
            const double amplitude =
                amp[m.k2] * (0.5 * sd - ((1.5 * (double)kd) * dot) / (double)m.k2);
            out = make_double2(amplitude * -z.y, amplitude * z.x);
        }
        dst[(i64)m.a * dst_si + (i64)m.bl * cp + m.kk] = out;
    }
}

// out[layer][j][k] (dense) from the real cells of the mesh's owned layers.
// kVar 0: c0 * (1 + v); 1: the same after v += c1 * v²; 2: v * c0; 3: out + c0 * v
template <int kVar>
__global__ __launch_bounds__(kThreads) void k_fluid_from_mesh(const double *mesh, double *out,
                                                              int N, i64 nrows, i64 ny, i64 pad,
                                                              double c0, double c1) {
#pragma clang fp contract(off)
    const int half = N / 2;  // pairs of cells per row (N is even)
    const i64 total = nrows * half;
    for (i64 t = (i64)blockIdx.x * kThreads + threadIdx.x; t < total;
         t += (i64)gridDim.x * kThreads) {
        const i64 row = t / half;
        const int p = (int)(t - row * half);
        const i64 layer = row / N;
        double2 v = *(const double2 *)(mesh + (layer * ny + (row - layer * N)) * pad + 2 * p);
        if (kVar == 1)  // ic.py:436
            v = make_double2(v.x + c1 * (v.x * v.x), v.y + c1 * (v.y * v.y));
        double2 *o = (double2 *)(out + row * N + 2 * p);
        if (kVar == 3) {  // fluid.py:1028, 1042
            const double2 w = *o;
            v = make_double2(w.x + c0 * v.x, w.y + c0 * v.y);
        } else if (kVar == 2) {
            v = make_double2(v.x * c0, v.y * c0);  // ic.py:456
        } else {
            v = make_double2(c0 * (1 + v.x), c0 * (1 + v.y));  // ic.py:437
        }
        *o = v;
    }
}

// ---- 3LPT and Orszag dealiasing: the passes between the realisation size N and the dealiasing
// size M = 3N/2 (+1 when odd).  The size-change phase of copy_modes (mesh.py:1302) is
// theta = (pi/N_onto - pi/N_from)*((ki + kj) + kk), applied on the way up and on the way down.

// `small` is the cube of |k| < n/2 of a grid of size n inside a larger one
__device__ __forceinline__ bool in_cube(const KspaceMode &m, int n) {
    const int h = n / 2;
    return m.ki > -h && m.ki < h && m.kj > -h && m.kj < h && m.kk < h;
}
// array index of signed wave number k in a grid of size n
__device__ __forceinline__ i64 wrap_index(i64 k, int n) { return k + (k < 0 ? n : 0); }

// fourier_diff at N (k_lpt_diff's rounding) + resize_grid to M (mesh.py:916-922) in one pass over
// dst: inside the cube the rotated derivative, everywhere else (src's Nyquist planes and all of
// dst's included) zero without a read.  Every mode of dst is written exactly once.
__global__ __launch_bounds__(kThreads) void k_lpt_diff_enlarge(double2 *dst, const double2 *src,
                                                               int M, int N, i64 dst_si, i64 dst_cp,
                                                               i64 src_si, i64 src_cp, int dim0,
                                                               int dim1, double scale,
                                                               double dtheta) {
#pragma clang fp contract(off)
    const i64 total = (i64)M * M * (M / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, M, 0, M);
        double2 out = make_double2(0.0, 0.0);
        if (m.k2 != 0 && in_cube(m, N)) {
            const double2 z =
                src[wrap_index(m.ki, N) * src_si + wrap_index(m.kj, N) * src_cp + m.kk];
            const i64 kl0 = dim0 == 0 ? m.ki : (dim0 == 1 ? m.kj : m.kk);
            double re, im;
            if (dim1 < 0) {
                const double amplitude = scale * (double)kl0;  // mesh.py:3496
                re = amplitude * -z.y;
                im = amplitude * z.x;
            } else {
                const i64 kl1 = dim1 == 0 ? m.ki : (dim1 == 1 ? m.kj : m.kk);
                const double amplitude = scale * (double)kl0 * (double)kl1;  // mesh.py:3506
                re = amplitude * -z.x;
                im = amplitude * -z.y;
            }
            const double theta = dtheta * (double)((m.ki + m.kj) + m.kk);  // mesh.py:1302
            const double c = cos(theta), s = sin(theta);
            out = make_double2(re * c - im * s, re * s + im * c);  // mesh.py:1310-1313
        }
        dst[(i64)m.a * dst_si + (i64)m.bl * dst_cp + m.kk] = out;
    }
}

// nullify_modes(slab, 'beyond cube of |k| < n/2') (ic.py:2025): zeros outside the cube, nothing
// read, nothing written inside
__global__ __launch_bounds__(kThreads) void k_lpt_dealias_cube(double2 *mesh, int M, int n, i64 si,
                                                               i64 cp) {
    const i64 total = (i64)M * M * (M / 2 + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, M, 0, M);
        if (!in_cube(m, n)) mesh[(i64)m.a * si + (i64)m.bl * cp + m.kk] = make_double2(0.0, 0.0);
    }
}

// resize_grid down to N (nullify 'nyquist', copy_modes; mesh.py:912-922) + the move to the output
// grid (ic.py:2038-2057) in one pass over out: rotation, factor and sum rounded in turn.  On
// out's Nyquist planes the shrunk grid is zero: '=' writes it, '+=' and '-=' leave out as it is.
template <int kOp>
__global__ __launch_bounds__(kThreads) void k_lpt_shrink_accumulate(double2 *out,
                                                                    const double2 *src, int N,
                                                                    int M, i64 out_si, i64 out_cp,
                                                                    i64 src_si, i64 src_cp,
                                                                    double factor, double dtheta) {
#pragma clang fp contract(off)
    const int nyq = N / 2;
    const i64 total = (i64)N * N * (nyq + 1);
    for (i64 e = (i64)blockIdx.x * kThreads + threadIdx.x; e < total;
         e += (i64)gridDim.x * kThreads) {
        const KspaceMode m = kspace_mode(e, N, 0, N);
        double2 *o = out + (i64)m.a * out_si + (i64)m.bl * out_cp + m.kk;
        if (m.a == nyq || m.bl == nyq || m.kk == nyq) {
            if (kOp == 0) *o = make_double2(0.0, 0.0);
            continue;
        }
        const double2 z = src[wrap_index(m.ki, M) * src_si + wrap_index(m.kj, M) * src_cp + m.kk];
        const double theta = dtheta * (double)((m.ki + m.kj) + m.kk);  // mesh.py:1302
        const double c = cos(theta), s = sin(theta);
        double2 v = make_double2(z.x * c - z.y * s, z.x * s + z.y * c);
        if (factor != 1) v = make_double2(factor * v.x, factor * v.y);  // ic.py:2042-2057
        if (kOp == 0) {
            *o = v;
        } else {
            const double2 w = *o;
            *o = kOp == 1 ? make_double2(w.x + v.x, w.y + v.y) : make_double2(w.x - v.x, w.y - v.y);
        }
    }
}

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

// two meshes of a realisation in Fourier space and its k²-indexed table of amplitudes
int realize_checks(const char *name, cg_ctx *out, cg_ctx *src, const double *amplitudes,
                   int64_t k2_max) {
    if (fourier_pair_checks(name, out, src)) return 1;
    const i64 nyq = out->N / 2;
    CG_CHECK(amplitudes != nullptr, "%s: no amplitudes", name);
    CG_CHECK(k2_max == 3 * (nyq - 1) * (nyq - 1),
             "%s: %lld amplitudes for grid size %lld, which needs 3*(nyquist - 1)**2 + 1 = %lld",
             name, (long long)(k2_max + 1), (long long)out->N,
             (long long)(3 * (nyq - 1) * (nyq - 1) + 1));
    return 0;
}

// two single-domain contexts of different grid size in Fourier space: `large` of size M, `small`
// of size N < M
int resize_pair_checks(const char *name, cg_ctx *large, cg_ctx *small) {
    CG_CHECK(large && small, "%s: null context", name);
    CG_CHECK(large->four != nullptr && small->four != nullptr,
             "%s: no Fourier buffer bound (cg_dist_bind_fourier)", name);
    CG_CHECK(large->p.nprocs == 1 && small->p.nprocs == 1, "%s: single-domain entry point", name);
    CG_CHECK(small->N >= 2 && small->N % 2 == 0 && large->N % 2 == 0,
             "%s: grid sizes %lld and %lld are not both even", name, (long long)small->N,
             (long long)large->N);
    CG_CHECK(large->N > small->N, "%s: grid size %lld is not larger than %lld", name,
             (long long)large->N, (long long)small->N);
    CG_CHECK(large->p.boxsize == small->p.boxsize, "%s: the two meshes span different boxes", name);
    CG_CHECK(large->N * large->N < ((i64)1 << 31), "%s: %lld rows", name,
             (long long)(large->N * large->N));
    return 0;
}

}  // namespace

extern "C" int cg_lpt_potential(cg_ctx *dst, cg_ctx *noise_src, const double *amplitudes,
                                int64_t k2_max, const double *shift, double factor) {
    if (fourier_pair_checks("cg_lpt_potential", dst, noise_src)) return 1;
    const i64 nyq = dst->N / 2;
    CG_CHECK(!amplitudes || k2_max == 3 * (nyq - 1) * (nyq - 1),
             "cg_lpt_potential: %lld amplitudes for grid size %lld, which needs "
             "3*(nyquist - 1)**2 + 1 = %lld", (long long)(k2_max + 1), (long long)dst->N,
             (long long)(3 * (nyq - 1) * (nyq - 1) + 1));
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
    const i64 total = dst->N * (i64)dst->f_nj * (nyq + 1);
    hipLaunchKernelGGL(k_lpt_potential, dim3(grid_for(total)), dim3(kThreads), 0, dst->stream,
                       dst->four, (const double2 *)noise_src->four, (int)dst->N, dst->f_si,
                       noise_src->f_si, dst->pad / 2, dst->f_j0, dst->f_nj, P);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_lpt_diff(cg_ctx *dst, cg_ctx *src, int dim0, int dim1, double factor) {
    if (fourier_pair_checks("cg_lpt_diff", dst, src)) return 1;
    CG_CHECK(dim0 >= 0 && dim0 < 3 && dim1 >= -1 && dim1 < 3,
             "cg_lpt_diff: dimensions (%d, %d) outside 0..2 (the second may be -1)", dim0, dim1);
    // the first derivative with factor 1 into another mesh is fourier_operate(diff_dim) to the bit
    if (dim1 < 0 && factor == 1 && dst != src)
        return cgk_fourier_operate(dst, src, 0, 1, nullptr, dim0, 0);
    const double k_fundamental = 2 * kPi / dst->p.boxsize;
    const double scale = dim1 < 0 ? factor * k_fundamental
                                  : factor * (k_fundamental * k_fundamental);
    const i64 total = dst->N * (i64)dst->f_nj * (dst->N / 2 + 1);
    hipLaunchKernelGGL(k_lpt_diff, dim3(grid_for(total)), dim3(kThreads), 0, dst->stream,
                       dst->four, (const double2 *)src->four, (int)dst->N, dst->f_si, src->f_si,
                       dst->pad / 2, dst->f_j0, dst->f_nj, dim0, dim1, scale);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_lpt_product(cg_ctx *out, cg_ctx *a, cg_ctx *b, int op, double factor) {
    CG_CHECK(out && a && b, "cg_lpt_product: null context");
    CG_CHECK(op >= 0 && op <= 2, "cg_lpt_product: operation %d not in {0 '=', 1 '+=', 2 '-='}", op);
    CG_CHECK(out->N >= 2 && out->N % 2 == 0, "cg_lpt_product: grid size %lld is not even",
             (long long)out->N);
    CG_CHECK(same_geometry(out, a) && same_geometry(out, b),
             "cg_lpt_product: the meshes differ in grid size or domain");
    const i64 nrows = out->xmap.nxl * out->N;
    const i64 total = nrows * (out->N / 2);
#define CG_LPT_PRODUCT(OP)                                                                      \
    hipLaunchKernelGGL(k_lpt_product<OP>, dim3(grid_for(total)), dim3(kThreads), 0, out->stream, \
                       out->mesh0, (const double *)a->mesh0, (const double *)b->mesh0,          \
                       (int)out->N, nrows, out->ny, out->pad, factor)
    if (op == 0) CG_LPT_PRODUCT(0);
    else if (op == 1) CG_LPT_PRODUCT(1);
    else CG_LPT_PRODUCT(2);
#undef CG_LPT_PRODUCT
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_lpt_diff_enlarge(cg_ctx *dst, cg_ctx *src, int dim0, int dim1, double factor) {
    if (resize_pair_checks("cg_lpt_diff_enlarge", dst, src)) return 1;
    CG_CHECK(dim0 >= 0 && dim0 < 3 && dim1 >= -1 && dim1 < 3,
             "cg_lpt_diff_enlarge: dimensions (%d, %d) outside 0..2 (the second may be -1)", dim0,
             dim1);
    const double k_fundamental = 2 * kPi / src->p.boxsize;
    const double scale = dim1 < 0 ? factor * k_fundamental
                                  : factor * (k_fundamental * k_fundamental);
    const double dtheta = kPi / (double)dst->N - kPi / (double)src->N;  // mesh.py:1302
    const i64 total = dst->N * dst->N * (dst->N / 2 + 1);
    hipLaunchKernelGGL(k_lpt_diff_enlarge, dim3(grid_for(total)), dim3(kThreads), 0, dst->stream,
                       dst->four, (const double2 *)src->four, (int)dst->N, (int)src->N, dst->f_si,
                       dst->pad / 2, src->f_si, src->pad / 2, dim0, dim1, scale, dtheta);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_lpt_dealias_cube(cg_ctx *mesh, int64_t n_small) {
    CG_CHECK(mesh, "cg_lpt_dealias_cube: null context");
    CG_CHECK(mesh->four != nullptr,
             "cg_lpt_dealias_cube: no Fourier buffer bound (cg_dist_bind_fourier)");
    CG_CHECK(mesh->p.nprocs == 1, "cg_lpt_dealias_cube: single-domain entry point");
    CG_CHECK(n_small >= 2 && n_small % 2 == 0 && mesh->N % 2 == 0,
             "cg_lpt_dealias_cube: grid sizes %lld and %lld are not both even", (long long)n_small,
             (long long)mesh->N);
    CG_CHECK(n_small < mesh->N, "cg_lpt_dealias_cube: grid size %lld is not larger than %lld",
             (long long)mesh->N, (long long)n_small);
    CG_CHECK(mesh->N * mesh->N < ((i64)1 << 31), "cg_lpt_dealias_cube: %lld rows",
             (long long)(mesh->N * mesh->N));
    const i64 total = mesh->N * mesh->N * (mesh->N / 2 + 1);
    hipLaunchKernelGGL(k_lpt_dealias_cube, dim3(grid_for(total)), dim3(kThreads), 0, mesh->stream,
                       mesh->four, (int)mesh->N, (int)n_small, mesh->f_si, mesh->pad / 2);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_lpt_shrink_accumulate(cg_ctx *out, cg_ctx *src, int op, double factor) {
    if (resize_pair_checks("cg_lpt_shrink_accumulate", src, out)) return 1;
    CG_CHECK(op >= 0 && op <= 2,
             "cg_lpt_shrink_accumulate: operation %d not in {0 '=', 1 '+=', 2 '-='}", op);
    const double dtheta = kPi / (double)out->N - kPi / (double)src->N;  // mesh.py:1302
    const i64 total = out->N * out->N * (out->N / 2 + 1);
#define CG_LPT_SHRINK(OP)                                                                        \
    hipLaunchKernelGGL(k_lpt_shrink_accumulate<OP>, dim3(grid_for(total)), dim3(kThreads), 0,    \
                       out->stream, out->four, (const double2 *)src->four, (int)out->N,          \
                       (int)src->N, out->f_si, out->pad / 2, src->f_si, src->pad / 2, factor,    \
                       dtheta)
    if (op == 0) CG_LPT_SHRINK(0);
    else if (op == 1) CG_LPT_SHRINK(1);
    else CG_LPT_SHRINK(2);
#undef CG_LPT_SHRINK
    CG_LAUNCH_CHECK();
    return 0;
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
    hipLaunchKernelGGL(k_lpt_displace, dim3(grid_for(n / 2)), dim3(kThreads), 0, psi->stream,
                       (const double *)psi->mesh0, (int)psi->N, psi->ny, psi->pad,
                       pos ? pos + 3 * index_bgn : nullptr, mom ? mom + 3 * index_bgn : nullptr,
                       dim, pos_factor, mom_factor);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_realize_grid(cg_ctx *out, cg_ctx *noise, const double *amplitudes, int64_t k2_max,
                               int tensor_rank, int index0) {
    if (realize_checks("cg_realize_grid", out, noise, amplitudes, k2_max)) return 1;
    const i64 nyq = out->N / 2;
    CG_CHECK(tensor_rank == 0 || tensor_rank == 1,
             "cg_realize_grid: tensor rank %d (0 and 1 are implemented)", tensor_rank);
    CG_CHECK(tensor_rank == 0 || (index0 >= 0 && index0 < 3),
             "cg_realize_grid: index %d not in {0, 1, 2}", index0);
    const double vec = -out->p.boxsize / (2 * kPi);  // ℝ[-boxsize/(2*π)], ic.py:741
    const i64 total = out->N * (i64)out->f_nj * (nyq + 1);
#define CG_REALIZE_GRID(RANK)                                                                     \
    hipLaunchKernelGGL(k_realize_grid<RANK>, dim3(grid_for(total)), dim3(kThreads), 0,           \
                       out->stream, out->four, (const double2 *)noise->four, (int)out->N,        \
                       out->f_si, noise->f_si, out->pad / 2, out->f_j0, out->f_nj, amplitudes,   \
                       index0, vec)
    if (tensor_rank == 0) CG_REALIZE_GRID(0);
    else CG_REALIZE_GRID(1);
#undef CG_REALIZE_GRID
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_realize_grid_tensor(cg_ctx *out, cg_ctx *structure, const double *amplitudes,
                                      int64_t k2_max, int index0, int index1) {
    if (realize_checks("cg_realize_grid_tensor", out, structure, amplitudes, k2_max)) return 1;
    CG_CHECK(index0 >= 0 && index0 < 3 && index1 >= 0 && index1 < 3,
             "cg_realize_grid_tensor: indices (%d, %d) not in {0, 1, 2}", index0, index1);
    const i64 total = out->N * (i64)out->f_nj * (out->N / 2 + 1);
    hipLaunchKernelGGL(k_realize_grid_tensor, dim3(grid_for(total)), dim3(kThreads), 0,
                       out->stream, out->four, (const double2 *)structure->four, (int)out->N,
                       out->f_si, structure->f_si, out->pad / 2, out->f_j0, out->f_nj, amplitudes,
                       index0, index1);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_shear_divergence(cg_ctx *out, cg_ctx *structure, const double *amplitudes,
                                   int64_t k2_max, int dim) {
    if (realize_checks("cg_shear_divergence", out, structure, amplitudes, k2_max)) return 1;
    CG_CHECK(dim >= 0 && dim < 3, "cg_shear_divergence: dim = %d not in {0, 1, 2}", dim);
    CG_CHECK(out->N <= 4096, "cg_shear_divergence: grid size %lld above 4096 (the table of sines "
             "is kept in LDS)", (long long)out->N);
    const double inv_dx = (double)out->N / out->p.boxsize;
    const i64 total = out->N * (i64)out->f_nj * (out->N / 2 + 1);
    hipLaunchKernelGGL(k_shear_divergence, dim3(grid_for(total)), dim3(kThreads),
                       (size_t)out->N * sizeof(double), out->stream, out->four,
                       (const double2 *)structure->four, (int)out->N, out->f_si, structure->f_si,
                       out->pad / 2, out->f_j0, out->f_nj, amplitudes, dim, inv_dx);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_fluid_add_from_mesh(cg_ctx *mesh, double *out, double factor) {
    CG_CHECK(mesh && out, "cg_fluid_add_from_mesh: null %s", mesh ? "output grid" : "context");
    CG_CHECK(mesh->N >= 2 && mesh->N % 2 == 0,
             "cg_fluid_add_from_mesh: grid size %lld is not even", (long long)mesh->N);
    CG_CHECK((uintptr_t)out % 16 == 0,
             "cg_fluid_add_from_mesh: the output grid is not 16-byte aligned");
    const i64 nrows = mesh->xmap.nxl * mesh->N;
    const i64 total = nrows * (mesh->N / 2);
    hipLaunchKernelGGL(k_fluid_from_mesh<3>, dim3(grid_for(total)), dim3(kThreads), 0,
                       mesh->stream, (const double *)mesh->mesh0, out, (int)mesh->N, nrows,
                       mesh->ny, mesh->pad, factor, 0.0);
    CG_LAUNCH_CHECK();
    return 0;
}

extern "C" int cg_fluid_from_mesh(cg_ctx *mesh, double *out, int mode, double c0, double c1) {
    CG_CHECK(mesh && out, "cg_fluid_from_mesh: null %s", mesh ? "output grid" : "context");
    CG_CHECK(mode == 0 || mode == 1, "cg_fluid_from_mesh: mode %d not in {0 ϱ, 1 J}", mode);
    CG_CHECK(mesh->N >= 2 && mesh->N % 2 == 0, "cg_fluid_from_mesh: grid size %lld is not even",
             (long long)mesh->N);
    CG_CHECK((uintptr_t)out % 16 == 0, "cg_fluid_from_mesh: the output grid is not 16-byte aligned");
    const i64 nrows = mesh->xmap.nxl * mesh->N;
    const i64 total = nrows * (mesh->N / 2);
#define CG_FLUID_FROM_MESH(VAR)                                                                   \
    hipLaunchKernelGGL(k_fluid_from_mesh<VAR>, dim3(grid_for(total)), dim3(kThreads), 0,         \
                       mesh->stream, (const double *)mesh->mesh0, out, (int)mesh->N, nrows,      \
                       mesh->ny, mesh->pad, c0, c1)
    if (mode == 1) CG_FLUID_FROM_MESH(2);
    else if (c1 != 0) CG_FLUID_FROM_MESH(1);
    else CG_FLUID_FROM_MESH(0);
#undef CG_FLUID_FROM_MESH
    CG_LAUNCH_CHECK();
    return 0;
}
