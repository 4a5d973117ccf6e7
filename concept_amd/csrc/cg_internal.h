// cg_internal.h — shared declarations of libconcept_gpu.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "concept_gpu.h"

typedef int64_t i64;

void cg_set_error(const char *fmt, ...);

#define CG_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            cg_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,     \
                         __LINE__);                                                           \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

// after a kernel launch
#define CG_LAUNCH_CHECK()                                                                     \
    do {                                                                                      \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess) {                                                               \
            cg_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, \
                         __LINE__);                                                           \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

#define CG_CHECK(cond, ...)                                                                   \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            cg_set_error(__VA_ARGS__);                                                        \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

// A template argument from a run-time integer (host): f(std::integral_constant<int, K>) for
// K = which.  The last of the kCases takes whatever is left, as the `else` of a chain does: the
// caller has refused a `which` outside 0 .. kCases - 1 before
template <int kCases, int K = 0, class F>
int with_case(int which, F f) {
    if constexpr (K + 1 < kCases) {
        if (which != K) return with_case<kCases, K + 1>(which, f);
    }
    return f(std::integral_constant<int, K>{});
}

// Geometry of the CIC index map for one domain, computed on the host with
// the reference's own expressions (mesh.py:1577-1606 deposit, :408-432 gather).
struct CicGeom {
    double off[3];  // offset_x/y/z
    double scale;   // (1/cellsize)*(1 - machine_eps)
};

// How a global x cell index maps to a layer of the local mesh buffer.
// Single domain: the buffer is the whole periodic mesh (layer = x mod N).
// x-slab domains (one per GPU): the buffer holds layers [x0-G, x0+nxl+G) of
// the global mesh — nxl owned layers between G ghost layers — and y, z stay
// periodic.  Cell (x, j, k) lives at mesh[(layer*ny + j)*pad + k]: a layer is ny >= N rows
// of pad doubles (ny = N + 1 when N is a multiple of 16, see cg_ctx::ny).
struct XMap {
    i64 x0;    // first owned global layer
    i64 nxl;   // owned layers
    int G;     // ghost layers on each side (0 when periodic)
    int periodic;
};
__host__ __device__ inline i64 cg_xlayer(const XMap &m, i64 a, i64 N) {
    if (m.periodic) {
        a = a < 0 ? a + N : a;
        return a >= N ? a - N : a;
    }
    i64 l = a - m.x0;
    if (l < -(i64)m.G) l += N;             // periodic image across the box seam
    else if (l >= m.nxl + m.G) l -= N;
    l += m.G;
    // a cell outside the local layers can only come from a particle this domain does
    // not own (host-side contract: exchange before use); never index out of the buffer
    l = l < 0 ? 0 : l;
    return l >= m.nxl + 2 * m.G ? m.nxl + 2 * m.G - 1 : l;
}

// Tile decomposition used for the particle memory order and the LDS-tiled
// deposit / gather kernels.
struct TileGeom {
    int tx, ty, tz;     // tile extent in cells
    int ntx, nty, ntz;  // tiles per dimension
};

// A device allocation that belongs to its holder (the context, RocfftBackend) and is freed with it.
// reserve() returns at once when the buffer is large enough; otherwise it drains c->stream (the
// old buffer may be in use), frees it and allocates the new size: the contents are not kept.
// On failure the buffer is left empty, the error is set and 1 is returned.
struct cg_ctx;
struct cg_devmem {
    void *ptr = nullptr;
    size_t bytes = 0;
    cg_devmem() = default;
    cg_devmem(const cg_devmem &) = delete;
    cg_devmem &operator=(const cg_devmem &) = delete;
    ~cg_devmem() { release(); }
    int reserve(cg_ctx *c, size_t need);
    void release();
};
// ... seen as an array of T
template <typename T>
struct cg_buf : cg_devmem {
    operator T *() const { return (T *)ptr; }
};

struct cg_ctx {
    // ---- parameters and geometry ----
    cg_params p;
    hipStream_t stream = nullptr;
    i64 N = 0, pad = 0;          // grid size and row pitch: N+16 when N is a multiple of 16, else N+2
    XMap xmap{};                 // local layers of the mesh buffer
    // rows per x layer.  N rows are used; with N a power of two the layer stride N*pad*8 B
    // is 2^17 x odd at 1024^3 and the 1024 row segments an x-pass tile touches alias onto
    // few memory channels (measured with tools/stride_probe.cpp: 3.99 ms per in-place
    // sweep at stride 8,519,680 B, 3.52 ms at 8,528,000 B): one unused row per layer
    // breaks the pattern.
    i64 ny = 0;
    CicGeom geom_deposit{}, geom_gather{};
    i64 device_bytes = 0;        // cg_device_bytes: the mesh, the tile tables, rocFFT's work buffer

    // ---- mesh and Fourier view ----
    cg_buf<double> mesh;         // double[layers][ny][pad], layers = nxl + 2G
    double *mesh0 = nullptr;     // first OWNED layer (= mesh + G*ny*pad)
    i64 mesh_doubles = 0;
    // Fourier view: where the modes of this context live and which of them.  Mode (ki, kj, kk)
    // with array indices (a, b, kk), b in [f_j0, f_j0 + f_nj), sits at
    // four[a*f_si + (b - f_j0)*cp + kk], cp = pad/2.  Single domain: the mesh itself, in place
    // (f_si = ny*cp, all N rows b).  x-slab domains: the transposed buffer of the distributed
    // FFT, complex[N][JB + 1][cp] with the rows b of this domain's block [rank*JB, (rank+1)*JB)
    // (fft.c:55-72: FFTW-MPI's transposed output is distributed the same way), bound by the
    // caller with cg_dist_bind_fourier.
    double2 *four = nullptr;
    i64 f_si = 0;
    int f_j0 = 0, f_nj = 0;
    cg_buf<double> fetch_tmp;    // lazily allocated, for CG_FETCH_MESH_FOURIER
    // k-space tables: numerator n(k), denominator sin(n(k)) and their quotient by array index
    cg_buf<double> ktab_n, ktab_s, ktab_q;

    // ---- FFT ----
    // the rocFFT backend (cg_rocfft.hip): its plans, execution info and work buffer; null on a
    // context of the hand-written FFT
    struct RocfftBackend *libfft = nullptr;
    // hand-written FFT (cg_fft.hip): twiddles exp(-2 pi i k/N) as double2[N]
    bool custom_fft = false;
    cg_buf<double2> fft_tw;
    // what its plans (cg_fft_plan.h) depend on: the device's CU count and CONCEPT_GPU_FFT_SPLIT
    int ncu = 0, fft_split = 1;

    // ---- tiles, sort and regions ----
    TileGeom tiles{};
    i64 ntiles = 0;
    cg_buf<unsigned> tile_count;   // [8 ntiles + 1]: 8 buckets per tile (cg_particles.hip)
    cg_buf<unsigned> tile_cursor;  // [8 ntiles + 1]
    cg_buf<void> scan_tmp;         // cg_exclusive_sum's temporary storage
    // tile kernels: heavy tiles first when the tiles' populations are far from equal
    // (cgk_tile_order; off = the plain walk)
    cg_buf<unsigned> tile_order_buf;     // populations, the list, counters and ranks
    unsigned int *tile_order = nullptr;  // the list [tile_order_cap] inside tile_order_buf
    unsigned tile_order_cap = 0;
    unsigned *tile_order_seen = nullptr;  // pinned: length of the list of the last build done
    bool tile_order_on = false;          // list and bytes of one build are there
    int tile_order_mode = -1;            // from CONCEPT_GPU_TILE_ORDER_MIN: 0 off, 1 on, 2 also on small boxes
    unsigned tile_order_floor = 1536;    // |CONCEPT_GPU_TILE_ORDER_MIN|
    const void *tile_order_src[2] = {nullptr, nullptr};  // (start, count) it was made from

    // ---- fused pass and emigrants ----
    // tile histogram of the NEXT drift prepared by cg_gather_kick_tiled_prepare
    bool prep_valid = false;
    const double *prep_pos = nullptr, *prep_mom = nullptr;
    i64 prep_n = 0;
    double prep_dtm = 0;
    hipEvent_t *pass_events = nullptr;  // when set: 6 events recorded around the 5 passes
    // caller-owned list of the particles leaving the slab with the prepared drift
    i64 *emig_idx = nullptr;
    unsigned *emig_count = nullptr;
    i64 emig_cap = 0;
    // fused kick + drift + scatter on x-slab domains: the particles the drift takes out of the
    // slab are appended here as rows of 8 doubles (pos 3, mom 3, id bits, unused) — caller-owned
    double *emig_rows = nullptr;
    unsigned *emig_rows_count = nullptr;
    i64 emig_rows_cap = 0;
    // cg_set_momentum_sum: where the fused pass leaves the sum of |mom|^2 (null: not summed;
    // caller-owned), and its per-workgroup partial sums
    double *mom2_sum_out = nullptr;
    cg_buf<double> mom2_partial;

    // ---- short-range list and sweeps ----
    cg_buf<unsigned> sr_tmp;  // cell-list and tile-list counters
    // side streams of the short-range sweep (its interior and face launches are independent and
    // run side by side: a clustered box otherwise waits for the few dense tiles of each launch
    // in turn), created at the first sweep
    hipStream_t sr_streams[3] = {nullptr, nullptr, nullptr};
    hipEvent_t sr_fork = nullptr, sr_join[3] = {nullptr, nullptr, nullptr};
    cg_buf<unsigned long long> sr_stats;   // cg_shortrange_stats: device counters while on
    cg_buf<unsigned char> sr_tile_active;  // cells sweep with rungs: one byte per tile
    cg_buf<unsigned> sr_active;   // [0] count, [64..] the cells that hold an active receiver
    cg_buf<double> sr_sparse_partial;      // cg_shortrange_sparse: per-workgroup partial sums

    // ---- dense tiles ----
    // the dense tiles' sweep (cg_shortrange_dense.hip): counters, pinned read-back, lists, stream;
    // srd_look: what is known about the cell lists built last (keyed by their offsets' address)
    struct SrdLook {
        const unsigned *off = nullptr;
        i64 nt = 0;
        int min_pop = 0;
        hipEvent_t ev = nullptr;
        bool harvested = true;   // its result is known to be in srd_host
    } srd_look[4];
    // looks taken (look k sits in slot k % 4 until look k + 4 takes it over), and how many of
    // them, in the order taken, have been counted in srd_quiet
    unsigned long long srd_looks = 0, srd_counted = 0;
    int srd_idle = 0;
    int srd_quiet = 0;   // counted looks in a row that found no dense tile
    bool srd_hilbert_done = false;
    unsigned *srd_host = nullptr;
    cg_buf<unsigned> srd_small;
    cg_buf<void> srd_buf;
    cg_buf<signed char> srd_rung;
    hipStream_t srd_stream = nullptr;
    hipEvent_t srd_fork = nullptr, srd_join = nullptr;
    cg_buf<void> sr_sub_tmp;  // rows of the dense tiles while they are re-ordered by sub-cell

    // ---- sub-step ----
    // a sub-step's first pass, deferred to the cell list that follows it (cg_substep.h)
    struct SubstepBegin *sub_begin = nullptr;
    bool sub_pending = false;
    long long *sub_counts = nullptr;     // where the pending pass leaves the populations (DEV)
    cg_buf<unsigned> sub_partial;        // ... per workgroup first

    // ---- fluid solver ----
    cg_buf<double> fluid_partial;        // cg_fluid_vmax: per-workgroup partial maxima

    // ---- measure() ----
    cg_buf<double> measure_partial;      // cg_measure_*: per-workgroup partial results

    // ---- bispectrum ----
    cg_buf<double> bispec_partial;       // cg_bispec_sums: per-workgroup partial sums

    // ---- errors ----
    // device word of sticky error bits set by kernels (CG_ERR_*), read by cg_error_flags
    cg_buf<unsigned> err_flags;
};

// ---- cg_mesh_kernels.hip: CIC gather-kick, k-space kernel, slab helpers ----
int cgk_kspace(cg_ctx *c, int deconv_order, double C, int long_range, double E);
int cgk_gather_kick(cg_ctx *c, const double *pos, double *mom, i64 n, int diff_order,
                    double factor);
int cgk_cic_indices(cg_ctx *c, const double *pos, i64 n, int for_gather, i64 *idx);
int cgk_transpose_fourier(cg_ctx *c, const double *src, double *dst);
int cgk_emigrant_dest(cg_ctx *c, const double *pos, const double *mom, const i64 *idx,
                      const unsigned *count, i64 cap, double dtm, int *dest, int *send_counts);
int cgk_layers_write(cg_ctx *c, i64 layer0, i64 nlayers, const double *src, int add);
int cgk_owner_rank(cg_ctx *c, const double *pos, i64 n, int *owner);

// ---- cg_general.hip: the general particle_mesh() pieces ----
int cgk_copy_modes_pack(cg_ctx *from, i64 n_small, const int *rows_local, i64 n_rows, double *out);
int cgk_copy_modes_unpack(cg_ctx *onto, cg_ctx *from, i64 n_small, const int *rows_local,
                          i64 n_rows, const double *in, int deconv_order, int nlattice,
                          const double *shift, int op_add);
int cgk_fluid_add(cg_ctx *c, const double *fluid, double factor, int op_add);
int cgk_nullify_nyquist(cg_ctx *c);
int cgk_fourier_operate(cg_ctx *onto, cg_ctx *from, int deconv_order, int nlattice,
                        const double *shift, int diff_dim, int op_add);
int cgk_copy_modes(cg_ctx *onto, cg_ctx *from, int deconv_order, int nlattice,
                   const double *shift, int op_add);
int cgk_deposit_general(cg_ctx *c, const double *pos, i64 n, double contribution, int order,
                        const CicGeom &geo);
int cgk_gather_scalar(cg_ctx *c, const double *pos, double *mom, i64 n, int dim, int order,
                      const CicGeom &geo, double factor);
int cgk_mesh_diff(cg_ctx *dst, cg_ctx *src, int dim, int diff_order);
int cgk_fluid_kick(cg_ctx *c, double *J, const double *rho, const double *P, int dim,
                   int diff_order, double minus_dt, double inv_c2);

// ---- cg_fft.hip: the hand-written FFT ----
// the single-domain solve: Solve = forward + Poisson kernel + backward with the x pass fused
enum class FftOp { Forward, Backward, Solve };
// its pieces on x-slab domains, around the two transposes (also of the rocFFT backend,
// cg_rocfft.hip): z and y of owned layers into / out of the transpose buffer, x on that buffer
enum class SlabOp { ZYForward, XSolve, XForward, XBackward, ZYBackward };
bool cgk_fft_supported(i64 N);
int cgk_fft(cg_ctx *c, FftOp op, int deconv_order, double C, int long_range, double E);
// layers [layer0, layer0 + nlayers) of the owned ones (nlayers < 0: from layer0 on) for the ZY
// pieces; deconv_order, C, long_range, E for XSolve
int cgk_fft_dist(cg_ctx *c, SlabOp op, double2 *buf, int deconv_order, double C, int long_range,
                 double E, i64 layer0, i64 nlayers);

// ---- cg_rocfft.hip: the rocFFT backend ----
// init: the library's set-up, once, and the backend of a context that is not custom_fft (on a
// single domain with its 3-D plans); the transforms are those of cgk_fft and cgk_fft_dist
int cgk_libfft_init(cg_ctx *c);
void cgk_libfft_destroy(cg_ctx *c);
int cgk_libfft(cg_ctx *c, FftOp op, int deconv_order, double C, int long_range, double E);
int cgk_libfft_dist(cg_ctx *c, SlabOp op, double2 *buf, int deconv_order, double C,
                    int long_range, double E, i64 layer0, i64 nlayers);

// ---- cg_particles.hip: drift, tile sort, regions ----
// out[i] = in[0] + ... + in[i-1] for i < n, on c->stream (temporary storage: c->scan_tmp)
int cg_exclusive_sum(cg_ctx *c, const unsigned *in, unsigned *out, i64 n);
int cgk_drift(cg_ctx *c, double *pos, const double *mom, i64 n, double dt_over_mass);
int cgk_measure_mom(cg_ctx *c, const double *mom, i64 n, double *out, double *scratch);
int cgk_measure_mom_regions(cg_ctx *c, const double *mom, const unsigned *start,
                            const unsigned *count, double *out, double *scratch);
int cgk_sort(cg_ctx *c, const double *pos_in, const double *mom_in, const i64 *ids_in,
             double *pos_out, double *mom_out, i64 *ids_out, i64 n, unsigned *tile_offset_out,
             int drift, double dt_over_mass, int use_prepared);
int cgk_permute_rows(cg_ctx *c, const i64 *perm, i64 n, int ncols, const void *const *src,
                     void *const *dst, const int *row_bytes);
int cgk_owner_rank_drifted(cg_ctx *c, const double *pos, const double *mom, i64 n, double dtm,
                           int *owner);
int cgk_prepare_rebind(cg_ctx *c, const double *pos, const double *mom, i64 n_total,
                       const double *add_pos, const double *add_mom, i64 n_add);
int cgk_predict_regions(cg_ctx *c, const unsigned *start_in, const unsigned *count_in,
                        unsigned *start_out);
int cgk_emigrant_rows_dest(cg_ctx *c, const double *rows, const unsigned *count, i64 cap,
                           int *dest, int *send_counts);
int cgk_region_insert(cg_ctx *c, const double *rows, i64 m, const unsigned *start,
                      unsigned *count, double *pos_out, double *mom_out, i64 *ids_out,
                      i64 *aux_out, i64 capacity);

// ---- cg_tiled_kernels.hip: the LDS-tiled deposit and the fused particle pass ----
int cgk_deposit_cic_tiled(cg_ctx *c, const double *pos, i64 n, const unsigned *tile_offset,
                          const unsigned *count, double contribution, int accumulate);
// output side of the fused kick + drift + scatter (cg_gather_kick_drift_scatter)
struct FusedScatter {
    const unsigned *count_in;  // populations of the input regions (null: dense tile order)
    const unsigned *start_out;
    unsigned *count_out;
    double *pos_out, *mom_out;
    const i64 *ids_in;
    i64 *ids_out;
    const i64 *aux_in;
    i64 *aux_out;
    i64 out_capacity;
};
int cgk_gather_kick_tiled(cg_ctx *c, const double *pos, double *mom, i64 n,
                          const unsigned *tile_offset, int diff_order, double factor,
                          int prepare, double next_dtm, const FusedScatter *fs = nullptr);
// workgroup -> tile for the kernels that give a tile to a workgroup
int cgk_tile_order(cg_ctx *c, const unsigned *start, const unsigned *count);

// ---- cg_shortrange.hip: cell list and the cells sweep ----
int cgk_shortrange_cells(cg_ctx *c, const double *pos, i64 n, i64 nt, double tile_extent,
                         unsigned *order, unsigned *offset, double *pos_sorted,
                         const signed char *rung, const signed char *rung_jumped,
                         int lowest_active, unsigned *nact, signed char *rj_sorted);
int cgk_shortrange_sparse(cg_ctx *c, const double *pos_r, const i64 *active, int K, double *dmom_r,
                          const double *pos_s, i64 n_s, const double *table,
                          double r2_index_scaling, double r2_max, double factor,
                          const double *factors, const signed char *rung_jumped);
int cgk_shortrange_sweep_cells(cg_ctx *c, const double *pos_r_sorted, const unsigned *order_r,
                               const unsigned *off_r, double *dmom_r, const double *pos_s_sorted,
                               const unsigned *off_s, i64 nt, const double *table,
                               double r2_index_scaling, double r2_max, double factor,
                               const double *factors, const signed char *rung,
                               const signed char *rung_jumped, int lowest_active,
                               const unsigned *nact_r, const signed char *rj_sorted_r,
                               i64 n_active_max);

// ---- cg_shortrange_dense.hip: tile lists and the dense tiles' sweep ----
int cgk_shortrange_dense(cg_ctx *c, const double *pos_r_sorted, const unsigned *order_r,
                         const unsigned *off_r, double *dmom_r, const double *pos_s_sorted,
                         const unsigned *off_s, i64 nt, const double *table,
                         double r2_index_scaling, double r2_max, double factor,
                         const double *factors, const signed char *rung,
                         const signed char *rung_jumped, int lowest_active,
                         const unsigned char *active_in, const unsigned char **take_out);
int cgk_shortrange_tiles_phase(cg_ctx *c, int phase, const double *pos, i64 n, i64 nt,
                               double tile_extent, const signed char *rung, int lowest_active,
                               unsigned *order, unsigned *offset, double *pos_sorted,
                               i64 sub_min, i64 sub_rows);
int cgk_shortrange_dense_join(cg_ctx *c);
int cgk_shortrange_dense_look(cg_ctx *c, const unsigned *off_cells, i64 nt);
int cgk_shortrange_tiles(cg_ctx *c, const double *pos, i64 n, i64 nt, double tile_extent,
                         const signed char *rung, int lowest_active, unsigned *order,
                         unsigned *offset, double *pos_sorted);

// ---- cg_rungs.hip: rungs and the sub-step passes ----
int cgk_dmom_active(cg_ctx *c, double *mom, double *dmom, const signed char *rung, i64 n,
                    int lowest_active, int op);
int cgk_dmom_to_acc(cg_ctx *c, double *dmom, const signed char *rung,
                    const signed char *rung_jumped, i64 n, int lowest_active, const double *conv,
                    int any_jumps);
int cgk_assign_rungs(cg_ctx *c, const double *dmom, signed char *rung, signed char *rung_jumped,
                     i64 n, double rung_factor, int N_rungs);
int cgk_flag_rung_jumps(cg_ctx *c, const double *dmom, const signed char *rung,
                        signed char *rung_jumped, i64 n, int lowest_active,
                        const double *integrals, double rf_up, double rf_down, int N_rungs,
                        int *any_out);
int cgk_apply_rung_jumps(cg_ctx *c, signed char *rung, signed char *rung_jumped, i64 n,
                         int N_rungs);
// (3 N_rungs - 1 entries of a rung table passed to a kernel by value)
#define CG_RUNG_TABLE_MAX 64
int cgk_substep_begin(cg_ctx *c, double *pos, const double *mom, double *dmom,
                      const signed char *rung, signed char *rung_jumped, i64 n, int do_drift,
                      double dt_over_mass, int do_flag, int lowest_active,
                      const double *integrals_1, double rf_up, double rf_down, int N_rungs,
                      int *any_out, long long *counts_after, int defer);
int cgk_substep_flush(cg_ctx *c);
// The gate.  A context remembers two things about particle arrays it does not own: a deferred
// sub-step pass (sub_pending) and a drift histogram prepared for one pos/mom pair (prep_valid).
// Every extern "C" entry that takes live particle arrays (pos, mom, Δmom, rungs, ids, rows of
// particles) begins with exactly one of these lines and holds no flush or invalidation of its own
// (tests/test_particle_gate_host.py reads the sources for it); a new entry picks its kind:
//   CG_READS_PARTICLES   launches a pending pass first.  Writing Δmom, rungs or arrays of the
//                        entry's own leaves the histogram alone: it depends on pos, mom and dt only.
//   CG_WRITES_PARTICLES  the same, and pos or mom change: the prepared histogram is void.
//   CG_ADOPTS_PENDING_PASS  cg_shortrange_cells[_rungs] only, and on purpose no flush here:
//                        cgk_shortrange_cells takes a pending pass over the same pos and n into its
//                        counting pass and flushes any other itself.
//   CG_WHOLE_CONTEXT     cg_set_stream, cg_synchronize: what was deferred runs before the stream
//                        changes or is waited for.  (cg_destroy drops a pending pass.)
// A null context passes: the entry's own check reports it under the entry's name.
inline int cg_particle_gate(cg_ctx *c, bool writes) {
    if (!c) return 0;
    if (writes) c->prep_valid = false;
    return cgk_substep_flush(c);
}
#define CG_WRITES_PARTICLES_IF(c, writes)                    \
    do {                                                     \
        if (cg_particle_gate((c), (writes))) return 1;       \
    } while (0)
#define CG_READS_PARTICLES(c) CG_WRITES_PARTICLES_IF(c, false)
#define CG_WRITES_PARTICLES(c) CG_WRITES_PARTICLES_IF(c, true)
#define CG_WHOLE_CONTEXT(c) CG_WRITES_PARTICLES_IF(c, false)
#define CG_ADOPTS_PENDING_PASS(c) ((void)(c))
int cgk_substep_partial(cg_ctx *c, i64 n, i64 per, int N_rungs, i64 *nwg_out);
int cgk_substep_populations(cg_ctx *c, i64 nwg, int N_rungs, long long *counts);
int cgk_substep_end(cg_ctx *c, double *mom, double *dmom, signed char *rung,
                    signed char *rung_jumped, i64 n, int do_apply, int lowest_active,
                    const double *conversion_factors, int N_rungs, long long *counts);
int cgk_rung_populations(cg_ctx *c, const signed char *rung, i64 n, int N_rungs, long long *counts);

// ---- cg_pp.hip: direct summation ----
int cgk_ewald_tabulate(cg_ctx *c, int gridsize, double *grid);
int cgk_pp_kick(cg_ctx *c, const double *pos_r, i64 n_r, double *dmom_r, const double *pos_s,
                i64 n_s, int same, const double *ewald_grid, int ewald_gridsize,
                double softening, int kernel, double factor, const double *factors,
                const signed char *rung, const signed char *rung_jumped, int lowest_active);
