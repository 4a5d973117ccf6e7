// cg_rocfft.hip — the rocFFT backend: every plan, the execution info, the work buffer and every
// call of the library, for grids that are not a power of two (the reference accepts any size
// divisible by the decomposition, communication.py:692-741, mesh.py:1898-1905; its own tests use
// 24 and 36) and, with CONCEPT_GPU_FFT=rocfft, for every grid.  MI355X / gfx950 only.
// Single domain: the in-place 3-D real transforms of the mesh, planned with the context.
// x-slab domains: the same stages and the same transpose-buffer layout as the hand-written path
// (cg_fft.hip fft_dist): 2-D real transforms of the owned layers, rows packed by destination
// domain, all-to-all (the caller's), 1-D transforms along x on complex[N][JB + 1][cp], and back.
// The pack / unpack is a pass of its own here (the hand-written y pass writes the blocked layout
// directly).  These plans are made on first use.  The layouts are those of cg_rocfft_layout.h.
#include <rocfft/rocfft.h>

#include <array>
#include <map>

#include "cg_internal.h"
#include "cg_rocfft_layout.h"

#define CG_FFT(call)                                                                          \
    do {                                                                                      \
        rocfft_status s_ = (call);                                                            \
        if (s_ != rocfft_status_success) {                                                    \
            cg_set_error("%s failed: rocfft status %d (%s:%d)", #call, (int)s_, __FILE__,     \
                         __LINE__);                                                           \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

// plans are indexed [inverse]; all of them share the one execution info and the one work buffer
struct RocfftBackend {
    rocfft_plan mesh3d[2] = {nullptr, nullptr};  // single domain
    // z and y of a slab's layers by number of layers; a null plan: rocFFT did not make it, the
    // layers take the 1-D plans
    std::map<i64, std::array<rocfft_plan, 2>> layers2d;
    // one layer in two steps: z along the rows (r2c / c2r in place), y along the columns kk
    rocfft_plan z1[2] = {nullptr, nullptr}, y1[2] = {nullptr, nullptr};
    rocfft_plan x1[2] = {nullptr, nullptr};  // x on the transpose buffer
    rocfft_execution_info info = nullptr;
    cg_buf<void> work;
};

// The plan of a layout.  may_refuse: a plan rocFFT does not make comes back null instead of as an
// error (only the 2-D layer plans: the in-place inverse one at 16 and 64 points in rows of N + 16
// doubles answers rocfft_status_failure, and such layers are transformed by the 1-D pair).
static int make_plan(const RocfftLayout &l, bool may_refuse, rocfft_plan *plan) {
    static const rocfft_transform_type types[4] = {
        rocfft_transform_type_real_forward, rocfft_transform_type_real_inverse,
        rocfft_transform_type_complex_forward, rocfft_transform_type_complex_inverse};
    rocfft_array_type in = rocfft_array_type_complex_interleaved, out = in;
    if (l.kind == RocfftKind::RealForward)
        in = rocfft_array_type_real, out = rocfft_array_type_hermitian_interleaved;
    if (l.kind == RocfftKind::RealInverse)
        in = rocfft_array_type_hermitian_interleaved, out = rocfft_array_type_real;
    size_t off[1] = {0};
    *plan = nullptr;
    rocfft_plan_description d = nullptr;
    CG_FFT(rocfft_plan_description_create(&d));
    rocfft_status s = rocfft_plan_description_set_data_layout(
        d, in, out, off, off, l.dims, l.in_stride, l.in_dist, l.dims, l.out_stride, l.out_dist);
    const bool described = s == rocfft_status_success;
    if (described)
        s = rocfft_plan_create(plan, rocfft_placement_inplace, types[(int)l.kind],
                               rocfft_precision_double, l.dims, l.lengths, l.batch, d);
    CG_FFT(rocfft_plan_description_destroy(d));
    if (s == rocfft_status_success) return 0;
    *plan = nullptr;
    if (described && may_refuse) return 0;
    cg_set_error("rocFFT backend: %s of a %d-D plan of %zu points, batch %zu, failed: rocfft "
                 "status %d", described ? "rocfft_plan_create" : "the data layout", (int)l.dims,
                 l.lengths[0], l.batch, (int)s);
    return 1;
}

// `plan` in place on `buf`, on the context's stream, with the work buffer grown to its need
static int execute(cg_ctx *c, rocfft_plan plan, void *buf) {
    RocfftBackend *b = c->libfft;
    size_t w = 0;
    CG_FFT(rocfft_plan_get_work_buffer_size(plan, &w));
    if (b->work.reserve(c, w)) return 1;
    if (!b->info) CG_FFT(rocfft_execution_info_create(&b->info));
    if (b->work.bytes)
        CG_FFT(rocfft_execution_info_set_work_buffer(b->info, b->work, b->work.bytes));
    CG_FFT(rocfft_execution_info_set_stream(b->info, c->stream));
    void *io[1] = {buf};
    CG_FFT(rocfft_execute(plan, io, nullptr, b->info));
    return 0;
}

int cgk_libfft_init(cg_ctx *c) {
    static bool ready = false;
    if (!ready) {
        CG_FFT(rocfft_setup());
        ready = true;
    }
    if (c->custom_fft) return 0;
    RocfftBackend *b = c->libfft = new RocfftBackend();
    if (c->p.nprocs > 1) return 0;  // (x-slab domains: plans made on first use)
    size_t work = 0;
    for (int inv = 0; inv < 2; inv++) {
        size_t w = 0;
        if (make_plan(fft_layout_3d(inv, c->N, c->ny, c->pad), false, &b->mesh3d[inv])) return 1;
        CG_FFT(rocfft_plan_get_work_buffer_size(b->mesh3d[inv], &w));
        work = w > work ? w : work;
    }
    if (b->work.reserve(c, work)) return 1;
    c->device_bytes += (i64)work;
    return 0;
}

// every plan, then the execution info, then (with the struct) the work buffer
void cgk_libfft_destroy(cg_ctx *c) {
    RocfftBackend *b = c->libfft;
    if (!b) return;
    for (auto &kv : b->layers2d)
        for (rocfft_plan p : kv.second)
            if (p) rocfft_plan_destroy(p);
    for (rocfft_plan *set : {b->mesh3d, b->z1, b->y1, b->x1})
        for (int inv = 0; inv < 2; inv++)
            if (set[inv]) rocfft_plan_destroy(set[inv]);
    if (b->info) rocfft_execution_info_destroy(b->info);
    delete b;
    c->libfft = nullptr;
}

int cgk_libfft(cg_ctx *c, FftOp op, int deconv_order, double C, int long_range, double E) {
    RocfftBackend *b = c->libfft;
    if (op != FftOp::Backward && execute(c, b->mesh3d[0], c->mesh)) return 1;
    if (op == FftOp::Solve && cgk_kspace(c, deconv_order, C, long_range, E)) return 1;
    if (op != FftOp::Forward && execute(c, b->mesh3d[1], c->mesh)) return 1;
    return 0;
}

// ---- x-slab domains ----
// the 2-D plans of `nlayers` layers, made on first use (null on an error)
static const std::array<rocfft_plan, 2> *plans_2d(cg_ctx *c, i64 nlayers) {
    auto &m = c->libfft->layers2d;
    auto it = m.find(nlayers);
    if (it != m.end()) return &it->second;
    std::array<rocfft_plan, 2> p{};
    for (int inv = 0; inv < 2; inv++)
        if (make_plan(fft_layout_2d(inv, c->N, c->ny, c->pad, nlayers), true, &p[inv])) {
            if (p[0]) rocfft_plan_destroy(p[0]);
            return nullptr;
        }
    return &m.emplace(nlayers, p).first->second;
}

// The 2-D transform of the layers [layer0, layer0 + nlayers) in two 1-D steps per layer, for
// the sizes whose 2-D plan rocFFT does not make: z on the N rows of a layer, y on its columns
// kk <= N/2.  Forward z then y, inverse y then z; unnormalised like the 2-D plans.
static int layers_1d(cg_ctx *c, bool inverse, i64 layer0, i64 nlayers) {
    RocfftBackend *b = c->libfft;
    const int inv = inverse;
    if (!b->z1[inv] && (make_plan(fft_layout_z_rows(inverse, c->N, c->pad), false, &b->z1[inv]) ||
                        make_plan(fft_layout_y_columns(inverse, c->N, c->pad), false, &b->y1[inv])))
        return 1;
    for (i64 l = layer0; l < layer0 + nlayers; l++)
        for (int step = 0; step < 2; step++)
            if (execute(c, (step == 0) != inverse ? b->z1[inv] : b->y1[inv],
                        c->mesh0 + l * c->ny * c->pad))
                return 1;
    return 0;
}

// rows j of the layers [layer0, layer0 + nlayers) between the slab's Fourier layout
// complex[layer][ny][cp] and the transpose buffer blocked by destination domain
// buf[q = j / JB][layer][j - q JB][cp] (JB + 1 rows per layer)
template <bool PACK>
__global__ __launch_bounds__(256) void k_dist_rows(double2 *__restrict__ slab,
                                                   double2 *__restrict__ buf, i64 N, i64 ny,
                                                   i64 cp, i64 nxl, i64 JB, i64 layer0) {
    const i64 row = blockIdx.x;  // (layer - layer0) * N + j
    const i64 l = layer0 + row / N, j = row % N, q = j / JB;
    double2 *a = slab + (l * ny + j) * cp;
    double2 *b = buf + ((q * nxl + l) * (JB + 1) + (j - q * JB)) * cp;
    for (i64 kk = threadIdx.x; kk < N / 2 + 1; kk += blockDim.x) {
        if (PACK) b[kk] = a[kk];
        else a[kk] = b[kk];
    }
}

// one piece of the slab transform (the pieces of cgk_fft_dist)
int cgk_libfft_dist(cg_ctx *c, SlabOp op, double2 *buf, int deconv_order, double C, int long_range,
                    double E, i64 layer0, i64 nlayers) {
    RocfftBackend *b = c->libfft;
    const i64 cp = c->pad / 2, N = c->N, nxl = c->xmap.nxl, JB = N / c->p.nprocs;
    if (nlayers < 0) nlayers = nxl - layer0;
    double2 *m = (double2 *)c->mesh0;
    if (op == SlabOp::ZYForward || op == SlabOp::ZYBackward) {
        const bool inverse = op == SlabOp::ZYBackward;
        const auto *plans = plans_2d(c, nlayers);
        if (!plans) return 1;
        const rocfft_plan plan = (*plans)[inverse];
        if (inverse)
            hipLaunchKernelGGL((k_dist_rows<false>), dim3((unsigned)(nlayers * N)), dim3(256), 0,
                               c->stream, m, buf, N, c->ny, cp, nxl, JB, layer0);
        if (plan ? execute(c, plan, m + layer0 * c->ny * cp)
                 : layers_1d(c, inverse, layer0, nlayers))
            return 1;
        if (!inverse)
            hipLaunchKernelGGL((k_dist_rows<true>), dim3((unsigned)(nlayers * N)), dim3(256), 0,
                               c->stream, m, buf, N, c->ny, cp, nxl, JB, layer0);
        hipError_t e_ = hipGetLastError();
        if (e_ != hipSuccess) {
            cg_set_error("cg_dist_fft (rocFFT backend): pack / unpack launch failed: %s",
                         hipGetErrorString(e_));
            return 1;
        }
        return 0;
    }
    for (int inv = 0; inv < 2; inv++)
        if (!b->x1[inv] &&
            make_plan(fft_layout_x(inv, N, c->pad, c->p.nprocs), false, &b->x1[inv]))
            return 1;
    if ((op == SlabOp::XSolve || op == SlabOp::XForward) && execute(c, b->x1[0], buf)) return 1;
    if (op == SlabOp::XSolve) {
        // the Poisson / deconvolution kernel on the rows of this domain (the Fourier view of
        // cg_dist_bind_fourier, for the duration of the call on `buf`)
        double2 *four = c->four;
        const i64 f_si = c->f_si;
        const int f_j0 = c->f_j0, f_nj = c->f_nj;
        c->four = buf;
        c->f_si = (JB + 1) * cp;
        c->f_j0 = (int)(JB * c->p.rank);
        c->f_nj = (int)JB;
        int rc = cgk_kspace(c, deconv_order, C, long_range, E);
        c->four = four, c->f_si = f_si, c->f_j0 = f_j0, c->f_nj = f_nj;
        if (rc) return rc;
    }
    if ((op == SlabOp::XSolve || op == SlabOp::XBackward) && execute(c, b->x1[1], buf)) return 1;
    return 0;
}
