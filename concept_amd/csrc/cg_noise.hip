// cg_noise.hip — the primordial noise on the device, from the reference's own random streams.
//   k_noise_generate   generate_primordial_noise, 'distributed' scheme   ic.py:928-1163
// numpy's Generator draws the noise in the reference: Rayleigh amplitudes sqrt(2 E) with E from
// the ziggurat of random_standard_exponential, phases from uniform doubles, PCG64DXSM underneath.
// A stream is sequential on the host; here it is not:
//   raw words   PCG64DXSM steps state' = a*state + inc (128 bits) and puts out a hash of the state
//               before the step, so word k of a stream is the hash of a^k*state + S_k*inc with
//               S_k = 1 + a + ... + a^(k-1): thread p of a trip holds (a^p, S_p) of the jump-ahead
//               table in registers and the trip's first state is wave-uniform.
//   ziggurat    a draw takes one word when it is fast (ri < ke[idx], about 98 %), else a second word
//               as the uniform number of the tail (idx = 0) or of the wedge test, and where that
//               test fails it starts again after the two.  Whether a word starts a draw follows
//               s_0 = 1, s_(p+1) = !(s_p && slow_p), slow_p what word p would be as a start: 1
//               after a fast word, alternating inside a run of slow words.  A wave gets its flags
//               from the ballot of slow_p, the waves of a trip chain through LDS, the trips
//               through a carry.  A slow draw is finished by the thread of its SECOND word (it
//               reads the first from LDS), so every thread needs its own word only, and the trip's
//               last word is carried to the next trip's thread 0.
//   order       the emitting threads' prefix count is the draw's number in the stream; the
//               amplitudes of a trip are compacted in LDS by it, so that in the phase part thread
//               q has draw count + q: its amplitude from LDS, its phase word by the jump-ahead
//               table from the phase state at draw `count`.
// One workgroup of kTrip threads per spawn key; a last workgroup zeroes the slice kj = -N/2.
// Every element of the view is written exactly once (see cg_noise_generate, concept_gpu.h).
// Compiled with -ffp-contract=off.  FP64 and 64-bit integers throughout; no atomics.
#include "cg_internal.h"

#define CG_ZIG_TABLE static __device__ const
#include "cg_ziggurat_tables.h"

namespace {

typedef unsigned long long u64;

constexpr int kTrip = 1024;  // raw words per trip = threads of a workgroup
constexpr int kWaves = kTrip / 64;
constexpr u64 kMultiplier = 0xda942042e4dd58b5ull;  // PCG_CHEAP_MULTIPLIER_128
const double kPi = 3.141592653589793;               // float(np.pi), commons.py:1816

struct U128 {
    u64 lo, hi;
};
__device__ __forceinline__ U128 load128(const u64 *p) { return U128{p[0], p[1]}; }
// a*b + c*d mod 2^128
__device__ __forceinline__ U128 mul_add128(U128 a, U128 b, U128 c, U128 d) {
    const u64 ab_lo = a.lo * b.lo, cd_lo = c.lo * d.lo;
    const u64 ab_hi = __umul64hi(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo;
    const u64 cd_hi = __umul64hi(c.lo, d.lo) + c.lo * d.hi + c.hi * d.lo;
    U128 r;
    r.lo = ab_lo + cd_lo;
    r.hi = ab_hi + cd_hi + (r.lo < ab_lo ? 1 : 0);
    return r;
}
// the output of PCG64DXSM for the state before its step (pcg_cm_random_r)
__device__ __forceinline__ u64 dxsm(U128 s) {
    u64 hi = s.hi;
    const u64 lo = s.lo | 1;
    hi ^= hi >> 32;
    hi *= kMultiplier;
    hi ^= hi >> 48;
    hi *= lo;
    return hi;
}
// next_double: 53 bits
__device__ __forceinline__ double to_double(u64 w) {
    return (double)(w >> 11) * (1.0 / 9007199254740992.0);
}

// s_lane of a wave from the ballot of slow_p and the flag s_in of its lane 0: r slow lanes stand
// right before `lane` (after a fast one, whose successor starts a draw): s = r even.  Where the
// run reaches lane 0 it goes on with s_in: as if one more slow start stood in front when !s_in.
// lane = 64 gives the flag of the next wave's lane 0.
__device__ __forceinline__ bool start_flag(u64 slow, int lane, bool s_in) {
    const u64 below = lane >= 64 ? ~0ull : ((1ull << lane) - 1);
    const u64 fast_below = ~slow & below;
    const int r = fast_below ? lane - 1 - (63 - __clzll((long long)fast_below))
                             : lane + (s_in ? 0 : 1);
    return !(r & 1);
}

struct NoiseArgs {
    double2 *four;
    i64 f_si, cp;
    int N, n_keys, n_slice, fixed;
    const u64 *streams, *jump;
    const int2 *order;
    double phase_shift, scale;
};

__global__ __launch_bounds__(kTrip) void k_noise_generate(NoiseArgs P) {
#pragma clang fp contract(off)
    __shared__ u64 s_ke[256];
    __shared__ double s_we[256], s_fe[256];
    __shared__ u64 s_word[kTrip];
    __shared__ double s_amp[kTrip];
    __shared__ u64 s_slow[kWaves];
    __shared__ int s_emitted[kWaves];
    const int p = threadIdx.x, lane = p & 63, wave = p >> 6;
    const int N = P.N, nyq = N / 2;
    const i64 cp = P.cp;
    const double2 zero = make_double2(0.0, 0.0);

    if ((int)blockIdx.x == P.n_keys) {  // the slice kj = -nyquist: no stream draws it
        for (i64 e = p; e < N * cp; e += kTrip) {
            const i64 a = e / cp;
            P.four[a * P.f_si + nyq * cp + (e - a * cp)] = zero;
        }
        return;
    }
    const int kappa = (int)blockIdx.x - (nyq - 1);
    const int b = kappa < 0 ? kappa + N : kappa;        // kappa mod N
    const int b_conj = kappa > 0 ? N - kappa : -kappa;  // -kappa mod N
    // what no draw of any key writes in this slice: the row ki = -nyquist, and in every other row
    // the plane kk = nyquist with the row padding behind it
    double2 *slice = P.four + b * cp;
    for (i64 kk = p; kk < cp; kk += kTrip) slice[nyq * P.f_si + kk] = zero;
    const i64 tail = cp - nyq;
    for (i64 e = p; e < N * tail; e += kTrip) {
        const i64 a = e / tail;
        if (a != nyq) slice[a * P.f_si + nyq + (e - a * tail)] = zero;
    }

    const u64 *stream = P.streams + 8 * (i64)blockIdx.x;
    U128 amp_state = load128(stream), amp_inc = load128(stream + 2);
    U128 phase_state = load128(stream + 4);
    const U128 phase_inc = load128(stream + 6);
    const U128 jump_a = load128(P.jump + 4 * p), jump_s = load128(P.jump + 4 * p + 2);
    const U128 trip_a = load128(P.jump + 4 * kTrip), trip_s = load128(P.jump + 4 * kTrip + 2);
    if (!P.fixed) {
        if (p < 256) {
            s_ke[p] = cg_zig_ke_double[p];
            s_we[p] = __longlong_as_double((long long)cg_zig_we_double[p]);
            s_fe[p] = __longlong_as_double((long long)cg_zig_fe_double[p]);
        }
        __syncthreads();
    }

    int count = 0;          // draws made so far: the number of the next one
    bool carry = false;     // the trip's first word is the second word of a slow draw ...
    u64 carry_word = 0;     // ... whose first word this is
    while (count < P.n_slice) {
        int n_out = kTrip;
        if (!P.fixed) {
            const u64 w = dxsm(mul_add128(jump_a, amp_state, jump_s, amp_inc));
            u64 ri = w >> 3;
            const int idx = (int)(ri & 0xff);
            ri >>= 8;
            const bool slow = !(ri < s_ke[idx]);
            s_word[p] = w;
            const u64 slow_mask = __ballot(slow);
            if (lane == 0) s_slow[wave] = slow_mask;
            __syncthreads();
            // the flag of lane 0 of every wave in turn; after the last, of the next trip
            bool s_in = !carry, s_mine = s_in;
            for (int v = 0; v < kWaves; v++) {
                if (v == wave) s_mine = s_in;
                s_in = start_flag(s_slow[v], 64, s_in);
            }
            bool emit = false;
            double E = 0.0;
            if (start_flag(slow_mask, lane, s_mine)) {
                if (!slow) {  // random_standard_exponential: the first return
                    emit = true;
                    E = (double)ri * s_we[idx];
                }
            } else {  // standard_exponential_unlikely of the draw that started one word back
                const u64 first = p ? s_word[p - 1] : carry_word;
                u64 ri1 = first >> 3;
                const int idx1 = (int)(ri1 & 0xff);
                ri1 >>= 8;
                const double x = (double)ri1 * s_we[idx1];
                const double U = to_double(w);
                if (idx1 == 0) {
                    emit = true;
                    E = 7.69711747013104972 - log1p(-U);  // ziggurat_exp_r
                } else if ((s_fe[idx1 - 1] - s_fe[idx1]) * U + s_fe[idx1] < exp(-x)) {
                    emit = true;
                    E = x;
                }
            }
            const u64 emit_mask = __ballot(emit);
            if (lane == 0) s_emitted[wave] = __popcll(emit_mask);
            carry = !s_in;
            carry_word = s_word[kTrip - 1];
            __syncthreads();
            int before = 0;
            n_out = 0;
            for (int v = 0; v < kWaves; v++) {
                const int c = s_emitted[v];
                if (v < wave) before += c;
                n_out += c;
            }
            if (emit) s_amp[before + __popcll(emit_mask & ((1ull << lane) - 1))] = E;
            amp_state = mul_add128(trip_a, amp_state, trip_s, amp_inc);
            __syncthreads();
        }
        const int t = count + p;
        if (p < n_out && t < P.n_slice) {
            const double U = to_double(dxsm(mul_add128(jump_a, phase_state, jump_s, phase_inc)));
            double theta = -kPi + U * (kPi - (-kPi));  // uniform(-π, π)
            if (P.phase_shift != 0) theta = theta + P.phase_shift;
            // rayleigh(1)·scale: mode·sqrt(2.0·E) with mode 1, then the scale 1/√2
            const double r = P.fixed ? 1.0 : sqrt(2.0 * s_amp[p]) * P.scale;
            double re = r * cos(theta), im = r * sin(theta);
            const int2 point = P.order[t];
            const int ki = point.x, kk = point.y;
            if (ki > -nyq && ki < nyq && kk >= 0 && kk < nyq) {
                if (kk != 0 || ki < 0 || (ki == 0 && kappa < 0))
                    slice[(i64)(ki < 0 ? ki + N : ki) * P.f_si + kk] = make_double2(re, im);
                if (kk == 0 && !(ki > 0 || (ki == 0 && kappa > 0))) {
                    if (ki == 0 && kappa == 0) re = im = 0.0;  // nullify_modes(slab, 'origin')
                    P.four[(i64)(ki < 0 ? -ki : 0) * P.f_si + b_conj * cp] = make_double2(re, -im);
                }
            }
        }
        // the phase stream moves on by the draws made (n_out <= kTrip rows of the table)
        phase_state = mul_add128(load128(P.jump + 4 * n_out), phase_state,
                                 load128(P.jump + 4 * n_out + 2), phase_inc);
        count += n_out;
        // no barrier here: the next trip writes s_word and s_slow before its first barrier, and
        // they were last read before the second barrier of this trip; s_emitted and s_amp are
        // written after the next trip's first barrier, which every thread reaches after its reads
    }
}

}  // namespace

extern "C" int cg_noise_trip(void) { return kTrip; }

extern "C" int cg_noise_generate(cg_ctx *mesh, const uint64_t *streams, int64_t n_keys,
                                 const int32_t *order, int64_t n_slice, const uint64_t *jump,
                                 int64_t n_jump, int fixed_amplitude, double phase_shift) {
    CG_CHECK(mesh, "cg_noise_generate: null context");
    CG_CHECK(mesh->four != nullptr,
             "cg_noise_generate: no Fourier buffer bound (cg_dist_bind_fourier)");
    CG_CHECK(mesh->p.nprocs == 1 && mesh->f_j0 == 0 && mesh->f_nj == mesh->N,
             "cg_noise_generate: single-domain entry point");
    const i64 N = mesh->N;
    CG_CHECK(N >= 2 && N % 2 == 0, "cg_noise_generate: grid size %lld is not even", (long long)N);
    CG_CHECK(N * N < ((i64)1 << 31), "cg_noise_generate: %lld rows", (long long)(N * N));
    CG_CHECK(streams && order && jump, "cg_noise_generate: null table");
    CG_CHECK(n_keys == N - 1, "cg_noise_generate: %lld spawn keys for grid size %lld, which has %lld",
             (long long)n_keys, (long long)N, (long long)(N - 1));
    CG_CHECK(n_slice == (N - 1) * N / 2,
             "cg_noise_generate: %lld points per slice for grid size %lld, which has %lld",
             (long long)n_slice, (long long)N, (long long)((N - 1) * N / 2));
    CG_CHECK(n_jump == kTrip + 1, "cg_noise_generate: a jump-ahead table of %lld rows, %d needed",
             (long long)n_jump, kTrip + 1);
    CG_CHECK(mesh->pad / 2 > N / 2, "cg_noise_generate: row pitch %lld", (long long)mesh->pad);
    NoiseArgs P{};
    P.four = mesh->four;
    P.f_si = mesh->f_si;
    P.cp = mesh->pad / 2;
    P.N = (int)N;
    P.n_keys = (int)n_keys;
    P.n_slice = (int)n_slice;
    P.fixed = fixed_amplitude != 0;
    P.streams = (const u64 *)streams;
    P.jump = (const u64 *)jump;
    P.order = (const int2 *)order;
    P.phase_shift = phase_shift;
    P.scale = 1.0 / sqrt(2.0);  // rayleigh(1/sqrt(2)), ic.py:1114
    hipLaunchKernelGGL(k_noise_generate, dim3((unsigned)n_keys + 1), dim3(kTrip), 0, mesh->stream,
                       P);
    CG_LAUNCH_CHECK();
    return 0;
}
