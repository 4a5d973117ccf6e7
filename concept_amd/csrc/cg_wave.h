// cg_wave.h — the wave-level and workgroup-level building blocks of the kernels, in one place:
// every reduction whose order is part of the project's promise (fixed order, run-to-run
// bit-reproducible, no floating-point atomics) is stated here once, and a kernel calls it.
// Device-only.  A wave is 64 lanes, all active at the call; a workgroup is 256 threads.
// The floating-point helpers pin contraction off themselves: they mean the same in a file that is
// built with contraction on.
#pragma once
#include "cg_internal.h"

// Sum over the 64 lanes by xor butterfly: v = v + v[lane ^ m] for m = 32, 16, ..., 1.
// Every lane ends with the sum.
__device__ __forceinline__ double wave_sum_xor(double v) {
#pragma clang fp contract(off)
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

// Largest of the 64 lanes: v = fmax(v, v[lane + off]) for off = 32, 16, ..., 1, a lane without
// that neighbour taking its own value.  Lane 0 holds the result.
// (The sum of the same shape is wave_sum_xor: lane 0 reads only lanes whose own reads stayed in
// range, there v[lane + off] is v[lane ^ off], and the operands stand in the same order — lane
// 0's bits are the same.)
__device__ __forceinline__ double wave_max_down(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
    return v;
}

// Smallest and largest int of the 64 lanes by xor butterfly, m = 1, 2, ..., 32.  Every lane ends
// with the result.
__device__ __forceinline__ int wave_min_xor(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ int wave_max_xor(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m));
    return v;
}

// v + the DPP move of v (0 where the move has no source lane or the row is masked out)
template <int kCtrl, int kRows>
__device__ __forceinline__ double dpp_add(double v) {
#pragma clang fp contract(off)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, kRows, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, kRows, 0xf, false);
    return v + __hiloint2double(hi, lo);
}

// Sum over the 64 lanes in DPP moves (no LDS round trips): row_shr 1, 2, 4, 8 make an inclusive
// scan inside the rows of 16 lanes, row_bcast 15 and 31 carry the row totals forward.
// Lane 63 holds the sum.
__device__ __forceinline__ double wave_sum_dpp(double v) {
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    return v;
}

// Inclusive scan over the 64 lanes in the same DPP moves: lane l ends with v[0] + ... + v[l]
// (unsigned: the order does not matter).
__device__ __forceinline__ unsigned wave_scan_dpp(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// Runs of consecutive lanes with equal key: every lane gets the first lane of its run and the
// run's length.  (One atomic per run instead of one per lane: device-scope atomics execute
// memory-side on MI355X, and particle memory is in mesh-tile order, so runs are long.)
__device__ __forceinline__ void wave_runs(unsigned key, int lane, int &run_start, int &run_len) {
    unsigned prev = __shfl_up(key, 1);
    bool head = (lane == 0) || (key != prev);
    unsigned long long mask = __ballot(head);
    unsigned long long below = mask & (~0ull >> (63 - lane));  // heads at lanes <= lane
    run_start = 63 - __clzll(below);
    unsigned long long above = (lane == 63) ? 0ull : (mask >> (lane + 1));
    int next = above ? (lane + 1 + (__ffsll((long long)above) - 1)) : 64;
    run_len = next - run_start;
}

// The operations of block_tree and k_reduce_columns: op(a, b) and the value a fold starts from.
struct OpPlus {
    static __device__ __forceinline__ double identity() { return 0.0; }
    __device__ __forceinline__ double operator()(double a, double b) const {
#pragma clang fp contract(off)
        return a + b;
    }
};
struct OpFmin {
    static __device__ __forceinline__ double identity() { return INFINITY; }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct OpFmax {
    static __device__ __forceinline__ double identity() { return -INFINITY; }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};
// the reference's maximum (value > maximum, from 0): a NaN never compares greater, so none gets in
struct OpGreaterFrom0 {
    static __device__ __forceinline__ double identity() { return 0.0; }
    __device__ __forceinline__ double operator()(double a, double b) const { return b > a ? b : a; }
};

// the extremes of measure(): a NaN gets in and stays in (fmin and fmax would drop it)
struct OpMinNan {
    static __device__ __forceinline__ double identity() { return INFINITY; }
    __device__ __forceinline__ double operator()(double a, double b) const {
        return (b < a || b != b) ? b : a;
    }
};
struct OpMaxNan {
    static __device__ __forceinline__ double identity() { return 0.0; }
    __device__ __forceinline__ double operator()(double a, double b) const {
        return (b > a || b != b) ? b : a;
    }
};

// Fold over the 64 lanes by xor butterfly, m = 32, 16, ..., 1, for an Op whose result does not
// depend on the order of its two operands.  Every lane ends with the result.
template <class Op>
__device__ __forceinline__ double wave_fold_xor(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = Op()(v, __shfl_xor(v, m));
    return v;
}

// ---- double-double: a value hi + lo with |lo| <= ulp(hi)/2, about 106 bits ----
// The sums of measure() (momenta add up to about zero: a double-precision tree sum returns
// round-off).  u = 2^-53 below.  The error bounds are those of Joldes, Muller and Popescu, "Tight
// and rigorous error bounds for basic building blocks of double-word arithmetic", ACM TOMS 44(2),
// 2017, and hold without underflow and overflow.  A NaN or an infinity among the operands ends
// as a NaN or an infinity in hi.
struct dd {
    double hi, lo;
};
// a + b = s + e exactly (Knuth's TwoSum, 6 operations, any magnitudes)
__device__ __forceinline__ dd two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b;
    const double bb = s - a;
    return dd{s, (a - (s - bb)) + (b - bb)};
}
// the same in 3 operations where |a| >= |b| or a = 0 (Dekker's Fast2Sum)
__device__ __forceinline__ dd fast_two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b;
    return dd{s, b - (s - a)};
}
// x + y for a double y: DWPlusFP (algorithm 4 of the paper), relative error <= 2u^2
__device__ __forceinline__ dd dd_add_double(dd x, double y) {
#pragma clang fp contract(off)
    const dd s = two_sum(x.hi, y);
    return fast_two_sum(s.hi, x.lo + s.lo);
}
// x + y: AccurateDWPlusDW (algorithm 6 of the paper), relative error <= 3u^2 + 13u^3.  The
// result does not depend on the order of x and y: two_sum's two outputs do not.
__device__ __forceinline__ dd dd_add(dd x, dd y) {
#pragma clang fp contract(off)
    const dd s = two_sum(x.hi, y.hi);
    const dd t = two_sum(x.lo, y.lo);
    const dd v = fast_two_sum(s.hi, s.lo + t.hi);
    return fast_two_sum(v.hi, t.lo + v.lo);
}
// x*x = hi + lo exactly (no underflow of the low part)
__device__ __forceinline__ dd dd_square(double x) {
#pragma clang fp contract(off)
    const double p = x * x;
    return dd{p, fma(x, x, -p)};
}
// Sum over the 64 lanes by xor butterfly, as wave_sum_xor, with dd_add.  Every lane ends with
// the sum.
__device__ __forceinline__ dd wave_sum_xor_dd(dd v) {
    for (int m = 32; m >= 1; m >>= 1) v = dd_add(v, dd{__shfl_xor(v.hi, m), __shfl_xor(v.lo, m)});
    return v;
}

// Tree over the 256 threads of a workgroup in LDS: red[t] = v of thread t, then for
// m = 128, 64, ..., 1 the threads t < m set red[t] = op(red[t], red[t + m]).
// Every thread returns red[0]; a second call needs another red (or a barrier in between).
template <class Op>
__device__ __forceinline__ double block_tree(double *red, double v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] = Op()(red[threadIdx.x], red[threadIdx.x + m]);
        __syncthreads();
    }
    return red[0];
}

// The sum and the maximum of the 256 threads' (sum, mx), stored by thread 0 as pair[0], pair[1]:
// lanes by wave_sum_xor and wave_max_down, then the four wave leaders' values through LDS as
// (s0 + s1) + (s2 + s3) and fmax(fmax(m0, m1), fmax(m2, m3)).
__device__ __forceinline__ void block_sum_max_store(double sum, double mx, double *pair) {
#pragma clang fp contract(off)
    __shared__ double s_sum[4], s_max[4];
    sum = wave_sum_xor(sum);
    mx = wave_max_down(mx);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_sum[w] = sum;
        s_max[w] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pair[0] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        pair[1] = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3]));
    }
}

// out[q] = the partials of column q, partial[p*stride + q] for p < npartials, under Op in a fixed
// order: workgroup q, thread t folds p = t, t + 256, ... in turn from Op::identity(), then
// block_tree.  Launched with 256 threads and one workgroup per column.
// (Unnamed namespace: the files compile separately and each instantiates its own.)
namespace {
template <class Op>
__global__ __launch_bounds__(256) void k_reduce_columns(const double *__restrict__ partial,
                                                        i64 npartials, i64 stride,
                                                        double *__restrict__ out) {
    __shared__ double red[256];
    const i64 q = blockIdx.x;
    double s = Op::identity();
    for (i64 p = threadIdx.x; p < npartials; p += 256) s = Op()(s, partial[p * stride + q]);
    s = block_tree<Op>(red, s);
    if (threadIdx.x == 0) out[q] = s;
}
}  // namespace
