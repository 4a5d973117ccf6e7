// cg_sr_pairs.h — the pair test of the P3M short-range sweeps, once (device only).
//
//   particle_particle           interactions.py:1563-1791  x_ji = xi - xj, + the image's offset
//   gravity_pairwise_shortrange gravity.py:263-354         r2 cut, r2-indexed table, Δmom
//
// Every form of the sweep — the blocks of tiles inside a range and across two ranges, one
// wavefront per active receiver, a handful of receivers without a cell list (cg_shortrange.hip),
// the dense tiles' quads (cg_shortrange_dense.hip) — fetches its suppliers and forms the pair
// vector (xi - xj) + offset in its own way, and hands it to the three phases below.  A tile may
// go to the cells sweep or to the dense tiles' sweep: that its pairs contribute the same bits
// either way, and that the counters of bench.py's pair_sweep_roofline count the same things, is
// what this header holds in one place.
#pragma once
#include "cg_internal.h"
#include "cg_tiles.h"

// cg_shortrange_stats, per sweep form three words: pair tests executed (lanes that hold a
// receiver and a supplier), of them in range, wavefront trips (64 lane slots each).  Counted by
// the STATS instantiations only, per wavefront; lane 0 flushes.
struct SrCount {
    unsigned tests = 0, hits = 0, trips = 0;
    // one slot of a trip (wave-wide: every lane of the wave calls it)
    __device__ __forceinline__ void add(bool valid, bool hit) {
        tests += (unsigned)__popcll(__ballot(valid));
        hits += (unsigned)__popcll(__ballot(valid && hit));
    }
    __device__ __forceinline__ void flush(unsigned long long *stats3) const {
        atomicAdd(&stats3[0], (unsigned long long)tests);
        atomicAdd(&stats3[1], (unsigned long long)hits);
        atomicAdd(&stats3[2], (unsigned long long)trips);
    }
};

// NB pairs of one lane and one trip.
//  set: r2 as one product and two fused multiply-adds (sr_r2: within 1 ulp of the reference's
//    x*x + y*y + z*z, so that a pair at the range or at a table entry's boundary may fall on the
//    other side of it), the range test; `valid` is false for a slot that holds no supplier;
//  accumulate: the table loads of the hits, all issued before the first is used, then
//    a += x_ji * table[int(r2 * scaling)] as fused multiply-adds (a pair out of range adds
//    x_ji * 0: nothing, the positions being finite).  The receiver's factor comes once, at the end.
template <int NB>
struct SrPairs {
    double x[NB], y[NB], z[NB], r2[NB];
    bool hit[NB];
    __device__ __forceinline__ void set(int j, double xj, double yj, double zj, bool valid,
                                        double r2_max) {
        x[j] = xj, y[j] = yj, z[j] = zj;
        r2[j] = sr_r2(xj, yj, zj);         // gravity.py:306
        hit[j] = valid && r2[j] <= r2_max;  // gravity.py:311: skip r2 > r2_max
    }
    __device__ __forceinline__ void accumulate(double r2_index_scaling,
                                               const double *__restrict__ table, double &ax,
                                               double &ay, double &az) const {
        double t[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            t[j] = 0.0;
            if (hit[j]) t[j] = table[(unsigned)(int)(r2[j] * r2_index_scaling)];  // gravity.py:316-321
        }
#pragma unroll
        for (int j = 0; j < NB; j++) {
            ax = __builtin_fma(x[j], t[j], ax);
            ay = __builtin_fma(y[j], t[j], ay);
            az = __builtin_fma(z[j], t[j], az);
        }
    }
};

// The image of a supplier run as 2 bits per dimension, (ox + 1) | (oy + 1) << 2 | (oz + 1) << 4
// with o in {-1, 0, +1} box lengths (0x15: none) -> the offset to add to the pair vector in
// dimension d (gravity.py:299-302; the product is exact)
__device__ __forceinline__ double sr_image_offset(int code, int d, double L) {
    return (double)((code >> 2 * d & 3) - 1) * L;
}

// A coordinate's tile exactly as Tiling.sort (species.py:775-780) with tiling location 0
__device__ __forceinline__ unsigned sr_tile1(double x, double inv, unsigned nt) {
    const unsigned t = (unsigned)(i64)((x - 0.0) * inv);
    return t >= nt ? nt - 1 : t;
}
