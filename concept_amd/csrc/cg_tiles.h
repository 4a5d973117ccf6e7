// cg_tiles.h — device helpers shared by the particle kernels: the reference's mod(),
// the tile / bucket key of a particle; with it come the wave primitives of cg_wave.h (wave_runs
// turns runs of equal keys into one atomic each, reserve_run below gives such a run its slots).
#pragma once
#include "cg_internal.h"
#include "cg_wave.h"

// Component.drift's mod (species.py:2194-2196, commons.py:5103-5110): numpy floored
// modulo, then a result that rounded to exactly boxsize becomes 0.
__device__ __forceinline__ double ref_mod(double x, double L) {
    if (x > 0 && x < L) return x;  // fmod(x, L) == x, same sign as L
    double m = fmod(x, L);          // exact
    if (m != 0) {
        if (m < 0) m += L;          // npy_divmod: sign fix-up (L > 0)
    } else {
        m = 0.0;                    // copysign(0, L)
    }
    if (m == L) m = 0;              // commons.py:5108-5109
    return m;
}

// a pair's squared distance (gravity.py:306, r2 = x**2 + y**2 + z**2 in that order): the two
// additions fused with their products — three FP64 instructions instead of five in the loops
// that are bound by their issue rate; within an ulp of the unfused sum (the reference's own
// build contracts them as its compiler sees fit: -O3 -ffast-math -march=native, src/Makefile:175-189)
__device__ __forceinline__ double sr_r2(double x, double y, double z) {
    return __builtin_fma(z, z, __builtin_fma(y, y, x * x));
}

// 32-bit: x is positive and < gridsize + 2*nghosts + 1, so truncating to int equals the
// reference's truncation to Py_ssize_t (one v_cvt_i32_f64 instead of the double -> int64
// sequence)
__device__ __forceinline__ int lower_cell(double pos, double off, double scale, int g, int N) {
    double x = (pos - off) * scale;
    int a = (int)x - g;
    a = a < 0 ? a + N : a;
    return a >= N ? a - N : a;
}
// key = 8*tile + bucket; bucket bit d is set when the lower cell is the last of
// the tile in dimension d, i.e. the CIC cloud reaches the next tile there
// (bit 2: x, bit 1: y, bit 0: z).  The pull-deposit of a tile reads its own 8
// buckets plus the matching boundary buckets of its 7 lower neighbours.
constexpr unsigned kNoTile = 0xffffffffu;
__device__ __forceinline__ unsigned tile_of(double x, double y, double z, const CicGeom &geo,
                                            int g, i64 N, const TileGeom &t, i64 x0) {
    const int Ni = (int)N;
    int cx = lower_cell(x, geo.off[0], geo.scale, g, Ni) - (int)x0;  // local layer of this domain
    if (cx < 0 || cx >= t.ntx * t.tx) return kNoTile;                 // not owned here
    unsigned ca = (unsigned)cx;
    unsigned cb = (unsigned)lower_cell(y, geo.off[1], geo.scale, g, Ni);
    unsigned cc = (unsigned)lower_cell(z, geo.off[2], geo.scale, g, Ni);
    // the tile extent is a power of two (cg_create): shifts and masks, not divisions
    const unsigned sh = (unsigned)(__ffs(t.tx) - 1), last = (unsigned)t.tx - 1u;
    unsigned a = ca >> sh, b = cb >> sh, c = cc >> sh;
    unsigned f = (((ca & last) == last) ? 4u : 0u) | (((cb & last) == last) ? 2u : 0u) |
                 (((cc & last) == last) ? 1u : 0u);
    return ((a * t.nty + b) * t.ntz + c) * 8u + f;
}

// A run of `rl` consecutive lanes with the same key (wave_runs: the run starts at lane rs) takes
// `rl` slots of the key's region [start[key], start[key + 1]) with ONE atomic on taken[key],
// issued by its first lane; every lane of the run gets the run's first slot.  A run that does not
// fit is dropped — kNoTile, never a slot outside its region — and raises `err_bit` in err_flags.
// `capacity`: rows of the arrays behind the regions — a region that reaches beyond them has no
// room at all — or kNoCapacity (more than any table can hold: the test folds away) where the
// regions are known to lie inside.
constexpr i64 kNoCapacity = INT64_MAX;
__device__ __forceinline__ unsigned reserve_run(const unsigned *start, unsigned *taken,
                                                unsigned key, int lane, int rs, int rl,
                                                i64 capacity, unsigned *err_flags,
                                                unsigned err_bit) {
    unsigned first = kNoTile;
    if (lane == rs && key != kNoTile) {
        const unsigned o0 = start[key], o1 = start[key + 1];
        const unsigned room = (i64)o1 <= capacity ? o1 - o0 : 0u;
        const unsigned local = atomicAdd(&taken[key], (unsigned)rl);
        if (local + (unsigned)rl > room) atomicOr(err_flags, err_bit);
        else first = o0 + local;
    }
    return __shfl(first, rs);
}
