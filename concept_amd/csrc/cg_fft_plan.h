// cg_fft_plan.h — the host-side arithmetic of the hand-written solve (cg_fft.hip): how the
// layers are chunked for the interleaved z / y passes, and which form a strided pass takes with
// which launch numbers.  Plain C++ without HIP, so that tests/fft_plan_print.cpp can print these
// plans on any host (tests/test_fft_plan_host.py).
#pragma once
#include <cstdint>

typedef int64_t i64;

constexpr i64 kFftLdsBytes = 160 * 1024;  // LDS of one CU

// Layers per chunk of the interleaved z / y passes.  Measured at 1024^3 (8.5 MB per layer, ms
// for z + y forward and inverse together): 16 layers 13.4, 24: 12.2, 27: 11.6, 28: 11.7,
// 31: 11.3, 32: 11.9, 36: 13.2, 40: 13.6, no chunks: 14.4 — the chunk must fit the 256 MB
// infinity cache (the cliff sits just above 32 layers = 273 MB), and among the sizes that do,
// those whose tile count nl*ceil((N/2+1)/8) fills whole rounds of the persistent y pass (one
// workgroup per CU) win: 31 layers = 2015 tiles = 7.9 rounds of 256 beats 32 = 8.1 rounds.
inline i64 zy_chunk_layers(i64 N, i64 ny, i64 pad, int ncu) {
    const i64 plane_bytes = ny * pad * 8;
    i64 cap = 266000000ll / plane_bytes;
    if (cap < 1) cap = 1;
    if (cap >= N) return N + 1;  // the whole mesh fits: no chunks
    const i64 nkb = (N / 2 + 1 + 7) / 8;
    i64 best = cap;
    double best_eff = 0;
    for (i64 nl = cap; nl >= cap - cap / 4 && nl >= 1; nl--) {
        i64 tiles = nl * nkb, rounds = (tiles + ncu - 1) / ncu;
        double eff = (double)tiles / (double)(rounds * ncu);
        if (eff > best_eff + 1e-9) {
            best_eff = eff;
            best = nl;
        }
    }
    return best;
}

// Split `total` layers into chunks of about `chunk` layers whose sizes differ by at most one
// (no tiny last chunk): chunk i covers [begin(i), begin(i + 1)).
struct ChunkPlan {
    i64 n, base, extra;
    ChunkPlan(i64 total, i64 chunk) {
        n = chunk >= total ? 1 : (total + chunk / 2) / chunk;
        if (n < 1) n = 1;
        base = total / n;
        extra = total % n;
    }
    i64 begin(i64 i) const { return i * base + (i < extra ? i : extra); }
};

// The forms of a strided (y or x) pass over pencils of 2^logn points, mode 0 forward, 1 inverse,
// 2 fused (forward, k-space factor, inverse):
//   Split, SplitBlocked  k_fft_strided_h: even/odd halves of 8 pencils, persistent workgroups
//                        (Blocked: a pencil map in blocks, the transpose buffers of the slabs)
//   Persistent           k_fft_strided_p: whole pencils, tables in LDS, persistent workgroups
//   Plain                k_fft_strided: whole pencils, one workgroup per tile
// W adjacent kk per workgroup.  Measured at 1024^3 (ms per y pass / fused x pass):
//   W = 2 (32 B row segments, 4 workgroups per CU)  9.4 / 9.6
//   W = 4 (64 B, 2 per CU)                          4.6 / 7.9
//   W = 8 (128 B = one full cache line, 1 per CU)   3.95 / 7.4
// The row-segment width, not the occupancy, decides: default 8 (N <= 1024; 8 pencils of
// 2048 points exceed the 160 KB LDS, so 4 there).
enum class PassForm { Split, SplitBlocked, Persistent, Plain };
// (LDS bytes below: 16 per double2, 8 per double)

constexpr int whole_W(int logn) { return logn <= 10 ? 8 : 4; }
// one radix-16 butterfly per lane and pass: N*W/16 lanes, 64..1024
constexpr int whole_NT(int logn) {
    const int ntw = (1 << logn) * whole_W(logn) / 16;
    return ntw < 64 ? 64 : (ntw > 1024 ? 1024 : ntw);
}
constexpr i64 plain_lds(int logn) { return 16 * (1 << logn) * whole_W(logn); }
// persistent form: the twiddles (and the k-space table of the fused pass) on top of the tile
constexpr i64 persistent_lds(int logn, int mode) {
    return plain_lds(logn) + 16 * ((1 << logn) / 2) + (mode == 2 ? 8 * (1 << logn) : 0);
}
// ... only where every lane holds 16 points and the tables fit
// (2048 points x 4 pencils + tables = exactly 160 KB in the fused pass)
constexpr bool can_persist(int logn, int mode) {
    return logn <= 11 && (1 << logn) * whole_W(logn) == 16 * whole_NT(logn) &&
           whole_NT(logn) % whole_W(logn) == 0 && persistent_lds(logn, mode) <= kFftLdsBytes;
}
constexpr bool can_split(int logn) { return logn >= 9 && logn <= 11; }
constexpr int kSplitW = 8;
constexpr int split_NT(int logn) { return ((1 << logn) / 2) * kSplitW / 16; }
constexpr i64 split_lds(int logn, int mode) {
    return 16 * ((1 << logn) / 2) * kSplitW + 16 * ((1 << logn) / 4) +
           (mode == 2 ? 8 * (1 << logn) : 0) + 16 * (split_NT(logn) / kSplitW);
}

struct MapShape {  // of a PencilMap (cg_fft.hip)
    i64 es;        // complex elements between consecutive pencil points inside a block
    int sh;        // log2(points per block); 31 = one block
};
struct StridedChoice {
    PassForm form;
    int W, NT;   // pencils per tile, lanes per workgroup
    i64 lds;     // dynamic LDS bytes
    i64 grid;    // workgroups
    int nkb;     // tiles per outer index
    i64 ntiles;  // nouter * nkb
};

// split_mode: CONCEPT_GPU_FFT_SPLIT.  0: the whole-pencil passes everywhere (what small meshes
// and the blocked maps of narrow slabs take anyway: the tests run them at size this way); 1, the
// default: the split pass from 1024 points; 2: at 512 points too (it does not pay there: 0.48
// against 0.46 ms).
inline StridedChoice strided_choice(int logn, int mode, i64 N, i64 pad, int ncu, int split_mode,
                                    i64 nouter, MapShape smap, MapShape dmap) {
    const bool plain_maps = smap.sh == 31 && dmap.sh == 31;
    if (can_split(logn) && (logn < 10 ? split_mode >= 2 : split_mode != 0)) {
        const int W = kSplitW, NT = split_NT(logn), rows = 2 * (NT / W);  // rows a lane spans
        const int nkb = (int)((N / 2 + 1 + W - 1) / W);
        const i64 ntiles = nouter * nkb;
        // per-lane offsets are 32-bit byte offsets: rows 2 ml (ml < NT/W) must span < 4 GB
        const i64 reach = ((i64)(rows - 2) * (smap.es > dmap.es ? smap.es : dmap.es) + W) * 16;
        // blocked maps: whole multiples of the rows a lane spans per block
        auto blocks_ok = [rows](MapShape m) { return m.sh == 31 || (1 << m.sh) >= rows; };
        // ... and enough tiles to keep every CU busy, the last tile inside the row
        if (ntiles >= 2 * (i64)ncu && blocks_ok(smap) && blocks_ok(dmap) &&
            reach < ((i64)1 << 32) && (i64)nkb * W <= pad / 2) {
            const i64 lds = split_lds(logn, mode);
            // workgroups per CU the LDS allows (2048: one; 1024: two, each the other's cover)
            const i64 per_cu = kFftLdsBytes / lds < 1 ? 1 : kFftLdsBytes / lds;
            return {plain_maps ? PassForm::Split : PassForm::SplitBlocked, W, NT, lds,
                    ncu * per_cu, nkb, ntiles};
        }
    }
    const int W = whole_W(logn), NT = whole_NT(logn);
    const int nkb = (int)((N / 2 + 1 + W - 1) / W);
    const i64 ntiles = nouter * nkb;
    // persistent: plain maps only, and only where it pays (many tiles per CU)
    if (can_persist(logn, mode) && plain_maps && ntiles >= 4 * (i64)ncu) {
        const i64 lds = persistent_lds(logn, mode);
        i64 per_cu = kFftLdsBytes / lds;
        if (per_cu < 1) per_cu = 1;
        if (per_cu > 4) per_cu = 4;
        return {PassForm::Persistent, W, NT, lds, ncu * per_cu, nkb, ntiles};
    }
    return {PassForm::Plain, W, NT, plain_lds(logn), ntiles, nkb, ntiles};
}
