// cg_rocfft_layout.h — the data layouts of the plans the rocFFT backend (cg_rocfft.hip) makes, as
// plain data: the stride arithmetic of that backend is here and nowhere else.  Plain C++ without
// HIP or rocFFT, so that tests/rocfft_layout_print.cpp can print the layouts on any host
// (tests/test_rocfft_layout_host.py).
//
// All transforms are in place, double precision and unnormalised both ways (mesh.py:4015-4022).
// N: grid size; pad: doubles per row (cp = pad/2 complex numbers); ny: rows per layer (cg_ctx).
// Strides and distances are in elements of the side they describe: doubles on the real side of a
// real transform, complex numbers everywhere else.
#pragma once
#include <cstddef>

enum class RocfftKind { RealForward, RealInverse, ComplexForward, ComplexInverse };

struct RocfftLayout {
    RocfftKind kind;
    size_t dims;
    size_t lengths[3];  // fastest first
    size_t in_stride[3], in_dist;
    size_t out_stride[3], out_dist;
    size_t batch;
};

// a real transform of `dims` dimensions of N points: real rows of pad doubles <-> hermitian rows
// of cp complex numbers in the same memory; s1, s2: the strides of the second and third dimension
// and dist the distance between transforms, all in rows
inline RocfftLayout fft_layout_real(bool inverse, size_t dims, size_t N, size_t pad, size_t s1,
                                    size_t s2, size_t dist, size_t batch) {
    const size_t cp = pad / 2;
    RocfftLayout r{RocfftKind::RealForward, dims, {N, N, N}, {1, pad * s1, pad * s2}, pad * dist,
                   {1, cp * s1, cp * s2}, cp * dist, batch};
    if (!inverse) return r;
    return RocfftLayout{RocfftKind::RealInverse, dims, {N, N, N}, {1, cp * s1, cp * s2}, cp * dist,
                        {1, pad * s1, pad * s2}, pad * dist, batch};
}
// `batch` complex transforms of N points `stride` apart, one per consecutive complex number
inline RocfftLayout fft_layout_columns(bool inverse, size_t N, size_t stride, size_t batch) {
    return RocfftLayout{inverse ? RocfftKind::ComplexInverse : RocfftKind::ComplexForward, 1,
                        {N, 1, 1}, {stride, 0, 0}, 1, {stride, 0, 0}, 1, batch};
}

// The single-domain mesh, the padded layout FFTW uses (fft.c:34-73):
// real double[N][ny][pad] <-> hermitian complex[N][ny][cp].  The row pitch pad >= N + 2 doubles is
// a multiple of 16 doubles when N is, so that rows and 16-cell tile rows start on 128-byte lines.
inline RocfftLayout fft_layout_3d(bool inverse, size_t N, size_t ny, size_t pad) {
    return fft_layout_real(inverse, 3, N, pad, 1, ny, N * N, 1);
}
// z and y of `nlayers` consecutive layers of a slab: one 2-D transform per layer of ny rows
inline RocfftLayout fft_layout_2d(bool inverse, size_t N, size_t ny, size_t pad, size_t nlayers) {
    return fft_layout_real(inverse, 2, N, pad, 1, 0, ny, nlayers);
}
// the same in two steps on one layer: z on its N rows, real <-> hermitian in place ...
inline RocfftLayout fft_layout_z_rows(bool inverse, size_t N, size_t pad) {
    return fft_layout_real(inverse, 1, N, pad, 0, 0, 1, N);
}
// ... and y on its columns kk <= N/2, complex numbers one row apart
inline RocfftLayout fft_layout_y_columns(bool inverse, size_t N, size_t pad) {
    return fft_layout_columns(inverse, N, pad / 2, N / 2 + 1);
}
// x on the transpose buffer complex[N][JB + 1][cp], JB = N/nprocs: one transform per (row of the
// own block, kk), JB*cp of them (the unused row JB of a layer is not transformed)
inline RocfftLayout fft_layout_x(bool inverse, size_t N, size_t pad, size_t nprocs) {
    const size_t cp = pad / 2, JB = N / nprocs;
    return fft_layout_columns(inverse, N, (JB + 1) * cp, JB * cp);
}
