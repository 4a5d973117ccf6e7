// cg_bispec.h — the overlap of a unit grid cell with a bispectrum shell, and the set of modes
// the reference's shell loop visits.  No HIP runtime header: the file compiles with the host
// C++ compiler alone (tests/test_bispec_host.py builds it into a program of its own).
//   bispec_overlap_cellshell             get_bispec_overlap_cellshell            analysis.py:2803-2807
//   bispec_overlap_cellball              get_bispec_overlap_cellball             analysis.py:2831-2871
//   bispec_overlap_blockball             get_bispec_overlap_blockball            analysis.py:2887-2896
//   bispec_overlap_blockball_indefinite  get_bispec_overlap_blockball_indefinite analysis.py:2923-2982
//   BispecShellBounds, bispec_shell_row  fourier_shell_loop                      mesh.py:3186-3296
// The expressions, their order and the guards are the reference's; masks (x > 0) multiply as
// 0.0 / 1.0 like the reference's booleans do.  Build with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CG_BISPEC_HD __host__ __device__
#else
#define CG_BISPEC_HD
#endif

CG_BISPEC_HD inline double bispec_mask(bool b) { return b ? 1.0 : 0.0; }

CG_BISPEC_HD inline double bispec_overlap_blockball_indefinite(double x, double y_bgn,
                                                               double z_bgn, double r,
                                                               double y_bgn2, double z_bgn2,
                                                               double r2) {
    x = x * bispec_mask(x <= r) + r * bispec_mask(x > r);
    const double x2 = x * x;
    const double x4 = x2 * x2;
    const double r4 = r2 * r2;
    const double r8 = r4 * r4;
    const double r2_x2 = r2 - x2;
    double sqrt_y = r2_x2 - y_bgn2;
    sqrt_y = sqrt(sqrt_y * bispec_mask(sqrt_y > 0));
    double sqrt_z = r2_x2 - z_bgn2;
    sqrt_z = sqrt(sqrt_z * bispec_mask(sqrt_z > 0));
    const double sqrt_yz = sqrt_y * sqrt_z;
    const double yz = y_bgn * z_bgn;
    const double y2z2 = y_bgn2 * z_bgn2;
    const double y2_z2 = y_bgn2 + z_bgn2;
    const double two_x2 = 2 * x2;
    const double y_z2 = y_bgn * z_bgn2;
    const double y2_z = y_bgn2 * z_bgn;
    const double y_sqrt_y = y_bgn * sqrt_y;
    const double z_sqrt_z = z_bgn * sqrt_z;
    const double three_r2 = 3 * r2;
    const double arctan_xy = atan2(x, sqrt_y);
    const double arctan_xz = atan2(x, sqrt_z);
    const double arctan_yz = atan2(sqrt_yz - yz, y_bgn * sqrt_z + z_bgn * sqrt_y);
    double xx = (x4 * y2z2 +
                 r2 * ((x4 * y2_z2 + two_x2 * y_bgn * (y_z2 - 2 * z_bgn * sqrt_yz)) +
                       r2 * ((x4 + y2z2) + r2 * (-two_x2 - y2_z2)))) +
                r8;
    double yy = 2 * x * r *
                (-x2 * (y_z2 * sqrt_y + y2_z * sqrt_z) +
                 r2 * (y_sqrt_y * (r2_x2 - z_bgn2) + z_sqrt_z * (r2_x2 - y_bgn2)));
    const double eps = 1e-14 * (r8 + 1);
    const bool xx_zero = (-eps < xx) & (xx < eps);
    const bool yy_zero = (-eps < yy) & (yy < eps);
    xx = xx * bispec_mask(!xx_zero) - 1e-100 * bispec_mask(xx_zero);
    yy = yy * bispec_mask(!yy_zero) + 1e-200 * bispec_mask(yy_zero);
    const double arctan_xyz = atan2(yy, xx);
    return (x * yz - 1. / 3. * x * (y_sqrt_y + z_sqrt_z)) +
           1. / 6. *
               (((-y_bgn * (three_r2 - y_bgn2) * arctan_xy -
                  z_bgn * (three_r2 - z_bgn2) * arctan_xz) +
                 x * (three_r2 - x2) * arctan_yz) +
                r * r2 * arctan_xyz);
}

CG_BISPEC_HD inline double bispec_overlap_blockball(double x_bgn, double y_bgn, double z_bgn,
                                                    double r, double dx, double y_bgn2,
                                                    double z_bgn2, double r2) {
    const double s =
        sqrt(r2 - y_bgn2 * bispec_mask(y_bgn > 0) - z_bgn2 * bispec_mask(z_bgn > 0));
    const double x_end = fmin(x_bgn + dx, +s);
    x_bgn = fmax(x_bgn, -s);
    return bispec_overlap_blockball_indefinite(x_end, y_bgn, z_bgn, r, y_bgn2, z_bgn2, r2) -
           bispec_overlap_blockball_indefinite(x_bgn, y_bgn, z_bgn, r, y_bgn2, z_bgn2, r2);
}

// One leaf of get_bispec_overlap_cellball: a box that straddles no coordinate plane.
CG_BISPEC_HD inline double bispec_overlap_leaf(double x_bgn, double y_bgn, double z_bgn, double r,
                                               double dx, double dy, double dz) {
    const double x_end = x_bgn + dx, y_end = y_bgn + dy, z_end = z_bgn + dz;
    const double x_bgn2 = x_bgn * x_bgn, y_bgn2 = y_bgn * y_bgn, z_bgn2 = z_bgn * z_bgn;
    const double r2 = r * r;
    if ((x_bgn2 + y_bgn2) + z_bgn2 >= r2) return 0;
    const double x_end2 = x_end * x_end, y_end2 = y_end * y_end, z_end2 = z_end * z_end;
    if (x_end2 + y_end2 + z_end2 <= r2) return dx * dy * dz;
    double frac = bispec_overlap_blockball(x_bgn, y_bgn, z_bgn, r, dx, y_bgn2, z_bgn2, r2);
    if ((x_bgn2 + y_end2) + z_bgn2 < r2)
        frac -= bispec_overlap_blockball(x_bgn, y_end, z_bgn, r, dx, y_end2, z_bgn2, r2);
    if ((x_bgn2 + y_bgn2) + z_end2 < r2) {
        frac -= bispec_overlap_blockball(x_bgn, y_bgn, z_end, r, dx, y_bgn2, z_end2, r2);
        if ((x_bgn2 + y_end2) + z_end2 < r2)
            frac += bispec_overlap_blockball(x_bgn, y_end, z_end, r, dx, y_end2, z_end2, r2);
    }
    return frac;
}

// The reflection and the split of one axis (analysis.py:2832-2852): the box [bgn, bgn + len)
// becomes one piece (bgn, len), or, when it straddles the coordinate plane, the two pieces
// (0, len0) and (0, len1).  A half starts at 0 and is not split again, so the recursion of
// the reference ends after one level per axis.  (Scalars picked by the piece number, no
// arrays indexed by it: those would live in scratch memory on the device.)
struct BispecAxis {
    double bgn, len0, len1;
    int n;
};
CG_BISPEC_HD inline BispecAxis bispec_split_axis(double bgn, double len) {
    bgn -= (2 * bgn + len) * bispec_mask(bgn < -len);
    const double end = bgn + len;
    if (0 < end && end < len) return BispecAxis{0, +end, -bgn, 2};
    return BispecAxis{bgn, len, len, 1};
}

#if defined(__clang__)
#define CG_BISPEC_NOUNROLL _Pragma("nounroll")
#else
#define CG_BISPEC_NOUNROLL
#endif

// get_bispec_overlap_cellball, flat: at most 2 x 2 x 2 leaves, summed in the order of the
// reference's recursion (x halves outermost, each the sum of its y halves, each the sum of
// its z halves).  The loops stay rolled: one copy of the leaf's code.
CG_BISPEC_HD inline double bispec_overlap_cellball(double x_bgn, double y_bgn, double z_bgn,
                                                   double r, double dx, double dy, double dz) {
    const BispecAxis X = bispec_split_axis(x_bgn, dx);
    const BispecAxis Y = bispec_split_axis(y_bgn, dy);
    const BispecAxis Z = bispec_split_axis(z_bgn, dz);
    double sx = 0;
    CG_BISPEC_NOUNROLL
    for (int ix = 0; ix < X.n; ix++) {
        double sy = 0;
        CG_BISPEC_NOUNROLL
        for (int iy = 0; iy < Y.n; iy++) {
            double sz = 0;
            CG_BISPEC_NOUNROLL
            for (int iz = 0; iz < Z.n; iz++) {
                const double leaf = bispec_overlap_leaf(
                    X.bgn, Y.bgn, Z.bgn, r, ix ? X.len1 : X.len0, iy ? Y.len1 : Y.len0,
                    iz ? Z.len1 : Z.len0);
                sz = iz ? sz + leaf : leaf;
            }
            sy = iy ? sy + sz : sz;
        }
        sx = ix ? sx + sy : sy;
    }
    return sx;
}

CG_BISPEC_HD inline double bispec_overlap_cellshell(int64_t ki, int64_t kj, int64_t kk,
                                                    double k_inner, double k_outer) {
    return bispec_overlap_cellball(ki - 0.5, kj - 0.5, kk - 0.5, k_outer, 1, 1, 1) -
           bispec_overlap_cellball(ki - 0.5, kj - 0.5, kk - 0.5, k_inner, 1, 1, 1);
}

// fourier_shell_loop(gridsize, k_inner, k_outer, skip_origin=True) (mesh.py:3186-3296): what
// does not depend on the row
struct BispecShellBounds {
    double k2_min, k2_max;  // the shell's squared radii
    int64_t k_max_1D;       // |ki|, |kj|, kk <= this (<= nyquist - 1)
    int64_t k2_max_2D;      // ki^2 + kj^2 <= this
};

CG_BISPEC_HD inline BispecShellBounds bispec_shell_bounds(int64_t gridsize, double k_inner,
                                                          double k_outer) {
    const int64_t nyquist = gridsize / 2;
    BispecShellBounds b;
    b.k2_min = k_inner * k_inner;
    b.k2_max = k_outer * k_outer;
    b.k_max_1D = (int64_t)(k_outer + 0.5 * sqrt(1.0));
    const double d = k_outer + 0.5 * sqrt(2.0);
    b.k2_max_2D = (int64_t)(d * d);
    if (b.k_max_1D > nyquist - 1) b.k_max_1D = nyquist - 1;
    if (b.k2_max_2D > 2 * (nyquist - 1) * (nyquist - 1)) b.k2_max_2D = 2 * (nyquist - 1) * (nyquist - 1);
    return b;
}

// floor(sqrt(n)) for 0 <= n < 2^52, exact (the reference's isqrt)
CG_BISPEC_HD inline int64_t bispec_isqrt(int64_t n) {
    int64_t r = (int64_t)sqrt((double)n);
    while (r * r > n) r--;
    while ((r + 1) * (r + 1) <= n) r++;
    return r;
}

// The kk range [kk_bgn, kk_end] the loop visits in row (ki, kj) (signed mode numbers); false
// when the row is not visited at all.  The loop walks ki >= 0 and mirrors to -ki, so the
// bounds depend on |ki|; they depend on |kj| by construction.
CG_BISPEC_HD inline bool bispec_shell_row(const BispecShellBounds &b, int64_t ki, int64_t kj,
                                          int64_t *kk_bgn, int64_t *kk_end) {
    const int64_t ai = ki < 0 ? -ki : ki, aj = kj < 0 ? -kj : kj;
    if (aj > b.k_max_1D || aj * aj > b.k2_max_2D) return false;
    int64_t ki_lim = bispec_isqrt(b.k2_max_2D - aj * aj);
    if (ki_lim > b.k_max_1D) ki_lim = b.k_max_1D;
    if (ai > ki_lim) return false;
    const double kj_min = (double)aj + 0.5 * bispec_mask(aj != 0);
    const double kj_max = (double)aj - 0.5 * bispec_mask(aj != 0);
    const double ki_min = (double)ai + 0.5 * bispec_mask(ai != 0);
    const double ki_max = (double)ai - 0.5 * bispec_mask(ai != 0);
    const double kk2_corner_min = b.k2_min - kj_min * kj_min - ki_min * ki_min;
    const double kk2_corner_max = b.k2_max - kj_max * kj_max - ki_max * ki_max;
    int64_t bgn = (int64_t)(sqrt(kk2_corner_min * bispec_mask(kk2_corner_min > 0)) + 0.5);
    if (ai == 0 && aj == 0 && bgn == 0) bgn = 1;  // skip_origin
    int64_t end = (int64_t)(sqrt(kk2_corner_max * bispec_mask(kk2_corner_max > 0)) + 0.5);
    if (end > b.k_max_1D) end = b.k_max_1D;
    *kk_bgn = bgn;
    *kk_end = end;
    return bgn <= end;
}
