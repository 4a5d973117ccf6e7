"""NumPy restatements of the bispectrum core, for the tests of sizes that have no golden.

  overlap_cellshell()   get_bispec_overlap_cellshell (analysis.py:2803-2982), over arrays
  shell_rows()          the kk range fourier_shell_loop visits per (ki, kj) (mesh.py:3186-3296)
  shell_fill()          the loop of get_bispec_grid (analysis.py:2739-2778) on F[a, b, kk]
  backward()            fft(slab, 'backward'): unnormalised complex-to-real
  bispec_value()        compute_bispec_value (analysis.py:2576-2707) without its grid cache
  normalise()           the normalisation of compute_bispec (analysis.py:3097-3164)
Fourier arrays are complex F[a, b, kk] with a the x and b the y array index (the reference's
slab is its transpose [b][a][kk] with interleaved real and imaginary parts: from_slab())."""
import collections
import math

import numpy as np

# Bars.  The overlap's closed form cancels terms of size r³, so deviations are
# scaled by max(1, k_outer³).  OVERLAP_DEV_HOST is the largest scaled deviation of the host
# build of csrc/cg_bispec.h from tests/golden/bispec_overlap.npz, measured when the golden was
# made; the host bar is that rounded up to the next power of two, the device bar 8 times the
# measured deviation (device atan2 / sqrt).
OVERLAP_DEV_HOST = 6.86e-15          # measured 6.8595e-15, at cell (8, -1, 0) of shell (7.3, 8.3)
OVERLAP_BAR_HOST = 2.0**-47          # 7.105e-15
OVERLAP_BAR_DEVICE = 8*OVERLAP_DEV_HOST
# The sums: the largest deviation of this restatement from the value goldens, relative to
# Σ|g₀g₁g₂| (and to Σgᵢ²), measured on the CPU (9.38e-15 for the values, 1.0154e-14 for the
# powers, both at gridsize 12); the bar for the GPU path is 10 times that (another summation
# tree, another FFT).
SUMS_DEV_RESTATEMENT = 1.02e-14
SUMS_BAR = 10*SUMS_DEV_RESTATEMENT
GUARD_WINDOW = 1e-9


def _m(b):
    return np.asarray(b, dtype=np.float64)


def _indefinite(x, y_bgn, z_bgn, r, y_bgn2, z_bgn2, r2, guard=None):
    x = x*_m(x <= r) + r*_m(x > r)
    x2 = x*x
    x4 = x2*x2
    r4 = r2*r2
    r8 = r4*r4
    r2_x2 = r2 - x2
    sqrt_y = r2_x2 - y_bgn2
    sqrt_y = np.sqrt(sqrt_y*_m(sqrt_y > 0))
    sqrt_z = r2_x2 - z_bgn2
    sqrt_z = np.sqrt(sqrt_z*_m(sqrt_z > 0))
    sqrt_yz = sqrt_y*sqrt_z
    yz = y_bgn*z_bgn
    y2z2 = y_bgn2*z_bgn2
    y2_z2 = y_bgn2 + z_bgn2
    two_x2 = 2*x2
    y_z2 = y_bgn*z_bgn2
    y2_z = y_bgn2*z_bgn
    y_sqrt_y = y_bgn*sqrt_y
    z_sqrt_z = z_bgn*sqrt_z
    three_r2 = 3*r2
    arctan_xy = np.arctan2(x, sqrt_y)
    arctan_xz = np.arctan2(x, sqrt_z)
    arctan_yz = np.arctan2(sqrt_yz - yz, y_bgn*sqrt_z + z_bgn*sqrt_y)
    xx = (x4*y2z2
          + r2*(x4*y2_z2 + two_x2*y_bgn*(y_z2 - 2*z_bgn*sqrt_yz)
                + r2*(x4 + y2z2 + r2*(-two_x2 - y2_z2)))
          + r8)
    yy = 2*x*r*(-x2*(y_z2*sqrt_y + y2_z*sqrt_z)
                + r2*(y_sqrt_y*(r2_x2 - z_bgn2) + z_sqrt_z*(r2_x2 - y_bgn2)))
    eps = 1e-14*(r8 + 1)
    if guard is not None:
        for v in (xx, yy):
            guard.append((v != 0) & (np.abs(np.abs(v) - eps) < GUARD_WINDOW))
    xx_zero = (-eps < xx) & (xx < eps)
    yy_zero = (-eps < yy) & (yy < eps)
    xx = xx*_m(~xx_zero) - 1e-100*_m(xx_zero)
    yy = yy*_m(~yy_zero) + 1e-200*_m(yy_zero)
    arctan_xyz = np.arctan2(yy, xx)
    return (x*yz - 1./3.*x*(y_sqrt_y + z_sqrt_z)
            + 1./6.*(-y_bgn*(three_r2 - y_bgn2)*arctan_xy
                     - z_bgn*(three_r2 - z_bgn2)*arctan_xz
                     + x*(three_r2 - x2)*arctan_yz
                     + r*r2*arctan_xyz))


def _blockball(x_bgn, y_bgn, z_bgn, r, dx, y_bgn2, z_bgn2, r2, live, guard):
    with np.errstate(invalid='ignore'):
        s = np.sqrt(r2 - y_bgn2*_m(y_bgn > 0) - z_bgn2*_m(z_bgn > 0))
    x_end = np.minimum(x_bgn + dx, +s)
    x_bgn = np.maximum(x_bgn, -s)
    g = [] if guard is not None else None
    with np.errstate(invalid='ignore', divide='ignore'):
        out = (_indefinite(x_end, y_bgn, z_bgn, r, y_bgn2, z_bgn2, r2, g)
               - _indefinite(x_bgn, y_bgn, z_bgn, r, y_bgn2, z_bgn2, r2, g))
    if guard is not None:
        guard.append(live & np.logical_or.reduce(g))
    return np.where(live, out, 0.0)


def _leaf(x_bgn, y_bgn, z_bgn, r, dx, dy, dz, guard):
    x_end, y_end, z_end = x_bgn + dx, y_bgn + dy, z_bgn + dz
    x_bgn2, y_bgn2, z_bgn2 = x_bgn*x_bgn, y_bgn*y_bgn, z_bgn*z_bgn
    r2 = r*r
    outside = (x_bgn2 + y_bgn2) + z_bgn2 >= r2
    x_end2, y_end2, z_end2 = x_end*x_end, y_end*y_end, z_end*z_end
    inside = ~outside & (x_end2 + y_end2 + z_end2 <= r2)
    cut = ~outside & ~inside
    frac = _blockball(x_bgn, y_bgn, z_bgn, r, dx, y_bgn2, z_bgn2, r2, cut, guard)
    c1 = cut & ((x_bgn2 + y_end2) + z_bgn2 < r2)
    frac = frac - _blockball(x_bgn, y_end, z_bgn, r, dx, y_end2, z_bgn2, r2, c1, guard)
    c2 = cut & ((x_bgn2 + y_bgn2) + z_end2 < r2)
    frac = frac - _blockball(x_bgn, y_bgn, z_end, r, dx, y_bgn2, z_end2, r2, c2, guard)
    c3 = c2 & ((x_bgn2 + y_end2) + z_end2 < r2)
    frac = frac + _blockball(x_bgn, y_end, z_end, r, dx, y_end2, z_end2, r2, c3, guard)
    return np.where(outside, 0.0, np.where(inside, dx*dy*dz, frac))


def _split(bgn, length):
    bgn = bgn - (2*bgn + length)*_m(bgn < -length)
    end = bgn + length
    two = (0 < end) & (end < length)
    return (np.where(two, 0.0, bgn), np.where(two, end, length), np.where(two, -bgn, length),
            two)


def _cellball(x_bgn, y_bgn, z_bgn, r, guard):
    one = np.ones_like(x_bgn)
    xb, xl0, xl1, x2 = _split(x_bgn, one)
    yb, yl0, yl1, y2 = _split(y_bgn, one)
    zb, zl0, zl1, z2 = _split(z_bgn, one)
    sx = None
    for ix in range(2):
        sy = None
        for iy in range(2):
            sz = None
            for iz in range(2):
                g = [] if guard is not None else None
                leaf = _leaf(xb, yb, zb, r, xl1 if ix else xl0, yl1 if iy else yl0,
                             zl1 if iz else zl0, g)
                live = (x2 | (ix == 0)) & (y2 | (iy == 0)) & (z2 | (iz == 0))
                if guard is not None:
                    guard.append(live & np.logical_or.reduce(g))
                sz = leaf if iz == 0 else np.where(z2, sz + leaf, sz)
            sy = sz if iy == 0 else np.where(y2, sy + sz, sy)
        sx = sy if ix == 0 else np.where(x2, sx + sy, sx)
    return sx


def overlap_cellshell(ki, kj, kk, k_inner, k_outer, guard=None):
    """get_bispec_overlap_cellshell over arrays (broadcast against each other)"""
    ki, kj, kk, k_inner, k_outer = np.broadcast_arrays(
        *(np.asarray(v, dtype=np.float64) for v in (ki, kj, kk, k_inner, k_outer)))
    return (_cellball(ki - 0.5, kj - 0.5, kk - 0.5, k_outer, guard)
            - _cellball(ki - 0.5, kj - 0.5, kk - 0.5, k_inner, guard))


def near_guard(cases):
    """per row (ki, kj, kk, k_inner, k_outer): does an evaluated xx or yy of the closed form
    lie within GUARD_WINDOW of ±ϵ (an exact zero does not: it is zero in every build)"""
    cases = np.asarray(cases, dtype=np.float64)
    guard = []
    overlap_cellshell(*cases.T, guard=guard)
    return np.logical_or.reduce(guard)


# -- the visited set -----------------------------------------------------------------------------
def shell_rows(N, k_inner, k_outer):
    """(visited, kk_bgn, kk_end) as N x N arrays by array index (a, b): the inclusive kk range
    fourier_shell_loop(N, k_inner, k_outer, skip_origin=True) visits in row (ki, kj), mirrored
    to -ki"""
    nyq = N//2
    k1 = min(int(k_outer + 0.5*math.sqrt(1)), nyq - 1)
    k2d = min(int((k_outer + 0.5*math.sqrt(2))**2), 2*(nyq - 1)**2)
    idx = np.arange(N)
    kvec = idx - np.where(idx >= nyq, N, 0)
    ai, aj = np.meshgrid(np.abs(kvec), np.abs(kvec), indexing='ij')
    ki_lim = np.minimum(np.floor(np.sqrt(np.maximum(k2d - aj**2, 0))).astype(np.int64), k1)
    visited = (aj <= k1) & (aj**2 <= k2d) & (ai <= ki_lim)
    kj_min = (aj + 0.5*(aj != 0))**2
    kj_max = (aj - 0.5*(aj != 0))**2
    ki_min = (ai + 0.5*(ai != 0))**2
    ki_max = (ai - 0.5*(ai != 0))**2
    cmin = k_inner**2 - kj_min - ki_min
    cmax = k_outer**2 - kj_max - ki_max
    bgn = (np.sqrt(cmin*(cmin > 0)) + 0.5).astype(np.int64)
    bgn[(ai == 0) & (aj == 0) & (bgn == 0)] = 1
    end = np.minimum((np.sqrt(cmax*(cmax > 0)) + 0.5).astype(np.int64), k1)
    visited &= bgn <= end
    return visited, bgn, end


def shell_fill(N, shell, antialiasing, source=None):
    """the slab get_bispec_grid transforms: complex F[a, b, kk] of shape (N, N, N//2 + 1)"""
    k_inner, k_outer = shell
    visited, bgn, end = shell_rows(N, k_inner, k_outer)
    nyq = N//2
    idx = np.arange(N)
    kvec = idx - np.where(idx >= nyq, N, 0)
    kk = np.arange(nyq + 1)
    inside = (visited[:, :, None] & (kk[None, None, :] >= bgn[:, :, None])
              & (kk[None, None, :] <= end[:, :, None]))
    a, b, c = np.nonzero(inside)
    frac = np.zeros((N, N, nyq + 1))
    if len(a):
        ki, kj = np.abs(kvec[a]), kvec[b]
        if antialiasing:
            frac[a, b, c] = overlap_cellshell(ki, kj, c, k_inner, k_outer)
        else:
            k2 = kj**2 + ki**2 + c**2
            frac[a, b, c] = (k_inner**2 < k2) & (k2 <= k_outer**2)
    if source is None:
        return frac.astype(np.complex128)
    return frac*np.where(inside, source, 0)


def from_slab(slab):
    """the reference's slab double[b][a][N + 2] as complex F[a, b, kk]"""
    slab = np.asarray(slab)
    return (slab[:, :, 0::2] + 1j*slab[:, :, 1::2]).transpose(1, 0, 2).copy()


def backward(F, N):
    """fft(slab, 'backward'): the unnormalised complex-to-real transform"""
    return np.fft.irfftn(F, s=(N, N, N), axes=(0, 1, 2))*float(N)**3


def sums(grids, want_power):
    """the three cases of compute_bispec_value for 1, 2 or 3 unique grids: (value, powers)"""
    if len(grids) == 3:
        value = np.sum(grids[0]*grids[1]*grids[2])
    elif len(grids) == 2:
        value = np.sum(grids[0]*grids[1]**2)
    else:
        value = np.sum(grids[0]**3)
    return float(value), [float(np.sum(g**2)) if w else 0.0 for g, w in zip(grids, want_power)]


def sums_exact(grids, want_power):
    """the same with math.fsum: the correctly rounded sums of the rounded products"""
    g = [np.asarray(x, dtype=np.float64).ravel() for x in grids]
    if len(g) == 3:
        prod = g[0]*g[1]*g[2]
    elif len(g) == 2:
        prod = g[0]*(g[1]*g[1])
    else:
        prod = g[0]*g[0]*g[0]
    return (math.fsum(prod), [math.fsum(x*x) if w else 0.0 for x, w in zip(g, want_power)],
            math.fsum(np.abs(prod)))


def bispec_value(N, shells, power_dict, F_data=None, antialiasing=True, scale_out=None):
    """compute_bispec_value without the grid cache (which changes no value).  scale_out: a
    dict that receives Σ|g₀g₁g₂|, the scale deviations of the value are measured against."""
    counter = collections.Counter(tuple(s) for s in shells)
    infos = [(shell, mult, backward(shell_fill(N, shell, antialiasing, F_data), N))
             for shell, mult in counter.items()]
    if len(infos) == 2 and infos[0][1] > infos[1][1]:
        infos.reverse()
    want = [power_dict is not None and info[0] not in power_dict for info in infos]
    grids = [info[2] for info in infos]
    value, powers = sums(grids, want)
    if scale_out is not None:
        scale_out['abs'] = sums_exact(grids, [False]*len(grids))[2]
    shells_new = []
    for info, w, pw in zip(infos, want, powers):
        if w:
            power_dict[info[0]] = pw
            shells_new.append(info[0])
    return (value, shells_new) if F_data is None else value


def normalise(N, boxsize, mean_density, bpower_sum, n_modes, power_sums, n_modes_power):
    """analysis.py:3097-3164 for sums already combined over the domains.  bpower_sum, n_modes:
    per bin; power_sums, n_modes_power: 3 x nbins (the bin's shells in the given order).
    Returns (bpower, power, bpower_reduced)."""
    bpower_sum, n_modes = np.asarray(bpower_sum, float), np.asarray(n_modes, float)
    power_sums, n_modes_power = np.asarray(power_sums, float), np.asarray(n_modes_power, float)
    with np.errstate(divide='ignore', invalid='ignore'):
        norm = mean_density**-3*(0.5*boxsize**6)/N**3
        bpower = np.where(n_modes != 0, bpower_sum*(norm/n_modes), np.nan)
        norm = mean_density**-2*(0.5*boxsize**3)/N**3
        power = np.where(n_modes_power != 0, power_sums*(norm/n_modes_power), np.nan)
        reduced = bpower/(power[0]*power[1] + power[1]*power[2] + power[2]*power[0])
    return bpower, power, reduced
