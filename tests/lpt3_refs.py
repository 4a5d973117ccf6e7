"""Plain numpy references of the passes between the realisation size N and the dealiasing size M
(cg_lpt_diff_enlarge, cg_lpt_dealias_cube, cg_lpt_shrink_accumulate in csrc/cg_lpt.hip), written
from the formulas in include/concept_gpu.h, and the closed forms of the second-order potential of
two plane waves.  Slabs are in the layout of lpt_refs: double[j][i][N + 2]."""
import numpy as np

import lpt_refs


def cube(n_small, n):
    """modes of a grid of size n inside the cube |k| < n_small/2, over complex[j][i][n/2 + 1]"""
    ki, kj, kk = lpt_refs.wave_numbers(n)
    h = n_small//2
    return (np.abs(ki) < h) & (np.abs(kj) < h) & (kk < h)


def resize(slab, n_onto):
    """resize_grid: the modes of the cube |k| < min(N_from, N_onto)/2 rotated by
    θ = (π/N_onto - π/N_from)·((ki + kj) + kk) into a zeroed slab of size n_onto"""
    n_from = slab.shape[0]
    h = min(n_from, n_onto)//2
    k = np.arange(-h + 1, h)
    kj, ki, kk = np.meshgrid(k, k, np.arange(h), indexing='ij')
    re, im = slab[kj % n_from, ki % n_from, 2*kk], slab[kj % n_from, ki % n_from, 2*kk + 1]
    θ = (np.pi/n_onto - np.pi/n_from)*((ki + kj) + kk)
    c, s = np.cos(θ), np.sin(θ)
    out = np.zeros((n_onto, n_onto, n_onto + 2))
    out[kj % n_onto, ki % n_onto, 2*kk] = re*c - im*s
    out[kj % n_onto, ki % n_onto, 2*kk + 1] = re*s + im*c
    return out


def diff_enlarge(slab, n_large, dim0, dim1, factor, boxsize):
    return resize(lpt_refs.diff(slab, dim0, dim1, factor, boxsize), n_large)


def dealias_cube(slab, n_small):
    return np.where(np.repeat(cube(n_small, slab.shape[0]), 2, axis=2), slab, 0.0)


def nyquist_planes(n):
    """the three Nyquist planes over double[j][i][n + 2]"""
    ki, kj, kk = lpt_refs.wave_numbers(n)
    return np.repeat((ki == -(n//2)) | (kj == -(n//2)) | (kk == n//2), 2, axis=2)


def shrink_accumulate(out, slab, operation, factor):
    """out (= | += | -=) factor·resize(slab); on out's Nyquist planes the shrunk grid is zero:
    '=' writes it, '+=' and '-=' leave out as it is"""
    v = resize(slab, out.shape[0])
    if factor != 1:
        v = factor*v
    res = {'=': v, '+=': out + v, '-=': out - v}[operation]
    if operation != '=':
        res = np.where(nyquist_planes(out.shape[0]), out, res)
    return res


def plane_waves(g, boxsize, waves):
    """δ = Σ 2A cos(k⃗·x⃗) on the grid points and Φ⁽¹⁾ = Σ (2A/|k⃗|²) cos(k⃗·x⃗); waves =
    [((mx, my, mz), A)] in grid units"""
    x = np.arange(g)*(boxsize/g)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    k_f = 2*np.pi/boxsize
    phi1 = np.zeros((g, g, g))
    for (mx, my, mz), A in waves:
        phi1 += 2*A/(k_f**2*(mx*mx + my*my + mz*mz))*np.cos(k_f*(mx*X + my*Y + mz*Z))
    return phi1


def phi2_of_two_waves(g, boxsize, waves, alias_to=None, keep_sum=True):
    """Φ⁽²⁾ (D⁽²⁾/(D⁽¹⁾)² = 1) of two plane waves on the grid points: the source of Φ⁽²⁾ is
    -½[(∇²Φ)² - Φ,ᵢⱼΦ,ᵢⱼ] = -½φ₁φ₂|k⃗₁×k⃗₂|²[cos((k⃗₁+k⃗₂)·x⃗) + cos((k⃗₁-k⃗₂)·x⃗)], φ = 2A/|k⃗|², and
    ∇⁻² divides each cosine by -|k⃗|².  alias_to: the grid size on which the sum mode is seen
    (its wave numbers folded into [-N/2, N/2), which is where ∇⁻² then takes its |k⃗|² from);
    keep_sum=False: the sum mode is gone (dealiased)."""
    (m1, A1), (m2, A2) = waves
    k_f = 2*np.pi/boxsize
    m1, m2 = np.array(m1), np.array(m2)
    φ1, φ2 = (2*A/(k_f**2*(m @ m)) for m, A in ((m1, A1), (m2, A2)))
    cross = np.cross(m1, m2)
    strength = 0.5*φ1*φ2*(cross @ cross)*k_f**4
    x = np.arange(g)*(boxsize/g)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    out = np.zeros((g, g, g))
    for m, keep in ((m1 - m2, True), (m1 + m2, keep_sum)):
        if not keep:
            continue
        if alias_to is not None:
            m = (m + alias_to//2) % alias_to - alias_to//2
        out += strength/(k_f**2*(m @ m))*np.cos(k_f*(m[0]*X + m[1]*Y + m[2]*Z))
    return out
