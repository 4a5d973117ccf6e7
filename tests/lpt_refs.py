"""Plain numpy references of the LPT passes (csrc/cg_lpt.hip), written from the formulas in
include/concept_gpu.h.  Fourier slabs are in the layout of PotentialMesh.fetch_fourier():
double[j][i][N + 2], (re, im) interleaved along the last axis, kk = 0 .. N/2."""
import numpy as np


def wave_numbers(g):
    """(ki, kj, kk) broadcastable over a slab seen as complex[j][i][N/2 + 1]"""
    k = np.arange(g)
    k = k - g*(k >= g//2)
    return k[None, :, None], k[:, None, None], np.arange(g//2 + 1)[None, None, :]


def alive(g):
    """modes off the origin and the three Nyquist planes"""
    ki, kj, kk = wave_numbers(g)
    nyq = g//2
    return (ki != -nyq) & (kj != -nyq) & (kk != nyq) & ((ki != 0) | (kj != 0) | (kk != 0))


def split(slab):
    return slab[..., 0::2].copy(), slab[..., 1::2].copy()


def join(re, im):
    slab = np.empty(re.shape[:2] + (2*re.shape[2],))
    slab[..., 0::2], slab[..., 1::2] = re, im
    return slab


def potential(noise, amplitudes, shift, factor, boxsize):
    """(amplitudes[k2]·noise·exp(iθ))·((-factor/k_f²)/k2), θ = -2π/N·(k⃗·(-shift)); 0 where dead"""
    g = noise.shape[0]
    ki, kj, kk = wave_numbers(g)
    k2 = kj**2 + ki**2 + kk**2
    re, im = split(noise)
    if tuple(shift) != (0, 0, 0):
        A, B, C = (-2*np.pi/g*-s for s in shift)
        θ = (ki*A + kj*B) + kk*C
        re, im = re*np.cos(θ) - im*np.sin(θ), re*np.sin(θ) + im*np.cos(θ)
    if amplitudes is not None:
        amp = np.asarray(amplitudes)[np.minimum(k2, len(amplitudes) - 1)]
        re, im = amp*re, amp*im
    k_f = 2*np.pi/boxsize
    inv = (-factor/(k_f*k_f))/np.maximum(k2, 1)
    live = alive(g)
    return join(np.where(live, re*inv, 0.0), np.where(live, im*inv, 0.0))


def diff(slab, dim0, dim1, factor, boxsize):
    """i·k_dim0·slab (dim1 = -1) or -k_dim0·k_dim1·slab, times factor; 0 where dead"""
    g = slab.shape[0]
    k = wave_numbers(g)
    k_f = 2*np.pi/boxsize
    re, im = split(slab)
    if dim1 == -1:
        amplitude = (factor*k_f)*k[dim0]
        re, im = amplitude*-im, amplitude*re
    else:
        amplitude = (factor*(k_f*k_f))*k[dim0]*k[dim1]
        re, im = amplitude*-re, amplitude*-im
    live = alive(g)
    return join(np.where(live, re, 0.0), np.where(live, im, 0.0))


def displace(psi, pos, mom, index_bgn, dim, pos_factor, mom_factor):
    """psi: double[g][g][g]; rows index_bgn + (i·g + j)·g + k of copies of pos / mom"""
    pos, mom = pos.copy(), mom.copy()
    n = psi.size
    rows = slice(index_bgn, index_bgn + n)
    if pos_factor != 0:
        pos[rows, dim] = pos[rows, dim] + pos_factor*psi.ravel()
    if mom_factor != 0:
        mom[rows, dim] = mom[rows, dim] + mom_factor*psi.ravel()
    return pos, mom


def to_real(slab):
    """the unnormalised inverse transform of a slab: double[i][j][k]"""
    g = slab.shape[0]
    re, im = split(slab)
    return np.fft.irfftn((re + 1j*im).transpose(1, 0, 2), s=(g, g, g), axes=(0, 1, 2))*g**3


def to_fourier(field):
    """the unnormalised forward transform of double[i][j][k] as a slab"""
    c = np.fft.rfftn(field).transpose(1, 0, 2)
    return join(c.real, c.imag)


def phi2_source(phi1, boxsize):
    """Σ of the six 2LPT terms in real space from the Fourier slab of Φ⁽¹⁾"""
    d = {(i, j): to_real(diff(phi1, i, j, 1.0, boxsize)) for i in range(3) for j in range(i, 3)}
    return (-d[0, 0]*d[1, 1] - d[1, 1]*d[2, 2] - d[2, 2]*d[0, 0]
            + d[0, 1]**2 + d[1, 2]**2 + d[0, 2]**2)
