"""Plain numpy references of the two passes of the fluid realisation (cg_realize_grid,
cg_fluid_from_mesh in csrc/cg_lpt.hip), written from the formulas in include/concept_gpu.h.
Fourier slabs are in the layout of PotentialMesh.fetch_fourier(), as in lpt_refs."""
import numpy as np

from lpt_refs import alive, join, split, wave_numbers


def realize_grid(noise, amplitudes, tensor_rank, index0, boxsize):
    """amplitudes[k2]·noise (rank 0) or (amplitudes[k2]·((-boxsize/(2π))·k_index0)/k2)·i·noise
    (rank 1); 0 on the origin and the Nyquist planes"""
    g = noise.shape[0]
    ki, kj, kk = wave_numbers(g)
    k2 = (kj**2 + ki**2) + kk**2
    re, im = split(noise)
    amplitude = np.asarray(amplitudes)[np.minimum(k2, len(amplitudes) - 1)]
    if tensor_rank == 1:
        kl = np.broadcast_to((ki, kj, kk)[index0], k2.shape)
        amplitude = amplitude*(((-boxsize/(2*np.pi))*kl)/np.maximum(k2, 1))
        re, im = -im, re
    live = alive(g)
    return join(np.where(live, amplitude*re, 0.0), np.where(live, amplitude*im, 0.0))


def fluid_from_mesh(field, variable, c0, c1=0.0):
    """variable 0: c0·(1 + v) with v += c1·v² first when c1 ≠ 0; variable 1: v·c0"""
    v = np.asarray(field, dtype=np.float64)
    if variable == 1:
        return v*c0
    if c1 != 0:
        v = v + c1*(v*v)
    return c0*(1 + v)
