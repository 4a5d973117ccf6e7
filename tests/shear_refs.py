"""Plain numpy references of the shear of closure 'class' (cg_realize_grid_tensor,
cg_shear_divergence and cg_fluid_add_from_mesh in csrc/cg_lpt.hip, ic.realize_shear,
fluid.shear_sources), written from the formulas in include/concept_gpu.h.  Fourier slabs are in
the layout of PotentialMesh.fetch_fourier(), as in lpt_refs; real grids are double[i][j][k]."""
import numpy as np

from lpt_refs import alive, join, split, to_fourier, to_real, wave_numbers

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def k2_of(g):
    ki, kj, kk = wave_numbers(g)
    return (kj**2 + ki**2) + kk**2


def table_of(amplitudes, g):
    return np.asarray(amplitudes)[np.minimum(k2_of(g), len(amplitudes) - 1)]


def tensor_factor(g, index0, index1):
    """K = ½[index0 == index1] - ((3/2)·k_index0·k_index1)/k², with k² = 1 at the origin"""
    k = wave_numbers(g)
    shape = k2_of(g).shape
    kl, km = (np.broadcast_to(k[i], shape) for i in (index0, index1))
    return 0.5*(index0 == index1) - ((1.5*kl)*km)/np.maximum(k2_of(g), 1)


def realize_grid_tensor(structure, amplitudes, index0, index1):
    """(amplitudes[k2]·K)·structure; 0 on the origin and the Nyquist planes"""
    g = structure.shape[0]
    amplitude = table_of(amplitudes, g)*tensor_factor(g, index0, index1)
    re, im = split(structure)
    live = alive(g)
    return join(np.where(live, amplitude*re, 0.0), np.where(live, amplitude*im, 0.0))


def lattice_sines(g, boxsize):
    """sⱼ = sin(2π kⱼ/g)/Δx for the three dimensions, broadcastable like wave_numbers"""
    Δx = boxsize/g
    return [np.sin(2*np.pi*k/g)/Δx for k in wave_numbers(g)]


def shear_divergence(structure, amplitudes, dim, boxsize):
    """amplitudes[k2]·i·Σⱼ sⱼ·K_dim,j·structure; 0 on the origin and the Nyquist planes"""
    g = structure.shape[0]
    s = lattice_sines(g, boxsize)
    S = sum(s[j]*tensor_factor(g, dim, j) for j in range(3))
    amplitude = table_of(amplitudes, g)*S
    re, im = split(structure)
    live = alive(g)
    return join(np.where(live, amplitude*-im, 0.0), np.where(live, amplitude*re, 0.0))


def realize_shear(ϱ, amplitudes, index0, index1, c0):
    """ς = c0·ℱ⁻¹[amplitudes·K·ℱ[ϱ]], both transforms unnormalised; c0 = ϱ_bar(1 + w)"""
    return to_real(realize_grid_tensor(to_fourier(ϱ), amplitudes, index0, index1))*c0


def diff2(f, axis, Δx):
    """the order-2 central difference of diff_domaingrid on a periodic grid"""
    return ((1/2)/Δx)*(np.roll(f, -1, axis=axis) - np.roll(f, +1, axis=axis))


def shear_sources_six(ϱ, J, amplitudes, dt, c0, boxsize, ς=None):
    """the reference's route: the six ςₘₙ (or those given, keyed by PAIRS), the potential
    (-dt)·ςₘₙ and Jᵢ += ∂ⱼ potential for every i of {m, n}, j the other index"""
    g = ϱ.shape[0]
    Δx = boxsize/g
    J = np.array(J, dtype=np.float64)
    for m, n in PAIRS:
        ς_mn = ς[m, n] if ς is not None else realize_shear(ϱ, amplitudes, m, n, c0)
        potential = (-dt)*ς_mn
        for i in {m, n}:
            j = n if i == m else m
            J[i] += diff2(potential, j, Δx)
    return J


def shear_sources(ϱ, J, amplitudes, dt, c0, boxsize):
    """the route of fluid.shear_sources: the divergence formed in Fourier space"""
    structure = to_fourier(ϱ)
    J = np.array(J, dtype=np.float64)
    factor = (-dt)*c0
    for i in range(3):
        J[i] += factor*to_real(shear_divergence(structure, amplitudes, i, boxsize))
    return J


def random_density(g, seed=0, contrast=0.3):
    rng = np.random.default_rng(seed)
    return 2.5*(1 + contrast*rng.uniform(-1, 1, (g, g, g)))


def random_table(g, seed=0):
    """a table of σ amplitudes of both signs with the g⁻³ of the transform in it"""
    rng = np.random.default_rng(1000 + seed)
    table = rng.uniform(0.5, 2.0, 3*(g//2 - 1)**2 + 1)*rng.choice([-1.0, 1.0],
                                                                   3*(g//2 - 1)**2 + 1)
    table[0] = 0
    return table*float(g)**(-3)
