"""The fluid realisation on the GPU (cg_realize_grid and cg_fluid_from_mesh in csrc/cg_lpt.hip,
ic.realize_fluid and ic.realize): each kernel against the plain numpy references of
tests/fluid_ic_refs.py, the whole realisation against the reference's own
(tests/golden/fluid_ic_*.npz), a plane wave in closed form, and the hand-over to the time loop.

Bars.  cg_realize_grid evaluates the reference's expression in the reference's order and has no
phase: 1e-14 of the largest value (the bar of test_gpu_lpt.py for such a kernel), the scalar case
bit for bit.  cg_fluid_from_mesh rounds every product and sum in turn: bit-identical.  Everything
that goes through the transforms: the project's 1e-12 — of ϱ_bar for ϱ, of max |Jⁱ| for Jⁱ."""
import glob
import os

import numpy as np
import pytest

import fluid_ic_refs
import lpt_refs
from test_gpu_lpt import close, dev, meshes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(f)[9:-4] for f in glob.glob(os.path.join(GOLDEN,
                                                                         'fluid_ic_*.npz')))
L = 100.0


def random_inputs(g):
    """a slab that is dense also where the kernel must write zeros, and two tables without zeros"""
    rng = np.random.default_rng(g)
    return (rng.normal(size=(g, g, g + 2)), rng.uniform(0.5, 2.0, 3*(g//2 - 1)**2 + 1),
            rng.uniform(-2.0, -0.5, 3*(g//2 - 1)**2 + 1))


# ---- cg_realize_grid ----------------------------------------------------------------------------
@pytest.mark.parametrize('gridsize', [8, 12, 16])
def test_realize_grid_against_numpy(gridsize):
    g, nyq = gridsize, gridsize//2
    slab, amp, _ = random_inputs(g)
    noise, out = meshes(g, 2)
    noise.upload_fourier(slab)
    for rank, index in ((0, 0), (1, 0), (1, 1), (1, 2)):
        out.upload_fourier(np.full_like(slab, 7.0))
        out.realize_grid(noise, dev(amp), rank, index)
        got = out.fetch_fourier()
        assert close(got, fluid_ic_refs.realize_grid(slab, amp, rank, index, L), 1e-14), (rank, index)
        # the origin and every Nyquist plane are exactly 0.0
        assert not got[0, 0, :2].any()
        assert not got[nyq].any() and not got[:, nyq].any() and not got[:, :, 2*nyq:].any()
        if rank == 0:
            ki, kj, kk = lpt_refs.wave_numbers(g)
            table = amp[np.minimum(ki**2 + kj**2 + kk**2, amp.size - 1)]
            live = np.repeat(lpt_refs.alive(g), 2, axis=2)
            assert np.array_equal(got, np.where(live, np.repeat(table, 2, axis=2)*slab, 0.0))
    assert np.array_equal(noise.fetch_fourier(), slab)
    # in place
    noise.realize_grid(noise, dev(amp), 1, 2)
    assert close(noise.fetch_fourier(), fluid_ic_refs.realize_grid(slab, amp, 1, 2, L), 1e-14)


def test_realize_grid_refusals():
    from concept_amd.lib import ConceptGPUError
    a, b = meshes(8, 2)
    with pytest.raises(ConceptGPUError, match=r'27 amplitudes for grid size 8, which needs '
                                              r'3\*\(nyquist - 1\)\*\*2 \+ 1 = 28'):
        a.realize_grid(b, dev(np.zeros(27)))
    with pytest.raises(ConceptGPUError, match=r'tensor rank 2 \(0 and 1 are implemented\)'):
        a.realize_grid(b, dev(np.zeros(28)), 2)
    with pytest.raises(ConceptGPUError, match=r'index 3 not in \{0, 1, 2\}'):
        a.realize_grid(b, dev(np.zeros(28)), 1, 3)
    c, = meshes(12, 1)
    with pytest.raises(ConceptGPUError, match='differ in grid size or domain'):
        a.realize_grid(c, dev(np.zeros(28)))


@pytest.mark.parametrize('gridsize', [8, 12, 16])
def test_the_divergence_of_the_vector_realisation_is_the_scalar_one(gridsize):
    """Σᵢ i·k_f·kᵢ·ûⁱ(k) with ûⁱ = amplitude·(-i kⁱ/(k_f k²))·noise is amplitude·noise mode by
    mode: all three index branches, the sign of the rotation and the hoisted constant"""
    g = gridsize
    slab, _, amp_θ = random_inputs(g)
    noise, out = meshes(g, 2)
    noise.upload_fourier(slab)
    k_f = 2*np.pi/L
    div_re, div_im = 0.0, 0.0
    for index, k in enumerate(lpt_refs.wave_numbers(g)):
        re, im = lpt_refs.split(out.realize_grid(noise, dev(amp_θ), 1, index).fetch_fourier())
        div_re, div_im = div_re + (k_f*k)*-im, div_im + (k_f*k)*re
    scalar = out.realize_grid(noise, dev(amp_θ), 0).fetch_fourier()
    assert np.abs(scalar).max() > 0
    assert close(lpt_refs.join(div_re, div_im), scalar, 1e-14)


# ---- cg_fluid_from_mesh --------------------------------------------------------------------------
@pytest.mark.parametrize('gridsize', [12, 16])
def test_fluid_from_mesh_is_bit_identical(gridsize):
    """the mesh's padding (and the unused row of a layer at 16) is NaN: never read; the
    destination starts as a sentinel: every cell is written"""
    import torch
    rng = np.random.default_rng(gridsize)
    g = gridsize
    mesh, = meshes(g, 1)
    rows = mesh.layer_doubles//mesh.pad
    field = 0.3*rng.normal(size=(g, g, g))
    native = np.full((g, rows, mesh.pad), np.nan)
    native[:, :g, :g] = field
    mesh.layers_write(0, g, dev(native))
    sentinel = -1.25e300
    for variable, c0, c1 in ((0, 4.07, 0.0), (0, 4.07, 0.5), (0, 4.07, -1.75), (1, 0.0816, 0.0)):
        out = torch.full((g, g, g), sentinel, dtype=torch.float64, device='cuda')
        mesh.fluid_from_mesh(out, variable, c0, c1)
        got = out.cpu().numpy()
        assert np.isfinite(got).all() and not (got == sentinel).any()
        assert np.array_equal(got, fluid_ic_refs.fluid_from_mesh(field, variable, c0, c1)), (
            variable, c0, c1)
    from concept_amd.lib import ConceptGPUError
    with pytest.raises(ConceptGPUError, match='fluid grids must be contiguous float64 tensors'):
        mesh.fluid_from_mesh(torch.zeros((g, g, g - 1), dtype=torch.float64, device='cuda'), 0, 1.0)
    with pytest.raises(ConceptGPUError, match=r'mode 2 not in'):
        mesh.fluid_from_mesh(torch.zeros((g, g, g), dtype=torch.float64, device='cuda'), 2, 1.0)


# ---- end to end ----------------------------------------------------------------------------------
def fluid_component(g, boltzmann_order=1):
    from concept_amd.species import Component
    return Component('matter', 'matter', gridsize=int(g['gridsize']),
                     boltzmann_order=boltzmann_order)


@pytest.mark.parametrize('case', CASES)
def test_realize_against_the_golden(golden, case):
    from concept_amd import commons, ic
    g = golden('fluid_ic_' + case)
    commons.load_params(str(g['param_text']))
    a, ϱ_bar = float(g['a']), float(g['rho_bar'])
    c = fluid_component(g)
    assert c.ϱ_bar == pytest.approx(ϱ_bar, rel=1e-14)
    assert (c.w(a=a), c.w_eff(a=a)) == (float(g['w']), float(g['w_eff']))
    assert ic.realization_options(c)['nongaussianity'] == float(g['nongaussianity'])
    noise = ic.realize(c, a, g['amplitudes'], g['amplitudes_θ'])
    ϱ, J = c.host('ϱ'), c.host('J')
    live = np.repeat(lpt_refs.alive(int(g['gridsize'])), 2, axis=2)
    assert np.array_equal(noise.fetch_fourier()*live, g['noise'])
    e = np.abs(ϱ - g['rho']).max()/ϱ_bar
    print(f'{case}: ϱ within {e:.3e} of ϱ_bar')
    assert e <= 1e-12
    for i in range(3):
        e = np.abs(J[i] - g['J'][i]).max()/np.abs(g['J'][i]).max()
        print(f'{case}: J[{i}] within {e:.3e} of max |J[{i}]|')
        assert e <= 1e-12
    assert not c.host('𝒫').any()  # w = 0
    # a second run gives the same bits
    c2 = fluid_component(g)
    ic.realize(c2, a, g['amplitudes'], g['amplitudes_θ'])
    assert np.array_equal(c2.host('ϱ'), ϱ) and np.array_equal(c2.host('J'), J)
    # ϱ alone for a component without J
    c0 = fluid_component(g, boltzmann_order=0)
    ic.realize(c0, a, g['amplitudes'])
    assert np.array_equal(c0.host('ϱ'), ϱ) and not c0.host('J').any()


def test_pressure_and_the_momentum_factor_with_a_constant_w(golden):
    """w = 0.1: 𝒫 = c²wϱ to the bit, J carries a**(1 - 3w)·(1 + w), ϱ is as for w = 0"""
    from concept_amd import commons, ic
    g = golden('fluid_ic_plain_g12')
    w, a = 0.1, float(g['a'])
    p = commons.load_params(str(g['param_text']) + f"select_eos_w = {{'all': {w}}}\n"
                            "select_approximations = {'all': {'P=wρ': True}}\n")
    c = fluid_component(g)
    assert c.w(a=a) == w
    ic.realize(c, a, g['amplitudes'], g['amplitudes_θ'])
    ϱ, J, 𝒫 = c.host('ϱ'), c.host('J'), c.host('𝒫')
    assert np.abs(ϱ - g['rho']).max() <= 1e-12*float(g['rho_bar'])
    assert np.array_equal(𝒫, ϱ*(p.light_speed**2*w)) and 𝒫.min() > 0
    factor = a**(1 - 3*w)*c.ϱ_bar*(1 + w)
    ref = g['J']/float(g['J_factor'])*factor
    assert np.abs(J - ref).max() <= 1e-12*np.abs(ref).max()


@pytest.mark.parametrize('gridsize', [12, 16])
def test_a_plane_wave_in_closed_form(gridsize):
    """noise = A·exp(iφ) in the one mode k = (2, -1, 3): δ = 2·amp_δ·A·cos(k·x + φ) and
    uⁱ = 2·amp_θ·A·(boxsize/(2π))·(kⁱ/k²)·sin(k·x + φ), a quarter period behind and along k"""
    from concept_amd import commons, ic
    from concept_amd.species import Component
    g = gridsize
    commons.load_params({'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25})
    c = Component('matter', 'matter', gridsize=g, boltzmann_order=1)
    k, A, φ, a = (2, -1, 3), 0.8, 0.6, 0.05
    k2 = sum(q*q for q in k)
    slab = np.zeros((g, g, g + 2))
    slab[k[1] % g, k[0] % g, 2*k[2]:2*k[2] + 2] = A*np.cos(φ), A*np.sin(φ)
    rng = np.random.default_rng(1)
    amp, amp_θ = (rng.uniform(0.01, 0.02, 3*(g//2 - 1)**2 + 1) for _ in range(2))
    noise, = meshes(g, 1)
    noise.upload_fourier(slab)
    assert ic.realize_fluid(c, a, amp, 0, noise=noise) is noise
    for i in range(3):
        ic.realize_fluid(c, a, amp_θ, 1, i, noise=noise)
    n = np.arange(g)
    phase = 2*np.pi/g*(k[0]*n[:, None, None] + k[1]*n[None, :, None] + k[2]*n[None, None, :]) + φ
    ϱ_ref = c.ϱ_bar*(1 + 2*amp[k2]*A*np.cos(phase))
    assert np.abs(c.host('ϱ') - ϱ_ref).max() <= 1e-12*c.ϱ_bar
    J = c.host('J')
    for i in range(3):
        ref = (a*c.ϱ_bar)*2*amp_θ[k2]*A*(L/(2*np.pi))*(k[i]/k2)*np.sin(phase)
        assert np.abs(ref).max() > 0
        assert np.abs(J[i] - ref).max() <= 1e-12*np.abs(ref).max()


# ---- hand-over -----------------------------------------------------------------------------------
def test_a_realised_fluid_and_particles_take_a_time_loop_step():
    """from a P(k) table to Timeloop: a 16³ particle component (realize_particles through
    realize) and a 16³ fluid (realize) on the same noise, base steps with fluid.drift and PM
    gravity: ϱ stays positive and finite, Σϱ is conserved to rounding (1e-13 of Σϱ, the bar of
    the drift's own time-loop tests)"""
    from concept_amd import commons, fluid, ic, stepper
    from concept_amd.species import Component
    g = 16
    p = commons.load_params({
        'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02,
        'output_times': {'a': (0.0202,)}, 'enable_Hubble': True,
        'potential_options': {'gridsize': {'gravity': {'pm': g}}},
        'select_forces': {'all': {'gravity': 'pm'}},
        'realization_options': {'backscale': True}})
    k = np.geomspace(1e-3, 10, 200)
    amplitudes = 0.1*ic.amplitudes_from_power(k, 2e3*k/(1 + (k/0.1)**2)**1.5, g, L)
    part = Component('matter', 'matter', N=g**3, mass=-1)
    ic.reset_tally()
    ic.realize(part, p.a_begin, amplitudes, growth_factors={'D1': 0.02, 'f1': 1.0})
    assert np.abs(part.host('mom')).max() > 0
    fl = Component('matter fluid', 'matter', gridsize=g, boltzmann_order=1)
    ic.realize(fl, p.a_begin, amplitudes, -amplitudes)
    ϱ0, J0 = fl.host('ϱ'), fl.host('J')
    assert ϱ0.min() > 0 and ϱ0.std() > 1e-3*fl.ϱ_bar and np.abs(J0).max() > 0
    assert abs(ϱ0.mean()/fl.ϱ_bar - 1) <= 1e-12
    fluid.reset_steps()
    steps = []
    loop = stepper.Timeloop([part, fl], fluid_drift=fluid.drift, fluid_limiter=fluid.courant_limit,
                            on_step=lambda lp: steps.append(lp.cosmo.a))
    loop.run()
    assert len(steps) >= 1
    ϱ = fl.host('ϱ')
    assert np.isfinite(ϱ).all() and ϱ.min() > 0 and not np.array_equal(ϱ, ϱ0)
    assert np.isfinite(fl.host('J')).all() and np.isfinite(part.host('mom')).all()
    print(f'{len(steps)} base steps, Σϱ {ϱ0.sum():.15e} -> {ϱ.sum():.15e}')
    assert abs(ϱ.sum() - ϱ0.sum()) <= 1e-13*ϱ0.sum()
    fluid.reset_steps()
