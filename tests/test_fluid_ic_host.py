"""Host side of the fluid realisation (concept_amd/ic.py), no GPU: every refusal of
realize_fluid and realize by its message, the numpy references against each other, the goldens'
own consistency (tests/golden/fluid_ic_*.npz, made by make_golden_fluid_ic.py) and the binding's
new symbols."""
import glob
import os
import types

import numpy as np
import pytest

import fluid_ic_refs
import lpt_refs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(f)[9:-4] for f in glob.glob(os.path.join(GOLDEN,
                                                                         'fluid_ic_*.npz')))


def fake_fluid(params, **kw):
    fields = dict(name='nu', species='matter', representation='fluid', gridsize=8,
                  boltzmann_order=1, params=params, nprocs=1, device='cpu')
    fields.update(kw)
    return types.SimpleNamespace(**fields)


def test_the_goldens_are_all_there():
    assert CASES == sorted(f'{case}_g{g}' for case, sizes in (
        ('plain', (8, 12, 16)), ('nongauss', (8, 12, 16)), ('fixed_shift', (8, 12)),
        ('simple', (8, 12))) for g in sizes)


def test_every_refusal_by_its_message():
    from concept_amd import commons, ic
    from concept_amd.lib import ConceptGPUError
    p = commons.load_params({'boxsize': 10.0})
    amp = np.zeros(28)

    def refuse(message, call):
        with pytest.raises(ConceptGPUError) as e:
            call()
        assert str(e.value) == message
    particles = fake_fluid(p, name='matter', representation='particles')
    refuse('realize_fluid() called with non-fluid component matter',
           lambda: ic.realize_fluid(particles, 0.02, amp))
    for variable in (2, 3):
        refuse(f'nu: realize_fluid() got non-implemented variable = {variable} (ϱ and J are '
               'implemented; ς, δP and the "class" closure are not)',
               lambda: ic.realize_fluid(fake_fluid(p, boltzmann_order=2), 0.02, amp, variable))
    refuse('nu: fluid variable 1 exceeds the Boltzmann order 0 of the component (realisation '
           'from the "class" closure is not implemented)',
           lambda: ic.realize_fluid(fake_fluid(p, boltzmann_order=0), 0.02, amp, 1, 0))
    refuse("nu: realize_fluid() of J needs multi_index 0, 1 or 2, not 3",
           lambda: ic.realize_fluid(fake_fluid(p), 0.02, amp, 1, 3))
    refuse('nu: realize_fluid() with an active comm process group: multi-GPU realisation is '
           'not implemented', lambda: ic.realize_fluid(fake_fluid(p, nprocs=2), 0.02, amp))
    refuse('nu: (27,) amplitudes for a fluid grid of 8³ cells, which needs '
           '3*(nyquist - 1)**2 + 1 = 28',
           lambda: ic.realize_fluid(fake_fluid(p), 0.02, np.zeros(27)))
    refuse('nu: J comes from the amplitudes of θ: pass amplitudes_θ',
           lambda: ic.realize(fake_fluid(p), 0.02, amp))
    refuse("nu: realize() of a fluid component takes no ['growth_factors']",
           lambda: ic.realize(fake_fluid(p), 0.02, amp, amp, growth_factors={}))


def test_realize_hands_particles_to_realize_particles(monkeypatch):
    from concept_amd import commons, ic
    p = commons.load_params({'boxsize': 10.0})
    seen = []
    monkeypatch.setattr(ic, 'realize_particles', lambda *a, **kw: seen.append((a, kw)) or 'grids')
    c = fake_fluid(p, representation='particles')
    assert ic.realize(c, 0.02, 'δ', 'θ', growth_factors={'D1': 1}) == 'grids'
    assert seen == [((c, 0.02, 'δ', 'θ'), {'growth_factors': {'D1': 1}})]


@pytest.mark.parametrize('case', CASES)
def test_the_references_reproduce_the_golden(golden, case):
    """realize_grid and fluid_from_mesh in numpy, numpy's inverse transform between them, give
    the reference's ϱ and J from the recorded noise: the two restatements the GPU tests compare
    the kernels with are the reference's arithmetic"""
    g = golden('fluid_ic_' + case)
    L, ϱ_bar = float(g['boxsize']), float(g['rho_bar'])
    assert float(g['J_factor']) == float(g['a'])**(1 - 3*float(g['w_eff']))*ϱ_bar*(1 + float(g['w']))
    δ = lpt_refs.to_real(fluid_ic_refs.realize_grid(g['noise'], g['amplitudes'], 0, 0, L))
    ϱ = fluid_ic_refs.fluid_from_mesh(δ, 0, ϱ_bar, float(g['nongaussianity']))
    assert np.abs(ϱ - g['rho']).max() <= 1e-12*ϱ_bar
    for i in range(3):
        u = lpt_refs.to_real(fluid_ic_refs.realize_grid(g['noise'], g['amplitudes_θ'], 1, i, L))
        J = fluid_ic_refs.fluid_from_mesh(u, 1, float(g['J_factor']))
        assert np.abs(J - g['J'][i]).max() <= 1e-12*np.abs(g['J'][i]).max()
    assert g['rho'].min() > 0


def test_the_new_symbols_are_bound():
    from concept_amd import lib
    for name in ('cg_realize_grid', 'cg_fluid_from_mesh'):
        assert name in lib.SYMBOLS and hasattr(lib.raw(), name)
