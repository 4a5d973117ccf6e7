"""Host side of the particle realisation (concept_amd/ic.py), no GPU: the primordial noise and
the lattice against the reference's (tests/golden/lpt_*.npz, made by make_golden_lpt.py), the
amplitude table against its formula, every refusal by its message, the binding's new symbols."""
import glob
import os
import types

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, 'lpt_*.npz')))


def load(golden, case):
    from concept_amd import commons
    g = golden('lpt_' + case)
    return g, commons.load_params(str(g['param_text']))


def test_the_golden_cases_are_all_there():
    names = {'1lpt', '1lpt_backscale', '2lpt', '2lpt_bcc2', '1lpt_fixed_shift', '2lpt_vertex',
             '1lpt_simple'}
    assert set(CASES) == {f'{name}_g{g}' for name in names for g in (8, 12)}


@pytest.mark.parametrize('case', CASES)
def test_noise_is_the_reference_noise_bit_for_bit(golden, case):
    """both imprinting schemes, fixed amplitude, phase shift: equal streams, equal scatter"""
    from concept_amd import ic
    g, p = load(golden, case)
    noise = ic.generate_primordial_noise(int(g['gridsize']), p.primordial_amplitude_fixed,
                                         p.primordial_phase_shift)
    assert noise.shape == g['noise'].shape and np.array_equal(noise, g['noise'])
    if p.primordial_amplitude_fixed:
        re, im = noise[..., 0::2], noise[..., 1::2]
        r = np.hypot(re, im)
        assert np.abs(r[r > 0] - 1).max() <= 4e-16


@pytest.mark.parametrize('scheme', ['distributed', 'simple'])
@pytest.mark.parametrize('gridsize', [6, 8, 12])
def test_noise_zdc_plane_is_hermitian_and_the_origin_zero(scheme, gridsize):
    from concept_amd import commons, ic
    commons.load_params({'boxsize': 10.0, 'primordial_noise_imprinting': scheme})
    noise = ic.generate_primordial_noise(gridsize)
    z = noise[..., 0] + 1j*noise[..., 1]          # kk = 0: z[j][i]
    assert z[0, 0] == 0
    nyq = gridsize//2
    k = np.arange(-nyq + 1, nyq)
    for kj in k:
        for ki in k:
            assert z[kj % gridsize, ki % gridsize] == np.conj(z[-kj % gridsize, -ki % gridsize])
    # every other mode off the Nyquist planes has been drawn; the planes themselves are zero
    c = noise[..., 0::2] + 1j*noise[..., 1::2]
    alive = np.ones(c.shape, dtype=bool)
    alive[nyq], alive[:, nyq], alive[:, :, nyq] = False, False, False
    alive[0, 0, 0] = False
    assert np.all(c[alive] != 0) and np.all(c[~alive] == 0)


def test_noise_of_a_larger_grid_keeps_the_inner_modes():
    """the point of the curve's order: enlarging the grid adds a shell, nothing else"""
    from concept_amd import commons, ic
    commons.load_params({'boxsize': 10.0})
    small, large = ic.generate_primordial_noise(6), ic.generate_primordial_noise(10)
    for kj in range(-2, 3):
        for ki in range(-2, 3):
            assert np.array_equal(small[kj % 6, ki % 6, :6], large[kj % 10, ki % 10, :6])


def test_generator_draws_equal_single_draws():
    from concept_amd import commons, ic
    commons.load_params({'boxsize': 10.0})
    a = ic.PseudoRandomNumberGenerator(1000, cache_size=7).spawn(2**32 - 3)
    b = ic.PseudoRandomNumberGenerator(1000, cache_size=7).spawn(2**32 - 3)
    bulk = a.rayleigh(0.5, 23)
    single = np.array([b.rayleigh(0.5)[0] for _ in range(23)])
    assert np.array_equal(bulk, single)
    # salted seed, spawn keys and stream as stated
    seq = np.random.SeedSequence(1000 + int(np.pi*1e+8) + 137, spawn_key=(2**32 - 3,))
    raw = np.random.Generator(np.random.PCG64DXSM(seq)).rayleigh(1, size=7)
    assert np.array_equal(bulk[:7], raw*0.5)


class FakeComponent(types.SimpleNamespace):
    def __init__(self, params, n, **kw):
        import torch
        self._arrays = dict(pos=torch.zeros((n, 3), dtype=torch.float64),
                            mom=torch.ones((n, 3), dtype=torch.float64),
                            ids=torch.zeros(n, dtype=torch.int64))
        fields = dict(name='matter', species='matter', representation='particles', N=n,
                      N_local=n, params=params, mass=-1, nprocs=1, **self._arrays)
        fields.update(kw)
        super().__init__(**fields)


@pytest.mark.parametrize('case', CASES)
def test_lattice_positions_and_ids_are_the_reference_ones(golden, case):
    """preinitialize_particles (on CPU tensors here: the same torch expressions)"""
    from concept_amd import ic
    g, p = load(golden, case)
    n, N = int(g['gridsize']), int(g['gridsize'])**3
    shift = (0, 0, 0)
    if int(g['components_total']) == 2:
        shift = ic.lattice_shifts('bcc', p.cell_centered)[int(g['components_tally'])]
        assert shift == (-0.5,)*3
    c = FakeComponent(p, N)
    assert ic.preinitialize_particles(c, N, 0, int(g['id_bgn']), shift) == N
    assert np.array_equal(c.ids.numpy(), g['ids'])
    assert not c.mom.any()
    pos = c.pos.numpy().reshape(n, n, n, 3)
    for i in (0, 1, n - 1):
        expected = ((0 + 0.5*p.cell_centered + shift[0]) + i)*(p.boxsize/n)
        assert pos[i, 2, 3, 0] == expected and pos[2, i, 3, 1] == expected
        assert pos[2, 3, i, 2] == expected
    assert np.array_equal(c.pos.numpy(), g['pos_lattice'])


def test_lattice_shifts_and_kinds():
    from concept_amd import ic
    assert ic.lattice_shifts('fcc', True) == [(0, 0, 0), (0, -.5, -.5), (-.5, 0, -.5),
                                              (-.5, -.5, 0)]
    assert ic.lattice_shifts('bcc', False) == [(0, 0, 0), (.5, .5, .5)]
    assert [ic.preic_lattice(n) for n in (8**3, 2*8**3, 4*8**3, 3*8**3, 1000)] == \
        ['sc', 'bcc', 'fcc', '', 'sc']


def test_wrap_positions_is_the_reference_mod():
    import torch
    from concept_amd import ic
    L = 100.0
    x = np.array([0.0, -0.0, 5.0, L, -1e-20, -3.5, L + 2.25, np.nextafter(L, 0), 2*L, -L])
    got = ic.wrap_positions(torch.from_numpy(x.copy()), L).numpy()
    ref = np.mod(x, L)
    ref[ref == L] = 0
    assert np.array_equal(got, ref) and np.all((got >= 0) & (got < L))


def test_amplitudes_from_power_formula():
    from concept_amd import ic
    L, g = 200.0, 12
    k = np.geomspace(1e-3, 10, 400)
    P = 3e4*k**0.96/(1 + (k/0.02)**2)**1.3
    amp = ic.amplitudes_from_power(k, P, g, L)
    nyq = g//2
    assert amp.shape == (3*(nyq - 1)**2 + 1,) and amp[0] == 0
    k_f = 2*np.pi/L
    for k2 in (1, 2, 17, 3*(nyq - 1)**2):
        kmag = k_f*np.sqrt(k2)
        i = np.searchsorted(k, kmag)
        t = (np.log(kmag) - np.log(k[i - 1]))/(np.log(k[i]) - np.log(k[i - 1]))
        logP = (1 - t)*np.log(P[i - 1]) + t*np.log(P[i])
        assert amp[k2] == pytest.approx(np.sqrt(np.exp(logP))*L**-1.5, rel=1e-13)
    # a power law is interpolated exactly in log-log
    amp = ic.amplitudes_from_power(k, 7*k**-2.0, g, L)
    k2 = np.arange(1, amp.size)
    assert np.allclose(amp[1:], np.sqrt(7*(k_f*np.sqrt(k2))**-2.0)*L**-1.5, rtol=1e-13, atol=0)
    from concept_amd.lib import ConceptGPUError
    with pytest.raises(ConceptGPUError, match='the table covers k in'):
        ic.amplitudes_from_power(k[200:], P[200:], g, L)


def test_every_refusal_by_its_message():
    from concept_amd import commons, ic
    from concept_amd.lib import ConceptGPUError
    amp = np.zeros(28)

    def refuse(message, n=512, comp=None, **options):
        p = commons.load_params({'boxsize': 10.0, 'realization_options': options})
        c = FakeComponent(p, n, **(comp or {}))
        with pytest.raises(ConceptGPUError) as e:
            ic.realize_particles(c, 0.02, amp, amp)
        assert str(e.value) == message
    refuse('matter: realization_options["lpt"] = 3: 3LPT is not implemented (1LPT and 2LPT are)',
           lpt=3)
    refuse('matter: realize_particles() called with attempted 4LPT, though only 1LPT and 2LPT '
           'are implemented', lpt=4)
    refuse('matter: realization_options["dealias"]: Orszag dealiasing of the LPT products is '
           'not implemented', dealias=True)
    refuse('matter: realization_options["nongaussianity"] = 0.5: non-Gaussian initial '
           'conditions are not implemented', nongaussianity=0.5)
    refuse('matter: Can only realize particles using the primordial structure, not "nonlinear"',
           structure='non-linear')
    refuse('matter: realize_particles() called with a non-particle component (fluid realisation '
           'is not implemented)', comp={'representation': 'fluid'})
    refuse('Cannot initialize particle component matter with N = 1536 on a lattice, as neither '
           'of {N, N/2, N/4} is a cubic number', n=1536)
    refuse('matter: realize_particles() with an active comm process group: multi-GPU '
           'realisation is not implemented', comp={'nprocs': 2})
    # the options are looked up per component
    p = commons.load_params({'boxsize': 10.0, 'realization_options': {'LPT': {'matter': 3}}})
    assert ic.realization_options(FakeComponent(p, 8))['lpt'] == 3
    assert p.random_seeds == {'general': 0, 'primordial amplitudes': 1000,
                              'primordial phases': 2000}
    assert p.random_generator == 'PCG64DXSM' and p.primordial_noise_imprinting == 'distributed'
    assert {k: v['default'] for k, v in commons.load_params({}).realization_options.items()} == {
        'backscale': False, 'lpt': 1, 'dealias': False, 'nongaussianity': 0.0,
        'structure': 'primordial'}
    with pytest.raises(ValueError, match='not understood'):
        commons.load_params({'random_seeds': {'noise': 3}})


def test_the_new_symbols_are_bound():
    from concept_amd import lib
    for name in ('cg_lpt_potential', 'cg_lpt_diff', 'cg_lpt_product', 'cg_lpt_displace'):
        assert name in lib.SYMBOLS and hasattr(lib.raw(), name)
    assert lib.raw().cg_abi_version() == 2
