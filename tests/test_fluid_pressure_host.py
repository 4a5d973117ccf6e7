"""Host-side tests of the pressure term of concept_amd.fluid (no GPU): a NumPy restatement of the
realisation 𝒫 = ϱ c²w (ic.py:503-508) and of the pressure term of maccormack_internal_sources
(fluid.py:1044-1057, mesh.py:4966-4970; np.roll for the periodic neighbours, the reference's
parentheses) bit-compared to the goldens of tests/golden/make_golden_fluid_pressure.py; the new
parameters, Component.w / w_eff / approximations, the sound speed in v_max, the Timeloop refusal
and the step integrals of a w = 0.2 component.  The GPU tests (test_gpu_fluid_pressure.py) import
the restatement from here."""
import types
import warnings

import numpy as np
import pytest

from test_fluid_host import RTOL, STEP_TRIPLES, close, load, maccormack_np, settings_of

W = 0.2


# -- the NumPy restatement -----------------------------------------------------------------------
def realize_np(ϱ, c2w):
    return ϱ*c2w


def sources_np(ϱ, J, c2w, dt, Δx):
    """(𝒫, J) after realize_if_linear(2, 'trace') and the pressure term with
    ᔑdt['a**(-3*w_eff)'] = dt; J stacked (3, g, g, g)"""
    𝒫 = realize_np(ϱ, c2w)
    J = np.array(J, dtype=np.float64)
    for i in range(3):
        source = ((1/2)/Δx)*(np.roll(𝒫, -1, axis=i) - np.roll(𝒫, +1, axis=i))
        J[i] += (-dt)*source
    return 𝒫, J


def c2w_of(g):
    return float(g['light_speed'])**2*float(g['w'])


# -- the restatement against the goldens ---------------------------------------------------------
def test_restatement_reproduces_the_sources_golden_bit_for_bit():
    g = load('fluid_pressure_sources_g8')
    assert float(g['w']) == W
    ϱ, J = g['rho_in'], g['J_in']
    Δx = float(g['boxsize'])/int(g['gridsize'])
    for i, dt in enumerate(g['dt']):
        J_before = J
        𝒫, J = sources_np(ϱ, J, c2w_of(g), float(dt), Δx)
        # the generator's own guard: the source is no small part of J
        assert np.abs(g[f'J_{i}'] - J_before).max() >= 0.1*np.abs(J_before).max()
        assert np.array_equal(𝒫, g[f'P_{i}']) and np.array_equal(J, g[f'J_{i}']), i


def test_restatement_reproduces_the_sources_and_drifts_of_the_kdk_golden():
    g = load('fluid_pressure_kdk_g8')
    st = settings_of(g)
    keys = list(g['keys'])
    Δx = st['boxsize']/int(g['gridsize'])
    values = [g[f'dt_{r}'] for r in range(3)]
    # every key has a value of its own in every round
    assert all(len(set(v)) == len(keys) for v in values)
    worst = 0.0
    for r in range(3):
        dt = dict(zip(keys, map(float, values[r])))
        ϱ, J = (g['rho_in'], g['J_in']) if r == 0 else (g[f'rho_{r - 1}'], g[f'J_{r - 1}'])
        𝒫, J = sources_np(ϱ, J, c2w_of(g), dt['a**(-3*w_eff)'], Δx)
        assert np.array_equal(g[f'rho_src_{r}'], ϱ)
        assert np.array_equal(𝒫, g[f'P_src_{r}']) and np.array_equal(J, g[f'J_src_{r}']), r
        # the kick leaves ϱ alone; the drift re-realises 𝒫 before its first step and keeps it
        assert np.array_equal(g[f'rho_kick_{r}'], ϱ)
        assert np.array_equal(g[f'P_{r}'], realize_np(g[f'rho_kick_{r}'], c2w_of(g)))
        ϱ, J = maccormack_np(g[f'rho_kick_{r}'], g[f'J_kick_{r}'], g[f'P_{r}'],
                             dt['a**(3*w_eff-2)'], STEP_TRIPLES[r], st)
        worst = max(worst, close(ϱ, g[f'rho_{r}']), close(J, g[f'J_{r}']))
    print('restatement vs reference, kdk drifts with pressure:', worst)
    assert worst <= RTOL
    assert float(g['margin']) >= 1e-6


# -- parameters and Component --------------------------------------------------------------------
def fluid_like(name='fl', species='matter'):
    return types.SimpleNamespace(name=name, species=species, representation='fluid')


def test_eos_and_approximation_parameters():
    from concept_amd import commons
    p = commons.load_params({'boxsize': 8.0})
    assert commons.is_selected(fluid_like(), p.select_eos_w) == 0.0
    assert commons.is_selected(fluid_like(), p.select_boltzmann_closure) == 'truncate'
    assert commons.is_selected(fluid_like(), p.select_approximations, accumulate=True) == {
        'P=wρ': False}
    p = commons.load_params({'boxsize': 8.0, 'select_eos_w': {'matter': 0.2, 'nu': 1/3}})
    assert commons.is_selected(fluid_like(), p.select_eos_w) == 0.2
    assert commons.is_selected(fluid_like('nu', 'neutrino'), p.select_eos_w) == 1/3
    assert commons.is_selected(fluid_like('other', 'neutrino'), p.select_eos_w) == 0.0
    p = commons.load_params({'boxsize': 8.0, 'select_eos_w': 0.25})
    assert commons.is_selected(fluid_like(), p.select_eos_w) == 0.25
    # a bare {approximation: value} dict applies to all components (commons.py:3855-3857)
    p = commons.load_params("select_approximations = {'P = wρ': True}\n"
                            "select_boltzmann_closure = {'matter': 'Truncate'}\n")
    assert p.select_approximations['all'] == {'P = wρ': True}
    assert commons.is_selected(fluid_like(), p.select_boltzmann_closure) == 'truncate'
    for bad in ('class', 'default', '0.3*a', 'w.dat', None, True):
        with pytest.raises(ValueError, match='not implemented'):
            commons.load_params({'boxsize': 8.0, 'select_eos_w': {'matter': bad}})


class FakeComponent:
    """species.Component._init_eos on an object without GPU buffers"""

    def __init__(self, params, name='fl', species='matter', representation='fluid',
                 boltzmann_order=1):
        from concept_amd.species import Component
        self.params, self.name, self.species = params, name, species
        self.representation, self.boltzmann_order = representation, boltzmann_order
        Component._init_eos(self)
        self.w = types.MethodType(Component.w, self)
        self.w_eff = types.MethodType(Component.w_eff, self)


def test_w_w_eff_and_the_forced_approximation():
    from concept_amd import commons
    from concept_amd.lib import ConceptGPUError
    p = commons.load_params({'boxsize': 8.0, 'select_eos_w': {'warm': W}})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        c = FakeComponent(p, name='warm')
    assert c.w_type == 'constant' and c.w_constant == W
    assert c.w(a=0.3) == W == c.w_eff(a=0.3) == c.w_eff()
    assert c.boltzmann_closure == 'truncate'
    # species.py:1678-1685: forced on, with the reference's warning
    assert c.approximations['P=wρ'] is True and c.approximations['P=wrho'] is True
    assert any('The P=wρ approximation has been switched on for warm' in str(w.message)
               for w in caught)
    # given in any of the reference's spellings: no warning
    for spelling in ('P=wρ', 'P = wρ', 'P = w*rho', 'wρ = P', 'ρ×w=P'):
        p = commons.load_params({'boxsize': 8.0, 'select_approximations': {spelling: True}})
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            assert FakeComponent(p).approximations['P=wρ'] is True
    p = commons.load_params({'boxsize': 8.0, 'select_approximations': {'all': {'P=2ρ': True}}})
    with pytest.raises(ConceptGPUError, match='unknown approximation'):
        FakeComponent(p)
    # matter stays at 0, particles whatever the selection says
    p = commons.load_params({'boxsize': 8.0, 'select_eos_w': {'all': W}})
    cold = FakeComponent(p, representation='particles', boltzmann_order=-1)
    assert cold.w_constant == 0 == cold.w_eff(a=0.5) and cold.approximations['P=wρ'] is True
    p = commons.load_params({'boxsize': 8.0, 'select_eos_w': {'all': -0.1}})
    with pytest.raises(ConceptGPUError, match='non-linear J'):
        FakeComponent(p)
    assert FakeComponent(p, boltzmann_order=0).w_constant == -0.1


# -- scope, v_max, the hook ----------------------------------------------------------------------
def test_scope_accepts_a_constant_w_and_names_what_is_missing():
    from concept_amd import commons, fluid
    from concept_amd.lib import ConceptGPUError
    p = commons.load_params({'boxsize': 8.0, 'select_eos_w': {'all': W},
                             'select_approximations': {'P=wρ': True},
                             'select_boltzmann_closure': {'closed': 'class'}})
    fluid._check_scope(FakeComponent(p), 0.5)
    with pytest.raises(ConceptGPUError, match='closure "class"'):
        fluid._check_scope(FakeComponent(p, name='closed'), 0.5)
    with pytest.raises(ConceptGPUError, match='boltzmann_order = 2.*shear'):
        fluid._check_scope(FakeComponent(p, boltzmann_order=2), 0.5)
    c = FakeComponent(p)
    c.w_eff = lambda a=1.0: W*a   # an equation of state that varies in time
    with pytest.raises(ConceptGPUError, match='w_eff.*varies in time'):
        fluid._check_scope(c, 0.5)
    with pytest.raises(ConceptGPUError, match='w_eff'):
        fluid.apply_internal_sources(c, {}, 0.5)
    # w = 0: nothing to apply, nothing is launched (species.py:2886-2889)
    p0 = commons.load_params({'boxsize': 8.0, 'select_approximations': {'P=wρ': True}})
    assert fluid.apply_internal_sources(FakeComponent(p0), {}, 0.5) is None
    assert fluid.apply_internal_sources(
        FakeComponent(p0, representation='particles', boltzmann_order=-1), {}) is None
    pk = commons.load_params({'boxsize': 8.0, 'fluid_scheme_select': 'Kurganov-Tadmor'})
    with pytest.raises(ConceptGPUError, match='kurganovtadmor'):
        fluid.apply_internal_sources(FakeComponent(pk), {}, 0.5)


def test_v_max_adds_the_sound_speed(monkeypatch):
    """analysis.py:3955-3963 with the kernel's maximum replaced by a known number"""
    import ctypes
    import torch
    from concept_amd import commons, fluid
    p = commons.load_params({'boxsize': 8.0, 'select_eos_w': {'warm': W},
                             'select_approximations': {'P=wρ': True}})
    bulk2 = 7.0   # what the kernel finds: max (J/(ϱ + c⁻²𝒫))²

    class L:
        @staticmethod
        def cg_fluid_vmax(ctx, ϱ, 𝒫, J, n, inv_c2, out):
            ctypes.cast(out, ctypes.POINTER(ctypes.c_double))[0] = bulk2
            return 0
    monkeypatch.setattr(fluid, '_L', L)
    monkeypatch.setattr(fluid, '_ctx', lambda comp: None)
    a = 0.5
    for name, w in (('warm', W), ('cold', 0.0)):
        c = FakeComponent(p, name=name)
        c.ϱ = c.𝒫 = torch.ones(8, dtype=torch.float64)
        c.J, c.device, c.nprocs, c.gridsize = [c.ϱ]*3, 'cpu', 1, 16
        want = a**(3*w - 2)*np.sqrt(bulk2) + p.light_speed*np.sqrt(w)/a
        assert fluid.v_max(c, a) == pytest.approx(want, rel=1e-15)
        assert fluid.courant_limit(c, a) == pytest.approx(0.21*(8.0/16)/want, rel=1e-15)

def test_timeloop_refuses_a_fluid_with_pressure_without_the_sources_hook():
    from concept_amd import commons, stepper
    from concept_amd.lib import ConceptGPUError
    p = commons.load_params({'boxsize': 8.0, 'a_begin': 0.5, 'select_eos_w': {'warm': W},
                             'select_approximations': {'P=wρ': True}})
    warm = FakeComponent(p, name='warm')
    with pytest.raises(ConceptGPUError, match='warm is a fluid component with w = 0.2.*'
                                              'fluid_sources'):
        stepper.Timeloop([warm], fluid_drift=lambda c, ᔑdt, a: None)
    with pytest.raises(ConceptGPUError, match='fluid_drift'):
        stepper.Timeloop([warm], fluid_sources=lambda c, ᔑdt, a: None)


# -- the step integrals --------------------------------------------------------------------------
def simpson(f, t0, t1, n=2000):
    t = np.linspace(t0, t1, n + 1)
    y = np.array([f(float(t_)) for t_ in t])
    return (t1 - t0)/(3*n)*(y[0] + y[-1] + 4*y[1:-1:2].sum() + 2*y[2:-1:2].sum())


def test_step_integrals_of_a_component_with_pressure_against_direct_quadrature():
    """ᔑ a**(-3w) dt, ᔑ a**(3w-2) dt, ... of a w = 0.2 component over a step, against Simpson's
    rule on the same a(t) with 2000 intervals (its own error: (Δt)⁴/180 f⁗/n⁴, far below 1e-13
    for these smooth integrands).  The loop integrates a natural cubic spline through the
    integrand at the points of the a(t) table; the pressureless integrand 'a**(-2)', which goes
    the same way and has the same smoothness, is printed as a control.  The bar, 1e-6 relative,
    is the accuracy the reference asks of its tabulated background (a and H at a = 1 within
    rtol = 1e-6, integration.py:913-920): the step integrals cannot be trusted beyond the
    a(t) table they are built on.  A swapped or pressureless integrand is off by more than
    1e-3, which the test also asserts."""
    from concept_amd import commons
    from concept_amd.integration import Cosmology
    p = commons.load_params({'boxsize': 8.0, 'a_begin': 0.5, 'select_eos_w': {'warm': W},
                             'select_approximations': {'P=wρ': True}})
    cosmo = Cosmology(p)
    cosmo.init_time()
    warm, cold = FakeComponent(p, name='warm'), FakeComponent(p, name='cold')
    t0 = cosmo.t
    t1 = t0 + 0.03*(cosmo.cosmic_time(1.0) - t0)
    out = cosmo.get_time_step_integrals(t0, t1, [warm, cold])
    a = cosmo.scale_factor
    control = abs(out['a**(-2)']/simpson(lambda t: a(t)**(-2), t0, t1) - 1)
    print(f'control a**(-2): {control:.3e}')
    exponents = {'a**(-3*w_eff)': -3*W, 'a**(-3*(1+w_eff))': -3*(1 + W),
                 'a**(-3*w_eff-1)': -3*W - 1, 'a**(3*w_eff-2)': 3*W - 2}
    for key, e in exponents.items():
        want = simpson(lambda t: a(t)**e, t0, t1)
        dev = abs(out[key, 'warm']/want - 1)
        print(f'{key}: {out[key, "warm"]!r} vs {want!r}: {dev:.3e}')
        assert dev <= 1e-6
        # and it is not the pressureless integral
        assert abs(out[key, 'cold']/want - 1) > 1e-3
    e = -3*W - 3*0.0 - 1
    want = simpson(lambda t: a(t)**e, t0, t1)
    assert abs(out['a**(-3*w_eff₀-3*w_eff₁-1)', 'warm', 'cold']/want - 1) <= 1e-6
    e = -6*W - 1
    want = simpson(lambda t: a(t)**e, t0, t1)
    assert abs(out['a**(-3*w_eff₀-3*w_eff₁-1)', 'warm', 'warm']/want - 1) <= 1e-6
