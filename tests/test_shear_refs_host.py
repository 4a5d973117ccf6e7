"""Host-side tests of the shear of closure 'class' (no GPU): the identities of the numpy references
of tests/shear_refs.py, ic.amplitudes_from_transfer_ratio against a table computed by hand, the
refusals of the new scope and their messages, and the old refusals of closure 'class', which stay.

Bars.  K is a few products and one division: the trace vanishes to a few ulp of its largest
element (1).  The divergence formed in Fourier space and the order-2 difference of the six
separately realised grids are the same sum in exact arithmetic; both go through numpy's
transforms: the project's 1e-12, of max |ΔJ|."""
import numpy as np
import pytest

import lpt_refs
import shear_refs
from test_fluid_pressure_host import FakeComponent

L = 100.0
GRIDSIZES = [8, 12, 16]


# ---- the references' identities ------------------------------------------------------------------
@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_the_tensor_factor_is_traceless_and_symmetric(gridsize):
    g = gridsize
    live = lpt_refs.alive(g)
    assert live.sum() > 0
    trace = sum(shear_refs.tensor_factor(g, m, m) for m in range(3))
    print(f'g = {g}: max |Σₘ Kₘₘ| = {np.abs(trace[live]).max():.3e}')
    assert np.abs(trace[live]).max() <= 4e-16
    for m, n in ((0, 1), (0, 2), (1, 2)):
        assert np.array_equal(shear_refs.tensor_factor(g, m, n), shear_refs.tensor_factor(g, n, m))
    # along an axis K is diag(-1, ½, ½): k = (3, 0, 0)
    at = (0, 3, 0)  # [j][i][kk]
    assert [shear_refs.tensor_factor(g, m, m)[at] for m in range(3)] == [-1.0, 0.5, 0.5]
    assert shear_refs.tensor_factor(g, 0, 1)[at] == 0


@pytest.mark.parametrize('gridsize', GRIDSIZES)
def test_the_fourier_divergence_is_the_difference_of_the_six_grids(gridsize):
    g = gridsize
    ϱ = shear_refs.random_density(g, g)
    table = shear_refs.random_table(g, g)
    J0 = np.random.default_rng(g).normal(size=(3, g, g, g))
    dt, c0 = 0.037, 2.5*(1 + 1/3)
    six = shear_refs.shear_sources_six(ϱ, J0, table, dt, c0, L)
    fourier = shear_refs.shear_sources(ϱ, J0, table, dt, c0, L)
    ΔJ = six - J0
    scale = np.abs(ΔJ).max()
    err = np.abs(fourier - six).max()
    print(f'g = {g}: max |ΔJ| = {scale:.3e}, the two routes differ by {err:.3e} = '
          f'{err/scale:.3e} of it')
    assert scale > 1e-3*np.abs(J0).max()
    assert err <= 1e-12*scale
    # every dimension is moved, and a divergence moves no net momentum
    for i in range(3):
        assert np.abs(ΔJ[i]).max() > 0.1*scale
        assert abs(ΔJ[i].sum()) <= 1e-13*np.abs(ΔJ[i]).sum()


def test_the_sine_factor_is_the_central_difference():
    """(f[x + 1] - f[x - 1])·(½/Δx) of a single mode is the mode times i·sin(2π k/g)/Δx"""
    g, k = 12, 5
    x = np.arange(g)
    f = np.cos(2*np.pi*k*x/g + 0.3)[:, None, None]*np.ones((g, g, g))
    Δx = L/g
    want = -np.sin(2*np.pi*k/g)/Δx*np.sin(2*np.pi*k*x/g + 0.3)
    assert np.abs(shear_refs.diff2(f, 0, Δx)[:, 0, 0] - want).max() <= 1e-15/Δx*4


def golden_increment(g, dt, c0):
    """ΔJ of the reference's route from the golden's differences: Jᵢ += ∂ⱼ((-dt)·c0·σₘₙ)"""
    ΔJ = np.zeros((3,) + g['rho'].shape)
    for m, n in shear_refs.PAIRS:
        for i in {m, n}:
            j = n if i == m else m
            ΔJ[i] += (-dt)*c0*g[f'dsigma_{m}{n}_{j}']
    return ΔJ


def test_the_references_reproduce_the_golden_of_the_reference(golden):
    """tests/golden/fluid_shear_g8.npz (make_golden_fluid_shear.py): the reference's own
    realize_grid of rank 2 and diff_domaingrid of order 2, to the project's 1e-12"""
    g = golden('fluid_shear_g8')
    ϱ, table, boxsize = g['rho'], g['amplitudes'], float(g['boxsize'])
    for m, n in shear_refs.PAIRS:
        σ = shear_refs.realize_shear(ϱ, table, m, n, 1.0)
        err = np.abs(σ - g[f'sigma_{m}{n}']).max()/np.abs(g[f'sigma_{m}{n}']).max()
        print(f'σ[{m}{n}] within {err:.3e} of the golden\'s largest value')
        assert err <= 1e-12
        for j in {m, n}:
            want = g[f'dsigma_{m}{n}_{j}']
            got = shear_refs.diff2(g[f'sigma_{m}{n}'], j, boxsize/ϱ.shape[0])
            assert np.abs(got - want).max() <= 1e-12*np.abs(want).max()
    dt, c0 = 0.037, 2.5*(1 + 1/3)
    want = golden_increment(g, dt, c0)
    got = shear_refs.shear_sources(ϱ, np.zeros_like(want), table, dt, c0, boxsize)
    err = np.abs(got - want).max()/np.abs(want).max()
    print(f'ΔJ formed in Fourier space within {err:.3e} of max |ΔJ| of the golden\'s route')
    assert err <= 1e-12


# ---- the amplitude helper ------------------------------------------------------------------------
def test_amplitudes_from_transfer_ratio_against_a_table_by_hand():
    from concept_amd import ic
    from concept_amd.lib import ConceptGPUError
    g, ϱ_bar = 8, 2.5
    k_f = 2*np.pi/L
    # a ratio linear in log k: the interpolation is exact
    k = np.array([0.5*k_f, 2*k_f, 8*k_f])
    ratio = -0.3 + 0.2*np.log(k/k_f)
    got = ic.amplitudes_from_transfer_ratio(k, ratio, g, L, ϱ_bar)
    assert got.shape == (3*(g//2 - 1)**2 + 1,) and got[0] == 0
    for k2 in (1, 2, 3, 9, 27):
        want = (-0.3 + 0.2*np.log(np.sqrt(k2)))*g**(-3)/ϱ_bar
        assert got[k2] == pytest.approx(want, rel=1e-13), k2
    # a constant ratio gives a constant table
    flat = ic.amplitudes_from_transfer_ratio(k, np.full(3, 0.7), g, L, ϱ_bar)
    assert np.array_equal(flat[1:], np.full(27, 0.7*(float(g)**(-3)/ϱ_bar)))
    with pytest.raises(ConceptGPUError, match='the grid needs'):
        ic.amplitudes_from_transfer_ratio(k[1:], ratio[1:], g, L, ϱ_bar)
    with pytest.raises(ConceptGPUError, match='k must be increasing'):
        ic.amplitudes_from_transfer_ratio(k[::-1], ratio, g, L, ϱ_bar)


# ---- scope ---------------------------------------------------------------------------------------
def params(**more):
    from concept_amd import commons
    user = {'boxsize': 8.0, 'select_eos_w': {'all': 1/3},
            'select_approximations': {'all': {'P=wρ': True}},
            'select_boltzmann_closure': {'nu': 'class', 'nu kt': 'class', 'nu primordial': 'class',
                                         'nu exact': 'class'},
            'realization_options': {'structure': {'nu': 'nonlinear', 'nu kt': 'nonlinear',
                                                  'nu exact': 'nonlinear',
                                                  'cold': 'nonlinear'}}}
    user.update(more)
    return commons.load_params(user)


def test_closure_class_is_in_scope_only_through_the_keyword():
    from concept_amd import fluid
    from concept_amd.lib import ConceptGPUError
    p = params()
    nu = FakeComponent(p, name='nu', species='neutrino')
    assert nu.boltzmann_closure == 'class' and nu.approximations['P=wρ']
    # as before, word for word
    with pytest.raises(ConceptGPUError, match='nu: Boltzmann closure "class": realising ς with '
                                              r'CLASS \(the shear term of '
                                              r'maccormack_internal_sources\) is not implemented, '
                                              'only "truncate"'):
        fluid._check_scope(nu, 0.5)
    with pytest.raises(ConceptGPUError, match='closure "class"'):
        fluid.kurganov_tadmor(nu, {}, 0.5)
    with pytest.raises(ConceptGPUError, match='closure "class"'):
        fluid.apply_internal_sources(nu, {}, 0.5)
    with pytest.raises(ConceptGPUError, match='closure "class"'):
        fluid.sources_selected(nu, {}, 0.5)
    # opted in
    fluid._check_scope(nu, 0.5, closure_class=True)
    # the keyword changes nothing for another closure
    cold = FakeComponent(p, name='cold')
    fluid._check_scope(cold, 0.5, closure_class=True)
    with pytest.raises(ConceptGPUError, match='closure "truncate" has no shear term'):
        fluid.shear_sources(cold, {}, np.zeros(1))


def test_the_refusals_of_the_new_scope_name_what_is_missing(monkeypatch):
    from concept_amd import comm, fluid, ic
    from concept_amd.lib import ConceptGPUError
    p = params()
    for order in (0, 2):
        c = FakeComponent(p, name='nu', species='neutrino', boltzmann_order=order)
        with pytest.raises(ConceptGPUError, match=f'closure "class" with boltzmann_order = {order}'
                                                  '.*boltzmann_order = 1'):
            fluid._check_scope(c, 0.5, closure_class=True)
        with pytest.raises(ConceptGPUError, match=f'boltzmann_order = {order}'):
            ic.check_shear_scope(c)
    c = FakeComponent(p, name='nu primordial', species='neutrino')
    with pytest.raises(ConceptGPUError, match=r'realization_options\["structure"\] = "primordial"'
                                              '.*select "nonlinear"'):
        fluid._check_scope(c, 0.5, closure_class=True)
    pk = params(fluid_scheme_select={'nu kt': 'Kurganov-Tadmor'})
    c = FakeComponent(pk, name='nu kt', species='neutrino')
    with pytest.raises(ConceptGPUError, match='fluid scheme "kurganovtadmor": the ς flux inside '
                                              'the limiter stage'):
        fluid._check_scope(c, 0.5, closure_class=True)
    with pytest.raises(ConceptGPUError, match='limiter stage'):
        fluid.closure_sources(lambda c, a: None)(c, {}, 0.5)
    pe = params(select_approximations={'all': {'P=wρ': True}, 'nu exact': {'P=wρ': False}})
    c = FakeComponent(pe, name='nu exact', species='neutrino')
    assert not c.approximations['P=wρ']
    with pytest.raises(ConceptGPUError, match='without the P=wρ approximation: the realisation '
                                              'of δ𝒫.*Hubble term'):
        fluid._check_scope(c, 0.5, closure_class=True)
    nu = FakeComponent(params(), name='nu', species='neutrino')
    monkeypatch.setattr(comm, 'active', lambda: object())
    with pytest.raises(ConceptGPUError, match='active comm process group'):
        fluid._check_scope(nu, 0.5, closure_class=True)
    with pytest.raises(ConceptGPUError, match='active comm process group'):
        fluid.shear_sources(nu, {}, np.zeros(1))
    monkeypatch.undo()
    # not a fluid, not an index pair
    with pytest.raises(ConceptGPUError, match='fluid components'):
        ic.check_shear_scope(FakeComponent(params(), representation='particles',
                                           boltzmann_order=-1))
    for bad in (3, (0, 3), (1,), 'trace'):
        with pytest.raises(ConceptGPUError, match='multi_index'):
            ic.realize_shear(nu, 0.5, np.zeros(1), multi_index=bad)


def test_closure_sources_sends_the_other_components_on(monkeypatch):
    """a particle component and a 'truncate' fluid take sources_selected(); a 'class' fluid the
    table, the shear term and then the pressure term, in the reference's order"""
    from concept_amd import fluid
    p = params()
    calls = []
    monkeypatch.setattr(fluid, 'sources_selected',
                        lambda c, ᔑdt, a: calls.append(('selected', c.name, a)))
    monkeypatch.setattr(fluid, 'shear_sources',
                        lambda c, ᔑdt, table, a: calls.append(('shear', c.name, table, a)))
    monkeypatch.setattr(fluid, 'internal_sources',
                        lambda c, ᔑdt, a, closure_class=False: calls.append(
                            ('pressure', c.name, a, closure_class)))
    hook = fluid.closure_sources(lambda c, a: ('table of', c.name, a))
    part = FakeComponent(p, name='part', representation='particles', boltzmann_order=-1)
    cold = FakeComponent(p, name='cold')
    nu = FakeComponent(p, name='nu', species='neutrino')
    for c in (part, cold, nu):
        hook(c, {}, 0.25)
    assert calls == [('selected', 'part', 0.25), ('selected', 'cold', 0.25),
                     ('shear', 'nu', ('table of', 'nu', 0.25), 0.25),
                     ('pressure', 'nu', 0.25, True)]
    hooks = fluid.closure_hooks(lambda c, a: None)
    assert sorted(hooks) == ['fluid_drift', 'fluid_limiter', 'fluid_sources']
    assert hooks['fluid_drift'].func is fluid.drift and hooks['fluid_drift'].keywords == {
        'closure_class': True}


def test_the_new_symbols_are_declared():
    from concept_amd import lib
    for name in ('cg_realize_grid_tensor', 'cg_shear_divergence', 'cg_fluid_add_from_mesh'):
        assert name in lib.SYMBOLS
