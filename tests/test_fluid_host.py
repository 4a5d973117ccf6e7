"""Host-side tests of concept_amd.fluid (no GPU): a NumPy restatement of the reference's
MacCormack flux step and vacuum sweep (fluid.py:724-946, 1157-1343; np.roll for the periodic
neighbours, the reference's order of additions) that reproduces the goldens of
tests/golden/make_golden_fluid_drift.py, the new parameters, the refusals and the step cycle.
The GPU tests (test_gpu_fluid_drift.py) import the restatement from here."""
import itertools
import os
import types

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RTOL = 1e-12   # the project's bar for fields: |Δ| <= RTOL*max|golden|
STEP_TRIPLES = [tuple(sign*s for s in triple) for sign in (+1, -1)
                for triple in ((+1, +1, +1), (-1, +1, -1), (-1, -1, +1), (+1, -1, -1))]
MACHINE_ϵ = float(np.finfo(np.float64).eps)
ρ_VACUUM = 1e+2*MACHINE_ϵ
NEIGHBOURS = [(i, j, k) for i in range(-1, 2) for j in range(-1, 2) for k in range(-1, 2)]


def load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def settings_of(g):
    return dict(boxsize=float(g['boxsize']), light_speed=float(g['light_speed']),
                foresight=int(g['foresight']), smoothing=float(g['smoothing']),
                vacuum_corrections=bool(g['vacuum_corrections']),
                max_vacuum_corrections=[int(v) for v in g['max_vacuum_corrections']])


def close(a, b):
    """largest deviation in units of max|b|"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))/np.max(np.abs(b)))


# -- the NumPy restatement -----------------------------------------------------------------------
def step_np(src, dst, 𝒫, steps, mc_step, factor, inv_c2):
    """maccormack_step: src = [ϱ, Jx, Jy, Jz] as the stencil reads them, dst the grids written"""
    for v in range(4):
        if mc_step == 0:
            dst[v][...] = src[v]
        else:
            dst[v] += src[v]
    shifted = lambda a, d: np.roll(a, -steps[d], axis=d)
    ϱ, J = src[0], src[1:]
    for d in range(3):
        dst[0] += (steps[d]*(shifted(J[d], d) - J[d]))*factor
    den = ϱ + inv_c2*𝒫
    for el in range(3):
        for d in range(3):
            flux = J[el]*J[d]/den
            dst[1 + el] += (steps[d]*(shifted(flux, d) - flux))*factor
            # (a quotient of rolled arrays is the rolled quotient, value for value)


def sweep_np(var, fac_time, fac_smoothing):
    """the pair terms of fluid.py:1289-1319 for the centres with fac_time ≠ 0, in the reference's
    loop order; var += Δ"""
    gs = var[0].shape[0]
    Δ = [np.zeros_like(v) for v in var]
    for c in zip(*np.nonzero(fac_time)):
        f = fac_smoothing*fac_time[c]
        cells = [tuple((c[a] + o[a]) % gs for a in range(3)) for o in NEIGHBOURS]
        for m in range(27):
            for n in range(m + 1, 27):
                dist2 = sum((NEIGHBOURS[n][a] - NEIGHBOURS[m][a])**2 for a in range(3))
                for v in range(4):
                    correction = (var[v][cells[n]] - var[v][cells[m]])*f*(1/dist2)
                    Δ[v][cells[m]] += correction
                    Δ[v][cells[n]] -= correction
    for v in range(4):
        var[v] += Δ[v]


def detect_np(ϱ, ϱˣ, mc_step, foresight):
    """(imminent, fac_time) of fluid.py:1265-1286, the roles already swapped for mc_step 1"""
    if mc_step == 0:
        imminent = ϱ*(2/foresight - 1) + ϱˣ < 2/foresight*ρ_VACUUM
        with np.errstate(all='ignore'):
            fac_time = np.where(imminent, 0.5*(ϱ - ϱˣ)/(ϱ - ρ_VACUUM), 0.0)
    else:
        imminent = ϱˣ < 2*ρ_VACUUM
        fac_time = np.where(imminent, 1.0, 0.0)
    return imminent, fac_time


class GaveUp(RuntimeError):
    pass


def maccormack_np(ϱ, J, 𝒫, dt, steps, st, info=None):
    """maccormack (fluid.py:724-792) on whole periodic grids; returns (ϱ, J).  info receives the
    attempts and sweeps per step, the fac_time of every sweep and the starred grids."""
    gs = ϱ.shape[0]
    grid = [np.array(ϱ, dtype=np.float64)] + [np.array(j, dtype=np.float64) for j in J]
    star = [np.zeros_like(ϱ) for _ in range(4)]
    factor = -dt/(st['boxsize']/gs)
    inv_c2 = st['light_speed']**(-2)
    fac_smoothing = 1./(6 + 12./2. + 8./3.)*st['smoothing']
    steps = list(steps)
    attempts, sweeps, fac_times = [0, 0], [0, 0], []
    if info is not None:
        info.update(attempts=attempts, sweeps=sweeps, fac_time=fac_times, starred=star, grid=grid)
    for mc_step in range(2):
        src, dst = (grid, star) if mc_step == 0 else (star, grid)
        for attempt in range(st['max_vacuum_corrections'][mc_step]):
            attempts[mc_step] += 1
            if attempt == 0 or mc_step == 0:
                step_np(src, dst, 𝒫, steps, mc_step, factor, inv_c2)
            if not st['vacuum_corrections']:
                break
            # (second step: detection on the unstarred ϱ, corrections to the starred grids)
            imminent, fac_time = (detect_np(grid[0], star[0], 0, st['foresight']) if mc_step == 0
                                  else detect_np(star[0], grid[0], 1, st['foresight']))
            if not imminent.any():
                break
            sweeps[mc_step] += 1
            fac_times.append((mc_step, fac_time))
            sweep_np(src, fac_time, fac_smoothing)
        else:
            if mc_step == 1:
                raise GaveUp(f'Giving up after {st["max_vacuum_corrections"][1]} failed attempts')
        steps = [-s for s in steps]
    for v in range(4):
        grid[v] *= 0.5
    return grid[0], np.stack(grid[1:])


# -- the restatement against the goldens ---------------------------------------------------------
def test_restatement_reproduces_the_smooth_golden():
    g = load('fluid_drift_smooth_g8')
    st = settings_of(g)
    ϱ, J, 𝒫 = g['rho_in'], g['J_in'], g['P_in']
    assert np.all(𝒫 == 0) and np.all(g['P_out'] == 0)
    contrast = (ϱ.max() - ϱ.min())/(2*ϱ.mean())
    assert 0.2 < contrast < 0.45 and all(np.abs(J[d]).max() > 0 for d in range(3))
    worst = 0.0
    for i, steps in enumerate(STEP_TRIPLES):
        info = {}
        ϱ, J = maccormack_np(ϱ, J, 𝒫, float(g['dt'][i]), steps, st, info)
        assert info['sweeps'] == [0, 0] == list(g[f'sweeps_{i}'])
        worst = max(worst, close(ϱ, g[f'rho_{i}']), close(J, g[f'J_{i}']))
    print('restatement vs reference, smooth:', worst)
    assert worst <= RTOL
    assert float(g['margin']) >= 1e-6


def test_restatement_reproduces_the_vacuum_golden():
    g = load('fluid_drift_vacuum_g8')
    st = settings_of(g)
    assert st['max_vacuum_corrections'] == [1, 8] and st['smoothing'] == 2.0
    info = {}
    ϱ, J = maccormack_np(g['rho_in'], g['J_in'], g['P_in'], float(g['dt'][0]), STEP_TRIPLES[0],
                         st, info)
    assert info['attempts'] == list(g['attempts_0']) and info['sweeps'] == list(g['sweeps_0'])
    assert info['sweeps'][0] >= 1 and int(g['n_sweeps']) == len(info['fac_time'])
    for s, (mc_step, fac_time) in enumerate(info['fac_time']):
        assert mc_step == int(g[f'sweep{s}_mc_step'])
        assert np.array_equal(fac_time != 0, g[f'sweep{s}_fac_time'] != 0)
        assert close(fac_time, g[f'sweep{s}_fac_time']) <= RTOL
    # one void lies across the x layers 3|4, the other across the box face
    flagged_x = set(np.nonzero(g['sweep0_fac_time'])[0])
    assert {3, 4} & flagged_x and {0, 7} & flagged_x
    worst = max(close(ϱ, g['rho_0']), close(J, g['J_0']))
    print('restatement vs reference, vacuum:', worst)
    assert worst <= RTOL
    assert float(g['margin']) >= 1e-6


def test_restatement_gives_up_where_the_reference_gives_up():
    """the second step detects on the unstarred ϱ and corrects the starred grids: once it flags a
    cell it flags it on every attempt; the golden holds what the reference left behind"""
    g = load('fluid_drift_vacuum_abort_g8')
    st = settings_of(g)
    info = {}
    with pytest.raises(GaveUp):
        maccormack_np(g['rho_in'], g['J_in'], g['P_in'], float(g['dt'][0]), STEP_TRIPLES[0], st,
                      info)
    assert info['attempts'] == list(g['attempts_0']) == [1, 8]
    assert info['sweeps'] == list(g['sweeps_0']) and info['sweeps'][1] >= 2
    for s, (mc_step, fac_time) in enumerate(info['fac_time']):
        assert np.array_equal(fac_time != 0, g[f'sweep{s}_fac_time'] != 0)
    worst = max(close(info['grid'][0], g['rho_0']), close(np.stack(info['grid'][1:]), g['J_0']),
                close(info['starred'][0], g['rho_starred']),
                close(np.stack(info['starred'][1:]), g['J_starred']))
    print('restatement vs reference, abort:', worst)
    assert worst <= RTOL


def test_restatement_reproduces_the_drifts_of_the_kdk_golden():
    g = load('fluid_kdk_g8')
    st = settings_of(g)
    keys = list(g['keys'])
    𝒫 = np.zeros_like(g['rho_in'])
    worst = 0.0
    for r in range(3):
        dt = float(g[f'dt_{r}'][keys.index('a**(3*w_eff-2)')])
        ϱ, J = maccormack_np(g[f'rho_kick_{r}'], g[f'J_kick_{r}'], 𝒫, dt, STEP_TRIPLES[r], st)
        worst = max(worst, close(ϱ, g[f'rho_{r}']), close(J, g[f'J_{r}']))
        assert np.array_equal(g[f'rho_kick_{r}'], g['rho_in'] if r == 0 else g[f'rho_{r - 1}'])
    print('restatement vs reference, kdk drifts:', worst)
    assert worst <= RTOL


# -- parameters, refusals, the step cycle --------------------------------------------------------
def test_fluid_parameters_load_with_the_reference_defaults():
    from concept_amd import commons
    p = commons.load_params({'boxsize': 8.0})
    assert p.fluid_scheme_select == {'all': 'maccormack', 'default': 'maccormack'}
    mc = p.fluid_options['maccormack']
    matter = types.SimpleNamespace(name='fl', species='matter', representation='fluid')
    neutrino = types.SimpleNamespace(name='nu', species='neutrino', representation='fluid')
    assert commons.is_selected(matter, mc['vacuum_corrections_select']) is True
    assert commons.is_selected(matter, mc['max_vacuum_corrections_select']) == [1, 'gridsize']
    assert commons.is_selected(matter, mc['foresight_select']) == 25
    assert commons.is_selected(matter, mc['smoothing_select']) == 2.0
    assert commons.is_selected(neutrino, mc['smoothing_select']) == 1.0
    assert commons.ρ_vacuum == 1e+2*commons.machine_ϵ
    p = commons.load_params({
        'boxsize': 8.0, 'fluid_scheme_select': {'nu': 'Kurganov-Tadmor'},
        'fluid_options': {'MacCormack': {'foresight_select': 30.2, 'smoothing_select': {'nu': 3},
                                         'max_vacuum_corrections_select': 2,
                                         'Vacuum_Corrections_Select': {'nu': False}}}})
    assert commons.is_selected(neutrino, p.fluid_scheme_select) == 'kurganovtadmor'
    assert commons.is_selected(matter, p.fluid_scheme_select) == 'maccormack'
    mc = p.fluid_options['maccormack']
    assert commons.is_selected(neutrino, mc['foresight_select']) == 30
    assert commons.is_selected(neutrino, mc['smoothing_select']) == 3.0
    assert commons.is_selected(neutrino, mc['max_vacuum_corrections_select']) == [2, 2]
    assert commons.is_selected(neutrino, mc['vacuum_corrections_select']) is False
    assert commons.is_selected(matter, mc['vacuum_corrections_select']) is True


def fake_component(params, **kw):
    d = dict(name='fl', species='matter', representation='fluid', boltzmann_order=1, gridsize=8,
             params=params, w_eff=lambda a=1.0: 0.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_unknown_schemes_and_components_outside_the_scope_raise():
    from concept_amd import commons, fluid
    from concept_amd.lib import ConceptGPUError
    p = commons.load_params({'boxsize': 8.0, 'fluid_scheme_select': {'kt': 'Kurganov-Tadmor',
                                                                     'odd': 'upwind'}})
    with pytest.raises(ConceptGPUError, match='kurganovtadmor'):
        fluid.drift(fake_component(p, name='kt'), {}, 1.0)
    with pytest.raises(ConceptGPUError, match='upwind'):
        fluid.drift(fake_component(p, name='odd'), {}, 1.0)
    with pytest.raises(ConceptGPUError, match='boltzmann_order = 2'):
        fluid.drift(fake_component(p, boltzmann_order=2), {}, 1.0)
    with pytest.raises(ConceptGPUError, match='w_eff'):
        fluid.drift(fake_component(p, w_eff=lambda a=1.0: 0.1), {}, 1.0)
    with pytest.raises(ConceptGPUError, match='fluid components'):
        fluid.drift(fake_component(p, representation='particles'), {}, 1.0)
    # no J variable: nothing to do, and nothing is touched
    assert fluid.drift(fake_component(p, boltzmann_order=0), {}, 1.0) is None


def test_step_cycle_and_attempt_loop(monkeypatch):
    """the cycle of eight advances once per maccormack() call, whatever the attempts, is shared
    by all components and rewinds; the first step is re-evolved at each attempt, the second
    evolved once and corrected until it comes clean or the attempts run out"""
    from concept_amd import commons, fluid
    from concept_amd.lib import ConceptGPUError
    p = commons.load_params({'boxsize': 8.0, 'fluid_options': {
        'maccormack': {'max_vacuum_corrections_select': {'all': (1, 'gridsize'), 'twice': (2, 3)}}}})
    calls, dirty = [], {}
    monkeypatch.setattr(fluid, 'maccormack_step',
                        lambda c, ᔑdt, steps, mc_step, halve=False:
                        calls.append((c.name, mc_step, tuple(steps), halve)))

    def correct_vacuum(c, mc_step, record=None):   # sweeps while the step is "dirty"
        left = dirty.get((c.name, mc_step), 0)
        dirty[c.name, mc_step] = max(left - 1, 0)
        return left > 0
    monkeypatch.setattr(fluid, 'correct_vacuum', correct_vacuum)
    monkeypatch.setattr(fluid, 'finish', lambda c, halve=True: calls.append((c.name, 'finish', halve)))
    a, b = fake_component(p, name='a'), fake_component(p, name='b')
    assert fluid.STEP_TRIPLES == tuple(STEP_TRIPLES)
    fluid.reset_steps()
    for i in range(10):
        c = (a, b)[i % 2]
        del calls[:]
        fluid.maccormack(c, {})
        t = STEP_TRIPLES[i % 8]
        assert calls == [(c.name, 0, t, False), (c.name, 1, tuple(-s for s in t), False),
                         (c.name, 'finish', True)]
        assert c.maccormack_attempts == [1, 1] and c.maccormack_sweeps == [0, 0]
    fluid.reset_steps()
    # a dirty first step: swept once, not re-evolved (one attempt); a second step that needs
    # three sweeps: evolved once
    dirty.update({('a', 0): 1, ('a', 1): 3})
    del calls[:]
    fluid.maccormack(a, {})
    assert [c_[1] for c_ in calls] == [0, 1, 'finish'] and calls[0][2] == STEP_TRIPLES[0]
    assert a.maccormack_attempts == [1, 4] and a.maccormack_sweeps == [1, 3]
    # two attempts at the first step: re-evolved
    twice = fake_component(p, name='twice')
    dirty.update({('twice', 0): 5, ('twice', 1): 2})
    del calls[:]
    fluid.maccormack(twice, {})
    assert [c_[1] for c_ in calls] == [0, 0, 1, 'finish'] and calls[0][2] == STEP_TRIPLES[1]
    assert twice.maccormack_attempts == [2, 3]
    # a second step that never comes clean
    dirty.update({('a', 1): 100})
    with pytest.raises(ConceptGPUError, match='Giving up after 8 failed attempts to remove '
                                              'negative densities in a'):
        fluid.maccormack(a, {})
    assert a.maccormack_attempts == [1, 8]
    # corrections switched off: check only, and the second step leaves the halved values itself
    p.fluid_options['maccormack']['vacuum_corrections_select']['b'] = False
    checked = []
    monkeypatch.setattr(fluid, 'check_vacuum', lambda c, mc_step: checked.append(mc_step))
    del calls[:]
    fluid.maccormack(b, {})
    assert checked == [0, 1]
    assert [(c_[1], c_[-1]) for c_ in calls] == [(0, False), (1, True), ('finish', False)]
    assert calls[0][2] == STEP_TRIPLES[3]
    fluid.reset_steps()


def test_courant_limit_formula(monkeypatch):
    from concept_amd import commons, fluid
    p = commons.load_params({'boxsize': 8.0, 'Δt_base_nonlinear_factor': 0.5})
    c = fake_component(p, gridsize=16)
    monkeypatch.setattr(fluid, 'v_max', lambda comp, a, closure_class=False: 2.5)
    assert fluid.courant_limit(c, 0.5) == 0.21*0.5*(8.0/16)/2.5
    monkeypatch.setattr(fluid, 'v_max', lambda comp, a, closure_class=False: 0.0)
    assert fluid.courant_limit(c, 0.5) == 0.21*0.5*(8.0/16)/commons.machine_ϵ
    assert len(list(itertools.islice(fluid._steps, 3))) == 3
    fluid.reset_steps()
