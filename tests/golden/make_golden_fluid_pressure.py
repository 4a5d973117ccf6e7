"""Golden vectors of the reference's pressure term (maccormack_internal_sources,
fluid.py:990-1067; realize_approximative, ic.py:495-509) for a fluid with a constant w = 0.2.

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_fluid_pressure.py
The reference is imported in pure-Python mode through oracle/refharness/ref_import, as in
make_golden_fluid_drift.py, whose fields and helpers are reused.  The .npz files hold inputs,
settings, ᔑdt values and recorded grids only.

The reference's component has boltzmann_order = 2 with ς = 0, as the component of the reference's
own test/fluid_pressure has: with boltzmann_order = 1 and closure 'truncate' the reference's
realize() skips every variable above boltzmann_order (ic.py:339), so realize_if_linear(2, 'trace')
leaves 𝒫 at 0 and the pressure term vanishes, although species.py:906-909 and 1678-1685 describe
that component as having a linear 𝒫 under P = wρ.  With boltzmann_order = 2, closure 'truncate'
and P = wρ on, 𝒫 is linear and realised as ϱ c²w (ic.py:495-509), ς is "non-linear" and frozen
(species.py:917-927), and the shear term adds the difference of a zero grid: ϱ and J evolve by the
flux terms and the pressure term alone, which is the scope of concept_amd.fluid.

  fluid_pressure_sources_g8  the 3-D background() ϱ and J: four calls of
                          realize_if_linear(2, 'trace') + maccormack_internal_sources with
                          different ᔑdt['a**(-3*w_eff)']; 𝒫 and J after each.  Every call must
                          change J by at least 0.1 max|J|, so that a wrong source cannot hide
                          under a large J
  fluid_pressure_kdk_g8   a self-gravitating w = 0.2 fluid on a PM grid of 8: three rounds of
                          realize_if_linear(2, 'trace'), apply_internal_sources, gravity('pm')
                          and Component.drift, every ᔑdt key with a value of its own; ϱ, J and 𝒫
                          after each stage.  No round may trigger a vacuum sweep, and every
                          detection compare stays MARGIN away from its threshold"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_fluid_drift as drift_golden   # noqa: E402
from make_golden_fluid_drift import MARGIN, Watch, background, grids, noghosts  # noqa: E402

CASES = ('fluid_pressure_sources_g8', 'fluid_pressure_kdk_g8')
W = 0.2


def param_text():
    return drift_golden.param_text() + f"select_eos_w = {{'all': {W}}}\n"


def settings(commons, comp, out):
    drift_golden.settings(commons, comp, out)
    out.update(param=param_text(), w=W)
    assert comp.w_type == 'constant' and comp.w_constant == W and comp.w_eff(a=0.7) == W
    assert comp.approximations['P=wρ'] and comp.boltzmann_closure == 'truncate'


def load(name):
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    return load_reference(param_text(), f'/tmp/concept_golden_work/{name}')


def make_fluid2(ref, ϱ, J, name='fluid'):
    """make_fluid with boltzmann_order = 2 and ς = 0 (see the module docstring)"""
    comp = ref.species.Component(name, 'matter', gridsize=drift_golden.GS, boltzmann_order=2)
    comp.populate(np.ascontiguousarray(ϱ), 'ϱ')
    for d in range(3):
        comp.populate(np.ascontiguousarray(J[d]), 'J', d)
    for multi_index in comp.ς.multi_indices:
        comp.populate(np.zeros_like(ϱ), 'ς', multi_index)
    comp.communicate_nonlinear_fluid_grids('=')
    return comp


def shear_is_zero(commons, comp):
    return all(not noghosts(commons, comp.ς[mi].grid_mv).any() for mi in comp.ς.multi_indices)


def pressure(commons, comp):
    return noghosts(commons, comp.𝒫.grid_mv)


def child_sources(name):
    ref = load(name)
    commons = ref.commons
    import fluid
    ϱ, J = background(commons.ρ_mbar, commons.boxsize)
    comp = make_fluid2(ref, ϱ, J)
    out = {}
    settings(commons, comp, out)
    out['rho_in'], out['J_in'] = grids(commons, comp)
    # (a sound wave crosses a cell in Δx/(c sqrt(w)) ≈ 7e-3 Gyr: steps of this size change J by
    # about as much as it holds)
    dts = [1.0e-4, 0.7e-4, 1.3e-4, 0.9e-4]
    out['dt'] = np.array(dts)
    J_before = out['J_in']
    for i, dt in enumerate(dts):
        comp.realize_if_linear(2, 'trace')
        fluid.maccormack_internal_sources(comp, {('a**(-3*w_eff)', comp.name): dt, '1': dt})
        ϱ_after, J_after = grids(commons, comp)
        assert np.array_equal(ϱ_after, out['rho_in'])   # no Hubble term: ϱ is not touched
        out[f'P_{i}'], out[f'J_{i}'] = pressure(commons, comp), J_after
        change = np.abs(J_after - J_before).max()/np.abs(J_before).max()
        print(name, 'call', i, 'max|ΔJ|/max|J| =', change, flush=True)
        assert change >= 0.1, 'the source term is too small to be seen'
        J_before = J_after
    assert shear_is_zero(commons, comp)
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name)


def child_kdk(name):
    ref = load(name)
    commons, interactions = ref.commons, ref.interactions
    import fluid
    ϱ, J = background(commons.ρ_mbar, commons.boxsize)
    comp = make_fluid2(ref, ϱ, [0.2*j for j in J])
    out = {}
    settings(commons, comp, out)
    out.update(G_Newton=commons.G_Newton, nghosts=commons.nghosts,
               cell_centered=int(commons.cell_centered),
               deconvolve=np.array(commons.potential_options['deconvolve']['gravity']['pm'],
                                   dtype=np.int64))
    out['rho_in'], out['J_in'] = grids(commons, comp)
    watch = Watch(ref, fluid)
    inter = interactions.find_interactions([comp], 'long-range')
    assert len(inter) == 1
    keys = ('1', 'a**(-3*w_eff)', 'a**(-3*w_eff-1)', 'a**(3*w_eff-2)')
    out['keys'] = np.array(keys)
    for r in range(3):
        dt = 1.0e-3 + 0.2e-3*r   # (Courant number c sqrt(w) dt/Δx of about 0.2)
        values = dict(zip(keys, (dt, 0.9*dt, 1.7*dt, 1.3*dt)))
        ᔑdt = {'1': values['1']}
        for key in keys[1:]:
            ᔑdt[key, comp.name] = values[key]
        out[f'dt_{r}'] = np.array([values[k] for k in keys])
        comp.realize_if_linear(2, 'trace')
        comp.apply_internal_sources(ᔑdt)
        out[f'rho_src_{r}'], out[f'J_src_{r}'] = grids(commons, comp)
        out[f'P_src_{r}'] = pressure(commons, comp)
        for force, method, receivers, suppliers in inter:
            getattr(interactions, force)(method, receivers, suppliers, ᔑdt, 'long-range', False)
        out[f'rho_kick_{r}'], out[f'J_kick_{r}'] = grids(commons, comp)
        comp.drift(ᔑdt)
        out[f'rho_{r}'], out[f'J_{r}'] = grids(commons, comp)
        out[f'P_{r}'] = pressure(commons, comp)
        print(name, 'round', r, 'sweeps', watch.sweeps, 'margin', watch.margin,
              'max|ΔJ_src|/max|J| =',
              np.abs(out[f'J_src_{r}'] - (out['J_in'] if r == 0 else out[f'J_{r - 1}'])).max()
              /np.abs(out[f'J_src_{r}']).max(),
              'max|Δϱ|/ϱ_bar =', np.abs(out[f'rho_{r}'] - out[f'rho_kick_{r}']).max()
              /commons.ρ_mbar, flush=True)
    assert watch.sweeps == [0, 0], 'a round triggered a vacuum sweep'
    assert watch.margin >= MARGIN, f'a detection compare is {watch.margin} from its threshold'
    out['margin'] = watch.margin
    assert shear_is_zero(commons, comp)
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name)


def main():
    if len(sys.argv) > 1 and sys.argv[1] in CASES:
        (child_kdk if sys.argv[1] == 'fluid_pressure_kdk_g8' else child_sources)(sys.argv[1])
        return
    for name in CASES:
        print('===', name, flush=True)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name])
        if r.returncode:
            sys.exit(f'case {name} failed')


if __name__ == '__main__':
    main()
