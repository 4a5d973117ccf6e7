"""Golden vectors of the reference's Kurganov-Tadmor scheme (kurganov_tadmor, fluid.py:103-464,
with at_interface, slope_ratio, kurganov_tadmor_flux, finalize_rk_step and the nine flux limiters,
fluid.py:466-673).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_fluid_kt.py
The reference is imported in pure-Python mode through oracle/refharness/ref_import, as in
make_golden_fluid_drift.py and make_golden_fluid_pressure.py, whose fields and helpers are reused;
integration.init_time() is called after loading (kurganov_tadmor asks cosmic_time and
scale_factor).  The .npz files hold inputs, settings, ᔑdt values, the scale factors used and
recorded grids only.

The reference's component is make_fluid2 of make_golden_fluid_pressure.py (boltzmann_order = 2
with ς = 0, see that file's docstring): only then does the reference realise 𝒫, and the ς flux
terms add the exact zeros of a zero grid.  Component.drift passes no scale factor, so the scheme
takes universals.a (species.py:2230), which is a_begin here.

  fluid_kt_smooth_g8      w = 0, 'minmod' (the matter default), order 2, enable_Hubble: four
                          Component.drift calls, ϱ and J after each
  fluid_kt_pressure_g8    w = 0.2, 'mc', every ᔑdt key with a value of its own: three calls, ϱ, J
                          and both 𝒫 buffers after each.  No call may change J by more than its
                          own size, every call must change ϱ by at least 1e-3 of its maximum
  fluid_kt_limiter_<name>_g8  w = 0.2, one call per limiter on the background with random
                          contrast, spikes, a steep ramp and plateaus of exactly equal cells.
                          Every branch of the limiter and of slope_ratio must be taken, and apart
                          from the exact plateaus every r stays MARGIN (relative) away from each
                          threshold of the limiter
  fluid_kt_euler_g8       w = 0.2, 'mc', Runge-Kutta order 1: two calls
  fluid_kt_kdk_g8         a self-gravitating w = 0.2 fluid on a PM grid of 8: three rounds of
                          apply_internal_sources (nothing in this scheme), gravity('pm') and
                          Component.drift
  fluid_kt_rk_scale_factors  the scale factors of the two Runge-Kutta steps (fluid.py:160-173) for
                          a few (a, ᔑdt['1']), recorded by wrapping scale_factor"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_fluid_drift as drift_golden   # noqa: E402
from make_golden_fluid_drift import GS, MARGIN, background, grids, noghosts  # noqa: E402
from make_golden_fluid_pressure import make_fluid2, shear_is_zero   # noqa: E402

# case name of a limiter -> (the name given in the parameter file, the reference's function,
# its thresholds in the order of its branches)
LIMITERS = {
    'minmod': ('minmod', 'flux_limiter_minmod', (1, 0)),
    'mc': ('monotonizedcentral', 'flux_limiter_monotonized_central', (3, 1./3., 0)),
    'ospre': ('ospre', 'flux_limiter_ospre', (0,)),
    'superbee': ('superbee', 'flux_limiter_superbee', (2, 1, 0.5, 0)),
    'sweby': ('sweby', 'flux_limiter_sweby', (1.5, 1, 1/1.5, 0)),
    'umist': ('umist', 'flux_limiter_umist', (5, 1, 0.2, 0)),
    'vanalbada': ('vanalbada', 'flux_limiter_vanalbada', (0,)),
    'vanleer': ('muscl', 'flux_limiter_vanleer', (0,)),
    'koren': ('koren', 'flux_limiter_koren', (2.5, 0.25, 0)),
}
CASES = (('fluid_kt_smooth_g8', 'fluid_kt_pressure_g8', 'fluid_kt_euler_g8', 'fluid_kt_kdk_g8',
          'fluid_kt_rk_scale_factors')
         + tuple(f'fluid_kt_limiter_{name}_g8' for name in LIMITERS))
W = 0.2
J_SCALE = 60.0   # the bulk velocities of the w = 0.2 cases, in units of background()'s


def param_text(w, limiter=None, rk_order=None):
    kt = {}
    if limiter is not None:
        kt['flux_limiter_select'] = {'all': limiter}
    if rk_order is not None:
        kt['rungekuttaorder'] = {'all': rk_order}
    return (drift_golden.param_text()
            + "fluid_scheme_select = {'all': 'Kurganov-Tadmor'}\n"
            + f"fluid_options = {{'kurganovtadmor': {kt!r}}}\n"
            + (f"select_eos_w = {{'all': {w}}}\n" if w else ''))


def load(name, text):
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    ref = load_reference(text, f'/tmp/concept_golden_work/{name}')
    ref.integration.init_time()
    return ref


def settings(ref, comp, out, text, w):
    commons = ref.commons
    kt = commons.fluid_options['kurganovtadmor']
    out.update(boxsize=commons.boxsize, gridsize=GS, light_speed=commons.light_speed,
               ρ_mbar=commons.ρ_mbar, param=text, w=float(w), a=float(commons.universals.a),
               enable_Hubble=bool(commons.enable_Hubble),
               limiter=str(commons.is_selected(comp, kt['flux_limiter_select'])),
               rk_order=int(commons.is_selected(comp, kt['rungekuttaorder'])))
    assert commons.is_selected(comp, commons.fluid_scheme_select) == 'kurganovtadmor'
    assert comp.w_type == 'constant' and comp.w_constant == w and comp.w_eff(a=0.7) == w
    assert comp.approximations['P=wρ'] and comp.boltzmann_closure == 'truncate'


class Steps:
    """records the scale factor of every Runge-Kutta step: the results of the scale_factor calls
    of fluid.py:171-173"""

    def __init__(self, fluid):
        self.a, self.orig = [], fluid.scale_factor
        fluid.scale_factor = self

    def __call__(self, t=-1):
        a = self.orig(t)
        self.a.append(float(a))
        return a

    def take(self):
        a, self.a = self.a, []
        return np.array(a)


def sdt_of(comp, dt, dt_J, dt_P, dt_kick=None):
    ᔑdt = {'1': dt, ('a**(3*w_eff-2)', comp.name): dt_J, ('a**(-3*w_eff)', comp.name): dt_P}
    if dt_kick is not None:
        ᔑdt['a**(-3*w_eff-1)', comp.name] = dt_kick
    return ᔑdt


def both_𝒫(commons, comp):
    return noghosts(commons, comp.𝒫.grid_mv), noghosts(commons, comp.𝒫.gridˣ_mv)


def drifts(name, ref, comp, out, dts, check=None):
    """Component.drift once per row (ᔑdt['1'], ['a**(3*w_eff-2)'], ['a**(-3*w_eff)']) of dts"""
    import fluid
    commons = ref.commons
    steps = Steps(fluid)
    out['rho_in'], out['J_in'] = grids(commons, comp)
    out['dt'] = np.array(dts)
    ϱ_before, J_before = out['rho_in'], out['J_in']
    for i, row in enumerate(dts):
        comp.drift(sdt_of(comp, *row))
        out[f'rho_{i}'], out[f'J_{i}'] = grids(commons, comp)
        out[f'P_{i}'], out[f'Pstar_{i}'] = both_𝒫(commons, comp)
        out[f'a_steps_{i}'] = steps.take()
        Δϱ = np.abs(out[f'rho_{i}'] - ϱ_before).max()/np.abs(ϱ_before).max()
        ΔJ = np.abs(out[f'J_{i}'] - J_before).max()/np.abs(J_before).max()
        print(name, 'call', i, 'a of the steps', out[f'a_steps_{i}'], 'max|Δϱ|/max|ϱ| =', Δϱ,
              'max|ΔJ|/max|J| =', ΔJ, 'min ϱ/ϱ_bar =', out[f'rho_{i}'].min()/commons.ρ_mbar,
              flush=True)
        if check is not None:
            check(Δϱ, ΔJ)
        ϱ_before, J_before = out[f'rho_{i}'], out[f'J_{i}']
    assert shear_is_zero(commons, comp)


def save(name, out):
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name)


def child_smooth(name):
    text = param_text(0)
    ref = load(name, text)
    ϱ, J = background(ref.commons.ρ_mbar, ref.commons.boxsize)
    comp = make_fluid2(ref, ϱ, J)
    out = {}
    settings(ref, comp, out, text, 0)
    assert out['limiter'] == 'minmod' and out['rk_order'] == 2 and out['enable_Hubble']
    drifts(name, ref, comp, out, [(dt, 3.7*dt, 1.6*dt) for dt in (0.10, 0.09, 0.11, 0.08)])
    save(name, out)


def warm_background(commons):
    ϱ, J = background(commons.ρ_mbar, commons.boxsize)
    return ϱ, [J_SCALE*j for j in J]


def child_pressure(name):
    euler = name == 'fluid_kt_euler_g8'
    text = param_text(W, 'mc', 1 if euler else None)
    ref = load(name, text)
    ϱ, J = warm_background(ref.commons)
    comp = make_fluid2(ref, ϱ, J)
    out = {}
    settings(ref, comp, out, text, W)
    assert out['limiter'] == 'mc' and out['rk_order'] == (1 if euler else 2)

    def check(Δϱ, ΔJ):
        assert ΔJ <= 1.0, 'a call changed J by more than its own size'
        assert Δϱ >= 1e-3, 'the change of ϱ is too small to show a wrong term'
    # (sound crosses a cell in Δx a/(c sqrt(w)) ≈ 3.6e-3 Gyr: Courant numbers of about 0.07)
    dts = [(dt, 2.3*dt, 1.4*dt) for dt in ((2.0e-4, 1.7e-4) if euler else
                                           (2.0e-4, 1.7e-4, 2.2e-4))]
    drifts(name, ref, comp, out, dts, check)
    save(name, out)


def sharp(commons, seed=9):
    """warm_background() with a random contrast, spikes, a steep ramp and plateaus of exactly
    equal cells in ϱ and in every J"""
    rng = np.random.default_rng(seed)
    ϱ, J = warm_background(commons)
    fields = [ϱ] + J
    for n, f in enumerate(fields):
        f *= 1 + 0.25*rng.uniform(-1, 1, f.shape)
        if n:
            f += 0.3*np.abs(f).max()*rng.uniform(-1, 1, f.shape)
        f[5, 5, 5] *= 1.8   # local extrema
        f[1, 6, 2] *= 0.5
        f[:, 2, 6] *= np.array([1, 1, 1, 1.05, 1.6, 2.2, 2.25, 2.25])   # a steep ramp along x
        f[4, :, 0] *= np.array([2.25, 2.2, 1.6, 1.05, 1, 1, 1, 1])      # ... and down along y
        # plateaus along z, y and x (one across the box face), entered from both sides
        f[3, 1, 2:6] = f[3, 1, 2]
        f[6, 0, 1:4] = f[6, 0, 1]
        f[2, 3:7, 4] = f[2, 3, 4]
        f[7, 4:7, 1] = f[7, 4, 1]
        f[1:5, 7, 7] = f[1, 7, 7]
        f[[6, 7, 0], 3, 3] = f[6, 3, 3]
    return ϱ, J


def branch_of(r, thresholds):
    for n, T in enumerate(thresholds):
        if r > T:
            return n
    return len(thresholds)


def child_limiter(name):
    case = name[len('fluid_kt_limiter_'):-len('_g8')]
    given, function, thresholds = LIMITERS[case]
    text = param_text(W, given)
    ref = load(name, text)
    import fluid
    commons = ref.commons
    ϱ, J = sharp(commons)
    comp = make_fluid2(ref, ϱ, J)
    out = {}
    settings(ref, comp, out, text, W)
    assert out['limiter'] == given
    seen, ratio_seen, margin = set(), set(), [np.inf]
    ϕ, slope_ratio, ϵ = getattr(fluid, function), fluid.slope_ratio, fluid.slope_ratio_ϵ

    def watched_ϕ(r):
        seen.add(branch_of(r, thresholds))
        for T in thresholds:
            if r != 0:   # (r == 0: an exact plateau, or a numerator below slope_ratio_ϵ)
                margin[0] = min(margin[0], abs(r - T)/T if T else abs(r))
        return ϕ(r)

    def watched_slope_ratio(numerator, denominator):
        if abs(numerator) < ϵ:
            ratio_seen.add(0)
            assert numerator == 0, 'a numerator near slope_ratio_ϵ'
        elif abs(denominator) < ϵ:
            ratio_seen.add(1 if numerator > ϵ else 2)
            assert denominator == 0 and abs(numerator) > 1e+6*ϵ
        else:
            ratio_seen.add(3)
        return slope_ratio(numerator, denominator)
    setattr(fluid, function, watched_ϕ)
    fluid.slope_ratio = watched_slope_ratio
    drifts(name, ref, comp, out, [(1.0e-4, 2.3e-4, 1.4e-4)])
    print(name, 'branches of the limiter', sorted(seen), 'of slope_ratio', sorted(ratio_seen),
          'margin', margin[0], flush=True)
    assert seen == set(range(len(thresholds) + 1)), 'a branch of the limiter was not taken'
    assert ratio_seen == {0, 1, 2, 3}, 'a branch of slope_ratio was not taken'
    assert margin[0] >= MARGIN, f'an r is {margin[0]} from a threshold'
    out['margin'] = margin[0]
    save(name, out)


def child_kdk(name):
    text = param_text(W, 'mc')
    ref = load(name, text)
    commons, interactions = ref.commons, ref.interactions
    import fluid
    ϱ, J = warm_background(commons)
    comp = make_fluid2(ref, ϱ, J)
    out = {}
    settings(ref, comp, out, text, W)
    out.update(G_Newton=commons.G_Newton, nghosts=commons.nghosts,
               cell_centered=int(commons.cell_centered),
               deconvolve=np.array(commons.potential_options['deconvolve']['gravity']['pm'],
                                   dtype=np.int64))
    out['rho_in'], out['J_in'] = grids(commons, comp)
    steps = Steps(fluid)
    inter = interactions.find_interactions([comp], 'long-range')
    assert len(inter) == 1
    keys = ('1', 'a**(-3*w_eff)', 'a**(-3*w_eff-1)', 'a**(3*w_eff-2)')
    out['keys'] = np.array(keys)
    for r in range(3):
        dt = 2.0e-4 + 0.3e-4*r
        # (the kick's integral is far larger than a step of this size would give: the kick
        # changes J by 1e-4 of its size, where a wrong one shows)
        values = dict(zip(keys, (dt, 1.4*dt, 1.9e+4*dt, 2.3*dt)))
        ᔑdt = {'1': values['1']}
        for key in keys[1:]:
            ᔑdt[key, comp.name] = values[key]
        out[f'dt_{r}'] = np.array([values[k] for k in keys])
        before = grids(commons, comp)
        comp.apply_internal_sources(ᔑdt)
        after = grids(commons, comp)
        # (species.py:2902-2916: no internal source in this scheme under P = wρ)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        for force, method, receivers, suppliers in inter:
            getattr(interactions, force)(method, receivers, suppliers, ᔑdt, 'long-range', False)
        out[f'rho_kick_{r}'], out[f'J_kick_{r}'] = grids(commons, comp)
        comp.drift(ᔑdt)
        out[f'rho_{r}'], out[f'J_{r}'] = grids(commons, comp)
        out[f'P_{r}'] = noghosts(commons, comp.𝒫.grid_mv)
        out[f'a_steps_{r}'] = steps.take()
        print(name, 'round', r, 'max|ΔJ_kick|/max|J| =',
              np.abs(out[f'J_kick_{r}'] - before[1]).max()/np.abs(before[1]).max(),
              'max|Δϱ|/max|ϱ| =',
              np.abs(out[f'rho_{r}'] - before[0]).max()/np.abs(before[0]).max(), flush=True)
    assert shear_is_zero(commons, comp)
    save(name, out)


def child_scale_factors(name):
    text = param_text(0)
    ref = load(name, text)
    import fluid
    commons = ref.commons
    ϱ, J = background(commons.ρ_mbar, commons.boxsize)
    comp = make_fluid2(ref, ϱ, J)
    steps = Steps(fluid)
    pairs = [(0.5, 0.1), (0.5, 3e-4), (0.02, 1e-5), (0.7, 0.4), (0.95, 0.2)]
    out = {'param': text, 'a': np.array([p[0] for p in pairs]),
           'dt': np.array([p[1] for p in pairs])}
    found = []
    for a, dt in pairs:
        fluid.kurganov_tadmor(comp, sdt_of(comp, dt, 1e-3*dt, dt), a=a, rk_order=2)
        found.append(steps.take())
        assert len(found[-1]) == 2
        print(name, a, dt, found[-1], flush=True)
    out['a_steps'] = np.array(found)
    save(name, out)


def main():
    if len(sys.argv) > 1 and sys.argv[1] in CASES:
        name = sys.argv[1]
        child = {'fluid_kt_smooth_g8': child_smooth, 'fluid_kt_pressure_g8': child_pressure,
                 'fluid_kt_euler_g8': child_pressure, 'fluid_kt_kdk_g8': child_kdk,
                 'fluid_kt_rk_scale_factors': child_scale_factors}.get(name, child_limiter)
        child(name)
        return
    jobs = [(name, subprocess.Popen([sys.executable, os.path.abspath(__file__), name]))
            for name in CASES]
    for name, job in jobs:
        if job.wait():
            sys.exit(f'case {name} failed')


if __name__ == '__main__':
    main()
