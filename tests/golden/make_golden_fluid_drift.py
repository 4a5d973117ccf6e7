"""Golden vectors of the reference's MacCormack flux step (fluid.py:724-961, 1157-1363).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_fluid_drift.py
The reference is imported in pure-Python mode through oracle/refharness/ref_import.  The fluids
are built by hand (CLASS is not involved); the .npz files hold inputs, ᔑdt values, settings and
recorded grids only.

  fluid_drift_smooth_g8   sine-wave ϱ (contrast 0.3), J ≠ 0 in all directions, 𝒫 = 0: eight
                          maccormack() calls, one per step triple, ϱ and J after each; no call
                          may trigger a vacuum sweep
  fluid_drift_vacuum_g8   the same background with two deep voids, one across the x layers 3|4
                          (the boundary of two domains) and one across the box face x = 0 (the
                          periodic wrap): one maccormack() call; the attempts per step, the
                          sweeps per step, fac_time of the flagged cells of every sweep.  The
                          first step flags cells of both voids, the second comes clean
  fluid_drift_vacuum_abort_g8  deeper voids: the second step flags cells, sweeps `gridsize`
                          times and the reference gives up (see VOIDS below); the grids it
                          leaves behind, starred ones included
  fluid_kdk_g8            a self-gravitating w = 0 fluid on a PM grid of 8: three rounds of
                          gravity('pm', ...) and Component.drift(ᔑdt)

Every detection compare of the recorded calls is required to be at least MARGIN (relative) away
from its threshold, so that rounding cannot move a cell across it."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CASES = ('fluid_drift_smooth_g8', 'fluid_drift_vacuum_g8', 'fluid_drift_vacuum_abort_g8',
         'fluid_kdk_g8')
MARGIN = 1e-6
GS = 8


def param_text():
    return f"""
boxsize = 8*Mpc
potential_options = {{
    'gridsize': {{'global': {{'gravity': {{'pm': {GS}}}}}}},
    'differentiation': {{'fluid': {{'gravity': {{'pm': 2}}}}}},
}}
H0 = 70*km/s/Mpc
Ωcdm = 0.25
Ωb = 0.05
a_begin = 0.5
enable_class_background = False
select_forces = {{'all': {{'gravity': 'pm'}}}}
select_boltzmann_closure = {{'all': 'truncate'}}
select_approximations = {{'all': {{'P=wρ': True}}}}
"""


def background(ρ_mbar, L):
    """sine-wave ϱ of contrast 0.3 and J ≠ 0 in all three directions"""
    q = (np.arange(GS) + 0.5)*(2*np.pi/GS)
    x, y, z = np.meshgrid(q, q, q, indexing='ij')
    ϱ = ρ_mbar*(1 + 0.3*np.sin(x)*np.cos(y + 0.4) + 0.1*np.sin(2*z + x))
    u = [0.35*np.sin(y + 0.3) + 0.2*np.cos(z), -0.3*np.cos(x + z) + 0.1, 0.25*np.sin(x - y) - 0.15]
    return ϱ, [ϱ*u_d for u_d in u]


def voids(ϱ, J, ρ_mbar, depth, outflow):
    """two voids of 2x2x2 cells, one across the x layers 3|4 and one across the box face x = 0:
    a density `depth` times the mean, and the J of their cells pointing out of them"""
    ϱ, J = ϱ.copy(), [j.copy() for j in J]
    for xs, (y0, z0) in (((3, 4), (2, 5)), ((GS - 1, 0), (5, 1))):
        for ix, x in enumerate(xs):
            for iy in range(2):
                for iz in range(2):
                    cell = (x, y0 + iy, z0 + iz)
                    ϱ[cell] = depth*ρ_mbar
                    for d, side in enumerate((ix, iy, iz)):
                        J[d][cell] = outflow*ρ_mbar*(1 if side else -1)
    return ϱ, J


def noghosts(commons, grid_mv):
    ng = commons.nghosts
    return np.array(grid_mv)[ng:-ng, ng:-ng, ng:-ng].copy()


def make_fluid(ref, ϱ, J, name='fluid'):
    comp = ref.species.Component(name, 'matter', gridsize=GS, boltzmann_order=1)
    comp.populate(np.ascontiguousarray(ϱ), 'ϱ')
    for d in range(3):
        comp.populate(np.ascontiguousarray(J[d]), 'J', d)
    comp.communicate_nonlinear_fluid_grids('=')
    return comp


def grids(commons, comp):
    return (noghosts(commons, comp.ϱ.grid_mv),
            np.stack([noghosts(commons, comp.J[d].grid_mv) for d in range(3)]))


class Watch:
    """counts the attempts and sweeps of the reference's maccormack() and looks at every
    detection compare before correct_vacuum runs"""

    def __init__(self, ref, fluid):
        self.commons, self.fluid = ref.commons, fluid
        self.attempts, self.sweeps, self.fac_time, self.margin = [0, 0], [0, 0], [], np.inf
        self.orig = fluid.correct_vacuum
        fluid.correct_vacuum = self

    def __call__(self, component, mc_step):
        commons = self.commons
        ρ_vacuum = commons.ρ_vacuum
        foresight = commons.is_selected(
            component, commons.fluid_options['maccormack']['foresight_select'])
        ϱ = noghosts(commons, component.ϱ.grid_mv)
        ϱˣ = noghosts(commons, component.ϱ.gridˣ_mv)
        if mc_step == 0:
            lhs, threshold = ϱ*(2/foresight - 1) + ϱˣ, 2/foresight*ρ_vacuum
            scale = np.maximum(np.abs(ϱ*(2/foresight - 1)), np.abs(ϱˣ))
            with np.errstate(all='ignore'):
                fac_time = np.where(lhs < threshold, 0.5*(ϱ - ϱˣ)/(ϱ - ρ_vacuum), 0.0)
        else:
            lhs, threshold = ϱ, 2*ρ_vacuum   # (the unstarred grid: the roles are swapped)
            scale = np.abs(ϱ)
            fac_time = np.where(lhs < threshold, 1.0, 0.0)
        self.margin = min(self.margin, float(np.min(np.abs(lhs - threshold)
                                                    /np.maximum(scale, threshold))))
        self.attempts[mc_step] += 1
        swept = self.orig(component, mc_step)
        assert bool(swept) == bool(np.any(lhs < threshold))
        if swept:
            self.sweeps[mc_step] += 1
            self.fac_time.append((mc_step, fac_time))
        return swept

    def reset(self):
        self.attempts, self.sweeps, self.fac_time = [0, 0], [0, 0], []


def settings(commons, comp, out):
    mc = commons.fluid_options['maccormack']
    out.update(
        boxsize=commons.boxsize, gridsize=GS, light_speed=commons.light_speed,
        ρ_vacuum=commons.ρ_vacuum, ρ_mbar=commons.ρ_mbar, param=param_text(),
        foresight=commons.is_selected(comp, mc['foresight_select']),
        smoothing=commons.is_selected(comp, mc['smoothing_select']),
        vacuum_corrections=bool(commons.is_selected(comp, mc['vacuum_corrections_select'])),
        max_vacuum_corrections=np.array(
            [GS if v == 'gridsize' else v
             for v in commons.is_selected(comp, mc['max_vacuum_corrections_select'])]))


def child_drift(name):
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    ref = load_reference(param_text(), f'/tmp/concept_golden_work/{name}')
    commons = ref.commons
    import fluid
    ϱ, J = background(commons.ρ_mbar, commons.boxsize)
    vacuum = name in VOIDS
    abort = name == 'fluid_drift_vacuum_abort_g8'
    if vacuum:
        depth, outflow, void_dt = VOIDS[name]
        ϱ, J = voids(ϱ, J, commons.ρ_mbar, depth=depth, outflow=outflow)
    comp = make_fluid(ref, ϱ, J)
    out = {}
    settings(commons, comp, out)
    out['rho_in'], out['J_in'] = grids(commons, comp)
    out['P_in'] = noghosts(commons, comp.𝒫.grid_mv)
    watch = Watch(ref, fluid)
    ncalls = 1 if vacuum else 8
    dts = [void_dt] if vacuum else [0.21 - 0.01*i for i in range(ncalls)]
    out['dt'] = np.array(dts)
    for i, dt in enumerate(dts):
        watch.reset()
        try:
            fluid.maccormack(comp, {('a**(3*w_eff-2)', comp.name): dt, '1': dt})
            assert not abort, 'the reference did not give up'
        except RuntimeError:   # (the one-rank MPI stand-in's Abort)
            assert abort, 'the reference gave up'
            # what the reference leaves behind: the unstarred grids (not yet halved) and the
            # starred ones, which the sweeps of the second step smooth (fluid.py:1229-1237)
            out['rho_starred'] = noghosts(commons, comp.ϱ.gridˣ_mv)
            out['J_starred'] = np.stack([noghosts(commons, comp.J[d].gridˣ_mv)
                                         for d in range(3)])
        out[f'rho_{i}'], out[f'J_{i}'] = grids(commons, comp)
        out[f'attempts_{i}'] = np.array(watch.attempts)
        out[f'sweeps_{i}'] = np.array(watch.sweeps)
        print(name, 'call', i, 'attempts', watch.attempts, 'sweeps', watch.sweeps, 'margin',
              watch.margin, 'min ϱ/ϱ_bar', out[f'rho_{i}'].min()/commons.ρ_mbar, flush=True)
        if not vacuum:
            assert watch.sweeps == [0, 0], 'a call of the smooth case triggered a vacuum sweep'
        else:
            for s, (mc_step, fac_time) in enumerate(watch.fac_time):
                out[f'sweep{s}_mc_step'] = mc_step
                out[f'sweep{s}_fac_time'] = fac_time
                print('  sweep', s, 'step', mc_step, 'flagged', int(np.count_nonzero(fac_time)))
            out['n_sweeps'] = len(watch.fac_time)
            assert watch.sweeps[0] >= 1, 'step 0 flagged no cell'
            if abort:
                assert watch.sweeps[1] >= 2, 'step 1 needed fewer than two correction sweeps'
            else:
                assert watch.sweeps[1] == 0
    out['P_out'] = noghosts(commons, comp.𝒫.grid_mv)
    assert watch.margin >= MARGIN, f'a detection compare is {watch.margin} from its threshold'
    out['margin'] = watch.margin
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name)


# (depth, outflow, ᔑdt) of the voids.  The reference's second step detects vacuum on the
# unstarred ϱ but corrects the starred grids (the swapped roles of fluid.py:1229-1237), so a
# second step that flags a cell flags it again on every attempt and maccormack() gives up: no
# call of the reference both sweeps in its second step and returns.  fluid_drift_vacuum_g8 is
# tuned so that the first step flags cells and the second comes clean;
# fluid_drift_vacuum_abort_g8 so that the second step flags, sweeps `gridsize` times and gives up.
VOIDS = {'fluid_drift_vacuum_g8': (0.3, 0.05, 0.2),
         'fluid_drift_vacuum_abort_g8': (0.02, 0.05, 0.2)}


def child_kdk(name):
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    ref = load_reference(param_text(), f'/tmp/concept_golden_work/{name}')
    commons, interactions = ref.commons, ref.interactions
    import fluid
    ϱ, J = background(commons.ρ_mbar, commons.boxsize)
    comp = make_fluid(ref, ϱ, [0.2*j for j in J])
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
    rounds = 3
    keys = ('1', 'a**(-3*w_eff)', 'a**(-3*w_eff-1)', 'a**(3*w_eff-2)')
    out['keys'] = np.array(keys)
    for r in range(rounds):
        dt = 0.15 + 0.02*r
        values = dict(zip(keys, (dt, 0.9*dt, 1.7*dt, 1.3*dt)))
        ᔑdt = {'1': values['1']}
        for key in keys[1:]:
            ᔑdt[key, comp.name] = values[key]
        out[f'dt_{r}'] = np.array([values[k] for k in keys])
        for force, method, receivers, suppliers in inter:
            getattr(interactions, force)(method, receivers, suppliers, ᔑdt, 'long-range', False)
        out[f'rho_kick_{r}'], out[f'J_kick_{r}'] = grids(commons, comp)
        comp.drift(ᔑdt)
        out[f'rho_{r}'], out[f'J_{r}'] = grids(commons, comp)
        print(name, 'round', r, 'sweeps', watch.sweeps, 'margin', watch.margin, flush=True)
    assert watch.sweeps == [0, 0]
    assert watch.margin >= MARGIN
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name)


def main():
    if len(sys.argv) > 1 and sys.argv[1] in CASES:
        (child_kdk if sys.argv[1] == 'fluid_kdk_g8' else child_drift)(sys.argv[1])
        return
    for name in CASES:
        print('===', name, flush=True)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name])
        if r.returncode:
            sys.exit(f'case {name} failed')


if __name__ == '__main__':
    main()
