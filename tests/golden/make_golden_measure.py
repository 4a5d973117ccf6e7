"""Golden vectors of the reference's measure() (analysis.py:3860-4230): every quantity of one
particle component (N = 64) and one fluid component (gridsize 8, boltzmann_order = 1, w = 0.1).

Run in the development container:  python tests/golden/make_golden_measure.py
The reference is imported in pure-Python mode through oracle/refharness/ref_import, as in
make_golden_fluid_drift.py, whose background() is reused.  The .npz file holds inputs, settings
and the numbers measure() returned only.

  measure_g8   particles: 'v_max', 'v_rms', 'momentum', 'mass'
               fluid:     the same and 'ϱ', 'discontinuity' (five fluid scalars: ϱ, Jx, Jy, Jz and
               𝒫, the last two named alike by the reference: both are '<fluidscalar 0[0]>')
The 𝒫 grid is filled by hand with ϱ c²w: with boltzmann_order = 1 the reference's realize() leaves
it at 0 (see make_golden_fluid_pressure.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_fluid_drift as drift_golden   # noqa: E402
from make_golden_fluid_drift import background, grids, noghosts  # noqa: E402

NAME = 'measure_g8'
W = 0.1
N = 64
MASS_FACTOR = 1.0   # particle mass in units of ρ_mbar boxsize³/N


def param_text():
    return drift_golden.param_text() + f"select_eos_w = {{'fluid': {W}}}\n"


def main():
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    ref = load_reference(param_text(), f'/tmp/concept_golden_work/{NAME}')
    commons, species = ref.commons, ref.species
    import analysis
    if sys.version_info < (3, 11):
        # decimal.localcontext(prec=...) (analysis.py:4031) is the 3.11 signature: a driver-side
        # shim like those of ref_import, nothing in the reference is edited
        import decimal
        _localcontext = decimal.localcontext

        def localcontext(ctx=None, **kwargs):
            ctx = (ctx or decimal.getcontext()).copy()
            for key, value in kwargs.items():
                setattr(ctx, key, value)
            return _localcontext(ctx)
        decimal.localcontext = localcontext
    a = float(commons.universals.a)
    out = dict(param=param_text(), a=a, t=float(commons.universals.t), w=W,
               boxsize=commons.boxsize, light_speed=commons.light_speed, N=N)

    # the particle component
    rng = np.random.default_rng(20240611)
    mass = MASS_FACTOR*commons.ρ_mbar*commons.boxsize**3/N
    pos = rng.random((N, 3))*commons.boxsize
    mom = mass*(rng.standard_normal((N, 3))*np.array([30.0, 50.0, 80.0]) + np.array([3.0, -2.0, 0.5]))
    particles = species.Component('particles', 'matter', N=N, mass=mass)
    for d, s_ in enumerate('xyz'):
        particles.populate(np.ascontiguousarray(pos[:, d]), 'pos' + s_)
        particles.populate(np.ascontiguousarray(mom[:, d]), 'mom' + s_)
    out.update(mass=mass, pos=pos, mom=mom)
    for quantity in ('v_max', 'v_rms', 'mass'):
        out[f'particles_{quantity}'] = float(analysis.measure(particles, quantity))
    Σmom, σmom = analysis.measure(particles, 'momentum')
    out['particles_momentum_sum'], out['particles_momentum_sigma'] = np.array(Σmom), np.array(σmom)

    # the fluid component
    ϱ, J = background(commons.ρ_mbar, commons.boxsize)
    fluid = drift_golden.make_fluid(ref, ϱ, J)
    assert fluid.w_constant == W and fluid.w_eff(a=a) == W and fluid.w(a=a) == W
    assert fluid.approximations['P=wρ'] and fluid.boltzmann_closure == 'truncate'
    ng = commons.nghosts
    𝒫_mv = np.asarray(fluid.𝒫.grid_mv)
    𝒫_mv[ng:-ng, ng:-ng, ng:-ng] = ϱ*(commons.light_speed**2*W)
    ref.communication.communicate_ghosts(fluid.𝒫.grid_mv, '=')
    out['rho_in'], out['J_in'] = grids(commons, fluid)
    out['P_in'] = noghosts(commons, fluid.𝒫.grid_mv)
    assert np.array_equal(out['P_in'], ϱ*(commons.light_speed**2*W))
    for quantity in ('v_max', 'v_rms', 'mass'):
        out[f'fluid_{quantity}'] = float(analysis.measure(fluid, quantity))
    Σmom, σmom = analysis.measure(fluid, 'momentum')
    out['fluid_momentum_sum'], out['fluid_momentum_sigma'] = np.array(Σmom), np.array(σmom)
    out['fluid_rho'] = np.array([float(x) for x in analysis.measure(fluid, 'ϱ')])
    names, Δdiff_max_list, Δdiff_max_normalized_list = analysis.measure(fluid, 'discontinuity')
    out['fluid_discontinuity_names'] = np.array(names)
    out['fluid_discontinuity'] = np.array(Δdiff_max_list)
    out['fluid_discontinuity_normalized'] = np.array(Δdiff_max_normalized_list)
    for key in sorted(out):
        if key not in ('param', 'pos', 'mom', 'rho_in', 'J_in', 'P_in'):
            print(key, out[key])
    np.savez_compressed(os.path.join(HERE, NAME + '.npz'), **out)
    print('wrote', NAME)


if __name__ == '__main__':
    main()
