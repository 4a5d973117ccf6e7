"""Golden vectors of the reference's particle realisation (ic.py:1199-1589, 2038-2280).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_lpt.py
The reference is imported in pure-Python mode through oracle/refharness, its `ic` module the way
make_golden.py imports `main`.  realize_particles is driven whole; CLASS is kept out by two
replacements of module attributes:
  ic.get_amplitudes   a lookup in the tables below (δ for variable 0, θ for variable 1)
  ic.compute_cosmo    an object whose growth_fac_*(a) return the fixed numbers below
and three wrappers that only record: generate_primordial_noise (the noise slab after the call),
laplacian_inverse (the potential after every call: Φ⁽¹⁾ of θ, Φ⁽¹⁾ of δ, Φ⁽²⁾) and
preinitialize_particles (the positions on the lattice).
Each lpt_<case>_g<N>.npz holds the noise slab (its Nyquist planes, which the reference leaves
as it finds them, set to zero), the tables and growth factors, the potentials in Fourier space,
the lattice positions and the final pos, mom, ids."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

A = 0.02
GROWTH = {'D1': 0.02, 'f1': 0.98, 'D2': -1.7e-4, 'f2': 2.03, 'D3a': 0.0, 'f3a': 0.0, 'D3b': 0.0,
          'f3b': 0.0, 'D3c': 0.0, 'f3c': 0.0}

# name -> (realization_options, further parameters, (components_tally, components_total))
CASES = {
    '1lpt': ({}, {}, (0, 1)),
    '1lpt_backscale': ({'backscale': True}, {}, (0, 1)),
    '2lpt': ({'lpt': 2, 'backscale': True}, {}, (0, 1)),
    '2lpt_bcc2': ({'lpt': 2}, {}, (1, 2)),
    '1lpt_fixed_shift': ({}, {'primordial_amplitude_fixed': True,
                              'primordial_phase_shift': 'π'}, (0, 1)),
    '2lpt_vertex': ({'lpt': 2, 'backscale': True}, {'cell_centered': False}, (0, 1)),
    '1lpt_simple': ({}, {'primordial_noise_imprinting': "'simple'"}, (0, 1)),
}
GRIDSIZES = (8, 12)


def param_text(options, extra):
    lines = ['boxsize = 100.0*Mpc', 'H0 = 70*km/s/Mpc', 'Ωcdm = 0.25', 'Ωb = 0.05',
             f'a_begin = {A}', 'enable_class_background = False',
             "select_particle_id = {'all': True}",
             f'realization_options = {options!r}']
    lines += [f'{key} = {val}' for key, val in extra.items()]
    return '\n'.join(lines) + '\n'


def tables(g, boxsize):
    """a smooth made-up spectrum: displacements of a few tenths of a cell at N = 8 and 12, so
    that some particles cross a cell face and the box edge"""
    import numpy as np
    k2 = np.arange(3*(g//2 - 1)**2 + 1, dtype=np.float64)
    k = 2*np.pi/boxsize*np.sqrt(k2)
    amp = np.zeros_like(k2)
    amp[1:] = 0.2*k[1:]**0.5/(1 + (k[1:]/0.25)**2)
    amp_θ = -0.9*amp*(1 + 0.2*k/k[-1])
    return amp, amp_θ


def child(name, g):
    import importlib
    import types
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    options, extra, (tally, total) = CASES[name]
    text = param_text(options, extra)
    ref = load_reference(text, f'/tmp/concept_golden_work/lpt_{name}_g{g}')
    commons, species, integration = ref.commons, ref.species, ref.integration
    ic = importlib.import_module('ic')
    L = commons.boxsize
    N = g**3
    amp, amp_θ = tables(g, L)
    recorded = {'potentials': []}
    nyq = g//2

    ic.get_amplitudes = lambda gridsize, component, a, variable=0, **kw: (
        amp_θ if variable == 1 else amp).copy()
    ic.compute_cosmo = lambda **kw: types.SimpleNamespace(
        **{f'growth_fac_{key}': (lambda a, v=val: v) for key, val in GROWTH.items()})
    orig_noise = ic.generate_primordial_noise

    def noise(slab, fixed_amplitude=False, phase_shift=0):
        orig_noise(slab, fixed_amplitude, phase_shift)
        copy = np.array(slab).copy()
        copy[nyq, :, :] = 0
        copy[:, nyq, :] = 0
        copy[:, :, 2*nyq:] = 0
        recorded['noise'] = copy
    ic.generate_primordial_noise = noise
    orig_laplacian_inverse = ic.laplacian_inverse

    def laplacian_inverse(source, factor=1):
        out = orig_laplacian_inverse(source, factor)
        recorded['potentials'].append((factor, np.array(out).copy()))
        return out
    ic.laplacian_inverse = laplacian_inverse
    orig_preinitialize = ic.preinitialize_particles

    def preinitialize_particles(component, *args, **kwargs):
        n_local = orig_preinitialize(component, *args, **kwargs)
        recorded['pos_lattice'] = np.array(component.pos_mv3).copy()
        return n_local
    ic.preinitialize_particles = preinitialize_particles

    mass = commons.ρ_mbar*L**3/N
    comp = species.Component('matter', 'matter', N=N, mass=mass)
    id_bgn = tally*N
    ic.n_particles_realized.update(components_tally=tally, components_total=total,
                                   particles_tally=id_bgn)
    # with components_tally == 0 realize_particles counts the components to be realised itself,
    # by mass == -1 (this one has its mass): make that count come out as `total`
    comp.components_all = [types.SimpleNamespace(representation='particles', mass=-1, N=N)
                           for _ in range(total)]
    ic.realize_particles(comp, A)
    pots = recorded['potentials']
    lpt = options.get('lpt', 1)
    backscale = options.get('backscale', False)
    assert len(pots) == (1 if backscale else 2) + (lpt == 2), len(pots)
    out = dict(param_text=text, gridsize=g, boxsize=L, a=A, mass=mass, id_bgn=id_bgn,
               components_tally=tally, components_total=total,
               cell_centered=bool(commons.cell_centered), hubble=integration.hubble(A),
               amplitudes=amp, amplitudes_θ=amp_θ, noise=recorded['noise'],
               pos_lattice=recorded['pos_lattice'],
               growth_keys=np.array(list(GROWTH)), growth_values=np.array(list(GROWTH.values())),
               pos=np.array(comp.pos_mv3).copy(), mom=np.array(comp.mom_mv3).copy(),
               ids=np.array(comp.ids_mv).copy())
    if not backscale:
        assert pots[0][0] == 1 and pots[1][0] == -1
        out['Phi1_theta'] = pots[0][1]
    out['Phi1'] = pots[0 if backscale else 1][1]
    if lpt == 2:
        out['Phi2'] = pots[-1][1]
        out['potential_factor'] = pots[-1][0]
    cell = L/g
    lattice = (np.stack(np.meshgrid(*[np.arange(g)]*3, indexing='ij'), -1).reshape(-1, 3)
               + 0.5*commons.cell_centered)*cell
    d = (out['pos'] - lattice + L/2) % L - L/2
    print(f'{name} g{g}: displacement rms {d.std()/cell:.3f} max {np.abs(d).max()/cell:.3f} '
          f'cells, max |mom| {np.abs(out["mom"]).max():.4g}, pos in '
          f'[{out["pos"].min():.4g}, {out["pos"].max():.4g}]')
    assert out['pos'].min() >= 0 and out['pos'].max() < L
    np.savez_compressed(os.path.join(HERE, f'lpt_{name}_g{g}.npz'), **out)
    print('wrote', f'lpt_{name}_g{g}', {k: getattr(v, 'shape', v) for k, v in out.items()
                                         if k != 'param_text'})


def main():
    if len(sys.argv) > 1:
        child(sys.argv[1], int(sys.argv[2]))
        return
    for name in CASES:
        for g in GRIDSIZES:
            print('===', name, g, flush=True)
            log = f'/tmp/concept_golden_lpt_{name}_g{g}.log'
            with open(log, 'w') as f:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(g)],
                                   stdout=f, stderr=subprocess.STDOUT)
            print('\n'.join(open(log).read().splitlines()[-3:]))
            if r.returncode:
                sys.exit(f'case {name} g{g} failed, see {log}')


if __name__ == '__main__':
    main()
