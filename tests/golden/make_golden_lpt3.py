"""Golden vectors of the reference's 3LPT and dealiased particle realisations (ic.py:1199-2103).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_lpt3.py
Written like make_golden_lpt.py, whose spectrum, first- and second-order growth factors and
replacements of module attributes it shares; the third-order growth factors are non-zero, of the
size that makes each third-order potential comparable to Φ⁽²⁾.  Two further wrappers record:
  ic.get_lpt_grid   the grids in the order realize_particles asks for them (Φ1, tmp0, Φ2, tmp1,
                    Φ3, the two enlarged ones), by which a potential is told from its address
  ic.diff_ifft      every call as (potential, i, j, factor, enlarged or not)
Each lpt3_<case>_g<N>.npz holds what lpt_<case>_g<N>.npz holds, every potential after
laplacian_inverse with its factor (Phi1 [, Phi1_theta], Phi2, Phi3a, Phi3b, A3c0, A3c1, A3c2) and
the sequence of diff_ifft calls.

The maker asserts, and prints, what keeps a test from hiding a missing piece: each third-order
potential alone displaces some particle by at least 1e-3 of a cell; each dealiased case differs
from its un-dealiased twin (run in the same process) by at least 1e-3 of a cell somewhere; all
positions end in [0, boxsize)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_lpt import A, param_text, tables  # noqa: E402
from make_golden_lpt import GROWTH as GROWTH_2  # noqa: E402

GROWTH = dict(GROWTH_2, D3a=2.1e-6, f3a=3.05, D3b=5.3e-6, f3b=2.97, D3c=-1.9e-6, f3c=3.1)

# name -> (realization_options, further parameters, (components_tally, components_total))
CASES = {
    '3lpt': ({'lpt': 3, 'backscale': True}, {}, (0, 1)),
    '3lpt_dealias': ({'lpt': 3, 'backscale': True, 'dealias': True}, {}, (0, 1)),
    '2lpt_dealias': ({'lpt': 2, 'backscale': True, 'dealias': True}, {}, (0, 1)),
    '3lpt_bcc2': ({'lpt': 3}, {}, (1, 2)),
    '3lpt_dealias_vertex': ({'lpt': 3, 'backscale': True, 'dealias': True},
                            {'cell_centered': False}, (0, 1)),
}
GRIDSIZES = {name: (8, 12) for name in CASES}
GRIDSIZES['3lpt_dealias'] = (8, 10, 12)  # 10: M = 16 takes the +1 and the hand-written transform
THIRD_ORDER = ('Phi3a', 'Phi3b', 'A3c0', 'A3c1', 'A3c2')


def child(name, g):
    import importlib
    import types
    import numpy as np
    import lpt_refs
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    options, extra, (tally, total) = CASES[name]
    text = param_text(options, extra)
    ref = load_reference(text, f'/tmp/concept_golden_work/lpt3_{name}_g{g}')
    commons, species, integration = ref.commons, ref.species, ref.integration
    ic = importlib.import_module('ic')
    L = commons.boxsize
    N = g**3
    cell = L/g
    amp, amp_θ = tables(g, L)
    recorded = {}
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
    orig_get_lpt_grid = ic.get_lpt_grid

    def address(grid):
        return np.asarray(grid).__array_interface__['data'][0]

    def get_lpt_grid(*args, **kwargs):
        grid, buffer_number = orig_get_lpt_grid(*args, **kwargs)
        recorded['grids'].append(address(grid))
        return grid, buffer_number
    ic.get_lpt_grid = get_lpt_grid
    orig_diff_ifft = ic.diff_ifft
    lpt = options['lpt']
    # the order of get_lpt_grid in realize_particles (ic.py:1304-1315)
    grid_names = ['Φ1', 'tmp0', 'Φ2', 'tmp1', 'Φ3'][:{2: 4, 3: 5}[lpt]]

    def diff_ifft(Φ, out, out_dealias, i, j=-1, factor=1):
        names = dict(zip(recorded['grids'], grid_names))
        enlarged = out_dealias is not None and out_dealias.shape[1] > Φ.shape[1]
        recorded['diffs'].append((names[address(Φ)], int(i), int(j), float(factor),
                                  bool(enlarged)))
        return orig_diff_ifft(Φ, out, out_dealias, i, j, factor)
    ic.diff_ifft = diff_ifft

    mass = commons.ρ_mbar*L**3/N
    id_bgn = tally*N

    def run(dealias):
        recorded.update(potentials=[], grids=[], diffs=[])
        comp = species.Component('matter', 'matter', N=N, mass=mass)
        comp.realization_options['dealias'] = dealias
        ic.n_particles_realized.update(components_tally=tally, components_total=total,
                                       particles_tally=id_bgn)
        # with components_tally == 0 realize_particles counts the components to be realised
        # itself, by mass == -1 (this one has its mass): make that count come out as `total`
        comp.components_all = [types.SimpleNamespace(representation='particles', mass=-1, N=N)
                               for _ in range(total)]
        ic.realize_particles(comp, A)
        return comp

    def distance(x, y):
        d = np.abs(x - y)
        return np.minimum(d, L - d).max()/cell

    dealias = bool(options.get('dealias', False))
    if dealias:
        twin = np.array(run(False).pos_mv3).copy()
    comp = run(dealias)
    pots = recorded['potentials']
    backscale = options.get('backscale', False)
    n_first = 1 if backscale else 2
    assert len(pots) == n_first + {2: 1, 3: 6}[lpt], len(pots)
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
    out['Phi1'] = pots[n_first - 1][1]
    names = ('Phi2',) + THIRD_ORDER*(lpt == 3)
    for key, (factor, slab) in zip(names, pots[n_first:]):
        out[key] = slab
        out[key + '_factor'] = factor
    diffs = recorded['diffs']
    out['diff_potential'] = np.array([d[0] for d in diffs])
    out['diff_dims'] = np.array([d[1:3] for d in diffs], dtype=np.int64)
    out['diff_factor'] = np.array([d[3] for d in diffs])
    out['diff_enlarged'] = np.array([d[4] for d in diffs])
    lattice = (np.stack(np.meshgrid(*[np.arange(g)]*3, indexing='ij'), -1).reshape(-1, 3)
               + 0.5*commons.cell_centered)*cell
    d = (out['pos'] - lattice + L/2) % L - L/2
    print(f'{name} g{g}: displacement rms {d.std()/cell:.3f} max {np.abs(d).max()/cell:.3f} '
          f'cells, max |mom| {np.abs(out["mom"]).max():.4g}, pos in '
          f'[{out["pos"].min():.4g}, {out["pos"].max():.4g}], {len(diffs)} diff_ifft calls')
    assert out['pos'].min() >= 0 and out['pos'].max() < L
    # each third-order potential alone moves some particle by 1e-3 of a cell or more
    live = np.repeat(lpt_refs.alive(g), 2, axis=2)
    for key in names[1:]:
        dims = ((0, 1.0), (1, 1.0), (2, 1.0)) if key[0] == 'P' else (
            ((int(key[-1]) + 1) % 3, 1.0), ((int(key[-1]) + 2) % 3, -1.0))
        moved = max(np.abs(lpt_refs.to_real(lpt_refs.diff(out[key]*live, dim, -1, sign, L))).max()
                    for dim, sign in dims)/cell
        print(f'  {key} alone displaces by up to {moved:.3e} cells '
              f'(max |{key}| = {np.abs(out[key]*live).max():.3e}, '
              f'max |Phi2| = {np.abs(out["Phi2"]*live).max():.3e})')
        assert moved >= 1e-3, (key, moved)
    if dealias:
        moved = distance(out['pos'], twin)
        print(f'  dealiasing moves particles by up to {moved:.3e} cells')
        assert moved >= 1e-3, moved
    np.savez_compressed(os.path.join(HERE, f'lpt3_{name}_g{g}.npz'), **out)
    print('wrote', f'lpt3_{name}_g{g}', {k: getattr(v, 'shape', v) for k, v in out.items()
                                          if k != 'param_text'})


def main():
    if len(sys.argv) > 1:
        child(sys.argv[1], int(sys.argv[2]))
        return
    for name in CASES:
        for g in GRIDSIZES[name]:
            print('===', name, g, flush=True)
            log = f'/tmp/concept_golden_lpt3_{name}_g{g}.log'
            with open(log, 'w') as f:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(g)],
                                   stdout=f, stderr=subprocess.STDOUT)
            print('\n'.join(open(log).read().splitlines()[-9:]))
            if r.returncode:
                sys.exit(f'case {name} g{g} failed, see {log}')


if __name__ == '__main__':
    main()
