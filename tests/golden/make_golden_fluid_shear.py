"""Golden vector of the reference's rank-2 realisation and its order-2 difference (realize_grid
with variable 2, ic.py:743-764; diff_domaingrid, mesh.py:4966-4970): what
maccormack_internal_sources (fluid.py:1011-1043) differentiates for closure 'class'.

Run in the development container:  python tests/golden/make_golden_fluid_shear.py
The reference is imported in pure-Python mode through oracle/refharness, the way
make_golden_fluid_ic.py imports it.  No CLASS: the structure slab is made by the reference's own
slab_decompose and fft from a made-up density, the table of amplitudes is made up, and
realize_grid(gridsize, None, a, amplitudes, 2, multi_index=(m, n), slab_structure=…) is called
for the six elements, each followed by domain_decompose and diff_domaingrid(·, j, 2, Δx) for the
j of {m, n}.  fluid_shear_g8.npz holds the density ('rho'), the table, the six σₘₙ ('sigma_mn',
realize_grid's output without the factor ϱ_bar(1 + w)) and the differences ('dsigma_mn_j'), all
without ghost layers."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
G, A = 8, 0.5
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def main():
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    text = ('boxsize = 100.0*Mpc\nH0 = 70*km/s/Mpc\nΩcdm = 0.25\nΩb = 0.05\n'
            f'a_begin = {A}\nenable_class_background = False\n')
    ref = load_reference(text, '/tmp/concept_golden_work/fluid_shear_g8')
    commons = ref.commons
    ic, mesh = importlib.import_module('ic'), importlib.import_module('mesh')
    L, nghosts = commons.boxsize, commons.nghosts
    inner = (slice(nghosts, -nghosts),)*3
    rng = np.random.default_rng(G)
    ϱ = 2.5*(1 + 0.3*rng.uniform(-1, 1, (G, G, G)))
    table = np.zeros(3*(G//2 - 1)**2 + 1)
    table[1:] = rng.uniform(0.5, 2.0, table.size - 1)*rng.choice([-1.0, 1.0], table.size - 1)
    table *= float(G)**(-3)
    grid = np.zeros((G + 2*nghosts,)*3)
    grid[inner] = ϱ
    slab_structure = mesh.get_fftw_slab(G, 'slab_structure_golden')
    mesh.slab_decompose(grid, slab_structure)
    mesh.fft(slab_structure, 'forward')
    out = dict(param_text=text, gridsize=G, boxsize=L, a=A, rho=ϱ, amplitudes=table)
    for m, n in PAIRS:
        slab = ic.realize_grid(G, None, A, table, 2, multi_index=(m, n),
                               slab_structure=slab_structure)
        domain = np.zeros((G + 2*nghosts,)*3)
        mesh.domain_decompose(slab, domain)
        out[f'sigma_{m}{n}'] = domain[inner].copy()
        for j in sorted({m, n}):
            d = np.array(mesh.diff_domaingrid(domain, j, 2, L/G))
            out[f'dsigma_{m}{n}_{j}'] = (d if d.shape[0] == G else d[inner]).copy()
        assert np.abs(out[f'sigma_{m}{n}']).max() > 0
    np.savez_compressed(os.path.join(HERE, 'fluid_shear_g8.npz'), **out)
    print('wrote fluid_shear_g8', {k: getattr(v, 'shape', v) for k, v in out.items()
                                   if k != 'param_text'})


if __name__ == '__main__':
    main()
