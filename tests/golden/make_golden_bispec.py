"""Golden vectors of the reference's bispectrum core (analysis.py:2576-2982).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_bispec.py
The reference is imported in pure-Python mode the way make_golden_powerspec.py does it, with
its graphics / ic / linear stand-ins.  The reference's own functions are called directly:
  bispec_overlap.npz      get_bispec_overlap_cellshell on a list of (ki, kj, kk, k_inner,
                          k_outer) cases
  bispec_value_g<N>.npz   a seeded random real field, its Fourier slab through slab_decompose
                          + fft, and compute_bispec_value over a list of bins with and without
                          slab_data, for both settings of bispec_antialiasing
get_bispec_bins is not called (it needs h5py)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

PARAM = """
boxsize = 100.0*Mpc
H0 = 70*km/s/Mpc
Ωcdm = 0.25
Ωb = 0.05
a_begin = 0.5
enable_class_background = False
"""

# the bins of the value goldens, as functions of the Nyquist number: three distinct shells;
# two equal and one different in both multiplicity orders; three equal; an empty shell (no
# integer mode near it); a shell reaching nyquist - 1; consecutive bins share shells, so the
# reference's grid cache is hit
def value_bins(nyq):
    s1, s2, s3 = (0.5, 1.5), (1.5, 2.5), (2.25, 3.0)
    top = (nyq - 2.0, nyq - 0.5)
    thin = (1.0 - 0.125, 1.0 + 0.125)
    empty = (1.1, 1.3)
    return [(s1, s2, s3), (s1, s2, s2), (s2, s2, s3), (s2, s3, s3), (s3, s3, s3), (s3, s3, top),
            (s1, s2, top), (thin, thin, s2), (thin, thin, thin), (empty, s1, s2),
            (empty, empty, empty), (top, top, top), ((0.0, 1.5), s2, s2)]


def overlap_cases(rng):
    import numpy as np
    cases = []

    def add(ki, kj, kk, k_inner, k_outer):
        cases.append((int(ki), int(kj), int(kk), float(k_inner), float(k_outer)))
    # thin shells (0.25) at k ~ 1: every cell near the fundamental, the axes included (the
    # 2-, 4- and 8-leaf cases of the cell-ball split)
    for centre in (1.0, 1.25, 1.5, 2.0):
        for ki in range(0, 4):
            for kj in range(-3, 4):
                for kk in range(0, 4):
                    add(ki, kj, kk, centre - 0.125, centre + 0.125)
    # shells whose inner radius is 0
    for k_outer in (0.3, 0.5, 0.75, 1.0, 1.5, 2.5):
        for ki in range(0, 4):
            for kj in range(-3, 4):
                for kk in range(0, 4):
                    add(ki, kj, kk, 0.0, k_outer)
    # unit shells of medium radius: inside, outside, cut by one or both spheres
    for k_inner in (2.5, 4.0, 7.3):
        n = int(k_inner) + 3
        for _ in range(400):
            ki, kk = rng.integers(0, n, 2)
            kj = rng.integers(-n + 1, n)
            add(ki, kj, kk, k_inner, k_inner + 1.0)
    # thick shells (3) at k up to 31, cells near the two spheres and on the axes
    for k_outer in (8.0, 16.5, 24.0, 31.0):
        k_inner = k_outer - 3.0
        for _ in range(350):
            v = rng.normal(size=3)
            v *= rng.choice([k_inner, k_outer, 0.5*(k_inner + k_outer)])/np.linalg.norm(v)
            v += rng.uniform(-1, 1, 3)
            ki, kj, kk = np.rint(v).astype(int)
            add(abs(ki), kj, abs(kk), k_inner, k_outer)
        for k in range(int(k_inner) - 1, int(k_outer) + 2):
            add(k, 0, 0, k_inner, k_outer)
            add(0, -k, 0, k_inner, k_outer)
            add(0, 0, k, k_inner, k_outer)
            add(0, k, 3, k_inner, k_outer)
    return cases


def load():
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import REFERENCE, load_reference
    from make_golden_powerspec import _stub_modules
    ref = load_reference(PARAM, f'/tmp/concept_golden_work/bispec_{os.getpid()}')
    _stub_modules(f'{REFERENCE}/src')
    import analysis
    return ref, analysis


def child_overlap():
    import numpy as np
    ref, analysis = load()
    cases = overlap_cases(np.random.default_rng(20))
    arr = np.array(cases, dtype=np.float64)
    frac = np.array([analysis.get_bispec_overlap_cellshell(ki, kj, kk, a, b)
                     for ki, kj, kk, a, b in cases])
    # the reference alone against its own guards: how many cases a test may skip for lying
    # at an ϵ guard (tests/bispec_refs.py counts them the same way)
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import bispec_refs
    near = bispec_refs.near_guard(arr)
    print(f'{len(cases)} cases, {int(near.sum())} within the guard window '
          f'({100*near.mean():.3f} %, at most 0.5 % allowed)')
    assert near.mean() <= 0.005
    np.savez_compressed(os.path.join(HERE, 'bispec_overlap.npz'), cases=arr, frac=frac)
    print('wrote bispec_overlap', arr.shape, 'frac range', frac.min(), frac.max())


def child_value(N):
    import numpy as np
    ref, analysis = load()
    commons, mesh = ref.commons, ref.mesh
    ng = commons.nghosts
    rng = np.random.default_rng(100 + N)
    field = 1.0 + 0.5*rng.normal(size=(N, N, N))
    grid = np.zeros((N + 2*ng,)*3)
    grid[ng:-ng, ng:-ng, ng:-ng] = field*float(N)**(-3)
    slab = mesh.slab_decompose(grid, 'slab_golden', prepare_fft=True)
    mesh.fft(slab, 'forward')
    slab_data = np.array(slab).copy()
    bins = value_bins(N//2)
    out = dict(gridsize=N, field=field, slab=slab_data,
               bins=np.array(bins, dtype=np.float64))
    for aa in (True, False):
        analysis.bispec_antialiasing = aa
        tag = 'aa' if aa else 'noaa'
        analysis.bispec_grid_cache.clear()
        n_modes_power, n_modes, new = {}, [], []
        for shells in bins:
            value, shells_new = analysis.compute_bispec_value(N, shells, n_modes_power)
            n_modes.append(value)
            new.append(len(shells_new))
        analysis.bispec_grid_cache.clear()
        power, values = {}, []
        for shells in bins:
            values.append(analysis.compute_bispec_value(N, shells, power, slab_data))
        assert list(power) == list(n_modes_power)
        out[f'{tag}_indicator_value'] = np.array(n_modes)
        out[f'{tag}_indicator_new'] = np.array(new)
        out[f'{tag}_data_value'] = np.array(values)
        out[f'{tag}_power_shells'] = np.array(list(power), dtype=np.float64)
        out[f'{tag}_indicator_power'] = np.array(list(n_modes_power.values()))
        out[f'{tag}_data_power'] = np.array(list(power.values()))
    np.savez_compressed(os.path.join(HERE, f'bispec_value_g{N}.npz'), **out)
    print('wrote', f'bispec_value_g{N}', {k: getattr(v, 'shape', v) for k, v in out.items()})


def main():
    if len(sys.argv) > 1:
        if sys.argv[1] == 'overlap':
            child_overlap()
        else:
            child_value(int(sys.argv[1]))
        return
    for name in ('overlap', '8', '12'):
        print('===', name, flush=True)
        log = f'/tmp/concept_golden_bispec_{name}.log'
        with open(log, 'w') as f:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), name], stdout=f,
                               stderr=subprocess.STDOUT)
        print('\n'.join(open(log).read().splitlines()[-3:]))
        if r.returncode:
            sys.exit(f'case {name} failed, see {log}')


if __name__ == '__main__':
    main()
