"""Golden vectors of the reference's 2D render (graphics.py:1027-1955).

Run in the development container, one process per case (the reference keeps its parameters as
module globals):  python tests/golden/make_golden_render2d.py
The reference is imported in pure-Python mode through oracle/refharness/ref_import; its
graphics module is imported as it is (ic and linear, which need CLASS, are stubbed) and
save_render2D_data is not called.  Per case and declaration: the inputs, the 'data' projection
straight after compute_render2D (for the last declaration of the small cases also the grid it
was projected from), the image after enhance_render2D and rescale_render2D, the
terminal projection (upper half of the rows) at the same two stages, and terminal_resolution.

This file also carries a plain numpy restatement of enhance_render2D and rescale_render2D
(enhance_np, rescale_np).  For every image the generator asserts that
  - the restatement reproduces the reference's image bit for bit, and
  - the search ends on the same exponent, with the same colour limits to 1e-9, when the input
    projection is perturbed by up to ±1e-12·max|projection| (perturbations()),
and records the restatement's exponent and colour limits.  A case that fails the second check
gets another seed: that condition is what lets the GPU test demand the exact exponent.
The tests import the restatement from here (numpy only at import time)."""
import math
import os
import subprocess
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

CASES = {
    # (a) the defaults (PCS, axis z, extent (0, 0.1 boxsize)) on a clustered 16³ box, grid 32
    'render2d_a_defaults': dict(
        boxsize=100.0, components=[('matter', 16**3, None)], seed=1,
        options="""render2D_options = {'gridsize': 32}
""", clustered=True),
    # (b) axis x, both ends of the extent inside cells, CIC, deconvolved, interlaced, grid 64;
    # the terminal image at half the grid size, so that the slab is resized down for it
    'render2d_b_cic_x': dict(
        boxsize=80.0, components=[('matter', 16**3, None)], seed=2,
        options="""render2D_options = {'gridsize': 64, 'interpolation': 'CIC', 'deconvolve': True,
                    'interlace': True, 'axis': 'x', 'extent': (0.13*boxsize, 0.58*boxsize),
                    'terminal resolution': 32}
""", clustered=True),
    # (c) axis y, an extent inside one cell, two particle components, upstream 16 and 24 on a
    # global 24: per component and combined
    'render2d_c_multigrid_y': dict(
        boxsize=90.0, components=[('light', 8**3, None), ('heavy', 12**3, None)], seed=3,
        options="""render2D_options = {'upstream gridsize': {'light': 16, 'heavy': 24},
                    'global gridsize': 24, 'axis': 'y',
                    'extent': (0.43*boxsize, 0.45*boxsize)}
render2D_select = {'all': True, 'all combinations': True}
""", clustered=True),
    # (d) a fluid and particles, combined, the whole box, not enhanced
    'render2d_d_fluid': dict(
        boxsize=70.0, components=[('matter', 8**3, None), ('fluid', None, 16)], seed=4,
        options="""render2D_options = {'gridsize': 16, 'extent': (0, boxsize), 'enhance': False}
render2D_select = {'all combinations': True}
""", clustered=False),
}

DATA_RTOL = 1e-12   # the bar for the 'data' projection: |Δ| <= DATA_RTOL*max|golden|


# -- the numpy restatement of graphics.py:1568-1755 ----------------------------------------------
def rescale_np(image):
    """rescale_render2D (graphics.py:1745-1755) of one image; returns a new array"""
    image = np.array(image, dtype=np.float64)
    vmin, vmax = np.min(image), np.max(image)
    if vmin != 0 and vmax != 0 and abs(vmin - vmax) <= 1e-9*max(abs(vmin), abs(vmax)):
        image[...] = 0.5
    else:
        with np.errstate(divide='ignore', invalid='ignore'):
            image = (image - vmin)*(1/(vmax - vmin))
    return image


def enhance_np(image, info=None):
    """enhance_render2D (graphics.py:1607-1717) of one image; returns a new array.  info: a
    dict that receives exponent, n_bins, vmin, vmax and the (exponent, index_center) trace."""
    image = rescale_np(image)
    vmin, vmax = np.min(image), np.max(image)
    if vmin == vmax:
        return image
    size = image.size
    n_bins = max(int(1e-2*size), 25)
    exponent_lower, exponent_upper, exponent = 1e-2, 1e+2, 1
    index_min, index_max = -4, -2
    trace = []
    while True:
        bins, bin_edges = np.histogram(image**exponent, n_bins)
        Σbins = size - bins[0]
        occupation = 0
        for index in range(1, n_bins):
            occupation += bins[index]
            if occupation >= Σbins//2:
                index_center = index
                break
        else:
            exponent = 1
            break
        trace.append((float(exponent), index_center))
        if index_center < int(n_bins*0.28):
            exponent_upper = exponent
            index_min = index_center
        elif index_center > int(n_bins*0.28):
            exponent_lower = exponent
            index_max = index_center
        else:
            break
        if index_max >= index_min and index_max - index_min <= 1:
            break
        if exponent/1e-2 < 1 + 1e-3:
            exponent = 1e-2
            break
        elif 1e+2/exponent < 1 + 1e-3:
            exponent = 1e+2
            break
        exponent = math.sqrt(exponent_lower*exponent_upper)
    # the reference raises pixel by pixel (graphics.py:1684-1685): scalar powers
    flat = image.reshape(-1)
    for index in range(size):
        flat[index] **= exponent
    bins, bin_edges = np.histogram(image, n_bins)
    Σbins = size - bins[0]
    # colour limits (graphics.py:1700-1711), bins[0] left out: the left edge of the bin below
    # the first one where the counts summed upwards reach int(0.005·Σbins), and the right edge
    # of the first bin where the counts summed downwards reach int(0.0001·Σbins)
    reached = np.nonzero(np.cumsum(bins[1:]) >= int(0.005*Σbins))[0]
    if reached.size:
        vmin = bin_edges[reached[0]]
    reached = np.nonzero(np.cumsum(bins[:0:-1]) >= int(0.0001*Σbins))[0]
    if reached.size:
        vmax = bin_edges[n_bins - reached[0]]
    image = np.minimum(np.maximum(image, vmin), vmax)
    if info is not None:
        info.update(exponent=float(exponent), n_bins=n_bins, vmin=float(vmin), vmax=float(vmax),
                    trace=trace)
    return image


def render_np(projection, enhance=True, info=None):
    """enhance (if asked for) and rescale, as render2D() does (graphics.py:1049-1051)"""
    image = enhance_np(projection, info) if enhance else np.array(projection, dtype=np.float64)
    return rescale_np(image)


def perturbations(projection, rtol=DATA_RTOL):
    """The projection moved by up to ±rtol·max|projection|: all pixels up, all down, and two
    fixed patterns of per-pixel signs"""
    projection = np.asarray(projection, dtype=np.float64)
    δ = rtol*np.max(np.abs(projection))
    rng = np.random.default_rng(20261016)
    out = [projection + δ, projection - δ]
    for _ in range(2):
        out.append(projection + δ*rng.choice([-1.0, 1.0], size=projection.shape))
    return out


def stability(projection, enhance=True):
    """(exponent stays the same, largest pixel change) of render_np under perturbations()"""
    info = {}
    image = render_np(projection, enhance, info)
    same, worst = True, 0.0
    for perturbed in perturbations(projection):
        info_p = {}
        image_p = render_np(perturbed, enhance, info_p)
        same = same and info_p.get('exponent') == info.get('exponent')
        worst = max(worst, float(np.max(np.abs(image_p - image))))
    return same, worst


# -- the generator -----------------------------------------------------------------------------
def param_text(cfg):
    return f"""
boxsize = {cfg['boxsize']!r}*Mpc
H0 = 70*km/s/Mpc
Ωcdm = 0.25
Ωb = 0.05
a_begin = 0.5
enable_class_background = False
{cfg['options']}
"""


def _stub_modules():
    """ic / linear stand-ins (they need CLASS) for `import graphics`"""
    import types

    def nothing(*a, **k):
        return None
    ic = types.ModuleType('ic')
    ic.realize = nothing
    linear = types.ModuleType('linear')
    for fname in ('compute_cosmo', 'get_linear_powerspec', 'get_treelevel_bispec',
                  'get_linear_component'):
        setattr(linear, fname, nothing)
    for mod in (ic, linear):
        mod.__file__ = os.path.abspath(__file__)
    sys.modules.update(ic=ic, linear=linear)


def child(name, seed):
    sys.path.insert(0, os.path.join(REPO, 'oracle', 'refharness'))
    from ref_import import load_reference
    cfg = CASES[name]
    ref = load_reference(param_text(cfg), f'/tmp/concept_golden_work/{name}')
    commons, species = ref.commons, ref.species
    _stub_modules()
    import matplotlib
    matplotlib.use('Agg')
    import graphics
    L = commons.boxsize
    rng = np.random.default_rng(seed)
    out = dict(boxsize=L, a=commons.universals.a, param=param_text(cfg), seed=seed)
    comps = []
    for ci, (cname, N, gs) in enumerate(cfg['components']):
        if N is not None:
            n = round(N**(1/3))
            q = (np.arange(n) + 0.5)*L/n
            pos = np.stack(np.meshgrid(q, q, q, indexing='ij'), -1).reshape(-1, 3)
            if cfg['clustered']:
                centres = rng.uniform(0, L, (4, 3))
                pull = rng.integers(0, 4, len(pos))
                pos = pos + 0.35*(centres[pull] - pos) + rng.normal(0, 0.02*L, pos.shape)
            else:
                pos = pos + rng.normal(0, 0.05*L/n, pos.shape)
            pos = np.mod(pos, L)
            mass = commons.ρ_mbar*L**3/N*(1.0 + 0.3*ci)
            comp = species.Component(cname, 'matter', N=N, mass=mass)
            for d, s_ in enumerate('xyz'):
                comp.populate(np.ascontiguousarray(pos[:, d]), 'pos' + s_)
                comp.populate(np.zeros(N), 'mom' + s_)
            out[f'{cname}_pos'] = pos
            out[f'{cname}_mass'] = mass
            out[f'{cname}_N'] = N
        else:
            comp = species.Component(cname, 'matter', gridsize=gs, boltzmann_order=1)
            rho = commons.ρ_mbar*0.4*(1 + 0.3*rng.normal(size=(gs, gs, gs)))
            comp.populate(np.ascontiguousarray(rho), 'ϱ')
            out[f'{cname}_rho'] = rho
            out[f'{cname}_gridsize'] = gs
        out[f'{cname}_upstream'] = comp.render2D_upstream_gridsize
        comps.append(comp)
    out['component_names'] = np.array([c[0] for c in cfg['components']])
    declarations = graphics.get_render2D_declarations(comps)
    out['n_declarations'] = len(declarations)
    # the real-space grids project_render2D is given (the global one first, then the terminal's)
    grids = []
    project_render2D = graphics.project_render2D

    def capture(grid, projection, axis, extent):
        ng = commons.nghosts
        grids.append(np.array(grid)[ng:-ng, ng:-ng, ng:-ng])
        return project_render2D(grid, projection, axis, extent)
    graphics.project_render2D = capture
    for i in range(len(declarations)):
        # (the projections of all declarations share memory: fetch them again each time)
        d = graphics.get_render2D_declarations(comps)[i]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            graphics.compute_render2D(d)
        T = d.terminal_resolution
        if d.gridsize <= 24 and i == len(declarations) - 1:
            # a grid small enough to keep: the plane arithmetic is checked against it
            out[f'd{i}_grid'] = grids[-2]
        data = np.array(d.projections['image'])
        term = np.array(d.projections['terminalimage'])[:T//2]
        graphics.enhance_render2D(d)
        graphics.rescale_render2D(d)
        image = np.array(d.projections['image'])
        term_image = np.array(d.projections['terminalimage'])[:T//2]
        out[f'd{i}_components'] = np.array([c.name for c in d.components])
        out[f'd{i}_gridsize'] = d.gridsize
        out[f'd{i}_terminal_resolution'] = T
        out[f'd{i}_axis'] = d.axis
        out[f'd{i}_extent'] = np.array(d.extent, dtype=np.float64)
        out[f'd{i}_interpolation'] = d.interpolation
        out[f'd{i}_deconvolve'] = bool(d.deconvolve)
        out[f'd{i}_interlace'] = str(d.interlace)
        out[f'd{i}_enhance'] = bool(d.enhance)
        out[f'd{i}_colormap'] = d.colormap
        out[f'd{i}_data'] = data
        out[f'd{i}_image'] = image
        out[f'd{i}_terminal_data'] = term
        out[f'd{i}_terminal_image'] = term_image
        for tag, before, after in (('image', data, image), ('terminal', term, term_image)):
            info = {}
            again = render_np(before, d.enhance, info)
            if not np.array_equal(again.view(np.int64), after.view(np.int64)):
                sys.exit(f'{name} d{i} {tag}: the restatement differs from the reference by '
                         f'{np.max(np.abs(again - after)):.3e}')
            same, worst = stability(before, d.enhance)
            print(f'{name} d{i} {tag}: exponent {info.get("exponent")}, limits '
                  f'{info.get("vmin")} {info.get("vmax")}, {len(info.get("trace", []))} '
                  f'iterations; perturbed: same exponent {same}, pixels move {worst:.3e}')
            if not same or worst > 1e-9:
                sys.exit(3)   # unstable under the perturbation: another seed
            out[f'd{i}_{tag}_exponent'] = info.get('exponent', float('nan'))
            out[f'd{i}_{tag}_n_bins'] = info.get('n_bins', 0)
            out[f'd{i}_{tag}_vmin'] = info.get('vmin', float('nan'))
            out[f'd{i}_{tag}_vmax'] = info.get('vmax', float('nan'))
            out[f'd{i}_{tag}_trace'] = np.array(info.get('trace', []), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print('wrote', name, {k: getattr(v, 'shape', v) for k, v in out.items() if k != 'param'})


def main():
    if len(sys.argv) > 2 and sys.argv[1] in CASES:
        child(sys.argv[1], int(sys.argv[2]))
        return
    for name, cfg in CASES.items():
        print('===', name, flush=True)
        log = f'/tmp/concept_golden_{name}.log'
        for attempt in range(8):
            seed = cfg['seed'] + 100*attempt
            with open(log, 'w') as f:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(seed)],
                                   stdout=f, stderr=subprocess.STDOUT)
            print('\n'.join(open(log).read().splitlines()[-8:]))
            if r.returncode != 3:
                break
            print(f'seed {seed} is not stable under the perturbation: the next one', flush=True)
        if r.returncode:
            sys.exit(f'case {name} failed, see {log}')


if __name__ == '__main__':
    main()
