"""2D renders on the GPU (concept_amd.render, csrc/cg_render.hip): against the reference's own
results (tests/golden/render2d_*.npz), the PNG, the device histogram against numpy, properties
of the projection, the projection past one tile against a direct weighted sum of the mesh, the
time loop's dumps and the utility, a 1024³ run, and x-slab domains.

Bars.  The 'data' projection: |Δ| <= 1e-12·max|golden| for every pixel (the project's bar for
mesh values).  The images: the exponent of the search equals the golden's; the pixel tolerance
is derived per image by feeding the golden 'data' projection, moved by up to ± the data
tolerance, through the numpy restatement of the enhancement (tests/golden/
make_golden_render2d.py) and taking 4× the largest pixel change (the factor covers pow
differing in the last bit between device and host).  The powered image against the host's
image**e: 2 ulps — the HIP math API documents FP64 pow with a maximum error of 1 ulp, plus one
ulp for the host's libm."""
import importlib.util
import io
import os
import socket
import subprocess
import sys
import time
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = ('render2d_a_defaults', 'render2d_b_cic_x', 'render2d_c_multigrid_y', 'render2d_d_fluid')
DATA_RTOL = 1e-12
POW_ULPS = 2


def restatement():
    spec = importlib.util.spec_from_file_location(
        'make_golden_render2d', os.path.join(HERE, 'golden', 'make_golden_render2d.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden(name):
    return np.load(os.path.join(HERE, 'golden', name + '.npz'))


def golden_components(g):
    from concept_amd import commons
    from concept_amd.species import Component
    commons.load_params(str(g['param']))
    comps = []
    for name in g['component_names']:
        name = str(name)
        if f'{name}_N' in g:
            c = Component(name, 'matter', N=int(g[f'{name}_N']), mass=float(g[f'{name}_mass']))
            c.populate(g[f'{name}_pos'], 'pos')
            c.populate(np.zeros((int(g[f'{name}_N']), 3)), 'mom')
        else:
            c = Component(name, 'matter', gridsize=int(g[f'{name}_gridsize']), boltzmann_order=1)
            c.populate(g[f'{name}_rho'], 'ϱ')
        comps.append(c)
    return comps


def image_tolerance(np_mod, data, enhance):
    """4× the largest pixel change of the restated image under the perturbed projections"""
    return 4*np_mod.stability(data, enhance)[1]


def check_against_golden(g, comps, tag=''):
    """compute, enhance and rescale every declaration; compare with the golden at both stages.
    Returns the final images (host arrays) per declaration."""
    from concept_amd import render
    np_mod = restatement()
    a = float(g['a'])
    decls = render.get_render2D_declarations(comps)
    assert len(decls) == int(g['n_declarations'])
    images = []
    for i in range(len(decls)):
        d = decls[i]
        assert [c.name for c in d.components] == [str(s) for s in g[f'd{i}_components']]
        assert d.gridsize == int(g[f'd{i}_gridsize'])
        T = d.terminal_resolution
        render.compute_render2D(d, a)
        stages = {'image': d.projections['image'], 'terminal': d.projections['terminalimage'][:T//2]}
        for key, golden_key in (('image', 'data'), ('terminal', 'terminal_data')):
            got, want = stages[key].cpu().numpy(), g[f'd{i}_{golden_key}']
            assert got.shape == want.shape
            err, bar = np.max(np.abs(got - want)), DATA_RTOL*np.max(np.abs(want))
            print(f'{tag}d{i} {golden_key}: max |Δ| = {err:.3e}, bar {bar:.3e} '
                  f'(max |golden| = {np.max(np.abs(want)):.6e})')
            assert err <= bar, (key, err, bar)
        info = {}
        render.enhance_render2D(d, info)
        render.rescale_render2D(d)
        for key, golden_key, data_key in (('image', 'image', 'data'),
                                          ('terminal', 'terminal_image', 'terminal_data')):
            got, want = stages[key].cpu().numpy(), g[f'd{i}_{golden_key}']
            enhance = bool(g[f'd{i}_enhance'])
            if enhance:
                sub = info['image' if key == 'image' else 'terminalimage']
                assert sub['exponent'] == float(g[f'd{i}_{key}_exponent']), (
                    key, sub['trace'], g[f'd{i}_{key}_trace'])
                assert sub['n_bins'] == int(g[f'd{i}_{key}_n_bins'])
            tol = image_tolerance(np_mod, g[f'd{i}_{data_key}'], enhance)
            err = np.max(np.abs(got - want))
            print(f'{tag}d{i} {golden_key}: max |Δ| = {err:.3e}, derived tolerance {tol:.3e}')
            assert err <= tol, (key, err, tol)
        images.append(d.projections['image'].cpu().numpy())
    return images


@pytest.mark.parametrize('name', GOLDEN)
def test_render2D_matches_the_reference(name):
    g = golden(name)
    comps = golden_components(g)
    check_against_golden(g, comps, tag=name + ' ')


def test_png_is_the_colormap_of_the_gpu_image(tmp_path):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.cm
    from PIL import Image
    from concept_amd import render
    g = golden('render2d_a_defaults')
    comps = golden_components(g)
    stream = io.StringIO()
    decls, files = render.render2D(comps, str(tmp_path/'render2D_a=0.5'), a=float(g['a']),
                                   t=1.0, stream=stream)
    assert sorted(os.path.basename(f) for f in files) == ['render2D_a=0.5.npz',
                                                          'render2D_a=0.5.png']
    assert sorted(os.listdir(tmp_path)) == ['render2D_a=0.5.npz', 'render2D_a=0.5.png']
    image = decls[0].projections['image'].cpu().numpy()
    assert image.min() == 0.0 and abs(image.max() - 1.0) <= 4e-16
    png = np.asarray(Image.open(tmp_path/'render2D_a=0.5.png'))
    want = getattr(matplotlib.cm, decls[0].colormap)(image, bytes=True)
    assert png.shape == want.shape and np.array_equal(png, want)
    # the data file holds the projection before the enhancement
    data = np.load(tmp_path/'render2D_a=0.5.npz')
    bar = DATA_RTOL*np.max(np.abs(g['d0_data']))
    assert np.max(np.abs(data['data'] - g['d0_data'])) <= bar
    assert str(data['axis']) == 'z' and float(data['a']) == float(g['a'])
    # the terminal image: the colormap sequences, then T/2 rows of T coloured spaces
    T = decls[0].terminal_resolution
    text = stream.getvalue()
    assert text.count(']4;') == 238
    body = text[text.rindex('\\') + 1:]
    assert body.count('\n') == T//2 and body.count('[48;5;') == T*T//2


# -- the device histogram against numpy --------------------------------------------------------
def ulp_distance(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


@pytest.mark.parametrize('n_bins', [25, 20000])
def test_histogram_matches_numpy(n_bins):
    import torch
    from concept_amd import commons, render
    from concept_amd.mesh import PotentialMesh
    commons.load_params({'boxsize': 100.0})
    mesh = PotentialMesh(16, 100.0)
    rng = np.random.default_rng(n_bins)
    image = rng.uniform(0.0, 1.0, 300*300)
    image[0], image[1] = 0.0, 1.0
    # values exactly on bin edges, and the maximum more than once
    edges = np.linspace(0.0, 1.0, n_bins + 1)
    image[2:2 + 200] = edges[rng.integers(0, n_bins + 1, 200)]
    image[300:310] = 1.0
    dev = torch.tensor(image, device='cuda')
    for exponent in (1.0, 0.01, 0.3, 7.0):
        counts, bin_edges = render._histogram(mesh, dev, exponent, n_bins)
        powered = mesh.render2D_apply(dev.clone(), exponent=exponent).cpu().numpy()
        want, want_edges = np.histogram(powered, n_bins)
        np.testing.assert_array_equal(bin_edges, want_edges)
        np.testing.assert_array_equal(counts, want)
        assert counts.sum() == image.size
        if exponent == 1.0:
            np.testing.assert_array_equal(powered, image)
            np.testing.assert_array_equal(counts, np.histogram(image, n_bins)[0])
        else:
            ulps = ulp_distance(powered, image**exponent).max()
            print(f'n_bins {n_bins}, exponent {exponent}: device pow within {ulps} ulp of the '
                  f'host (bound {POW_ULPS})')
            assert ulps <= POW_ULPS
        again, _ = render._histogram(mesh, dev, exponent, n_bins)
        np.testing.assert_array_equal(again, counts)
    vmin, vmax = render._minmax(mesh, dev)
    assert (vmin, vmax) == (image.min(), image.max())
    # clamp and rescale; the homogeneous image
    out = mesh.render2D_apply(dev.clone(), exponent=0.3, vmin=0.2, vmax=0.8, shift=0.2,
                              scale=1/(0.8 - 0.2)).cpu().numpy()
    want = (np.minimum(np.maximum(powered_at(mesh, dev, 0.3), 0.2), 0.8) - 0.2)*(1/(0.8 - 0.2))
    np.testing.assert_array_equal(out, want)
    flat = torch.full((1000,), 3.25, device='cuda', dtype=torch.float64)
    assert torch.all(render.rescale_image(mesh, flat) == 0.5)
    mesh.close()


def powered_at(mesh, dev, exponent):
    return mesh.render2D_apply(dev.clone(), exponent=exponent).cpu().numpy()


# -- properties of the projection -------------------------------------------------------------
def _one_component(n_lin, L, seed, clustered=True):
    from concept_amd import commons
    from concept_amd.species import Component
    p = commons.params
    n = n_lin**3
    rng = np.random.default_rng(seed)
    q = (np.arange(n_lin) + 0.5)*L/n_lin
    pos = np.stack(np.meshgrid(q, q, q, indexing='ij'), -1).reshape(-1, 3)
    if clustered:
        centres = rng.uniform(0, L, (3, 3))
        pos = pos + 0.3*(centres[rng.integers(0, 3, n)] - pos)
    pos = np.mod(pos + rng.normal(0, 0.03*L, pos.shape), L)
    c = Component('matter', 'matter', N=n, mass=p.ρ_mbar*L**3/n)
    c.populate(pos, 'pos')
    c.populate(np.zeros_like(pos), 'mom')
    return c, pos


def _project(comps, axis, extent, gridsize, L, a=1.0, **options):
    from concept_amd import commons, render
    commons.load_params({'boxsize': L, 'render2D_select': {'all': {'data': True}},
                         'render2D_options': dict(
                             {'gridsize': gridsize, 'axis': axis, 'extent': extent}, **options)})
    d = render.get_render2D_declarations(comps)[0]
    render.compute_render2D(d, a)
    return d.projections['data'].cpu().numpy().copy()


def test_projection_properties():
    import torch
    from concept_amd import commons, render
    from concept_amd.species import Component
    L, N, a = 120.0, 48, 0.7
    commons.load_params({'boxsize': L})
    c, pos = _one_component(16, L, 12)
    total = c.N*c.mass   # matter: w = 0, so a**(-3w) = 1
    full = {}
    for axis in 'xyz':
        full[axis] = _project([c], axis, (0, L), N, L, a)
        assert abs(full[axis].sum()/total - 1) <= 1e-12, (axis, full[axis].sum()/total - 1)
    # two adjacent extents add up to the extent of their union
    for axis in 'xyz':
        lower = _project([c], axis, (0.1*L, 0.37*L), N, L, a)
        upper = _project([c], axis, (0.37*L, 0.62*L), N, L, a)
        union = _project([c], axis, (0.1*L, 0.62*L), N, L, a)
        assert np.max(np.abs(lower + upper - union)) <= 1e-12*np.max(np.abs(union)), axis
    # the three axes agree on a box rotated accordingly: the image along z of (x, y, z) is the
    # image along x of (z, x, y) and the image along y of (x, z, y)
    extent = (0.21*L, 0.55*L)
    along_z = _project([c], 'z', extent, N, L, a)
    for axis, order in (('x', [2, 0, 1]), ('y', [0, 2, 1])):
        rotated = Component('matter', 'matter', N=c.N, mass=c.mass)
        rotated.populate(np.ascontiguousarray(pos[:, order]), 'pos')
        rotated.populate(np.zeros_like(pos), 'mom')
        image = _project([rotated], axis, extent, N, L, a)
        assert np.max(np.abs(image - along_z)) <= 1e-12*np.max(np.abs(along_z)), axis
    # two calls give bit-identical images: the projection of one mesh and its enhancement
    mesh = render._mesh(N, 'render2D')
    for axis in 'xyz':
        planes = render.projection_planes(N, L, extent)
        one = mesh.render2D_project(axis, *planes, 1.0)
        two = mesh.render2D_project(axis, *planes, 1.0)
        assert torch.equal(one, two), axis
        e1, e2 = render.enhance_image(mesh, one), render.enhance_image(mesh, two)
        assert torch.equal(e1, e2) and float(e1.min()) < float(e1.max())


# -- the projection against a direct weighted sum, past one tile --------------------------------
# k_project_along_z gives a wave 64 rows j at a time and walks the planes with k += 64;
# k_project_across works in tiles of 64 k by 16 d0.  N = 72 has two j-blocks and two k-blocks (the
# second with 8 live entries) and a partial d0 tile (72 % 16 = 8); N = 136 has three blocks and
# up to 136 planes, a third trip.  The mesh holds seeded values of both signs (NaN in the padding,
# which no projection may read); the reference is the kernel's contract restated on the host,
#     P[d0, d1] = factor · Σ_s w_s · M[…],   image = flipud(P.T),
# summed in np.longdouble, with w = frac_bgn on plane_bgn, frac_end on plane_end - 1 and 1
# between them (a one-plane range: frac_bgn), and (d0, d1, s) = (y, z, x), (x, z, y), (x, y, z).
#
# Bar per pixel: n·2⁻⁵³·factor·Σ_s |w_s·M|, n the number of planes.  Every term takes at most
# one rounding in w_s·M and at most n - 1 in the additions, whatever their order (the sum over
# the domains' images included), and the factor is a power of two here, so multiplying by it
# rounds nothing: n roundings in all, each 2⁻⁵³ relative to a partial sum that Σ |w_s·M| bounds.
SYNTHETIC_FACTOR = 0.125
SYNTHETIC_RANGES = {
    72: ((0, 72, 1.0, 1.0),
         (5, 69, 0.25, 0.6),     # exactly 64 planes
         (7, 72, 0.25, 0.6),     # 65 planes
         (3, 70, 0.9, 0.1),
         (40, 41, 0.37, 0.0),
         (40, 42, 0.8, 0.0),     # an extent of at most one cell (projection_planes)
         (71, 72, 1.0, 1.0)),
    136: ((0, 136, 1.0, 1.0),
          (1, 131, 0.5, 0.5)),   # 130 planes: 2 live lanes in the third trip
}
# on x-slab domains of 18 layers: the clipping of cg_render2d_project for axis x
DOMAIN_RANGES = {
    'x': ((17, 19, 0.75, 0.0),   # the two planes of an extent <= 1 cell on different ranks
          (18, 37, 0.3, 0.6),    # from a rank's first layer to a lone plane two ranks on
          (35, 36, 0.5, 0.0),    # one plane: three ranks have none
          (10, 60, 0.2, 0.7)),
    'y': ((3, 70, 0.9, 0.1),),
    'z': ((3, 70, 0.9, 0.1),),
}
_synthetic_fields = {}
_synthetic_meshes = {}


def _synthetic_field(N):
    """the seeded global array [x][y][z], made once per N and left unchanged"""
    if N not in _synthetic_fields:
        _synthetic_fields[N] = np.random.default_rng(1000 + N).normal(0, 1, (N, N, N))
    return _synthetic_fields[N]


def _synthetic_mesh(N):
    """a mesh of size N (one x-slab domain under comm.init()) holding this domain's layers of
    _synthetic_field(N); the test's own, so that free_meshes() of another test leaves it alone"""
    import torch
    from concept_amd import comm
    from concept_amd.mesh import PotentialMesh
    mesh = _synthetic_meshes.get(N)
    if mesh is None:
        mesh = PotentialMesh(N, 100.0, comm=comm.active())
        per, pad, nxl = mesh.layer_doubles, mesh.pad, mesh.nxl
        buf = np.full((nxl, per), np.nan)
        buf[:, :N*pad].reshape(nxl, N, pad)[:, :, :N] = _synthetic_field(N)[mesh.x0:mesh.x0 + nxl]
        mesh.layers_write(0, nxl, torch.tensor(buf.reshape(-1), device='cuda'))
        _synthetic_meshes[N] = mesh
    return mesh


def direct_projection(field, axis, planes, factor):
    """(image, bar) of the contract above: the longdouble weighted sum and the per-pixel bar"""
    bgn, end, frac_bgn, frac_end = planes
    w = np.ones(end - bgn, dtype=np.longdouble)
    w[-1] = frac_end
    w[0] = frac_bgn   # a one-plane range counts with frac_bgn
    terms = np.moveaxis(field, 'xyz'.index(axis), -1)[..., bgn:end].astype(np.longdouble)*w
    P = factor*terms.sum(-1)
    bar = (end - bgn)*2.0**-53*factor*np.abs(terms).sum(-1)
    return np.flipud(P.T), np.flipud(bar.T)


def check_synthetic_projection(N, axis, planes, comm=None, tag=''):
    """render2D_project of the synthetic mesh (summed over the domains of `comm` the way
    project_render2D sums them) against direct_projection.  Returns the device image."""
    mesh = _synthetic_mesh(N)
    image = mesh.render2D_project(axis, *planes, SYNTHETIC_FACTOR)
    if comm is not None and comm.world > 1:
        image.copy_(comm.sum_in_rank_order(image))
    want, bar = direct_projection(_synthetic_field(N), axis, planes, SYNTHETIC_FACTOR)
    got = image.cpu().numpy()
    assert got.shape == want.shape == (N, N)
    assert np.all(np.isfinite(got)), f'{tag}axis {axis} {planes}: the image is not finite'
    assert np.all(bar > 0)
    ratio = np.abs(got.astype(np.longdouble) - want)/bar
    print(f'{tag}N = {N}, axis {axis}, planes {planes}: worst |Δ| = '
          f'{float(np.max(np.abs(got - want))):.3e}, worst ratio to the bar = '
          f'{float(ratio.max()):.3f}')
    assert ratio.max() <= 1, (axis, planes, float(ratio.max()))
    return image


@pytest.mark.parametrize('N, planes', [(N, planes) for N in SYNTHETIC_RANGES
                                       for planes in SYNTHETIC_RANGES[N]])
def test_projection_matches_a_direct_sum(N, planes):
    import torch
    for axis in 'xyz':
        image = check_synthetic_projection(N, axis, planes)
        again = _synthetic_mesh(N).render2D_project(axis, *planes, SYNTHETIC_FACTOR)
        assert torch.equal(image, again), axis


@pytest.mark.parametrize('n_bins', [25, 20000])
def test_enhancement_of_a_projected_image(n_bins):
    """the device minimum, maximum and histogram of a real projected image (N = 136, both signs)
    against numpy's of the same image, exactly"""
    from concept_amd import render
    N = 136
    mesh = _synthetic_mesh(N)
    image = mesh.render2D_project('z', *SYNTHETIC_RANGES[N][1], SYNTHETIC_FACTOR)
    host = image.cpu().numpy()
    assert host.min() < 0 < host.max()
    assert render._minmax(mesh, image) == (np.min(host), np.max(host))
    counts, bin_edges = render._histogram(mesh, image, 1.0, n_bins)
    want, want_edges = np.histogram(host, n_bins)
    np.testing.assert_array_equal(bin_edges, want_edges)
    np.testing.assert_array_equal(counts, want)
    print(f'N = {N}, {n_bins} bins: {int(np.count_nonzero(want))} bins filled, the fullest '
          f'holds {int(want.max())} of {host.size} pixels; counts, edges, min and max equal '
          f"numpy's")
    assert counts.sum() == host.size


def check_synthetic_on_domains(N, comm):
    """One rank's part of the synthetic projections on x-slab domains: every rank writes its own
    layers of the same global array and projects them; the summed images meet the bar of one
    domain against the same host sum and are the same on all ranks bit for bit."""
    import torch
    assert N == 72 and comm.world == 4
    for axis, ranges in DOMAIN_RANGES.items():
        for planes in ranges:
            image = check_synthetic_projection(N, axis, planes, comm, tag=f'rank {comm.rank} ')
            rows = comm.all_gather_rows(image.reshape(1, -1))
            assert all(torch.equal(rows[r], rows[0]) for r in range(comm.world)), \
                'the ranks hold different images'


# -- the time loop's dumps and the utility ------------------------------------------------------
def test_timeloop_dumps_render2D_files(tmp_path):
    import torch
    from concept_amd import commons, snapshot
    from concept_amd import render2D as utility
    from concept_amd.stepper import Timeloop
    from concept_amd.species import Component
    out = tmp_path/'out'
    param = tmp_path/'param'
    param.write_text(f"""
boxsize = 64*Mpc
potential_options = {{'gridsize': {{'gravity': {{'pm': 32}}}}}}
select_forces = {{'matter': {{'gravity': 'pm'}}}}
a_begin = 0.1
output_dirs = {{'snapshot': '{out}', 'render2D': '{out}'}}
output_times = {{'snapshot': [0.12, 0.14], 'render2D': [0.11, 0.12, 0.14]}}
snapshot_type = 'gadget'
gadget_snapshot_params = {{'dataformat': {{'POS': 64, 'VEL': 64}}}}
render2D_options = {{'gridsize': 32, 'terminal resolution': 16, 'extent': 0.4*boxsize}}
render2D_select = {{'matter': True}}
""")
    p = commons.load_params(str(param))
    n = 16**3
    rng = np.random.default_rng(3)
    c = Component('matter', 'matter', N=n, mass=p.ρ_mbar*p.boxsize**3/n)
    q = (np.arange(16) + 0.5)*p.boxsize/16
    pos = np.stack(np.meshgrid(q, q, q, indexing='ij'), -1).reshape(-1, 3)
    c.populate(np.mod(pos + rng.normal(0, 1.0, pos.shape), p.boxsize), 'pos')
    c.populate(rng.normal(0, 1e-3, pos.shape)*c.mass, 'mom')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loop = Timeloop([c])
        loop.run()
    torch.cuda.synchronize()
    names = sorted(os.listdir(out))
    assert names == ['render2D_a=0.11.npz', 'render2D_a=0.11.png', 'render2D_a=0.12.npz',
                     'render2D_a=0.12.png', 'render2D_a=0.14.npz', 'render2D_a=0.14.png',
                     'snapshot_a=0.12', 'snapshot_a=0.14'], names
    assert sorted(os.path.basename(f) for f in loop.renders2D_written) == names[:6]
    for a in ('0.12', '0.14'):
        snap_fn = str(out/f'snapshot_a={a}')
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            files = utility.main([snap_fn, '--params', str(param), '--output-dir', str(tmp_path)])
        assert sorted(os.path.basename(f) for f in files) == [
            f'render2D_snapshot_a={a}.npz', f'render2D_snapshot_a={a}.png']
        dumped = np.load(out/f'render2D_a={a}.npz')
        again = np.load(tmp_path/f'render2D_snapshot_a={a}.npz')
        assert dumped['data'].shape == (32, 32)
        np.testing.assert_allclose(again['data'], dumped['data'], rtol=0,
                                   atol=1e-10*np.max(np.abs(dumped['data'])))
        assert float(dumped['a']) == pytest.approx(float(a), rel=1e-12)
        assert tuple(dumped['extent']) == (0.0, 0.4*p.boxsize)
        commons.load_params(str(param))


def test_dumps_without_render2D_are_unchanged(tmp_path):
    """with no 'render2D' in output_times and output_dirs the time loop writes the snapshots and
    power spectra it wrote before, under the same names, and no render"""
    import torch
    from concept_amd import commons
    from concept_amd.stepper import Timeloop
    from concept_amd.species import Component
    out = tmp_path/'out'
    p = commons.load_params(f"""
boxsize = 64*Mpc
potential_options = {{'gridsize': {{'gravity': {{'pm': 32}}}}}}
select_forces = {{'matter': {{'gravity': 'pm'}}}}
a_begin = 0.1
output_dirs = {{'snapshot': '{out}', 'powerspec': '{out}'}}
output_times = {{'snapshot': [0.12], 'powerspec': [0.11, 0.12]}}
snapshot_type = 'gadget'
powerspec_options = {{'gridsize': 32}}
powerspec_select = {{'matter': True}}
""")
    assert p.render2D_dir is None and p.render2D_times == {'a': (), 't': ()}
    n = 16**3
    rng = np.random.default_rng(3)
    c = Component('matter', 'matter', N=n, mass=p.ρ_mbar*p.boxsize**3/n)
    c.populate(rng.uniform(0, p.boxsize, (n, 3)), 'pos')
    c.populate(np.zeros((n, 3)), 'mom')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        loop = Timeloop([c])
        loop.run()
    torch.cuda.synchronize()
    assert sorted(os.listdir(out)) == ['powerspec_a=0.11', 'powerspec_a=0.12', 'snapshot_a=0.12']
    assert not hasattr(loop, 'renders2D_written')
    assert [os.path.basename(f) for f in loop.powerspecs_written] == ['powerspec_a=0.11',
                                                                      'powerspec_a=0.12']


# -- at size -------------------------------------------------------------------------------------
def test_render2D_at_1024():
    import torch
    from concept_amd import commons, render
    from concept_amd.species import Component
    from concept_amd.mesh import free_meshes
    np_mod = restatement()
    n_lin, N, L = 512, 1024, 1000.0
    n = n_lin**3
    p = commons.load_params({'boxsize': L, 'render2D_options': {'gridsize': N},
                             'render2D_select': {'matter': {'data': True, 'image': True}}})
    c = Component('matter', 'matter', N=n, mass=p.ρ_mbar*L**3/n)
    g = torch.Generator(device='cuda').manual_seed(11)
    q = (torch.arange(n_lin, device='cuda', dtype=torch.float64) + 0.5)*(L/n_lin)
    pos = torch.stack(torch.meshgrid(q, q, q, indexing='ij'), -1).reshape(-1, 3)
    pos += torch.randn(pos.shape, generator=g, device='cuda', dtype=torch.float64)*(0.3*L/n_lin)
    pos.remainder_(L)
    c.pos.copy_(pos)
    c.mom.zero_()
    del pos
    timings = {}
    d = render.get_render2D_declarations([c])[0]
    render.compute_render2D(d, 1.0, timings)   # warm-up (plans, tables)
    render.compute_render2D(d, 1.0, timings)
    print(f'\n1024^3 render of {n} particles (PCS): upstream (deposit + FFT) '
          f'{timings["upstream"]*1e3:.1f} ms, inverse FFT + projection '
          f'{timings["projection"]*1e3:.1f} ms')
    mesh = render._mesh(N, 'render2D')
    image = d.projections['image']
    total = c.N*c.mass
    reps = 5
    for extent in ((0.0, 0.1*L), (0.0, L)):
        planes = render.projection_planes(N, L, extent)
        for axis in 'xyz':
            mesh.render2D_project(axis, *planes, (L/N)**3, out=image)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            for _ in range(reps):
                mesh.render2D_project(axis, *planes, (L/N)**3, out=image)
            e[1].record()
            e[1].synchronize()
            t = e[0].elapsed_time(e[1])*1e-3/reps
            nbytes = 8*N*N*(planes[1] - planes[0])
            print(f'projection along {axis}, {planes[1] - planes[0]} planes: {t*1e3:.3f} ms, '
                  f'{nbytes/1e9:.2f} GB read, {nbytes/t/1e12:.2f} TB/s = '
                  f'{nbytes/t/8e12:.2f} of 8 TB/s')
            assert bool(torch.isfinite(image).all())
            if extent[1] == L:
                assert abs(float(image.sum())/total - 1) <= 1e-12, axis
    # the enhancement of the 1024² image beside the numpy restatement on the host
    planes = render.projection_planes(N, L, (0.0, 0.1*L))
    mesh.render2D_project('z', *planes, (L/N)**3, out=image)
    host = image.cpu().numpy()
    info = {}
    work = image.clone()
    render.enhance_image(mesh, work, info)   # warm-up
    work.copy_(image)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    render.enhance_image(mesh, work, info)
    render.rescale_image(mesh, work)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    info_np = {}
    want = np_mod.render_np(host, True, info_np)
    t_host = time.perf_counter() - t0
    got = work.cpu().numpy()
    print(f'enhancement of the 1024^2 image ({info["n_bins"]} bins, {len(info["trace"])} '
          f'iterations, exponent {info["exponent"]}): {t_dev*1e3:.1f} ms on the device, '
          f'{t_host*1e3:.0f} ms numpy on the host (exponent {info_np["exponent"]}); '
          f'max |Δ| = {np.max(np.abs(got - want)):.3e}')
    assert np.all(np.isfinite(got)) and got.min() == 0.0 and abs(got.max() - 1.0) <= 4e-16
    del c, mesh, image, work, d
    free_meshes()
    torch.cuda.empty_cache()


# -- x-slab domains ------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [2, 4])
def test_render2D_on_domains(world):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    # four domains of 18 layers also project the synthetic mesh of size 72 (DOMAIN_RANGES)
    cases = list(GOLDEN[:3]) + (['synthetic:72'] if world == 4 else [])
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, 'render2d_worker.py')] + cases,
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0 and f'RANK{r}-OK' in outs[r], f'rank {r}:\n{outs[r][-4000:]}'
    print(outs[0][-3000:])
