"""Power spectra on the GPU (concept_amd.analysis, cg_powerspec_bin): against the reference's
own results (tests/golden/powerspec_*.npz), the reference's test/powerspec checks replayed,
determinism of the binning, the binning beyond the first chunk of 64 kk against longdouble host
sums and against plane waves of known power, the time loop's dumps and the utility, a 1024³ run,
and x-slab domains against one domain."""
import math
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
GOLDEN = ('powerspec_a_defaults', 'powerspec_b_cic', 'powerspec_c_multigrid', 'powerspec_d_fluid')


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


def check_against_golden(g, decls, rtol=1e-12):
    from concept_amd import analysis
    assert len(decls) == int(g['n_declarations'])
    for i, d in enumerate(decls):
        np.testing.assert_array_equal(d.n_modes, g[f'd{i}_n_modes'])
        np.testing.assert_allclose(d.k_bin_centers, g[f'd{i}_k_bin_centers'], rtol=1e-12, atol=0)
        np.testing.assert_allclose(d.power, g[f'd{i}_power'], rtol=rtol, atol=0)
        assert analysis.compute_powerspec_σ(d) == pytest.approx(float(g[f'd{i}_sigma']),
                                                                 rel=rtol)


@pytest.mark.parametrize('name', GOLDEN)
def test_powerspec_matches_the_reference(name, tmp_path):
    from concept_amd import analysis
    g = golden(name)
    comps = golden_components(g)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        decls = analysis.powerspec(comps, str(tmp_path/'powerspec'), a=float(g['a']))
    check_against_golden(g, decls)
    cols = np.loadtxt(str(tmp_path/'powerspec'), unpack=True)
    np.testing.assert_allclose(cols[2], decls[0].power, rtol=1e-7)


# -- the reference's test/powerspec, replayed --------------------------------------------------
def _lattice_run(tmp_path, tag, boxsize, gridsize, pos, mass):
    from concept_amd import analysis, commons
    from concept_amd.species import Component
    commons.load_params({
        'boxsize': boxsize, 'enable_Hubble': False,
        'powerspec_select': {'all': {'data': True, 'plot': True}},
        'powerspec_options': {'gridsize': gridsize, 'interpolation': 'PCS', 'interlace': True,
                              'k_max': '1.5*Nyquist', 'tophat': 8.0,
                              'significant figures': 8}})
    c = Component('test particles', 'matter', N=pos.shape[0], mass=mass)
    c.populate(pos, 'pos')
    c.populate(np.zeros_like(pos), 'mom')
    fn = str(tmp_path/f'powerspec_{tag}')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        analysis.powerspec([c], fn)
    del c
    return fn


def test_reference_powerspec_checks(tmp_path):
    from concept_amd import analysis, commons
    L, n_lin, tophat = 512.0, 128, 8.0
    N = n_lin**3
    rng = np.random.default_rng(2024)
    q = np.arange(n_lin)*L/n_lin
    pos = np.stack(np.meshgrid(q, q, q, indexing='ij'), -1).reshape(-1, 3)
    pos = np.mod(pos + rng.normal(0, tophat, (N, 3)), L)
    p = commons.load_params({'boxsize': L, 'enable_Hubble': False})
    mass = p.ρ_mbar*L**3/N
    fn = _lattice_run(tmp_path, 'single', L, 256, pos, mass)
    # counts in cells of the volume of the tophat sphere (test/powerspec/analyze.py:22-55)
    side = (4*math.pi/3*tophat**3)**(1/3)
    n_cubes = int(L//side)
    idx = (pos//side).astype(np.int64)
    keep = (idx < n_cubes).all(1)
    counts = np.bincount(np.ravel_multi_index(idx[keep].T, (n_cubes,)*3),
                         minlength=n_cubes**3)
    σ = np.std(counts/(N*side**3/L**3) - 1)
    σ_file = analysis.load_powerspec_σ(fn, tophat)
    assert σ_file is not None and σ_file == pytest.approx(σ, rel=4e-2), (σ_file, σ)
    # doubled box: k halves, P x 8
    fn2 = _lattice_run(tmp_path, 'double', 2*L, 256, 2*pos, 8*mass)
    k1, _, P1 = np.loadtxt(fn, unpack=True)
    k2, _, P2 = np.loadtxt(fn2, unpack=True)
    assert np.all(np.abs((k1/2 - k2)/k2) < 1e-4)
    assert np.all(np.abs((P1*8 - P2)/P2) < 1e-4)
    # half grid: the same first k, the last k halved, the same power below k_max_half/1.5
    fn3 = _lattice_run(tmp_path, 'half', L, 128, pos, mass)
    k3, _, P3 = np.loadtxt(fn3, unpack=True)
    assert k3[0] == k1[0]
    assert abs(k3[-1]/(k1[-1]/2) - 1) < 4e-2
    below = k3 < k3[-1]/1.5
    P1_at = np.interp(np.log(k3[below]), np.log(k1), P1)
    assert np.all(np.abs(P3[below]/P1_at - 1) < 4e-2), np.abs(P3[below]/P1_at - 1).max()


# -- determinism, and the global-memory path -----------------------------------------------------
def test_binning_is_deterministic_and_matches_numpy():
    import torch
    from concept_amd import analysis, commons
    from concept_amd.mesh import PotentialMesh
    N, L = 64, 100.0
    commons.load_params({'boxsize': L})
    mesh = PotentialMesh(N, L)
    rng = np.random.default_rng(5)
    pos = torch.tensor(rng.uniform(0, L, (40000, 3)), device='cuda')
    mesh.zero()
    mesh.deposit(pos, 1.0)
    mesh.fft_forward()
    mesh.nullify_nyquist()
    slab = mesh.fetch_fourier()
    four = slab[..., 0::2] + 1j*slab[..., 1::2]   # [a][b][kk]
    nyq = N//2
    for bpd, k_max in ((4, 'nyquist'), (10**6, '1.5*nyquist')):
        k2_max, kbi, centers, n_modes = analysis.get_powerspec_bins(N, k_max, {1: bpd, 2: bpd})
        nbins = len(centers)
        table = torch.tensor(kbi, dtype=torch.int32, device='cuda')
        a = mesh.powerspec_bin(table, k2_max, nbins).cpu().numpy()
        b = mesh.powerspec_bin(table, k2_max, nbins).cpu().numpy()
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), 'binning is not deterministic'
        # float64 numpy binning of the fetched slab over the reference's mode set
        k1 = np.arange(N) - np.where(np.arange(N) >= nyq, N, 0)
        ki, kj, kk = np.meshgrid(k1, k1, np.arange(nyq + 1), indexing='ij')
        k2 = ki**2 + kj**2 + kk**2
        visit = ((np.abs(ki) != nyq) & (np.abs(kj) != nyq) & (kk != nyq) & (k2 <= k2_max)
                 & ~((kk == 0) & ((ki > 0) | ((ki == 0) & (kj >= 0)))))
        ref = np.zeros(nbins)
        np.add.at(ref, kbi[k2[visit]], np.abs(four[visit])**2)
        np.testing.assert_allclose(a, ref, rtol=1e-12, atol=1e-300)
        assert np.array_equal(np.bincount(kbi[k2[visit]], minlength=nbins), n_modes)
        if nbins > 1024:
            print(f'global-memory path: {nbins} bins')
    assert nbins > 1024, 'the second binning must exceed the LDS histograms'


def test_the_final_reduction_adds_in_the_documented_order():
    """k_reduce_columns (csrc/cg_wave.h), bit for bit.  cg_powerspec_bin leaves the partial
    histograms in the caller's workspace, so its second stage can be recomputed from them:
    workgroup `bin`, thread t folds the partials t, t + 256, ... of the bin in turn from 0.0, then
    for m = 128, 64, ..., 1 the threads t < m add red[t + m] to red[t].  Grid size 48 on one
    domain gives min(ceil(48·48/4), 2048) = 576 = 2·256 + 64 partials: threads 0-63 fold three,
    the others two — the smallest launch with both the strided fold and a ragged last trip."""
    import torch
    from concept_amd import commons, lib
    from concept_amd.mesh import PotentialMesh
    N, L, nbins = 48, 100.0, 7
    npartials, k2_max = 576, 3*(N//2)**2
    commons.load_params({'boxsize': L})
    mesh = PotentialMesh(N, L)
    _write_real_mesh(mesh, np.random.default_rng(48).standard_normal((N, N, N)))
    mesh.fft_forward()
    table = torch.tensor(np.arange(k2_max + 1)*nbins//(k2_max + 1), dtype=torch.int32,
                         device='cuda')
    assert int(table.min()) == 0 and int(table.max()) == nbins - 1
    assert lib.raw().cg_powerspec_workspace(mesh._ctx, nbins) == npartials*nbins
    workspace = torch.full((npartials*nbins,), np.nan, dtype=torch.float64, device='cuda')
    power = torch.empty(nbins, dtype=torch.float64, device='cuda')
    lib.check(lib.raw().cg_powerspec_bin(mesh._ctx, lib._ptr(table), k2_max, nbins,
                                         lib._ptr(power), lib._ptr(workspace),
                                         workspace.numel()))
    partial = workspace.cpu().numpy().reshape(npartials, nbins)
    assert np.isfinite(partial).all() and (partial > 0).any(axis=0).all()
    red = np.zeros((256, nbins))
    for p0 in range(0, npartials, 256):   # thread t takes partial p0 + t in trip p0/256
        trip = partial[p0:p0 + 256]
        red[:len(trip)] = red[:len(trip)] + trip
    m = 128
    while m >= 1:
        red[:m] = red[:m] + red[m:2*m]
        m >>= 1
    got = power.cpu().numpy()
    assert np.array_equal(got.view(np.int64), red[0].view(np.int64)), (got, red[0])


# -- the binning beyond the first chunk of 64 kk ------------------------------------------------
# A wave of k_powerspec_bin walks a row in chunks of 64 kk and carries a pending run from chunk to
# chunk.  N = 144 (nyq = 72: a second chunk of 8 live lanes, the library FFT's view) and N = 256
# (nyq = 128: two full chunks, the hand-written FFT's view) are the smallest grids of each kind
# with a second chunk.  The reference is the fetched slab binned on the host in np.longdouble, so
# the FFT's own rounding does not enter.
#
# Bar per bin b of n_b visited modes: |got - ref| <= (n_b + 3)·2⁻⁵³·ref.  All terms are
# non-negative, so n_b - 1 additions in any order are off by at most (n_b - 1)·2⁻⁵³ relative to
# first order, and x² + y² brings two roundings of the squares and one of their sum.  The
# longdouble reference itself (64-bit mantissa) is within n_b·2⁻⁶⁴ of the exact sum, 2⁻¹¹ of the
# bar.  A lost or misplaced mode moves a bin by about 1/n_b of itself, which is >= 5e-7 for the
# largest bin here.  On top of that the project's bar of the N = 64 test, 1e-12, is asserted: the
# kernel's lane-wise, butterfly and tree sums stayed below it at every table (measured on an
# MI355X: at most 4.8e-16 in any bin of any table; the figures are printed).
CHUNK_SIZES = (144, 256)
BIN_TABLES = ('coarse', 'fine', 'sqrt', 'one', 'scrambled', 'small', 'edge')
SMALL_RADIUS = {144: 70**2 + 5, 256: 100**2 + 5}
_binning_states = {}


def _sum_by_key(keys, values, n):
    """(sums, counts) of `values` per key in [0, n), added in the values' own precision"""
    order = np.argsort(keys, kind='stable')
    sorted_keys = keys[order]
    starts = np.flatnonzero(np.r_[True, sorted_keys[1:] != sorted_keys[:-1]])
    sums = np.zeros(n, dtype=values.dtype)
    if starts.size:
        sums[sorted_keys[starts]] = np.add.reduceat(values[order], starts)
    return sums, np.bincount(keys, minlength=n)


def _write_real_mesh(mesh, field):
    """the (N, N, N) host array [x][y][z] into the mesh's layers; zeros in the padding"""
    import torch
    N, per, pad = mesh.gridsize, mesh.layer_doubles, mesh.pad
    buf = np.zeros((N, per))
    buf[:, :N*pad].reshape(N, N, pad)[:, :, :N] = field
    mesh.layers_write(0, N, torch.tensor(buf.reshape(-1), device='cuda'))


def _plane_waves(N):
    """[((px, py, pz), amplitude)] with pz = kk at the edges of the chunks of 64"""
    nyq = N//2
    vectors = [(1, 2, 63), (1, 2, 64), (0, 0, 65), (-3, 5, nyq - 1), (2, -1, 0), (0, 3, 0),
               (-(nyq - 1), nyq - 1, 1)]
    rng = np.random.default_rng(N)
    return list(zip(vectors, rng.uniform(0.5, 2.0, len(vectors))))


def _binning_state(N, kind):
    """A mesh whose Fourier view holds `kind` ('particles': the transform of a deposit with
    the Nyquist planes nullified; 'waves': the transform of _plane_waves), with the longdouble
    sum of |z|² and the number of the visited modes of the fetched slab for every k².  Made
    once per (N, kind) and left unchanged."""
    import types
    import torch
    from concept_amd import commons
    from concept_amd.mesh import PotentialMesh
    state = _binning_states.get((N, kind))
    if state is not None:
        return state
    L = 100.0
    commons.load_params({'boxsize': L})
    mesh = PotentialMesh(N, L)
    nyq = N//2
    if kind == 'particles':
        rng = np.random.default_rng(5 + N)
        pos = torch.tensor(rng.uniform(0, L, (40000, 3)), device='cuda')
        mesh.zero()
        mesh.deposit(pos, 1.0)
        mesh.fft_forward()
        mesh.nullify_nyquist()
    else:
        cos_table = np.cos(2*np.pi*np.arange(N)/N)
        x = np.arange(N)
        field = np.zeros((N, N, N))
        for (px, py, pz), amplitude in _plane_waves(N):
            phase = (px*x[:, None, None] + py*x[None, :, None] + pz*x[None, None, :]) % N
            field += amplitude*cos_table[phase]
        _write_real_mesh(mesh, field)
        mesh.fft_forward()
    # the debug fetch is the reference's transposed slab: [b][a][kk] for the view's four[a][b][kk]
    slab = mesh.fetch_fourier().transpose(1, 0, 2)
    k1 = np.arange(N) - np.where(np.arange(N) >= nyq, N, 0)
    ki, kj, kk = np.meshgrid(k1, k1, np.arange(nyq + 1), indexing='ij', sparse=True)
    k2 = ki**2 + kj**2 + kk**2
    visit = ((np.abs(ki) != nyq) & (np.abs(kj) != nyq) & (kk != nyq)
             & ~((kk == 0) & ((ki > 0) | ((ki == 0) & (kj >= 0)))))
    re = slab[..., 0::2][visit].astype(np.longdouble)
    im = slab[..., 1::2][visit].astype(np.longdouble)
    k2_top = 3*nyq**2
    power, n_modes = _sum_by_key(k2[visit], re*re + im*im, k2_top + 1)
    state = types.SimpleNamespace(mesh=mesh, N=N, nyq=nyq, k2_top=k2_top, power=power,
                                  n_modes=n_modes)
    _binning_states[N, kind] = state
    return state


def _check_binning(state, label, k2_max, table, nbins, known=()):
    """cg_powerspec_bin with `table` (k2_max + 1 bins) against the longdouble sums of the fetched
    slab at the bar above; two calls bit for bit; known: (bin, power) pairs asserted at 1e-12.
    Returns the worst |got - ref|/ref."""
    import torch
    table = np.ascontiguousarray(table, dtype=np.int32)
    assert table.shape == (k2_max + 1,) and table.min() >= 0 and table.max() < nbins
    device_table = torch.tensor(table, device='cuda')
    got = state.mesh.powerspec_bin(device_table, k2_max, nbins).cpu().numpy()
    again = state.mesh.powerspec_bin(device_table, k2_max, nbins).cpu().numpy()
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), 'binning is not deterministic'
    occupied = np.flatnonzero(state.n_modes[:k2_max + 1])
    ref, _ = _sum_by_key(table[occupied].astype(np.int64), state.power[occupied], nbins)
    n_b = np.bincount(table[occupied], weights=state.n_modes[occupied], minlength=nbins)
    assert np.all(got[n_b == 0] == 0), f'{label}: power in bins without modes'
    assert np.all(got[ref == 0] == 0), f'{label}: power in bins whose modes are all zero'
    filled = ref > 0
    assert filled.any()
    rel = np.abs(got[filled].astype(np.longdouble) - ref[filled])/ref[filled]
    ratio = rel/((n_b[filled] + 3)*2.0**-53)
    worst = int(np.argmax(ratio))
    print(f'{label}: {nbins} bins ({int(filled.sum())} filled, {int(n_b.sum())} modes, largest '
          f'{int(n_b.max())}), {"global-memory" if nbins > 1024 else "LDS"} histograms: worst '
          f'|got - ref|/ref = {float(rel.max()):.3e}; worst ratio to (n_b + 3)·2^-53 = '
          f'{float(ratio[worst]):.3f} (a bin of {int(n_b[filled][worst])} modes)')
    assert ratio.max() <= 1, (label, float(ratio.max()))
    assert rel.max() <= 1e-12, (label, float(rel.max()))
    for b, power in known:
        err = abs(got[b]/power - 1)
        print(f'{label}: bin {b}: {got[b]:.16e} against the known {power:.16e}, '
              f'relative {err:.3e}')
        assert err <= 1e-12, (label, b, got[b], power)
    return n_b, float(rel.max())


def _bin_table(name, N):
    """(k2_max, table, nbins, n_modes of the analysis or None)"""
    from concept_amd import analysis
    nyq = N//2
    if name in ('coarse', 'fine'):
        k_max, bpd = ('nyquist', 4) if name == 'coarse' else ('1.5*nyquist', 10**6)
        k2_max, table, centers, n_modes = analysis.get_powerspec_bins(N, k_max, {1: bpd, 2: bpd})
        return k2_max, table, len(centers), n_modes
    k2_max = SMALL_RADIUS[N] if name == 'small' else 3*nyq**2
    k2 = np.arange(k2_max + 1)
    if name == 'one':
        table = np.zeros(k2_max + 1, dtype=np.int64)
    elif name == 'scrambled':   # not monotonic along kk
        table = (k2*7) % 13
    elif name == 'edge':
        # the bin changes between kk = 63 and 64 in the rows with ki² + kj² < 127: a chunk inside
        # one bin follows a chunk inside another, so a pending run is closed by a one-bin chunk
        table = (k2 >= 64**2).astype(np.int64)
    else:                       # 'sqrt', 'small': chunks that straddle an edge, chunks inside a bin
        table = np.array([math.isqrt(int(v)) for v in k2])//3
    return k2_max, table, int(table.max()) + 1, None


@pytest.mark.parametrize('name', BIN_TABLES)
@pytest.mark.parametrize('N', CHUNK_SIZES)
def test_binning_past_the_first_chunk(N, name):
    state = _binning_state(N, 'particles')
    k2_max, table, nbins, n_modes = _bin_table(name, N)
    n_b, _ = _check_binning(state, f'N = {N}, {name} bins', k2_max, table, nbins)
    if name == 'fine':
        assert nbins > 1024, 'the fine bins must exceed the LDS histograms'
    if name == 'small':   # rows near the axis end inside the second chunk, others before it
        assert 64**2 < k2_max < (state.nyq - 1)**2
    if n_modes is not None:
        np.testing.assert_array_equal(n_b.astype(np.int64), n_modes)


@pytest.mark.parametrize('N', CHUNK_SIZES)
def test_plane_waves_at_the_chunk_edges(N):
    """A·cos(2π p·x/N) has the two modes ±p of amplitude A·N³/2, of which the walk visits one:
    the bin of |p|² holds (A·N³/2)² (the other modes of the bin hold the transform's rounding,
    some 1e-30 of it)."""
    state = _binning_state(N, 'waves')
    waves = _plane_waves(N)
    nyq = N//2
    for (px, py, pz), _ in waves:   # none on a Nyquist plane
        assert abs(px) < nyq and abs(py) < nyq and 0 <= pz < nyq
    power = {px*px + py*py + pz*pz: (amplitude*N**3/2)**2 for (px, py, pz), amplitude in waves}
    assert len(power) == len(waves)
    k2_max = state.k2_top
    k2 = np.arange(k2_max + 1)
    # bin = k²: the global-memory histograms
    assert k2_max + 1 > 1024
    _check_binning(state, f'N = {N}, waves, bin = k2', k2_max, k2, k2_max + 1,
                   known=sorted(power.items()))
    # bin = min(k², 1023): the LDS histograms; the waves beyond share the last bin
    known = [(b, v) for b, v in sorted(power.items()) if b < 1023]
    known.append((1023, math.fsum(v for b, v in power.items() if b >= 1023)))
    assert len(known) == 3
    _check_binning(state, f'N = {N}, waves, bin = min(k2, 1023)', k2_max, np.minimum(k2, 1023),
                   1024, known=known)


# -- the time loop's dumps and the utility ------------------------------------------------------
def test_timeloop_dumps_powerspec_files(tmp_path):
    import torch
    from concept_amd import analysis, commons, snapshot
    from concept_amd import powerspec as utility
    from concept_amd.stepper import Timeloop
    from concept_amd.species import Component
    out = tmp_path/'out'
    param = tmp_path/'param'
    param.write_text(f"""
boxsize = 64*Mpc
potential_options = {{'gridsize': {{'gravity': {{'pm': 32}}}}}}
select_forces = {{'matter': {{'gravity': 'pm'}}}}
a_begin = 0.1
output_dirs = {{'snapshot': '{out}', 'powerspec': '{out}'}}
output_times = {{'snapshot': [0.12, 0.14], 'powerspec': [0.11, 0.12, 0.14]}}
snapshot_type = 'gadget'
gadget_snapshot_params = {{'dataformat': {{'POS': 64, 'VEL': 64}}}}
powerspec_options = {{'gridsize': 32}}
powerspec_select = {{'matter': True}}
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
    assert names == ['powerspec_a=0.11', 'powerspec_a=0.12', 'powerspec_a=0.14',
                     'snapshot_a=0.12', 'snapshot_a=0.14'], names
    for a in ('0.12', '0.14'):
        snap_fn = str(out/f'snapshot_a={a}')
        s = snapshot.load(snap_fn, params=p, units=p.gadget_snapshot_params['units'])
        comps = s.to_components()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            decls = analysis.powerspec(comps, str(tmp_path/f'again_{a}'), a=float(s.params['a']))
        k, modes, P = np.loadtxt(str(out/f'powerspec_a={a}'), unpack=True)
        k2, modes2, P2 = np.loadtxt(str(tmp_path/f'again_{a}'), unpack=True)
        np.testing.assert_array_equal(modes, modes2)
        np.testing.assert_allclose(P, P2, rtol=1e-10)
        np.testing.assert_allclose(P, decls[0].power, rtol=1e-7)
        # the utility (-u powerspec): <base>_<snapshot basename>
        fn = utility.main([snap_fn, '--params', str(param), '--output-dir', str(tmp_path)])
        assert os.path.basename(fn) == f'powerspec_snapshot_a={a}'
        k3, modes3, P3 = np.loadtxt(fn, unpack=True)
        np.testing.assert_array_equal(P3, P2)
        commons.load_params(str(param))


# -- at size -------------------------------------------------------------------------------------
def test_powerspec_at_1024(tmp_path):
    import torch
    from concept_amd import analysis, commons
    from concept_amd.species import Component
    from concept_amd.mesh import free_meshes
    n_lin, N, L = 512, 1024, 1000.0
    n = n_lin**3
    opts = {'gridsize': N, 'interpolation': 'PCS', 'interlace': True}
    p = commons.load_params({'boxsize': L, 'powerspec_options': opts,
                             'powerspec_select': {'matter': True}})
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
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        decl = analysis.get_powerspec_declarations([c])[0]
        analysis.compute_powerspec(decl, timings=timings)   # warm-up (plans, tables)
        t0 = time.perf_counter()
        analysis.compute_powerspec(decl, timings=timings)
        wall = time.perf_counter() - t0
    P = decl.power.copy()
    # the binning alone, repeated
    mesh = analysis._mesh(N, 'powerspec')
    table = analysis._device_bin_table(decl, mesh.device)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = 10
    e[0].record()
    for _ in range(reps):
        mesh.powerspec_bin(table, decl.k2_max, len(decl.k_bin_centers))
    e[1].record()
    e[1].synchronize()
    t_bin = e[0].elapsed_time(e[1])*1e-3/reps
    # bytes read: the rows and kk ranges inside the sphere, 16 B per complex mode
    nyq = N//2
    k1 = np.arange(N) - np.where(np.arange(N) >= nyq, N, 0)
    r2 = (k1[:, None]**2 + k1[None, :]**2).astype(np.int64)
    inside = (np.abs(k1[:, None]) != nyq) & (np.abs(k1[None, :]) != nyq) & (r2 <= decl.k2_max)
    kk_end = np.minimum(np.floor(np.sqrt(np.maximum(decl.k2_max - r2, 0))).astype(np.int64) + 1,
                        nyq)
    bytes_read = 16*int(kk_end[inside].sum())
    print(f'\n1024^3 power spectrum of {n} particles: upstream (deposits + FFTs) '
          f'{timings["upstream"]*1e3:.1f} ms, binning {timings["binning"]*1e3:.3f} ms in the '
          f'run, {t_bin*1e3:.3f} ms alone ({bytes_read/1e9:.2f} GB read, '
          f'{bytes_read/t_bin/1e12:.2f} TB/s = {bytes_read/t_bin/8e12:.2f} of 8 TB/s); '
          f'wall {wall*1e3:.0f} ms')
    assert decl.n_modes.sum() == analysis.n_modes_per_k2(N, decl.k2_max)[1:].sum()
    assert np.all(np.isfinite(P)) and np.all(P > 0)
    # the same particles through CIC without interlacing: the same spectrum below k_nyq/2
    commons.load_params({'boxsize': L, 'powerspec_select': {'matter': True},
                         'powerspec_options': dict(opts, interpolation='CIC', interlace=False)})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        decl_cic = analysis.get_powerspec_declarations([c])[0]
        analysis.compute_powerspec(decl_cic)
    k_nyq = 2*math.pi/L*nyq
    low = decl.k_bin_centers < k_nyq/2
    np.testing.assert_array_equal(decl.k_bin_centers, decl_cic.k_bin_centers)
    rel = np.abs(decl_cic.power[low]/P[low] - 1)
    assert rel.max() < 0.05, rel.max()
    del c, mesh, table
    free_meshes()
    torch.cuda.empty_cache()


# -- x-slab domains ------------------------------------------------------------------------------
@pytest.mark.parametrize('world', [2, 4])
def test_powerspec_on_domains(world):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, 'powerspec_worker.py')] + list(GOLDEN),
            env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0 and f'RANK{r}-OK' in outs[r], f'rank {r}:\n{outs[r][-4000:]}'
