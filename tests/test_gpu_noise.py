"""The primordial noise drawn on the GPU (csrc/cg_noise.hip, ic.generate_primordial_noise_device)
against the host slab of ic.generate_primordial_noise, which tests/test_ic_host.py pins to the
reference bit for bit, and the realisations with noise_on='device' against the reference's own
(tests/golden/lpt_*.npz, fluid_ic_*.npz).

Bars.  The amplitudes and the uniform numbers are integer arithmetic and one rounding each: the
host's bits.  cos, sin and the ziggurat's rare exp and log1p are the device library's, a few ulp
of a value of order 1: |device - host| <= 1e-12·max |host slab|, the project's parity bar.  A
wedge comparison of the ziggurat that went the other way would shift the rest of its stream and
show as a difference of order 1.  What the host leaves 0 is exactly 0.  The realisations: the bars
of tests/test_gpu_lpt.py and tests/test_gpu_fluid_ic.py for the host path."""
import functools
import glob
import os

import numpy as np
import pytest

import lpt_refs
from test_gpu_lpt import close

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
L = 100.0
SENTINEL = 1234.5
KW = {
    'plain': {},
    'shift': {'primordial_phase_shift': 0.75},
    'fixed': {'primordial_amplitude_fixed': True},
    'fixed-shift': {'primordial_amplitude_fixed': True, 'primordial_phase_shift': np.pi},
    'seeds': {'random_seeds': {'primordial amplitudes': 77, 'primordial phases': 4242}},
}


def load(kw):
    from concept_amd import commons
    return commons.load_params({'boxsize': L, **KW[kw]})


@functools.lru_cache(maxsize=None)
def host_slab(gridsize, kw):
    from concept_amd import ic
    p = load(kw)
    slab = ic.generate_primordial_noise(gridsize, p.primordial_amplitude_fixed,
                                        p.primordial_phase_shift, p)
    slab.setflags(write=False)
    return slab


def more_than_a_trip():
    """64 (2016 draws a slice), or the smallest even grid size whose slice outlasts a trip"""
    from concept_amd import lib
    trip = int(lib.raw().cg_noise_trip())
    g = 64
    while (g - 1)*g//2 <= trip:
        g += 2
    return g


def device_native(gridsize, kw):
    """the mesh's whole buffer, double[i][rows][pad], after the device noise was drawn into a
    mesh full of the sentinel"""
    import torch
    from concept_amd import ic
    from concept_amd.mesh import PotentialMesh
    p = load(kw)
    g = gridsize
    mesh = PotentialMesh(g, L)
    rows = mesh.layer_doubles//mesh.pad
    fill = torch.full((g, rows, mesh.pad), SENTINEL, dtype=torch.float64, device='cuda')
    mesh.layers_write(0, g, fill)
    out = ic.generate_primordial_noise_device(mesh, p.primordial_amplitude_fixed,
                                              p.primordial_phase_shift, p)
    assert out is mesh
    buf = torch.empty(g*mesh.layer_doubles, dtype=torch.float64, device='cuda')
    mesh.layers_read(0, g, buf)
    return buf.cpu().numpy().reshape(g, rows, mesh.pad), mesh


CASES = [(8, kw) for kw in KW] + [(12, kw) for kw in KW] + [('trip', 'plain'), ('trip', 'seeds'),
                                                            ('trip', 'fixed-shift')]


@pytest.mark.parametrize('gridsize, kw', CASES)
def test_the_device_noise_is_the_host_s(gridsize, kw):
    g = more_than_a_trip() if gridsize == 'trip' else gridsize
    nyq = g//2
    ref = host_slab(g, kw)
    native, mesh = device_native(g, kw)
    got = native[:, :g, :g + 2].transpose(1, 0, 2)  # the host's [j][i][g + 2]
    # the Nyquist planes, the origin and whatever else the host leaves 0: exactly 0
    assert not got[nyq].any() and not got[:, nyq].any() and not got[:, :, 2*nyq:].any()
    assert not got[0, 0, :2].any()
    assert not got[ref == 0].any()
    assert not native[:, :g, g + 2:].any()              # the row padding of the view
    assert (native[:, g:] == SENTINEL).all()            # the unused row of a layer
    assert np.array_equal(mesh.fetch_fourier(), got)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f'g = {g}, {kw}: largest deviation {err:.3e} = {err/scale:.3e} of max |host slab| '
          f'{scale:.3e}; {np.count_nonzero(got != ref)} of {np.count_nonzero(ref)} numbers differ')
    assert err <= 1e-12*scale
    # the kk = 0 plane is Hermitian
    plane = got[:, :, 0] + 1j*got[:, :, 1]
    mirror = np.conj(plane[(-np.arange(g)) % g][:, (-np.arange(g)) % g])
    assert np.array_equal(plane, mirror)
    # a second run gives the same bits
    again, _ = device_native(g, kw)
    assert np.array_equal(again, native)


def golden_cases(prefix):
    names = sorted(os.path.basename(f)[len(prefix):-4]
                   for f in glob.glob(os.path.join(GOLDEN, prefix + '*.npz')))
    return [n for n in names if 'simple' not in n]  # the 'simple' scheme is refused: see below


@pytest.mark.parametrize('case', golden_cases('lpt_'))
def test_realize_particles_with_device_noise_against_the_golden(golden, case):
    from concept_amd import commons, ic
    from concept_amd.species import Component
    g = golden('lpt_' + case)
    commons.load_params(str(g['param_text']))
    n = int(g['gridsize'])
    assert n in (8, 12)

    def realize():
        c = Component('matter', 'matter', N=n**3, mass=float(g['mass']))
        ic.n_particles_realized.update(components_tally=int(g['components_tally']),
                                       components_total=int(g['components_total']),
                                       particles_tally=int(g['id_bgn']))
        growth = dict(zip(g['growth_keys'].tolist(), g['growth_values'].tolist()))
        timings = {}
        grids = ic.realize_particles(c, float(g['a']), g['amplitudes'], g['amplitudes_θ'], growth,
                                     timings=timings, noise_on='device')
        assert timings['noise (device)'] > 0
        assert 'noise (host)' not in timings and 'upload' not in timings
        return c, grids
    c, grids = realize()
    pos, mom, ids = c.host('pos'), c.host('mom'), c.host('ids')
    assert np.array_equal(ids, g['ids'])
    d = np.abs(pos - g['pos'])
    d = np.minimum(d, L - d).max()/(L/n)
    e = np.abs(mom - g['mom']).max()/np.abs(g['mom']).max()
    print(f'{case}: positions within {d:.3e} of a cell, momenta within {e:.3e} of max |mom|')
    assert d <= 1e-12 and e <= 1e-12
    assert (pos >= 0).all() and (pos < L).all()
    live = np.repeat(lpt_refs.alive(n), 2, axis=2)
    assert close(grids['Φ1'].fetch_fourier()*live, g['Phi1'], 1e-14)
    if 'Phi2' in g.files:
        err = np.abs(grids['Φ2'].fetch_fourier()*live - g['Phi2']*live).max()
        print(f'Φ2 within {err/np.abs(g["Phi1"]).max():.3e} of the Φ1 scale')
        assert err <= 1e-12*np.abs(g['Phi1']).max()
    c2, _ = realize()
    assert np.array_equal(c2.host('pos'), pos) and np.array_equal(c2.host('mom'), mom)


@pytest.mark.parametrize('case', golden_cases('fluid_ic_'))
def test_realize_a_fluid_with_device_noise_against_the_golden(golden, case):
    from concept_amd import commons, ic
    from concept_amd.species import Component
    g = golden('fluid_ic_' + case)
    commons.load_params(str(g['param_text']))
    a, ϱ_bar = float(g['a']), float(g['rho_bar'])
    c = Component('matter', 'matter', gridsize=int(g['gridsize']), boltzmann_order=1)
    timings = {}
    noise = ic.realize(c, a, g['amplitudes'], g['amplitudes_θ'], noise_on='device',
                       timings=timings)
    assert timings['noise (device) passes'] == 1  # one slab for ϱ and the three J
    assert 'noise (host)' not in timings and 'upload' not in timings
    ϱ, J = c.host('ϱ'), c.host('J')
    live = np.repeat(lpt_refs.alive(int(g['gridsize'])), 2, axis=2)
    assert close(noise.fetch_fourier()*live, g['noise'], 1e-12)
    e = np.abs(ϱ - g['rho']).max()/ϱ_bar
    print(f'{case}: ϱ within {e:.3e} of ϱ_bar')
    assert e <= 1e-12
    for i in range(3):
        e = np.abs(J[i] - g['J'][i]).max()/np.abs(g['J'][i]).max()
        print(f'{case}: J[{i}] within {e:.3e} of max |J[{i}]|')
        assert e <= 1e-12
    c0 = Component('matter', 'matter', gridsize=int(g['gridsize']), boltzmann_order=0)
    ic.realize_fluid(c0, a, g['amplitudes'], noise_on='device')
    assert np.array_equal(c0.host('ϱ'), ϱ)


def small_particles(**kw):
    from concept_amd import commons, ic
    from concept_amd.species import Component
    p = commons.load_params({'boxsize': L, 'H0': 0.07, 'Ωb': 0.05, 'Ωcdm': 0.25, 'a_begin': 0.02,
                             'realization_options': {'backscale': True}, **kw})
    k = np.geomspace(1e-3, 10, 200)
    amplitudes = ic.amplitudes_from_power(k, 2e3*k/(1 + (k/0.1)**2)**1.5, 8, L)
    c = Component('matter', 'matter', N=8**3, mass=-1)
    ic.reset_tally()
    return p, c, amplitudes, {'D1': 0.02, 'f1': 1.0}


@pytest.mark.parametrize('kw, what', [
    ({'primordial_noise_imprinting': 'simple'},
     'primordial_noise_imprinting = "simple" is not implemented'),
    ({'random_generator': 'PCG64'}, 'random_generator = "PCG64" is not implemented'),
    ({'random_generator': 'Philox'}, 'random_generator = "Philox" is not implemented'),
    ({'nprocs': 2}, "noise_on='device' with an active comm process group"),
    ({'noise_on': 'gpu'}, "noise_on = 'gpu' is neither 'host' nor 'device'"),
])
def test_device_noise_refuses_by_name(kw, what):
    from concept_amd import ic
    from concept_amd.lib import ConceptGPUError
    from concept_amd.species import Component
    kw = dict(kw)
    nprocs, noise_on = kw.pop('nprocs', 1), kw.pop('noise_on', 'device')
    p, c, amplitudes, growth = small_particles(**kw)
    c.nprocs = nprocs
    mom = c.host('mom').copy()
    with pytest.raises(ConceptGPUError, match=what):
        ic.realize_particles(c, p.a_begin, amplitudes, growth_factors=growth, noise_on=noise_on)
    assert np.array_equal(c.host('mom'), mom)  # nothing was realised, on the host either
    fluid = Component('fluid', 'matter', gridsize=8, boltzmann_order=0)
    fluid.nprocs = nprocs
    with pytest.raises(ConceptGPUError, match=what):
        ic.realize(fluid, p.a_begin, amplitudes, noise_on=noise_on)
    if nprocs == 1 and noise_on == 'device':
        from concept_amd.mesh import PotentialMesh
        with pytest.raises(ConceptGPUError, match=what):
            ic.generate_primordial_noise_device(PotentialMesh(8, L), params=p)


@pytest.mark.parametrize('noise_on', [None, 'host'])
def test_the_host_path_keeps_its_timings(noise_on):
    from concept_amd import ic
    p, c, amplitudes, growth = small_particles()
    timings = {}
    kw = {} if noise_on is None else {'noise_on': noise_on}
    ic.realize_particles(c, p.a_begin, amplitudes, growth_factors=growth, timings=timings, **kw)
    assert timings['noise (host)'] > 0 and timings['upload'] > 0
    assert not [key for key in timings if 'device' in key]
    host = c.host('pos').copy()
    # and the device path moves the particles to the same places
    p, c, amplitudes, growth = small_particles()
    ic.realize_particles(c, p.a_begin, amplitudes, growth_factors=growth, noise_on='device')
    d = np.abs(c.host('pos') - host)
    assert np.minimum(d, L - d).max() <= 1e-12*(L/8)


def test_the_entry_checks_its_tables():
    import torch
    from concept_amd import ic, lib
    from concept_amd.mesh import PotentialMesh
    mesh = PotentialMesh(8, L)
    trip = int(lib.raw().cg_noise_trip())
    assert trip % 64 == 0

    def dev(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    streams = dev(ic.noise_stream_table(8, False, load('plain')))
    order, jump = dev(ic.noise_order_table(8)), dev(ic.pcg64dxsm_jump_table(trip))
    mesh.noise_generate(streams, order, jump)
    with pytest.raises(lib.ConceptGPUError, match='6 spawn keys for grid size 8, which has 7'):
        mesh.noise_generate(streams[:6], order, jump)
    with pytest.raises(lib.ConceptGPUError, match='27 points per slice for grid size 8, which '
                                                  'has 28'):
        mesh.noise_generate(streams, order[:27], jump)
    with pytest.raises(lib.ConceptGPUError, match=f'{trip} rows, {trip + 1} needed'):
        mesh.noise_generate(streams, order, jump[:trip])
    with pytest.raises(lib.ConceptGPUError, match='order must be a contiguous torch.int32'):
        mesh.noise_generate(streams, order.to(torch.int64), jump)
