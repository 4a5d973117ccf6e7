"""The bispectrum core on the GPU: cg_bispec_shell and cg_bispec_sums against
the NumPy restatement (tests/bispec_refs.py), compute_bispec_value against the reference's
goldens, bispec_measure on one domain and on two x-slab domains, and a known answer."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bispec_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
BOXSIZE = 100.0
SENTINEL = 777.25


def setup(boxsize=BOXSIZE):
    from concept_amd import analysis, commons
    commons.load_params({'boxsize': boxsize})
    analysis.bispec_grid_cache.clear()
    return analysis


def raw(mesh):
    """the mesh buffer as it lies in memory: double[N][ny][pad]"""
    import torch
    N = mesh.gridsize
    buf = torch.empty(N*mesh.layer_doubles, dtype=torch.float64, device=mesh.device)
    mesh.layers_read(0, N, buf)
    return buf.cpu().numpy().reshape(N, mesh.layer_doubles//mesh.pad, mesh.pad)


def fill_raw(mesh, value):
    import torch
    N = mesh.gridsize
    mesh.layers_write(0, N, torch.full((N*mesh.layer_doubles,), value, dtype=torch.float64,
                                       device=mesh.device))


def fourier_view(mesh):
    """complex F[a, b, kk] of the whole view, padding included: (N, N, pad/2)"""
    r = raw(mesh)[:, :mesh.gridsize, :]
    return r[..., 0::2] + 1j*r[..., 1::2]


def load_real(mesh, field):
    import torch
    mesh.fluid_add(torch.from_numpy(np.ascontiguousarray(field)).to(mesh.device).reshape(-1), 1.0,
                   '=')


def load_fourier(mesh, field):
    """the reference's slab of a real field: the forward transform of field/N³"""
    load_real(mesh, field*float(mesh.gridsize)**-3)
    mesh.fft_forward()


@pytest.fixture(scope='module')
def fields():
    rng = np.random.default_rng(5)
    return {N: 1.0 + 0.5*rng.normal(size=(3, N, N, N)) for N in (12, 40)}


SHELLS = {8: [(0.5, 1.5), (0.0, 1.2), (2.0, 3.5), (1.1, 1.3)],
          12: [(0.875, 1.125), (1.5, 2.5), (3.5, 5.5), (1.1, 1.3)],
          40: [(0.875, 1.125), (3.3, 6.1), (16.5, 19.5), (5.1, 5.2)]}


@pytest.mark.parametrize('N', [8, 12, 40])
def test_shell_fill_matches_the_restatement(N):
    analysis = setup()
    rng = np.random.default_rng(N)
    src, dst = analysis._mesh(N, 'bispec'), analysis._mesh(N, 'bispec 0')
    load_fourier(src, 1.0 + 0.5*rng.normal(size=(N, N, N)))
    F_src = fourier_view(src)
    nyq, cp = N//2, src.pad//2
    unused_rows = raw(dst).shape[1] - N
    for shell in SHELLS[N]:
        tol = R.OVERLAP_BAR_DEVICE*max(1.0, shell[1]**3)
        for antialiasing in (True, False):
            for source in (None, src):
                fill_raw(dst, SENTINEL)
                dst.bispec_shell(shell, source, antialiasing)
                got = fourier_view(dst)
                want = np.zeros((N, N, cp), dtype=np.complex128)
                want[:, :, :nyq + 1] = R.shell_fill(
                    N, shell, antialiasing, None if source is None else F_src[:, :, :nyq + 1])
                scale = 1.0 if source is None else np.abs(F_src)
                zero = want == 0
                label = (N, shell, antialiasing, source is not None)
                # outside the shell, the padding included: assigned, and exactly zero
                assert (got[zero] == 0).all(), label
                dev = np.abs(got - want)
                assert (dev <= tol*scale).all(), (label, dev.max())
                if not antialiasing:
                    assert (got[~zero] == want[~zero]).all(), label
                if unused_rows:   # the row outside the view is not written
                    assert (raw(dst)[:, N:, :] == SENTINEL).all()
        if shell != SHELLS[N][-1]:
            assert (want != 0).sum() > 0
    # the source is only read
    np.testing.assert_array_equal(fourier_view(src), F_src)


@pytest.mark.parametrize('N', [12, 40])
def test_sums_match_fsum_and_repeat_bit_for_bit(N, fields):
    import torch
    analysis = setup()
    meshes = [analysis._mesh(N, f'bispec {n}') for n in range(3)]
    for mesh, field in zip(meshes, fields[N]):
        fill_raw(mesh, 1e30)   # the padding must not be summed
        load_real(mesh, field)
    grids = [raw(m)[:, :N, :N].copy() for m in meshes]
    for g, field in zip(grids, fields[N]):
        np.testing.assert_array_equal(g, field)
    for n_unique in (1, 2, 3):
        for mask in range(1 << n_unique):
            want = [bool(mask >> q & 1) for q in range(n_unique)]
            value, powers, scale = R.sums_exact(grids[:n_unique], want)
            out = meshes[0].bispec_sums(meshes[1:n_unique], mask)
            again = meshes[0].bispec_sums(meshes[1:n_unique], mask)
            assert torch.equal(out, again)
            got = out.cpu().tolist()
            print(N, n_unique, mask, abs(got[0] - value)/scale)
            assert abs(got[0] - value) <= R.SUMS_BAR*scale
            for q in range(3):
                if q < n_unique and want[q]:
                    assert abs(got[1 + q] - powers[q]) <= R.SUMS_BAR*powers[q]
                else:
                    assert got[1 + q] == 0
    from concept_amd.lib import ConceptGPUError
    with pytest.raises(ConceptGPUError, match='power mask'):
        meshes[0].bispec_sums((), 2)
    with pytest.raises(ConceptGPUError, match='are one'):
        meshes[0].bispec_sums((meshes[1], meshes[1]), 0)


@pytest.mark.parametrize('N', [8, 12])
def test_compute_bispec_value_matches_the_reference(golden, N):
    analysis = setup()
    g = golden(f'bispec_value_g{N}')
    slab = analysis._mesh(N, 'bispec')
    load_fourier(slab, g['field'])
    F = R.from_slab(g['slab'])
    np.testing.assert_allclose(fourier_view(slab)[:, :, :N//2 + 1], F, atol=1e-14)
    for antialiasing, tag in ((True, 'aa'), (False, 'noaa')):
        analysis.bispec_grid_cache.clear()
        power_ind, power = {}, {}
        for data in (False, True):
            pd = power if data else power_ind
            kind = 'data' if data else 'indicator'
            for b, shells in enumerate(g['bins']):
                shells = tuple(tuple(s) for s in shells)
                scale = {}
                R.bispec_value(N, shells, None, F if data else None, antialiasing, scale)
                if data:
                    value = analysis.compute_bispec_value(N, shells, pd, slab,
                                                          antialiasing=antialiasing)
                else:
                    value, new = analysis.compute_bispec_value(N, shells, pd,
                                                               antialiasing=antialiasing)
                    assert len(new) == g[f'{tag}_indicator_new'][b]
                ref = g[f'{tag}_{kind}_value'][b]
                print(N, tag, kind, b, abs(value - ref)/max(scale['abs'], 1e-300))
                assert abs(value - ref) <= R.SUMS_BAR*scale['abs'], (tag, kind, b, value, ref)
            assert [list(k) for k in pd] == g[f'{tag}_power_shells'].tolist()
            for value, ref in zip(pd.values(), g[f'{tag}_{kind}_power']):
                assert abs(value - ref) <= R.SUMS_BAR*ref
    analysis.bispec_grid_cache.clear()


# -- bispec_measure on one and on two domains ----------------------------------------------------
MEASURE_N = 16
MEASURE_BINS = [((0.5, 1.5), (1.5, 2.5), (2.25, 3.0)), ((1.5, 2.5), (1.5, 2.5), (2.25, 3.0)),
                ((2.25, 3.0), (2.25, 3.0), (2.25, 3.0)), ((1.1, 1.3), (0.5, 1.5), (1.5, 2.5)),
                ((4.0, 5.5), (5.0, 7.5), (0.5, 1.5))]


def measure(antialiasing):
    from concept_amd.species import Component
    analysis = setup()
    from concept_amd import commons
    rng = np.random.default_rng(11)
    n = 8**3
    pos = rng.uniform(0, BOXSIZE, (n, 3))
    c = Component('matter', 'matter', N=n, mass=commons.params.ρ_mbar*BOXSIZE**3/n)
    c.populate(pos, 'pos')
    c.populate(np.zeros((n, 3)), 'mom')
    return analysis.bispec_measure([c], MEASURE_BINS, MEASURE_N, a=0.5,
                                   antialiasing=antialiasing)


def test_bispec_measure_on_one_and_on_two_domains():
    from concept_amd import commons
    N = MEASURE_N
    one, scales = {}, {}
    for antialiasing in (True, False):
        res = measure(antialiasing)
        tag = 'aa' if antialiasing else 'noaa'
        one[tag] = res
        # Σ|g₀g₁g₂| per bin from the slab the measurement left on the device
        analysis = setup()
        F = fourier_view(analysis._mesh(N, 'bispec'))[:, :, :N//2 + 1]
        scales[tag], scales[tag + ' indicator'] = [], []
        for shells in MEASURE_BINS:
            scale = {}
            R.bispec_value(N, shells, None, F, antialiasing, scale)
            scales[tag].append(scale['abs'])
            R.bispec_value(N, shells, None, None, antialiasing, scale)
            scales[tag + ' indicator'].append(scale['abs'])
    res = one['noaa']
    np.testing.assert_allclose(res.n_modes, np.rint(res.n_modes), atol=1e-9)
    assert res.n_modes[3] == 0 and np.isnan(res.bpower[3]) and res.n_modes[0] > 0
    assert np.isfinite(res.bpower[[0, 1, 2, 4]]).all()
    world = 2
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'bispec_worker.py')],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0 and f'RANK{r}-OK' in outs[r], f'rank {r}:\n{outs[r][-4000:]}'
    line = [ln for ln in outs[0].splitlines() if ln.startswith('RESULT ')][0]
    two = json.loads(line[len('RESULT '):])
    ρ_bar = 0.5**-3*commons.params.ρ_mbar
    for tag in ('aa', 'noaa'):
        a, b = one[tag], two[tag]
        tol = R.SUMS_BAR*np.array(scales[tag + ' indicator'])*0.5/N**3
        assert (np.abs(np.array(b['n_modes']) - a.n_modes) <= tol).all()
        np.testing.assert_allclose(b['n_modes_power'], a.n_modes_power, rtol=R.SUMS_BAR, atol=0)
        np.testing.assert_allclose(b['power'], a.power, rtol=2*R.SUMS_BAR, atol=0)
        for i in range(len(MEASURE_BINS)):
            if a.n_modes[i] == 0:
                assert math.isnan(b['bpower'][i]) and math.isnan(b['bpower_reduced'][i])
                continue
            # the sum bar on the unnormalised sum, in the units of B
            tol = R.SUMS_BAR*scales[tag][i]*ρ_bar**-3*0.5*BOXSIZE**6/N**3/a.n_modes[i]
            print(tag, i, abs(b['bpower'][i] - a.bpower[i])/tol*R.SUMS_BAR)
            assert abs(b['bpower'][i] - a.bpower[i]) <= tol


def triangles(N, shells):
    """closed triangles k₁ + k₂ + k₃ ≡ 0 (mod N) of modes off the Nyquist planes, kᵢ in shell i,
    by brute force; every triangle and its mirror image count once together"""
    nyq = N//2
    k = np.arange(-(nyq - 1), nyq)
    K = np.stack(np.meshgrid(k, k, k, indexing='ij'), -1).reshape(-1, 3)
    k2 = (K**2).sum(axis=1)
    sets = [K[(s[0]**2 < k2) & (k2 <= s[1]**2)] for s in shells]
    third = {tuple(v) for v in sets[2] % N}
    count = 0
    for v in ((sets[0][:, None, :] + sets[1][None, :, :]).reshape(-1, 3)*-1) % N:
        count += tuple(v) in third
    return count/2


def test_mode_counts_without_antialiasing_are_triangle_counts():
    analysis = setup()
    N = 8
    bins = [((0.5, 1.5), (1.5, 2.5), (2.25, 3.0)), ((0.5, 1.5), (0.5, 1.5), (0.5, 1.5)),
            ((1.5, 2.5), (1.5, 2.5), (2.25, 3.5)), ((1.1, 1.3), (0.5, 1.5), (1.5, 2.5)),
            ((2.5, 3.5), (2.5, 3.5), (2.5, 3.5))]
    for shells in bins:
        value, _ = analysis.compute_bispec_value(N, shells, None, antialiasing=False)
        n_modes = value*0.5/N**3
        assert abs(n_modes - round(n_modes)) < 1e-9
        assert round(n_modes) == triangles(N, shells), shells
    analysis.bispec_grid_cache.clear()


def test_three_plane_waves_give_the_known_bispectrum():
    """δ(x) = 1 + Σᵢ Aᵢ cos(2π kᵢ·x/N + φᵢ) with k₁ + k₂ + k₃ = 0 and three different |kᵢ|.
    The slab (the transform of δ/N³) holds Aᵢ/2 e^{±iφᵢ} at ±kᵢ, so a shell without
    antialiasing that holds |kᵢ| alone of the three filters out gᵢ(x) = Aᵢ cos(2π kᵢ·x/N +
    φᵢ).  Of the eight sign combinations in the product of the three cosines only
    ±(k₁ + k₂ + k₃) = 0 survives the sum over the cells:
        Σ g₁g₂g₃ = N³ A₁A₂A₃ cos(φ₁ + φ₂ + φ₃)/4.
    The reference's normalisation (analysis.py:3097-3123) multiplies by ρ̄⁻³·½L⁶/N³/n_modes
    with ρ̄ = 1 the mean of the field and n_modes half the number of closed triangles in the
    shells:  B = A₁A₂A₃ cos(φ₁ + φ₂ + φ₃) L⁶/(8 n_modes).  With a k₃ that does not close the
    triangle no combination survives and the sum is 0 to rounding."""
    analysis = setup()
    N, L = 16, BOXSIZE
    ks = np.array([(1, 2, 0), (2, -1, 3), (-3, -1, -3)])
    A, φ = np.array([0.3, 0.2, 0.25]), np.array([0.4, 1.1, -0.7])
    shells = [(math.sqrt(k @ k) - 0.1, math.sqrt(k @ k) + 0.1) for k in ks]
    x = np.stack(np.meshgrid(*(np.arange(N),)*3, indexing='ij'), -1)

    def field(kvecs):
        return 1.0 + sum(a*np.cos(2*math.pi*(x @ k)/N + p) for a, k, p in zip(A, kvecs, φ))
    expected = N**3*A.prod()*math.cos(φ.sum())/4
    slab = analysis._mesh(N, 'bispec')
    for kvecs, want in ((ks, expected), (np.array([ks[0], ks[1], (-3, -1, 3)]), 0.0)):
        # the restatement on the CPU first
        F = np.fft.rfftn(field(kvecs)*float(N)**-3)
        scale = {}
        value = R.bispec_value(N, shells, None, F, False, scale)
        assert scale['abs'] > 0.1*N**3*A.prod()/4
        assert abs(value - want) <= R.SUMS_BAR*scale['abs']
        load_fourier(slab, field(kvecs))
        analysis.bispec_grid_cache.clear()
        value = analysis.compute_bispec_value(N, shells, None, slab, antialiasing=False)
        assert abs(value - want) <= R.SUMS_BAR*scale['abs'], (value, want)
    analysis.bispec_grid_cache.clear()
    count, _ = analysis.compute_bispec_value(N, shells, None, antialiasing=False)
    n_modes = count*0.5/N**3
    assert round(n_modes) == triangles(N, shells) > 0
    B, _, _ = R.normalise(N, L, 1.0, [expected], [n_modes], np.ones((3, 1)), np.ones((3, 1)))
    assert B[0] == pytest.approx(A.prod()*math.cos(φ.sum())*L**6/(8*n_modes), rel=1e-12)
    analysis.bispec_grid_cache.clear()
