"""The bispectrum core without a GPU: the overlap header built with the host compiler against
the reference's golden, the NumPy restatement (tests/bispec_refs.py) against the value
goldens, the grid cache of compute_bispec_value on fake meshes, the normalisation and NaN
rules of bispec_measure, and what is refused or absent by design."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bispec_refs as R  # noqa: E402

CSRC = os.path.join(REPO, 'concept_amd', 'csrc')


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('bispec')/'bispec_overlap_main')
    subprocess.check_call([cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-Wall', '-I' + CSRC,
                           os.path.join(HERE, 'bispec_overlap_main.cpp'), '-o', exe])
    return exe


def test_header_includes_no_hip_runtime():
    text = open(os.path.join(CSRC, 'cg_bispec.h'), encoding='utf-8').read()
    includes = [line for line in text.splitlines() if line.startswith('#include')]
    assert includes == ['#include <math.h>', '#include <stdint.h>']


def test_overlap_header_on_the_host_matches_the_reference(host_program, golden, tmp_path):
    g = golden('bispec_overlap')
    cases, frac = g['cases'], g['frac']
    assert len(cases) > 3000
    near = R.near_guard(cases)
    print(f'{int(near.sum())} of {len(cases)} cases lie at an ϵ guard and are skipped')
    assert near.mean() <= 0.005
    path = tmp_path/'cases.txt'
    with open(path, 'w') as f:
        for ki, kj, kk, k_inner, k_outer in cases:
            f.write(f'{int(ki)} {int(kj)} {int(kk)} {float(k_inner)!r} {float(k_outer)!r}\n')
    out = np.array(subprocess.check_output([host_program, 'overlap', str(path)]).split(),
                   dtype=np.float64)
    assert out.shape == frac.shape
    dev = (np.abs(out - frac)/np.maximum(1, cases[:, 4]**3))[~near]
    print('largest scaled deviation of the host build:', dev.max())
    assert dev.max() <= R.OVERLAP_BAR_HOST
    # the leaves: cells on 0, 1, 2 and 3 coordinate planes are among the cases
    on_planes = (cases[:, :3] == 0).sum(axis=1)
    assert set(on_planes) == {0, 1, 2, 3}
    assert frac.min() == 0 and frac.max() == 1 and ((frac > 0) & (frac < 1)).sum() > 500


def test_overlap_restatement_matches_the_reference(golden):
    g = golden('bispec_overlap')
    cases, frac = g['cases'], g['frac']
    dev = np.abs(R.overlap_cellshell(*cases.T) - frac)/np.maximum(1, cases[:, 4]**3)
    assert dev.max() <= R.OVERLAP_BAR_HOST


@pytest.mark.parametrize('N, shell', [(8, (0.5, 1.5)), (8, (2.0, 3.5)), (12, (4.0, 5.5)),
                                      (12, (1.1, 1.3)), (40, (3.3, 6.1)), (40, (17.5, 19.5)),
                                      (40, (0.0, 0.7)), (40, (25.0, 40.0))])
def test_shell_rows_of_the_header_match_the_restatement(host_program, N, shell):
    out = np.array(subprocess.check_output(
        [host_program, 'rows', str(N), repr(float(shell[0])), repr(float(shell[1]))]).split(),
        dtype=np.int64).reshape(N, N, 3)
    visited, bgn, end = R.shell_rows(N, *shell)
    np.testing.assert_array_equal(out[..., 0].astype(bool), visited)
    np.testing.assert_array_equal(out[..., 1][visited], bgn[visited])
    np.testing.assert_array_equal(out[..., 2][visited], end[visited])
    nyq = N//2
    assert not visited[nyq].any() and not visited[:, nyq].any() and end[visited].max() < nyq


@pytest.mark.parametrize('N', [8, 12])
def test_restatement_matches_the_value_goldens(golden, N):
    g = golden(f'bispec_value_g{N}')
    F = R.from_slab(g['slab'])
    # the slab is the transform of the stored field
    np.testing.assert_allclose(np.fft.rfftn(g['field']*float(N)**-3), F, atol=1e-15)
    worst = 0
    for antialiasing, tag in ((True, 'aa'), (False, 'noaa')):
        power, power_ind = {}, {}
        for b, shells in enumerate(g['bins']):
            shells = tuple(tuple(s) for s in shells)
            scale = {}
            value, new = R.bispec_value(N, shells, power_ind, None, antialiasing, scale)
            assert len(new) == g[f'{tag}_indicator_new'][b]
            ref = g[f'{tag}_indicator_value'][b]
            if scale['abs'] == 0:
                assert value == ref == 0    # the empty shell
            else:
                worst = max(worst, abs(value - ref)/scale['abs'])
            scale = {}
            value = R.bispec_value(N, shells, power, F, antialiasing, scale)
            ref = g[f'{tag}_data_value'][b]
            if scale['abs'] == 0:
                assert value == ref == 0
            else:
                worst = max(worst, abs(value - ref)/scale['abs'])
        assert [list(k) for k in power] == g[f'{tag}_power_shells'].tolist()
        for got, ref in ((power, g[f'{tag}_data_power']),
                         (power_ind, g[f'{tag}_indicator_power'])):
            for value, r in zip(got.values(), ref):
                if r == 0:
                    assert value == 0
                else:
                    worst = max(worst, abs(value - r)/r)
    print('largest deviation of the restatement:', worst)
    assert worst <= R.SUMS_DEV_RESTATEMENT
    # without antialiasing an indicator sum is 2 N³ x a whole number of triangles
    counts = g['noaa_indicator_value']*0.5/N**3
    np.testing.assert_allclose(counts, np.rint(counts), atol=1e-9)
    assert counts.max() > 100


# -- the grid cache ------------------------------------------------------------------------------
class FakeGrid:
    def __init__(self, shell, n, is_indicator):
        self.shell, self.n, self.is_indicator = shell, n, is_indicator


@pytest.fixture
def fake_analysis(monkeypatch):
    from concept_amd import analysis, commons
    commons.load_params({'boxsize': 100.0})
    built, summed = [], []

    def get_bispec_grid(gridsize, shell, n, slab_data, antialiasing):
        built.append((shell, n))
        return FakeGrid(shell, n, slab_data is None)

    def sums(grids, power_mask):
        summed.append(([g.shell for g in grids], [g.n for g in grids], power_mask))
        return [float(len(grids)), 10.0, 20.0, 30.0]
    monkeypatch.setattr(analysis, 'get_bispec_grid', get_bispec_grid)
    monkeypatch.setattr(analysis, '_bispec_sums', sums)
    analysis.bispec_grid_cache.clear()
    yield analysis, built, summed
    analysis.bispec_grid_cache.clear()


def test_grid_cache_of_compute_bispec_value(fake_analysis):
    analysis, built, summed = fake_analysis
    A, B, C, D = (0.5, 1.5), (1.5, 2.5), (2.5, 3.5), (3.5, 4.5)
    power = {}
    # three new grids in buffers 0, 1, 2
    value, new = analysis.compute_bispec_value(16, (A, B, C), power)
    assert built == [(A, 0), (B, 1), (C, 2)] and value == 3.0 and new == [A, B, C]
    assert summed[-1] == ([A, B, C], [0, 1, 2], 0b111)
    assert power == {A: 10.0, B: 20.0, C: 30.0}
    # (A, B, B): both from the cache; the grid that counts twice is grid 1
    del built[:]
    value, new = analysis.compute_bispec_value(16, (B, A, B), power)
    assert built == [] and new == [] and summed[-1] == ([A, B], [0, 1], 0)
    # the other multiplicity order: A counts twice and goes last
    analysis.compute_bispec_value(16, (A, A, B), power)
    assert built == [] and summed[-1] == ([B, A], [1, 0], 0)
    # C left the cache with the previous calls: it is rebuilt, in the free buffer; cached
    # grids come first
    analysis.compute_bispec_value(16, (C, B, B), power)
    assert built == [(C, 0)] and summed[-1] == ([C, B], [0, 1], 0)
    # a new shell takes the buffer no cached grid holds
    del built[:]
    value, new = analysis.compute_bispec_value(16, (D, D, D), power)
    assert built == [(D, 0)] and new == [D] and summed[-1] == ([D], [0], 1) and power[D] == 10.0
    analysis.compute_bispec_value(16, (B, D, C), power)
    assert built == [(D, 0), (B, 1), (C, 2)] and summed[-1] == ([D, B, C], [0, 1, 2], 0)
    # a data grid is not an indicator grid, another grid size is another grid
    del built[:]
    assert analysis.compute_bispec_value(16, (D, B, C), None, slab_data=object()) == 3.0
    assert [n for _, n in built] == [0, 1, 2] and summed[-1][2] == 0
    del built[:]
    analysis.compute_bispec_value(32, (D, B, C), None, slab_data=object())
    assert len(built) == 3
    # the other setting of the antialiasing empties the cache
    del built[:]
    analysis.compute_bispec_value(32, (D, B, C), None, slab_data=object(), antialiasing=False)
    assert len(built) == 3
    with pytest.raises(analysis.ConceptGPUError, match='2 shells'):
        analysis.compute_bispec_value(16, (A, B), None)


def test_bispec_antialiasing_parameter():
    from concept_amd import analysis, commons
    assert commons.load_params({'boxsize': 1.0}).bispec_antialiasing is True
    assert analysis._bispec_antialiasing(None) is True
    p = commons.load_params('boxsize = 1.0\nbispec_antialiasing = False\n'
                            "bispec_options = {'gridsize': 64}\n"
                            "bispec_select = {'all': True}\n")
    assert p.bispec_antialiasing is False and analysis._bispec_antialiasing(None) is False
    assert analysis._bispec_antialiasing(True) is True
    assert not hasattr(p, 'bispec_options') and not hasattr(p, 'bispec_select')


class FakeComponent:
    representation, name, species = 'particles', 'matter', 'matter'
    N, ϱ_bar = 8**3, 2.5

    def w_eff(self, a=1.0):
        return 0.0


def test_normalisation_and_nan_rules_of_bispec_measure(monkeypatch):
    from concept_amd import analysis, commons
    commons.load_params({'boxsize': 50.0})
    A, B, E = (0.5, 1.5), (1.5, 2.5), (1.1, 1.3)
    modes = {A: 18.0, B: 62.0, E: 0.0}
    N, a = 16, 0.5

    def value(gridsize, shells, power_dict, slab_data=None, *, antialiasing=None):
        assert antialiasing is True and gridsize == N
        shells = [tuple(s) for s in shells]
        for s in shells:
            if power_dict is not None and s not in power_dict:
                power_dict[s] = modes[s]*(2*N**3 if slab_data is None else 3.0)
        if slab_data is None:
            return (0.0 if E in shells else 7.0*2*N**3), []
        return 11.0
    monkeypatch.setattr(analysis, 'compute_bispec_value', value)
    monkeypatch.setattr(analysis, 'interpolate_upstream', lambda *args, **kw: object())
    comp = FakeComponent()
    assert analysis.upstream_gridsize(comp, 'bispec') == 16
    res = analysis.bispec_measure([comp], [(A, B, B), (A, E, B), (E, E, E)], N, a=a)
    np.testing.assert_array_equal(res.n_modes, [7.0, 0.0, 0.0])
    np.testing.assert_array_equal(res.n_modes_power, [[18, 18, 0], [62, 0, 0], [62, 62, 0]])
    ρ_bar = a**-3*2.5
    B_ref = 11.0*ρ_bar**-3*0.5*50.0**6/N**3/7.0
    P = {s: 3.0*modes[s]*ρ_bar**-2*0.5*50.0**3/N**3/modes[s] for s in (A, B)}
    assert res.bpower[0] == pytest.approx(B_ref, rel=1e-14)
    assert np.isnan(res.bpower[1:]).all()
    np.testing.assert_allclose(res.power[:, 0], [P[A], P[B], P[B]], rtol=1e-14)
    assert np.isnan(res.power[1, 1]) and np.isnan(res.power[:, 2]).all()
    assert res.power[0, 1] == pytest.approx(P[A]) and res.power[2, 1] == pytest.approx(P[B])
    assert res.bpower_reduced[0] == pytest.approx(
        B_ref/(P[A]*P[B] + P[B]*P[B] + P[B]*P[A]), rel=1e-14)
    assert np.isnan(res.bpower_reduced[1:]).all()
    got, power, reduced = R.normalise(N, 50.0, ρ_bar, [11.0]*3, res.n_modes,
                                      3.0*res.n_modes_power, res.n_modes_power)
    np.testing.assert_allclose(got, res.bpower, rtol=1e-14)
    np.testing.assert_allclose(power, res.power, rtol=1e-14)
    np.testing.assert_allclose(reduced, res.bpower_reduced, rtol=1e-14)
    res = analysis.bispec_measure([comp], [(A, B, B)], N, a=a, do_reduced=False)
    assert res.bpower[0] == pytest.approx(B_ref, rel=1e-14)
    assert np.isnan(res.power).all() and np.isnan(res.bpower_reduced).all()


def test_what_is_not_built_is_absent_by_name():
    from concept_amd import analysis, commons, stepper
    for name in ('parse_bispec_configuration', 'get_bispec_shell_boundary', 'get_bispec_bins',
                 'get_bispec_declarations', 'get_bispec_computation_order', 'save_bispec',
                 'compute_bispec_treelevel', 'plot_bispec', 'bispec'):
        assert not hasattr(analysis, name), name
    p = commons.load_params({'boxsize': 1.0, 'output_times': {'a': {'bispec': (1.0,)}}})
    assert not hasattr(p, 'bispec_times') and 'bispec' not in p.output_bases
    assert 'bispec' not in open(stepper.__file__, encoding='utf-8').read()
