"""CPU checks of the power spectrum's host layer (concept_amd.analysis): the parameters, the
selection into declarations, the bins and mode counts, σ and the file — against the reference's
own results (tests/golden/powerspec_*.npz, made by make_golden_powerspec.py) and brute force."""
import math
import os
import re
import types
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = ('powerspec_a_defaults', 'powerspec_b_cic', 'powerspec_c_multigrid', 'powerspec_d_fluid')


def golden(name):
    return np.load(os.path.join(HERE, 'golden', name + '.npz'))


def fake_components(g):
    """what the declarations read of a component"""
    out = []
    for name in g['component_names']:
        name = str(name)
        if f'{name}_N' in g:
            out.append(types.SimpleNamespace(name=name, species='matter',
                                             representation='particles', N=int(g[f'{name}_N'])))
        else:
            out.append(types.SimpleNamespace(name=name, species='matter', representation='fluid',
                                             gridsize=int(g[f'{name}_gridsize']), N=0))
    return out


def declarations_of(name):
    from concept_amd import analysis, commons
    g = golden(name)
    commons.load_params(str(g['param']))
    comps = fake_components(g)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return g, comps, analysis.get_powerspec_declarations(comps)


def brute_force_n_modes(N, k2_max):
    """fourier_loop(N, sparse=True, skip_origin=True, k2_max) (mesh.py:2748-2838) mode by mode"""
    nyq = N//2
    n = np.zeros(k2_max + 1, dtype=np.int64)
    ks = [k for k in range(-nyq + 1, nyq)]
    for ki in ks:
        for kj in ks:
            for kk in range(0, nyq):
                if kk == 0 and (ki > 0 or (ki == 0 and kj >= 0)):
                    continue
                k2 = ki*ki + kj*kj + kk*kk
                if k2 <= k2_max:
                    n[k2] += 1
    return n


@pytest.mark.parametrize('name', GOLDEN)
def test_bins_match_the_reference(name):
    g, comps, decls = declarations_of(name)
    assert len(decls) == int(g['n_declarations'])
    for i, d in enumerate(decls):
        assert [c.name for c in d.components] == [str(s) for s in g[f'd{i}_components']]
        assert d.gridsize == int(g[f'd{i}_gridsize'])
        assert d.k2_max == int(g[f'd{i}_k2_max'])
        assert d.interpolation == int(g[f'd{i}_interpolation'])
        assert str(d.interlace) == str(g[f'd{i}_interlace'])
        np.testing.assert_array_equal(d.k_bin_indices, g[f'd{i}_k_bin_indices'])
        np.testing.assert_array_equal(d.n_modes, g[f'd{i}_n_modes'])
        np.testing.assert_allclose(d.k_bin_centers, g[f'd{i}_k_bin_centers'], rtol=1e-12, atol=0)
        assert d.tophat == pytest.approx(float(g[f'd{i}_tophat']), rel=1e-14)
    from concept_amd import analysis
    for c in comps:
        assert analysis.upstream_gridsize(c) == int(g[f'{c.name}_upstream'])


@pytest.mark.parametrize('N', [16, 24])
def test_mode_counts_against_brute_force(N):
    from concept_amd import analysis
    for k2_max in (3*(N//2)**2, (N//2)**2, 7):
        np.testing.assert_array_equal(analysis.n_modes_per_k2(N, k2_max),
                                      brute_force_n_modes(N, k2_max))


@pytest.mark.parametrize('name', GOLDEN)
def test_sigma_from_golden_power(name):
    g, comps, decls = declarations_of(name)
    from concept_amd import analysis
    for i, d in enumerate(decls):
        d.power[:] = g[f'd{i}_power']
        σ = analysis.compute_powerspec_σ(d)
        assert σ == pytest.approx(float(g[f'd{i}_sigma']), rel=1e-12)


def test_option_parsing_and_defaults():
    from concept_amd import commons
    p = commons.load_params({})
    o = p.powerspec_options
    assert o['upstream gridsize'] == {'default': -1} and o['global gridsize'] == {'default': -1}
    assert o['interpolation'] == {'default': 4} and o['deconvolve'] == {'default': True}
    assert o['interlace'] == {'default': 'bcc'} and o['k_max'] == {'default': 'nyquist'}
    assert o['bins per decade'] == {'default': {'  4*k_min': 4, '100*k_min': 40}}
    assert o['significant figures'] == {'default': 8}
    h = 67/100   # H0 = 67 km/s/Mpc by default
    assert o['tophat']['default'] == pytest.approx(8/h, rel=1e-14)
    assert p.powerspec_select == {'default': {'data': True, 'corrected': False, 'linear': True,
                                              'plot': True}}
    assert p.output_bases['powerspec'] == 'powerspec' and p.powerspec_dir is None
    assert p.nghosts == 2
    p = commons.load_params({'enable_Hubble': False,
                             'powerspec_options': {'gridsize': 64, 'interlace': False,
                                                   'interpolation': 'cic',
                                                   'bins per decade': {'matter': 10}},
                             'powerspec_select': {'matter': {'da ta': True, 'linear-': False}},
                             'output_dirs': {'snapshot': '/s', 'powerspec': '/p'},
                             'output_times': {'a': {'powerspec': [0.5, 1], 'snapshot': 1}}})
    o = p.powerspec_options
    assert o['upstream gridsize']['default'] == 64 and o['global gridsize']['default'] == 64
    assert o['interlace']['default'] == 'sc' and o['interpolation']['default'] == 2
    assert o['bins per decade']['matter'] == {1: 10, 2: 10}
    assert o['tophat']['default'] == pytest.approx(8.0, rel=1e-14)   # h = 1 without Hubble
    assert p.powerspec_select['matter'] == {'data': True, 'linear': False, 'corrected': False,
                                            'plot': False}
    assert p.powerspec_select['default'] == {'data': False, 'corrected': False, 'linear': False,
                                             'plot': False}
    assert p.powerspec_dir == '/p' and p.output_dirs == {'snapshot': '/s', 'powerspec': '/p'}
    assert p.powerspec_times['a'] == (0.5, 1.0) and p.snapshot_times['a'] == (1.0,)
    # one directory for every output kind (commons.py:2547-2572)
    p = commons.load_params({'output_dirs': '/all'})
    assert p.output_dirs == {'snapshot': '/all'} and p.powerspec_dir == '/all'
    # CIC and odd interlacing raise nghosts as the reference does (commons.py:4412-4419)
    assert commons.load_params({'powerspec_options': {'interpolation': 'TSC'}}).nghosts == 2
    assert commons.load_params({'cell_centered': False}).nghosts == 3
    with pytest.raises(ValueError, match='not implemented'):
        commons.load_params({'powerspec_options': {'gridsizes': 32}})
    with pytest.raises(ValueError, match='Unknown selections'):
        commons.load_params({'powerspec_select': {'default': {'datta': True}}})


def test_selection_to_declarations_and_warnings():
    from concept_amd import analysis, commons
    commons.load_params({'boxsize': 100.0, 'powerspec_options': {'gridsize': 16}})
    comps = [types.SimpleNamespace(name=n, species='matter', representation='particles', N=512)
             for n in ('a', 'b')]
    analysis._unsupported_warned.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        decls = analysis.get_powerspec_declarations(comps)
    # the default selection: every component and every combination ('default' is a key of
    # both, commons.py:5506-5536); 'linear' and 'plot' warn once each
    assert [[c.name for c in d.components] for d in decls] == [['a'], ['b'], ['a', 'b']]
    msgs = [str(x.message) for x in w]
    assert sum('needs CLASS' in m for m in msgs) == 1
    assert sum('plots are not produced' in m for m in msgs) == 1
    commons.load_params({'boxsize': 100.0, 'powerspec_options': {'gridsize': 16},
                         'powerspec_select': {'b': True, ('a', 'b'): {'data': True}}})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        decls = analysis.get_powerspec_declarations(comps)
    assert [[c.name for c in d.components] for d in decls] == [['b'], ['a', 'b']]


def test_writer_round_trip(tmp_path):
    from concept_amd import analysis
    g, comps, decls = declarations_of('powerspec_c_multigrid')
    for i, d in enumerate(decls):
        d.power[:] = g[f'd{i}_power']
    fn = str(tmp_path/'powerspec_a=1.00')
    analysis.save_powerspec(decls, fn, a=1.0, t=13.0)
    cols = np.loadtxt(fn, unpack=True)
    # every declaration here has the same bins: one column group k, modes, P, P, P
    assert cols.shape[0] == 2 + len(decls)
    sf = 8
    np.testing.assert_allclose(cols[0], decls[0].k_bin_centers, rtol=10**(1 - sf))
    np.testing.assert_array_equal(cols[1], decls[0].n_modes)
    for i, d in enumerate(decls):
        np.testing.assert_allclose(cols[2 + i], d.power, rtol=10**(1 - sf))
    # test/powerspec/analyze.py:78-90 finds σ in the header
    text = open(fn, encoding='utf-8').read()
    tophat_Mpc_over_h = decls[0].tophat*0.7   # H0 = 70 km/s/Mpc: the subscript is in Mpc/h
    m = re.search('σ' + analysis.unicode_subscript(f'{tophat_Mpc_over_h:.2g}')
                  + r' = ([0-9\.e+-]*)', text)
    assert m and float(m.group(1)) == pytest.approx(analysis.compute_powerspec_σ(decls[0]),
                                                    rel=10**(1 - sf))
    assert 'a = 1' in text.splitlines()[0] and 't = 13' in text.splitlines()[0]
    # column groups of different bins: padded with NaN
    g2, comps2, decls2 = declarations_of('powerspec_b_cic')
    for i, d in enumerate(decls2):
        d.power[:] = g2[f'd{i}_power']
    mixed = [decls[0], decls2[0]]
    fn2 = str(tmp_path/'mixed')
    analysis.save_powerspec(mixed, fn2)
    cols = np.loadtxt(fn2, unpack=True)
    assert cols.shape == (6, max(len(decls[0].n_modes), len(decls2[0].n_modes)))
    short = min(mixed, key=lambda d: len(d.n_modes))
    j = 0 if short is decls[0] else 3
    assert np.isnan(cols[j, len(short.n_modes):]).all()
    assert not math.isnan(cols[j, len(short.n_modes) - 1])
