"""Host logic of the rung loop (no GPU): the step integrals worked out when read and the
ᔑdt_rungs arrays filled in when read (stepper._LazyIntegrals, _RungIntegrals) give what the
eager forms give (get_time_step_integrals, main.py:998-1073; the arrays of main.py:1480-1552);
the integrals' cache; bench.py's link model; the on_dump callbacks of the three dumpers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lazy_integrals_equal_the_eager_ones():
    from concept_amd import stepper
    keys = ['1', 'a**2', 'a**(-2)', ('a**(-3*w_eff)', 'matter'), ('pair', 'matter', 'matter')]
    calls = []

    def one(key, t0, t1):
        calls.append(key)
        return (hash(key) % 97 + 1)*(t1 - t0)
    eager = {k: one(k, 0.25, 0.75) for k in keys}
    calls.clear()
    lazy = stepper._LazyIntegrals(one, keys, 0.25, 0.75)
    assert calls == [] and len(lazy) == len(keys) and list(lazy) == keys and '1' in lazy
    assert 'b' not in lazy and lazy.get('b', 7) == 7
    assert lazy['a**2'] == eager['a**2'] and calls == ['a**2']
    assert lazy['a**2'] == eager['a**2'] and calls == ['a**2']          # worked out once
    assert dict(lazy.items()) == eager and sorted(map(str, lazy.keys())) == sorted(map(str, keys))
    try:
        lazy['b']
    except KeyError:
        pass
    else:
        raise AssertionError('an integrand outside the run\'s keys must raise')


def test_rung_integral_arrays_fill_in_when_read():
    from concept_amd import stepper
    keys = ['1', 'a**2']
    one = lambda key, t0, t1: (2.0 if key == '1' else 3.0)*(t1 - t0)   # noqa: E731
    nr = 4
    eager = {k: np.zeros(3*nr - 1) for k in keys}
    R = stepper._RungIntegrals(3*nr - 1)
    script = [(0, 0.0, 1.0), (nr, None, None), (2*nr, 0.0, 0.5), (1, 0.5, 1.0), (0, 0.25, 0.5),
              (nr + 1, 0.0, 0.125), (nr, None, None)]
    for index, t0, t1 in script:
        if t0 is None:
            R.set(-1, index)
            for arr in eager.values():
                arr[index] = -1
        else:
            R.set(stepper._LazyIntegrals(one, keys, t0, t1), index)
            for k, arr in eager.items():
                arr[index] = one(k, t0, t1)
        if index == 1:
            assert np.array_equal(R['1'], eager['1'])       # read in between: later sets still land
    for k in keys:
        assert k in R and np.array_equal(R[k], eager[k]) and np.array_equal(R.get(k), eager[k])
    assert 'x' not in R and R.get('x') is None
    # a plain dictionary of numbers (what a caller's own integrals give) works the same
    R2 = stepper._RungIntegrals(5)
    R2.set({'1': 0.5, 'a**2': 0.25}, 3)
    assert R2['1'][3] == 0.5 and R2['a**2'][3] == 0.25 and set(R2.keys()) == {'1', 'a**2'}
    assert all(a.shape == (5,) for a in R2.values())


def test_integrals_cache_prefetch():
    from concept_amd import stepper
    n = []

    def f(t0, t1):
        n.append((t0, t1))
        return {'1': t1 - t0}
    c = stepper._CachedIntegrals(f)
    assert c(0.0, 1.0) == {'1': 1.0} and len(n) == 1
    c.prefetch(1.0, 2.0)
    c.prefetch(1.0, 2.0)
    assert len(n) == 2
    assert c(1.0, 2.0) == {'1': 1.0} and len(n) == 2      # from the cache
    assert c(2.0, 3.0) == {'1': 1.0} and len(n) == 3


def _dump_loop(stepper, components=()):
    """a Timeloop as far as the dumpers look at it: begins at a = 0.1, t = 0.5; the dump times
    need four digits to differ (0.1251 / 0.1254)"""
    import types
    loop = object.__new__(stepper.Timeloop)
    loop.cosmo = types.SimpleNamespace(a=0.1, t=0.5)
    loop.components = list(components)
    loop.params = types.SimpleNamespace(
        output_times={'a': (0.1251, 0.1254, 0.5), 't': (13.5,)},
        snapshot_times={'a': (0.1254,), 't': (13.5,)},
        powerspec_times={'a': (0.1251, 0.5), 't': ()},
        render2D_times={'a': (0.5,), 't': (13.5,)})
    assert loop._dump_ndigits() == 4
    dumps = [stepper.DumpTime('a', t=1.0, a=0.1251), stepper.DumpTime('a', t=1.1, a=0.1254),
             stepper.DumpTime('a', t=9.0, a=0.5*(1 + 5e-13)), stepper.DumpTime('t', t=13.5, a=0.9)]
    return loop, dumps


def test_dumpers_name_match_and_record(monkeypatch):
    """snapshot_dumper, powerspec_dumper and render2D_dumper: the names <dir>/<base>_<a|t>=
    <value> with the digits of _dump_ndigits, dump times outside their list skipped (matched to
    1e-12), the *_written lists filled."""
    import types
    from concept_amd import analysis, render, snapshot, stepper
    calls = []
    monkeypatch.setattr(snapshot, 'save', lambda components, name, **kw: (
        calls.append(('snapshot', [c.name for c in components], name, kw)), name + '.0')[1])
    monkeypatch.setattr(analysis, 'powerspec', lambda components, name, **kw: calls.append(
        ('powerspec', [c.name for c in components], name, kw)))
    monkeypatch.setattr(render, 'render2D', lambda components, name, **kw: (
        calls.append(('render2D', [c.name for c in components], name, kw)),
        (None, [name + '.png', name + '.hdf5']))[1])
    matter = types.SimpleNamespace(name='matter', representation='particles')
    gas = types.SimpleNamespace(name='gas', representation='fluid')
    loop, dumps = _dump_loop(stepper, [matter, gas])

    def run(dumper):
        calls.clear()
        for dump_time in dumps:
            dumper(loop, dump_time)
        return list(calls)
    # power spectra: at a = 0.1251 and 0.5 (the latter matched within 1e-12), not at 0.1254, t
    assert run(loop.powerspec_dumper('out/dir')) == [
        ('powerspec', ['matter', 'gas'], 'out/dir/powerspec_a=0.1251', {'a': 0.1, 't': 0.5}),
        ('powerspec', ['matter', 'gas'], 'out/dir/powerspec_a=0.5000', {'a': 0.1, 't': 0.5})]
    assert loop.powerspecs_written == ['out/dir/powerspec_a=0.1251', 'out/dir/powerspec_a=0.5000']
    # renders: at a = 0.5 and t = 13.5; the stream is handed on; an empty base drops the '_'
    assert run(loop.render2D_dumper('r', '', stream='tty')) == [
        ('render2D', ['matter', 'gas'], 'r/a=0.5000', {'a': 0.1, 't': 0.5, 'stream': 'tty'}),
        ('render2D', ['matter', 'gas'], 'r/t=13.5000', {'a': 0.1, 't': 0.5, 'stream': 'tty'})]
    assert loop.renders2D_written == ['r/a=0.5000.png', 'r/a=0.5000.hdf5', 'r/t=13.5000.png',
                                      'r/t=13.5000.hdf5']
    # snapshots: every dump unless only_snapshot_times; particle components only, one warning
    with pytest.warns(UserWarning, match='GADGET snapshots hold particle components only: gas'):
        got = run(loop.snapshot_dumper('s', 'snap', snapformat=2))
    kw = {'a': 0.1, 'output_base': 'snap', 'snapformat': 2}
    assert got == [('snapshot', ['matter'], f's/snap_{stamp}', kw)
                   for stamp in ('a=0.1251', 'a=0.1254', 'a=0.5000', 't=13.5000')]
    assert loop.snapshots_written == [f's/snap_{stamp}.0' for stamp in (
        'a=0.1251', 'a=0.1254', 'a=0.5000', 't=13.5000')]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')   # (warned once per loop)
        got = run(loop.snapshot_dumper('s', '', only_snapshot_times=True))
    kw = {'a': 0.1, 'output_base': 'snapshot'}
    assert got == [('snapshot', ['matter'], 's/a=0.1254', kw),
                   ('snapshot', ['matter'], 's/t=13.5000', kw)]
    assert loop.snapshots_written == ['s/a=0.1254.0', 's/t=13.5000.0']
    # nothing but fluids: nothing written
    loop.components = [gas]
    assert run(loop.snapshot_dumper('s')) == [] and loop.snapshots_written == []


def test_link_model_prediction():
    """bench.py --link-model: the prediction a first SCALE run is compared with;
    one xGMI link per peer bounds the two transposes of a step."""
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--link-model'],
                         stdout=subprocess.PIPE, check=True, timeout=300).stdout.decode()
    d = json.loads(out)
    assert d['particles'] == 2**28 and d['gridsize'] == 1024
    rows = d['by_gpus']
    assert set(rows) == {'1', '2', '4', '8'}
    assert rows['1']['transpose_ms_at_link_rate'] == 0 and rows['1']['predicted_speedup'] == 1
    for P in (2, 4, 8):
        r = rows[str(P)]
        per_peer = 1024*1024*1026*8/P/P
        assert abs(r['bytes_per_peer_per_transpose'] - per_peer) <= 8
        assert abs(r['transpose_ms_at_link_rate'] - per_peer/76.8e9*1e3) < 1e-2
        assert r['predicted_step_ms'] >= 2*r['transpose_ms_at_link_rate']
    assert rows['8']['predicted_speedup'] > rows['4']['predicted_speedup'] > rows['2']['predicted_speedup']
    committed = json.load(open(os.path.join(REPO, 'profiles', 'r06_link_model_ns.json')))
    assert committed['by_gpus'] == rows
