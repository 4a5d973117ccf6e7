"""The device algorithm of the primordial noise (csrc/cg_noise.hip), restated in tests/noise_refs.py,
against numpy itself on the host: the raw words through the jump-ahead table, the ziggurat in
trips with its carries, the committed tables, and the whole slab against
ic.generate_primordial_noise.  numpy computes both sides (the C library's exp and log1p under the
ziggurat on both), so they can be, and have to be, equal to the bit."""
import numpy as np
import pytest

import noise_refs
from concept_amd import commons, ic

# seeds found by search: with T = 64 each meets both carry cases within its first 38 trips (a pair
# of slow words across a trip boundary is one boundary in some thousands)
SEEDS = (43, 170, 320)
T = 64


def stream(seed):
    state = np.random.PCG64DXSM(seed).state['state']
    return state['state'], state['inc']


@pytest.mark.parametrize('seed', SEEDS)
def test_the_jump_ahead_table_gives_the_stream_s_raw_words(seed):
    bit_generator = np.random.PCG64DXSM(seed)
    words = bit_generator.random_raw(3*T + 5)
    state, inc = stream(seed)
    jump = ic.pcg64dxsm_jump_table(T)
    assert jump.shape == (T + 1, 4) and jump.dtype == np.uint64
    got = []
    for _ in range(4):
        got += [noise_refs.dxsm(noise_refs.jumped(state, inc, jump[p])) for p in range(T)]
        state = noise_refs.jumped(state, inc, jump[T])
    assert got[:len(words)] == words.tolist()


@pytest.mark.parametrize('seed', SEEDS)
def test_rayleigh_and_uniform_bit_for_bit(seed):
    """n from less than a trip to many; every seed has to meet both carry cases"""
    state, inc = stream(seed)
    stats = {}
    n_max = 38*T
    E = noise_refs.exponentials(state, inc, n_max, T, stats=stats)
    print(seed, stats)
    assert stats.get('second word in next trip', 0) >= 1
    assert stats.get('slow run across trips', 0) >= 1
    for n in (1, T - 1, T, T + 1, 3*T, n_max):
        ref = np.random.Generator(np.random.PCG64DXSM(seed)).rayleigh(1, n)
        assert np.array_equal(np.sqrt(2.0*E[:n]), ref), n
        if n != n_max:
            assert np.array_equal(noise_refs.exponentials(state, inc, n, T), E[:n]), n
        ref = np.random.Generator(np.random.PCG64DXSM(seed)).uniform(0, 1, n)
        assert np.array_equal(noise_refs.uniforms(state, inc, n, T), ref), n
    # the trip length does not matter
    assert np.array_equal(noise_refs.exponentials(state, inc, 700, 256), E[:700])
    assert np.array_equal(noise_refs.exponentials(state, inc, 700, 1024), E[:700])


def test_the_start_flags_from_masks():
    """start_flag against the recurrence, for masks with long runs of slow words and both flags
    of the first word"""
    rng = np.random.default_rng(4)
    masks = [0, noise_refs.MASK64, 1, 1 << 63, 3, 7 << 61, noise_refs.MASK64 >> 1,
             noise_refs.MASK64 ^ (1 << 31)]
    masks += [int(rng.integers(0, 2**63)) | int(rng.integers(0, 2)) << 63 for _ in range(50)]
    masks += [int(m) for m in (rng.random((50, 64)) < 0.9) @ (1 << np.arange(64, dtype=object))]
    for mask in masks:
        slow = [bool(mask >> lane & 1) for lane in range(64)]
        for s_in in (True, False):
            plain, s_next = noise_refs.start_flags_plain(slow, s_in)
            assert [noise_refs.start_flag(mask, lane, s_in) for lane in range(64)] == plain
            assert noise_refs.start_flag(mask, 64, s_in) == s_next


def test_the_committed_tables_are_the_installed_numpy_s():
    tool = noise_refs.numpy_ziggurat_tables
    if tool.missing_tools():
        pytest.skip(f'not installed: {", ".join(tool.missing_tools())}')
    try:
        extracted = tool.extract()
    except FileNotFoundError as e:
        pytest.skip(f'this numpy ships no libnpyrandom.a: {e}')
    assert tool.read_header(noise_refs.HEADER) == extracted


def params(**kw):
    return commons.load_params({'boxsize': 100.0, **kw})


@pytest.mark.parametrize('gridsize', [8, 12])
@pytest.mark.parametrize('kw', [
    {},
    {'primordial_phase_shift': 0.75},
    {'primordial_amplitude_fixed': True},
    {'primordial_amplitude_fixed': True, 'primordial_phase_shift': np.pi},
    {'random_seeds': {'primordial amplitudes': 77, 'primordial phases': 4242}},
], ids=['plain', 'shift', 'fixed', 'fixed-shift', 'seeds'])
def test_the_slab_is_the_host_s(gridsize, kw):
    p = params(**kw)
    fixed, shift = p.primordial_amplitude_fixed, p.primordial_phase_shift
    ref = ic.generate_primordial_noise(gridsize, fixed, shift, p)
    got = noise_refs.slab(gridsize, fixed, shift, p)
    assert np.array_equal(got, ref)
    assert np.abs(ref).max() > 0


def test_every_stream_is_made_once_and_fixed_amplitudes_make_none():
    p = params()
    g = 12
    table = ic.noise_stream_table(g, False, p)
    assert table.shape == (g - 1, 8) and table.dtype == np.uint64
    assert len({tuple(row[:4]) for row in table} | {tuple(row[4:]) for row in table}) == 2*(g - 1)
    fixed = ic.noise_stream_table(g, True, p)
    assert not fixed[:, :4].any() and np.array_equal(fixed[:, 4:], table[:, 4:])
    # the stream of key κ is the one the host spawns for the slice kj = κ
    for row, κ in ((0, -g//2 + 1), (g//2 - 1, 0), (g - 2, g//2 - 1)):
        state = ic.PseudoRandomNumberGenerator(p.random_seeds['primordial phases'],
                                               p.random_generator).spawn(2**32 + κ) \
            .generator.bit_generator.state['state']
        assert noise_refs.join128(table[row], 4) == state['state']
        assert noise_refs.join128(table[row], 6) == state['inc']
    order = ic.noise_order_table(g)
    assert order.shape == ((g - 1)*g//2, 2) and order.dtype == np.int32
    assert len({tuple(point) for point in order}) == len(order)


@pytest.mark.parametrize('kw, what', [
    ({'primordial_noise_imprinting': 'simple'}, '"simple" is not implemented'),
    ({'random_generator': 'PCG64'}, 'random_generator = "PCG64" is not implemented'),
    ({'random_generator': 'Philox'}, 'random_generator = "Philox" is not implemented'),
])
def test_the_stream_table_refuses_by_name(kw, what):
    from concept_amd.lib import ConceptGPUError
    with pytest.raises(ConceptGPUError, match=what):
        ic.noise_stream_table(8, False, params(**kw))
