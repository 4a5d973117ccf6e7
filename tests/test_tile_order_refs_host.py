"""CPU tests of tests/tile_order_refs.py: the checker of the heavy-tile list accepts a correct
list and rejects each way a list can be wrong; the integer arithmetic of the threshold, the
class unit and the list's capacity at hand-computed values; the four population shapes of
test_gpu_tile_order.py have their defining properties on every grid that file runs, and the
particles made for them land in the tiles (and buckets) they were made for."""
import numpy as np
import pytest

import tile_order_refs as R

FLOOR = 6
# (gridsize, tile extent) of test_gpu_tile_order.py
GRIDS = [(160, 16), (72, 8), (36, 4), (18, 2), (80, 16), (40, 8), (20, 4)]


def _pops():
    """64 tiles (cap 8) of 2 particles, 5 heavy ones in classes 10, 10, 5, 4, 3: total 185,
    thr 6, unit 2"""
    pops = np.full(64, 2, dtype=np.int64)
    pops[[3, 40, 17, 9, 60]] = [20, 21, 10, 9, 7]
    return pops


def test_the_example_is_what_its_docstring_says():
    o = R.order_numbers(_pops(), FLOOR)
    assert (o.total, o.thr, o.unit, o.cap) == (185, 6, 2, 8)
    assert list(np.flatnonzero(o.heavy)) == [3, 9, 17, 40, 60]
    assert list(o.cls[[3, 40, 17, 9, 60]]) == [10, 10, 5, 4, 3]


def _good(pops):
    o = R.order_numbers(pops, FLOOR)
    heavy = np.flatnonzero(o.heavy)
    return heavy[np.argsort(-o.cls[heavy], kind='stable')][:o.cap]


def test_checker_accepts_a_correct_list():
    pops = _pops()
    good = _good(pops)
    R.check_list(good, pops, FLOOR)
    # the order inside a class is free: tiles 3 and 40 are both of class 10
    swapped = good.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert R.order_numbers(pops, FLOOR).cls[good[0]] == R.order_numbers(pops, FLOOR).cls[good[1]]
    R.check_list(swapped, pops, FLOOR)
    R.check_list(swapped.astype(np.uint32), pops, FLOOR)
    # nobody heavy: the empty list
    R.check_list(np.empty(0, dtype=np.uint32), np.full(64, 3), FLOOR)


@pytest.mark.parametrize('what', ['duplicate', 'not heavy', 'top class missing', 'rising',
                                  'too short', 'too long'])
def test_checker_rejects(what):
    pops = _pops()
    good = _good(pops)
    o = R.order_numbers(pops, FLOOR)
    if what == 'duplicate':
        bad = good.copy()
        bad[-1] = bad[-2]                 # (same length, still falling)
    elif what == 'not heavy':
        bad = good.copy()
        bad[-1] = 0                       # tile 0 holds 2 particles
        assert not o.heavy[0]
    elif what == 'top class missing':
        # the right length, falling, no duplicate, all heavy — but a tile of the top class gave
        # its place to one more tile of the lowest: only on an overflowing list
        pops = pops.copy()
        pops[10:20] = 7                   # 10 more heavy tiles of the lowest class: 15 > cap 8
        o = R.order_numbers(pops, FLOOR)
        assert o.thr == 6 and o.heavy.sum() > o.cap
        good = _good(pops)
        R.check_list(good, pops, FLOOR)
        left_out = np.setdiff1d(np.flatnonzero(o.heavy), good)
        assert o.cls[left_out[0]] == o.cls[good[-1]] < o.cls[good[0]]
        bad = np.concatenate([good[1:], left_out[:1]])
    elif what == 'rising':
        bad = good[::-1]
    elif what == 'too short':
        bad = good[:-1]
    else:
        pops = pops.copy()
        pops[10:20] = 7                   # 15 heavy tiles, cap 8
        o = R.order_numbers(pops, FLOOR)
        good = _good(pops)
        left_out = np.setdiff1d(np.flatnonzero(o.heavy), good)
        bad = np.concatenate([good, left_out[:1]])   # heavy, falling, no duplicate: 9 > cap
        assert bad.size == o.cap + 1 and o.cls[left_out[0]] == o.cls[good[-1]]
    with pytest.raises(AssertionError):
        R.check_list(bad, pops, FLOOR)


def test_overflowing_list_may_leave_out_tiles_of_its_last_class_only():
    pops = _pops().copy()
    pops[10:20] = 7
    o = R.order_numbers(pops, FLOOR)
    good = _good(pops)
    assert good.size == o.cap == 8
    # any tile of the last class may stand in for another one of it
    left_out = np.setdiff1d(np.flatnonzero(o.heavy), good)
    other = good.copy()
    other[-1] = left_out[-1]
    R.check_list(other, pops, FLOOR)


def test_threshold_unit_and_cap_by_hand():
    # 1000 tiles, 4321 particles: 3*4321//2000 = 6 -> the floor and the mean agree; unit 2
    pops = np.zeros(1000, dtype=np.int64)
    pops[0], pops[1], pops[2], pops[3] = 4000, 300, 14, 7
    o = R.order_numbers(pops, 6)
    assert (o.total, o.thr, o.unit, o.cap) == (4321, 6, 2, 128)
    assert list(o.cls[:4]) == [63, 63, 7, 3] and list(o.heavy[:4]) == [True]*4
    assert 4000//2 >= 64 and 126//2 == 63 and 128//2 == 64      # class 63 is where it saturates
    # the mean above the floor: 3*20000//2000 = 30, unit 10; 30 itself is not heavy, 31 is
    pops = np.full(1000, 20, dtype=np.int64)
    pops[5], pops[6] = 30, 31
    pops[7] -= 21
    o = R.order_numbers(pops, 6)
    assert (o.total, o.thr, o.unit) == (20000, 30, 10)
    assert not o.heavy[5] and o.heavy[6] and o.cls[6] == 3 and o.heavy.sum() == 1
    # a threshold below 3: the unit stays 1
    o = R.order_numbers(np.array([0, 0, 0, 0, 0, 0, 0, 3]), 1)
    assert (o.thr, o.unit, o.cap) == (1, 1, 8) and o.cls[7] == 3 and o.heavy[7]
    # the floor of a production box against a clustered one: 4096 tiles of 512 on average
    pops = np.full(4096, 512, dtype=np.int64)
    o = R.order_numbers(pops, 1536)
    assert (o.thr, o.unit, o.cap) == (1536, 512, 512) and not o.heavy.any()
    # cap: an eighth of the tiles, up to a multiple of 8
    for ntiles, cap in ((8, 8), (64, 8), (125, 16), (729, 96), (1000, 128), (1331, 168),
                        (4096, 512)):
        assert R.order_numbers(np.zeros(ntiles), 6).cap == cap


def test_front_by_hand():
    assert R.expected_front(None, 128) == 128                   # no build seen yet
    assert R.expected_front(0, 128) == 0                        # the plain launch
    assert R.expected_front(8, 128) == 80                       # 8 + 2 + 64 = 74 -> 80
    assert R.expected_front(8, 96) == 80
    assert R.expected_front(8, 16) == 16
    assert R.expected_front(50, 128) == 128                     # 50 + 12 + 64 = 126 -> 128
    assert R.expected_front(51, 128) == 128 and R.expected_front(128, 128) == 128
    assert R.expected_front(1, 128) == 72                       # the shortest front there is


@pytest.mark.parametrize('N,T', GRIDS)
def test_shapes_and_their_particles(N, T):
    box = R.Box(N, T, 100.0)
    seen_buckets = set()
    for s, shape in enumerate(R.SHAPES):
        rng = np.random.default_rng(100*N + s)
        pops = R.shape_pops(shape, box.ntiles, FLOOR, rng)
        R.shape_check(shape, pops, FLOOR)
        pos = box.particles(pops, rng)
        assert np.array_equal(box.pops(pos), pops)
        keys = box.keys(pos)
        seen_buckets |= set(np.unique(keys % 8))
        # the tables hold every particle once, in the region of its key
        perm, start = R.dense_table(box, pos)
        assert np.array_equal(np.diff(start), np.bincount(keys, minlength=8*box.ntiles))
        assert (np.diff(keys[perm]) >= 0).all()
        assert np.array_equal(R.table_pops(start), pops)
        slot, rstart, count, rows = R.region_table(box, pos, rng)
        assert np.unique(slot).size == slot.size and slot.max() < rows
        assert ((slot >= rstart[keys]) & (slot < rstart[keys] + count[keys])).all()
        assert (np.diff(rstart) >= count).all() and (np.diff(rstart) > count).any()
        assert np.array_equal(R.table_pops(rstart, count), pops)
    assert seen_buckets == set(range(8))


def test_stage_three_of_the_sequence_has_a_front_shorter_than_its_list():
    """few -> over: the word holds the few's list length when the over's kernels are launched"""
    for ntiles in (1000, 729):
        rng = np.random.default_rng(ntiles)
        few = R.shape_check('few', R.shape_pops('few', ntiles, FLOOR, rng), FLOOR)
        over = R.shape_check('over', R.shape_pops('over', ntiles, FLOOR, rng), FLOOR)
        front = R.expected_front(int(few.heavy.sum()), over.cap)
        assert 0 < front < min(int(over.heavy.sum()), over.cap)


def test_deposit_reference_conserves_mass_and_wraps():
    box = R.Box(20, 4, 100.0)
    rng = np.random.default_rng(5)
    pops = R.shape_pops('few', box.ntiles, FLOOR, rng)
    pos = box.particles(pops, rng)
    dens = box.deposit(pos, 0.25)
    assert dens.dtype == np.longdouble and dens.shape == (20, 20, 20)
    assert abs(float(dens.sum()) - 0.25*pos.shape[0]) <= 1e-12*pos.shape[0]
    # one particle a quarter of a cell into the last cell of every axis: an eighth of its
    # cloud's corner weights across the seam
    one = np.full((1, 3), (19 + 0.5 + 0.25)*5.0)
    dens = box.deposit(one, 1.0)
    assert np.count_nonzero(dens) == 8
    assert abs(float(dens[19, 19, 19]) - 0.75**3) < 1e-12
    assert abs(float(dens[0, 0, 0]) - 0.25**3) < 1e-12
    assert abs(float(dens[0, 19, 19]) - 0.25*0.75**2) < 1e-12
