"""NumPy restatement of the heavy-tiles-first launch order of the tile kernels (cgk_tile_order
and tile_order_args in concept_amd/csrc/cg_tiled_kernels.hip), the properties its device list
must have whatever the order of the atomics that placed it, and what the tests of that order
need on the host: particle sets with chosen tile populations, their tile tables (dense, and
regions with gaps) and the long-double CIC deposit they are compared with.

The numbers of one build, from the tiles' populations and the floor
(|CONCEPT_GPU_TILE_ORDER_MIN|), all in integers:
    total = sum(pops)                    thr  = max(floor, (3*total)//(2*ntiles))
    unit  = max(thr//3, 1)               heavy = pops > thr
    cls   = minimum(pops//unit, 63)      cap  = ((ntiles//8) + 7) & ~7
The list holds the heavy tiles by falling class, cap of them at most; inside a class the order
is free (one cursor per class, taken with atomics).

The deposit reference is test_gpu_general_interp.ref_deposit (terms in float64 as the kernels
form them, summed per cell in np.longdouble) with the geometry of oracle.deposit_geometry."""
import collections

import numpy as np

LD = np.longdouble
CLASSES = 64
NGHOSTS = 2

Order = collections.namedtuple('Order', 'total thr unit heavy cls cap')


def order_numbers(pops, floor):
    pops = np.asarray(pops, dtype=np.int64)
    ntiles = pops.size
    total = int(pops.sum())
    thr = max(int(floor), (3*total)//(2*ntiles))
    unit = max(thr//3, 1)
    heavy = pops > thr
    cls = np.minimum(pops//unit, CLASSES - 1)
    cap = ((ntiles//8) + 7) & ~7
    return Order(total, thr, unit, heavy, cls, cap)


def expected_front(seen, cap):
    """blocks tile_order_args puts in front of the walk when the pinned word holds `seen`
    (None: no build seen yet, the word is all ones); 0: the plain launch, no list passed"""
    if seen is None:
        return cap
    if seen == 0:
        return 0
    want = seen + seen//4 + 64
    return (want + 7) & ~7 if want < cap else cap


def check_list(heavy_list, pops, floor):
    """what the device list of one build must satisfy -> its Order numbers"""
    o = order_numbers(pops, floor)
    lst = np.asarray(heavy_list).astype(np.int64)
    assert lst.ndim == 1
    assert ((lst >= 0) & (lst < o.heavy.size)).all(), 'an entry is no tile'
    assert np.unique(lst).size == lst.size, 'a tile is on the list twice'
    assert o.heavy[lst].all(), f'tiles {lst[~o.heavy[lst]]} on the list are not heavy (thr {o.thr})'
    n_heavy = int(o.heavy.sum())
    assert lst.size == min(n_heavy, o.cap), \
        f'{lst.size} tiles on the list, {n_heavy} heavy tiles, cap {o.cap}'
    along = o.cls[lst]
    assert (np.diff(along) <= 0).all(), 'classes rise along the list'
    if lst.size:
        on = np.zeros(o.heavy.size, dtype=bool)
        on[lst] = True
        must = o.heavy & (o.cls > along[-1])
        assert on[must].all(), f'tiles {np.flatnonzero(must & ~on)} of a class above the last ' \
                               f'entry\'s ({along[-1]}) are missing'
        if n_heavy <= o.cap:
            assert on[o.heavy].all()
    return o


# -- particles with chosen tile populations -------------------------------------------------
class Box:
    """N cells and N/T tiles per dimension, cell-centred, two ghost layers: where a particle's
    lower CIC cell is (mesh.py:1577-1606 through oracle.deposit_geometry).  N, order and
    stencil() are what test_gpu_general_interp.ref_deposit asks of its `case`."""
    order = 2   # CIC

    def __init__(self, N, T, L):
        from oracle import oracle
        assert N % T == 0
        self.N, self.T, self.nt, self.L = N, T, N//T, float(L)
        self.ntiles = self.nt**3
        self.cs = self.L/N
        self.off, self.scale = oracle.deposit_geometry(self.L, N, NGHOSTS)

    def stencil(self, pos, sign=-1):
        """lower cells (n, 3) before the periodic wrap, weights [axis][0 | 1] -> (n,): the
        interface ref_deposit wants of its `case`"""
        from test_gpu_general_interp import index_weights
        first, w = [], []
        for d in range(3):
            i, wd = index_weights((pos[:, d] - self.off[d])*self.scale, 2)
            first.append(i - NGHOSTS)
            w.append(wd)
        return np.stack(first, 1), w

    def keys(self, pos):
        """8*tile + bucket (cg_tiles.h tile_of)"""
        cell = np.mod(self.stencil(pos)[0], self.N)
        t = cell//self.T
        last = (cell % self.T == self.T - 1).astype(np.int64)
        return ((t[:, 0]*self.nt + t[:, 1])*self.nt + t[:, 2])*8 + 4*last[:, 0] + 2*last[:, 1] \
            + last[:, 2]

    def particles(self, pops, rng):
        """positions (in random memory order) that put pops[t] particles into tile t: three in
        ten of them per dimension in the tile's last cell (buckets 1 to 7), all of them at
        least 1/16 of a cell away from the cell's ends"""
        pops = np.asarray(pops, dtype=np.int64)
        tile = np.repeat(np.arange(self.ntiles), pops)
        n = tile.size
        t3 = np.stack([tile//(self.nt*self.nt), (tile//self.nt) % self.nt, tile % self.nt], 1)
        inside = rng.integers(0, self.T, (n, 3))
        inside[rng.uniform(size=(n, 3)) < 0.3] = self.T - 1
        cell = t3*self.T + inside
        frac = rng.uniform(1/16, 15/16, (n, 3))
        # cell c holds the positions [(c + 1/2)*cs, (c + 3/2)*cs), through the box's seam
        pos = np.mod((cell + 0.5 + frac)*self.cs, self.L)
        pos = pos[rng.permutation(n)]
        assert (pos >= 0).all() and (pos < self.L).all()
        return pos

    def pops(self, pos):
        return np.bincount(self.keys(pos)//8, minlength=self.ntiles)

    def deposit(self, pos, contribution):
        """the CIC deposit of pos as an (N, N, N) np.longdouble mesh"""
        from test_gpu_general_interp import ref_deposit
        cells, total, _, _ = ref_deposit(self, pos, contribution)
        mesh = np.zeros(self.N**3, dtype=LD)
        mesh[cells] = total
        return mesh.reshape(self.N, self.N, self.N)


SHAPES = ('quiet', 'few', 'over', 'saturated')


def shape_pops(shape, ntiles, floor, rng):
    """populations of the four shapes the order is tested with; shape_check states what
    makes each of them what it is.  The first and the last tile of the box (first and last
    in every dimension: their lower neighbours lie across the periodic seam) are populated in
    every shape and heavy in all but the quiet one."""
    cap = ((ntiles//8) + 7) & ~7
    corners = np.array([0, ntiles - 1])
    others = rng.permutation(np.arange(1, ntiles - 1))
    if shape == 'quiet':
        pops = rng.integers(0, floor, ntiles)       # nobody above the floor
        pops[corners] = floor - 1
        return pops
    pops = rng.integers(0, 4, ntiles)
    if shape == 'few':
        sizes = np.array([1100, 700, 13, 20, 40, 90, 150, 300])
    elif shape == 'over':
        # half as many heavy tiles again as the list holds, in four classes of equal size:
        # the list ends inside the third
        sizes = np.repeat([150, 40, 90, 60], (cap + cap//2)//4)
    elif shape == 'saturated':
        sizes = np.array([2000, 600, 8, 14, 20, 50, 100, 30])
    else:
        raise ValueError(shape)
    where = np.concatenate([corners, others[:sizes.size - 2]])
    pops[where] = sizes
    return pops


def shape_check(shape, pops, floor):
    """the defining condition of each shape -> its Order numbers"""
    o = order_numbers(pops, floor)
    n_heavy = int(o.heavy.sum())
    if shape == 'quiet':
        assert n_heavy == 0 and o.total > 0
    elif shape == 'few':
        assert 1 <= n_heavy <= 16 and n_heavy < o.cap
    elif shape == 'over':
        assert n_heavy > o.cap
        falling = np.sort(o.cls[o.heavy])[::-1]
        assert np.unique(falling).size >= 3
        assert falling[o.cap - 1] == falling[o.cap], 'the list must end inside a class'
        assert falling[0] > falling[o.cap] > falling[-1]
        assert falling[0] < CLASSES - 1
    elif shape == 'saturated':
        assert (pops[o.heavy]//o.unit >= CLASSES).any()
        assert (o.heavy & (o.cls < CLASSES - 1)).sum() >= 2
        assert n_heavy < o.cap
    else:
        raise ValueError(shape)
    if shape != 'quiet':
        assert o.heavy[0] and o.heavy[-1]
    assert pops[0] > 0 and pops[-1] > 0
    return o


# -- tile tables ------------------------------------------------------------------------------
def dense_table(box, pos):
    """-> permutation into tile order, start int64[8*ntiles + 1]"""
    keys = box.keys(pos)
    perm = np.argsort(keys, kind='stable')
    count = np.bincount(keys, minlength=8*box.ntiles)
    return perm, np.concatenate([[0], np.cumsum(count)])


def region_table(box, pos, rng):
    """regions with gaps: every (tile, bucket) has room for its population and 0 to 5 slots
    more -> slot of every particle, start int64[8*ntiles + 1], count int64[8*ntiles], rows"""
    keys = box.keys(pos)
    count = np.bincount(keys, minlength=8*box.ntiles)
    room = count + rng.integers(0, 6, count.size)
    start = np.concatenate([[0], np.cumsum(room)])
    perm = np.argsort(keys, kind='stable')
    rank = np.arange(pos.shape[0]) - np.repeat(np.cumsum(count) - count, count)
    slot = np.empty(pos.shape[0], dtype=np.int64)
    slot[perm] = start[keys[perm]] + rank
    return slot, start, count, int(start[-1])


def table_pops(start, count=None):
    """per-tile populations of a tile table, as k_order_pops reads them"""
    if count is None:
        start = np.asarray(start, dtype=np.int64)
        return start[8::8] - start[:-8:8]
    return np.asarray(count, dtype=np.int64).reshape(-1, 8).sum(1)
