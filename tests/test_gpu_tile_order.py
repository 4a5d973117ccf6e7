"""GPU tests of the heavy-tiles-first launch order of the tile kernels (cgk_tile_order,
tile_order_args and the block -> tile prologues of k_deposit_cic_pull and k_gather_kick_tiled
in cg_tiled_kernels.hip) at its edges: every tile is run exactly once whatever the list, its
overflow and the number of blocks in front of the walk are.

In one process, on one domain, with CONCEPT_GPU_TILE_ORDER_MIN=-6: boxes of a few tiles qualify
and a tile of seven particles can be heavy.  tests/tile_order_refs.py restates the order's
numbers, checks the device list and makes the particles; the four population shapes are
    quiet      nobody above the threshold
    few        1 to 16 heavy tiles
    over       half as many heavy tiles again as the list holds, in four classes: the list
               ends inside a class
    saturated  tiles of 64 class units and more (class 63) beside lower classes
each with particles in the last cell of their tile in every dimension (buckets 1 to 7) and
with the first and the last tile of the box populated (heavy, in all but the quiet shape): their
lower neighbours in the pull deposit lie across the periodic seam.

Grids.  The tile extent is the largest of 16, 8, 4, 2 that divides the grid into at least two
tiles per dimension, so an extent below 16 has an odd number of tiles per dimension (or two):
ten per dimension exist at T = 16 only.
    160 (T 16, 10^3 tiles)  cap 128, the XCD-interleaved walk (ntiles % 8 == 0)
    72, 36, 18 (T 8, 4, 2; 9^3 tiles)  cap 96, the plain walk
are the smallest grids of each extent whose front can be shorter than the list
(front < cap needs cap > 72, i.e. 584 tiles);
    80, 40, 20 (T 16, 8, 4; 5^3 tiles)  cap 16: the list overflows at 17 heavy tiles and
the front is always the whole cap.

Bars.  Deposit: 1e-12 of the rms of the long-double reference (TOL of test_gpu_pm.py), on a
mesh filled with 1e30 before (assign: a tile run by nobody keeps it) and on a known field
(accumulate: a tile run twice adds twice).  Gather-kick: torch.equal with the direct
cg_gather_kick on the same mesh (the identity of test_tiled_accumulate_and_strays).  Fused pass:
bit-equal per particle id with the same call on a context whose order is off
(CONCEPT_GPU_TILE_ORDER_MIN=0).  Sum of |mom|^2: 1e-13 of math.fsum over the pass's output
(the bar of test_fused_pass_leaves_the_sum_of_mom2)."""
import math

import numpy as np
import pytest

import tile_order_refs as R

pytestmark = pytest.mark.gpu

ENV = 'CONCEPT_GPU_TILE_ORDER_MIN'
FLOOR = 6
TOL = 1e-12          # test_gpu_pm.py
TOL_SUM = 1e-13      # test_fused_pass_leaves_the_sum_of_mom2
L = 100.0
SENTINEL = 1e30
CONTRIBUTION = 0.7
# (gridsize, tile extent, the front can be shorter than the list)
GRIDS = [(160, 16, True), (72, 8, True), (36, 4, True), (18, 2, True),
         (80, 16, False), (40, 8, False), (20, 4, False)]
SEQUENCE = ('quiet', 'few', 'over', 'few', 'quiet', 'saturated')


def rms(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64)**2).mean()))


def latch(torch, mesh):
    """the context reads the environment with its first tile kernel: an empty deposit"""
    mesh.deposit_tiled(torch.empty((0, 3), dtype=torch.float64, device='cuda'),
                       mesh.new_tile_table(), 1.0)
    mesh.synchronize()


def fill(torch, mesh, field):
    """the mesh's cells = field ((N, N, N) or a number); its padding 0"""
    N, per, pad = mesh.gridsize, mesh.layer_doubles, mesh.pad
    buf = np.zeros((N, per))
    buf[:, :N*pad].reshape(N, N, pad)[:, :, :N] = field
    mesh.layers_write(0, N, torch.tensor(buf.reshape(-1), device='cuda'))


def cells(mesh):
    return mesh.fetch_real()[:, :, :mesh.gridsize]


class World:
    """one grid: a context with the order on, one with it off, and per shape the particles,
    their tables and the references — made once, never changed"""

    def __init__(self, torch, N, T, short, mp):
        from concept_amd.mesh import PotentialMesh
        self.torch, self.N, self.T, self.short = torch, N, T, short
        self.box = R.Box(N, T, L)
        mp.setenv(ENV, str(-FLOOR))
        self.on = PotentialMesh(N, L)
        latch(torch, self.on)
        mp.setenv(ENV, '0')
        self.off = PotentialMesh(N, L)
        latch(torch, self.off)
        self.meshes = [self.on, self.off]
        # a change of the tile rule must not quietly move the case
        for m in self.meshes:
            assert (m.tile_extent, m.tiles_per_dim, m.ntiles) == (T, N//T, (N//T)**3)
        assert self.on.tile_order() is not None and self.on.tile_order().size == 0
        assert self.off.tile_order() is None
        self.cap = ((self.box.ntiles//8) + 7) & ~7
        assert (self.cap > 72) == short
        assert (self.box.ntiles % 8 == 0) == (N == 160)     # the interleaved walk
        self._shapes, self._refs = {}, {}
        rng = np.random.default_rng(7*N)
        self.potential = rng.normal(0, 1, (N, N, N))
        self.base = rng.uniform(0.5, 1.5, (N, N, N))

    def close(self):
        for m in self.meshes:
            m.close()

    def shape(self, name):
        """particles of a shape in three layouts: dense tile order, regions with gaps whose
        count table is 16-byte aligned, and the same regions with the count table one
        element into a larger tensor"""
        if name in self._shapes:
            return self._shapes[name]
        torch, box = self.torch, self.box
        rng = np.random.default_rng(1000*self.N + R.SHAPES.index(name))
        pops = R.shape_pops(name, box.ntiles, FLOOR, rng)
        order = R.shape_check(name, pops, FLOOR)       # (on the CPU, before any GPU call)
        pos = box.particles(pops, rng)
        n = pos.shape[0]
        mom = rng.normal(0, 1, (n, 3))
        s = {'name': name, 'pops': pops, 'order': order, 'pos': pos, 'mom': mom, 'n': n}
        dev = 'cuda'
        perm, start = R.dense_table(box, pos)
        s['dense'] = {'slot': np.argsort(perm), 'rows': n, 'count': None,
                      'start': torch.tensor(start, dtype=torch.int32, device=dev)}
        slot, start, count, rows = R.region_table(box, pos, rng)
        aligned = torch.tensor(count, dtype=torch.int32, device=dev)
        larger = torch.zeros(count.size + 1, dtype=torch.int32, device=dev)
        larger[1:] = aligned
        assert aligned.data_ptr() % 16 == 0 and larger[1:].data_ptr() % 16 == 4
        rstart = torch.tensor(start, dtype=torch.int32, device=dev)
        s['regions'] = {'slot': slot, 'rows': rows, 'start': rstart, 'count': aligned}
        s['regions_unaligned'] = {'slot': slot, 'rows': rows, 'start': rstart,
                                  'count': larger[1:], 'keep': larger}
        for lay in ('dense', 'regions', 'regions_unaligned'):
            d = s[lay]
            for what in ('pos', 'mom'):
                rows_ = np.full((d['rows'], 3), np.nan)     # (no kernel may read a gap)
                rows_[d['slot']] = s[what]
                d[what] = torch.tensor(rows_, device=dev)
            ids = np.full(d['rows'], -1, dtype=np.int64)
            ids[d['slot']] = np.arange(n)
            d['ids'] = torch.tensor(ids, device=dev)
            host_count = None if d['count'] is None else d['count'].cpu().numpy()
            assert np.array_equal(R.table_pops(d['start'].cpu().numpy(), host_count), pops)
        self._shapes[name] = s
        return s

    def density(self, name):
        if name not in self._refs:
            s = self.shape(name)
            self._refs[name] = self.box.deposit(s['pos'], CONTRIBUTION)
            total = float(self._refs[name].sum())
            assert abs(total - CONTRIBUTION*s['n']) <= 1e-12*s['n']
        return self._refs[name]

    # -- the checks ---------------------------------------------------------------------------
    def deposit(self, mesh, s, layout, accumulate):
        d = s[layout]
        if layout == 'dense':
            mesh.deposit_tiled(d['pos'], d['start'], CONTRIBUTION, accumulate=accumulate)
        else:
            mesh.deposit_regions(d['pos'], d['start'], d['count'], CONTRIBUTION,
                                 accumulate=accumulate)

    def check_deposit(self, mesh, s, layout, accumulate, label):
        """deposit onto the sentinel (assign) or onto the known field (accumulate), the list
        of the build it made, the mesh against the long-double reference"""
        fill(self.torch, mesh, self.base if accumulate else SENTINEL)
        self.deposit(mesh, s, layout, accumulate)
        mesh.synchronize()
        if mesh is not self.off:
            R.check_list(mesh.tile_order(), s['pops'], FLOOR)
        ref = self.density(s['name'])
        if accumulate:
            ref = ref + self.base
        err = float(np.abs(cells(mesh) - ref).max())
        bar = TOL*rms(ref)
        print(f'{label} {s["name"]} {layout} accumulate={accumulate}: err {err:.3g} bar {bar:.3g}')
        assert err <= bar, (label, s['name'], layout, accumulate, err, bar)

    def check_gather(self, mesh, s, diff_order, label, table=None):
        """tiled gather-kick of the dense layout against the direct one: bit-equal"""
        torch, d = self.torch, s['dense']
        table = d['start'] if table is None else table
        direct, tiled = d['mom'].clone(), d['mom'].clone()
        mesh.gather_kick(d['pos'], direct, diff_order, -0.5)
        mesh.gather_kick_tiled(d['pos'], tiled, table, diff_order, -0.5)
        mesh.synchronize()
        assert not torch.equal(direct, d['mom']), 'the kick must not vanish'
        assert torch.equal(direct, tiled), (label, s['name'], diff_order)
        return direct


@pytest.fixture(scope='module', params=GRIDS, ids=lambda g: f'N{g[0]}-T{g[1]}')
def world(request):
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    with pytest.MonkeyPatch.context() as mp:
        w = World(torch, *request.param, mp)
        yield w
        w.close()


def test_host_keys_are_the_library_s(world):
    """the tile and bucket tile_order_refs gives a position are those of the library's own CIC
    index map (cg_cic_indices): the tables made on the host describe the GPU's tiles"""
    torch, box = world.torch, world.box
    for name in R.SHAPES:
        s = world.shape(name)
        idx = world.on.cic_indices(torch.tensor(s['pos'], device='cuda')).cpu().numpy()
        assert np.array_equal(idx - R.NGHOSTS, box.stencil(s['pos'])[0])


@pytest.mark.parametrize('shape', R.SHAPES)
def test_deposit_runs_every_tile_once(world, shape):
    """the list of each of the three population sources of k_order_pops (dense start
    differences, the count table through two 16-byte loads, the count table through eight
    scalar loads — the binding takes the unaligned view as it is), and the deposit of each in
    both modes"""
    s = world.shape(shape)
    for layout in ('dense', 'regions', 'regions_unaligned'):
        for accumulate in (False, True):
            world.check_deposit(world.on, s, layout, accumulate, 'on')
    world.check_deposit(world.off, s, 'regions', True, 'off')


@pytest.mark.parametrize('shape', R.SHAPES)
def test_gather_kick_runs_every_particle_once(world, shape):
    torch = world.torch
    s = world.shape(shape)
    d, n = s['dense'], s['n']
    dtm = 0.1*world.box.cs       # momenta of rms 1: a tenth of a cell per drift
    for mesh in world.meshes:
        fill(torch, mesh, world.potential)
    for diff_order in (2, 4):
        direct = world.check_gather(world.on, s, diff_order, 'on')
        assert torch.equal(direct, world.check_gather(world.off, s, diff_order, 'off'))
        # with the histogram of the next drift: the momenta, and the histogram through the
        # table cg_drift_sort makes of it (twice the rows: a histogram that counted a tile
        # twice would send the scatter past the particles' own n rows)
        tables = []
        for mesh in world.meshes:
            mom = d['mom'].clone()
            mesh.gather_kick_tiled_prepare(d['pos'], mom, d['start'], diff_order, -0.5, dtm)
            assert torch.equal(mom, direct), (shape, diff_order)
            out = [torch.zeros((2*n + 64, 3), dtype=torch.float64, device='cuda')
                   for _ in range(2)]
            ids_out = torch.zeros(2*n + 64, dtype=torch.int64, device='cuda')
            table = mesh.drift_sort(d['pos'], mom, d['ids'], out[0][:n], out[1][:n],
                                    ids_out[:n], dtm)
            assert mesh.error_flags() == 0
            assert int(table[-1]) == n
            assert np.array_equal(np.sort(ids_out[:n].cpu().numpy()), np.arange(n))
            tables.append(table)
        assert torch.equal(tables[0], tables[1])


def run_fused(world, mesh, s, layout, diff_order, want_sum):
    """cg_gather_kick_drift_scatter of a layout -> per particle id: positions, momenta; the
    output populations; the device's sum of |mom|^2"""
    torch = world.torch
    d, n = s[layout], s['n']
    dtm = 0.1*world.box.cs
    rows = mesh.region_capacity(n)
    pos_out = torch.full((rows, 3), math.nan, dtype=torch.float64, device='cuda')
    mom_out = torch.full((rows, 3), math.nan, dtype=torch.float64, device='cuda')
    ids_out = torch.full((rows,), -1, dtype=torch.int64, device='cuda')
    start_out, count_out = mesh.new_region_table()
    total = torch.full((1,), math.nan, dtype=torch.float64, device='cuda')
    mesh.set_momentum_sum(total if want_sum else None)
    try:
        mesh.predict_regions(d['start'], d['count'], start_out)
        mesh.gather_kick_drift_scatter(d['pos'], d['mom'], d['ids'], d['start'], d['count'],
                                       pos_out, mom_out, ids_out, start_out, count_out,
                                       diff_order, -0.5, dtm)
        assert mesh.error_flags() == 0
    finally:
        mesh.set_momentum_sum(None)
    st, ct = start_out.cpu().numpy().astype(np.int64), count_out.cpu().numpy().astype(np.int64)
    assert int(ct.sum()) == n and (np.diff(st) >= ct).all() and st[-1] <= rows
    live = np.repeat(st[:-1] - (np.cumsum(ct) - ct), ct) + np.arange(n)
    ids = ids_out.cpu().numpy()[live]
    assert np.array_equal(np.sort(ids), np.arange(n))
    pos, mom = np.empty((n, 3)), np.empty((n, 3))
    pos[ids] = pos_out.cpu().numpy()[live]
    mom[ids] = mom_out.cpu().numpy()[live]
    return pos, mom, count_out, float(total[0])


def check_fused(world, s, layout, diff_order, label):
    on = run_fused(world, world.on, s, layout, diff_order, True)
    key = (s['name'], diff_order)
    if key not in world._refs:
        # the order off; its momenta are those of the direct kick, bit for bit
        off = run_fused(world, world.off, s, 'regions', diff_order, False)
        direct = world.torch.tensor(s['mom'], device='cuda')
        world.off.gather_kick(world.torch.tensor(s['pos'], device='cuda'), direct, diff_order,
                              -0.5)
        assert np.array_equal(off[1], direct.cpu().numpy())
        assert not np.array_equal(off[1], s['mom']) and not np.array_equal(off[0], s['pos'])
        world._refs[key] = off
    off = world._refs[key]
    assert np.array_equal(on[0], off[0]), (label, 'positions')
    assert np.array_equal(on[1], off[1]), (label, 'momenta')
    assert world.torch.equal(on[2], off[2]), (label, 'count_out')
    want = math.fsum((on[1]**2).ravel())
    print(f'{label} {s["name"]} {layout}: sum of mom^2 {on[3]!r}, fsum {want!r}, '
          f'relative difference {abs(on[3] - want)/want:.3g}')
    assert abs(on[3] - want) <= TOL_SUM*want, (label, on[3], want)


@pytest.mark.parametrize('shape', R.SHAPES)
def test_fused_pass_equals_the_pass_without_the_order(world, shape):
    s = world.shape(shape)
    for mesh in world.meshes:
        fill(world.torch, mesh, world.potential)
    for layout, diff_order in (('regions', 2), ('regions_unaligned', 2), ('dense', 2),
                               ('regions', 4)):
        check_fused(world, s, layout, diff_order, 'fused')


def test_momentum_sum_with_a_full_and_a_shortened_front(world):
    """the partials of cg_set_momentum_sum are laid out by the number of blocks the pass was
    launched with: the whole cap after a build that filled the list, fewer after a short one
    (where the grid's cap admits it) — on the overflowing list in both cases"""
    torch, mesh = world.torch, world.on
    over, few = world.shape('over'), world.shape('few')
    for m in world.meshes:
        fill(torch, m, world.potential)
    n_list = min(int(over['order'].heavy.sum()), world.cap)
    for before, seen, name in ((over, n_list, 'full'), (few, int(few['order'].heavy.sum()),
                                                        'short')):
        world.deposit(mesh, before, 'dense', False)
        mesh.synchronize()               # the pinned word now holds this build's length
        assert mesh.tile_order().size == seen
        front = R.expected_front(seen, world.cap)
        if name == 'full':
            assert front == world.cap
        elif world.short:
            assert 0 < front < n_list    # tiles ranked [front, n_list) are left to the walk
        else:
            assert front == world.cap
        fill(torch, mesh, world.potential)
        check_fused(world, over, 'regions', 2, f'{name} front {front}')


@pytest.mark.parametrize('accumulate', [False, True], ids=['assign', 'accumulate'])
def test_the_stale_word_of_the_last_build(world, accumulate, monkeypatch):
    """deposit -> solve -> gather-kick through the shapes on a fresh context, synchronised
    after each call: the word tile_order_args reads then holds the previous build's length
    when the deposit is launched, and the deposit's own when the gather takes its build over"""
    from concept_amd.mesh import PotentialMesh
    torch = world.torch
    monkeypatch.setenv(ENV, str(-FLOOR))
    mesh = PotentialMesh(world.N, L)
    cap = world.cap
    diff_order = 4 if accumulate else 2
    try:
        seen = None                      # no build yet: the word is all ones
        for stage, name in enumerate(SEQUENCE, 1):
            s = world.shape(name)
            n_list = min(int(s['order'].heavy.sum()), cap)
            front = R.expected_front(seen, cap)
            if stage == 1:               # quiet, word all ones: the whole cap in front, all of
                assert front == cap and n_list == 0        # its blocks end at once
            elif stage == 2:             # few after quiet, word 0: the plain launch although
                assert front == 0 and n_list > 0           # a list exists
            elif stage == 3 and world.short:
                # over after few: the front is shorter than the list — the tiles ranked
                # [front, cap) are walked, those beyond the list were never on it
                assert n_list == cap and 0 < front < min(int(s['order'].heavy.sum()), cap)
            elif stage == 3:             # (125 tiles: the front is always the whole cap)
                assert n_list == cap == front
            elif stage == 4:             # few after over: a list much shorter than the front
                assert front == cap and 0 < n_list <= 16 and n_list < front
            elif stage == 5:             # quiet after few: blocks in front of an empty list
                assert front > 0 and n_list == 0
            else:                        # saturated after quiet: the plain launch again
                assert front == 0 and n_list > 0
            world.check_deposit(mesh, s, 'dense', accumulate, f'stage {stage} front {front}')
            assert mesh.tile_order().size == n_list
            mesh.poisson_solve(4, -1.0, False, 0.0)
            mesh.synchronize()
            # the gather takes the deposit's build over (same table) with a front made from
            # the word as it is now: the length of this very list
            world.check_gather(mesh, s, diff_order, f'stage {stage}')
            R.check_list(mesh.tile_order(), s['pops'], FLOOR)
            seen = n_list
    finally:
        mesh.close()


def test_gather_takes_over_a_build_whose_tables_were_rewritten(world):
    """the gather-kick reuses the deposit's list when it is given the same table pointers —
    also when another particle set was sorted into them in between: list and places of one
    build describe every tile once whatever the populations have become"""
    torch, mesh = world.torch, world.on
    a, b = world.shape('over'), world.shape('saturated')
    # dense: deposit with A's table, B's table written into the same tensor, gather B
    table = a['dense']['start'].clone()
    fill(torch, mesh, SENTINEL)
    mesh.deposit_tiled(a['dense']['pos'], table, CONTRIBUTION, accumulate=False)
    mesh.synchronize()
    list_a = mesh.tile_order()
    R.check_list(list_a, a['pops'], FLOOR)
    table.copy_(b['dense']['start'])
    fill(torch, mesh, world.potential)
    for diff_order in (2, 4):
        world.check_gather(mesh, b, diff_order, 'rewritten', table=table)
        assert np.array_equal(mesh.tile_order(), list_a)       # still A's build
    # regions: deposit with A's (start, count), B's written into them, the fused pass on B
    start, count = a['regions']['start'].clone(), a['regions']['count'].clone()
    mesh.deposit_regions(a['regions']['pos'], start, count, CONTRIBUTION)
    mesh.synchronize()
    list_a = mesh.tile_order()
    R.check_list(list_a, a['pops'], FLOOR)
    start.copy_(b['regions']['start'])
    count.copy_(b['regions']['count'])
    rewritten = dict(b, rewritten=dict(b['regions'], start=start, count=count))
    for m in world.meshes:
        fill(torch, m, world.potential)
    check_fused(world, rewritten, 'rewritten', 2, 'rewritten')
    assert np.array_equal(mesh.tile_order(), list_a)
