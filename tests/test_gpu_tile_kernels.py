"""GPU tests of the two tile kernels of concept_amd/csrc/cg_tiled_kernels.hip against the plain
references of tests/tile_kernel_refs.py, at every tile extent, stencil order and mode.

Sizes: N = 4, 6 (T = 2), 8, 12 (T = 4), 16, 24 (T = 8), 32, 48 (T = 16): two and three tiles per
dimension of every extent; the constructor accepts all of them.  One PotentialMesh(N, 96) per
size, one process; and x-slab contexts of N = 16, 24 (2 domains) and 48 (3), in the same process.

The input (tile_kernel_refs.placed_particles; test_tile_kernel_refs_host.py checks each claim on
the CPU, check_placed() repeats it here on what is uploaded): a particle in every cell of the
first and last layer of tile 0 along each dimension; coordinates exactly 0, nextafter(L, 0) and on
a cell face (a weight of exactly 0); lower cells of -1 before the wrap; an empty tile; tiles of
exactly 512 and 513 particles; a tile whose bucket 0 is empty and whose bucket 5 holds 65; a tile
with bucket 0 only; momenta that change bucket, change tile, wrap the box both ways in every
dimension and (aim_at_zero) drift one coordinate per axis to exactly 0; 128 rows at rest (the
kick is added to 0: no ulp of a momentum hides the sum's roundings); a seeded fill elsewhere.
The potential is NOT a solved one: independent normal values, NaN in the row padding and in the
unused row of every layer — a misread neighbour is a wrong kick of order one, a read of the
padding a kick that is not finite.

Bars.
  deposit   per cell (m + 2)*2^-53*sum|term|, m the number of terms: three roundings per term
            (the reference forms the terms in float64 as the kernel does), m - 1 additions in any
            order.  Accumulated a second time: twice the reference, twice the bar.
  kick      per particle and dimension 10*2^-53*|factor|*sum|w*f| + ulp(momentum before).  The
            roundings, counted in k_gather_kick_tiled (the same for both orders: force_cell and
            the weights (w_x*w_y)*w_z are formed in float64 by the reference too):
                val += f*w      1 product, 7 additions (the first one adds to 0)      8
                val *= factor                                                         1
                mom + val       half an ulp of the sum <= 2^-53*(|mom| + |val|)       1 (+ ulp)
  positions bit-equal to oracle.drift of the input positions and the pass's OWN output momenta
  sum       of |mom|^2: n*2^-53*sum|mom|^2 against math.fsum over the pass's output momenta

Coverage, one row per instantiation (T, ORDER, MODE, input).  "now": the worst error/bar this
file measured on the MI355X against the plain reference (the larger of the two sizes of the
extent; all particles / the rows at rest, whose bar has no ulp of a momentum in it: the sum's
roundings alone).  "before this file": who reached the row, and against what —
    A  test_gpu_tile_order.py: another GPU path (cg_gather_kick) on a random potential; its
       deposit against a long-double sum at 1e-12 of the rms
    B  test_gpu_pm.py: goldens of the oracle (a solved potential) and the untiled cg_gather_kick
    C  test_gpu_pm.py, test_gpu_bench_kernels_parity.py: cg_gather_kick_tiled + cg_drift_sort, i.e.
       a GPU path with the same LDS layout, on a solved potential
    D  the small gravity() goldens (N 12): the oracle, whole step, solved potential
    E  test_gpu_particle_gate.py (N 16): two contexts against each other
    F  test_gpu_pm.py: long-double sum at 1e-12 of the rms
   T order mode      input    now: all / at rest   before this file
  16   2   mode 0    dense    0.902 / 0.241        B, A
  16   2   mode 1    dense    0.902 / 0.241        B, A
  16   2   mode 2    dense    0.902 / 0.241        C, A
  16   2   mode 2    gapped   0.886 /   -          C, A
  16   4   mode 0    dense    0.876 / 0.235        B, A
  16   4   mode 1    dense    0.876 / 0.235        B, A
  16   4   mode 2    dense    0.876 / 0.235        C
  16   4   mode 2    gapped   0.976 /   -          C, A
   8   2   mode 0    dense    0.937 / 0.246        A
   8   2   mode 1    dense    0.937 / 0.246        A
   8   2   mode 2    dense    0.937 / 0.246        A, E
   8   2   mode 2    gapped   0.914 /   -          A
   8   4   mode 0    dense    0.866 / 0.214        A
   8   4   mode 1    dense    0.866 / 0.214        A
   8   4   mode 2    dense    0.866 / 0.214        nobody
   8   4   mode 2    gapped   0.854 /   -          A
   4   2   mode 0    dense    0.858 / 0.323        A, D
   4   2   mode 1    dense    0.858 / 0.323        A, D
   4   2   mode 2    dense    0.858 / 0.323        A
   4   2   mode 2    gapped   0.873 /   -          A
   4   4   mode 0    dense    0.827 / 0.248        A
   4   4   mode 1    dense    0.827 / 0.248        A
   4   4   mode 2    dense    0.827 / 0.248        nobody
   4   4   mode 2    gapped   0.838 /   -          A
   2   2   mode 0    dense    0.832 / 0.238        A
   2   2   mode 1    dense    0.832 / 0.238        A
   2   2   mode 2    dense    0.832 / 0.238        A
   2   2   mode 2    gapped   0.732 /   -          A
   2   4   mode 0    dense    0.595 / 0.252        A
   2   4   mode 1    dense    0.595 / 0.252        A
   2   4   mode 2    dense    0.595 / 0.252        nobody
   2   4   mode 2    gapped   0.636 /   -          A
  16   -   deposit   dense, regions, assign, accumulate   0.381   F, A
   8   -   deposit   dense, regions, assign, accumulate   0.336   A
   4   -   deposit   dense, regions, assign, accumulate   0.206   A
   2   -   deposit   dense, regions, assign, accumulate   0.127   A
  MODE 2 runs with and without the sum of |mom|^2 (MOM2) and with and without ids/aux: bit-equal
  outputs, the sum below 0.001 of its bar everywhere.  MODE 0 with a particle off its tile
  (order 4, every size): the ratios of the mode 0 rows.  The ratios of "all" are those of the last
  addition, mom + val: half an ulp of the sum against one ulp of the momentum before.
  Slab contexts (k_deposit_cic_pull with a non-periodic xmap and the ghost row ta == ntx), summed
  as the hand-over does: N 16 / 2 domains (T 8, 1 tile row) 0.333, N 24 / 2 (T 4, 3 rows) 0.292,
  N 48 / 3 (T 16, 1 row) 0.378; before this file test_gpu_slab_handover.py at T 16 against the
  untiled deposit at 1e-12 of the maximum.
"""
import functools
import math

import numpy as np
import pytest

import tile_kernel_refs as R

pytestmark = pytest.mark.gpu

U = 2.0**-53
CONTRIBUTION = 0.7
FSENT, ISENT = 1e150, -7
PAD = 64
ORDERS = (2, 4)


@functools.lru_cache(maxsize=None)
def placed_input(N, T):
    """the placed particles of a size, checked, with their per-(tile, bucket) populations"""
    placed = R.placed_particles(N, T)
    return placed, R.check_placed(placed)


@functools.lru_cache(maxsize=None)
def density_ref(N, T):
    return R.deposit_ref(placed_input(N, T)[0]['pos'], N, R.L, R.NGHOSTS, True, CONTRIBUTION)


def density_ratio(cells, times, dens, m, mag, label):
    """worst error/bar of deposited cells against `times` the reference"""
    assert np.isfinite(cells).all(), f'{label}: a cell was not written'
    err = np.abs(cells - times*dens)
    bar = times*(m + 2)*U*mag
    assert (err[bar == 0] == 0).all(), f'{label}: an empty cell is not 0'
    return float((err[bar > 0]/bar[bar > 0]).max())


class World:
    """one size: the mesh, the placed particles in memory order and tile-sorted on the device,
    and the references, each made once and never changed"""

    def __init__(self, torch, N, T):
        from concept_amd.mesh import PotentialMesh
        self.torch, self.N, self.T = torch, N, T
        self.mesh = PotentialMesh(N, R.L)
        m = self.mesh
        # a change of the tile rule must not quietly move the case
        assert (m.tile_extent, m.tiles_per_dim, m.ntiles) == (T, N//T, (N//T)**3)
        self.nb = 8*m.ntiles
        self.placed, self.pops = placed_input(N, T)
        self.pos = self.placed['pos']
        self.n = self.pos.shape[0]
        self.factor = R.factor_of(N)
        self.keys = R.keys_ref(self.pos, N, R.L, T)
        self._cache = {}
        dev = 'cuda'
        self.ids_dev = torch.arange(self.n, device=dev)
        self.aux_dev = torch.tensor(self.aux_of(np.arange(self.n)), device=dev)

    def close(self):
        self.mesh.close()

    @staticmethod
    def aux_of(ids):
        """the second 64-bit column: bits that are NaNs and negative numbers as doubles"""
        return (np.asarray(ids, dtype=np.int64)*0x0123456789AB) ^ np.int64(-0x7FF0000000000001)

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def phi(self, step):
        return self.cached(('phi', step), lambda: R.potential(self.N, 10*self.N + 1 + step))

    def mom(self, order):
        """the placed momenta, three rows aimed at 0 for this order's kick of phi(0)"""
        return self.cached(('mom', order), lambda: R.aim_at_zero(self.placed, self.phi(0), order))

    def density(self):
        return density_ref(self.N, self.T)

    def sorted(self, order):
        """tile-sorted on the device: pos, mom(order), ids, table"""
        def make():
            torch = self.torch
            pos = torch.tensor(self.pos, device='cuda')
            mom = torch.tensor(self.mom(order), device='cuda')
            out = torch.empty_like(pos), torch.empty_like(mom), torch.empty_like(self.ids_dev)
            table = self.mesh.sort_particles(pos, mom, self.ids_dev, *out)
            self.mesh.synchronize()
            want = np.concatenate([[0], np.cumsum(np.bincount(self.keys, minlength=self.nb))])
            assert np.array_equal(table.cpu().numpy().astype(np.int64), want), \
                'the tile table of cg_sort_particles is not that of keys_ref'
            ids = out[2].cpu().numpy()
            assert np.array_equal(self.keys[ids], np.sort(self.keys))
            return out + (table,)
        return self.cached(('sorted', order), make)

    # -- the mesh -----------------------------------------------------------------------------
    def write(self, field):
        """the mesh's cells = field ((N, N, N) or a number), NaN in the row padding and in the
        unused row of every layer"""
        m, N = self.mesh, self.N
        buf = np.full((N, m.layer_doubles), np.nan)
        buf[:, :N*m.pad].reshape(N, N, m.pad)[:, :, :N] = field
        m.layers_write(0, N, self.torch.tensor(buf.reshape(-1), device='cuda'))

    def read(self):
        """-> cells (N, N, N), everything else of the layers (1-D)"""
        m, N = self.mesh, self.N
        dst = self.torch.empty(N*m.layer_doubles, dtype=self.torch.float64, device='cuda')
        m.layers_read(0, N, dst)
        buf = dst.cpu().numpy().reshape(N, m.layer_doubles)
        inside = np.zeros(buf.shape, dtype=bool)
        inside[:, :N*m.pad].reshape(N, N, m.pad)[:, :, :N] = True
        return buf[inside].reshape(N, N, N), buf[~inside]

    # -- comparisons --------------------------------------------------------------------------
    def check_density(self, times, label):
        dens, (m, mag) = self.density()
        cells, rest = self.read()
        assert np.isnan(rest).all(), f'{label}: the padding was written'
        ratio = density_ratio(cells, times, dens, m, mag, label)
        print(f'N {self.N} T {self.T} {label}: worst error/bar {ratio:.3f}')
        assert ratio <= 1, (self.N, self.T, label, ratio)

    def check_kick(self, got, pos, mom_before, step, order, label):
        """momenta (host arrays, any common row order) against gather_kick_ref of phi(step)"""
        assert np.isfinite(got).all(), f'N {self.N} {label}: a kick is not finite (padding read?)'
        ref, mag = R.gather_kick_ref(self.phi(step), pos, mom_before, self.N, R.L, order,
                                     self.factor)
        err = np.abs(got - ref)
        bar = 10*U*abs(self.factor)*mag + np.spacing(np.abs(mom_before))
        ratio = float((err/bar).max())
        worst = int(np.argmax((err/bar).max(1)))
        print(f'N {self.N} T {self.T} order {order} {label}: worst error/bar {ratio:.3f}')
        rest = (mom_before == 0).all(1)
        if step == 0:
            # the rows at rest: no ulp of the momentum in their bar, the sum's roundings alone
            assert rest.sum() == self.placed['edges']['at_rest'].size
            at_rest = float((err[rest]/bar[rest]).max())
            print(f'N {self.N} T {self.T} order {order} {label}, rows at rest: worst error/bar '
                  f'{at_rest:.3f}')
        assert ratio <= 1, (self.N, self.T, order, label, ratio, 'key', int(
            R.keys_ref(pos[worst:worst + 1], self.N, R.L, self.T)[0]))
        assert np.abs(got - mom_before).max() > 0


@pytest.fixture(scope='module', params=R.SIZES, ids=lambda s: f'N{s[0]}-T{s[1]}')
def world(request):
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    w = World(torch, *request.param)
    yield w
    w.close()


class Fused:
    """the arrays of one cg_gather_kick_drift_scatter call and what the checks need of them"""

    def __init__(self, w, with_ids):
        torch = w.torch
        self.w, self.with_ids = w, with_ids
        self.cap = w.mesh.region_capacity(w.n)
        rows = self.cap + PAD
        self.pos = torch.full((rows, 3), FSENT, dtype=torch.float64, device='cuda')
        self.mom = torch.full((rows, 3), FSENT, dtype=torch.float64, device='cuda')
        self.ids = torch.full((rows,), ISENT, dtype=torch.int64, device='cuda')
        self.aux = torch.full((rows,), ISENT, dtype=torch.int64, device='cuda')
        self.start, self.count = w.mesh.new_region_table()
        self.total = torch.full((1,), math.nan, dtype=torch.float64, device='cuda')

    def run(self, src, order, want_sum):
        """src: (pos, mom, ids, aux, start, count | None) on the device"""
        w, mesh = self.w, self.w.mesh
        pos, mom, ids, aux, start, count = src
        mesh.set_momentum_sum(self.total if want_sum else None)
        try:
            mesh.predict_regions(start, count, self.start)
            mesh.gather_kick_drift_scatter(
                pos, mom, ids if self.with_ids else None, start, count, self.pos[:self.cap],
                self.mom[:self.cap], self.ids[:self.cap] if self.with_ids else None, self.start,
                self.count, order, w.factor, R.DTM,
                aux_in=aux if self.with_ids else None,
                aux_out=self.aux[:self.cap] if self.with_ids else None)
            self.flags = mesh.error_flags()
        finally:
            mesh.set_momentum_sum(None)
        return self

    def source(self):
        return (self.pos[:self.cap], self.mom[:self.cap], self.ids[:self.cap],
                self.aux[:self.cap], self.start, self.count)

    def host(self):
        """-> live slots, their region, and the host copies"""
        w = self.w
        st = self.start.cpu().numpy().astype(np.int64)
        ct = self.count.cpu().numpy().astype(np.int64)
        assert st[0] == 0 and (np.diff(st) >= ct).all() and st[-1] <= self.cap
        region = np.repeat(np.arange(w.nb), ct)
        live = np.repeat(st[:-1] - (np.cumsum(ct) - ct), ct) + np.arange(int(ct.sum()))
        return (live, region, ct, self.pos.cpu().numpy(), self.mom.cpu().numpy(),
                self.ids.cpu().numpy(), self.aux.cpu().numpy())


def check_fused(w, out, pos_in, mom_in, ids_in, step, order, label):
    """every claim of the fused pass on one output; pos_in, mom_in, ids_in: the live input rows on
    the host (any order) -> (pos, mom) of the output by particle id"""
    N, T, n = w.N, w.T, w.n
    assert out.flags == 0, (N, label, 'error flags', out.flags)
    live, region, ct, pos, mom, ids, aux = out.host()
    assert int(ct.sum()) == n, (N, label, 'particles lost', int(ct.sum()), n)
    dead = np.ones(pos.shape[0], dtype=bool)
    dead[live] = False
    assert (pos[dead] == FSENT).all() and (mom[dead] == FSENT).all(), f'{label}: a dead row written'
    assert (ids[dead] == ISENT).all() and (aux[dead] == ISENT).all()
    got_ids = ids[live]
    assert np.array_equal(np.sort(got_ids), np.arange(n)), f'{label}: ids are no permutation'
    assert np.array_equal(aux[live], w.aux_of(got_ids)), f'{label}: aux does not travel with ids'
    p_out, m_out = np.empty((n, 3)), np.empty((n, 3))
    p_out[got_ids], m_out[got_ids] = pos[live], mom[live]
    p_in, m_in = np.empty((n, 3)), np.empty((n, 3))
    p_in[ids_in], m_in[ids_in] = pos_in, mom_in
    w.check_kick(m_out, p_in, m_in, step, order, label)
    assert np.array_equal(p_out, R.drift_ref(p_in, m_out, R.DTM, R.L)), \
        (N, label, 'positions are not oracle.drift of the kicked momenta')
    keys = R.keys_ref(pos[live], N, R.L, T)
    assert np.array_equal(keys, region), (N, label, 'a row outside the region of its key')
    assert np.array_equal(ct, np.bincount(keys, minlength=w.nb))
    return p_out, m_out


def live_input(src_host):
    live, _, _, pos, mom, ids, _ = src_host
    return pos[live], mom[live], ids[live]


def test_deposit(world):
    """k_deposit_cic_pull<T, false> then <T, true> from the dense order, the NaN of the padding
    stays; then both from regions with gaps, which one fused step of particles at rest makes"""
    w, torch, mesh = world, world.torch, world.mesh
    p0, _, _, table = w.sorted(2)
    w.write(np.nan)
    mesh.deposit_tiled(p0, table, CONTRIBUTION, accumulate=False)
    w.check_density(1, 'deposit dense assign')
    mesh.deposit_tiled(p0, table, CONTRIBUTION, accumulate=True)
    w.check_density(2, 'deposit dense accumulate')
    # regions with gaps: one fused step of particles at rest on a flat potential leaves every
    # particle where it is (kick 0, drift 0), in the regions predicted from the dense order
    w.write(0.0)
    rest = torch.zeros_like(p0)
    out = Fused(w, True)
    _, _, i0, _ = w.sorted(2)
    out.run((p0, rest, i0, w.aux_dev[i0], table, None), 2, False)
    assert out.flags == 0
    live, _, ct, pos, _, ids, _ = out.host()
    assert int(ct.sum()) == w.n and np.array_equal(pos[live][np.argsort(ids[live])], w.pos)
    assert (np.diff(out.start.cpu().numpy().astype(np.int64)) > ct).all()     # gaps everywhere
    w.write(np.nan)
    mesh.deposit_regions(out.pos[:out.cap], out.start, out.count, CONTRIBUTION, accumulate=False)
    w.check_density(1, 'deposit regions assign')
    mesh.deposit_regions(out.pos[:out.cap], out.start, out.count, CONTRIBUTION, accumulate=True)
    w.check_density(2, 'deposit regions accumulate')


@pytest.mark.parametrize('order', ORDERS)
def test_kick_in_place_and_prepared(world, order):
    """MODE 0 and MODE 1 against gather_kick_ref; MODE 1's histogram through the table
    cg_drift_sort makes of it, against keys_ref of oracle.drift of the kicked particles, and
    against the table of a cg_drift_sort that counts for itself"""
    w, torch, mesh = world, world.torch, world.mesh
    p0, m0, i0, table = w.sorted(order)
    ids = i0.cpu().numpy()
    pos_h, mom_h = w.pos[ids], w.mom(order)[ids]
    w.write(w.phi(0))
    plain = m0.clone()
    mesh.gather_kick_tiled(p0, plain, table, order, w.factor)
    w.check_kick(plain.cpu().numpy(), pos_h, mom_h, 0, order, 'mode 0')
    prepared = m0.clone()
    mesh.gather_kick_tiled_prepare(p0, prepared, table, order, w.factor, R.DTM)
    assert torch.equal(prepared, plain), (w.N, order, 'mode 1 momenta differ from mode 0')
    w.check_kick(prepared.cpu().numpy(), pos_h, mom_h, 0, order, 'mode 1')
    tables = []
    for mom in (prepared, plain):       # the first call finds the histogram, the second counts
        out = (torch.full_like(p0, FSENT), torch.full_like(m0, FSENT), torch.full_like(i0, ISENT))
        tables.append(mesh.drift_sort(p0, mom, i0, *out, R.DTM))
        assert mesh.error_flags() == 0
        new = R.drift_ref(pos_h, mom.cpu().numpy(), R.DTM, R.L)
        moved = np.empty_like(new)
        moved[ids] = new
        got = np.empty_like(new)
        got[out[2].cpu().numpy()] = out[0].cpu().numpy()
        assert np.array_equal(got, moved), (w.N, order, 'drift_sort positions')
        want = np.bincount(R.keys_ref(new, w.N, R.L, w.T), minlength=w.nb)
        assert np.array_equal(np.diff(tables[-1].cpu().numpy().astype(np.int64)), want), \
            (w.N, order, 'prepared' if mom is prepared else 'counted', 'histogram')
    assert torch.equal(tables[0], tables[1])
    # the rows aimed at 0 arrive there
    for r, d in w.placed['edges']['to_zero']:
        assert moved[r, d] == 0.0, (w.N, order, r, d, moved[r, d])


@pytest.mark.parametrize('order', ORDERS)
def test_fused_two_steps(world, order):
    """MODE 2 from the dense order, then from the regions with gaps it left, on a NEW potential;
    with ids and aux and without either; with and without the sum of |mom|^2"""
    w, torch, mesh = world, world.torch, world.mesh
    p0, m0, i0, table = w.sorted(order)
    src0 = (p0, m0, i0, w.aux_dev[i0], table, None)
    ids0 = i0.cpu().numpy()
    results = {}
    for want_sum in (False, True):
        w.write(w.phi(0))
        one = Fused(w, True).run(src0, order, want_sum)
        label = f'mode 2 dense{" +sum" if want_sum else ""}'
        p1, m1 = check_fused(w, one, w.pos[ids0], w.mom(order)[ids0], ids0, 0, order, label)
        sums = [float(one.total[0])]
        for r, d in w.placed['edges']['to_zero']:
            assert p1[r, d] == 0.0 and m1[r, d] < 0, (w.N, order, r, d)
        w.write(w.phi(1))
        src1 = one.source()
        two = Fused(w, True).run(src1, order, want_sum)
        label = f'mode 2 gapped{" +sum" if want_sum else ""}'
        p2, m2 = check_fused(w, two, *live_input(one.host()), 1, order, label)
        sums.append(float(two.total[0]))
        results[want_sum] = (p1, m1, p2, m2)
        if want_sum:
            for s, m in zip(sums, (m1, m2)):
                want = math.fsum((m**2).ravel())
                ratio = abs(s - want)/(w.n*U*want)
                print(f'N {w.N} T {w.T} order {order} sum of |mom|^2: error/bar {ratio:.3f}')
                assert ratio <= 1, (w.N, order, s, want)
        else:
            # without ids and aux (null pointers): the same rows, whoever they belong to
            bare = Fused(w, False).run(src1, order, False)
            assert bare.flags == 0
            live, region, ct, pos, mom, ids, aux = bare.host()
            assert (ids == ISENT).all() and (aux == ISENT).all()
            assert np.array_equal(ct, two.count.cpu().numpy().astype(np.int64))
            rows = np.concatenate([pos[live], mom[live]], 1)
            ref = np.concatenate([p2, m2], 1)
            assert np.array_equal(rows[np.lexsort(rows.T)], ref[np.lexsort(ref.T)])
            dead = np.ones(pos.shape[0], dtype=bool)
            dead[live] = False
            assert (pos[dead] == FSENT).all() and (mom[dead] == FSENT).all()
    for a, b in zip(results[False], results[True]):
        assert np.array_equal(a, b), (w.N, order, 'the sum of |mom|^2 changed the pass')


def test_particle_outside_its_tile(world):
    """one particle moved to another tile after the sort: MODE 0 reads the mesh directly for it
    and still meets the reference; MODE 2 raises CG_ERR_NOT_IN_TILE and leaves its inputs alone"""
    from concept_amd import lib
    w, torch, mesh = world, world.torch, world.mesh
    order = 4
    p0, m0, i0, table = w.sorted(order)
    ids = i0.cpu().numpy()
    e = w.placed['edges']
    row = int(np.flatnonzero(ids == e['move_tile'][0])[0])
    pos = p0.clone()
    # the far corner of the box, on the seam: the stencil of the direct read wraps
    there = torch.tensor([0.25*R.L/w.N, R.L - 0.75*R.L/w.N, 0.25*R.L/w.N], dtype=torch.float64,
                         device='cuda')
    pos[row] = there
    pos_h = pos.cpu().numpy()
    assert R.keys_ref(pos_h[row:row + 1], w.N, R.L, w.T)[0]//8 != w.keys[ids[row]]//8
    w.write(w.phi(0))
    mom = m0.clone()
    mesh.gather_kick_tiled(pos, mom, table, order, w.factor)
    w.check_kick(mom.cpu().numpy(), pos_h, w.mom(order)[ids], 0, order, 'mode 0 stray')
    assert mesh.error_flags() == 0
    keep = pos.clone(), m0.clone()
    out = Fused(w, True).run((pos, m0, i0, w.aux_dev[i0], table, None), order, False)
    assert out.flags & lib.CG_ERR_NOT_IN_TILE, out.flags
    assert torch.equal(pos, keep[0]) and torch.equal(m0, keep[1])


# (N, T of the single domain, domains, tile extent of a slab, tile rows of a slab)
SLABS = [(16, 8, 2, 8, 1), (24, 8, 2, 4, 3), (48, 16, 3, 16, 1)]


@pytest.mark.parametrize('N,T,P,Ts,ntx', SLABS, ids=lambda v: str(v))
def test_deposit_ghost_row_of_slab_contexts(N, T, P, Ts, ntx):
    """k_deposit_cic_pull on x-slab contexts (non-periodic xmap, in one process as
    test_gpu_slab_handover.py makes them): the extra tile row ta == ntx writes the first ghost
    layer only, the row below the first one is another domain's.  Each slab sorts the whole box
    (it keeps what it owns), deposits, and the layers are summed the way the hand-over does: a
    slab's first ghost layer is added to the next slab's first layer.  Same reference, same bar."""
    import torch
    from concept_amd.mesh import PotentialMesh
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    placed, _ = placed_input(N, T)
    dens, (m, mag) = density_ref(N, T)
    n = placed['pos'].shape[0]
    pos, mom = (torch.tensor(placed[k], device='cuda') for k in ('pos', 'mom'))
    ids = torch.arange(n, device='cuda')
    slabs = [PotentialMesh(N, R.L, nprocs=P, rank=r) for r in range(P)]
    try:
        total = np.zeros((N, N, N), dtype=R.LD)
        kept_all = 0
        for times, accumulate in ((1, False), (2, True)):
            total[:] = 0
            for s in slabs:
                assert (s.tile_extent, s.nxl//s.tile_extent, s.tiles_per_dim) == (Ts, ntx, N//Ts)
                G, nxl, per = s.ghost_layers, s.nxl, s.layer_doubles
                assert G >= 1 and s.x0 == s.rank*nxl
                if not accumulate:
                    s.layers_write(-G, nxl + 2*G, torch.full(((nxl + 2*G)*per,), math.nan,
                                                             dtype=torch.float64, device='cuda'))
                po, mo, io = torch.empty_like(pos), torch.empty_like(mom), torch.empty_like(ids)
                table = s.sort_particles(pos, mom, ids, po, mo, io)
                kept = int(table[-1])
                kept_all += kept
                s.deposit_tiled(po[:kept], table, CONTRIBUTION, accumulate=accumulate)
                buf = torch.empty((nxl + 2*G)*per, dtype=torch.float64, device='cuda')
                s.layers_read(-G, nxl + 2*G, buf)
                assert s.error_flags() == 0
                lay = buf.cpu().numpy().reshape(nxl + 2*G, per)
                inside = np.zeros(lay.shape, dtype=bool)
                inside[:, :N*s.pad].reshape(-1, N, s.pad)[G:G + nxl + 1, :, :N] = True
                assert np.isnan(lay[~inside]).all(), \
                    (N, P, s.rank, 'padding or a ghost layer beyond the first was written')
                cells = lay[:, :N*s.pad].reshape(-1, N, s.pad)[G:G + nxl + 1, :, :N]
                assert np.isfinite(cells).all(), (N, P, s.rank, 'a cell was not written')
                total[s.x0:s.x0 + nxl] += cells[:nxl]
                total[(s.x0 + nxl) % N] += cells[nxl]
            ratio = density_ratio(total, times, dens, m, mag, 'slabs')
            print(f'N {N} P {P} T {Ts} x {ntx} rows, slab deposit '
                  f'{"accumulate" if accumulate else "assign"}: worst error/bar {ratio:.3f}')
            assert ratio <= 1, (N, P, Ts, accumulate, ratio)
        assert kept_all == 2*n      # every particle is owned by exactly one slab
    finally:
        for s in slabs:
            s.close()
