"""Host logic of shortrange.component_component and distributed.shortrange_kick (no GPU): which
of the four sweeps kicks a receiver (no cell list / by active receiver / in blocks / plain),
which cell list is built for whom and when, the boundary suppliers of several domains, the
deferred substep_begin and the CG_ERR_ACTIVE_OVERFLOW check.  get_mesh is replaced by a
recording stub, the components are namespaces of small CPU tensors; the whole sequence of calls
is compared with literal lists, and every factor with the expression written out here in the
reference's order (compute_factors, gravity.py:51-64), bit for bit.

The lists are those component_component gave on the same stubs before the dispatch moved into
shortrange.sweep_form: every case here passed against that version too.

Rows: 40 per component, where 8 active rows and 16 % of the rows (6.4) are different
thresholds — but 16 % lies below 8 there, so the sweep by active receiver is reached with 100
rows (9..16 active), or with 40 rows once the sweep without a list is kept to 4 rows."""
import types

import pytest
import torch

BOX, GRID, NT = 100.0, 32, 10
SR = {'scale': 1.6, 'range': 8.0, 'tilesize': 10.0, 'subtiling': 'automatic', 'tablesize': 4096}
EXT = BOX/NT
MAXR2 = (1 + 1/4096)*8.0**2
SCALING, R2_MAX = (4096 - 1)/MAXR2, 8.0**2
G = 4.3e-9
MASS = {'A': 1.7, 'B': 0.43}
SOFT = {'A': 0.03, 'B': 0.05}
KEY = 'a**(-3*w_eff₀-3*w_eff₁-1)'
N_RUNGS = 4
INTEGRALS = [0.0173, 0.0087, 0.0044, 0.0021, 0.0, 0.013, 0.0065, 0.0033, 0.0, 0.0131, 0.0066]
LOWEST = 2  # the lowest active rung of the sub-step cases


def factors(rec, sup):
    """compute_factors (gravity.py:51-64): G*m_r*m_s*ᔑdt_rungs[...][k] in that order"""
    return ('factors', tuple(G*MASS[rec]*MASS[sup]*v for v in INTEGRALS))


def sdt(*names):
    return {(KEY, r, s): list(INTEGRALS) for r in names for s in names}


class Env:
    """the stubs of one case and the log they write"""

    def __init__(self, monkeypatch, nprocs=1, sr=None):
        from concept_amd import commons, distributed, shortrange
        from concept_amd.mesh import PotentialMesh
        self.log, self.names, self.lists = [], {}, 0
        self.shortrange, self.distributed = shortrange, distributed
        self.params = types.SimpleNamespace(
            boxsize=BOX, nghosts=2, cell_centered=True, G_Newton=G, softening_kernel='spline',
            shortrange_params={'gravity': dict(sr or SR)}, units=types.SimpleNamespace())
        env, log = self, self.log

        class StubMesh:
            name, dist, boxsize, gridsize, nxl = 'mesh', nprocs > 1, BOX, GRID, GRID//nprocs
            # the thresholds are the class's (tests patch them there)
            SHORTRANGE_SPARSE_MAX = property(lambda self: PotentialMesh.SHORTRANGE_SPARSE_MAX)
            SHORTRANGE_BY_CELL_MAX = property(lambda self: PotentialMesh.SHORTRANGE_BY_CELL_MAX)

            def __init__(self):
                self.nprocs = nprocs

            def shortrange_cells(self, pos, nt, tile_extent, rungs=None, sorted_jumps=False):
                log.append(('cells', env.nm(pos), nt, tile_extent, env.nm(rungs), sorted_jumps))
                env.lists += 1
                return f'L{env.lists - 1}'

            def shortrange_sweep_cells(self, cells_r, dmom_r, cells_s, nt, table,
                                       r2_index_scaling, r2_max, factor, rungs=None,
                                       n_active=None):
                log.append(('sweep', cells_r, env.nm(dmom_r), cells_s, nt, table,
                            r2_index_scaling, r2_max, factor, env.nm(rungs), n_active))

            def shortrange_sparse(self, pos_r, active, dmom_r, pos_s, table, r2_index_scaling,
                                  r2_max, factor, rungs=None, overflow_slot=False):
                log.append(('sparse', env.nm(pos_r), tuple(active.tolist()), env.nm(dmom_r),
                            env.nm(pos_s), table, r2_index_scaling, r2_max, factor,
                            env.nm(rungs), overflow_slot))

            def check_errors(self):
                log.append(('check_errors',))

        self.mesh = StubMesh()

        def get_mesh(gridsize, boxsize, nghosts=2, cell_centered=True, interp_order=2,
                     device=None, role='global'):
            assert (gridsize, boxsize, nghosts, cell_centered, interp_order, str(device), role) \
                == (GRID, BOX, 2, True, 2, 'cpu', 'global')
            return self.mesh

        def table(softening, scale, range_, tablesize, kernel, device):
            log.append(('table', softening, scale, range_, tablesize, kernel, str(device)))
            return 'table', MAXR2

        def upload(values, device, dtype=None):
            log.append(('upload', str(device)))
            return ('factors', tuple(values.tolist()))

        def ship(mesh, pos, margin):
            log.append(('ship', mesh.name, env.nm(pos), margin))
            return self.ghosts[mesh.name]

        def fits(mesh, range_):
            log.append(('fits', mesh.name, range_))
        monkeypatch.setattr(shortrange, 'get_mesh', get_mesh)
        monkeypatch.setattr(shortrange, 'get_shortrange_table', table)
        monkeypatch.setattr(commons, 'upload', upload)
        monkeypatch.setattr(distributed, 'ship_boundary_positions', ship)
        monkeypatch.setattr(distributed, 'check_shortrange_fits', fits)
        shortrange.by_receiver_meshes.clear()
        self.sparse0 = shortrange.sparse_sweeps
        self.ghosts = {}

    def nm(self, x):
        """tensors by the name they were registered under (others by their rows)"""
        if isinstance(x, torch.Tensor):
            return self.names.get(id(x)) or ('rows', tuple(map(tuple, x.tolist())))
        if isinstance(x, tuple) and x[:1] != ('factors',):
            return tuple(self.nm(v) for v in x)
        return x

    def component(self, name, n=40, active=None, rungs=True, deferred=False, grid=GRID,
                  representation='particles', has_dmom=True):
        """`active`: how many rows (the odd ones first) sit on rung LOWEST, which then is the
        lowest active rung; None: every rung is active"""
        gen = torch.Generator().manual_seed(len(name) + n)
        log = self.log
        c = types.SimpleNamespace(
            name=name, representation=representation, params=self.params, device='cpu',
            mass=MASS[name], softening_length=SOFT[name], use_rungs=rungs, N_rungs=N_RUNGS, N=n,
            pos=torch.rand((n, 3), generator=gen, dtype=torch.float64)*BOX,
            mom=torch.zeros((n, 3), dtype=torch.float64),
            rung_indices=torch.zeros(n, dtype=torch.int8),
            rung_indices_jumped=torch.zeros(n, dtype=torch.int8),
            lowest_active_rung=0 if active is None else LOWEST, rungs_N=[n, 0, 0, 0])
        if active is not None:
            c.rung_indices[1:2*active:2] = LOWEST
            c.rungs_N = [n - active, 0, active, 0]
        c._store = types.SimpleNamespace(
            cols={'Δmom': None} if has_dmom else {},
            mesh=types.SimpleNamespace(name=f'{name}.mesh', boxsize=BOX, gridsize=grid,
                                       nprocs=self.mesh.nprocs))
        if has_dmom:
            c.Δmom = torch.zeros((n, 3), dtype=torch.float64)

        def take_begin(mesh):
            assert mesh is self.mesh
            log.append((name, 'take_begin'))
            return deferred
        c.take_begin = take_begin
        c.begin_queued = lambda: log.append((name, 'begin_queued'))
        c.flush_begin = lambda: log.append((name, 'flush_begin'))
        for attr, short in (('pos', 'pos'), ('Δmom', 'Δmom'), ('rung_indices', 'rung'),
                            ('rung_indices_jumped', 'jumped')):
            if hasattr(c, attr):
                self.names[id(getattr(c, attr))] = f'{name}.{short}'
        self.ghosts[f'{name}.mesh'] = (torch.full((1, 3), 1.5, dtype=torch.float64),
                                       torch.full((2, 3), 97.5, dtype=torch.float64))
        return c

    def run(self, receivers, suppliers, ᔑdt=None, force='gravity'):
        ᔑdt = ᔑdt if ᔑdt is not None else sdt(*{c.name for c in receivers + suppliers})
        self.shortrange.component_component(force, receivers, suppliers, ᔑdt, GRID)
        return self.log

    @property
    def sparse_sweeps(self):
        return self.shortrange.sparse_sweeps - self.sparse0


def table_call(r, s):
    return ('table', 0.5*(SOFT[r] + SOFT[s]), 1.6, 8.0, 4096, 'spline', 'cpu')


def rungs_of(rec, sup, lowest):
    return (factors(rec, sup), f'{rec}.rung', f'{rec}.jumped', lowest)


def sweep(cells_r, rec, cells_s, sup, lowest, n_active=None):
    """a rung sweep as the mesh sees it"""
    return ('sweep', cells_r, f'{rec}.Δmom', cells_s, NT, 'table', SCALING, R2_MAX, 0.0,
            rungs_of(rec, sup, lowest), n_active)


def rows_slots(active, slots=9):
    """commons.sparse_rows: the active rows (the odd ones first), then -1"""
    rows = tuple(range(1, 2*active, 2))
    return rows + (-1,)*(slots - len(rows))


def test_one_component_without_rungs(monkeypatch):
    env = Env(monkeypatch)
    a = env.component('A', rungs=False)
    assert env.run([a], [a], {(KEY, 'A', 'A'): 0.0173}) == [
        table_call('A', 'A'),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, None, False),
        ('sweep', 'L0', 'A.Δmom', 'L0', NT, 'table', SCALING, R2_MAX, G*1.7*1.7*0.0173, None,
         None),
    ]
    assert env.shortrange.by_receiver_meshes == {} and env.sparse_sweeps == 0


def test_missing_dmom_is_made_without_reading_it(monkeypatch):
    env = Env(monkeypatch)
    a = env.component('A', rungs=False, has_dmom=False)
    log = env.run([a], [a])
    assert torch.equal(a.Δmom, torch.zeros_like(a.mom)) and a.Δmom is not a.mom
    assert log[-1][0] == 'sweep' and log[-1][2] == ('rows', ((0.0, 0.0, 0.0),)*40)


def test_rungs_all_active(monkeypatch):
    env = Env(monkeypatch)
    a = env.component('A')
    assert env.run([a], [a]) == [
        table_call('A', 'A'),
        ('upload', 'cpu'),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', 0), False),
        sweep('L0', 'A', 'L0', 'A', 0),
    ]
    assert env.shortrange.by_receiver_meshes == {} and env.sparse_sweeps == 0


@pytest.mark.parametrize('active', [0, 1, 8])
def test_sparse_up_to_8_active_rows(active, monkeypatch):
    env = Env(monkeypatch)
    a = env.component('A', n=100, active=active)
    assert env.run([a], [a]) == [
        table_call('A', 'A'),
        ('upload', 'cpu'),
        ('A', 'flush_begin'),
        ('A', 'flush_begin'),
        ('sparse', 'A.pos', rows_slots(active), 'A.Δmom', 'A.pos', 'table', SCALING, R2_MAX, 0.0,
         (factors('A', 'A'), 'A.jumped'), True),
        ('check_errors',),
    ]
    assert env.sparse_sweeps == 1
    assert env.shortrange.by_receiver_meshes == {}  # (entered, then taken by the check)


def test_sparse_enters_the_mesh_and_flushes_both_partners(monkeypatch):
    env = Env(monkeypatch)
    a, b = env.component('A', active=8), env.component('B', active=3)
    with env.shortrange.deferred_active_checks():
        log = env.run([a], [b])
    assert log == [
        table_call('A', 'B'),
        ('upload', 'cpu'),
        ('A', 'flush_begin'),
        ('B', 'flush_begin'),
        ('sparse', 'A.pos', rows_slots(8), 'A.Δmom', 'B.pos', 'table', SCALING, R2_MAX, 0.0,
         (factors('A', 'B'), 'A.jumped'), True),
    ]
    assert env.sparse_sweeps == 1
    assert env.shortrange.by_receiver_meshes == {id(env.mesh): env.mesh}


def test_by_cell_from_9_active_rows(monkeypatch):
    env = Env(monkeypatch)
    a = env.component('A', n=100, active=9)
    assert env.run([a], [a]) == [
        table_call('A', 'A'),
        ('upload', 'cpu'),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', LOWEST), False),
        sweep('L0', 'A', 'L0', 'A', LOWEST, 9),
        ('check_errors',),
    ]
    assert env.sparse_sweeps == 0


def by_cell_log(n_active):
    return [
        table_call('A', 'A'),
        ('upload', 'cpu'),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', LOWEST), False),
        sweep('L0', 'A', 'L0', 'A', LOWEST, n_active),
    ]


def blocks_log():
    return [
        table_call('A', 'A'),
        ('upload', 'cpu'),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', LOWEST), True),
        sweep('L0', 'A', 'L0', 'A', LOWEST, None),
    ]


@pytest.mark.parametrize('n, active, sparse_max, form', [
    (40, 6, 4, 'by_cell'), (40, 7, 4, 'blocks'),        # 15 % and 17.5 %
    (100, 16, 8, 'by_cell'), (100, 17, 8, 'blocks')])   # the same with the sparse sweep as it is
def test_active_share_on_both_sides_of_16_percent(n, active, sparse_max, form, monkeypatch):
    from concept_amd.mesh import PotentialMesh
    monkeypatch.setattr(PotentialMesh, 'SHORTRANGE_SPARSE_MAX', sparse_max)
    env = Env(monkeypatch)
    a = env.component('A', n=n, active=active)
    with env.shortrange.deferred_active_checks():
        log = env.run([a], [a])
    if form == 'by_cell':
        assert log == by_cell_log(active)
        assert env.shortrange.by_receiver_meshes == {id(env.mesh): env.mesh}
    else:
        assert log == blocks_log()
        assert env.shortrange.by_receiver_meshes == {}
    assert env.sparse_sweeps == 0


@pytest.mark.parametrize('n, active', [(40, 9), (100, 9), (100, 16), (100, 50)])
def test_by_cell_switched_off_gives_blocks_above_8(n, active, monkeypatch):
    from concept_amd.mesh import PotentialMesh
    monkeypatch.setattr(PotentialMesh, 'SHORTRANGE_BY_CELL_MAX', -1.0)
    env = Env(monkeypatch)
    a = env.component('A', n=n, active=active)
    assert env.run([a], [a]) == blocks_log()   # (and no check: no sweep bounded by the counts)
    assert env.shortrange.by_receiver_meshes == {} and env.sparse_sweeps == 0


def test_two_components_kick_each_other(monkeypatch):
    env = Env(monkeypatch)
    a, b = env.component('A'), env.component('B')
    assert env.run([a, b], [a, b]) == [
        table_call('A', 'A'),
        ('upload', 'cpu'),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', 0), False),
        sweep('L0', 'A', 'L0', 'A', 0),
        table_call('A', 'B'),
        ('upload', 'cpu'),
        ('B', 'take_begin'),
        ('cells', 'B.pos', NT, EXT, ('B.rung', 'B.jumped', 0), False),
        sweep('L0', 'A', 'L1', 'B', 0),
        ('upload', 'cpu'),
        sweep('L1', 'B', 'L0', 'A', 0),
        table_call('B', 'B'),
        ('upload', 'cpu'),
        sweep('L1', 'B', 'L1', 'B', 0),
    ]


def test_two_components_without_rungs_receiver_first(monkeypatch):
    env = Env(monkeypatch)
    a, b = env.component('A', rungs=False), env.component('B', rungs=False)
    f = lambda r, s: G*MASS[r]*MASS[s]*float(INTEGRALS[0])  # noqa: E731

    def plain(cells_r, rec, cells_s, sup):
        return ('sweep', cells_r, f'{rec}.Δmom', cells_s, NT, 'table', SCALING, R2_MAX,
                f(rec, sup), None, None)
    assert env.run([a, b], [b, a]) == [
        table_call('A', 'B'),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, None, False),
        ('B', 'take_begin'),
        ('cells', 'B.pos', NT, EXT, None, False),
        plain('L0', 'A', 'L1', 'B'),
        plain('L1', 'B', 'L0', 'A'),
        table_call('A', 'A'),
        plain('L0', 'A', 'L0', 'A'),
        table_call('B', 'B'),
        plain('L1', 'B', 'L1', 'B'),
    ]


def test_supplier_that_is_no_receiver_gets_a_plain_list(monkeypatch):
    env = Env(monkeypatch)
    a, b = env.component('A', active=20), env.component('B', active=20)
    assert env.run([a], [b]) == [
        table_call('A', 'B'),
        ('upload', 'cpu'),
        ('B', 'take_begin'),
        ('cells', 'B.pos', NT, EXT, None, False),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', LOWEST), True),
        sweep('L1', 'A', 'L0', 'B', LOWEST, None),
    ]


def test_deferred_begin_is_reported_queued_after_the_build(monkeypatch):
    env = Env(monkeypatch)
    a, b = env.component('A', active=20, deferred=True), env.component('B', active=20)
    assert env.run([a], [b]) == [
        table_call('A', 'B'),
        ('upload', 'cpu'),
        ('B', 'take_begin'),
        ('cells', 'B.pos', NT, EXT, None, False),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', LOWEST), True),
        ('A', 'begin_queued'),
        sweep('L1', 'A', 'L0', 'B', LOWEST, None),
    ]


def test_two_domains(monkeypatch):
    env = Env(monkeypatch, nprocs=2)
    a, b = env.component('A', active=3, grid=32), env.component('B', active=3, grid=16)
    slack = max(BOX/32, BOX/16)
    margin = 8.0*(1 + 1e-9) + slack + 1e-9*BOX
    extended = lambda c: ('rows', tuple(map(tuple, torch.cat(  # noqa: E731
        [c.pos, torch.full((1, 3), 1.5, dtype=torch.float64),
         torch.full((2, 3), 97.5, dtype=torch.float64)]).tolist())))
    assert env.run([a], [b]) == [
        ('fits', 'A.mesh', 8.0 + slack),
        ('fits', 'B.mesh', 8.0 + slack),
        ('A', 'take_begin'),
        ('cells', 'A.pos', NT, EXT, ('A.rung', 'A.jumped', LOWEST), False),
        ('ship', 'A.mesh', 'A.pos', margin),
        ('cells', extended(a), NT, EXT, None, False),
        ('B', 'take_begin'),
        ('cells', 'B.pos', NT, EXT, None, False),
        ('ship', 'B.mesh', 'B.pos', margin),
        ('cells', extended(b), NT, EXT, None, False),
        table_call('A', 'B'),
        ('upload', 'cpu'),
        sweep('L0', 'A', 'L3', 'B', LOWEST, 3),   # by active receiver: no sweep without a list
        ('check_errors',),
    ]
    assert env.sparse_sweeps == 0


@pytest.mark.parametrize('active, checked', [(3, True), (6 + 40, False), (None, False)])
def test_check_outside_deferred_only_after_a_bounded_sweep(active, checked, monkeypatch):
    env = Env(monkeypatch)
    a = env.component('A', n=100, active=active)
    log = env.run([a], [a])
    assert log.count(('check_errors',)) == int(checked)
    assert (log[-1] == ('check_errors',)) == checked
    assert env.shortrange.by_receiver_meshes == {}


@pytest.mark.parametrize('active', [3, 12])
def test_check_inside_deferred_is_left_to_the_caller(active, monkeypatch):
    env = Env(monkeypatch)
    a = env.component('A', n=100, active=active)
    with env.shortrange.deferred_active_checks():
        log = env.run([a], [a])
        log = env.run([a], [a])
    assert ('check_errors',) not in log
    assert env.shortrange.by_receiver_meshes == {id(env.mesh): env.mesh}
    # outside again, the next call looks
    assert env.run([a], [a])[-1] == ('check_errors',)


def test_refusals(monkeypatch):
    from concept_amd.lib import ConceptGPUError
    env = Env(monkeypatch, sr=dict(SR, tilesize=30.0))
    with pytest.raises(ConceptGPUError, match=(
            r'^The global gravity tiling needs to have at least 4 tiles across the box in every '
            r'direction\. Consider lowering shortrange_params\["gravity"\]\["tilesize"\]\.$')):
        env.run([env.component('A')], [env.component('A')])
    env = Env(monkeypatch, sr=dict(SR, range=12.0))
    with pytest.raises(ConceptGPUError,
                       match=r'^shortrange_params: tilesize must be at least the range$'):
        env.run([env.component('A')], [env.component('A')])
    env = Env(monkeypatch)
    a, f = env.component('A'), env.component('B', representation='fluid')
    with pytest.raises(ConceptGPUError,
                       match=r'^B: only particle components have short-range forces$'):
        env.run([a], [f])
    with pytest.raises(ConceptGPUError, match=r'^short-range force "lapse" is not built$'):
        env.run([a], [a], force='lapse')
    assert 'cells' not in [entry[0] for entry in env.log]


def test_shortrange_kick_on_one_domain(monkeypatch):
    env = Env(monkeypatch)
    pos = torch.rand((40, 3), generator=torch.Generator().manual_seed(3),
                     dtype=torch.float64)*BOX
    env.names[id(pos)] = 'pos'
    domain = types.SimpleNamespace(mesh=env.mesh)
    particles = types.SimpleNamespace(view=lambda name: {'pos': pos}[name])
    dmom = env.distributed.shortrange_kick(
        domain, particles, scale=1.6, range_=8.0, tilesize=10.0, tablesize=4096, softening=0.04,
        factor=3e-4)
    assert torch.equal(dmom, torch.zeros((40, 3), dtype=torch.float64))
    assert env.log == [
        ('fits', 'mesh', 8.0),
        ('cells', 'pos', NT, EXT, None, False),
        ('table', 0.04, 1.6, 8.0, 4096, 'spline', 'cpu'),
        ('sweep', 'L0', ('rows', ((0.0, 0.0, 0.0),)*40), 'L0', NT, 'table', (4096 - 1)/MAXR2,
         8.0**2, 3e-4, None, None),
    ]
