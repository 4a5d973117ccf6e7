"""The gate of the particle entries (cg_internal.h) on the GPU, entry by entry.

Deferred pass: substep_begin(defer=True) followed by an entry gives what the pass run at once
followed by the entry gives — the particle arrays bit for bit, and so the entry's output (the
stream is in order: the arrays alone would be equal whichever ran first).  Outputs that do not
depend on an order of atomics are compared bit for bit, deposits and sweeps to 1e-12 of their
maximum; for those the same entry on the arrays WITHOUT the pass must be off by more than 1e-3 of
the maximum, so that the tolerance cannot hide a pass that ran late (for the deposit this margin
is also shown on the host with numpy).

Prepared histogram: gather_kick_tiled_prepare, a write-kind entry on the same pos / mom, then
drift_sort — the tile table and the rows of every tile are those of a context where nothing was
prepared.

16^3 cells, 3001 particles (the last workgroup of 256 is partial; lpt_displace takes its 16^3),
N_rungs = 4, a drift of 2.5 cells per unit of momentum.

Left out: emigrant_dest, emigrant_rows_dest and prepare_rebind (what they return on one domain
does not depend on the positions), shortrange_sweep_cells_active (its list is tied to the rung
array it was made with, and making it adopts the pass)."""
import types

import numpy as np
import pytest

G, L, N_RUNGS, DTM, DTM_NEXT, NT = 16, 16.0, 4, 2.5, 0.7, 4
RF_UP, RF_DOWN = 1.3, 2.1
INTEGRALS = np.random.default_rng(3).uniform(0.1, 1.0, 3*N_RUNGS - 1)
CONV = np.random.default_rng(4).uniform(0.5, 2.0, 3*N_RUNGS - 1)
R2_MAX, R2_SCALING, TABLESIZE = 4.0, 16.0, 66


def host_particles(n):
    rng = np.random.default_rng(n)
    pos = rng.random((n, 3))*L*(1 - 1e-13)
    mom = rng.standard_normal((n, 3))
    acc = rng.standard_normal((n, 3))*np.exp(4*rng.standard_normal((n, 1)))
    rung = rng.integers(0, N_RUNGS, n).astype(np.int8)
    return pos, mom, acc, rung


def cic_host(pos):
    """plain CIC deposit of unit masses on the cell-centred 16^3 lattice"""
    rho = np.zeros((G, G, G))
    x = pos*(G/L) - 0.5
    i0 = np.floor(x).astype(np.int64)
    w1 = x - i0
    for a in range(8):
        d = np.array([(a >> 2) & 1, (a >> 1) & 1, a & 1])
        w = np.prod(np.where(d, w1, 1 - w1), axis=1)
        i = (i0 + d) % G
        np.add.at(rho, (i[:, 0], i[:, 1], i[:, 2]), w)
    return rho


def test_a_late_pass_shows_in_the_deposit_on_the_host():
    pos, mom, _, _ = host_particles(3001)
    a, u = cic_host((pos + mom*DTM) % L), cic_host(pos)
    assert abs(a.sum() - 3001) < 1e-9
    assert np.abs(u - a).max() > 1e-3*np.abs(a).max()
    assert np.abs(mom*DTM).mean() > 1.0*L/G      # a typical particle moves more than a cell


@pytest.fixture(scope='module')
def env():
    import torch
    from concept_amd.mesh import PotentialMesh
    e = types.SimpleNamespace(mesh=PotentialMesh(G, L), other=PotentialMesh(G, L), cases={})
    rng = np.random.default_rng(11)
    e.field = torch.from_numpy(rng.standard_normal(G*e.mesh.layer_doubles)).cuda()
    r2 = (torch.arange(TABLESIZE, dtype=torch.float64, device='cuda') + 0.5)/R2_SCALING
    e.table = -(r2 + 0.05)**-1.5
    e.factors = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 2.0, 3*N_RUNGS - 1)).cuda()
    yield e
    e.mesh.close()
    e.other.close()


def case(e, n, lowest):
    """n particles whose rows are ordered so that the DRIFTED positions are in exact tile order
    (table), and the cell list of the drifted positions; made once, never written"""
    import torch
    if (n, lowest) not in e.cases:
        pos, mom, acc, rung = (torch.from_numpy(a).cuda() for a in host_particles(n))
        drifted = pos.clone()
        e.mesh.drift(drifted, mom, DTM)
        ids = torch.arange(n, device='cuda')
        c = types.SimpleNamespace(n=n, lowest=lowest, drifted=torch.empty_like(pos))
        perm = torch.empty_like(ids)
        c.table = e.mesh.sort_particles(drifted, mom, ids, c.drifted, torch.empty_like(mom), perm)
        c.pos, c.mom, c.dmom, c.rung = (t[perm].contiguous() for t in (pos, mom, acc, rung))
        c.count = (c.table[1:] - c.table[:-1]).contiguous()
        c.cells = e.mesh.shortrange_cells(c.drifted, NT, L/NT)
        e.cases[n, lowest] = c
    return e.cases[n, lowest]


def fresh(c):
    import torch
    return types.SimpleNamespace(
        c=c, pos=c.pos.clone(), mom=c.mom.clone(), dmom=c.dmom.clone(), rung=c.rung.clone(),
        jumped=c.rung.clone(), any_out=torch.zeros(1, dtype=torch.int32, device='cuda'))


ARRAYS = ('pos', 'mom', 'dmom', 'rung', 'jumped', 'any_out')


def the_pass(mesh, s, defer):
    mesh.substep_begin(s.pos, s.mom, s.dmom, s.rung, s.jumped, DTM, True, s.c.lowest, INTEGRALS,
                       RF_UP, RF_DOWN, N_RUNGS, s.any_out, defer=defer)


def by_bucket(table, ids):
    """the sorted (bucket, id) keys of rows stored bucket after bucket: who is where, whatever
    order the atomics gave the rows inside a bucket"""
    import torch
    bucket = torch.repeat_interleave(torch.arange(table.numel() - 1, device='cuda'),
                                     (table[1:] - table[:-1]).long())
    return torch.sort(bucket*(ids.numel() + 1) + ids.long()[:bucket.numel()]).values


def mesh_of(e):
    import torch
    return torch.from_numpy(e.mesh.fetch_real())


def fill(e):
    e.mesh.layers_write(0, G, e.field)


# ---- the entries: f(e, s) -> what the entry returns, as a list of tensors ----
def deposit(e, s):
    e.mesh.zero()
    e.mesh.deposit(s.pos, 1.0)
    return [mesh_of(e)]


def deposit_tiled(e, s):
    e.mesh.deposit_tiled(s.pos, s.c.table, 1.0)
    return [mesh_of(e)]


def deposit_regions(e, s):
    e.mesh.deposit_regions(s.pos, s.c.table, s.c.count, 1.0)
    return [mesh_of(e)]


def deposit_general(e, s):
    e.mesh.zero()
    e.mesh.deposit_general(s.pos, 1.0, 3)
    return [mesh_of(e)]


def gather_kick(e, s):
    fill(e)
    e.mesh.gather_kick(s.pos, s.mom, 2, 0.3)
    return []


def gather_kick_tiled(e, s):
    fill(e)
    e.mesh.gather_kick_tiled(s.pos, s.mom, s.c.table, 2, 0.3)
    return []


def gather_kick_tiled_prepare(e, s):
    fill(e)
    e.mesh.gather_kick_tiled_prepare(s.pos, s.mom, s.c.table, 2, 0.3, DTM_NEXT)
    return []


def gather_kick_drift_scatter(e, s):
    import torch
    fill(e)
    m, c = e.mesh, s.c
    cap = m.region_capacity(c.n)
    start_out, count_out = m.new_region_table()
    m.predict_regions(c.table, c.count, start_out)
    pos_out = torch.zeros((cap, 3), dtype=torch.float64, device='cuda')
    mom_out, ids_out = torch.zeros_like(pos_out), torch.full((cap,), -1, device='cuda')
    m.gather_kick_drift_scatter(s.pos, s.mom, torch.arange(c.n, device='cuda'), c.table, c.count,
                                pos_out, mom_out, ids_out, start_out, count_out, 2, 0.3, DTM_NEXT)
    rows = torch.nonzero(ids_out >= 0)[:, 0]
    rows = rows[torch.argsort(ids_out[rows])]       # by identifier: the order is the atomics'
    return [count_out, ids_out[rows], pos_out[rows], mom_out[rows]]


def gather_scalar(e, s):
    fill(e)
    e.mesh.gather_scalar(s.pos, s.mom, 1, 3, (0.0, 0.0, 0.0), 0.3)
    return []


def drift(e, s):
    e.mesh.drift(s.pos, s.mom, 0.2)
    return []


def measure_momentum(e, s):
    import torch
    return [torch.tensor(e.mesh.measure_momentum(s.mom))]


def measure_momentum_regions(e, s):
    import torch
    return [torch.tensor(e.mesh.measure_momentum_regions(s.mom, s.c.table, s.c.count))]


def _sort(e, s, dtm):
    import torch
    ids = torch.arange(s.c.n, device='cuda')
    po, mo, io = torch.empty_like(s.pos), torch.empty_like(s.mom), torch.empty_like(ids)
    if dtm is None:
        table = e.mesh.sort_particles(s.pos, s.mom, ids, po, mo, io)
    else:
        table = e.mesh.drift_sort(s.pos, s.mom, ids, po, mo, io, dtm)
    back = torch.argsort(io)
    return [table, by_bucket(table, io), po[back], mo[back]]


def sort_particles(e, s):
    return _sort(e, s, None)


def drift_sort(e, s):
    return _sort(e, s, DTM_NEXT)


def owner_rank(e, s):
    return [e.mesh.owner_rank(s.pos)]


def owner_rank_drifted(e, s):
    return [e.mesh.owner_rank_drifted(s.pos, s.mom, DTM_NEXT)]


def cic_indices(e, s):
    return [e.mesh.cic_indices(s.pos), e.mesh.cic_indices(s.pos, True)]


def permute_rows(e, s):
    import torch
    perm = torch.arange(s.c.n - 1, -1, -1, device='cuda')
    out = [torch.zeros_like(s.pos), torch.zeros_like(s.jumped)]
    e.mesh.permute_rows(perm, [(s.pos, out[0]), (s.jumped, out[1])])
    return out


def shortrange_tiles(e, s):
    order, offset, pos_sorted = e.mesh.shortrange_tiles(s.pos, NT, L/NT)
    return [offset, by_bucket(offset, order), (pos_sorted - s.pos[order.long()]).abs().max()]


def sweep_cells(e, s):          # (the list of the drifted positions; the pass nullifies Δmom)
    e.mesh.shortrange_sweep_cells(s.c.cells, s.dmom, s.c.cells, NT, e.table, R2_SCALING, R2_MAX,
                                  0.3)
    return []


def sweep_cells_rungs(e, s):
    e.mesh.shortrange_sweep_cells(s.c.cells, s.dmom, s.c.cells, NT, e.table, R2_SCALING, R2_MAX,
                                  0.0, (e.factors, s.rung, s.jumped, s.c.lowest))
    return []


def shortrange_sparse(e, s):
    import torch
    active = torch.tensor([5, 0, -1, s.c.n - 1, 1234], device='cuda')
    e.mesh.shortrange_sparse(s.pos, active, s.dmom, s.pos, e.table, R2_SCALING, R2_MAX, 0.3)
    return []


def pp_kick(e, s):
    e.mesh.pp_kick(s.pos, s.dmom, s.pos, True, None, 0.05, 'plummer', 0.3)
    return []


def dmom_nullify(e, s):
    e.mesh.dmom_nullify(s.dmom, s.rung, 1)
    return []


def dmom_apply(e, s):
    e.mesh.dmom_apply(s.mom, s.dmom, s.rung, s.c.lowest)
    return []


def dmom_to_acc(e, s):
    import torch
    e.mesh.dmom_to_acc(s.dmom, s.rung, s.jumped, s.c.lowest, torch.from_numpy(CONV).cuda(), True)
    return []


def assign_rungs(e, s):
    e.mesh.assign_rungs(s.dmom, s.rung, s.jumped, 0.7, N_RUNGS)
    return []


def flag_rung_jumps(e, s):
    import torch
    flagged = e.mesh.flag_rung_jumps(s.dmom, s.rung, s.jumped, s.c.lowest,
                                     torch.from_numpy(INTEGRALS).cuda(), RF_UP, RF_DOWN, N_RUNGS)
    return [torch.tensor(flagged)]


def apply_rung_jumps(e, s):
    e.mesh.apply_rung_jumps(s.rung, s.jumped, N_RUNGS)
    return []


def substep_begin(e, s):
    e.mesh.substep_begin(s.pos, s.mom, None, s.rung, s.jumped, 0.3, False, s.c.lowest, None, 0.0,
                         0.0, N_RUNGS, s.any_out)
    return []


def substep_begin_deferred(e, s):
    e.mesh.substep_begin(s.pos, s.mom, None, s.rung, s.jumped, 0.3, False, s.c.lowest, None, 0.0,
                         0.0, N_RUNGS, s.any_out, defer=True)
    return []


def _substep_end(e, s, apply):
    import torch
    counts = torch.zeros(N_RUNGS, dtype=torch.int64, device='cuda')
    e.mesh.substep_end(s.mom, s.dmom, s.rung, s.jumped, apply, s.c.lowest, CONV, N_RUNGS, counts)
    return [counts]


def substep_end(e, s):
    return _substep_end(e, s, False)


def substep_end_apply(e, s):
    return _substep_end(e, s, True)


def rung_populations(e, s):
    return [e.mesh.rung_populations(s.rung, N_RUNGS)]


def lpt_displace(e, s):
    fill(e)
    e.mesh.lpt_displace(s.pos, s.mom, 0, 0.5, 0.25)
    return []


def region_insert(e, s):
    """five rows into five buckets whose last row is declared free: at the place of a particle of
    the same bucket, with a momentum that takes them elsewhere"""
    import torch
    c = s.c
    count = c.count.clone()
    k = torch.nonzero(count > 0)[:5, 0]
    j = c.table[k].long()
    count[k] -= 1
    rows = torch.zeros((5, 8), dtype=torch.float64, device='cuda')
    rows[:, 0:3], rows[:, 3:6] = c.drifted[j], 7.0 - c.mom[j]
    e.mesh.region_insert(rows, c.table, count, s.pos, s.mom, None, None, c.n)
    return [count]


def prepare_invalidate(e, s):
    s.mom += 1.0                        # (written outside the library)
    e.mesh.prepare_invalidate()
    return []


EXACT, MESH, SWEEP = 'exact', 'mesh', 'sweep'
DEFERRED = [(f, EXACT) for f in (
    gather_kick, gather_kick_tiled, gather_kick_tiled_prepare, gather_kick_drift_scatter,
    gather_scalar, drift, measure_momentum, measure_momentum_regions, sort_particles, drift_sort,
    owner_rank, owner_rank_drifted, cic_indices, permute_rows, shortrange_tiles,
    shortrange_sparse, pp_kick, dmom_nullify, dmom_apply, dmom_to_acc, assign_rungs,
    flag_rung_jumps, apply_rung_jumps, substep_begin, substep_end, substep_end_apply,
    rung_populations, lpt_displace, region_insert)]
DEFERRED += [(f, MESH) for f in (deposit, deposit_tiled, deposit_regions, deposit_general)]
DEFERRED += [(f, SWEEP) for f in (sweep_cells, sweep_cells_rungs)]
WRITERS = [gather_scalar, gather_kick, drift, gather_kick_tiled, gather_kick_tiled_prepare,
           gather_kick_drift_scatter, dmom_apply, substep_end_apply, substep_begin,
           substep_begin_deferred, lpt_displace, region_insert, prepare_invalidate]


def particles_of(f):
    return G**3 if f is lpt_displace else 3001


def close(a, b):
    return float((a - b).abs().max()) <= 1e-12*float(a.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('lowest', [0, 2])
@pytest.mark.parametrize('entry, kind', DEFERRED, ids=[f.__name__ for f, _ in DEFERRED])
def test_a_deferred_pass_runs_before_the_entry(env, entry, kind, lowest):
    import torch
    c = case(env, particles_of(entry), lowest)
    a, b = fresh(c), fresh(c)
    the_pass(env.mesh, a, False)
    out_a = entry(env, a)
    the_pass(env.mesh, b, True)
    try:
        out_b = entry(env, b)
    finally:
        env.mesh.substep_flush()        # (an entry that raised leaves no pass behind)
    flags = env.mesh.error_flags()      # (read, and so cleared, whatever fails below)
    assert torch.equal(a.pos, c.drifted) or entry in (drift, substep_begin, lpt_displace,
                                                      region_insert)
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert close(x, y) if (kind == SWEEP and name == 'dmom') else torch.equal(x, y), name
    assert len(out_a) == len(out_b)
    for x, y in zip(out_a, out_b):
        assert torch.equal(x, y) if kind == EXACT else close(x, y)
    if kind != EXACT:       # the same entry without the pass is far outside that tolerance
        u = fresh(c)
        out_u = entry(env, u)
        env.mesh.error_flags()          # (these rows are not in the tile order they claim)
        x, y = (a.dmom, u.dmom) if kind == SWEEP else (out_a[0], out_u[0])
        assert float((x - y).abs().max()) > 1e-3*float(x.abs().max())
    assert flags == 0


def tiles_after_the_next_drift(mesh, s):
    import torch
    ids = torch.arange(s.c.n, device='cuda')
    po, mo, io = torch.empty_like(s.pos), torch.empty_like(s.mom), torch.empty_like(ids)
    table = mesh.drift_sort(s.pos, s.mom, ids, po, mo, io, DTM_NEXT)
    return table, by_bucket(table, io)


def prepared(env, entry):
    """prepare, the entry, drift_sort — against the drift_sort of a context that prepared nothing"""
    import torch
    c = case(env, particles_of(entry), 0)
    s = fresh(c)
    s.pos = c.drifted.clone()           # (in tile order as they are)
    fill(env)
    env.mesh.gather_kick_tiled_prepare(s.pos, s.mom, c.table, 2, 0.3, DTM_NEXT)
    entry(env, s)
    table, keys = tiles_after_the_next_drift(env.mesh, s)
    table_plain, keys_plain = tiles_after_the_next_drift(env.other, s)
    flags = env.mesh.error_flags()      # (read, and so cleared, whatever fails below)
    assert int(table[-1]) == c.n
    assert torch.equal(table, table_plain) and torch.equal(keys, keys_plain)
    assert flags == 0


@pytest.mark.gpu
@pytest.mark.parametrize('entry', WRITERS, ids=[f.__name__ for f in WRITERS])
def test_a_write_voids_the_prepared_histogram(env, entry):
    prepared(env, entry)


@pytest.mark.gpu
def test_a_read_leaves_the_prepared_histogram_to_the_sort(env):
    prepared(env, measure_momentum)
