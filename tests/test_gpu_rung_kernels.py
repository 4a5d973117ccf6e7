"""The per-particle rung kernels (cg_assign_rungs, cg_flag_rung_jumps, cg_apply_rung_jumps,
cg_dmom_nullify, cg_dmom_apply, cg_dmom_to_acc) and the fused cg_substep_begin / cg_substep_end
against oracle/rungs.py, the numpy restatement of the reference's own functions
(species.py:2253-2587), on the populations of test_rungs_oracle_host.py: the exact edge table,
repeated for every current rung, and random accelerations that stay 1e-2 away from every
decision (host and device log2 may differ by an ulp or two).

Every comparison is exact: the rung arrays are integers, apply_Δmom is one IEEE add per element,
convert_Δmom_to_acc one IEEE multiply, the drift is the oracle's own, and the library is built
with -ffp-contract=off.

The reference's get_rung returns N_rungs, one past the top rung, for f == N_rungs - 1 exactly.
A particle on the top rung with that f is flagged upwards (index 3 N_rungs - 1: 125 with
N_rungs = 42, the most an int8 takes) by the reference, the oracle and the kernels alike; the
separate kernels are run on it.  The fused passes use the jumped index to look up a table of
3 N_rungs - 1 entries, where the reference itself would read one past its end: those rows (and
only those) are left out of the edge table there."""
import numpy as np
import pytest

import test_rungs_oracle_host as host
from oracle import oracle, rungs

pytestmark = pytest.mark.gpu

L = 37.0
RF = 1.5                     # on the half grid: the edge table holds f == 0, k and N_rungs - 1
# (rung_factor_up, rung_factor_down), whole numbers away from RF so that both f are the table's:
# the time loop's hysteresis (stays between the jumps), and an overlap in which a particle can
# qualify for both jumps
ARRANGEMENTS = {'hysteresis': (RF, RF + 1), 'overlap': (RF + 1, RF - 1)}
SIZES = [1, 255, 256, 257, 100003]
CASES = [('edges', 0)] + [('random', n) for n in SIZES]
SENTINEL = 99


@pytest.fixture(scope='module')
def mesh():
    from concept_amd.mesh import PotentialMesh
    m = PotentialMesh(16, L)
    yield m
    m.close()


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def population(kind, n, N_rungs):
    if kind == 'edges':
        acc, rung, f, want = host.edge_table(N_rungs, RF)
        return acc, rung
    acc, rung = host.random_population(10**7*N_rungs + n, n, N_rungs, RF)
    p = host.particles(acc, rung, N_rungs)
    for factor in (RF - 1, RF, RF + 1):
        assert host.distance_from_decisions(p, factor) >= 1e-2
    return acc, rung


def lowest_values(N_rungs):
    return sorted({0, min(1, N_rungs - 1), N_rungs//2, N_rungs - 1})


def integrals_table(N_rungs, seed=5):
    """dt_rungs['1']: zeros on some rungs, -1 (no down-jump) on some rung + N_rungs entries"""
    t = np.random.default_rng(seed).uniform(0.1, 1.0, 3*N_rungs - 1)
    t[1:N_rungs:3] = 0.0                       # (with N_rungs = 4: rung 1 has no kick,
    t[N_rungs + 1:2*N_rungs:2] = -1.0          # rung 3 is locked, rungs 0 and 2 are free)
    return t


def oracle_flag(acc, rung, N_rungs, lowest, integrals, factors):
    p = host.particles(acc, rung, N_rungs)
    p.lowest_active_rung = lowest
    flagged = p.flag_rung_jumps(None, None, None, {rungs.KEY_1: integrals}, factors)
    return p, flagged


def flag_raw(mesh, acc, rung, jumped, lowest, integrals, factors, N_rungs, any_out):
    """cg_flag_rung_jumps with the caller's own any_out"""
    from concept_amd import lib
    lib.check(lib.raw().cg_flag_rung_jumps(
        mesh._ctx, lib._ptr(acc), lib._ptr(rung), lib._ptr(jumped), int(rung.numel()), int(lowest),
        lib._ptr(integrals), float(factors[0]), float(factors[1]), int(N_rungs),
        lib._ptr(any_out)))


@pytest.mark.parametrize('kind,n', CASES)
@pytest.mark.parametrize('N_rungs', [1, 4, 8, 21, 42])
def test_assign_rungs(mesh, N_rungs, kind, n):
    acc, rung = population(kind, n, N_rungs)
    want = host.particles(acc, rung, N_rungs).get_rung(RF)
    if kind == 'edges':
        assert np.array_equal(want, host.edge_table(N_rungs, RF)[3])
        assert N_rungs == 1 or (want == N_rungs).any()       # the reference's 1 + cast(...)
    r, j = gpu(rung), gpu(np.full(rung.size, SENTINEL, dtype=np.int8))
    mesh.assign_rungs(gpu(acc), r, j, RF, N_rungs)
    assert same(r, want)
    assert same(j, want)


@pytest.mark.parametrize('kind,n', CASES)
@pytest.mark.parametrize('N_rungs', [1, 4, 8, 21, 42])
def test_flag_and_apply_rung_jumps(mesh, N_rungs, kind, n):
    acc, rung = population(kind, n, N_rungs)
    integrals = integrals_table(N_rungs)
    acc_t, rung_t, integrals_t = gpu(acc), gpu(rung), gpu(integrals)
    r = rung.astype(np.int64)
    seen = set()
    for name, factors in ARRANGEMENTS.items():
        for lowest in lowest_values(N_rungs):
            p, flagged = oracle_flag(acc, rung, N_rungs, lowest, integrals, factors)
            jumped_t = rung_t.clone()
            got = mesh.flag_rung_jumps(acc_t, rung_t, jumped_t, lowest, integrals_t, *factors,
                                       N_rungs)
            j = jumped_t.cpu().numpy()
            assert np.array_equal(j, p.rung_jumped), (name, lowest)
            assert got == flagged
            assert same(rung_t, rung)
            # what the population holds (from the oracle's own get_rung)
            up, down = j >= 2*N_rungs, (j >= N_rungs) & (j < 2*N_rungs)
            ought_up, ought_down = p.get_rung(factors[0]), p.get_rung(factors[1])
            considered = (r >= lowest) & (integrals[r] != 0)
            locked = integrals[r + N_rungs] == -1
            assert np.array_equal(j[~(up | down)], rung[~(up | down)])   # unflagged: untouched
            assert not (up | down)[~considered].any()
            assert not down[rung == 0].any()
            # (an up flag on the top rung: only the reference's own f == N_rungs - 1)
            f_up = p.rung_index_float(factors[0])[1]
            assert not (up & (rung == N_rungs - 1) & (f_up != N_rungs - 1)).any()
            if lowest == 0:
                for tag, which in (
                        ('up', up), ('down', down),
                        ('locked', considered & ~up & locked & (ought_down < r)),
                        ('both', up & ~locked & (ought_down < r)),
                        ('stay', considered & ~locked & (acc != 0).any(1) & ~up & ~down)):
                    if which.any():
                        seen.add((name, tag))
            if (j == 125).any():
                seen.add('125')
            # apply_rung_jumps on these flags
            r_t = rung_t.clone()
            mesh.apply_rung_jumps(r_t, jumped_t, N_rungs)
            p.apply_rung_jumps()
            assert same(r_t, p.rung) and same(jumped_t, p.rung) and same(r_t, jumped_t)
            moved = up | down
            assert np.array_equal(p.rung[~moved], rung[~moved])
            assert np.array_equal(p.rung[moved], rung[moved] + np.where(up[moved], 1, -1))
    if N_rungs >= 4 and (kind == 'edges' or n == 100003):
        assert seen >= {('hysteresis', 'up'), ('hysteresis', 'down'), ('hysteresis', 'locked'),
                        ('hysteresis', 'stay'), ('overlap', 'both'), ('overlap', 'locked')}
    if N_rungs == 42 and kind == 'edges':
        assert '125' in seen               # 41 + 84: the top rung's f == N_rungs - 1


def test_flag_rung_jumps_any_out(mesh):
    import torch
    N_rungs, n = 8, 1000
    acc, rung = population('random', n, N_rungs)
    factors = ARRANGEMENTS['hysteresis']
    integrals = integrals_table(N_rungs)
    acc_t, rung_t = gpu(acc), gpu(rung)

    def run(acc_t, rung_t, lowest, integrals, before):
        any_out = torch.full((1,), before, dtype=torch.int32, device='cuda')
        jumped = rung_t.clone()
        flag_raw(mesh, acc_t, rung_t, jumped, lowest, gpu(integrals), factors, N_rungs, any_out)
        return int(any_out.item()), jumped

    for before in (0, 1):
        assert oracle_flag(acc, rung, N_rungs, 0, integrals, factors)[1]
        assert run(acc_t, rung_t, 0, integrals, before)[0] == 1
        # no jumps: all integrals 0; no accelerations; every particle below the lowest active rung
        for a, r, lowest, table in ((acc, rung, 0, np.zeros(3*N_rungs - 1)),
                                    (np.zeros_like(acc), rung, 0, integrals),
                                    (acc, np.minimum(rung, 4), 5, integrals)):
            assert not oracle_flag(a, r, N_rungs, lowest, table, factors)[1]
            flag, jumped = run(gpu(a), gpu(r), lowest, table, before)
            assert flag == 0 and same(jumped, r)
        empty = torch.empty((0, 3), dtype=torch.float64, device='cuda')
        assert run(empty, rung_t[:0], 0, integrals, before)[0] == 0
    assert mesh.flag_rung_jumps(empty, rung_t[:0], rung_t[:0].clone(), 0, gpu(integrals),
                                *factors, N_rungs) is False


@pytest.mark.parametrize('n', SIZES)
def test_dmom_nullify_and_apply(mesh, n):
    N_rungs = 8
    rng = np.random.default_rng(n)
    mom = rng.normal(size=(n, 3))*np.exp(3*rng.normal(size=(n, 1)))
    dmom = rng.normal(size=(n, 3))*np.exp(3*rng.normal(size=(n, 1)))
    rung = rng.integers(0, N_rungs, n).astype(np.int8)
    # rung=None: every particle
    m, d = gpu(mom), gpu(dmom)
    mesh.dmom_apply(m, d)
    assert same(m, mom + dmom) and same(d, dmom)
    mesh.dmom_nullify(d)
    assert same(d, np.zeros((n, 3)))
    # active rungs only; NaN waits in the Δmom of the inactive rows
    for lowest in lowest_values(N_rungs):
        inactive = rung < lowest
        poisoned = dmom.copy()
        poisoned[inactive] = np.nan
        p = host.particles(poisoned, rung, N_rungs)
        p.mom[...] = mom
        p.lowest_active_rung = lowest
        p.apply_dmom()
        m, d = gpu(mom), gpu(poisoned)
        mesh.dmom_apply(m, d, gpu(rung), lowest)
        assert same(m, p.mom) and same(d, poisoned)
        out = m.cpu().numpy()
        assert np.isfinite(out).all() and same(out[inactive], mom[inactive])
        assert same(out[~inactive], (mom + dmom)[~inactive])
        p.nullify_dmom()
        mesh.dmom_nullify(d, gpu(rung), lowest)
        assert same(d, p.dmom) and same(m, p.mom)
        out = d.cpu().numpy()
        assert same(out[inactive], poisoned[inactive]) and same(out[~inactive],
                                                                np.zeros_like(out[~inactive]))


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('N_rungs', [1, 4, 8, 21, 42])
def test_dmom_to_acc(mesh, N_rungs, n):
    rng = np.random.default_rng(100*N_rungs + n % 100)
    mass = 3.0
    a2 = rng.uniform(0.5, 2.0, 3*N_rungs - 1)            # dt_rungs['a**2']
    conv = 1.0/(mass*(rungs.machine_eps + a2))           # species.py:2305
    assert np.unique(conv).size == conv.size
    dmom = rng.normal(size=(n, 3))*np.exp(3*rng.normal(size=(n, 1)))
    rung = rng.integers(0, N_rungs, n).astype(np.int8)
    r = rung.astype(np.int64)
    # flags as flag_rung_jumps leaves them, inside the table
    kind = rng.integers(0, 3, n)
    flags = np.where((kind == 2) & (r < N_rungs - 1), r + 2*N_rungs,
                     np.where((kind == 1) & (r > 0), r + N_rungs, r)).astype(np.int8)
    # valid, but different from the rung everywhere: must not be read without jumps
    decoy = (r + N_rungs).astype(np.int8)
    assert flags.max(initial=0) <= 3*N_rungs - 2 and decoy.max(initial=0) <= 3*N_rungs - 2
    for any_jumps, jumped in ((0, decoy), (1, flags)):
        for lowest in lowest_values(N_rungs):
            p = host.particles(dmom, rung, N_rungs)
            p.mass = mass
            p.rung_jumped[:] = jumped
            p.lowest_active_rung = lowest
            p.convert_dmom_to_acc({rungs.KEY_A2: a2}, bool(any_jumps))
            d = gpu(dmom)
            mesh.dmom_to_acc(d, gpu(rung), gpu(jumped), lowest, gpu(conv), any_jumps)
            assert same(d, p.dmom), (any_jumps, lowest)
            assert same(d.cpu().numpy()[rung < lowest], dmom[rung < lowest])


@pytest.mark.parametrize('kind,n', CASES + [('random', 700001)])
@pytest.mark.parametrize('N_rungs', [1, 4, 8, 21])
def test_substep_passes(mesh, N_rungs, kind, n):
    """k_substep_begin = drift -> flag_rung_jumps -> nullify_Δ and k_substep_end = apply_Δmom ->
    convert_Δmom_to_acc -> apply_rung_jumps -> set_rungs_N (main.py:1347-1624) against the same
    steps of the oracle; 700001 particles take k_substep_end beyond one trip of its 2048
    workgroups."""
    import torch
    acc, rung = population(kind, n, N_rungs)
    if kind == 'edges':
        # (the rows on which the reference itself reads one past its tables: module docstring)
        p = host.particles(acc, rung, N_rungs)
        beyond = np.zeros(rung.size, dtype=bool)
        for factors in ARRANGEMENTS.values():
            beyond |= (rung == N_rungs - 1) & (p.rung_index_float(factors[0])[1] == N_rungs - 1)
        acc, rung = acc[~beyond], rung[~beyond]
    n = rung.size
    rng = np.random.default_rng(7*N_rungs + n % 7)
    pos = rng.uniform(0, L, (n, 3))*(1 - 1e-13)
    mom = rng.normal(size=(n, 3))
    kick = rng.normal(size=(n, 3))
    integrals = integrals_table(N_rungs)
    mass, dtm = 3.0, 0.37
    a2 = rng.uniform(0.5, 2.0, 3*N_rungs - 1)
    conv = 1.0/(mass*(rungs.machine_eps + a2))
    lows = lowest_values(N_rungs) if n < 700001 else [0, N_rungs//2]
    mom_t, rung0_t = gpu(mom), gpu(rung)
    for i, lowest in enumerate(lows):
        factors = list(ARRANGEMENTS.values())[i % 2]
        # the oracle: first pass
        p = host.particles(acc, rung, N_rungs)
        p.pos[...], p.mom[...], p.mass, p.lowest_active_rung = pos, mom, mass, lowest
        oracle.drift(p.pos, p.mom, dtm, L)
        flagged = p.flag_rung_jumps(None, None, None, {rungs.KEY_1: integrals}, factors)
        p.nullify_dmom()
        flags = p.rung_jumped.copy()
        nullified = p.dmom.copy()
        # the pass
        pos_t, dmom_t, rung_t, jumped_t = gpu(pos), gpu(acc), gpu(rung), gpu(rung)
        any_out = torch.full((1,), 7, dtype=torch.int32, device='cuda')
        after = torch.full((N_rungs,), -1, dtype=torch.int64, device='cuda')
        mesh.substep_begin(pos_t, mom_t, dmom_t, rung_t, jumped_t, dtm, True, lowest, integrals,
                           *factors, N_rungs, any_out, after)
        assert same(pos_t, p.pos) and same(dmom_t, nullified) and same(jumped_t, flags)
        assert same(rung_t, rung) and same(mom_t, mom)
        assert int(any_out.item()) == int(flagged)
        # drift alone, flag alone
        pos2, j2 = gpu(pos), gpu(rung)
        mesh.substep_begin(pos2, mom_t, None, rung_t, j2, dtm, False, lowest, None, 0.0, 0.0,
                           N_rungs, any_out)
        assert same(pos2, p.pos) and same(j2, rung)
        pos3, d3, j3 = gpu(pos), gpu(acc), gpu(rung)
        any3 = torch.full((1,), 7, dtype=torch.int32, device='cuda')
        mesh.substep_begin(pos3, mom_t, d3, rung_t, j3, None, True, lowest, integrals, *factors,
                           N_rungs, any3)
        assert same(pos3, pos) and same(d3, nullified) and same(j3, flags)
        assert int(any3.item()) == int(flagged)
        # a kick arrives in Δmom; the oracle's second pass
        p.dmom += kick
        dmom_t += gpu(kick)
        assert same(dmom_t, p.dmom)
        p.apply_dmom()
        p.convert_dmom_to_acc({rungs.KEY_A2: a2}, flagged)
        if flagged:
            p.apply_rung_jumps()
        counts_ref = np.bincount(p.rung, minlength=N_rungs)
        assert counts_ref.size == N_rungs and counts_ref.sum() == n
        assert same(after, counts_ref)                 # counted before the jumps were applied
        m_t = gpu(mom)
        counts = torch.full((N_rungs,), -1, dtype=torch.int64, device='cuda')
        mesh.substep_end(m_t, dmom_t, rung_t, jumped_t, True, lowest, conv, N_rungs, counts)
        assert same(m_t, p.mom) and same(dmom_t, p.dmom)
        assert same(rung_t, p.rung) and same(jumped_t, p.rung)
        assert same(counts, counts_ref)
        # a component that received nothing: the jumps and the populations only
        m4, d4, r4, j4 = gpu(mom), gpu(acc), gpu(rung), gpu(flags)
        counts4 = torch.full((N_rungs,), -1, dtype=torch.int64, device='cuda')
        mesh.substep_end(m4, d4, r4, j4, False, lowest, None, N_rungs, counts4)
        assert same(m4, mom) and same(d4, acc)
        assert same(r4, p.rung) and same(j4, p.rung) and same(counts4, counts_ref)
    assert same(rung0_t, rung)
