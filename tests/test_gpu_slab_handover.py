"""The hand-over of particles between x-slab domains, kernel by kernel, in ONE process.

PotentialMesh(N, L, nprocs=P, rank=r) without a comm is a slab context whose local entry points
need no collective: the P contexts of a box live side by side on one GPU, the exchange is done by
hand with torch indexing and every kernel is compared with a plain numpy reference —
cg_owner_rank[_drifted], cg_emigrant_rows_dest, cg_emigrant_dest, the slab branch of tile_of()
(through cg_sort_particles), the row branch of cg_gather_kick_drift_scatter, cg_region_insert,
cg_set_emigrant_list and cg_prepare_rebind.  The multi-process tests (test_gpu_distributed.py)
move a particle less than a cell per step; here particles cross several slabs and the box face,
sit on slab faces, overflow the row buffer, the list and a region, and carry 64-bit columns whose
bits are NaNs as doubles.

References (numpy float64; L and N are powers of two, so x/cell is exact):
  lower cell   floor(x/cell - 0.5) mod N on cell-centred grids, floor(x/cell) mod N on
               vertex-centred ones.  The library evaluates the reference's own index map
               (mesh.py:1577-1606: offset and scale carry factors 1 +- machine epsilon), which
               moves every face up by a relative 2^-52 and rounds twice: within FACE_BAND of a
               face it may name the neighbouring cell (a particle exactly ON a face belongs to the
               cell below it).  Outside the band the two rules must agree — lower_ref() asserts
               that for every position it is given — and inside it the index map, restated in
               numpy, decides.
  owner        lower // nxl
  drift        np.mod(pos + mom*dtm, L), a result equal to L becomes 0 (test_drift_bit_exact)
  kick         the single-domain cg_gather_kick_tiled on a tile-sorted copy (bit-identical to the
               fused pass: test_fused_kick_drift_scatter_equals_separate)
Every output array is larger than what the call is told about and pre-filled with a sentinel;
the kernel gets a view, and everything outside the permitted slots must keep the sentinel."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 64.0
NGHOSTS = 2
EPS = float(np.finfo(np.float64).eps)
GEOMETRIES = [(2, 32), (4, 64)]
N_PART = 20_000
SUM_RTOL = 1e-13          # the bar of tests/test_gpu_measure_momentum.py
DENSITY_TOL = 1e-12       # the bar of test_full_size_properties
FSENT, ISENT = 1e150, -7  # sentinels of the float and the integer arrays
PAD = 64                  # canary rows behind every array
# |x - off| < L + 2*cell, the face shift is x*eps < L*eps, the offset's own rounding below
# 2*cell*eps: the index map and the exact rule can differ only within eps*(2L + 4*cell) < 3*eps*L
FACE_BAND = 3*EPS*L
# as int64: -1, the sign bit, a signalling NaN, the quiet NaN, the smallest subnormal
SPECIAL_BITS = np.array([-1, -2**63, 0x7FF0000000000001, 0x7FF8000000000000, 1], dtype=np.int64)


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def contexts(torch_cuda):
    """get(P, N, cell_centered) -> (full, [slab contexts]); made once, closed at the end"""
    from concept_amd.mesh import PotentialMesh
    made = {}

    def get(P, N, cc=True):
        key = (P, N, bool(cc))
        if key not in made:
            made[key] = (PotentialMesh(N, L, nghosts=NGHOSTS, cell_centered=cc),
                         [PotentialMesh(N, L, nghosts=NGHOSTS, cell_centered=cc, nprocs=P, rank=r)
                          for r in range(P)])
        return made[key]
    yield get
    for full, slabs in made.values():
        for m in [full] + slabs:
            m.close()


# ---------------------------------------------------------------------------------------------
# plain references
# ---------------------------------------------------------------------------------------------
def rule_lower(x, N, cc):
    return np.floor(x/(L/N) - 0.5*cc).astype(np.int64) % N


def map_lower(x, N, cc):
    """the reference's index map (mesh.py:1577-1606), which include/concept_gpu.h names as the
    ownership rule, operation by operation"""
    cell = L/N
    off = 0.0 - (1 + EPS)*(NGHOSTS - 0.5*cc)*cell
    scale = (1/cell)*(1 - EPS)
    return (((x - off)*scale).astype(np.int64) - NGHOSTS) % N


def lower_ref(x, N, cc):
    x = np.asarray(x, dtype=np.float64)
    assert ((x >= 0) & (x < L)).all()
    d = x/(L/N) - 0.5*cc
    near = np.abs(d - np.rint(d))*(L/N) <= FACE_BAND
    rule, imap = rule_lower(x, N, cc), map_lower(x, N, cc)
    assert np.array_equal(rule[~near], imap[~near]), 'the two rules differ away from a face'
    assert np.isin((rule[near] - imap[near]) % N, (0, 1, N - 1)).all()
    return np.where(near, imap, rule)


def owner_ref(x, P, N, cc=True):
    return lower_ref(x, N, cc)//(N//P)


def drift_ref(pos, mom, dtm):
    out = np.mod(pos + mom*dtm, L)
    out[out == L] = 0.0
    return out


def key_ref(pos, N, cc, x0, nxl, T):
    """8*tile + bucket of cg_tile_info for a slab [x0, x0 + nxl); -1: not owned"""
    ca = lower_ref(pos[:, 0], N, cc) - x0
    cb, cz = lower_ref(pos[:, 1], N, cc), lower_ref(pos[:, 2], N, cc)
    nt = N//T
    f = 4*(ca % T == T - 1) + 2*(cb % T == T - 1) + (cz % T == T - 1)
    key = ((ca//T*nt + cb//T)*nt + cz//T)*8 + f
    return np.where((ca >= 0) & (ca < nxl), key, -1)


def handplaced_x(N, cc):
    """every cell face (the slab faces among them) and its two neighbours, 0, the last double
    below L, and the strip below the first cell centre (cell N-1 on a cell-centred grid)"""
    cell = L/N
    faces = (np.arange(N) + 0.5*cc)*cell
    xs = np.concatenate([faces, np.nextafter(faces, -np.inf), np.nextafter(faces, np.inf),
                         [0.0, np.nextafter(L, 0.0)], np.linspace(0.0, 0.5*cell, 9)])
    return xs[(xs >= 0) & (xs < L)]


DTM_EXACT = 0.5   # a power of two: the hand-made drifts below are exact


def drift_cases(P, N, cc):
    """(start x, displacement) pairs, all exact in binary: landings on every slab face from
    both sides, below 0, beyond L, exactly on L, two and more slabs, several boxes"""
    cell, W = L/N, L/P
    faces = (np.arange(P)*(N//P) + 0.5*cc)*cell
    s = [(f - 3*cell) % L for f in faces] + [(f + 5*cell) % L for f in faces]
    d = [3*cell]*P + [-5*cell]*P
    s += [0.25*cell, 0.0, L - cell, L - 4*cell, 4*cell, 1.25*cell, 1.25*cell, L - 0.25*cell,
          0.75*cell]
    d += [-3*cell, -2.0**-60, 5*cell + 0.25, 4*cell, -4*cell, 2*W + 0.5*cell, 3*W,
          -2*W - 0.5*cell, 3*L + W + 0.25]
    return np.array(s), np.array(d)


_ownership = {}


def ownership_case(P, N, cc):
    """positions, momenta and their reference owners before and after the drift (made once)"""
    key = (P, N, cc)
    if key in _ownership:
        return _ownership[key]
    rng = np.random.default_rng(1000*P + N + cc)
    hx = handplaced_x(N, cc)
    s, d = drift_cases(P, N, cc)
    n = N_PART + hx.size + s.size
    pos = rng.uniform(0, L, (n, 3))
    mom = rng.normal(0, 8.0, (n, 3))
    pos[N_PART:N_PART + hx.size, 0] = hx
    pos[N_PART + hx.size:, 0] = s
    mom[N_PART + hx.size:, 0] = d/DTM_EXACT
    raw = s + d
    after = drift_ref(pos, mom, DTM_EXACT)
    xd = after[N_PART + hx.size:, 0]
    # the hand-made drifts do what they are meant to do
    faces = (np.arange(P)*(N//P) + 0.5*cc)*(L/N)
    assert np.isin(faces, xd).all() and (raw < 0).sum() >= 2 and (raw > L).sum() >= 2
    assert (raw == L).any() and (xd == 0).sum() >= 2 + (not cc)
    assert (np.abs(d) >= 2*L/P).sum() >= 4 and (np.abs(d) > L).any()
    assert ((after >= 0) & (after < L)).all()
    case = dict(pos=pos, mom=mom, after=after, own=owner_ref(pos[:, 0], P, N, cc),
                own_after=owner_ref(after[:, 0], P, N, cc))
    assert set(case['own']) == set(range(P)) and set(case['own_after']) == set(range(P))
    if cc:  # the strip below the first cell centre belongs to the last domain
        strip = pos[:, 0] < 0.5*L/N - FACE_BAND
        assert strip.sum() >= 8 and (case['own'][strip] == P - 1).all()
    _ownership[key] = case
    return case


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def dev(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device='cuda')


def padded(torch, rows, width=None, dtype=None):
    """a sentinel-filled array of rows + PAD rows"""
    dtype = dtype or torch.float64
    shape = (rows + PAD,) if width is None else (rows + PAD, width)
    return torch.full(shape, FSENT if dtype == torch.float64 else ISENT, dtype=dtype,
                      device='cuda')


def untouched(t):
    return bool((t == (FSENT if t.dtype.is_floating_point else ISENT)).all())


def bits(t):
    """the 64-bit patterns of a float64 (or int64) tensor"""
    import torch
    return t.contiguous().view(torch.int64)


def host_bits(t):
    return bits(t).cpu().numpy()


def u32(t):
    return t.long() & 0xffffffff


def live_mask(torch, start, count, cap):
    """live slots of a region table: [start[k], start[k] + count[k])"""
    st, ct = u32(start), u32(count)
    slot = torch.arange(cap, device='cuda')
    k = (torch.searchsorted(st, slot, right=True) - 1).clamp(max=ct.numel() - 1)
    return (slot - st[k]) < ct[k]


def copy_potential(torch, full, slabs):
    """every slab gets its own layers and its halo from the single-domain mesh, layer by layer:
    both paths then read the same potential bits"""
    N = full.gridsize
    buf = torch.empty(full.layer_doubles, dtype=torch.float64, device='cuda')
    for s in slabs:
        assert s.layer_doubles == full.layer_doubles
        G = s.ghost_layers
        for g in range(s.x0 - G, s.x0 + s.nxl + G):
            full.layers_read(g % N, 1, buf)
            s.layers_write(g - s.x0, 1, buf)


def owned_density(torch, mesh, layers):
    per = mesh.layer_doubles
    buf = torch.empty(layers*per, dtype=torch.float64, device='cuda')
    mesh.layers_read(0, layers, buf)
    N = mesh.gridsize
    return buf.view(layers, per//mesh.pad, mesh.pad)[:, :N, :N].clone()


def tile_sorted(torch, mesh, pos, mom, ids):
    """(pos, mom, ids, table) in the tile order of `mesh`; every particle must be owned"""
    po, mo, io = torch.empty_like(pos), torch.empty_like(mom), torch.empty_like(ids)
    table = mesh.sort_particles(pos, mom, ids, po, mo, io)
    assert int(u32(table)[-1]) == pos.shape[0]
    return po, mo, io, table


# ---------------------------------------------------------------------------------------------
# 1. ownership and destinations against the numpy rule
# ---------------------------------------------------------------------------------------------
OWN_CASES = [(P, N, cc) for (P, N) in GEOMETRIES for cc in (True, False)]


@pytest.mark.parametrize('P,N,cc', OWN_CASES)
def test_owner_equals_rule_on_every_context(torch_cuda, contexts, P, N, cc):
    torch = torch_cuda
    case = ownership_case(P, N, cc)
    _, slabs = contexts(P, N, cc)
    pos, mom = dev(torch, case['pos']), dev(torch, case['mom'])
    for s in slabs:   # every context answers for the whole box, and all give the same answer
        got = s.owner_rank(pos).cpu().numpy()
        bad = np.flatnonzero(got != case['own'])
        assert bad.size == 0, (s.rank, case['pos'][bad[:5], 0], got[bad[:5]], case['own'][bad[:5]])
        got = s.owner_rank_drifted(pos, mom, DTM_EXACT).cpu().numpy()
        bad = np.flatnonzero(got != case['own_after'])
        assert bad.size == 0, (s.rank, case['after'][bad[:5], 0], got[bad[:5]],
                               case['own_after'][bad[:5]])
        assert s.error_flags() == 0


@pytest.mark.parametrize('P,N,cc', OWN_CASES)
def test_row_destinations(torch_cuda, contexts, P, N, cc):
    """cg_emigrant_rows_dest: rows hold drifted positions; *count below, at and above cap"""
    torch = torch_cuda
    case = ownership_case(P, N, cc)
    _, slabs = contexts(P, N, cc)
    n = case['after'].shape[0]
    rows_h = np.random.default_rng(3).normal(0, 1, (n, 8))
    rows_h[:, :3] = case['after']
    rows = dev(torch, rows_h)
    ref = case['own_after']
    for s in slabs:
        for count, cap in ((n, n), (777, n), (n, 1000), (n, 0)):
            cnt = torch.tensor([count], dtype=torch.int32, device='cuda')
            dest = padded(torch, n, dtype=torch.int32)
            counts = padded(torch, P, dtype=torch.int32)
            s.emigrant_rows_dest(rows[:cap], cnt, dest[:cap], counts[:P])
            m = min(count, cap)
            assert np.array_equal(dest[:m].cpu().numpy(), ref[:m]), (s.rank, count, cap)
            assert untouched(dest[m:]) and untouched(counts[P:])
            got = counts[:P].cpu().numpy()
            assert np.array_equal(got, np.bincount(ref[:m], minlength=P)) and got.sum() == m
            assert int(cnt[0]) == count and s.error_flags() == 0


@pytest.mark.parametrize('P,N,cc', OWN_CASES)
def test_list_destinations(torch_cuda, contexts, P, N, cc):
    """cg_emigrant_dest: destination of the listed rows under the drift"""
    torch = torch_cuda
    case = ownership_case(P, N, cc)
    _, slabs = contexts(P, N, cc)
    n = case['pos'].shape[0]
    pos, mom = dev(torch, case['pos']), dev(torch, case['mom'])
    idx_h = np.random.default_rng(4).permutation(n)[:n//2 + 3].astype(np.int64)
    idx_h[:64] = np.arange(n - 64, n)       # the hand-made drifts are on the list
    idx = dev(torch, idx_h)
    ref = case['own_after'][idx_h]
    cap = idx_h.size
    for s in slabs:
        for count in (cap, 501, cap + 1000):
            cnt = torch.tensor([count], dtype=torch.int32, device='cuda')
            dest = padded(torch, cap, dtype=torch.int32)
            counts = padded(torch, P, dtype=torch.int32)
            s.emigrant_dest(pos, mom, idx, cnt, DTM_EXACT, dest[:cap], counts[:P])
            m = min(count, cap)
            assert np.array_equal(dest[:m].cpu().numpy(), ref[:m]), (s.rank, count)
            assert untouched(dest[m:]) and untouched(counts[P:])
            assert np.array_equal(counts[:P].cpu().numpy(), np.bincount(ref[:m], minlength=P))
            assert s.error_flags() == 0


@pytest.mark.parametrize('P,N,cc', OWN_CASES)
def test_slab_sort_keeps_the_owned_particles(torch_cuda, contexts, P, N, cc):
    """the slab branch of tile_of(): cg_sort_particles of the whole box keeps exactly the owned
    particles, in the buckets of the numpy key; the last table entry is their number"""
    torch = torch_cuda
    case = ownership_case(P, N, cc)
    _, slabs = contexts(P, N, cc)
    n = case['pos'].shape[0]
    pos, mom = dev(torch, case['pos']), dev(torch, case['mom'])
    ids = torch.arange(n, device='cuda')
    for s in slabs:
        key = key_ref(case['pos'], N, cc, s.x0, s.nxl, s.tile_extent)
        assert np.array_equal(key >= 0, case['own'] == s.rank)
        po, mo, io = padded(torch, n, 3), padded(torch, n, 3), padded(torch, n, dtype=torch.int64)
        table = s.sort_particles(pos, mom, ids, po[:n], mo[:n], io[:n])
        t = u32(table).cpu().numpy()
        kept = int((key >= 0).sum())
        assert t[0] == 0 and t[-1] == kept and s.error_flags() == 0
        assert np.array_equal(np.diff(t), np.bincount(key[key >= 0], minlength=8*s.ntiles))
        got = io[:kept].cpu().numpy()
        assert np.array_equal(np.sort(got), np.flatnonzero(key >= 0))
        assert np.array_equal(key[got], np.repeat(np.arange(8*s.ntiles), np.diff(t)))
        assert np.array_equal(po[:kept].cpu().numpy(), case['pos'][got])
        assert np.array_equal(mo[:kept].cpu().numpy(), case['mom'][got])
        assert untouched(po[kept:]) and untouched(mo[kept:]) and untouched(io[kept:])


# ---------------------------------------------------------------------------------------------
# 2. the fused pass on slabs with the row buffer, two steps, exchange by hand
# ---------------------------------------------------------------------------------------------
class Rank:
    """one domain's particle arrays (two sets, sentinel-filled) and region tables"""

    def __init__(self, torch, mesh, pos, mom, ids, aux):
        self.mesh, n = mesh, pos.shape[0]
        po, mo, io, table = tile_sorted(torch, mesh, pos, mom, ids)
        lookup = torch.empty(int(ids.max()) + 1, dtype=torch.int64, device='cuda')
        lookup[ids] = aux
        self.cap = cap = mesh.region_capacity(int(1.25*n) + 1024)
        self.sets = [[padded(torch, cap, 3), padded(torch, cap, 3),
                      padded(torch, cap, dtype=torch.int64), padded(torch, cap, dtype=torch.int64)]
                     for _ in range(2)]
        for dst, src in zip(self.sets[0], (po, mo, io, lookup[io])):
            dst[:n] = src
        self.cur, self.start, self.count = 0, table, None
        self.tables = [mesh.new_region_table(), mesh.new_region_table()]
        self.rows_cap = 4096
        self.rows = padded(torch, self.rows_cap, 8)
        self.dest = padded(torch, self.rows_cap, dtype=torch.int32)
        self.meta = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.m2 = torch.zeros(1, dtype=torch.float64, device='cuda')
        self.held = io.cpu().numpy()     # ids of the particles the next pass kicks

    def views(self, which):
        return [a[:self.cap] for a in self.sets[which]]

    def live(self, torch):
        return live_mask(torch, self.start, self.count, self.cap)


@pytest.mark.parametrize('order', [2, 4])
@pytest.mark.parametrize('P,N', GEOMETRIES)
def test_fused_pass_on_slabs_two_steps(torch_cuda, contexts, P, N, order):
    torch = torch_cuda
    full, slabs = contexts(P, N)
    n, W, cell = N_PART, L/P, L/N
    dtm, sigma = 0.9, 0.04*W/0.9
    rng = np.random.default_rng(100*P + order)
    pos = rng.uniform(0, L, (n, 3))
    mom = rng.normal(0, sigma, (n, 3))           # about 3 % of a slab leave per step
    # through the box face both ways, over two slabs, once round the box
    pos[:6, 0] = [0.75*cell, L - 0.25*cell, 2.0, 2.0, L - 2.0, 5.0]
    mom[:6, 0] = np.array([-3*cell, 3*cell, 2*W + 4, W + 4, -2*W - 4, L + W + 4])/dtm
    ids_h = rng.permutation(n).astype(np.int64)   # particle j carries the id ids_h[j]
    aux_h = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    aux_h[:200] = SPECIAL_BITS[np.arange(200) % 5]
    by_id = np.empty(n, dtype=np.int64)
    by_id[ids_h] = np.arange(n)
    pos, mom, aux_by_id = pos[by_id], mom[by_id], aux_h[by_id]   # from here on: indexed by id
    owner = owner_ref(pos[:, 0], P, N)

    all_ids = torch.arange(n, device='cuda')
    ranks = []
    for r, s in enumerate(slabs):
        sel = np.flatnonzero(owner == r)
        ranks.append(Rank(torch, s, dev(torch, pos[sel]), dev(torch, mom[sel]), dev(torch, sel),
                          dev(torch, aux_by_id[sel])))
    full.zero()
    full.deposit(dev(torch, pos), 1.0)
    moved_far = 0
    for step in range(2):
        # the reference: potential and kick on the single domain, the drift in numpy
        full.poisson_solve(4, -1.0, False, 0.0)
        copy_potential(torch, full, slabs)
        ps, ms, is_, table = tile_sorted(torch, full, dev(torch, pos), dev(torch, mom), all_ids)
        if step == 0:   # a kick a quarter of the momenta's spread: it matters and moves nobody far
            force = torch.zeros_like(ms)
            full.gather_kick_tiled(ps, force, table, order, 1.0)
            kick = -0.25*sigma/float(force.std())
        full.gather_kick_tiled(ps, ms, table, order, kick)
        kicked = np.empty_like(mom)
        kicked[is_.cpu().numpy()] = ms.cpu().numpy()
        assert not np.array_equal(kicked, mom)
        after = drift_ref(pos, kicked, dtm)
        owner_after = owner_ref(after[:, 0], P, N)
        moved_far += int((np.abs(kicked[:, 0]*dtm) > W).sum())
        leavers = int((owner_after != owner).sum())
        assert 0.01*n < leavers < 0.1*n

        row_ids, row_dest, row_data = [], [], []
        for r, k in enumerate(ranks):
            s, o = k.mesh, 1 - k.cur
            for a in k.sets[o]:
                a.fill_(FSENT if a.dtype.is_floating_point else ISENT)
            k.rows.fill_(FSENT)
            k.dest.fill_(ISENT)
            start_out, count_out = k.tables[o]
            pa, ma, ia, xa = k.views(k.cur)
            pb, mb, ib, xb = k.views(o)
            s.predict_regions(k.start, k.count, start_out)
            s.set_emigrant_rows(k.rows[:k.rows_cap], k.meta)
            s.set_momentum_sum(k.m2)
            try:
                s.gather_kick_drift_scatter(pa, ma, ia, k.start, k.count, pb, mb, ib, start_out,
                                            count_out, order, kick, dtm, aux_in=xa, aux_out=xb)
            finally:
                s.set_momentum_sum(None)
                s.set_emigrant_rows(None, None)
            counts = padded(torch, P, dtype=torch.int32)
            s.emigrant_rows_dest(k.rows[:k.rows_cap], k.meta, k.dest[:k.rows_cap], counts[:P])
            assert s.error_flags() == 0
            k.start, k.count, k.cur = start_out, count_out, o
            c = int(u32(k.meta)[0])
            live = k.live(torch)
            res_ids = ib[live].cpu().numpy()
            rid = bits(k.rows[:c, 6]).cpu().numpy()
            # a row exactly for the particles this rank kicked that belong elsewhere afterwards
            assert np.array_equal(np.sort(np.concatenate([res_ids, rid])), np.sort(k.held))
            assert np.array_equal(np.sort(rid), np.sort(k.held[owner_after[k.held] != r]))
            assert (owner_after[res_ids] == r).all()
            st, ct = u32(start_out), u32(count_out)
            assert int(ct.sum()) == res_ids.size and int(st[-1]) <= k.cap
            assert bool((st[1:] - st[:-1] >= ct).all())
            # payload, bit for bit
            for got, ref in ((pb[live], after[res_ids]), (mb[live], kicked[res_ids]),
                             (k.rows[:c, 0:3], after[rid]), (k.rows[:c, 3:6], kicked[rid])):
                assert np.array_equal(host_bits(got), ref.view(np.int64))
            assert np.array_equal(xb[live].cpu().numpy(), aux_by_id[res_ids])
            assert np.array_equal(bits(k.rows[:c, 7]).cpu().numpy(), aux_by_id[rid])
            # destinations and counts of the rows
            d = k.dest[:c].cpu().numpy()
            assert np.array_equal(d, owner_after[rid])
            assert np.array_equal(counts[:P].cpu().numpy(), np.bincount(d, minlength=P))
            # nothing outside the live slots, the rows [:count] and the P counts
            for a, v in zip(k.sets[o], (pb, mb, ib, xb)):
                assert untouched(v[~live]) and untouched(a[k.cap:])
            assert untouched(k.rows[c:]) and untouched(k.dest[c:]) and untouched(counts[P:])
            # sum of |mom|^2 over the particles this rank kicked, leavers included
            q = kicked[k.held]
            m2_ref = math.fsum((q[:, 0]*q[:, 0] + q[:, 1]*q[:, 1]) + q[:, 2]*q[:, 2])
            m2 = float(k.m2[0])
            print(f'step {step} rank {r}: {c} rows, sum {m2!r} (fsum {m2_ref!r}, '
                  f'rel {abs(m2 - m2_ref)/m2_ref:.2e})')
            assert abs(m2 - m2_ref) <= SUM_RTOL*m2_ref
            row_ids.append(rid)
            by_dest = torch.argsort(k.dest[:c].long(), stable=True)
            row_dest.append(k.dest[:c].long()[by_dest])
            row_data.append(k.rows[:c][by_dest])
        every = np.concatenate([x.held for x in ranks])
        assert np.array_equal(np.sort(every), np.arange(n))

        # the exchange, by hand: rows sorted by destination, concatenated per destination
        for r, k in enumerate(ranks):
            s = k.mesh
            inc = torch.cat([rows[d == r] for rows, d in zip(row_data, row_dest)]).contiguous()
            pb, mb, ib, xb = k.views(k.cur)
            s.region_insert(inc, k.start, k.count, pb, mb, ib, xb, k.cap)
            assert s.error_flags() == 0
            live = k.live(torch)
            k.held = ib[live].cpu().numpy()
            assert np.array_equal(np.sort(k.held), np.flatnonzero(owner_after == r))
            for got, ref in ((pb[live], after[k.held]), (mb[live], kicked[k.held])):
                assert np.array_equal(host_bits(got), ref.view(np.int64))
            assert np.array_equal(xb[live].cpu().numpy(), aux_by_id[k.held])
            for a, v in zip(k.sets[k.cur], (pb, mb, ib, xb)):
                assert untouched(v[~live]) and untouched(a[k.cap:])
            # the populations are those of an exact sort of the rank's new particles
            *_, exact = tile_sorted(torch, s, pb[live], mb[live], ib[live])
            dense = u32(exact)
            assert torch.equal(u32(k.count), dense[1:] - dense[:-1])
        assert np.array_equal(np.sort(np.concatenate([x.held for x in ranks])), np.arange(n))

        pos, mom, owner = after, kicked, owner_after
        full.zero()
        full.deposit(dev(torch, pos), 1.0)
        if step == 0:
            # the pull deposit from the regions sees a particle seated in a wrong bucket: part
            # of its cloud is lost.  One ghost layer folded by hand into the next domain.
            ref = owned_density(torch, full, N)
            per = full.layer_doubles
            ghost = []
            for k in ranks:
                k.mesh.deposit_regions(k.views(k.cur)[0], k.start, k.count, 1.0)
                g = torch.empty(per, dtype=torch.float64, device='cuda')
                k.mesh.layers_read(k.mesh.nxl, 1, g)
                ghost.append(g)
            for r, k in enumerate(ranks):
                ranks[(r + 1) % P].mesh.layers_write(0, 1, ghost[r], add=True)
            got = torch.cat([owned_density(torch, k.mesh, k.mesh.nxl) for k in ranks])
            err = float((got - ref).abs().max())
            print(f'density: max error {err:.3e}, max {float(ref.max()):.3e}')
            assert err <= DENSITY_TOL*float(ref.abs().max())
            assert abs(float(got.sum()) - n) <= 1e-9*n
    assert moved_far >= 8    # the hand-set particles kept crossing slabs and the box face


# ---------------------------------------------------------------------------------------------
# 3. failure paths stay inside their bounds ((2, 32), rank 0: lower cells 0..15, x in [1, 33))
# ---------------------------------------------------------------------------------------------
def small_domain(torch, contexts, n=2000, seed=7):
    """rank 0 of (2, 32) with a zero potential and n owned particles, tile-sorted (numpy + GPU)"""
    _, slabs = contexts(2, 32)
    s = slabs[0]
    s.zero()
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, L, (n, 3))
    pos[:, 0] = rng.uniform(2.0, 32.0, n)
    mom = rng.normal(0, 0.05, (n, 3))
    assert (owner_ref(pos[:, 0], 2, 32) == 0).all()
    return s, pos, mom


def test_row_buffer_too_small(torch_cuda, contexts):
    torch = torch_cuda
    from concept_amd import lib
    s, pos, mom = small_domain(torch, contexts)
    n, cap_rows, dtm = pos.shape[0], 16, 1.0
    mom[::7, 0] = 32.0 + mom[::7, 0]            # into the other slab
    mom[5::70, 0] = -(pos[5::70, 0] + 1.5)      # through the box face into the other slab
    after = drift_ref(pos, mom, dtm)
    leaves = owner_ref(after[:, 0], 2, 32) != 0
    assert 250 < leaves.sum() < 400
    aux_h = np.resize(SPECIAL_BITS, n)
    po, mo, io, table = tile_sorted(torch, s, dev(torch, pos), dev(torch, mom),
                                    torch.arange(n, device='cuda'))
    xo = dev(torch, aux_h)[io]
    cap = s.region_capacity(n)
    ins = [torch.cat([a, torch.zeros((cap - n,) + tuple(a.shape[1:]), dtype=a.dtype,
                                     device='cuda')]) for a in (po, mo, io, xo)]
    keep = [a.clone() for a in ins]
    outs = [padded(torch, cap, 3), padded(torch, cap, 3), padded(torch, cap, dtype=torch.int64),
            padded(torch, cap, dtype=torch.int64)]
    rows = padded(torch, cap_rows, 8)
    meta = torch.zeros(1, dtype=torch.int32, device='cuda')
    start_out, count_out = s.new_region_table()
    s.predict_regions(table, None, start_out)
    s.set_emigrant_rows(rows[:cap_rows], meta)
    try:
        s.gather_kick_drift_scatter(ins[0], ins[1], ins[2], table, None, outs[0][:cap],
                                    outs[1][:cap], outs[2][:cap], start_out, count_out, 2, 1.0,
                                    dtm, aux_in=ins[3], aux_out=outs[3][:cap])
    finally:
        s.set_emigrant_rows(None, None)
    assert s.error_flags() == lib.CG_ERR_BUCKET_OVERFLOW
    assert int(u32(meta)[0]) == leaves.sum()
    rid = bits(rows[:cap_rows, 6]).cpu().numpy()
    assert np.unique(rid).size == cap_rows and leaves[rid].all()
    got = rows[:cap_rows].cpu().numpy()
    assert np.array_equal(got[:, 0:3].view(np.int64), after[rid].view(np.int64))
    assert np.array_equal(got[:, 3:6].view(np.int64), mom[rid].view(np.int64))
    assert np.array_equal(bits(rows[:cap_rows, 7]).cpu().numpy(), aux_h[rid])
    assert untouched(rows[cap_rows:])
    assert all(torch.equal(a, b) for a, b in zip(ins, keep))
    assert all(untouched(a[cap:]) for a in outs)
    # the residents are all there, in live slots
    live = live_mask(torch, start_out, count_out, cap)
    assert np.array_equal(np.sort(outs[2][:cap][live].cpu().numpy()), np.flatnonzero(~leaves))


def test_fused_pass_without_row_buffer_is_refused(torch_cuda, contexts):
    torch = torch_cuda
    from concept_amd import lib
    s, pos, mom = small_domain(torch, contexts, n=500)
    n = pos.shape[0]
    po, mo, io, table = tile_sorted(torch, s, dev(torch, pos), dev(torch, mom),
                                    torch.arange(n, device='cuda'))
    cap = s.region_capacity(n)
    pb, mb = padded(torch, cap, 3), padded(torch, cap, 3)
    start_out, count_out = s.new_region_table()
    s.predict_regions(table, None, start_out)
    count_out.fill_(5)
    s.set_emigrant_rows(None, None)
    with pytest.raises(lib.ConceptGPUError, match='row buffer'):
        s.gather_kick_drift_scatter(po, mo, None, table, None, pb[:cap], mb[:cap], None,
                                    start_out, count_out, 2, 1.0, 1.0)
    # no kernel, no memset ran
    assert untouched(pb) and untouched(mb) and bool((count_out == 5).all())
    assert s.error_flags() == 0


def test_emigrant_list_too_small_and_large(torch_cuda, contexts):
    torch = torch_cuda
    s, pos, mom = small_domain(torch, contexts)
    n, dtm = pos.shape[0], 0.75
    mom[::9, 0] += 45.0
    mom[4::90, 0] = -(pos[4::90, 0] + 3.0)/dtm
    po, mo, io, table = tile_sorted(torch, s, dev(torch, pos), dev(torch, mom),
                                    torch.arange(n, device='cuda'))
    order = io.cpu().numpy()
    after = drift_ref(pos[order], mom[order], dtm)       # by row of the sorted arrays
    own_after = owner_ref(after[:, 0], 2, 32)
    leavers = np.flatnonzero(own_after != 0)
    assert 200 < leavers.size < 300
    try:
        for cap in (8, 1024):
            idx = padded(torch, cap, dtype=torch.int64)
            cnt = torch.full((1,), 99, dtype=torch.int32, device='cuda')
            p1, m1 = po.clone(), mo.clone()
            s.set_emigrant_list(idx[:cap], cnt)
            s.gather_kick_tiled_prepare(p1, m1, table, 2, 1.0, dtm)
            assert s.error_flags() == 0          # the caller falls back: no error
            assert int(u32(cnt)[0]) == leavers.size
            m = min(cap, leavers.size)
            got = idx[:m].cpu().numpy()
            assert np.unique(got).size == m and np.isin(got, leavers).all()
            assert untouched(idx[m:])
            assert torch.equal(p1, po) and torch.equal(m1, mo)   # zero potential: no kick
            if cap > leavers.size:
                assert np.array_equal(np.sort(got), leavers)
                dest = padded(torch, cap, dtype=torch.int32)
                counts = padded(torch, 2, dtype=torch.int32)
                s.emigrant_dest(p1, m1, idx[:cap], cnt, dtm, dest[:cap], counts[:2])
                assert np.array_equal(dest[:m].cpu().numpy(), own_after[got])
                assert np.array_equal(counts[:2].cpu().numpy(),
                                      np.bincount(own_after[got], minlength=2))
                assert untouched(dest[m:]) and untouched(counts[2:])
                assert s.error_flags() == 0
    finally:
        s.set_emigrant_list(None, None)
        s.prepare_invalidate()


class Layout:
    """a small domain laid out in regions with gaps by a fused pass that moves nobody"""

    def __init__(self, torch, contexts):
        s, pos, mom = small_domain(torch, contexts)
        n = pos.shape[0]
        mom[:] = 0.0
        ids = np.arange(n) + 10_000
        po, mo, io, table = tile_sorted(torch, s, dev(torch, pos), dev(torch, mom), dev(torch, ids))
        self.s, self.cap = s, s.region_capacity(n)
        cap = self.cap
        self.arrays = [padded(torch, cap, 3), padded(torch, cap, 3),
                       padded(torch, cap, dtype=torch.int64), padded(torch, cap, dtype=torch.int64)]
        rows = padded(torch, 64, 8)
        meta = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.start, self.count = s.new_region_table()
        s.predict_regions(table, None, self.start)
        s.set_emigrant_rows(rows[:64], meta)
        try:
            s.gather_kick_drift_scatter(po, mo, io, table, None, *[a[:cap] for a in self.arrays[:3]],
                                        self.start, self.count, 2, 1.0, 1.0, aux_in=io,
                                        aux_out=self.arrays[3][:cap])
        finally:
            s.set_emigrant_rows(None, None)
        assert s.error_flags() == 0 and int(meta[0]) == 0
        self.st, self.ct = u32(self.start).cpu().numpy(), u32(self.count).cpu().numpy()
        assert self.ct.sum() == n
        self.before = [a.clone() for a in self.arrays]
        self.count0 = self.count.clone()

    def views(self):
        return [a[:self.cap] for a in self.arrays]

    def changed_rows(self, torch):
        """rows of the arrays (canary rows included) that differ from the layout"""
        ch = torch.zeros(self.arrays[0].shape[0], dtype=torch.bool, device='cuda')
        for a, b in zip(self.arrays, self.before):
            d = bits(a) != bits(b)
            ch |= d.view(ch.numel(), -1).any(1)
        return torch.nonzero(ch).flatten().cpu().numpy()


def rows_at(torch, xyz, m, first_id):
    """m rows at (nearly) the position xyz: momenta, ids and aux that identify the row"""
    rows = np.zeros((m, 8))
    rows[:, 0:3] = np.asarray(xyz) + 1e-3*np.arange(m)[:, None]/m
    rows[:, 3:6] = 1000.0 + np.arange(m)[:, None]
    rows[:, 6] = (first_id + np.arange(m, dtype=np.int64)).view(np.float64)
    rows[:, 7] = np.resize(SPECIAL_BITS, m).view(np.float64)
    return rows


def test_region_insert_bucket_overflow_stays_in_its_region(torch_cuda, contexts):
    torch = torch_cuda
    from concept_amd import lib
    lay = Layout(torch, contexts)
    s = lay.s
    xyz = (10.5, 10.5, 10.5)                          # lower cell (4, 4, 4): tile 0, bucket 0
    k = int(key_ref(np.array([xyz]), 32, True, s.x0, s.nxl, s.tile_extent)[0])
    assert k == 0 and lay.ct[k] > 0 and lay.ct[k + 1] > 0
    room = lay.st[k + 1] - lay.st[k]
    m = int(room - lay.ct[k]) + 40
    rows = rows_at(torch, xyz, m, 50_000)
    assert (key_ref(rows[:, :3], 32, True, s.x0, s.nxl, s.tile_extent) == k).all()
    s.region_insert(dev(torch, rows), lay.start, lay.count, *lay.views(), lay.cap)
    assert s.error_flags() & lib.CG_ERR_BUCKET_OVERFLOW
    ch = lay.changed_rows(torch)
    # only the free slots of the region itself: its own live rows and every other region are
    # as they were (the counts are unusable afterwards by contract: not asserted)
    assert ch.size == room - lay.ct[k]
    assert ch.min() >= lay.st[k] + lay.ct[k] and ch.max() < lay.st[k + 1]
    got = lay.arrays[2].cpu().numpy()[ch]
    assert np.unique(got).size == ch.size and ((got >= 50_000) & (got < 50_000 + m)).all()


def test_region_insert_refuses_a_row_of_another_slab(torch_cuda, contexts):
    torch = torch_cuda
    from concept_amd import lib
    lay = Layout(torch, contexts)
    rows = rows_at(torch, (40.0, 10.5, 10.5), 3, 60_000)
    rows[1, 0] = 0.5                                   # the strip that belongs to cell N-1
    assert (owner_ref(rows[:, 0], 2, 32) == 1).all()
    lay.s.region_insert(dev(torch, rows), lay.start, lay.count, *lay.views(), lay.cap)
    assert lay.s.error_flags() & lib.CG_ERR_BUCKET_OVERFLOW
    assert lay.changed_rows(torch).size == 0 and torch.equal(lay.count, lay.count0)


def test_region_insert_respects_capacity(torch_cuda, contexts):
    torch = torch_cuda
    from concept_amd import lib
    lay = Layout(torch, contexts)
    s = lay.s
    xyz = (10.5, 10.5, 50.5)                           # tile 1, bucket 0
    k = int(key_ref(np.array([xyz]), 32, True, s.x0, s.nxl, s.tile_extent)[0])
    assert k == 8 and lay.ct[k] + 5 < lay.st[k + 1] - lay.st[k]    # the region itself has room
    capacity = int(lay.st[k + 1]) - 1                  # ... but is cut off by the arrays' end
    rows = rows_at(torch, xyz, 5, 70_000)
    s.region_insert(dev(torch, rows), lay.start, lay.count, *lay.views(), capacity)
    assert s.error_flags() & lib.CG_ERR_BUCKET_OVERFLOW
    ch = lay.changed_rows(torch)
    assert (ch < capacity).all()
    assert ch.size == 0            # a region cut off has no room at all (see the fused pass)


def test_region_insert_without_ids_and_with_zero_rows(torch_cuda, contexts):
    torch = torch_cuda
    lay = Layout(torch, contexts)
    s = lay.s
    pb, mb, ib, xb = lay.views()
    # (e) zero rows
    s.region_insert(torch.empty((0, 8), dtype=torch.float64, device='cuda'), lay.start, lay.count,
                    pb, mb, ib, xb, lay.cap)
    assert s.error_flags() == 0 and lay.changed_rows(torch).size == 0
    assert torch.equal(lay.count, lay.count0)
    # (d) no 64-bit columns: rows for three different (tile, bucket)s, one of them on a tile's
    # last cells (bucket 7) and one next to the slab's upper face
    rows = np.concatenate([rows_at(torch, (10.5, 10.5, 10.5), 4, 1),
                           rows_at(torch, (32.5, 32.5, 32.5), 3, 1),
                           rows_at(torch, (32.5, 40.5, 10.5), 2, 1)])
    keys = key_ref(rows[:, :3], 32, True, s.x0, s.nxl, s.tile_extent)
    assert list(np.unique(keys)) == [0, 7, 2*8 + 4]
    s.region_insert(dev(torch, rows), lay.start, lay.count, pb, mb, None, None, lay.cap)
    assert s.error_flags() == 0
    ct = u32(lay.count).cpu().numpy()
    assert np.array_equal(ct - lay.ct, np.bincount(keys, minlength=ct.size))
    assert torch.equal(lay.arrays[2], lay.before[2]) and torch.equal(lay.arrays[3], lay.before[3])
    ch = lay.changed_rows(torch)
    want = np.concatenate([lay.st[k] + lay.ct[k] + np.arange(c)
                           for k, c in zip(*np.unique(keys, return_counts=True))])
    assert np.array_equal(ch, np.sort(want))
    for k in np.unique(keys):
        slots = lay.st[k] + lay.ct[k] + np.arange((keys == k).sum())
        got = np.concatenate([pb[slots].cpu().numpy(), mb[slots].cpu().numpy()], axis=1)
        ref = rows[keys == k, :6]
        assert np.array_equal(got[np.argsort(got[:, 3])], ref[np.argsort(ref[:, 3])])


# ---------------------------------------------------------------------------------------------
# 4. the exact path's prepared sort on a slab (ParticleStore.drift_exchange_sort by hand)
# ---------------------------------------------------------------------------------------------
def by_bucket(table, ids, pos, mom):
    """rows ordered by (bucket, id): the order inside a bucket is that of the atomics"""
    t = u32(table).cpu().numpy()
    n = int(t[-1])
    bucket = np.repeat(np.arange(t.size - 1), np.diff(t))
    i = ids[:n].cpu().numpy()
    o = np.lexsort((i, bucket))
    return i[o], host_bits(pos[:n])[o], host_bits(mom[:n])[o]


def test_prepared_sort_after_exchange(torch_cuda, contexts):
    torch = torch_cuda
    from concept_amd import lib
    P, N, n, dtm = 2, 32, N_PART, 0.9
    sigma = 0.04*(L/P)/dtm
    full, slabs = contexts(P, N)
    rng = np.random.default_rng(77)
    pos = rng.uniform(0, L, (n, 3))
    mom = rng.normal(0, sigma, (n, 3))
    pos[:2, 0] = [1.5, L - 0.5]
    mom[:2, 0] = np.array([-4.0, 4.0])/dtm            # through the box face, both ways
    owner = owner_ref(pos[:, 0], P, N)
    full.zero()
    full.deposit(dev(torch, pos), 1.0)
    full.poisson_solve(4, -1.0, False, 0.0)
    copy_potential(torch, full, slabs)
    ps, force, _, table = tile_sorted(torch, full, dev(torch, pos), torch.zeros((n, 3), device='cuda',
                                      dtype=torch.float64), torch.arange(n, device='cuda'))
    full.gather_kick_tiled(ps, force, table, 2, 1.0)
    kick = -0.25*sigma/float(force.std())     # a quarter of the momenta's spread

    def prepare():
        """per rank: sorted arrays, kicked in place, and the rows the prepared drift takes away"""
        out = []
        for r, s in enumerate(slabs):
            sel = np.flatnonzero(owner == r)
            po, mo, io, table = tile_sorted(torch, s, dev(torch, pos[sel]), dev(torch, mom[sel]),
                                            dev(torch, sel))
            idx = padded(torch, 4096, dtype=torch.int64)
            cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
            s.set_emigrant_list(idx[:4096], cnt)
            try:
                s.gather_kick_tiled_prepare(po, mo, table, 2, kick, dtm)
            finally:
                s.set_emigrant_list(None, None)
            c = int(u32(cnt)[0])
            assert 0 < c <= 4096 and untouched(idx[c:])
            out.append((po, mo, io, idx[:c].clone()))
        # rank 0: drop the listed rows, append the undrifted immigrants, rebind
        (p0, m0, i0, l0), (p1, m1, i1, l1) = out
        stay = torch.ones(p0.shape[0], dtype=torch.bool, device='cuda')
        stay[l0] = False
        add_p, add_m = p1[l1].contiguous(), m1[l1].contiguous()
        pn = torch.cat([p0[stay], add_p]).contiguous()
        mn = torch.cat([m0[stay], add_m]).contiguous()
        idn = torch.cat([i0[stay], i1[l1]]).contiguous()
        slabs[0].prepare_rebind(pn, mn, add_p, add_m)
        return pn, mn, idn

    def sort(pn, mn, idn):
        m = pn.shape[0]
        po, mo, io = padded(torch, m, 3), padded(torch, m, 3), padded(torch, m, dtype=torch.int64)
        table = slabs[0].drift_sort(pn, mn, idn, po[:m], mo[:m], io[:m], dtm)
        return table, io, po, mo

    s = slabs[0]
    try:
        pn, mn, idn = prepare()
        m = pn.shape[0]
        after = drift_ref(pn.cpu().numpy(), mn.cpu().numpy(), dtm)
        assert (owner_ref(after[:, 0], P, N) == 0).all()      # the hand-made exchange was complete
        assert 0.01*m < (owner[idn.cpu().numpy()] != 0).sum() < 0.1*m      # immigrants
        prepared = sort(pn, mn, idn)
        assert s.error_flags() == 0
        s.prepare_invalidate()
        plain = sort(pn, mn, idn)
        assert s.error_flags() == 0
        assert int(u32(prepared[0])[-1]) == m and torch.equal(prepared[0], plain[0])
        a, b = by_bucket(*prepared), by_bucket(*plain)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert all(untouched(t[m:]) for t in prepared[1:] + plain[1:])
        # ... and they are the drifted inputs, in the buckets of the numpy key
        o = np.argsort(idn.cpu().numpy())
        o2 = np.argsort(a[0])
        assert np.array_equal(a[0][o2], idn.cpu().numpy()[o])
        assert np.array_equal(a[1][o2], after[o].view(np.int64))
        assert np.array_equal(a[2][o2], mn.cpu().numpy()[o].view(np.int64))
        t = u32(prepared[0]).cpu().numpy()
        key = key_ref(after, N, True, s.x0, s.nxl, s.tile_extent)
        assert np.array_equal(np.diff(t), np.bincount(key, minlength=8*s.ntiles))

        # control: the prepared histogram is the one in use — one momentum changed after the
        # rebind, so that its particle lands in another tile, must be noticed
        pn, mn, idn = prepare()
        key_of_first = lambda: int(key_ref(drift_ref(pn[:1].cpu().numpy(), mn[:1].cpu().numpy(),
                                                     dtm), N, True, s.x0, s.nxl, s.tile_extent)[0])
        k1 = key_of_first()
        mn[0, 1] += s.tile_extent*(L/N)/dtm        # one tile further in y
        k2 = key_of_first()
        assert k1 >= 0 and k2 >= 0 and k1//8 != k2//8
        sort(pn, mn, idn)
        assert s.error_flags() & lib.CG_ERR_STALE_HISTOGRAM
    finally:
        for x in slabs:
            x.set_emigrant_list(None, None)
            x.prepare_invalidate()
