"""GPU tests of the general-order deposit and scalar gather (cg_deposit / cg_gather_scalar:
k_deposit_general<1..4>, k_gather_scalar<1..4> in cg_general.hip) and of the untiled CIC deposit
(cg_deposit_cic: the order-2 deposit with the context's own geometry), on BOTH of their code paths.

A workgroup of these kernels takes 2048 consecutive particles.  When the first cells of their
stencils span a box that fits 4096 cells of LDS (stencil width included) the chunk works in LDS
(the box path), else on global memory (the direct path).  The particle sets below are built so
that the path of every chunk is certain from the geometry alone: chunks confined to a cube of 8
first cells (box), chunks holding two particles 32 cells apart on every axis (direct), cubes
across the periodic seam, boxes at and one past the 4096-cell limit, boxes that cover a whole
axis, 6144 particles on one spot, and particles on and one ulp off the points where the cell
index switches.

Reference: NumPy, written from the formulas.  Cell index and weights per axis in float64 with
the expressions of the four assignment schemes (exact on both sides: no contraction in the
kernels); deposit terms ((wx*contribution)*wy)*wz in float64, summed per cell in np.longdouble;
gather sum(mesh*((wx*wy)*wz)) in longdouble, then factor, then + mom.

Bounds (u = 2**-53), derived, not tuned:
  deposit, per cell:    2*m*u*sum|term| + u*|value|      (m terms landed in the cell; the two
                        sides differ in summation order only: (m - 1)*u*sum|term| to first order)
  gather, per particle: |factor|*2*ORDER**3*u*sum|mesh*w| + u*|value*factor| + u*|mom|
  gather, compact against shuffled memory order: bit-identical per particle (the loop over the
                        stencil is the same on both paths)
Every test prints its largest error/bound ratio."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0**-53
CHUNK = 2048                       # particles per workgroup of the chunked kernels
COUNTS = (5*CHUNK + 1, 3*CHUNK - 1, CHUNK)
ORDER_NAMES = {1: 'NGP', 2: 'CIC', 3: 'TSC', 4: 'PCS'}
# t-space: a particle with coordinate t (in cells) has floor(t) as the first cell of its stencil;
# the grid coordinate the kernels see is t + nghosts + T_SHIFT[order]
T_SHIFT = {1: -0.5, 2: 0.0, 3: 0.5, 4: 1.0}
KINDS = [1, 2, 3, 4, 'cic']        # 'cic': PotentialMesh.deposit (cg_deposit_cic)
L_BOX = 100.0                      # cell sizes 100/64, 100/256, 100/16: exact in binary


# -- the reference ---------------------------------------------------------------------------
def index_weights(x, order):
    """first stencil cell (ghosted index) and the `order` weights along one axis, float64"""
    if order == 1:
        return np.trunc(x + 0.5).astype(np.int64), [np.ones_like(x)]
    if order == 2:
        index = np.trunc(x)
        dist = x - index
        return index.astype(np.int64), [1 - dist, dist]
    if order == 3:
        index = np.trunc(x + 0.5)
        dist = x - index
        dist2 = dist*dist
        w0 = 0.125 + 0.5*(dist2 - dist)
        w1 = 0.75 - dist2
        return index.astype(np.int64) - 1, [w0, w1, (1 - w0) - w1]
    index = np.trunc(x) - 1
    dist = x - index
    tmp = 2 - dist
    tmp2 = tmp*tmp
    tmp3 = tmp*tmp2
    w0 = (1/6)*tmp3
    w2 = ((2/3) - tmp2) + 0.5*tmp3
    d1 = dist - 1
    w3 = (1/6)*((d1*d1)*d1)
    return index.astype(np.int64), [w0, ((1 - w0) - w2) - w3, w2, w3]


class Case:
    """one mesh configuration: grid, centring, interpolation order, lattice shift, and the
    ghost count commons.load_params derives for them"""
    _nghosts = {}

    def __init__(self, N, order, cc, lattice):
        from concept_amd import commons
        from oracle import pm_general
        self.N, self.order, self.cc, self.lattice = N, order, cc, lattice
        # (0, 0, 0), (a, a, a), (0, a, a)
        which = {'sc': 0, 'bcc': 1, 'fcc': 1}[lattice]
        self.shift = tuple(float(s) for s in pm_general.lattice_shifts(lattice, cc)[which])
        key = (order, cc, lattice)
        if key not in Case._nghosts:
            p = commons.load_params({
                'boxsize': L_BOX, 'cell_centered': cc,
                'potential_options': {
                    'gridsize': {'global': {'gravity': {'pm': 64}}},
                    'interpolation': {'gravity': {'pm': ORDER_NAMES[order]}},
                    'interlace': {'gravity': {'pm': (lattice, lattice)}}},
                'select_forces': {'all': {'gravity': 'pm'}}})
            Case._nghosts[key] = int(p.nghosts)
        self.g = Case._nghosts[key]
        self.geom = {sign: pm_general.interp_geometry(L_BOX, N, self.g, self.shift, sign, cc)
                     for sign in (-1, +1)}
        self.cs = L_BOX/N

    def __repr__(self):
        return (f'N={self.N} order={self.order} cell_centered={self.cc} shift={self.shift} '
                f'nghosts={self.g}')

    def stencil(self, pos, sign):
        """first cells (n, 3) before the periodic wrap, and weights [axis][i] -> (n,)"""
        off, scale = self.geom[sign]
        first, w = [], []
        for d in range(3):
            i, wd = index_weights((pos[:, d] - off[d])*scale, self.order)
            first.append(i - self.g)
            w.append(wd)
        return np.stack(first, 1), w

    def to_pos(self, t, sign):
        """positions in [0, L) whose stencils start (rounding aside) at cell floor(t)"""
        off, scale = self.geom[sign]
        pos = np.mod((t + (self.g + T_SHIFT[self.order]))/scale + off[None, :], L_BOX)
        pos[pos >= L_BOX] = 0.0
        return pos


def cases(N, kind):
    """the matrix of one order: shifts (0,0,0), (a,a,a), (0,a,a) x cell- and vertex-centred"""
    if kind == 'cic':
        return [Case(N, 2, cc, 'sc') for cc in (True, False)]
    return [Case(N, kind, cc, lat) for cc in (True, False) for lat in ('sc', 'bcc', 'fcc')]


def ref_deposit(case, pos, contribution):
    """-> flat cell numbers touched, their sums (longdouble), sum|term| and term counts"""
    N, O = case.N, case.order
    first, w = case.stencil(pos, -1)
    flat, terms = [], []
    for i in range(O):
        wi = w[0][i]*contribution
        for j in range(O):
            wij = wi*w[1][j]
            for k in range(O):
                terms.append(wi if O == 1 else wij*w[2][k])
                flat.append((((first[:, 0] + i) % N)*N + (first[:, 1] + j) % N)*N
                            + (first[:, 2] + k) % N)
    flat, terms = np.concatenate(flat), np.concatenate(terms)
    cells, inv = np.unique(flat, return_inverse=True)
    total = np.zeros(cells.size, dtype=np.longdouble)
    np.add.at(total, inv, terms.astype(np.longdouble))
    mag = np.zeros(cells.size, dtype=np.longdouble)
    np.add.at(mag, inv, np.abs(terms).astype(np.longdouble))
    return cells, total, mag, np.bincount(inv, minlength=cells.size)


def ref_gather(case, pos, mom_dim, field, factor):
    """-> expected momentum column (longdouble) and the bound per particle"""
    N, O = case.N, case.order
    first, w = case.stencil(pos, +1)
    value = np.zeros(pos.shape[0], dtype=np.longdouble)
    mag = np.zeros(pos.shape[0], dtype=np.longdouble)
    for i in range(O):
        for j in range(O):
            wij = w[0][i]*w[1][j]
            for k in range(O):
                wgt = np.ones(pos.shape[0]) if O == 1 else wij*w[2][k]
                v = field[(first[:, 0] + i) % N, (first[:, 1] + j) % N, (first[:, 2] + k) % N]
                term = v.astype(np.longdouble)*wgt.astype(np.longdouble)
                value += term
                mag += np.abs(term)
    if factor != 1:
        value = value*np.longdouble(factor)
    expected = mom_dim.astype(np.longdouble) + value
    bound = abs(factor)*2*O**3*U*mag + U*np.abs(value) + U*np.abs(expected)
    return expected, bound


def worst_ratio(err, bound):
    """largest error/bound and where; a bound of 0 (all terms exactly 0) admits no error"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = np.where(err == 0, 0.0, err/np.where(bound > 0, bound, 1.0))
    ratio = np.where((bound <= 0) & (err != 0), np.inf, ratio)
    ratio = np.where(np.isnan(err), np.inf, ratio)
    worst = int(np.argmax(ratio))
    return float(ratio[worst]), worst


# -- the GPU side ----------------------------------------------------------------------------
@contextlib.contextmanager
def meshes():
    """get(case) -> the PotentialMesh of the case's grid; all closed at exit"""
    import torch
    from concept_amd.mesh import PotentialMesh
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    made = {}

    def get(case):
        key = (case.N, case.g, case.cc)
        if key not in made:
            made[key] = PotentialMesh(case.N, L_BOX, nghosts=case.g, cell_centered=case.cc)
        return made[key]
    try:
        yield get
    finally:
        for m in made.values():
            m.close()


def check_deposit(mesh, case, kind, pos, contribution, label):
    import torch
    mesh.zero()
    pos_d = torch.tensor(pos, device='cuda')
    if kind == 'cic':
        mesh.deposit(pos_d, contribution)
    else:
        mesh.deposit_general(pos_d, contribution, case.order, case.shift)
    got = np.ascontiguousarray(mesh.fetch_real()[:, :, :case.N]).reshape(-1)
    cells, total, mag, m = ref_deposit(case, pos, contribution)
    bound = 2*m*U*mag + U*np.abs(total)
    err = np.abs(got[cells].astype(np.longdouble) - total)
    ratio, worst = worst_ratio(err, bound)
    assert ratio <= 1, (f'{label} {case}: cell {np.unravel_index(cells[worst], (case.N,)*3)} '
                        f'got {got[cells[worst]]!r} expected {float(total[worst])!r} '
                        f'({m[worst]} terms), error/bound {ratio:.3g}')
    got[cells] = 0.0
    stray = np.flatnonzero(got)
    assert stray.size == 0, (f'{label} {case}: {stray.size} cells outside every stencil were '
                             f'written, first {np.unravel_index(stray[0], (case.N,)*3)}')
    return ratio


def random_field(mesh, N, rng):
    """a random mesh written with layers_write (NaN in the padding, which no stencil may
    read) -> its (N, N, N) host copy"""
    import torch
    field = rng.normal(0, 1, (N, N, N))
    per, pad = mesh.layer_doubles, mesh.pad
    buf = np.full((N, per), np.nan)
    rows = buf[:, :N*pad].reshape(N, N, pad)
    rows[:, :, :N] = field
    mesh.layers_write(0, N, torch.tensor(buf.reshape(-1), device='cuda'))
    return field


def run_gather(mesh, case, pos, mom, dim, factor):
    import torch
    pos_d = torch.tensor(pos, device='cuda')
    mom_d = torch.tensor(mom, device='cuda')
    mesh.gather_scalar(pos_d, mom_d, dim, case.order, case.shift, factor)
    torch.cuda.synchronize()
    return mom_d.cpu().numpy()


def check_gather(mesh, case, field, pos, mom, dim, factor, label):
    got = run_gather(mesh, case, pos, mom, dim, factor)
    expected, bound = ref_gather(case, pos, mom[:, dim], field, factor)
    others = [d for d in range(3) if d != dim]
    assert np.array_equal(got[:, others], mom[:, others]), f'{label} {case}: other columns moved'
    err = np.abs(got[:, dim].astype(np.longdouble) - expected)
    ratio, worst = worst_ratio(err, bound)
    assert ratio <= 1, (f'{label} {case}: particle {worst} at {pos[worst]!r} got '
                        f'{got[worst, dim]!r} expected {float(expected[worst])!r}, '
                        f'error/bound {ratio:.3g}')
    return ratio, got


# -- what the inputs are: first-cell spans of the chunks ---------------------------------------
def chunk_spans(case, pos, sign):
    """per chunk of 2048 consecutive particles, per axis: the span of the stencils' first cells,
    measured from the chunk's first particle through the periodic seam"""
    N = case.N
    first, _ = case.stencil(pos, sign)
    spans = []
    for b in range(0, pos.shape[0], CHUNK):
        c = first[b:b + CHUNK]
        rel = (c - c[0] + N//2) % N - N//2
        spans.append(rel.max(0) - rel.min(0))
    return np.array(spans)


# -- particle sets -----------------------------------------------------------------------------
CUBES = [(2, 24, 46), (24, 46, 2), (46, 2, 24), (2, 46, 24), (24, 2, 46), (46, 24, 2)]


def compact_set(case, sign, n, rng, origins=CUBES):
    """chunk c lies in the cube of 8 first cells at origins[c]"""
    t = np.empty((n, 3))
    for c, b in enumerate(range(0, n, CHUNK)):
        m = min(CHUNK, n - b)
        t[b:b + m] = np.array(origins[c % len(origins)]) + 0.001 + 7.998*rng.random((m, 3))
    pos = case.to_pos(t, sign)
    assert chunk_spans(case, pos, sign).max() <= 7
    return pos


def spread_set(case, sign, n, rng):
    """uniform particles; the first two of every chunk are 32 cells apart on every axis"""
    t = case.N*rng.random((n, 3))
    for b in range(0, n - 1, CHUNK):
        t[b + 1] = t[b] + 32.0
    pos = case.to_pos(t, sign)
    sizes = np.diff(np.append(np.arange(0, n, CHUNK), n))
    # (a tail chunk of one particle has no second particle)
    assert chunk_spans(case, pos, sign)[sizes >= 2].min() >= 31
    return pos


def seam_set(case, sign, rng):
    """seven compact cubes across one, two and all three faces of the box (the corner), with
    particles at exactly 0, at the last double below L and at the cell boundaries on both
    sides of the face"""
    L, cs = L_BOX, case.cs
    special = np.array([0.0, np.nextafter(L, 0), np.nextafter(0, 1),
                        cs, np.nextafter(cs, 0), np.nextafter(cs, L),
                        L - cs, np.nextafter(L - cs, 0), np.nextafter(L - cs, L),
                        0.5*cs, L - 0.5*cs, np.nextafter(0.5*cs, 0), np.nextafter(L - 0.5*cs, L)])
    masks = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
    parts = []
    for mask in masks:
        origin = np.where(np.array(mask) == 1, case.N - 4, 20)
        pos = case.to_pos(origin + 0.001 + 7.998*rng.random((CHUNK, 3)), sign)
        k = np.arange(3*special.size**2)
        for d, stride in zip(range(3), (1, special.size, 5)):
            if mask[d]:
                pos[k, d] = special[(k//stride) % special.size]
        parts.append(pos)
    pos = np.concatenate(parts)
    assert chunk_spans(case, pos, sign).max() <= 7
    return pos


def limit_set(case, sign, spans, origin, rng, n=2000):
    """one chunk whose first cells span exactly `spans`: corner particles pin the extents, the
    first particle sits in the middle (the spans are measured from it)"""
    spans = np.array(spans)
    cell = rng.integers(0, spans + 1, (n, 3))
    cell[0] = (spans + 1)//2
    for c in range(8):
        cell[1 + c] = [spans[d] if c >> d & 1 else 0 for d in range(3)]
    t = np.array(origin) + cell + rng.uniform(0.05, 0.95, (n, 3))
    pos = case.to_pos(t, sign)
    got = chunk_spans(case, pos, sign)
    assert got.shape[0] == 1 and tuple(got[0]) == tuple(spans), (got, spans)
    return pos


def limit_cases(order):
    """(label, gridsize, spans, origin): boxes at the limit of 4096 cells and one past it"""
    O = order
    out = [('16x16x16 cells', 64, (16 - O,)*3, (50, 3, 60)),
           ('17x16x16 cells', 64, (17 - O, 16 - O, 16 - O), (50, 3, 60)),
           ('16x16x17 cells', 64, (16 - O, 16 - O, 17 - O), (3, 60, 50)),
           ('4x4x256 cells, the whole z axis', 256, (4 - O, 4 - O, 256 - O), (254, 7, 100)),
           ('5x4x256 cells', 256, (5 - O, 4 - O, 256 - O), (254, 7, 100))]
    if O >= 2:  # (NGP: 256 first cells are the whole axis already)
        out.append(('4x4x257 cells', 256, (4 - O, 4 - O, 257 - O), (254, 7, 100)))
    if O == 4:
        out += [('16x16x16 cells = the whole 16-cell grid', 16, (12, 12, 12), (5, 11, 14)),
                ('17x16x16 cells on the 16-cell grid', 16, (13, 12, 12), (5, 11, 14)),
                ('17x15x16 cells on the 16-cell grid', 16, (13, 11, 12), (5, 11, 14))]
    return out


def switch_set(case, sign, rng):
    """two chunks (one inside the box, one across the seam) of particles on exact cell centres
    and cell edges, on the positions where the kernels' grid coordinate is a whole or a half
    number (where (int)x and (int)(x + 0.5) switch), and one and two ulp to either side"""
    L, cs = L_BOX, case.cs
    off, scale = case.geom[sign]

    def around(v):
        v = np.asarray(v, dtype=np.float64)
        lo1, hi1 = np.nextafter(v, -np.inf), np.nextafter(v, np.inf)
        return np.concatenate([v, lo1, hi1, np.nextafter(lo1, -np.inf), np.nextafter(hi1, np.inf)])
    parts = []
    for k0 in (40, 2*case.N - 5):
        pos = np.empty((CHUNK, 3))
        for d in range(3):
            half = np.arange(k0, k0 + 11)*(0.5*cs)            # centres and edges, 5 cells wide
            m = np.arange(k0, k0 + 11)*0.5 + np.floor(scale*-off[d])
            cand = np.concatenate([around(half), around(m/scale + off[d])])
            cand = np.mod(cand, L)
            cand[cand >= L] = 0.0
            pos[:, d] = rng.choice(cand, CHUNK)
        parts.append(pos)
    pos = np.concatenate(parts)
    assert chunk_spans(case, pos, sign).max() <= 7
    return pos


def contribution_of(i):
    """alternating sign: a negative deposit must pass the flush like a positive one"""
    return (1.37, -0.7313)[i % 2]


# -- scenarios 1-6: deposit ----------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_deposit_compact_chunks(kind):
    """Scenario 1: every chunk in its own cube of 8 first cells (a box of at most 11^3 = 1331
    cells: the box path at every order); 5*2048 + 1 (a tail chunk of one), 3*2048 - 1, 2048."""
    rng = np.random.default_rng(101)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, kind)):
            for n in COUNTS:
                pos = compact_set(case, -1, n, rng)
                worst = max(worst, check_deposit(get(case), case, kind, pos,
                                                 contribution_of(ci), f'compact n={n}'))
    print(f'\ndeposit compact {kind}: error/bound {worst:.3f}')


@pytest.mark.parametrize('kind', KINDS)
def test_deposit_spread_chunks(kind):
    """Scenario 2: chunks that hold two particles 32 cells apart on every axis (a box of at
    least 32^3 cells: the direct path), and the compact particles of scenario 1 in shuffled
    memory order (every chunk then holds particles of several cubes)."""
    rng = np.random.default_rng(102)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, kind)):
            for n in COUNTS:
                pos = spread_set(case, -1, n, rng)
                worst = max(worst, check_deposit(get(case), case, kind, pos,
                                                 contribution_of(ci + 1), f'spread n={n}'))
                pos = compact_set(case, -1, n, rng)[rng.permutation(n)]
                worst = max(worst, check_deposit(get(case), case, kind, pos,
                                                 contribution_of(ci), f'shuffled n={n}'))
    print(f'\ndeposit spread {kind}: error/bound {worst:.3f}')


@pytest.mark.parametrize('kind', KINDS)
def test_deposit_across_the_seam(kind):
    """Scenario 3: compact cubes across one, two and three faces of the box."""
    rng = np.random.default_rng(103)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, kind)):
            pos = seam_set(case, -1, rng)
            worst = max(worst, check_deposit(get(case), case, kind, pos, contribution_of(ci),
                                             'seam'))
    print(f'\ndeposit seam {kind}: error/bound {worst:.3f}')


@pytest.mark.parametrize('kind', KINDS)
def test_deposit_at_the_lds_limit(kind):
    """Scenario 4: boxes of exactly 4096 cells, one cell over, a box that covers a whole axis
    (256 cells of z: the LDS ring maps every z cell once), the same one cell wider, and with
    PCS the whole 16-cell grid.  Whichever path a chunk takes, the mesh must match."""
    rng = np.random.default_rng(104)
    worst = 0.0
    with meshes() as get:
        for label, N, spans, origin in limit_cases(2 if kind == 'cic' else kind):
            for ci, case in enumerate(cases(N, kind)):
                pos = limit_set(case, -1, spans, origin, rng)
                worst = max(worst, check_deposit(get(case), case, kind, pos,
                                                 contribution_of(ci), label))
    print(f'\ndeposit limit {kind}: error/bound {worst:.3f}')


@pytest.mark.parametrize('kind', KINDS)
def test_deposit_contention_and_switch_points(kind):
    """Scenario 5: 3*2048 particles on one spot (every LDS atomic of a chunk contends), and
    particles on and next to the points where the cell index switches."""
    rng = np.random.default_rng(105)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, kind)):
            spot = np.tile(np.array([[0.2093, 0.7317, 0.9991]])*L_BOX, (3*CHUNK, 1))
            worst = max(worst, check_deposit(get(case), case, kind, spot, contribution_of(ci),
                                             'one spot'))
            pos = switch_set(case, -1, rng)
            worst = max(worst, check_deposit(get(case), case, kind, pos, contribution_of(ci + 1),
                                             'switch points'))
    print(f'\ndeposit contention {kind}: error/bound {worst:.3f}')


# -- scenarios 1-5: gather -----------------------------------------------------------------------
def gather_both_orders(mesh, case, field, pos, rng, dim, factor, label):
    """the gather in the given memory order against the reference, and in a shuffled order:
    the same particle must receive the same bits"""
    n = pos.shape[0]
    mom = rng.normal(0, 1, (n, 3))
    ratio, got = check_gather(mesh, case, field, pos, mom, dim, factor, label)
    perm = rng.permutation(n)          # row r of the shuffled arrays is particle perm[r]
    shuffled = run_gather(mesh, case, pos[perm], mom[perm], dim, factor)
    back = np.empty_like(shuffled)
    back[perm] = shuffled
    same = back.view(np.uint64) == got.view(np.uint64)
    assert same.all(), (f'{label} {case}: {np.count_nonzero(~same.all(1))} particles gather '
                        f'different bits in shuffled memory order, first '
                        f'{int(np.flatnonzero(~same.all(1))[0])}')
    return ratio


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_gather_compact_and_shuffled_chunks(order):
    """Scenarios 1 and 2 of the gather: compact chunks (the box is copied into LDS and read
    there) against the reference and, bit for bit, against the same particles in shuffled
    order (chunks of several cubes: global reads)."""
    rng = np.random.default_rng(201)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, order)):
            field = random_field(get(case), 64, rng)
            for n in COUNTS:
                pos = compact_set(case, +1, n, rng)
                worst = max(worst, gather_both_orders(get(case), case, field, pos, rng, ci % 3,
                                                      (-0.37, 1.0)[ci % 2], f'compact n={n}'))
    print(f'\ngather compact {order}: error/bound {worst:.3f}')


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_gather_spread_chunks(order):
    """Scenario 2 of the gather: chunks with two particles 32 cells apart on every axis."""
    rng = np.random.default_rng(202)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, order)):
            field = random_field(get(case), 64, rng)
            for n in COUNTS:
                pos = spread_set(case, +1, n, rng)
                mom = rng.normal(0, 1, (n, 3))
                worst = max(worst, check_gather(get(case), case, field, pos, mom, (ci + 1) % 3,
                                                (1.0, 2.5)[ci % 2], f'spread n={n}')[0])
    print(f'\ngather spread {order}: error/bound {worst:.3f}')


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_gather_across_the_seam(order):
    """Scenario 3 of the gather."""
    rng = np.random.default_rng(203)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, order)):
            field = random_field(get(case), 64, rng)
            pos = seam_set(case, +1, rng)
            worst = max(worst, gather_both_orders(get(case), case, field, pos, rng, ci % 3,
                                                  (-0.37, 1.0)[ci % 2], 'seam'))
    print(f'\ngather seam {order}: error/bound {worst:.3f}')


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_gather_at_the_lds_limit(order):
    """Scenario 4 of the gather."""
    rng = np.random.default_rng(204)
    worst = 0.0
    with meshes() as get:
        for N in (64, 256, 16):
            fields = {}
            for label, N_case, spans, origin in limit_cases(order):
                if N_case != N:
                    continue
                for ci, case in enumerate(cases(N, order)):
                    mesh = get(case)
                    if id(mesh) not in fields:
                        fields[id(mesh)] = random_field(mesh, N, rng)
                    pos = limit_set(case, +1, spans, origin, rng)
                    worst = max(worst, gather_both_orders(mesh, case, fields[id(mesh)], pos, rng,
                                                          ci % 3, (-0.37, 1.0)[ci % 2], label))
    print(f'\ngather limit {order}: error/bound {worst:.3f}')


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_gather_contention_and_switch_points(order):
    """Scenario 5 of the gather."""
    rng = np.random.default_rng(205)
    worst = 0.0
    with meshes() as get:
        for ci, case in enumerate(cases(64, order)):
            field = random_field(get(case), 64, rng)
            spot = np.tile(np.array([[0.2093, 0.7317, 0.9991]])*L_BOX, (3*CHUNK, 1))
            worst = max(worst, gather_both_orders(get(case), case, field, spot, rng, ci % 3,
                                                  (-0.37, 1.0)[ci % 2], 'one spot'))
            pos = switch_set(case, +1, rng)
            worst = max(worst, gather_both_orders(get(case), case, field, pos, rng, (ci + 2) % 3,
                                                  (1.0, -0.37)[ci % 2], 'switch points'))
    print(f'\ngather contention {order}: error/bound {worst:.3f}')


# -- end to end ----------------------------------------------------------------------------------
def blob_positions(n_blob=7500, gridsize=64):
    """four tight Gaussian blobs (sigma = 0.7 cells, far apart; one sits on the corner of the
    box).  Tile-sorted, the chunks inside a blob are compact, those across two blobs are not;
    shuffled, none is."""
    rng = np.random.default_rng(77)
    cs = L_BOX/gridsize
    centres = np.array([[0.3, 63.8, 0.1], [20.4, 31.7, 45.2], [50.9, 10.2, 12.5],
                        [40.1, 52.6, 60.3]])*cs
    parts = [c + rng.normal(0, 0.7*cs, (n_blob, 3)) for c in centres]
    pos = np.mod(np.concatenate(parts), L_BOX)
    pos[pos >= L_BOX] = 0.0
    return pos[rng.permutation(pos.shape[0])]


@pytest.mark.parametrize('interp,lattice,diff', [('TSC', 'bcc', 2), ('PCS', 'fcc', 4)])
def test_gravity_pm_on_tile_sorted_blobs_vs_oracle(interp, lattice, diff):
    """gravity('pm') with interlaced TSC / PCS on tile-sorted clustered particles (the general
    deposit and gather work through their LDS boxes inside the full pipeline: ghost folds,
    Fourier shifts, downstream gather) against the CPU oracle, at the bar of
    test_random_configurations_vs_oracle.  Also run over 2 and 4 domains."""
    from concept_amd import comm, commons, interactions
    from concept_amd.species import Component
    from oracle import pm_general
    gs = 64
    p = commons.load_params({
        'boxsize': L_BOX,
        'potential_options': {
            'gridsize': {'global': {'gravity': {'pm': gs}}},
            'interpolation': {'gravity': {'pm': interp}},
            'interlace': {'gravity': {'pm': (lattice, lattice)}},
            'differentiation': {'cdm': {'gravity': {'pm': diff}}}},
        'select_forces': {'all': {'gravity': 'pm'}}})
    pos = blob_positions(gridsize=gs)
    n = pos.shape[0]
    rng = np.random.default_rng(78)
    mom = rng.normal(0, 1, (n, 3))
    mass = 1.7
    part = Component('cdm', 'matter', N=n, mass=mass)
    part.populate(pos, 'pos')
    part.populate(mom, 'mom')
    part.tile_sort()
    if comm.active() is None:
        # the input is what it is meant to be: some chunk of 2048 consecutive particles lies
        # within 7 cells on every axis (8 first cells: a box at every order)
        sorted_pos = part.pos.cpu().numpy()
        widths = [np.ptp(sorted_pos[b:b + CHUNK], axis=0).max()
                  for b in range(0, n - CHUNK + 1, CHUNK)]
        assert min(widths) <= 7*L_BOX/gs, min(widths)
    sdt = {'1': 0.02, ('a**(-3*w_eff)', 'cdm'): 0.021, ('a**(-3*w_eff-1)', 'cdm'): 0.033}
    interactions.gravity('pm', [part], [part], sdt, 'long-range', False)
    o_part = dict(kind='particles', pos=pos, mom=mom.copy(), mass=mass, dt_dens=0.033,
                  dt_kick=0.021, diff_order=diff)
    pm_general.particle_mesh(
        [o_part], boxsize=L_BOX, gridsize=gs, G_Newton=p.G_Newton, dt_1=0.02,
        light_speed=p.light_speed, nghosts=p.nghosts,
        interp_order=commons.interpolation_orders[interp], interlace=(lattice, lattice))
    got, ref = part.host('mom'), o_part['mom']
    scale = np.abs(ref - mom).max()
    assert scale > 0
    err = np.abs(got - ref).max()
    print(f'\ngravity pm {interp}/{lattice}: error {err/scale:.3g} of the largest kick')
    assert err <= 1e-11*scale + 4e-16*np.abs(ref).max(), err/scale


def test_powerspec_sorted_equals_shuffled():
    """compute_powerspec with its default options (PCS, interlaced) on the blob particles in
    tile order (LDS boxes) and in shuffled order (global atomics): the same power to 1e-12,
    the bar of the power-spectrum goldens, and the same mode counts."""
    import warnings
    from concept_amd import analysis, commons
    from concept_amd.species import Component
    gs = 64
    p = commons.load_params({'boxsize': L_BOX, 'powerspec_options': {'gridsize': gs},
                             'powerspec_select': {'matter': True}})
    opts = p.powerspec_options
    assert max(opts['interpolation'].values()) == 4
    assert any(v != 'sc' for v in opts['interlace'].values())
    pos = blob_positions(gridsize=gs)
    n = pos.shape[0]
    results = []
    for sort in (True, False):
        c = Component('matter', 'matter', N=n, mass=p.ρ_mbar*L_BOX**3/n)
        c.populate(pos, 'pos')
        c.populate(np.zeros((n, 3)), 'mom')
        if sort:
            c.tile_sort()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            decl = analysis.get_powerspec_declarations([c])[0]
            analysis.compute_powerspec(decl)
        assert decl.interpolation == 4 and decl.interlace != 'sc'
        results.append((decl.power.copy(), np.array(decl.n_modes).copy()))
    (P_sorted, modes_sorted), (P_shuffled, modes_shuffled) = results
    np.testing.assert_array_equal(modes_sorted, modes_shuffled)
    assert np.all(np.isfinite(P_shuffled)) and np.all(P_shuffled > 0)
    rel = np.abs(P_sorted - P_shuffled)/np.abs(P_shuffled)
    print(f'\npower spectrum sorted vs shuffled: {rel.max():.3g}')
    assert rel.max() <= 1e-12, rel.max()


def test_powerspec_cic_sorted_equals_shuffled():
    """compute_powerspec with CIC on the 'sc' lattice, where tile-sorted components — what
    Timeloop hands to a dump after a drift — take the LDS-tiled deposit (it assigns the mesh:
    no zero-fill pass, no global atomics) and shuffled ones the direct deposit onto a zeroed
    mesh: the same power to 1e-12, the bar of the power-spectrum goldens, and the same mode
    counts.  A 32^3 grid is two 16-cell tiles per axis, the smallest on which a tile has a
    lower neighbour and a wrapped one.  Also run over 2 and 4 domains."""
    import warnings
    from concept_amd import analysis, commons
    from concept_amd.mesh import PotentialMesh
    from concept_amd.species import Component
    gs = 32
    p = commons.load_params({
        'boxsize': L_BOX,
        'potential_options': {'gridsize': {'global': {'gravity': {'pm': gs}}}},
        'select_forces': {'all': {'gravity': 'pm'}},
        'powerspec_options': {'gridsize': gs, 'interpolation': 'CIC', 'interlace': False},
        'powerspec_select': {'matter': True}})
    pos = blob_positions(n_blob=5000, gridsize=gs)
    n = pos.shape[0]
    results = []
    for sort in (True, False):
        c = Component('matter', 'matter', N=n, mass=p.ρ_mbar*L_BOX**3/n)
        c.populate(pos, 'pos')
        c.populate(np.zeros((n, 3)), 'mom')
        if sort:
            c.tile_sort()
        calls = []
        with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for name in ('zero', 'deposit', 'deposit_tiled', 'deposit_general'):
                def counted(self, *args, _name=name, _method=getattr(PotentialMesh, name), **kw):
                    calls.append(_name)
                    return _method(self, *args, **kw)
                mp.setattr(PotentialMesh, name, counted)
            decl = analysis.get_powerspec_declarations([c])[0]
            analysis.compute_powerspec(decl)
        assert decl.interpolation == 2 and decl.gridsize == gs
        assert calls == (['deposit_tiled'] if sort else ['zero', 'deposit']), calls
        results.append((decl.power.copy(), np.array(decl.n_modes).copy()))
    (P_sorted, modes_sorted), (P_shuffled, modes_shuffled) = results
    np.testing.assert_array_equal(modes_sorted, modes_shuffled)
    assert np.all(np.isfinite(P_shuffled)) and np.all(P_shuffled > 0)
    rel = np.abs(P_sorted - P_shuffled)/np.abs(P_shuffled)
    print(f'\npower spectrum CIC sorted vs shuffled: {rel.max():.3g}')
    assert rel.max() <= 1e-12, rel.max()
