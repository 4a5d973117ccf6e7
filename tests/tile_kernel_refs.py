"""Plain NumPy references of the two tile kernels of concept_amd/csrc/cg_tiled_kernels.hip
(k_deposit_cic_pull, k_gather_kick_tiled) and the deliberately placed particles they are tested
with (tests/test_tile_kernel_refs_host.py pins both on the CPU, tests/test_gpu_tile_kernels.py
compares the kernels with them).

Order of every expression, from the kernels' own comments:
    index map   x = (pos - off)*scale, index = trunc(x), w1 = x - index, w0 = 1 - w1
                (mesh.py:1577-1606 deposit, 408-432 gather; off and scale of oracle.*_geometry)
    deposit     term = ((w_x*contribution)*w_y)*w_z in float64 (mesh.py:5142-5155); the sum per
                cell is the reference's business: np.longdouble here
    force cell  c1*(phi[+1] - phi[-1]) [- c2*(phi[+2] - phi[-2])] in float64 (mesh.py:4966-4981)
    kick        sum over the 8 cells of f*((w_x*w_y)*w_z), weights in float64, products and sum in
                np.longdouble; times factor; added to the momentum
    drift       oracle.drift (species.py:2194-2196), pinned by test_oracle_golden.py
    key         8*tile + bucket of the lower CIC cell (cg_tiles.h tile_of)
"""
import numpy as np

from oracle import oracle

LD = np.longdouble
NGHOSTS = 2
# (N, T): the two smallest grids of every tile extent, 2 and 3 tiles per dimension
SIZES = [(4, 2), (6, 2), (8, 4), (12, 4), (16, 8), (24, 8), (32, 16), (48, 16)]
L = 96.0        # L/N is a whole number for every size
DTM = 0.5       # dt_over_mass of the tests: a power of two


def factor_of(N):
    """kick factor of the tests: |kick|*DTM stays below 1/16 cell for normal potentials (|f| <
    8/cell), so that the placed moves land where they were aimed"""
    return -(L/N)**2/128


def index_weights(x1d, N, boxsize, nghosts=NGHOSTS, cell_centered=True, gather=False):
    """lower cell before the periodic wrap (int64), w0, w1 along one axis"""
    if gather:
        off, scale = oracle.gather_geometry(boxsize, N + 2*nghosts, nghosts, cell_centered)
    else:
        off, scale = oracle.deposit_geometry(boxsize, N, nghosts, cell_centered)
    x = (np.asarray(x1d, dtype=np.float64) - off[0])*scale
    idx = x.astype(np.int64)
    dist = x - idx
    return idx - nghosts, 1 - dist, dist


def lower_cells(pos, N, boxsize, nghosts=NGHOSTS, cell_centered=True):
    """(n, 3) lower CIC cells before the wrap: -1 .. N - 1"""
    return np.stack([index_weights(pos[:, d], N, boxsize, nghosts, cell_centered)[0]
                     for d in range(3)], 1)


def deposit_ref(pos, N, boxsize, nghosts, cell_centered, contribution):
    """-> density (N, N, N) np.longdouble, stats (2, N, N, N): the number m of terms and the
    sum of |term| of every cell"""
    iw = [index_weights(pos[:, d], N, boxsize, nghosts, cell_centered) for d in range(3)]
    dens = np.zeros(N**3, dtype=LD)
    m = np.zeros(N**3, dtype=np.int64)
    mag = np.zeros(N**3, dtype=LD)
    for i in range(2):
        wi = iw[0][1 + i]*contribution
        for j in range(2):
            wij = wi*iw[1][1 + j]
            for k in range(2):
                term = wij*iw[2][1 + k]
                cell = ((np.mod(iw[0][0] + i, N)*N + np.mod(iw[1][0] + j, N))*N
                        + np.mod(iw[2][0] + k, N))
                np.add.at(dens, cell, term.astype(LD))
                np.add.at(mag, cell, np.abs(term).astype(LD))
                np.add.at(m, cell, 1)
    shape = (N, N, N)
    return dens.reshape(shape), np.stack([m.astype(LD).reshape(shape), mag.reshape(shape)])


def force_cells(phi, N, boxsize, order):
    """the three force grids of diff_domaingrid in float64, from the periodic potential"""
    dx = boxsize/N
    out = []
    for d in range(3):
        def at(s):
            return np.roll(phi, -s, axis=d)
        if order == 2:
            c1 = (1.0/2)/dx
            out.append(c1*(at(1) - at(-1)))
        elif order == 4:
            c1, c2 = (2.0/3)/dx, (1.0/12)/dx
            out.append(c1*(at(1) - at(-1)) - c2*(at(2) - at(-2)))
        else:
            raise ValueError(order)
    return out


def gather_kick_ref(phi, pos, mom, N, boxsize, order, factor, nghosts=NGHOSTS,
                    cell_centered=True):
    """-> kicked momenta (n, 3) np.longdouble, sum of |w*f| (n, 3) np.longdouble"""
    phi = np.asarray(phi, dtype=np.float64)
    assert phi.shape == (N, N, N)
    force = force_cells(phi, N, boxsize, order)
    iw = [index_weights(pos[:, d], N, boxsize, nghosts, cell_centered, gather=True)
          for d in range(3)]
    val = np.zeros(pos.shape, dtype=LD)
    mag = np.zeros(pos.shape, dtype=LD)
    for i in range(2):
        for j in range(2):
            wij = iw[0][1 + i]*iw[1][1 + j]
            for k in range(2):
                w = (wij*iw[2][1 + k]).astype(LD)
                cell = (np.mod(iw[0][0] + i, N), np.mod(iw[1][0] + j, N),
                        np.mod(iw[2][0] + k, N))
                for d in range(3):
                    term = force[d][cell].astype(LD)*w
                    val[:, d] += term
                    mag[:, d] += np.abs(term)
    return np.asarray(mom, dtype=LD) + LD(factor)*val, mag


def keys_ref(pos, N, boxsize, T, nghosts=NGHOSTS, cell_centered=True):
    """8*tile + bucket (cg_tiles.h tile_of) on a single domain"""
    cell = np.mod(lower_cells(pos, N, boxsize, nghosts, cell_centered), N)
    nt = N//T
    t = cell//T
    last = (cell % T == T - 1).astype(np.int64)
    return ((t[:, 0]*nt + t[:, 1])*nt + t[:, 2])*8 + 4*last[:, 0] + 2*last[:, 1] + last[:, 2]


def drift_ref(pos, mom, dt_over_mass, boxsize):
    """oracle.drift on a copy"""
    return oracle.drift(np.array(pos, dtype=np.float64, order='C'),
                        np.ascontiguousarray(mom, dtype=np.float64), dt_over_mass, boxsize)


def potential(N, seed):
    """NOT a solved potential: independent normal values, so that a misread neighbour is a
    wrong kick of order one"""
    return np.random.default_rng(seed).normal(0.0, 1.0, (N, N, N))


def region_capacities(count):
    """cg_predict_regions: room of every (tile, bucket) from its present population"""
    count = np.asarray(count, dtype=np.int64)
    return count + count//4 + 32


def aim_at_zero(placed, phi, order):
    """-> a copy of the placed momenta in which the rows of edges['to_zero'] (coordinate exactly
    0 along their axis) get minus the kick they will receive, a relative 2^-44 more: the kicked
    momentum is a negative number so small that pos + mom*DTM rounds to the box size when the
    modulo lifts it, which Component.drift turns into 0.  (The kick does not depend on the
    momentum; its own rounding on the device, < 2^-49 of it, cannot change the sign.)"""
    pos, N = placed['pos'], placed['N']
    mom = placed['mom'].copy()
    rows = np.array([r for r, _ in placed['edges']['to_zero']])
    kick = gather_kick_ref(phi, pos[rows], np.zeros((rows.size, 3)), N, L, order,
                           factor_of(N))[0].astype(np.float64)
    for n, (r, d) in enumerate(placed['edges']['to_zero']):
        assert pos[r, d] == 0.0 and abs(kick[n, d]) > 1e-6*abs(factor_of(N))
        mom[r, d] = -kick[n, d] - abs(kick[n, d])*2.0**-44
    return mom


# -- the placed input -------------------------------------------------------------------------
NAMED = {'layers': 0, 'empty': 1, 'full512': 2, 'full513': 3, 'no_bucket0': 4, 'only_bucket0': 5}
NO_BUCKET0_POPS = (0, 7, 40, 3, 64, 65, 1, 130)    # bucket 5: a run that crosses a wave
ONLY_BUCKET0_POP = 200


def _exact_face(face, N):
    """a double within 64 ulp of the cell face whose upper weight is exactly 0 (the index map
    carries factors 1 +- eps: the face itself need not be it), else the face"""
    cand = [face]
    lo = hi = face
    for _ in range(64):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cand += [lo, hi]
    cand = np.array(cand)
    w1 = index_weights(cand, N, L)[2]
    hit = np.flatnonzero(w1 == 0.0)
    return float(cand[hit[0]]) if hit.size else float(face)


def placed_particles(N, T, boxsize=L, seed=0):
    """-> dict(N, T, pos, mom, edges): the input of the tile-kernel tests (module docstring of
    test_gpu_tile_kernels.py).  Tiles 0 .. 5 are the named ones (NAMED), the last tile takes the
    particles at the box's seam, every other tile a seeded uniform fill.  edges names the rows
    and tiles that reach each edge; the host test recomputes every claim from pos with keys_ref."""
    assert boxsize == L and N % T == 0
    nt, cs = N//T, L/N
    ntiles = nt**3
    seam = ntiles - 1
    rng = np.random.default_rng(1000*N + seed)
    pos_parts, mom_parts = [], []
    count = [0]

    def origin(tile):
        return np.array([tile//(nt*nt), (tile//nt) % nt, tile % nt])*T

    def add(cells, sigma, frac=None):
        """particles in the given cells (k, 3), at least 1/16 cell from the faces; momenta of
        rms sigma cells per drift -> their rows"""
        cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
        k = cells.shape[0]
        if frac is None:
            frac = rng.uniform(1/16, 15/16, (k, 3))
        # cell c holds the positions [(c + 1/2)*cs, (c + 3/2)*cs) through the box's seam
        pos_parts.append(np.mod((cells + 0.5 + frac)*cs, L))
        mom_parts.append(rng.normal(0.0, sigma*cs/DTM, (k, 3)))
        rows = np.arange(count[0], count[0] + k)
        count[0] += k
        return rows

    def bucket_cells(tile, f, k):
        """k cells of bucket f of a tile"""
        c = rng.integers(0, T - 1, (k, 3))
        for d in range(3):
            if f & (4 >> d):
                c[:, d] = T - 1
        return origin(tile) + c

    edges = {'tiles': dict(NAMED, seam=seam), 'run65': (NAMED['no_bucket0'], 5)}
    # (rms drift in cells: the empty tile's regions, 32 slots each, must hold who moves in)
    QUIET, LIVELY = 0.02, 0.1
    # first and last layer of a tile along every dimension: all cells with a coordinate 0 or T-1
    g = np.stack(np.meshgrid(*[np.arange(T)]*3, indexing='ij'), -1).reshape(-1, 3)
    shell = g[((g == 0) | (g == T - 1)).any(1)]
    edges['layers'] = add(origin(NAMED['layers']) + shell, LIVELY)
    add(origin(NAMED['layers']) + g[rng.integers(0, g.shape[0], min(3*T**3, 1000))], LIVELY)
    # a full batch, and a batch with one live lane
    for name, k in (('full512', 512), ('full513', 513)):
        add(origin(NAMED[name]) + rng.integers(0, T, (k, 3)), QUIET)
    for f, k in enumerate(NO_BUCKET0_POPS):
        add(bucket_cells(NAMED['no_bucket0'], f, k), QUIET)
    add(bucket_cells(NAMED['only_bucket0'], 0, ONLY_BUCKET0_POP), QUIET)
    # the fill of every other tile
    for tile in range(len(NAMED), ntiles):
        add(origin(tile) + g[rng.integers(0, g.shape[0], min(3*T**3, 1000))], LIVELY)

    # the seam tile: coordinates exactly 0, the last double below L, exactly on a cell face
    inside = origin(seam) + (T - 2)        # a cell of the last tile that is not its last
    top = np.nextafter(L, 0.0)
    rows = add(np.tile(inside, (5, 1)), LIVELY)
    edges['coord0'], edges['coord_top'] = rows[:3], rows[2:5]
    fix = [(rows[0], (0.0, 0.0, 0.0)), (rows[1], (0.0, None, None)), (rows[2], (None, top, 0.0)),
           (rows[3], (top, top, top)), (rows[4], (None, None, top))]
    face = _exact_face((N - 0.5)*cs, N)    # between the cells N - 2 and N - 1
    rows = add(np.tile(inside, (9, 1)), LIVELY)
    edges['face'] = rows
    for n, r in enumerate(rows):
        v = [None, None, None]
        v[n % 3] = (face, np.nextafter(face, -np.inf), np.nextafter(face, np.inf))[n//3]
        fix.append((r, tuple(v)))
    # lower cell -1 before the wrap: the first half cell of the box, per axis
    edges['lower_m1'] = []
    for d in range(3):
        rows = add(np.tile(inside, (8, 1)), LIVELY)
        edges['lower_m1'].append(rows)
        for r in rows:
            v = [None, None, None]
            v[d] = float(rng.uniform(1/16, 7/16))*cs
            fix.append((r, tuple(v)))
    # aimed moves (momenta in cells per drift along one axis, nothing along the others)
    aimed = []
    edges.update(move_tile=[], wrap_up=[], wrap_down=[], wrap_twice=[], to_zero=[])
    free = len(NAMED) if ntiles - 1 > len(NAMED) else seam     # a fill tile
    for d in range(3):
        e = np.eye(3, dtype=np.int64)[d]
        r = add(origin(free) + e*0 + (T - 2)*(1 - e), 0.0)[0]        # one tile further along d
        aimed.append((r, d, float(T)))
        edges['move_tile'].append(r)
        r = add(inside, 0.0)[0]                                       # through the upper face
        aimed.append((r, d, 2.0))
        edges['wrap_up'].append(r)
        r = add(origin(NAMED['layers']), 0.0)[0]                      # through the lower face
        aimed.append((r, d, -2.0))
        edges['wrap_down'].append(r)
        r = add(inside, 0.0)[0]                                       # once round and on
        aimed.append((r, d, float(N + 1)))
        edges['wrap_twice'].append(r)
        r = add(inside, 0.0)[0]                                       # see aim_at_zero
        fixv = [None, None, None]
        fixv[d] = 0.0
        fix.append((r, tuple(fixv)))
        edges['to_zero'].append((int(r), d))
    # at rest: the kick is added to a momentum of 0, so its error is that of the sum alone
    edges['at_rest'] = np.concatenate([
        add(origin(free) + g[rng.integers(0, g.shape[0], 48)], 0.0),
        add(origin(NAMED['layers']) + shell[rng.integers(0, shell.shape[0], 48)], 0.0),
        add(np.tile(inside, (16, 1)), 0.0),
        add(np.tile(origin(seam) + (T - 1), (16, 1)), 0.0)])    # the box's last cell: bucket 7
    pos = np.concatenate(pos_parts)
    mom = np.concatenate(mom_parts)
    for r, v in fix:
        for d in range(3):
            if v[d] is not None:
                pos[r, d] = v[d]
    for r, d, cells in aimed:
        mom[r] = 0.0
        mom[r, d] = cells*cs/DTM
    # memory order: random, so that the sort has work to do (rows in edges follow)
    perm = rng.permutation(pos.shape[0])
    inv = np.argsort(perm)
    pos, mom = pos[perm], mom[perm]
    for key, val in list(edges.items()):
        if key in ('tiles', 'run65'):
            continue
        if key == 'to_zero':
            edges[key] = [(int(inv[r]), d) for r, d in val]
        elif isinstance(val, list):
            edges[key] = [inv[v] for v in val]
        else:
            edges[key] = inv[val]
    assert (pos >= 0).all() and (pos < L).all()
    return {'N': N, 'T': T, 'pos': np.ascontiguousarray(pos), 'mom': np.ascontiguousarray(mom),
            'edges': edges}


def check_placed(placed, verbose=False):
    """every edge of the placed input, recomputed from the positions with keys_ref (cheap: the
    GPU tests call it again on what they upload) -> per-(tile, bucket) populations"""
    N, T, pos, mom, e = placed['N'], placed['T'], placed['pos'], placed['mom'], placed['edges']
    nt = N//T
    ntiles = nt**3
    keys = keys_ref(pos, N, L, T)
    pops = np.bincount(keys, minlength=8*ntiles).reshape(ntiles, 8)
    t = e['tiles']
    assert len(set(t.values())) == len(t) and max(t.values()) == ntiles - 1
    assert pops[t['empty']].sum() == 0
    assert pops[t['full512']].sum() == 512 and pops[t['full513']].sum() == 513
    assert tuple(pops[t['no_bucket0']]) == NO_BUCKET0_POPS and NO_BUCKET0_POPS[0] == 0
    assert all(p > 0 for p in NO_BUCKET0_POPS[1:])
    assert tuple(pops[t['only_bucket0']]) == (ONLY_BUCKET0_POP,) + (0,)*7
    assert pops[e['run65'][0], e['run65'][1]] == 65
    # a particle in every cell of the first and of the last layer of the tile, per dimension
    cell = np.mod(lower_cells(pos[e['layers']], N, L), N)
    assert (keys[e['layers']]//8 == t['layers']).all()
    for d in range(3):
        for la in (0, T - 1):
            sel = cell[cell[:, d] % T == la]
            assert np.unique(sel, axis=0).shape[0] == T*T, (d, la)
    # the seam
    low = lower_cells(pos, N, L)
    assert (pos[e['coord0']] == 0.0).any(1).all() and (pos[e['coord0'][0]] == 0.0).all()
    top = np.nextafter(L, 0.0)
    assert (pos[e['coord_top']] == top).any(1).all()
    assert (low[pos == 0.0] == -1).all() and (low[pos == top] == N - 1).all()
    for d in range(3):
        rows = e['lower_m1'][d]
        assert (low[rows, d] == -1).all() and (keys[rows]//8 == t['seam']).all()
        assert ((keys[rows] >> (2 - d)) & 1).all()      # the last cell of the last tile
    # on a cell face: one weight 1 and the other 0 (or within 2^-44 of it where no double near
    # the face gives an exact 0), on both sides of it
    w = np.stack([index_weights(pos[e['face'], d], N, L)[2] for d in range(3)], 1)
    onface = np.minimum(w, 1 - w).min(1)
    assert (onface <= 2.0**-44).all()
    exact = int((w == 0.0).any(1).sum())
    assert exact >= 1, 'no particle with a weight of exactly 0'
    cells_at_face = {int(low[r, n % 3]) for n, r in enumerate(e['face'])}
    assert cells_at_face == {N - 2, N - 1}
    if verbose:
        print(f'N {N} T {T}: {pos.shape[0]} particles, {exact} of {len(e["face"])} face '
              f'particles with a weight of exactly 0')
    # the aimed moves, by the drift without a kick (the kick is < 1/16 cell: factor_of)
    new = drift_ref(pos, mom, DTM, L)
    nkeys = keys_ref(new, N, L, T)
    for d in range(3):
        r = e['move_tile'][d]
        assert nkeys[r]//8 != keys[r]//8 and mom[r, d] > 0
        r = e['wrap_up'][d]
        assert new[r, d] < pos[r, d] and mom[r, d] > 0
        r = e['wrap_down'][d]
        assert new[r, d] > pos[r, d] and mom[r, d] < 0
        r = e['wrap_twice'][d]
        assert pos[r, d] + mom[r, d]*DTM > 2*L - 3*L/N
    assert ((nkeys//8 == keys//8) & (nkeys != keys)).any(), 'nobody changes bucket only'
    for r, d in e['to_zero']:
        assert pos[r, d] == 0.0
    assert e['at_rest'].size == 128 and (mom[e['at_rest']] == 0.0).all()
    assert set(keys[e['at_rest']] % 8) >= {0, 7}
    return pops
