"""Plain references of the direct-summation kernels (csrc/cg_pp.hip: k_ewald_tabulate and
k_pp_kick), and the input sets their tests run on.  No HIP, no torch, no oracle.

ewald_summation_mp   the Ewald sum of ewald.py:62-118, 245-271 in mpmath (golden script only)
pp_kick_ref          one-sided kick of every receiver by every supplier (gravity.py:121-206,
                     491-560; ewald.py:146-197; interactions.py:1847-1914) in np.longdouble,
                     with the operation's discrete decisions taken in float64
pp_kick_f64          the same code in float64 throughout: the kernel's arithmetic on a CPU,
                     with switches that plant one defect each (the mutation check of
                     test_pp_refs_host.py)

The bound of the kick tests, per receiver and component:
    |got - ref| <= (n_s + 64) 2^-53 A,   A = sum_j |factor| (inv_box2 sum_corners w |g| + |x| r3inv)
n_s for the sequential float64 sum over suppliers, 64 for the roundings inside one term."""
import functools
from math import isqrt

import numpy as np

MACHINE_EPS = float(np.finfo(np.float64).eps)   # commons.py:1814
U53 = 2.0**-53
KERNELS = ('none', 'plummer', 'spline')
LD = np.longdouble


# ---------------------------------------------------------------------------------------------
# the Ewald table
# ---------------------------------------------------------------------------------------------
def ewald_summation_mp(x, y, z, digits=40):
    """summation(x, y, z) of ewald.py with its constants, loop ranges and cuts, every sum in
    mpmath.  Returns (force[3], S[3]): S = sum of |term| with |sin| replaced by 1."""
    import mpmath as mp
    with mp.workdps(max(int(digits), 40)):
        rs, maxdist, maxh2 = mp.mpf(0.25), mp.mpf(3.6), 10
        pi = mp.mpf(float(np.pi))
        h_lower, h_upper = -isqrt(maxh2), isqrt(maxh2) + 1
        n_lower, n_upper = -int(3.6 + 1), int(3.6 + 1) + 1
        c = [mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(z))]
        f = [mp.mpf(0)]*3
        S = [mp.mpf(0)]*3
        if c[0] == 0 and c[1] == 0 and c[2] == 0:
            return f, S
        r3 = c[0]**2 + c[1]**2 + c[2]**2
        r3 *= mp.sqrt(r3)
        for d in range(3):
            f[d] += c[d]/r3
            S[d] += abs(c[d])/r3
        maxdist2 = maxdist**2
        a1, a2, a3 = 1/(2*rs), 1/(mp.sqrt(pi)*rs), -1/(4*rs**2)
        for sx in range(n_lower, n_upper):
            for sy in range(n_lower, n_upper):
                for sz in range(n_lower, n_upper):
                    dv = (c[0] - sx, c[1] - sy, c[2] - sz)
                    dist2 = (dv[0]**2 + dv[1]**2) + dv[2]**2
                    if dist2 > maxdist2:
                        continue
                    dist = mp.sqrt(dist2)
                    part = -(mp.erfc(dist*a1) + dist*a2*mp.exp(dist2*a3))/dist**3
                    for d in range(3):
                        f[d] += dv[d]*part
                        S[d] += abs(dv[d]*part)
        for sx in range(h_lower, h_upper):
            for sy in range(h_lower, h_upper):
                for sz in range(h_lower, h_upper):
                    h2 = (sx*sx + sy*sy) + sz*sz
                    if h2 > maxh2 or h2 == 0:
                        continue
                    kv = (2*pi*sx, 2*pi*sy, 2*pi*sz)
                    k2 = (kv[0]**2 + kv[1]**2) + kv[2]**2
                    amp = 4*pi/k2*mp.exp(-k2*rs**2)
                    part = -amp*mp.sin(kv[0]*c[0] + kv[1]*c[1] + kv[2]*c[2])
                    for d in range(3):
                        f[d] += kv[d]*part
                        S[d] += abs(kv[d])*amp
        return f, S


def table_coordinate(index, gridsize):
    """the float64 argument tabulate_vectorgrid hands to summation (mesh.py:212-290)"""
    return np.float64(index)*np.float64(0.5/(gridsize - 1))


# ---------------------------------------------------------------------------------------------
# the kick
# ---------------------------------------------------------------------------------------------
def lookup_scale(boxsize, gridsize, mut=()):
    """ℝ[2/boxsize*(ewald_gridsize - 1)*(1 - machine_ϵ)] (ewald.py:184), in float64"""
    scale = 2/np.float64(boxsize)*np.float64(gridsize - 1)
    if 'no_eps' not in mut:
        scale = scale*(1 - MACHINE_EPS)
    return np.float64(scale)


def ewald_lookup_ref(table, x, y, z, boxsize, real=LD, mut=()):
    """ewald(x, y, z) (ewald.py:146-197) for float64 arrays of nearest-image separations.
    Signs, g = c·scale, idx and dist = g - idx in float64; weights and the eight-corner sum in
    `real`.  Returns (f, fabs), shape x.shape + (3,); fabs = inv_box2·Σ_corners w·|g|.
    Raises where a look-up would leave the table."""
    table = np.asarray(table, dtype=np.float64)
    gs = table.shape[0]
    scale = lookup_scale(boxsize, gs, mut)
    inv_box2 = real(1)/(real(boxsize)*real(boxsize))
    tab = table.astype(real)
    idx, w, neg = [], [], []
    for c in (x, y, z):
        c = np.asarray(c, dtype=np.float64)
        n = (c < 0) if 'neg_lt' in mut else ~(c > 0)
        c = np.where(n, -c, c)
        g = c*scale
        i = g.astype(np.int64)
        dist = (g - i.astype(np.float64)).astype(real)
        idx.append(i)
        neg.append(n)
        w.append((1 - dist, dist))
    top = max(int(i.max()) for i in idx) + 1 if idx[0].size else 0
    if 'no_eps' in mut and top == gs:
        # the planted defect reads one layer past the table: undefined there, NaN here
        tab = np.pad(tab, ((0, 1),)*3 + ((0, 0),), constant_values=np.nan)
    elif top > gs - 1 or any(i.size and i.min() < 0 for i in idx):
        raise ValueError('pp reference: a look-up leaves the Ewald table '
                         f'(idx + 1 = {top}, gridsize {gs})')
    f = np.zeros(idx[0].shape + (3,), dtype=real)
    fabs = np.zeros_like(f)
    for a in range(2):
        wi = w[0][a]*inv_box2
        for b in range(2):
            wij = wi*w[1][b]
            for cc in range(2):
                weight = (wij*w[2][cc])[..., None]
                g = tab[idx[0] + a, idx[1] + b, idx[2] + cc]
                f += g*weight
                fabs += np.abs(g)*weight
    for d in range(3):
        f[..., d] = np.where(neg[d], -f[..., d], f[..., d])
    return f, fabs


def spline_branch(r2, softening, mut=()):
    """0: u < 1/2, 1: 1/2 <= u < 1, 2: r >= h — the float64 tests of get_softened_r3inv"""
    r2 = np.asarray(r2, dtype=np.float64)
    h = np.float64(2.8)*np.float64(softening)
    r = np.sqrt(r2)
    u = r/h
    inner = (u <= 0.5) if 'u_le' in mut else (u < 0.5)
    return np.where(r >= h, 2, np.where(inner, 0, 1))


def softened_r3inv(r2_64, R2, softening, kernel, real=LD, mut=()):
    """get_softened_r3inv (interactions.py:1847-1914): branches from the float64 r2_64, values
    from R2 (the same sum in `real`)"""
    eps = real(softening)
    with np.errstate(divide='ignore', invalid='ignore'):
        if kernel == 'none':
            r3_64 = r2_64*np.sqrt(r2_64)
            r3 = R2*np.sqrt(R2)
            return np.where(r3_64 == 0, real(0), 1/np.where(r3_64 == 0, real(1), r3))
        if kernel == 'plummer':
            s = R2 + eps*eps
            return 1/(s*np.sqrt(s))
        if kernel != 'spline':
            raise ValueError(f'Softening kernel "{kernel}" not understood')
        branch = spline_branch(r2_64, softening, mut)
        h = real(np.float64(2.8))*eps
        r = np.sqrt(R2)
        u = r/h
        c185 = real(17 if 'coef' in mut else 18)/real(5)
        outer = 1/np.where(branch == 2, R2*r, real(1))
        inner = 32/(h*h*h)*(real(1)/real(3) + u*u*(-real(6)/real(5) + u))
        rr = np.where(branch == 1, r, real(1))
        mid = 32/(3*(rr*rr*rr))*((u*u*u)*(2 + u*(-real(9)/real(2) + u*(c185 - u)))
                                 - real(3)/real(480))
        return np.where(branch == 2, outer, np.where(branch == 0, inner, mid))


def separations(pos_r, pos_s, boxsize, periodic):
    """x_ji = x_i - x_j and the nearest-image step (gravity.py:151-162), float64, (3, n_r, n_s)"""
    pos_r = np.asarray(pos_r, dtype=np.float64)
    pos_s = np.asarray(pos_s, dtype=np.float64)
    d = pos_r.T[:, :, None] - pos_s.T[:, None, :]
    if periodic:
        L, half = np.float64(boxsize), np.float64(0.5*boxsize)
        d = np.where(d > half, d - L, np.where(d < -half, d + L, d))
    return d


def _kick(pos_r, pos_s, same, boxsize, table, softening, kernel, factor_per_receiver,
          active_mask, real, mut=(), j_index=None):
    pos_r = np.ascontiguousarray(pos_r, dtype=np.float64).reshape(-1, 3)
    pos_s = np.ascontiguousarray(pos_s, dtype=np.float64).reshape(-1, 3)
    n_r, n_s = pos_r.shape[0], pos_s.shape[0]
    if not (np.isfinite(pos_r).all() and np.isfinite(pos_s).all()):
        raise ValueError('pp reference: positions must be finite')
    periodic = table is not None
    if periodic:
        for p in (pos_r, pos_s):
            if p.size and (p.min() < 0 or p.max() >= boxsize):
                raise ValueError('pp reference: periodic positions must lie in [0, boxsize)')
    if same and n_r > n_s:
        raise ValueError('pp reference: same = 1 needs the receivers first among the suppliers')
    factor = np.broadcast_to(np.asarray(factor_per_receiver, dtype=np.float64), (n_r,))
    active = (np.ones(n_r, dtype=bool) if active_mask is None
              else np.asarray(active_mask, dtype=bool))
    x, y, z = separations(pos_r, pos_s, boxsize, periodic)
    if periodic:
        f, fabs = ewald_lookup_ref(table, x, y, z, boxsize, real, mut)
    else:
        f = np.zeros((n_r, n_s, 3), dtype=real)
        fabs = np.zeros_like(f)
    r2_64 = x*x + y*y + z*z
    X = np.stack([x, y, z], axis=-1).astype(real)
    R2 = X[..., 0]*X[..., 0] + X[..., 1]*X[..., 1] + X[..., 2]*X[..., 2]
    r3inv = softened_r3inv(r2_64, R2, softening, kernel, real, mut)[..., None]
    term = f - X*r3inv
    tabs = fabs + np.abs(X)*r3inv
    keep = np.ones((n_r, n_s), dtype=bool)
    if same:
        j = np.arange(n_s) if j_index is None else np.asarray(j_index)
        keep &= j[None, :] != np.arange(n_r)[:, None]
    keep &= active[:, None]
    term = np.where(keep[..., None], term, real(0))
    tabs = np.where(keep[..., None], tabs, real(0))
    fac = factor.astype(real)[:, None, None]
    contrib = fac*term
    if real is np.float64:
        dmom = np.zeros((n_r, 3))
        for k in range(n_s):            # the kernel's order: one supplier after the other
            dmom += contrib[:, k]
    else:
        dmom = contrib.sum(axis=1)
    A = (np.abs(fac)*tabs).sum(axis=1)
    return dmom, A


def pp_kick_ref(pos_r, pos_s, same, boxsize, table_or_None, softening, kernel,
                factor_per_receiver, active_mask=None):
    """Δmom (n_r, 3) and A (n_r, 3), both np.longdouble; inactive receivers get zeros."""
    return _kick(pos_r, pos_s, same, boxsize, table_or_None, softening, kernel,
                 factor_per_receiver, active_mask, LD)


def staged_suppliers(pos_s, ignore_cnt=False):
    """What the kernel's k loop reads: the suppliers in chunks of 256 through a staging buffer.
    ignore_cnt: the loop runs over all 256 slots of every chunk, so a partial chunk also reads
    what the chunk before left behind (zeros before the first).  Returns (positions, j): j is
    base + k, the index the kernel compares with the receiver's."""
    pos_s = np.asarray(pos_s, dtype=np.float64).reshape(-1, 3)
    buf = np.zeros((256, 3))
    out, jj = [], []
    for base in range(0, pos_s.shape[0], 256):
        cnt = min(256, pos_s.shape[0] - base)
        buf[:cnt] = pos_s[base:base + cnt]
        m = 256 if ignore_cnt else cnt
        out.append(buf[:m].copy())
        jj.append(base + np.arange(m))
    return np.concatenate(out), np.concatenate(jj)


def pp_kick_f64(pos_r, pos_s, same, boxsize, table_or_None, softening, kernel, factors_or_factor,
                rung=None, rung_jumped=None, lowest_active=0, mut=()):
    """The kernel's arithmetic in float64 on a CPU, from the kernel's own arguments.
    mut plants defects: 'coef' (18/5 -> 17/5), 'u_le', 'no_eps', 'neg_lt', 'rung_factor',
    'rung_le', 'ignore_cnt'."""
    n_r = np.asarray(pos_r).reshape(-1, 3).shape[0]
    if rung is None:
        factor, active = np.full(n_r, float(factors_or_factor)), None
    else:
        rung = np.asarray(rung)
        active = (rung > lowest_active) if 'rung_le' in mut else (rung >= lowest_active)
        pick = rung if 'rung_factor' in mut else np.asarray(rung_jumped)
        factor = np.asarray(factors_or_factor, dtype=np.float64)[pick]
    staged, j = staged_suppliers(pos_s, 'ignore_cnt' in mut)
    if same and staged.shape[0] < n_r:
        staged, j = np.asarray(pos_s, dtype=np.float64).reshape(-1, 3), None
    return _kick(pos_r, staged, same, boxsize, table_or_None, softening, kernel, factor, active,
                 np.float64, mut, j)[0]


def kick_bound(A, n_s):
    return (n_s + 64)*LD(U53)*A


def sentinels(A, seed):
    """Non-zero starting Δmom of the size of the kick's own terms (0.25 .. 0.75 A, either sign;
    ±1 .. ±2 where A is 0), so that the final += rounds inside the bound's room."""
    rng = np.random.default_rng(seed)
    A = np.asarray(A, dtype=np.float64)
    s = rng.uniform(0.25, 0.75, A.shape)*np.where(rng.random(A.shape) < 0.5, -1.0, 1.0)
    return np.where(A > 0, s*A, 4*s)


# ---------------------------------------------------------------------------------------------
# input sets (test_gpu_pp_kernels.py runs them on the GPU, test_pp_refs_host.py checks them)
# ---------------------------------------------------------------------------------------------
BOX = 7.3                 # not a power of two
SOFT = 0.05               # spline radius h = 0.14
CHUNK_CASES = [(1, 1, 1), (1, 2, 1), (255, 255, 1), (256, 256, 1), (257, 257, 1),
               (513, 513, 1), (100, 600, 1), (300, 257, 0), (257, 1, 0), (5, 512, 0)]
DIRECTION = np.array([0.48, 0.6, 0.64])      # oblique, unit length


def chunk_case(n_r, n_s, same):
    rng = np.random.default_rng(1000*n_r + 10*n_s + same)
    pos_r = rng.uniform(0, BOX, (n_r, 3))
    pos_s = rng.uniform(0, BOX, (n_s, 3))
    if same:
        pos_s[:n_r] = pos_r
    return pos_r, pos_s


def plant(target):
    """A float64 vector along DIRECTION whose float64 length sqrt((x² + y²) + z²) is exactly
    `target` (searched over a few ulps of each component)."""
    target = np.float64(target)
    if target == 0:
        return np.zeros(3)
    base = target*DIRECTION
    steps = np.arange(-12, 13)
    ulp = np.spacing(base)
    cx = base[0] + steps*ulp[0]
    cy = base[1] + steps*ulp[1]
    cz = base[2] + steps*ulp[2]
    X, Y, Z = np.meshgrid(cx, cy, cz, indexing='ij')
    r = np.sqrt((X*X + Y*Y) + Z*Z)
    hit = np.argwhere(r == target)
    if not len(hit):
        raise ValueError(f'no float64 vector of length {target!r} near the direction')
    cost = np.abs(steps[hit]).sum(axis=1)
    i, j, k = hit[np.argmin(cost)]
    return np.array([cx[i], cy[j], cz[k]])


def planted_separations(softening=SOFT):
    h = np.float64(2.8)*np.float64(softening)
    half = h/2
    return [0.0, 1e-3*h, h/4, np.nextafter(half, 0), half, np.nextafter(half, 1), 0.75*h,
            np.nextafter(h, 0), h, np.nextafter(h, 1), 1.5*h]


@functools.lru_cache(maxsize=None)
def softening_cloud():
    """(positions, number of planted partners): an anchor at the origin, one partner per planted
    separation along DIRECTION (anchor - partner is exact, the anchor being 0), then 300
    particles in a ball of radius 2h.  All inside [0, BOX)."""
    h = 2.8*SOFT
    partners = np.array([plant(s) for s in planted_separations()])
    rng = np.random.default_rng(77)
    v = rng.normal(size=(300, 3))
    v *= (2*h*rng.random(300)**(1/3)/np.linalg.norm(v, axis=1))[:, None]
    cloud = v + np.array([0.3, 0.31, 0.29])
    pos = np.concatenate([np.zeros((1, 3)), partners, cloud])
    pos.setflags(write=False)
    return pos, len(partners)


def branch_pair_counts(pos, boxsize, periodic, softening=SOFT):
    """ordered pairs (i != j) per spline branch"""
    x, y, z = separations(pos, pos, boxsize, periodic)
    b = spline_branch(x*x + y*y + z*z, softening)
    off = ~np.eye(len(pos), dtype=bool)
    return [int(((b == k) & off).sum()) for k in range(3)]


EDGE_BOX = 2.0            # exact halves: L/2 = 1
_T = 2.0**-53


@functools.lru_cache(maxsize=None)
def ewald_edge_case():
    """64 receivers and 7 suppliers in a box of 2 whose separations x_i - x_j (exact in float64)
    hit 0, ±1, ±(1 - 2^-53), ±(1 + 2^-52) (which wraps to ∓(1 - 2^-52)), every sign octant, and
    the cell boundaries of tables of size 4, 6 and 9 (multiples of 1/3, 1/5 and 1/8)."""
    up = 1 + 2.0**-52
    pos_s = np.array([[0, 0, 0], [1, 1, 1], [_T, 1, up], [1, up, _T], [up, _T, 1],
                      [0.5, 1.5, 0.5], [1.5, 0.5, 1.5]], dtype=np.float64)
    values = [0, _T, 1, up, 0.5, 1.5, 0.125, 0.375, 0.75, 1.25, 1.875, 0.2, 0.6, 1.4,
              1/3, 2/3, 5/3, 1.0371, 0.2113, 1.7717]
    designed = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [up, up, up],
                         [_T, _T, _T], [1, _T, up], [up, 1, 0], [0, up, 1], [0.5, 1.5, 0.5],
                         [1.5, 0.5, 1.5], [0.125, 0.25, 1.875], [0.2, 0.4, 0.6],
                         [1/3, 2/3, 4/3], [1.2, 1.4, 1.8]], dtype=np.float64)
    rng = np.random.default_rng(5)
    cols = [np.concatenate([rng.permutation(values), rng.choice(values, 48 - len(values))])
            for _ in range(3)]
    pos_r = np.concatenate([designed, np.stack(cols, axis=1)])
    assert pos_r.shape == (64, 3)
    pos_r.setflags(write=False)
    pos_s.setflags(write=False)
    return pos_r, pos_s


def synthetic_table(gridsize=5, seed=9):
    """A table with no symmetry at all: on it the sign rule at a separation of exactly 0
    (`x > 0` is positive, everything else is mirrored) shows in the values."""
    return np.random.default_rng(seed).normal(size=(gridsize,)*3 + (3,))


N_RUNGS = 4


@functools.lru_cache(maxsize=None)
def rung_case():
    """300 particles on rungs 0..3, jumped indices rung, rung + 4 and rung + 8 (below 11),
    eleven distinct factors, factors[5] (rung 1 flagged upwards) zero."""
    rng = np.random.default_rng(41)
    n = 300
    pos = rng.uniform(0, BOX, (n, 3))
    rung = rng.integers(0, N_RUNGS, n).astype(np.int8)
    jump = rng.integers(0, 3, n)
    jump[(rung == 3) & (jump == 2)] = 0
    jumped = (rung + N_RUNGS*jump).astype(np.int8)
    factors = 1e-3*(1 + 0.37*np.arange(3*N_RUNGS - 1))*np.where(np.arange(11) % 2, -1, 1)
    factors[5] = 0.0
    for a in (pos, rung, jumped, factors):
        a.setflags(write=False)
    return pos, rung, jumped, factors


# ---------------------------------------------------------------------------------------------
# the kick cases, as the kernel's arguments
# ---------------------------------------------------------------------------------------------
LOWEST_ACTIVE = (0, 2, 3, 4)
FACTOR = 0.0123


def kick_cases():
    """name -> dict(group, pos_r, pos_s, same, boxsize, table (key or None), softening, kernel,
    factor, rungs (None or (factors, rung, jumped, lowest_active))).  The table keys: 'g4' and
    'g6' are the reference's own tables of the goldens pp_none_n4 and pp_ewald_n4, 'g9' the
    oracle's table of size 9, 'syn' synthetic_table()."""
    cases = {}

    def add(name, group, pos_r, pos_s, same, boxsize, table, softening, kernel, rungs=None):
        cases[name] = dict(group=group, pos_r=pos_r, pos_s=pos_s, same=same, boxsize=boxsize,
                           table=table, softening=softening, kernel=kernel,
                           factor=0.0 if rungs else FACTOR, rungs=rungs)
    for n_r, n_s, same in CHUNK_CASES:
        pos_r, pos_s = chunk_case(n_r, n_s, same)
        add(f'chunk-{n_r}-{n_s}-{same}', 'chunk', pos_r, pos_s, same, BOX, 'g6', SOFT, 'spline')
    cloud, _ = softening_cloud()
    for kernel in KERNELS:
        add(f'soft-{kernel}-periodic', 'softening', cloud, cloud, 1, BOX, 'g9', SOFT, kernel)
        add(f'soft-{kernel}-nonperiodic', 'softening', cloud, cloud, 1, BOX, None, SOFT, kernel)
    pos_r, pos_s = ewald_edge_case()
    for table in ('g4', 'g6', 'g9', 'syn'):
        add(f'edge-{table}', 'edge', pos_r, pos_s, 0, EDGE_BOX, table, 0.01, 'spline')
    pos, rung, jumped, factors = rung_case()
    for low in LOWEST_ACTIVE:
        add(f'rungs-low{low}', 'rungs', pos, pos, 1, BOX, 'g6', SOFT, 'spline',
            (factors, rung, jumped, low))
    return cases


def case_factors(case):
    """(factor_per_receiver, active_mask) as the reference defines them"""
    n_r = len(case['pos_r'])
    if case['rungs'] is None:
        return np.full(n_r, case['factor']), np.ones(n_r, dtype=bool)
    factors, rung, jumped, low = case['rungs']
    return factors[jumped], rung >= low


def case_reference(case, tables):
    factor, active = case_factors(case)
    table = None if case['table'] is None else tables[case['table']]
    return pp_kick_ref(case['pos_r'], case['pos_s'], case['same'], case['boxsize'], table,
                       case['softening'], case['kernel'], factor, active)


def case_f64(case, tables, mut=()):
    table = None if case['table'] is None else tables[case['table']]
    if case['rungs'] is None:
        return pp_kick_f64(case['pos_r'], case['pos_s'], case['same'], case['boxsize'], table,
                           case['softening'], case['kernel'], case['factor'], mut=mut)
    factors, rung, jumped, low = case['rungs']
    return pp_kick_f64(case['pos_r'], case['pos_s'], case['same'], case['boxsize'], table,
                       case['softening'], case['kernel'], factors, rung, jumped, low, mut=mut)


def worst_ratio(got, ref, A, n_s):
    """max |got - ref| / bound over the entries with A > 0; entries with A == 0 must be exact
    (returns inf otherwise, and for anything not finite)"""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    bound = kick_bound(A, n_s)
    if not np.isfinite(np.asarray(got, dtype=np.float64)).all() or np.any(err[A == 0] != 0):
        return np.inf
    if not np.any(A > 0):
        return 0.0
    return float((err[A > 0]/bound[A > 0]).max())
