"""k_ewald_tabulate and k_pp_kick (csrc/cg_pp.hip) one by one, through mesh.ewald_tabulate and
mesh.pp_kick, against the plain references of tests/pp_refs.py on the input sets that
test_pp_refs_host.py has already checked on the CPU.

Table: sizes 2, 3, 4, 5 and 64 against the 40-digit values of golden pp_ewald_mp, per point and
component |got - mp| <= K 2^-53 S, S the sum of the absolute values of the Ewald sum's terms.
K = max(4 k_oracle, 32) = 32: k_oracle = 6.457 (stored in the fixture) is what the CPU oracle
with the host's erfc/exp/sin reaches against the same mp values, the factor 4 the room for the
device library's.  Entry (0, 0, 0) is exactly zero.

Kick: per receiver and component |got - ref| <= (n_s + 64) 2^-53 A (pp_refs.kick_bound), ref
and A from pp_kick_ref in np.longdouble.  Every table is made on the host and uploaded; Δmom
starts from non-zero sentinels; every call is made twice on the same inputs and has to return
the same bits (no atomics in the kernel); rows of inactive receivers keep their sentinel bit
for bit.  The groups: chunk and block edges, the three softening kernels with pairs planted on
the spline's branch points, the look-up's edges in a box of 2, rungs.

Python layer: gravity('pp' | 'ppnonperiodic') against the goldens pp_none_n4, pp_plummer_n4,
ppnonperiodic_plummer_n4 and pp_rungs_n4 (the reference's own Δmom), and two components of
different mass and softening length, both on rungs, against pp_kick_ref composed as
component_component_pp composes the kicks."""
import numpy as np
import pytest

import pp_refs as R

pytestmark = pytest.mark.gpu

CASES = R.kick_cases()
PAIR_KEY = 'a**(-3*w_eff₀-3*w_eff₁-1)'


@pytest.fixture(scope='module')
def meshes():
    from concept_amd.mesh import PotentialMesh
    made = {}

    def get(boxsize):
        if boxsize not in made:
            made[boxsize] = PotentialMesh(16, boxsize)
        return made[boxsize]
    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope='module')
def tables(golden):
    from oracle import pp
    return {'g4': golden('pp_none_n4')['ewald_grid'], 'g6': golden('pp_ewald_n4')['ewald_grid'],
            'g9': pp.ewald_tabulate(9), 'syn': R.synthetic_table()}


def gpu(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).cuda()     # (a copy: the sets are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [2, 3, 4, 5, 64])
def test_ewald_table_vs_mp(meshes, golden, size):
    g = golden('pp_ewald_mp')
    K = max(4*float(g['k_oracle']), 32)
    table = meshes(R.BOX).ewald_tabulate(size).cpu().numpy()
    assert table.shape == (size, size, size, 3)
    assert np.isfinite(table).all()
    assert not table[0, 0, 0].any() and not np.signbit(table[0, 0, 0]).any()
    p = g[f'points_{size}']
    got = table[p[:, 0], p[:, 1], p[:, 2]].astype(R.LD)
    err = np.abs((got - g[f'hi_{size}']) - g[f'lo_{size}'])
    S = g[f'S_{size}']
    ratio = err[S > 0]/(R.LD(R.U53)*S[S > 0])
    print(f'table {size}: worst |got - mp| / (2^-53 S) = {float(ratio.max()):.3f} (K = {K:g})')
    assert np.all(err[S == 0] == 0)
    assert ratio.max() <= K


# ---------------------------------------------------------------------------------------------
# the kick
# ---------------------------------------------------------------------------------------------
def run_case(meshes, tables, name):
    """-> (got - sentinel in long double, reference, A, active mask); the call is made twice"""
    case = CASES[name]
    dm, A = R.case_reference(case, tables)
    factor, active = R.case_factors(case)
    start = R.sentinels(A, len(name))
    assert np.all(start != 0)
    table = None if case['table'] is None else gpu(tables[case['table']])
    pos_r, pos_s = gpu(case['pos_r']), gpu(case['pos_s'])
    rungs = None
    if case['rungs'] is not None:
        factors, rung, jumped, low = case['rungs']
        rungs = (gpu(factors), gpu(rung), gpu(jumped), low)
    outs = []
    for _ in range(2):
        dmom = gpu(start)
        meshes(case['boxsize']).pp_kick(pos_r, dmom, pos_s, case['same'], table,
                                        case['softening'], case['kernel'], case['factor'], rungs)
        outs.append(dmom.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1])), 'two calls, two results'
    got = outs[0]
    assert np.isfinite(got).all()
    assert np.array_equal(bits(got[~active]), bits(start[~active])), 'an inactive row was written'
    return got.astype(R.LD) - start.astype(R.LD), dm, A, active


def check_case(meshes, tables, name):
    case = CASES[name]
    delta, dm, A, active = run_case(meshes, tables, name)
    ratio = R.worst_ratio(delta, dm, A, len(case['pos_s']))
    print(f'{name}: worst |got - ref| / bound = {ratio:.4f}')
    assert ratio <= 1
    return delta, dm, A, active


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c['group'] == 'chunk'])
def test_kick_chunk_and_block_edges(meshes, tables, name):
    delta, dm, A, _ = check_case(meshes, tables, name)
    if name == 'chunk-1-1-1':
        assert not delta.any()              # a particle alone with itself: nothing changes


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c['group'] == 'softening'])
def test_kick_softening_kernels(meshes, tables, name):
    case = CASES[name]
    counts = R.branch_pair_counts(case['pos_r'], case['boxsize'], case['table'] is not None)
    assert min(counts) >= 2*20              # at least 20 pairs in each branch of the spline
    check_case(meshes, tables, name)


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c['group'] == 'edge'])
def test_kick_ewald_lookup_edges(meshes, tables, name):
    check_case(meshes, tables, name)


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c['group'] == 'rungs'])
def test_kick_rungs(meshes, tables, name):
    case = CASES[name]
    assert case['factor'] == 0.0            # the scalar factor, as the Python layer passes it
    delta, dm, A, active = check_case(meshes, tables, name)
    low = case['rungs'][3]
    assert active.sum() == (case['rungs'][1] >= low).sum()
    assert (low == 4) == (not active.any())
    if low < 2:
        zero = active & (case['rungs'][2] == 5)         # the factor that is zero
        assert zero.any() and not delta[zero].any()


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
def golden_arguments(g):
    N = int(g['N'])
    base = float(g['G_Newton'])*float(g['mass'])**2
    if 'rung_indices' in g.files:
        factor = base*g['dt_rungs_pair'][g['rung_indices_jumped']]
        active = g['rung_indices'] >= int(g['lowest_active_rung'])
    else:
        factor, active = np.full(N, base*float(g['dt_rungs_pair'][0])), np.ones(N, dtype=bool)
    table = g['ewald_grid'] if str(g['method']) == 'pp' else None
    return (g['pos_in'], g['pos_in'], 1, float(g['boxsize']), table,
            float(g['softening_length']), str(g['softening_kernel']), factor, active)


def set_rungs(c, rung, jumped, lowest):
    import torch
    c.rung_indices.copy_(torch.as_tensor(np.ascontiguousarray(rung)))
    c.rung_indices_jumped.copy_(torch.as_tensor(np.ascontiguousarray(jumped)))
    c.lowest_active_rung = int(lowest)


@pytest.mark.parametrize('name', ['pp_none_n4', 'pp_plummer_n4', 'ppnonperiodic_plummer_n4',
                                  'pp_rungs_n4'])
def test_gravity_vs_golden(golden, name):
    from concept_amd import commons, interactions
    from concept_amd.species import Component
    g = golden(name)
    method = str(g['method'])
    commons.load_params({
        'boxsize': float(g['boxsize']), 'select_forces': {'matter': {'gravity': method}},
        'select_softening_length': {'matter': '0.03*boxsize/cbrt(N)'},
        'ewald_gridsize': int(g['ewald_gridsize']), 'N_rungs': int(g['N_rungs']),
        'softening_kernel': str(g['softening_kernel'])})
    c = Component('matter', 'matter', N=int(g['N']), mass=float(g['mass']))
    c.populate(g['pos_in'], 'pos')
    c.nullify_Δ('mom')
    assert c.use_rungs
    if 'rung_indices' in g.files:
        set_rungs(c, g['rung_indices'], g['rung_indices_jumped'], g['lowest_active_rung'])
    sdt = {(PAIR_KEY, 'matter', 'matter'): g['dt_rungs_pair']}
    interactions.gravity(method, [c], [c], sdt, 'any', False)
    out = c.host('Δmom')
    args = golden_arguments(g)
    if method == 'pp':
        # the kernel looks up the table the GPU tabulated, the reference program its own: this
        # test is about the Python layer, so the reference here takes the GPU's table
        from concept_amd.shortrange import get_ewald_grid
        args = args[:4] + (get_ewald_grid(commons.params, c.device).cpu().numpy(),) + args[5:]
    dm, A = R.pp_kick_ref(*args)
    ratio = R.worst_ratio(out, dm, A, int(g['N']))
    dm_g, A_g = R.pp_kick_ref(*golden_arguments(g))
    own = R.worst_ratio(g['dmom'], dm_g, A_g, int(g['N']))
    print(f'{name}: gravity() vs pp_kick_ref {ratio:.4f} of the bound; the golden vs '
          f'pp_kick_ref on its own table {own:.4f}')
    assert ratio <= 1 and own <= 1
    # against the golden itself: each sits inside the bound of its own sum, and the two tables
    # differ per entry by at most 2 K 2^-53 S (each within K of the mp value), which the
    # look-up's weights carry into the kick
    extra = 0
    if method == 'pp':
        mp = golden('pp_ewald_mp')
        K = max(4*float(mp['k_oracle']), 32)
        assert np.array_equal(mp['points_4'], np.argwhere(np.ones((4, 4, 4))))
        x, y, z = R.separations(g['pos_in'], g['pos_in'], float(g['boxsize']), True)
        carried = R.ewald_lookup_ref(mp['S_4'].reshape(4, 4, 4, 3), x, y, z,
                                     float(g['boxsize']))[1]
        carried[np.eye(len(x), dtype=bool)] = 0
        extra = 2*K*R.LD(R.U53)*np.abs(args[7])[:, None]*carried.sum(axis=1)
    err = np.abs(out.astype(R.LD) - g['dmom'])
    assert np.all(err[args[8]] <= (2*R.kick_bound(A_g, int(g['N'])) + extra)[args[8]])
    assert not out[~args[8]].any()          # inactive rows: the zeros they started from
    assert np.array_equal(c.host('pos'), g['pos_in'])


def test_gravity_two_components_on_rungs():
    from concept_amd import commons, interactions
    from concept_amd.shortrange import get_ewald_grid
    from concept_amd.species import Component
    rng = np.random.default_rng(12)
    L, nr = R.BOX, R.N_RUNGS
    commons.load_params({'boxsize': L, 'select_forces': {'all': {'gravity': 'pp'}},
                         'select_softening_length': {'a': '0.02*boxsize/cbrt(N)',
                                                     'b': '0.05*boxsize/cbrt(N)'},
                         'ewald_gridsize': 9, 'N_rungs': nr})
    p = commons.params
    comps, data = {}, {}
    for nm, n, mass, low in (('a', 150, 2.0, 1), ('b', 90, 5.0, 2)):
        pos = rng.uniform(0, L, (n, 3))
        rung = rng.integers(0, nr, n).astype(np.int8)
        jump = rng.integers(0, 3, n)
        jump[(rung == nr - 1) & (jump == 2)] = 0
        jumped = (rung + nr*jump).astype(np.int8)
        c = Component(nm, 'matter', N=n, mass=mass)
        c.populate(pos, 'pos')
        c.nullify_Δ('mom')
        assert c.use_rungs
        set_rungs(c, rung, jumped, low)
        comps[nm], data[nm] = c, (pos, rung, jumped, low, mass)
    assert comps['a'].softening_length != comps['b'].softening_length
    sdt = {(PAIR_KEY, x, y): 0.01*(1 + 0.1*k)*(1 + 0.07*np.arange(3*nr - 1))
           for k, (x, y) in enumerate((x, y) for x in 'ab' for y in 'ab')}
    interactions.gravity('pp', [comps['a'], comps['b']], [comps['a'], comps['b']], sdt, 'any',
                         False)
    table = get_ewald_grid(p, comps['a'].device).cpu().numpy()
    for x in 'ab':
        pos, rung, jumped, low, mass = data[x]
        ref = np.zeros((len(pos), 3), dtype=R.LD)
        bound = np.zeros_like(ref)
        for y in 'ab':
            pos_y, mass_y = data[y][0], data[y][4]
            soft = 0.5*(comps[x].softening_length + comps[y].softening_length)
            factor = (p.G_Newton*mass*mass_y*sdt[PAIR_KEY, x, y])[jumped]
            dm, A = R.pp_kick_ref(pos, pos_y, x == y, L, table, soft, 'spline', factor,
                                  rung >= low)
            ref += dm
            bound += R.kick_bound(A, len(pos_y))
        out = comps[x].host('Δmom')
        err = np.abs(out.astype(R.LD) - ref)
        active = rung >= low
        assert active.any() and not active.all() and not out[~active].any()
        ratio = float((err[active]/bound[active]).max())
        print(f'two components, receiver {x}: worst |got - ref| / bound = {ratio:.4f}')
        assert ratio <= 1
