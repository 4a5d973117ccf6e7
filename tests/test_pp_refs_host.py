"""CPU checks of tests/pp_refs.py, the references and input sets of test_gpu_pp_kernels.py:

  * pp_kick_ref against the reference's own Δmom of every pp golden, its look-up against the
    reference's 40 sampled ewald() values;
  * oracle.pp.pp_kick (float64, the kernel's operation order) against pp_kick_ref for the three
    softening kernels: it has to sit at least fourfold inside the GPU test's bound
    (n_s + 64) 2^-53 A.  Worst ratio found, err / bound: WORST_ORACLE_RATIO below (measured
    0.108, a room of 9); k_oracle of the table fixture is 6.457, so K = 32;
  * every input set of the GPU test: positions in [0, L), nothing raised, the required pairs
    present;
  * the mutation check: pp_kick_f64, the kernel's arithmetic in float64, meets the bound on
    every case, and with one defect planted misses it on the cases named in MUTATIONS."""
import numpy as np
import pytest

import pp_refs as R

GOLDENS = ['pp_ewald_n4', 'ppnonperiodic_n4', 'pp_none_n4', 'pp_plummer_n4',
           'ppnonperiodic_plummer_n4', 'pp_rungs_n4']
WORST_ORACLE_RATIO = 0.25


@pytest.fixture(scope='module')
def tables(golden):
    from oracle import pp
    return {'g4': golden('pp_none_n4')['ewald_grid'], 'g6': golden('pp_ewald_n4')['ewald_grid'],
            'g9': pp.ewald_tabulate(9), 'syn': R.synthetic_table()}


@pytest.fixture(scope='module')
def cases():
    return R.kick_cases()


@pytest.fixture(scope='module')
def references(cases, tables):
    return {name: R.case_reference(case, tables) for name, case in cases.items()}


def golden_arguments(g):
    """the arguments of pp_kick_ref that restate one golden's gravity() call"""
    N = int(g['N'])
    base = float(g['G_Newton'])*float(g['mass'])**2
    if 'rung_indices' in g.files:
        factor = base*g['dt_rungs_pair'][g['rung_indices_jumped']]
        active = g['rung_indices'] >= int(g['lowest_active_rung'])
    else:
        factor, active = np.full(N, base*float(g['dt_rungs_pair'][0])), None
    kernel = str(g['softening_kernel']) if 'softening_kernel' in g.files else 'spline'
    table = g['ewald_grid'] if str(g['method']) == 'pp' else None
    return (g['pos_in'], g['pos_in'], 1, float(g['boxsize']), table,
            float(g['softening_length']), kernel, factor, active)


@pytest.mark.parametrize('name', GOLDENS)
def test_reference_reproduces_golden(golden, name):
    g = golden(name)
    dm, A = R.pp_kick_ref(*golden_arguments(g))
    ratio = R.worst_ratio(g['dmom'], dm, A, int(g['N']))
    print(f'{name}: reference program vs pp_kick_ref, err/bound = {ratio:.4f}')
    assert ratio <= 1
    if 'rung_indices' in g.files:
        inactive = g['rung_indices'] < int(g['lowest_active_rung'])
        assert inactive.any() and not g['dmom'][inactive].any()
        assert (g['rung_indices_jumped'] != g['rung_indices']).any()


def test_lookup_reproduces_sampled_ewald_values(golden):
    g = golden('pp_ewald_n4')
    pts = g['ewald_points']
    f, fabs = R.ewald_lookup_ref(g['ewald_grid'], pts[:, 0], pts[:, 1], pts[:, 2],
                                 float(g['boxsize']))
    err = np.abs(g['ewald_values'].astype(R.LD) - f)
    assert (pts[0, 0] == 0) and (pts[1, 1:] == 0).all()     # the sign rule at exactly 0
    assert np.all(err <= 64*R.LD(R.U53)*fabs)


def test_oracle_sits_fourfold_inside_the_bound(golden, cases, tables, references):
    from oracle import pp
    worst = {}
    for name in GOLDENS[:5]:
        g = golden(name)
        args = golden_arguments(g)
        dm, A = R.pp_kick_ref(*args)
        got = pp.pp_kick(args[0], boxsize=args[3], softening=args[5], factor=args[7][0],
                         periodic=args[4] is not None, ewald_grid=args[4], kernel=args[6])
        worst[name] = R.worst_ratio(got, dm, A, int(g['N']))
    for name, case in cases.items():
        if case['group'] != 'softening' and not (case['group'] == 'chunk' and case['same']
                                                 and len(case['pos_r']) == len(case['pos_s'])):
            continue
        table = None if case['table'] is None else tables[case['table']]
        got = pp.pp_kick(case['pos_r'], boxsize=case['boxsize'], softening=case['softening'],
                         factor=case['factor'], periodic=table is not None, ewald_grid=table,
                         kernel=case['kernel'])
        dm, A = references[name]
        worst[name] = R.worst_ratio(got, dm, A, len(case['pos_s']))
    for name, ratio in worst.items():
        print(f'oracle vs pp_kick_ref, {name}: err/bound = {ratio:.4f}')
    print(f'worst: {max(worst.values()):.4f}')
    assert {c['kernel'] for n, c in cases.items() if n in worst} == set(R.KERNELS)
    assert max(worst.values()) <= WORST_ORACLE_RATIO


def test_table_fixture(golden):
    g = golden('pp_ewald_mp')
    k_oracle = float(g['k_oracle'])
    print(f'k_oracle = {k_oracle:.3f}, K = {max(4*k_oracle, 32):.3f}')
    assert 0 < k_oracle < 8          # so that K = max(4 k_oracle, 32) is 32
    for size in (2, 3, 4, 5):
        assert len(g[f'points_{size}']) == size**3
    pts = {tuple(p) for p in g['points_64']}
    assert len(pts) <= 24
    assert {(0, 0, 1), (1, 0, 0), (1, 1, 1), (63, 63, 63), (63, 0, 0), (0, 63, 31),
            (32, 32, 32)} <= pts
    # the stored mp values against the reference program's own table of size 4
    ref = golden('pp_none_n4')['ewald_grid'].reshape(-1, 3)
    assert np.array_equal(g['points_4'], np.argwhere(np.ones((4, 4, 4))))
    err = np.abs((ref.astype(R.LD) - g['hi_4']) - g['lo_4'])
    assert np.all(err <= 32*R.LD(R.U53)*g['S_4'])
    assert not g['S_4'][0].any() and g['S_4'][1:].all()


def test_input_sets(cases, tables, references):
    assert [tuple(int(v) for v in n.split('-')[1:]) for n in cases if n.startswith('chunk')] \
        == R.CHUNK_CASES
    for name, case in cases.items():
        L = case['boxsize']
        for pos in (case['pos_r'], case['pos_s']):
            assert np.isfinite(pos).all()
            if case['table'] is not None:
                assert pos.min() >= 0 and pos.max() < L, name
        assert len(case['pos_r']) <= 600 and len(case['pos_s']) <= 600
        if case['same']:
            assert np.array_equal(case['pos_s'][:len(case['pos_r'])], case['pos_r'])
        dm, A = references[name]                    # (nothing raised)
        assert np.isfinite(dm.astype(np.float64)).all() and np.isfinite(A.astype(np.float64)).all()
    assert BOX_NOT_POW2()
    # softening: >= 20 ordered pairs in every spline branch, the planted separations exact
    pos, n_planted = R.softening_cloud()
    assert len(pos) == 1 + n_planted + 300
    for periodic in (True, False):
        counts = R.branch_pair_counts(pos, R.BOX, periodic)
        print('pairs per spline branch:', counts)
        assert min(counts) >= 2*20
    h = np.float64(2.8)*np.float64(R.SOFT)
    x, y, z = R.separations(pos[1:1 + n_planted], pos[:1], R.BOX, True)[:, :, 0]
    r = np.sqrt(x*x + y*y + z*z)
    assert np.array_equal(r, np.array(R.planted_separations()))
    assert np.array_equal(R.spline_branch(x*x + y*y + z*z, R.SOFT),
                          [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2])
    assert r[4] == h/2 and r[8] == h and r[0] == 0
    assert np.linalg.norm(pos[1 + n_planted:] - [0.3, 0.31, 0.29], axis=1).max() <= 2*h
    # a coincident pair under 'none': the pair's own term is zero and finite
    dm, A = R.pp_kick_ref(pos[:2], pos[:2], 1, R.BOX, tables['g9'], R.SOFT, 'none', 1.0)
    assert np.array_equal(pos[0], pos[1]) and not dm.any() and not A.any()
    # Ewald edges: the separations asked for are there
    pos_r, pos_s = R.ewald_edge_case()
    raw = pos_r.T[:, :, None] - pos_s.T[:, None, :]
    d = R.separations(pos_r, pos_s, R.EDGE_BOX, True)
    assert np.abs(d).max() == 1.0
    up, inside = 1 + 2.0**-52, 1 - 2.0**-53
    for v in (0.0, 1.0, -1.0, inside, -inside):
        assert (d == v).sum() >= 3, v
    for v in (up, -up):                              # wraps to the other side
        assert (raw == v).sum() >= 3 and ((raw == v) & (d == -np.sign(v)*(1 - 2.0**-52))).sum() >= 3
    octants = {tuple(s) for s in np.sign(d.reshape(3, -1).T) if np.all(s != 0)}
    assert len(octants) == 8
    assert (np.all(d == 1.0, axis=0)).any() and (np.all(d == -1.0, axis=0)).any()
    assert (np.all(d == 0.0, axis=0)).any()
    for size in (4, 6, 9):                           # cell boundaries: |d| (size - 1) whole
        g = np.abs(d)*(size - 1)
        on = (np.abs(g - np.rint(g)) <= 4*np.spacing(g)) & (g >= 1) & (g <= size - 2)
        assert on.sum() >= 20, size
    # rungs
    pos, rung, jumped, factors = R.rung_case()
    assert len(pos) == 300 and len(factors) == 11 and len(set(factors)) == 11
    assert (factors == 0).sum() == 1 and jumped.max() < 11
    assert set(rung) == {0, 1, 2, 3}
    for k in range(3):
        assert (jumped == rung + 4*k).sum() >= 50
    assert ((jumped == 5) & (rung == 1)).any()        # the zero factor is in use


def BOX_NOT_POW2():
    m, _ = np.frexp(R.BOX)
    return m != 0.5


def test_reference_refuses_what_the_kernel_must_not_get(tables):
    one = np.array([[0.5, 0.5, 0.5]])
    for bad in (np.array([[R.BOX, 1.0, 1.0]]), np.array([[-1e-9, 1.0, 1.0]])):
        with pytest.raises(ValueError):
            R.pp_kick_ref(one, bad, 0, R.BOX, tables['g6'], R.SOFT, 'spline', 1.0)
    with pytest.raises(ValueError):
        R.pp_kick_ref(np.array([[np.nan, 0, 0]]), one, 0, R.BOX, None, R.SOFT, 'spline', 1.0)
    # a separation beyond L/2: idx + 1 would be the table's size
    with pytest.raises(ValueError):
        R.ewald_lookup_ref(tables['g9'], np.array([1 + 2.0**-52]), np.array([0.5]),
                           np.array([0.5]), R.EDGE_BOX)


# defect -> the cases whose comparison it has to fail (every one named does)
MUTATIONS = {
    'coef': ['soft-spline-periodic', 'soft-spline-nonperiodic'],
    'no_eps': ['edge-g4', 'edge-g6', 'edge-g9', 'edge-syn'],
    'neg_lt': ['edge-syn'],
    'rung_factor': ['rungs-low0', 'rungs-low2', 'rungs-low3'],
    'rung_le': ['rungs-low0', 'rungs-low2', 'rungs-low3'],
    'ignore_cnt': ['chunk-1-2-1', 'chunk-255-255-1', 'chunk-257-257-1', 'chunk-513-513-1',
                   'chunk-100-600-1', 'chunk-300-257-0', 'chunk-257-1-0'],
}


def test_float64_twin_meets_the_bound(cases, tables, references):
    worst = 0.0
    for name, case in cases.items():
        dm, A = references[name]
        ratio = R.worst_ratio(R.case_f64(case, tables), dm, A, len(case['pos_s']))
        worst = max(worst, ratio)
        assert ratio <= 0.25, (name, ratio)
    print(f'float64 twin vs pp_kick_ref, worst err/bound = {worst:.4f}')


@pytest.mark.parametrize('mut', sorted(MUTATIONS))
def test_planted_defect_fails_the_comparison(cases, tables, references, mut):
    for name in MUTATIONS[mut]:
        case = cases[name]
        dm, A = references[name]
        got = R.case_f64(case, tables, mut=(mut,))
        ratio = R.worst_ratio(got, dm, A, len(case['pos_s']))
        print(f'{mut} on {name}: err/bound = {ratio:.3g}')
        assert ratio > 1, (mut, name, ratio)


def test_swapped_half_test_changes_the_branch():
    """`u <= 0.5` for `u < 0.5`: the spline is continuous at u = 1/2, so the value moves by
    rounding only; what the planted pair at exactly h/2 pins down is the branch taken."""
    pos, n = R.softening_cloud()
    x, y, z = R.separations(pos[1:1 + n], pos[:1], R.BOX, True)[:, :, 0]
    r2 = x*x + y*y + z*z
    assert np.array_equal(R.spline_branch(r2, R.SOFT), [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2])
    assert np.array_equal(R.spline_branch(r2, R.SOFT, mut=('u_le',)),
                          [0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2])
