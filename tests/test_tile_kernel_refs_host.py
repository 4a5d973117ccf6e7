"""CPU tests of tests/tile_kernel_refs.py: the restated deposit, gather-kick and tile key agree
with the C oracle, and the placed input reaches every edge it claims, for every (N, T) the GPU
tests of the tile kernels run (tests/test_gpu_tile_kernels.py)."""
import numpy as np
import pytest

import tile_kernel_refs as R
from oracle import oracle

U = 2.0**-53


@pytest.mark.parametrize('N', [8, 12, 16])
@pytest.mark.parametrize('order', [2, 4])
def test_refs_agree_with_the_c_oracle(N, order):
    """one PM kick of random particles through the oracle: its CIC indices, its folded deposit
    and its kick from ITS potential, against keys_ref / deposit_ref / gather_kick_ref.  The
    oracle sums in float64 in particle order, the references in long double: the bars are the
    oracle's own rounding, m additions per cell and 8 per particle."""
    g, Lbox, n = R.NGHOSTS, 50.0, 3000
    rng = np.random.default_rng(N + order)
    pos = rng.uniform(0, Lbox, (n, 3))
    pos[:3] = [[0.0, 0.0, 0.0], [np.nextafter(Lbox, 0)]*3, [0.0, Lbox/2, np.nextafter(Lbox, 0)]]
    mom0 = rng.normal(0, 1, (n, 3))
    mom = mom0.copy()
    kw = dict(mass=1.3, boxsize=Lbox, gridsize=N, G_Newton=0.7, dt_1=0.01, dt_dens=0.012,
              dt_kick=0.011)
    out = oracle.pm_long_range(pos.copy(), mom, diff_order=order, nghosts=g, want_indices=True,
                               **kw)
    # indices -> keys
    low = R.lower_cells(pos, N, Lbox)
    assert np.array_equal(low, out['cic_index_deposit'] - g)
    assert np.array_equal(low, out['cic_index_gather'] - g)
    T = 4
    cell = np.mod(out['cic_index_deposit'] - g, N)
    want = (((cell[:, 0]//T)*(N//T) + cell[:, 1]//T)*(N//T) + cell[:, 2]//T)*8 \
        + 4*(cell[:, 0] % T == T - 1) + 2*(cell[:, 1] % T == T - 1) + (cell[:, 2] % T == T - 1)
    assert np.array_equal(R.keys_ref(pos, N, Lbox, T), want)
    # deposit, folded
    contribution = oracle.deposit_contribution(kw['mass'], kw['dt_dens'], kw['dt_1'], N, Lbox)
    grid = out['grid_deposit'].copy()
    ng = N + 2*g
    oracle.lib().orc_communicate_ghosts(oracle._p(grid), ng, ng, ng, g, 1)
    dens, (m, mag) = R.deposit_ref(pos, N, Lbox, g, True, contribution)
    assert int(m.sum()) == 8*n
    err = np.abs(grid[g:-g, g:-g, g:-g] - dens)
    # (+ 8: the fold adds up to 8 partial sums)
    bar = (m + 8)*U*mag
    ratio = float(np.max(np.where(bar > 0, err/np.where(bar > 0, bar, 1), 0)))
    print(f'N {N}: deposit, worst error/bar {ratio:.3f}')
    assert (err <= bar).all()
    # kick from the oracle's own potential
    phi = out['grid_potential'][g:-g, g:-g, g:-g]
    factor = kw['mass']*(-kw['dt_kick'])
    ref, mag = R.gather_kick_ref(phi, pos, mom0, N, Lbox, order, factor)
    err = np.abs(mom - ref)
    bar = 10*U*abs(factor)*mag + np.spacing(np.abs(mom0))
    ratio = float((err/bar).max())
    print(f'N {N} order {order}: kick, worst error/bar {ratio:.3f}')
    assert (err <= bar).all()
    assert np.abs(mom - mom0).max() > 0


def test_drift_ref_is_the_oracle_s_and_leaves_its_input():
    rng = np.random.default_rng(5)
    pos, mom = rng.uniform(0, R.L, (100, 3)), rng.normal(0, 30, (100, 3))
    keep = pos.copy()
    new = R.drift_ref(pos, mom, R.DTM, R.L)
    assert np.array_equal(pos, keep)
    assert np.array_equal(new, oracle.drift(pos.copy(), mom, R.DTM, R.L))
    assert (new >= 0).all() and (new < R.L).all() and not np.array_equal(new, pos)


@pytest.fixture(scope='module', params=R.SIZES, ids=lambda s: f'N{s[0]}-T{s[1]}')
def placed(request):
    return R.placed_particles(*request.param)


def test_sizes_are_two_and_three_tiles_of_every_extent():
    assert sorted({T for _, T in R.SIZES}) == [2, 4, 8, 16]
    for T in (2, 4, 8, 16):
        assert sorted(N//T for N, t in R.SIZES if t == T) == [2, 3]
    for N, T in R.SIZES:
        # the rule of cg_create: the largest of 16, 8, 4, 2 with at least two tiles per dimension
        t = 16
        while t > 2 and (N % t or N//t < 2):
            t //= 2
        assert t == T and (R.L/N).is_integer()


def test_placed_particles_reach_every_edge(placed):
    N = placed['N']
    pops = R.check_placed(placed, verbose=True)
    n = placed['pos'].shape[0]
    assert n == pops.sum() and n <= 32000
    # at T = 16 bucket 0 is the rule ((15/16)^3), at T = 2 the exception (1/8): the fill decides
    fill = pops[len(R.NAMED):-1] if pops.shape[0] - 1 > len(R.NAMED) else pops[-1:]
    share = fill[:, 0].sum()/fill.sum()
    if placed['T'] == 16:
        assert share > 0.7
    elif placed['T'] == 2:
        assert share < 0.2
    else:                       # T = 4, 8: between the two, both paths of fetch() are common
        assert 0.2 < share < 0.7
    assert placed['pos'].shape == placed['mom'].shape == (n, 3) and placed['N'] == N


@pytest.mark.parametrize('order', [2, 4])
def test_predicted_regions_hold_two_fused_steps(placed, order):
    """two fused steps with the references (potentials and factor of the GPU test): the regions
    cg_predict_regions makes of each step's input populations (population + a quarter + 32) hold
    its output populations, the aimed moves land after the kick too, and the row aimed at 0
    arrives there"""
    N, T, e = placed['N'], placed['T'], placed['edges']
    pos = placed['pos']
    nb = 8*(N//T)**3
    factor = R.factor_of(N)
    phi = R.potential(N, 10*N + 1)
    mom = R.aim_at_zero(placed, phi, order)
    keys = R.keys_ref(pos, N, R.L, T)
    for step in range(2):
        count = np.bincount(keys, minlength=nb)
        kicked, mag = R.gather_kick_ref(phi, pos, mom, N, R.L, order, factor)
        kicked = kicked.astype(np.float64)
        assert (np.abs(kicked - mom)*R.DTM < R.L/N/16).all(), 'a kick beyond 1/16 cell'
        new = R.drift_ref(pos, kicked, R.DTM, R.L)
        nkeys = R.keys_ref(new, N, R.L, T)
        if step == 0:
            for r, d in e['to_zero']:
                assert new[r, d] == 0.0 and kicked[r, d] < 0
            for d in range(3):
                assert nkeys[e['move_tile'][d]]//8 != keys[e['move_tile'][d]]//8
                assert new[e['wrap_up'][d], d] < pos[e['wrap_up'][d], d]
                assert new[e['wrap_down'][d], d] > pos[e['wrap_down'][d], d]
            assert ((nkeys//8 == keys//8) & (nkeys != keys)).sum() >= 3
            assert (nkeys//8 != keys//8).sum() >= 3
        room = R.region_capacities(count)
        after = np.bincount(nkeys, minlength=nb)
        assert (after <= room).all(), (step, int((after - room).max()))
        assert room.sum() <= pos.shape[0] + pos.shape[0]//4 + 32*nb   # cg_region_capacity
        pos, mom, keys = new, kicked, nkeys
        phi = R.potential(N, 10*N + 2)
