"""GPU tests of analysis.measure() and its kernels (csrc/cg_measure.hip) against the restatement of
tests/measure_refs.py.

The sums: |Σ_gpu − Σ_exact| <= n 2⁻¹⁰⁰ Σ|x| + ulp(Σ_exact)/2 (measure_refs.sum_bound), Σ_gpu being
hi + lo rounded to double and Σ_exact the exact sum of the same doubles; the same for Σx² with
exact squares.  Extremes and the six maxima of 'discontinuity' are compared bit for bit.  σ, ϱ_bar
and v_rms: within 4 ulp of the restatement evaluated in decimal.

The sizes come from the launch code: workgroups of 256 threads, one per 256 rows up to 1024
(k_measure_sums), whose partials a last workgroup of 256 threads folds (k_measure_sums_final)."""
import fractions
import math

import numpy as np
import pytest

import measure_refs as refs
from test_measure_host import golden

pytestmark = pytest.mark.gpu

THREADS, BLOCKS = 256, 1024
SIZES = [0, 1, 63, 64, 65, 255, 256, 257,
         THREADS*THREADS + 1,                  # 257 partials: more than the last workgroup's threads
         THREADS*BLOCKS - 1, THREADS*BLOCKS, THREADS*BLOCKS + 1]   # the largest grid, a row each
ULPS = 4


@pytest.fixture(scope='module')
def ctx():
    from concept_amd.mesh import PotentialMesh
    m = PotentialMesh(32, 32.0)
    yield m._ctx
    m.close()


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_sums(ctx, x, n, stride=1, offset=0, ncols=1, start=None, count=None, nregions=0):
    """cg_measure_sums -> float64[ncols, 6]"""
    import torch
    from concept_amd.lib import _ptr, check, raw
    out = torch.full((6*ncols,), -7.0, dtype=torch.float64, device='cuda')
    check(raw().cg_measure_sums(ctx, _ptr(x), n, stride, offset, ncols, _ptr(start), _ptr(count),
                                nregions, _ptr(out)))
    return out.cpu().numpy().reshape(ncols, 6)


def values_of(n, seed):
    """normal, scaled by exp(3 normal), both signs: the sum is far below Σ|x|"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=n)*np.exp(3*rng.normal(size=n))


def check_sums(got, values, what):
    """the six numbers of one column against the exact sums of `values`"""
    n = values.size
    for name, square, hi, lo in (('Σx', False, got[0], got[1]), ('Σx²', True, got[2], got[3])):
        exact = refs.exact_sum(values, square)
        abs_sum = exact if square else refs.exact_sum(np.abs(values))
        bound = refs.sum_bound(n, abs_sum, exact)
        rounded = float(fractions.Fraction(hi) + fractions.Fraction(lo))
        miss = abs(fractions.Fraction(rounded) - exact)
        print(f'{what}: {name} = {rounded!r} (hi {hi!r}, lo {lo!r}), exact {float(exact)!r}, '
              f'off by {float(miss):.3e}, bound {float(bound):.3e}')
        assert miss <= bound, (what, name)
        assert abs(lo) <= refs.ulp(hi)/2, (what, name)
    assert got[4] == (values.min() if n else math.inf), what
    assert got[5] == (np.abs(values).max() if n else 0.0), what


# -- accuracy --------------------------------------------------------------------------------------
def test_sums_where_a_double_sum_fails(ctx):
    n = 2**16
    values = refs.cancelling_values(n, seed=1)
    exact, abs_sum = refs.exact_sum(values), refs.exact_sum(np.abs(values))
    bound = refs.sum_bound(n, abs_sum, exact)
    assert bound < abs_sum/2**80
    miss = abs(refs.exact_sum([np.sum(values)]) - exact)
    print(f'np.sum misses the exact sum by {float(miss):.3e}, the bound is {float(bound):.3e}')
    assert miss > bound
    x = gpu(values)
    got = device_sums(ctx, x, n)
    check_sums(got[0], values, 'cancelling pairs of 1e16')
    assert np.array_equal(got, device_sums(ctx, x, n)), 'a second call returned other bits'


def test_sums_of_squares_that_no_double_holds(ctx):
    n = 2**16
    values = refs.unrepresentable_squares(n, seed=refs.SQUARES_SEED)
    exact = refs.exact_sum(values, square=True)
    assert abs(refs.exact_sum([np.sum(values**2)]) - exact) > refs.sum_bound(n, exact, exact)
    x = gpu(values)
    got = device_sums(ctx, x, n)
    check_sums(got[0], values, 'unrepresentable squares')
    assert np.array_equal(got, device_sums(ctx, x, n)), 'a second call returned other bits'


# -- shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_sizes(ctx, n):
    values = values_of(n, seed=100 + n % 97)
    got = device_sums(ctx, gpu(values) if n else None, n)
    check_sums(got[0], values, f'n = {n}')


def test_stride_3_with_each_offset_and_the_three_columns_at_once(ctx):
    n = 1000
    rows = values_of(3*n, seed=7).reshape(n, 3)
    x = gpu(rows)
    single = []
    for offset in range(3):
        got = device_sums(ctx, x, n, stride=3, offset=offset)
        check_sums(got[0], rows[:, offset], f'stride 3, offset {offset}')
        single.append(got[0])
    fused = device_sums(ctx, x, n, stride=3, offset=0, ncols=3)
    assert np.array_equal(fused, np.array(single)), 'the fused pass adds in another order'
    pair = device_sums(ctx, x, n, stride=3, offset=1, ncols=2)
    assert np.array_equal(pair, np.array(single[1:]))


@pytest.mark.parametrize('nregions', [40, 1500])
def test_region_table_with_gaps(ctx, nregions):
    """empty regions, a region of one row, regions longer than a workgroup, NaN in every gap"""
    rng = np.random.default_rng(nregions)
    counts = rng.integers(0, 6, nregions)
    counts[::7] = 0
    counts[3], counts[5], counts[nregions - 1] = 1, 700, 1
    gaps = rng.integers(0, 4, nregions)
    gaps[0] = 2
    starts = np.cumsum(gaps + np.concatenate([[0], counts[:-1]]))
    total = int(starts[-1] + counts[-1] + 3)
    rows = np.full((total, 3), np.nan)
    live = np.zeros(total, dtype=bool)
    for s_, c_ in zip(starts, counts):
        live[s_:s_ + c_] = True
    rows[live] = values_of(3*int(live.sum()), seed=9).reshape(-1, 3)
    x = gpu(rows)
    start, count = gpu(starts.astype(np.int32)), gpu(counts.astype(np.int32))
    got = device_sums(ctx, x, 0, stride=3, offset=0, ncols=3, start=start, count=count,
                      nregions=nregions)
    for dim in range(3):
        check_sums(got[dim], rows[live, dim], f'{nregions} regions, column {dim}')
    # without populations: region r ends where region r + 1 begins, no gaps
    dense = rows[live]
    bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    got = device_sums(ctx, gpu(dense), 0, stride=3, offset=2, start=gpu(bounds),
                      nregions=nregions)
    check_sums(got[0], dense[:, 2], f'{nregions} dense regions')


@pytest.mark.parametrize('bad', [math.nan, math.inf])
def test_nan_and_infinity_reach_the_output(ctx, bad):
    n = 1000   # 4 workgroups of 250 rows: row 950 belongs to the last wave of the last one
    for where in (0, n - 1, 950):
        values = values_of(n, seed=11)
        values[where] = bad
        got = device_sums(ctx, gpu(values), n)[0]
        print(f'{bad} at {where}: {got}')
        if math.isnan(bad):
            assert math.isnan(got[0]) and math.isnan(got[2])
            assert math.isnan(got[4]) and math.isnan(got[5])
        else:
            assert not math.isfinite(got[0]) and not math.isfinite(got[2])
            assert got[5] == math.inf
            assert got[4] == np.delete(values, where).min()


# -- analysis.measure ------------------------------------------------------------------------------
def within_ulps(got, want, what):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    off = np.abs(got - want)/np.array([math.ulp(w) for w in want.tolist()])
    print(f'{what}: {got} against {want}: {off.max()} ulp')
    assert off.max() <= ULPS, what


def check_total(got, values, scale, what):
    """a sum of scale*values out of analysis.measure within the bound"""
    n = values.size
    exact = refs.exact_sum(values)*fractions.Fraction(scale)
    bound = refs.sum_bound(n, refs.exact_sum(np.abs(values))*fractions.Fraction(scale), exact)
    miss = abs(fractions.Fraction(float(got)) - exact)
    print(f'{what}: {float(got)!r}, exact {float(exact)!r}, off by {float(miss):.3e}, bound '
          f'{float(bound):.3e}')
    assert miss <= bound, what


def make_particles(mom, mass=2.5):
    from concept_amd import commons
    from concept_amd.species import Component
    commons.load_params(str(golden()['param']))
    N = mom.shape[0]
    c = Component('particles', 'matter', N=N, mass=mass)
    pos = np.random.default_rng(5).random((N, 3))*commons.params.boxsize
    for d, s_ in enumerate('xyz'):
        c.populate(np.ascontiguousarray(pos[:, d]), 'pos' + s_)
        c.populate(np.ascontiguousarray(mom[:, d]), 'mom' + s_)
    return c


def test_particle_momentum_and_mass():
    from concept_amd import analysis, stepper
    from concept_amd.lib import ConceptGPUError
    N, a = 1000, 0.5
    mom = values_of(3*N, seed=21).reshape(N, 3)
    c = make_particles(mom)
    Σmom, σmom = analysis.measure(c, 'momentum', a)
    want_Σ, want_σ = refs.momentum_particles(mom)
    for dim in range(3):
        check_total(Σmom[dim], mom[:, dim], 1.0, f'Σmom[{dim}]')
    within_ulps(σmom, want_σ, 'σmom')
    print(f'Σmom equal to the restatement in decimal: {np.array_equal(Σmom, want_Σ)}')
    assert analysis.measure(c, 'mass', a) == refs.mass_particles(a, 0.0, N, c.mass)
    for quantity in ('v_rms', 'v_max'):
        assert analysis.measure(c, quantity, a) == stepper.measure(c, quantity, a)
    with pytest.raises(ConceptGPUError, match='not implemented'):
        stepper.measure(c, 'momentum', a)   # the time loop's own measure() stays as it is
    with pytest.raises(ConceptGPUError, match='particle components do not have ϱ'):
        analysis.measure(c, 'ϱ', a)


def test_particle_momentum_of_the_golden_component():
    from concept_amd import analysis
    g = golden()
    c = make_particles(g['mom'], float(g['mass']))
    Σmom, σmom = analysis.measure(c, 'momentum', float(g['a']))
    for dim in range(3):
        check_total(Σmom[dim], g['mom'][:, dim], 1.0, f'golden Σmom[{dim}]')
    within_ulps(σmom, g['particles_momentum_sigma'], 'golden σmom')
    assert analysis.measure(c, 'mass', float(g['a'])) == float(g['particles_mass'])


def test_identical_rows_have_no_spread():
    """every row the same: σmom = 0 exactly.  The value is picked so that the variance, finished
    in decimal from exact sums, comes out negative: the branch that turns it into 0 is taken"""
    from concept_amd import analysis
    N = 997
    for k in range(1, 40):
        x = float(np.float32(1234.5678*k/7))   # 24 bits: every partial sum fits a double-double
        if refs.variance_from_partials([refs.partial_of(np.full(N, x))], N) < 0:
            break
    else:
        raise AssertionError('no value with a negative variance among the candidates')
    c = make_particles(np.full((N, 3), x))
    local = analysis._particle_momentum_sums(c, None)
    variance = refs.variance_from_partials([local[:6]], N)
    print(f'x = {x!r}: the variance from the device sums is {variance}')
    assert variance < 0 and local[:6] == refs.partial_of(np.full(N, x))
    Σmom, σmom = analysis.measure(c, 'momentum', 1.0)
    assert np.array_equal(σmom, np.zeros(3))
    assert np.array_equal(Σmom, np.full(3, N*x))


def make_fluid(g, seed, w):
    from concept_amd import commons
    from test_gpu_fluid_drift import make_fluid as make
    commons.load_params(str(golden()['param']))
    rng = np.random.default_rng(seed)
    ρ_mbar, c = commons.params.ρ_mbar, commons.params.light_speed
    ϱ = ρ_mbar*np.exp(0.5*rng.normal(size=(g, g, g)))
    J = [ϱ*rng.normal(size=(g, g, g))*0.3 for _ in range(3)]
    𝒫 = ϱ*(c**2*w)
    return make(ϱ, J, 𝒫), ϱ, np.array(J), 𝒫


def check_fluid(c, ϱ, J, 𝒫, a, w, tag):
    from concept_amd import analysis, commons, fluid
    L, light_speed = commons.params.boxsize, commons.params.light_speed
    Vcell = L**3/ϱ.size
    Σmom, σmom = analysis.measure(c, 'momentum', a)
    for dim in range(3):
        check_total(Σmom[dim], J[dim], Vcell, f'{tag} Σmom[{dim}]')
    within_ulps(σmom, refs.momentum_fluid(J, L)[1], f'{tag} σmom')
    ϱ_bar, σϱ, ϱ_min = analysis.measure(c, 'ϱ', a)
    want = refs.rho(ϱ, exact=True)
    within_ulps(ϱ_bar, want[0], f'{tag} ϱ_bar')
    within_ulps(σϱ, want[1], f'{tag} σϱ')
    assert ϱ_min == want[2]
    mass = analysis.measure(c, 'mass', a)
    within_ulps(mass, refs.mass_fluid(ϱ, a, w, L, exact=True), f'{tag} mass')
    v_max, v_rms = refs.v_fluid(ϱ, 𝒫, J, a, w, w, light_speed, exact=True)
    within_ulps(analysis.measure(c, 'v_rms', a), v_rms, f'{tag} v_rms')
    assert analysis.measure(c, 'v_max', a) == fluid.v_max(c, a) == v_max
    names, Δdiff_max_list, Δdiff_max_normalized_list = analysis.measure(c, 'discontinuity', a)
    want = refs.discontinuity_fluid(ϱ, J, 𝒫, L)
    assert names == want[0]
    assert np.array_equal(np.array(Δdiff_max_list), np.array(want[1])), tag
    assert np.array_equal(np.array(Δdiff_max_normalized_list), np.array(want[2])), tag


@pytest.mark.parametrize('g', [8, 12])
def test_fluid_quantities(g):
    w = float(golden()['w'])
    c, ϱ, J, 𝒫 = make_fluid(g, seed=30 + g, w=w)
    assert c.w_constant == w
    check_fluid(c, ϱ, J, 𝒫, 0.5, w, f'g = {g}')


def test_fluid_quantities_of_the_golden_component():
    """the fluid the reference's own measure() was called with"""
    from concept_amd import analysis, commons
    from test_gpu_fluid_drift import make_fluid as make
    g = golden()
    commons.load_params(str(g['param']))
    a, w = float(g['a']), float(g['w'])
    c = make(g['rho_in'], g['J_in'], g['P_in'])
    check_fluid(c, g['rho_in'], g['J_in'], g['P_in'], a, w, 'golden')
    Σmom, σmom = analysis.measure(c, 'momentum', a)
    within_ulps(σmom, g['fluid_momentum_sigma'], 'golden σmom')
    assert np.allclose(Σmom[1:], g['fluid_momentum_sum'][1:], rtol=1e-13, atol=0)
    assert analysis.measure(c, 'ϱ', a)[2] == g['fluid_rho'][2]
    assert np.array_equal(np.array(analysis.measure(c, 'discontinuity', a)[1]),
                          g['fluid_discontinuity'])
    assert abs(analysis.measure(c, 'v_rms', a) - float(g['fluid_v_rms'])) \
        <= 1e-13*float(g['fluid_v_rms'])


# -- discontinuity ---------------------------------------------------------------------------------
def device_discontinuity(ctx, grid, h, lo=None, hi=None, gridsize=None):
    import torch
    from concept_amd.lib import _ptr, check, raw
    out = torch.full((6,), -7.0, dtype=torch.float64, device='cuda')
    keep = [gpu(grid), None if lo is None else gpu(lo), None if hi is None else gpu(hi)]
    check(raw().cg_measure_discontinuity(ctx, _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                         gridsize or grid.shape[1], grid.shape[0], 1/h,
                                         _ptr(out)))
    out = out.cpu().numpy()
    return out[:3], out[3:]


def smooth(g, seed):
    rng = np.random.default_rng(seed)
    q = (np.arange(g) + 0.5)*(2*np.pi/g)
    x, y, z = np.meshgrid(q, q, q, indexing='ij')
    return 1 + 0.3*np.sin(x)*np.cos(y + 0.4) + 0.1*np.sin(2*z + x) + 0.05*rng.normal(size=(g, g, g))


@pytest.mark.parametrize('g', [4, 8, 12])
def test_discontinuity_of_a_whole_grid(ctx, g):
    grid, h = smooth(g, seed=g), 8.0/g
    got, want = device_discontinuity(ctx, grid, h), refs.discontinuity(grid, h)
    print(f'g = {g}: {got} against {want}')
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_discontinuity_of_slabs_with_their_neighbours_layers(ctx):
    """nxl < g with the layers below and above passed in: every slab equals the restatement, and
    the slabs' maxima are the whole grid's"""
    g, h = 8, 0.37
    grid = smooth(g, seed=41)
    whole = refs.discontinuity(grid, h)
    worst = [np.zeros(3), np.zeros(3)]
    for x0, nxl in ((0, 3), (3, 1), (4, 4)):
        slab, lo, hi = grid[x0:x0 + nxl], grid[(x0 - 1) % g], grid[(x0 + nxl) % g]
        got = device_discontinuity(ctx, slab, h, lo, hi, gridsize=g)
        want = refs.discontinuity(slab, h, lo, hi)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (x0, nxl)
        worst = [np.maximum(worst[0], got[0]), np.maximum(worst[1], got[1])]
    assert np.array_equal(worst[0], whole[0]) and np.array_equal(worst[1], whole[1])
    assert np.array_equal(device_discontinuity(ctx, grid, h)[0], whole[0])


@pytest.mark.parametrize('cell', [(0, 3, 4), (7, 3, 4), (3, 0, 4), (3, 7, 4), (3, 4, 0), (3, 4, 7)])
def test_discontinuity_with_the_extreme_on_a_face(ctx, cell):
    g, h = 8, 1.0
    grid = smooth(g, seed=43)
    grid[cell] += 50.0
    got, want = device_discontinuity(ctx, grid, h), refs.discontinuity(grid, h)
    assert want[0].min() > 90    # the spike sets all three maxima
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_discontinuity_of_a_constant_fluid():
    from concept_amd import analysis, commons
    from test_gpu_fluid_drift import make_fluid as make
    commons.load_params(str(golden()['param']))
    ϱ = np.full((8, 8, 8), 2.75)
    c = make(ϱ, [0.5*ϱ, -ϱ, 0*ϱ], 3*ϱ)
    names, Δdiff_max_list, Δdiff_max_normalized_list = analysis.measure(c, 'discontinuity')
    assert names == refs.FLUIDSCALAR_NAMES
    assert not np.array(Δdiff_max_list).any() and not np.array(Δdiff_max_normalized_list).any()
