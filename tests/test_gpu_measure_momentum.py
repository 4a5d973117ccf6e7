"""cg_measure_momentum and cg_measure_momentum_regions (k_measure_mom, k_measure_mom_regions,
k_measure_final: the sum of mom² and the largest |mom_i|² behind v_rms and v_max, and so behind
the base time step; analysis.py:3902-3972) against numpy.

The reference is m2 = (x*x + y*y) + z*z in float64, the kernel's own order of operations
without contraction.  max(m2) is compared bit for bit.  The sum is compared with math.fsum(m2)
within a relative 1e-13: every term is non-negative, so any order of adding n <= 2^20 terms
stays within about log2(n) ulp, 20 * 1.1e-16."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-13
BLOCKS, THREADS = 1024, 256     # k_measure_mom: at most 1024 workgroups of 256, contiguous shares
SIZES = [1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 700001]


@pytest.fixture(scope='module')
def mesh():
    from concept_amd.mesh import PotentialMesh
    m = PotentialMesh(32, 32.0)
    yield m
    m.close()


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def momenta(seed, n):
    """normal, scaled per particle by exp(3 normal): the sum is not a matter of the count"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3))*np.exp(3*rng.normal(size=(n, 1)))


def squares(mom):
    return (mom[:, 0]*mom[:, 0] + mom[:, 1]*mom[:, 1]) + mom[:, 2]*mom[:, 2]


def reference(mom):
    m2 = squares(mom)
    return math.fsum(m2), float(m2.max())


def check(got, mom, what=None, m2=None):
    """mom: the momenta, or None with their squares() in m2"""
    s_ref, m_ref = reference(mom) if m2 is None else (math.fsum(m2), float(m2.max()))
    s, m = got
    print(f'{what}: sum {s!r} (fsum {s_ref!r}, rel {abs(s - s_ref)/s_ref:.2e}), max {m!r} '
          f'(numpy {m_ref!r})')
    assert m == m_ref, what
    assert abs(s - s_ref) <= SUM_RTOL*s_ref, what


def shares(n):
    """k_measure_mom's split: (workgroups, rows per workgroup, non-empty workgroups)"""
    nb = max(1, min((n + THREADS - 1)//THREADS, BLOCKS))
    per = (n + nb - 1)//nb
    return nb, per, (n + per - 1)//per


def placements(n):
    """rows at which a lost maximum would show: the ends, the last row of the first
    workgroup's share, the first row of the last non-empty workgroup, and rows that lane 63
    of a wave — of the last wave, where the share is long enough — handles in the first and the
    last non-empty workgroup"""
    nb, per, used = shares(n)
    rows = {0, n - 1, min(per, n) - 1, (used - 1)*per}
    for p0 in (0, (used - 1)*per):
        p1 = min(p0 + per, n)
        rows |= {p0 + t for t in (63, 127, 191, 255, 255 + THREADS) if p0 + t < p1}
    return sorted(rows)


def test_the_split_this_file_assumes():
    assert shares(1) == (1, 1, 1) and shares(257) == (2, 129, 2)
    assert shares(262144) == (1024, 256, 1024) and shares(262145) == (1024, 257, 1021)
    assert shares(700001) == (1024, 684, 1024)
    assert placements(64) == [0, 63] and 255 in placements(256) and 255 not in placements(257)
    assert placements(262145) == [0, 63, 127, 191, 255, 256, 262140, 262144]
    assert {0, 255, 511, 683, 699732, 699987, 700000} <= set(placements(700001))


@pytest.mark.parametrize('n', SIZES)
def test_dense_sum_and_max(mesh, n):
    mom = momenta(n, n)
    t = gpu(mom)
    first = mesh.measure_momentum(t)
    check(first, mom, 'as drawn')
    assert mesh.measure_momentum(t) == first                   # the same bits again
    check(mesh.measure_momentum(gpu(-np.abs(mom))), -np.abs(mom), 'all components negative')
    # one dominant particle, a few times the second largest, wherever a reduction could lose it
    m2 = squares(mom)
    biggest = math.sqrt(m2.max())
    plants = [np.array([1.0, -1.0, 1.0])*biggest*1.7, np.array([3.1*biggest, 0.0, 0.0]),
              np.array([0.0, -3.1*biggest, 0.0]), np.array([0.0, 0.0, 3.1*biggest])]
    for row in placements(n):
        # (in one component only: at the last row)
        for k, plant in enumerate(plants if row == n - 1 else plants[:1]):
            planted = m2.copy()
            planted[row] = squares(plant[None, :])[0]
            assert planted[row] > 8*m2.max()       # (and so above every other particle's)
            t2 = t.clone()
            t2[row] = gpu(plant)
            check(mesh.measure_momentum(t2), None, f'row {row}, plant {k}', planted)


def test_dense_no_particles(mesh):
    import torch
    assert mesh.measure_momentum(torch.empty((0, 3), dtype=torch.float64, device='cuda')) \
        == (0.0, 0.0)


def test_regions_read_the_live_rows_only(mesh):
    """Particles in tile regions with gaps, laid out by cg_predict_regions as RegionParticles
    does; every dead slot holds 1e150, which would blow up the sum and the maximum if read.
    Some regions are empty, one holds more than 256 rows.  Then the dense tile order (count =
    None) of the same particles."""
    import torch
    L, n_box, n_blob = 32.0, 3000, 700
    n = n_box + n_blob
    rng = np.random.default_rng(12)
    pos = rng.uniform(0, L, (n, 3))
    pos[:n_box, 0] *= 0.5                                     # half of the box stays empty
    pos[n_box:] = 10.3 + rng.uniform(0, 0.2, (n_blob, 3))     # inside one cell
    mom = momenta(13, n)
    pos_t, mom_t, ids = gpu(pos), gpu(mom), torch.arange(n, device='cuda')
    po, mo, io = torch.empty_like(pos_t), torch.empty_like(mom_t), torch.empty_like(ids)
    table = mesh.sort_particles(pos_t, mom_t, ids, po, mo, io)
    nreg = 8*mesh.ntiles
    dense = table[:nreg + 1].contiguous()
    start_out, count = mesh.new_region_table()
    mesh.predict_regions(dense, None, start_out)
    d = dense.cpu().numpy().astype(np.int64)
    s = start_out.cpu().numpy().astype(np.int64)
    cnt = np.diff(d)
    assert d[0] == 0 and d[-1] == n and (cnt == 0).any() and cnt.max() > 256
    assert (np.diff(s) >= cnt).all() and s[-1] > n and s[-1] <= mesh.region_capacity(n)
    sorted_mom = mo.cpu().numpy()
    assert np.array_equal(sorted_mom, mom[io.cpu().numpy()])
    live = np.repeat(s[:-1] - d[:-1], cnt) + np.arange(n)    # row of every particle
    rows = np.full((mesh.region_capacity(n), 3), 1e150)
    rows[live] = sorted_mom
    assert (rows == 1e150).all(1).sum() == rows.shape[0] - n
    count.copy_(gpu(cnt.astype(np.int32)))
    check(mesh.measure_momentum_regions(gpu(rows), start_out, count), sorted_mom, 'regions')
    check(mesh.measure_momentum_regions(mo, dense, None), sorted_mom, 'dense tile order')
    # the maximum in the last live row of the big region, of the last populated region, and in
    # the first row of all
    biggest = math.sqrt(reference(mom)[1])
    big, last = int(np.argmax(cnt)), int(np.nonzero(cnt)[0][-1])
    for q in (d[big + 1] - 1, d[last + 1] - 1, d[big] + 255, d[big] + 256, 0):
        planted = sorted_mom.copy()
        planted[q] = (0.0, 0.0, -3.1*biggest)
        rows[live] = planted
        check(mesh.measure_momentum_regions(gpu(rows), start_out, count), planted,
              f'regions, row {q}')
        check(mesh.measure_momentum_regions(gpu(planted), dense, None), planted,
              f'dense tile order, row {q}')
