"""oracle/rungs.py at the inputs its goldens never reach (no GPU): Particles.get_rung on a
hand-written table read off the reference's get_rung (species.py:2341-2363), the rung factors
handed to flag_rung_jumps directly, and the two populations the GPU tests of the rung kernels
(test_gpu_rung_kernels.py) run on: the exact edge table and random accelerations that keep their
distance from every decision.

The edge table: accelerations (±2^m, 0, 0), (0, 2^m, 0), (0, 0, 2^m), so acc2 = 2^(2m), log2 is
exact and f = rung_factor + m/2 is exact for a rung factor that is a multiple of 0.25."""
import numpy as np
import pytest

from oracle import rungs

# (rung_factor, m, expected) for N_rungs = 4, by hand from species.py:2353-2360:
#   f = rung_factor + m/2;  f < 0 -> 0;  f > 3 -> 3;  else 1 + (signed char)f
HAND_N4 = [
    # rung factor 0
    (0.0, -600, 'current'),  # acc2 = 2^-1200 underflows to 0: "no information", current rung
    (0.0, -7, 0),     # f = -3.5
    (0.0, -1, 0),     # f = -0.5
    (0.0, 0, 1),      # f == 0
    (0.0, 1, 1),      # f = 0.5
    (0.0, 2, 2),      # f == 1
    (0.0, 3, 2),      # f = 1.5
    (0.0, 4, 3),      # f == 2
    (0.0, 5, 3),      # f = 2.5
    (0.0, 6, 4),      # f == N_rungs - 1 exactly: 1 + cast(3), one past the top rung
    (0.0, 7, 3),      # f = 3.5 > N_rungs - 1
    (0.0, 40, 3),     # f = 20
    (0.0, 600, 3),    # acc2 = inf
    # rung factor 1.5
    (1.5, -4, 0),     # f = -0.5
    (1.5, -3, 1),     # f == 0
    (1.5, -1, 2),     # f == 1
    (1.5, 0, 2),      # f = 1.5
    (1.5, 3, 4),      # f == 3
    (1.5, 4, 3),      # f = 3.5
    # rung factor -2.5
    (-2.5, 4, 0),     # f = -0.5
    (-2.5, 5, 1),     # f == 0
    (-2.5, 8, 2),     # f = 1.5
    (-2.5, 11, 4),    # f == 3
    (-2.5, 12, 3),    # f = 3.5
    # rung factors off the half grid: f is never an integer
    (0.25, -1, 0),    # f = -0.25
    (0.25, 0, 1),     # f = 0.25
    (0.25, 1, 1),     # f = 0.75
    (0.25, 5, 3),     # f = 2.75
    (0.25, 6, 3),     # f = 3.25 > 3
    (-0.75, 1, 0),    # f = -0.25
    (-0.75, 2, 1),    # f = 0.25
    (-0.75, 7, 3),    # f = 2.75
    (-0.75, 8, 3),    # f = 3.25
]
AXES = [(1.0, 0), (-1.0, 0), (1.0, 1), (1.0, 2)]   # (sign, component) of the acceleration


def particles(acc, rung, N_rungs):
    """the oracle's Particles around accelerations (held in Δmom) and current rungs"""
    acc = np.ascontiguousarray(acc, dtype=np.float64)
    p = rungs.Particles(np.zeros_like(acc), np.zeros_like(acc), 1.0, 1.0, N_rungs)
    p.dmom[...] = acc
    p.rung[:] = rung
    p.rung_jumped[:] = rung
    return p


def rung_rule(f, N_rungs):
    """species.py:2354-2360 for one exact f"""
    if f < 0:
        return 0
    if f > N_rungs - 1:
        return N_rungs - 1
    return 1 + int(f)


def edge_table(N_rungs, rung_factor):
    """Every f = rung_factor + m/2 in [-3, N_rungs + 2] — all of f < 0, f == 0, f == k,
    f == k + 0.5, f == N_rungs - 1 and f > N_rungs - 1 that the rung factor reaches — on the four
    AXES, then acc2 == 0 (exactly, and by underflow) and acc2 == inf; each row repeated for every
    current rung.  With N_rungs = 1 there is no f == 0.  Returns acc (R, 3), the current rungs
    (R,), the exact f (R,; -inf where acc2 == 0, inf where it overflows) and the rung the
    reference's get_rung returns (R,)."""
    assert 4*rung_factor == int(4*rung_factor)
    ms = [m for m in range(-200, 200)
          if -3 <= rung_factor + 0.5*m <= N_rungs + 2
          and not (N_rungs == 1 and rung_factor + 0.5*m == 0)]
    rows = []
    for m in ms:
        f = rung_factor + 0.5*m
        rows += [(s, ax, m, f, rung_rule(f, N_rungs)) for s, ax in AXES]
    for s, ax in AXES:
        rows.append((s, ax, 600, np.inf, N_rungs - 1))
        rows.append((s, ax, -600, -np.inf, None))
        rows.append((0.0, ax, 0, -np.inf, None))
    acc = np.zeros((len(rows), 3))
    for i, (s, ax, m, f, want) in enumerate(rows):
        acc[i, ax] = s*2.0**m
    f = np.array([row[3] for row in rows])
    R = len(rows)
    current = np.repeat(np.arange(N_rungs, dtype=np.int8), R)
    acc, f = np.tile(acc, (N_rungs, 1)), np.tile(f, N_rungs)
    want = np.array([current[i] if rows[i % R][4] is None else rows[i % R][4]
                     for i in range(R*N_rungs)], dtype=np.int8)
    return acc, current, f, want


def random_population(seed, n, N_rungs, rung_factor):
    """Accelerations that cannot sit on a decision: the target f uniform over [-3, N_rungs + 2]
    with its fractional part in [0.01, 0.99], |acc| = 2^(2 (f - rung_factor)) in a random
    direction; every seventh particle has none.  The current rungs are drawn over all rungs."""
    rng = np.random.default_rng(seed)
    f = rng.integers(-3, N_rungs + 2, n) + rng.uniform(0.01, 0.99, n)
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d**2).sum(1))[:, None]
    acc = d*(2.0**(2*(f - rung_factor)))[:, None]
    acc[::7] = 0
    return acc, rng.integers(0, N_rungs, n).astype(np.int8)


def distance_from_decisions(p, rung_factor):
    """how far the oracle's own rung_index_float stays from the integers (where every
    comparison and the cast of get_rung decide), over the particles that have an acceleration"""
    acc2, f = p.rung_index_float(rung_factor)
    f = f[acc2 != 0]
    return np.abs(f - np.rint(f)).min() if f.size else np.inf


@pytest.mark.parametrize('current', [0, 1, 2, 3])
def test_get_rung_hand_table(current):
    acc = np.zeros((len(HAND_N4)*len(AXES), 3))
    want, rf = [], []
    for i, (factor, m, w) in enumerate(HAND_N4):
        for j, (s, ax) in enumerate(AXES):
            acc[len(AXES)*i + j, ax] = s*2.0**m
            want.append(current if w == 'current' else w)
            rf.append(factor)
    rf = np.array(rf)
    p = particles(acc, current, 4)
    assert np.array_equal(p.get_rung(rf), np.array(want, dtype=np.int8))
    # one factor at a time, as the kernels take it
    for factor in sorted(set(rf)):
        sel = rf == factor
        q = particles(acc[sel], current, 4)
        assert np.array_equal(q.get_rung(factor), np.array(want, dtype=np.int8)[sel])
    # no acceleration at all: the current rung, whatever the factor
    z = particles(np.zeros((3, 3)), current, 4)
    for factor in (-50.0, 0.0, 50.0):
        assert np.array_equal(z.get_rung(factor), np.full(3, current, dtype=np.int8))


@pytest.mark.parametrize('rung_factor', [0.0, 1.5, -2.5, 0.25, -0.75])
@pytest.mark.parametrize('N_rungs', [1, 4, 8, 21, 42])
def test_edge_table_is_what_the_oracle_gives(N_rungs, rung_factor):
    acc, current, f, want = edge_table(N_rungs, rung_factor)
    p = particles(acc, current, N_rungs)
    acc2, f_oracle = p.rung_index_float(rung_factor)
    assert np.array_equal(f_oracle, f)                   # exact, ±inf included
    assert np.array_equal(p.get_rung(rung_factor), want)
    assert want.min() >= 0 and want.max() <= N_rungs
    if 2*rung_factor == int(2*rung_factor) and N_rungs > 1:
        assert (f == 0).any() and (want[f == 0] == 1).all()
        assert (want[f == N_rungs - 1] == N_rungs).all() and (f == N_rungs - 1).any()
    else:
        assert want.max() <= N_rungs - 1
    assert (want[f == np.inf] == N_rungs - 1).all() and (f == np.inf).any()
    assert (want[f == -np.inf] == current[f == -np.inf]).all()
    assert (want[(f < 0) & (f > -np.inf)] == 0).all()


@pytest.mark.parametrize('N_rungs', [1, 4, 8, 21, 42])
def test_random_population_keeps_its_distance(N_rungs):
    for rung_factor in (1.25, 0.25, 3.25):
        acc, rung = random_population(N_rungs, 100003, N_rungs, rung_factor)
        p = particles(acc, rung, N_rungs)
        assert distance_from_decisions(p, rung_factor) >= 1e-2
        assert distance_from_decisions(p, rung_factor + 2) >= 1e-2   # (an integer apart)
        got = p.get_rung(rung_factor)
        assert not (acc[::7] != 0).any() and np.array_equal(got[::7], rung[::7])
        if N_rungs >= 4:
            assert set(np.unique(got)) == set(range(N_rungs))     # never N_rungs: no exact hit


def test_flag_rung_jumps_takes_the_rung_factors():
    """rung_factors=(up, down) stands for what dt, dt_jump_fac and fac_softening give; a
    hand-made population: up, down, a locked down, an up that wins over a down, stays."""
    N_rungs, dt, jump, fs = 4, 0.37, 0.9, 0.03
    acc, rung = random_population(1, 5000, N_rungs, 1.0)
    dtr = rungs.new_dt_rungs(N_rungs)
    dtr[rungs.KEY_1][:] = 0.5
    dtr[rungs.KEY_1][N_rungs + 2] = -1
    p, q = particles(acc, rung, N_rungs), particles(acc, rung, N_rungs)
    p.softening_length = q.softening_length = 0.7
    factors = (p.get_rung_factor(dt*jump, fs), p.get_rung_factor(dt/jump, fs))
    assert p.flag_rung_jumps(dt, jump, fs, dtr) == q.flag_rung_jumps(None, None, None, dtr, factors)
    assert np.array_equal(p.rung_jumped, q.rung_jumped) and (p.rung_jumped != p.rung).any()
    # by hand: f_up = 2 + m/2, f_down = m/2 (factors 2 and 0), N_rungs = 4
    #   m   rung  lock   f_up f_down  ought_up ought_down   flag
    #   0    1     -      2     0       3        1          up     (1 + 8)
    #   0    3     -      2     0       3        1          down   (3 + 4)
    #   0    2    -1      2     0       3        1          up: the lock holds no up-jump (2 + 8)
    #  -4    2    -1      0    -2       1        0          stays: the down-jump is locked
    #  -4    3     -      0    -2       1        0          down   (3 + 4)
    #  -2    2    -1      1    -1       2        0          stays
    #  -2    1     -      1    -1       2        0          up wins over down (1 + 8)
    #   2    3     -      3     1       4        2          up, on the top rung (3 + 8)
    #  acc=0 2     -                                        stays
    #   0    0   integral 0                                 stays
    m = [0, 0, 0, -4, -4, -2, -2, 2, None, 0]
    rung = np.array([1, 3, 2, 2, 3, 2, 1, 3, 2, 0], dtype=np.int8)
    acc = np.zeros((len(m), 3))
    acc[:, 1] = [0.0 if v is None else 2.0**v for v in m]
    dtr[rungs.KEY_1][0] = 0
    p = particles(acc, rung, N_rungs)
    assert p.flag_rung_jumps(None, None, None, dtr, (2.0, 0.0))
    assert p.rung_jumped.tolist() == [9, 7, 10, 2, 7, 2, 9, 11, 2, 0]
    p.lowest_active_rung = 2
    p.rung_jumped[:] = rung
    assert p.flag_rung_jumps(None, None, None, dtr, (2.0, 0.0))
    assert p.rung_jumped.tolist() == [1, 7, 10, 2, 7, 2, 1, 11, 2, 0]
    p.apply_rung_jumps()
    assert p.rung.tolist() == [1, 2, 3, 2, 2, 2, 1, 4, 2, 0]
    assert np.array_equal(p.rung, p.rung_jumped)
