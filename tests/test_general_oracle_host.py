"""orc_fourier_operate and orc_copy_modes (oracle/pm_oracle.c, through oracle/pm_general.py)
against a numpy.longdouble restatement over the whole slab (tests/general_kernel_refs.py), at
every case test_gpu_general_kernels.py runs on the GPU (no GPU here).

Three things are asserted:
  * which elements the oracle leaves alone: the three Nyquist planes always (the zeroing of a
    nullified target is the caller's), and with copy_modes between different sizes every mode of
    the larger grid outside the small cube — bit for bit;
  * the oracle's deviation from the long-double value, mode by mode, in units of
    eps*|M|*|input mode| (M: the complex factor of the mode), stays within ORACLE_DEV_EPS;
  * ORACLE_DEV_EPS[deconv_order] IS the worst deviation measured over all '=' cases (rounded up
    to three digits): the GPU test takes its bar from that table alone."""
import functools

import numpy as np
import pytest

import general_kernel_refs as R
from oracle import oracle as O
from oracle import pm_general

BOX = 64.0
EPS = R.EPS
MODES = ('inplace', 'copy=', 'copy+=')


def test_long_double_resolves_a_double_rounding():
    assert np.finfo(np.longdouble).eps <= 2.0**-63
    assert abs(float(R.PI_LD - R.LD(np.pi)) - 1.2246467991473532e-16) < 1e-19


def random_slab(N, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.normal(0, 1, (N, N, N + 2)))


def orc_operate(src, onto, N, case, op_add):
    """the C function itself: the early exits of pm_general.fourier_operate would bypass it"""
    order, nl, shift, dd = case
    sh = np.ascontiguousarray(shift, dtype=np.float64)
    pm_general._lib().orc_fourier_operate(O._p(src), O._p(onto), N, int(order), int(nl), O._p(sh),
                                          int(dd), 2*np.pi/BOX, int(op_add), O.machine_eps)


def orc_copy(src, N_from, onto, N_onto, case, op_add):
    order, nl, shift = case
    sh = np.ascontiguousarray(shift, dtype=np.float64)
    pm_general._lib().orc_copy_modes(O._p(src), N_from, O._p(onto), N_onto, int(order), int(nl),
                                     O._p(sh), int(op_add), O.machine_eps)


@functools.lru_cache(maxsize=None)
def operate_sweep(N, mode):
    """{deconv_order: worst deviation in eps*|M|*|mode|} over the cases of (N, mode); with '+='
    the rounding of the sum is taken out first (half an eps of the result)"""
    large = N in R.GRIDS_LARGE
    cases = R.operate_cases_large() if large else R.operate_cases()
    if large and mode != 'inplace':
        cases = cases[:2]
    a, b = random_slab(N, N), random_slab(N, N + 1)
    A, B = R.as_modes(a), R.as_modes(b)
    live = R.live_mask(N)
    worst = {}
    for case in cases:
        op_add = mode == 'copy+='
        onto = a.copy() if mode == 'inplace' else b.copy()
        before = R.as_modes(onto).copy()
        orc_operate(onto if mode == 'inplace' else a, onto, N, case, op_add)
        got = R.as_modes(onto)
        # the Nyquist planes are not touched, in any mode
        assert R.same_bits(got[~live], before[~live]), (N, mode, case)
        M, ref = R.expect_operate(A, B, N, BOX, case, op_add)
        scale = (np.abs(M).astype(np.float64)*np.abs(A))[live]
        err = np.abs(got.astype(R.CLD) - ref).astype(np.float64)[live]
        if op_add:
            err = np.maximum(err - 0.5*EPS*np.abs(got[live]), 0)
        assert (err[scale == 0] == 0).all()
        dev = float((err[scale > 0]/(EPS*scale[scale > 0])).max()) if (scale > 0).any() else 0.0
        worst[case[0]] = max(worst.get(case[0], 0.0), dev)
    return worst


@functools.lru_cache(maxsize=None)
def copy_sweep(N_from, N_onto, op_add):
    large = max(N_from, N_onto) > 100
    cases = R.copy_cases_large() if large else R.copy_cases()
    a, b = random_slab(N_from, N_from), random_slab(N_onto, N_onto + 1)
    A, B = R.as_modes(a), R.as_modes(b)
    worst = {}
    for case in cases:
        onto = b.copy()
        orc_copy(a, N_from, onto, N_onto, case, op_add)
        got = R.as_modes(onto)
        cube, M, scale, ref = R.expect_copy(A, B, N_from, N_onto, BOX, case, op_add)
        outside = np.ones(got.shape, dtype=bool)
        outside[cube] = False
        # modes of a larger `onto` outside the cube, and the Nyquist planes of both index ranges
        assert outside.sum() == got.size - (min(N_from, N_onto) - 1)**2*(min(N_from, N_onto)//2)
        assert R.same_bits(got[outside], B[outside]), (N_from, N_onto, case)
        err = np.abs(got[cube].astype(R.CLD) - ref).astype(np.float64)
        if op_add:
            err = np.maximum(err - 0.5*EPS*np.abs(got[cube]), 0)
        assert (scale > 0).all()
        worst[case[0]] = max(worst.get(case[0], 0.0), float((err/(EPS*scale)).max()))
    return worst


def within_table(worst, slack=0.0):
    for order, dev in worst.items():
        assert dev <= R.ORACLE_DEV_EPS[order] + slack, (order, dev, R.ORACLE_DEV_EPS[order])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N', R.GRIDS_SMALL + R.GRIDS_LARGE)
def test_oracle_fourier_operate(N, mode):
    # '+=': the sum's own rounding beyond half an eps of the result (the term's share of it)
    within_table(operate_sweep(N, mode), slack=0.5 if mode == 'copy+=' else 0.0)


COPY_DIRECTIONS = [p for pair in R.COPY_PAIRS_SMALL + (R.COPY_PAIR_LARGE,)
                   for p in (pair, pair[::-1])]


@pytest.mark.parametrize('op_add', [False, True])
@pytest.mark.parametrize('N_from,N_onto', COPY_DIRECTIONS)
def test_oracle_copy_modes(N_from, N_onto, op_add):
    within_table(copy_sweep(N_from, N_onto, op_add), slack=0.5 if op_add else 0.0)


def test_equal_sizes_go_through_fourier_operate():
    N = 12
    a, b = random_slab(N, 1), random_slab(N, 2)
    for case in R.copy_cases((0, 4)):
        for op_add in (False, True):
            x, y = b.copy(), b.copy()
            orc_operate(a, x, N, case + (-1,), op_add)
            if case[0] == 0 and case[2] == (0.0, 0.0, 0.0):
                continue   # pm_general's early exit: plain numpy, the Nyquist planes included
            pm_general.copy_modes(a, y, BOX, case[0], case[1], case[2], op_add=op_add)
            assert R.same_bits(x, y)


def test_oracle_deviation_table():
    """the table is what was measured: no '=' case beyond it, and the worst one within 10 % of it"""
    worst = {}
    sweeps = [operate_sweep(N, mode) for N in R.GRIDS_SMALL + R.GRIDS_LARGE
              for mode in ('inplace', 'copy=')]
    sweeps += [copy_sweep(nf, no, False) for nf, no in COPY_DIRECTIONS]
    for s in sweeps:
        for order, dev in s.items():
            worst[order] = max(worst.get(order, 0.0), dev)
    print('measured worst deviation per deconv_order [eps*|M|*|mode|]:',
          {o: round(worst[o], 3) for o in sorted(worst)})
    assert sorted(worst) == list(R.ORDERS) == sorted(R.ORACLE_DEV_EPS)
    for order in R.ORDERS:
        assert 0.9*R.ORACLE_DEV_EPS[order] <= worst[order] <= R.ORACLE_DEV_EPS[order], (
            order, worst[order], R.ORACLE_DEV_EPS[order])
