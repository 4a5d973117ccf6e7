"""Plain references shared by test_general_oracle_host.py and test_gpu_general_kernels.py: the
k-space operations of the general particle_mesh() — fourier_operate (mesh.py:3327-3400) and
copy_modes (mesh.py:1018-1326) over fourier_loop (mesh.py:2615-2890) — restated in
numpy.longdouble over a whole slab, the finite differences of diff_domaingrid
(mesh.py:4874-5030) in float64 numpy, and the case lists both files run.

A slab is the reference's transposed one, double[j][i][N + 2] (what fetch_fourier() returns and
oracle/pm_oracle.c works on), seen as complex[j][i][N/2 + 1]: axis 0 is kj (y), axis 1 is ki (x).

The value of a mode after an operation is  M * (mode of `from`)  [+ previous value], with
  M = prod_d (n_d/sin n_d)^deconv_order / nlattice            n_d = k_d*pi/N_from + machine_eps
      * exp(i * -2*pi/N_from * (shift . k))                    the lattice phase
      * exp(i * (pi/N_onto - pi/N_from)*(ki + kj + kk))        re-centring (different sizes)
      * i*k_fundamental*k_dim                                  when diff_dim is given
Every factor is a product over the three dimensions, so M is an outer product of three vectors;
the vectors are evaluated in long double (64-bit mantissa: their own error is 2^-11 of a double's).

ORACLE_DEV_EPS is what test_general_oracle_host.py measured: the worst deviation of the float64
oracle (libm sin / cos / pow, theta and n rounded to double) from M * mode, in units of
eps*|M|*|mode|, per deconvolution order.  The GPU bar is made from it and from nothing else."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = float(np.finfo(np.float64).eps)
PI_LD = 4*np.arctan(LD(1))

# measured by test_general_oracle_host.py::test_oracle_deviation_table (which asserts it)
ORACLE_DEV_EPS = {0: 5.24, 1: 4.32, 2: 6.92, 3: 9.73, 4: 12.72, 5: 13.49, 6: 15.75, 7: 18.76,
                  8: 25.02}

GRIDS_SMALL = (12, 16)            # pad N + 2 / N + 16: the two layout families, cheap
GRIDS_LARGE = (144, 152)          # nyq 72 / 76: a second 64-lane trip; N*N > 16384 rows
COPY_PAIRS_SMALL = ((12, 16), (16, 24), (24, 32))
COPY_PAIR_LARGE = (144, 152)
ORDERS = tuple(range(9))
COPY_ORDERS = (0, 2, 4, 8)
DIFF_DIMS = (-1, 0, 1, 2)
SKEW_SHIFT = (0.5, -0.25, 0.125)  # three different components: a swapped A / B / Cc shows


def lattice_shifts(kind, cell_centered):
    """Lattice.shifts_all (mesh.py:77-100), as oracle/pm_general.py states it"""
    a = (1 - 2*cell_centered)*0.5
    return {'sc': [(0, 0, 0)],
            'bcc': [(0, 0, 0), (a, a, a)],
            'fcc': [(0, 0, 0), (0, a, a), (a, 0, a), (a, a, 0)]}[kind]


def lattice_cases(kinds=('sc', 'bcc', 'fcc')):
    """(nlattice, shift) of every sub-lattice of the SC, BCC and FCC lattices for both
    cell_centered values, and the skew shift"""
    cases = []
    for kind in kinds:
        for cc in (True, False):
            shifts = lattice_shifts(kind, cc)
            for s in shifts:
                case = (len(shifts), tuple(float(x) for x in s))
                if case not in cases:
                    cases.append(case)
    if 'bcc' in kinds:
        cases.append((2, SKEW_SHIFT))
    return cases


def operate_cases(orders=ORDERS, lattices=None, diff_dims=DIFF_DIMS):
    """the cross product (deconv_order, nlattice, shift, diff_dim)"""
    lattices = lattice_cases() if lattices is None else lattices
    return [(o, nl, sh, dd) for o in orders for (nl, sh) in lattices for dd in diff_dims]


def operate_cases_large():
    """the handful for N = 144 and 152: order 8 + FCC + each diff_dim among them"""
    a = 0.5
    return [(8, 4, (0.0, -a, -a), 0), (8, 4, (-a, 0.0, -a), 1), (8, 4, (a, a, 0.0), 2),
            (8, 4, (0.0, a, a), -1), (4, 2, (-a, -a, -a), -1), (3, 2, SKEW_SHIFT, 1),
            (0, 1, (0.0, 0.0, 0.0), 2), (1, 4, (0.0, 0.0, 0.0), -1)]


def copy_cases(orders=COPY_ORDERS):
    """(deconv_order, nlattice, shift) of copy_modes: SC, BCC, FCC and the skew shift"""
    return [(o, nl, sh) for o in orders for (nl, sh) in lattice_cases()]


def copy_cases_large():
    a = 0.5
    return [(8, 4, (0.0, -a, -a)), (8, 4, (a, 0.0, a)), (4, 2, (-a, -a, -a)),
            (2, 2, SKEW_SHIFT), (0, 1, (0.0, 0.0, 0.0))]


# ---------------------------------------------------------------------------------------------
# k-space
# ---------------------------------------------------------------------------------------------
def wave_numbers(N):
    """k of every array index of a grid of size N (the Nyquist index counts as -N/2)"""
    idx = np.arange(N)
    return idx - N*(idx >= N//2)


def live_mask(N):
    """[j][i][kk] -> True off the three Nyquist planes"""
    nyq = N//2
    m = np.ones((N, N, nyq + 1), dtype=bool)
    m[nyq, :, :] = False
    m[:, nyq, :] = False
    m[:, :, nyq] = False
    return m


def as_modes(slab):
    """double[j][i][N + 2] -> complex[j][i][N/2 + 1] (a view)"""
    return np.ascontiguousarray(slab).view(np.complex128)


def multiplier(kj, ki, kk, N_from, N_onto, boxsize, deconv_order=0, nlattice=1,
               shift=(0.0, 0.0, 0.0), diff_dim=-1):
    """M[j][i][kk] (clongdouble) for the wave numbers given per axis"""
    vectors = []
    dtheta = PI_LD/LD(N_onto) - PI_LD/LD(N_from)
    for dim, k in ((1, kj), (0, ki), (2, kk)):   # shift[0], diff_dim 0 belong to ki
        k = np.asarray(k).astype(LD)
        n = k*(PI_LD/LD(N_from)) + LD(EPS)
        v = (n/np.sin(n))**int(deconv_order)
        theta = (LD(-2)*PI_LD/LD(N_from)*LD(shift[dim]))*k + dtheta*k
        v = v*(np.cos(theta) + 1j*np.sin(theta)).astype(CLD)
        if diff_dim == dim:
            v = v*(1j*(LD(2)*PI_LD/LD(boxsize))*k).astype(CLD)
        vectors.append(v.astype(CLD))
    vj, vi, vk = vectors
    return (vj[:, None, None]*vi[None, :, None])*vk[None, None, :]/LD(nlattice)


def expect_operate(A, prev, N, boxsize, case, op_add):
    """fourier_operate / the equal-size copy_modes: (M, M*A [+ prev]) over the whole slab of
    modes; the caller masks the Nyquist planes"""
    order, nl, shift, dd = case
    k = wave_numbers(N)
    M = multiplier(k, k, np.arange(N//2 + 1), N, N, boxsize, order, nl, shift, dd)
    ref = M*A.astype(CLD)
    if op_add:
        ref = ref + prev.astype(CLD)
    return M, ref


def cube_index(N_small, N):
    """array indices in a grid of size N of the small grid's wave numbers off its Nyquist plane"""
    k = np.arange(-(N_small//2 - 1), N_small//2)
    return k, k % N


def expect_copy(A, prev, N_from, N_onto, boxsize, case, op_add):
    """copy_modes between different sizes: (index of the cube in `onto`, M, value) for the
    small cube's modes; everything else of `onto` is not touched"""
    order, nl, shift = case
    NS = min(N_from, N_onto)
    k, i_from = cube_index(NS, N_from)
    _, i_onto = cube_index(NS, N_onto)
    kk = np.arange(NS//2)
    M = multiplier(k, k, kk, N_from, N_onto, boxsize, order, nl, shift, -1)
    src = A[np.ix_(i_from, i_from, kk)]
    ref = M*src.astype(CLD)
    if op_add:
        ref = ref + prev[np.ix_(i_onto, i_onto, kk)].astype(CLD)
    return np.ix_(i_onto, i_onto, kk), M, np.abs(M).astype(np.float64)*np.abs(src), ref


def deviation(got, ref, scale):
    """max of |got - ref| / (eps*scale) where scale > 0; where it is 0 the two must agree"""
    err = np.abs(got.astype(CLD) - ref).astype(np.float64)
    zero = scale == 0
    assert (err[zero] == 0).all()
    if zero.all():
        return 0.0
    return float((err[~zero]/(EPS*scale[~zero])).max())


def mode_bar(order, scale, prev=None):
    """the bar of the GPU comparisons: 2*ORACLE_DEV_EPS[order]*eps*|M|*|mode|, and with '+='
    2*eps*|previous value| more"""
    bar = 2*ORACLE_DEV_EPS[order]*EPS*scale
    if prev is not None:
        bar = bar + 2*EPS*np.abs(prev)
    return bar


def check_modes(got, ref, bar, what):
    err = np.abs(got.astype(CLD) - ref).astype(np.float64)
    bad = err > bar
    if bad.any():
        worst = np.unravel_index(np.argmax(np.where(bar > 0, err/np.where(bar > 0, bar, 1), err)),
                                 err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} modes beyond the bar, worst at [j, i, kk] = '
                             f'{worst}: |got - ref| = {err[worst]:.3e}, bar {bar[worst]:.3e}')


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64),
                          np.ascontiguousarray(b).view(np.int64))


# ---------------------------------------------------------------------------------------------
# diff_domaingrid, term by term as fd_value() in cg_general.hip (contraction is off there, so
# float64 numpy in the same order gives the same bits)
# ---------------------------------------------------------------------------------------------
def fd_reference(f, dim, order, dx):
    def d(s):
        return np.roll(f, -s, axis=dim) - np.roll(f, s, axis=dim)
    if order == 0:
        return f.copy()
    if order == 1:
        return (1/dx)*(np.roll(f, -1, axis=dim) - f)
    if order == 2:
        return ((1.0/2)/dx)*d(1)
    if order == 4:
        return ((2.0/3)/dx)*d(1) - ((1.0/12)/dx)*d(2)
    if order == 6:
        return (((3.0/4)/dx)*d(1) - ((3.0/20)/dx)*d(2)) + ((1.0/60)/dx)*d(3)
    assert order == 8
    return ((((4.0/5)/dx)*d(1) - ((1.0/5)/dx)*d(2)) + ((4.0/105)/dx)*d(3)) - ((1.0/280)/dx)*d(4)


def kick_reference(J, rho, P, g, minus_dt, inv_c2):
    """Jᵢ += ℝ[-ᔑdt]*(ϱ + ℝ[c⁻²]*𝒫)*grid   (interactions.py:2397-2400)"""
    return J + minus_dt*(rho + inv_c2*P)*g


def distinct_field(N, seed):
    """a value per cell that no other cell has (a wrong wrap cannot cancel)"""
    rng = np.random.default_rng(seed)
    f = rng.permutation(N**3).astype(np.float64).reshape(N, N, N)
    return f/N**3 + rng.uniform(0.25, 0.5, (N, N, N))
