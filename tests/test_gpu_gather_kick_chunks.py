"""GPU tests of the fused gather + finite difference + kick for particles in any memory order
(cg_gather_kick: k_gather_kick_chunks<2|4> in cg_mesh_kernels.hip) on BOTH of its code paths,
with the particle sets of test_gpu_general_interp.py.

A workgroup takes 2048 consecutive particles.  Its box is the box of their CIC cells with the
reach H = diff_order/2 of the difference on both sides: per axis the span of the cells plus
W = 2 + 2*H (4 cells at order 2, 6 at order 4).  When that fits 4096 cells of LDS the chunk
copies the box of the potential in and reads it there (the box path), else it reads the mesh
(the direct path).  The sets are built so that the path of every chunk is certain from the
geometry: compact chunks (8 cells + W <= 14 per axis), chunks with two particles 32 cells
apart, cubes across the periodic seam, boxes at the 4096-cell limit and one cell past it (built
per difference order), boxes that cover a whole axis, 6144 particles on one spot, and particles
on and one ulp off the points where the cell index switches.

Reference: NumPy, written from the formulas.  CIC index and weights per axis in float64 (exact on
both sides: no contraction in the kernel), coefficients c1, c2 in float64 as the library forms
them; then in np.longdouble, for each dimension, the force cell values
    f = c1*(phi(+1) - phi(-1)) [- c2*(phi(+2) - phi(-2))]
at the particle's eight cells, value = sum f*((wx*wy)*wz), value*factor, mom + value.

Bound per particle and component (u = 2**-53), derived, not tuned.  One term f*w goes through
R roundings in the kernel: the difference, its product with c1 and the product with w at order
2 (R = 3); two differences, two products, their difference and the product with w at order 4
(R = 6).  Each rounding is relative to a partial result no larger than
    m = (c1*(|phi(+1)| + |phi(-1)|) + c2*(|phi(+2)| + |phi(-2)|))*w,
so a term is off by at most R*u*m to first order.  The eight additions add 8*u*sum(m) (seven
round; the eighth u*sum(m) covers the second-order terms, (R + 8)**2/2*u**2*sum(m)).  Then the
product with factor and the sum with mom round once each:
    |factor|*(R + 8)*u*sum(m) + u*|value*factor| + u*|mom + value*factor|
test_reference_in_kernel_order_is_inside_the_bound evaluates the same formulas in float64 in the
kernel's operation order on every scenario, without a GPU, and finds them inside this bound.

Compact against shuffled memory order: the same particles in compact order (box path) and in
shuffled order (direct path) receive bit-identical kicks (the loop over the stencil is the same
on both paths).  The field is written with NaN in the padding, so a stencil that reads outside
the mesh shows.  Every test prints its largest error/bound ratio."""
import numpy as np
import pytest

import test_gpu_general_interp as gi
from test_gpu_general_interp import CHUNK, COUNTS, L_BOX, U

DIFFS = [2, 4]
FACTORS = (-0.37, 1.0)


def kick_cases(N, diff):
    """CIC on the plain lattice, cell- and vertex-centred, with the ghosts the difference needs"""
    from oracle import pm_general
    out = []
    for cc in (True, False):
        case = gi.Case(N, 2, cc, 'sc')
        case.g = max(case.g, 2)
        case.geom = {sign: pm_general.interp_geometry(L_BOX, N, case.g, case.shift, sign, cc)
                     for sign in (-1, +1)}
        out.append(case)
    return out


def fd_coefficients(diff, dx):
    return ((1.0/2)/dx, 0.0) if diff == 2 else ((2.0/3)/dx, (1.0/12)/dx)


def ref_kick(case, diff, pos, mom, field, factor, dtype=np.longdouble):
    """-> expected momenta (n, 3) in `dtype` and the bound per particle and component;
    dtype=np.float64 evaluates in the kernel's operation order"""
    N = case.N
    first, w = case.stencil(pos, +1)
    c1, c2 = (dtype(c) for c in fd_coefficients(diff, L_BOX/N))
    phi = field.astype(dtype)
    n = pos.shape[0]
    value = np.zeros((n, 3), dtype=dtype)
    mag = np.zeros((n, 3), dtype=np.longdouble)
    for i in range(2):
        for j in range(2):
            wij = w[0][i]*w[1][j]
            for k in range(2):
                wgt = (wij*w[2][k]).astype(dtype)
                cell = [first[:, 0] + i, first[:, 1] + j, first[:, 2] + k]
                for d in range(3):
                    def at(s):
                        c = list(cell)
                        c[d] = c[d] + s
                        return phi[c[0] % N, c[1] % N, c[2] % N]
                    f = c1*(at(1) - at(-1))
                    m = c1*(np.abs(at(1)) + np.abs(at(-1)))
                    if diff == 4:
                        f = f - c2*(at(2) - at(-2))
                        m = m + c2*(np.abs(at(2)) + np.abs(at(-2)))
                    value[:, d] += f*wgt
                    mag[:, d] += m.astype(np.longdouble)*wgt.astype(np.longdouble)
    if factor != 1:
        value = value*dtype(factor)
    expected = mom.astype(dtype) + value
    R = 3 if diff == 2 else 6
    bound = (abs(factor)*(R + 8)*U*mag + U*np.abs(value).astype(np.longdouble)
             + U*np.abs(expected).astype(np.longdouble))
    return expected, bound


def run_kick(mesh, pos, mom, diff, factor):
    import torch
    pos_d = torch.tensor(pos, device='cuda')
    mom_d = torch.tensor(mom, device='cuda')
    mesh.gather_kick(pos_d, mom_d, diff, factor)
    torch.cuda.synchronize()
    return mom_d.cpu().numpy()


def kick_both_orders(mesh, case, diff, field, pos, rng, factor, label):
    """the kick in the given memory order against the reference, and in a shuffled order: the
    same particle must receive the same bits"""
    n = pos.shape[0]
    mom = rng.normal(0, 1, (n, 3))
    got = run_kick(mesh, pos, mom, diff, factor)
    expected, bound = ref_kick(case, diff, pos, mom, field, factor)
    err = np.abs(got.astype(np.longdouble) - expected)
    ratio, worst = gi.worst_ratio(err.reshape(-1), bound.reshape(-1))
    assert ratio <= 1, (f'{label} diff={diff} {case}: particle {worst//3} component {worst % 3} '
                        f'at {pos[worst//3]!r} got {got.reshape(-1)[worst]!r} expected '
                        f'{float(expected.reshape(-1)[worst])!r}, error/bound {ratio:.3g}')
    perm = rng.permutation(n)          # row r of the shuffled arrays is particle perm[r]
    shuffled = run_kick(mesh, pos[perm], mom[perm], diff, factor)
    back = np.empty_like(shuffled)
    back[perm] = shuffled
    same = back.view(np.uint64) == got.view(np.uint64)
    assert same.all(), (f'{label} diff={diff} {case}: {np.count_nonzero(~same.all(1))} particles '
                        f'are kicked by different bits in shuffled memory order, first '
                        f'{int(np.flatnonzero(~same.all(1))[0])}')
    return ratio


# -- the particle sets of every scenario ---------------------------------------------------------
def kick_limit_cases(diff):
    """(label, gridsize, spans of the CIC cells, origin): boxes of span + W cells per axis at
    the limit of 4096 cells and one cell past it, and boxes over a whole axis"""
    W = 2 + 2*(diff//2)
    out = [('16x16x16 cells', 64, (16 - W,)*3, (50, 3, 60)),
           ('17x16x16 cells', 64, (17 - W, 16 - W, 16 - W), (50, 3, 60)),
           ('16x16x17 cells', 64, (16 - W, 16 - W, 17 - W), (3, 60, 50)),
           ('8x8x64 cells, the whole z axis', 64, (8 - W, 8 - W, 64 - W), (62, 7, 30)),
           ('9x8x64 cells', 64, (9 - W, 8 - W, 64 - W), (62, 7, 30)),
           ('8x8x65 cells', 64, (8 - W, 8 - W, 65 - W), (62, 7, 30))]
    if diff == 2:
        out += [('4x4x256 cells, the whole z axis', 256, (0, 0, 252), (254, 7, 100)),
                ('5x4x256 cells', 256, (1, 0, 252), (254, 7, 100)),
                ('4x4x257 cells', 256, (0, 0, 253), (254, 7, 100))]
    else:   # (6 x 6 cells at the least: 256 of them are past the limit; 6*6*113 = 4068)
        out += [('6x6x113 cells', 256, (0, 0, 107), (254, 7, 100)),
                ('6x6x114 cells', 256, (0, 0, 108), (254, 7, 100))]
    return out


def scenarios(diff, rng, gridsizes=(64, 256)):
    """-> (gridsize, case index, label, positions) of every scenario of one difference order"""
    for N in gridsizes:
        for ci, case in enumerate(kick_cases(N, diff)):
            if N == 64:
                for n in COUNTS:
                    yield N, ci, f'compact n={n}', gi.compact_set(case, +1, n, rng)
                    yield N, ci, f'spread n={n}', gi.spread_set(case, +1, n, rng)
                yield N, ci, 'seam', gi.seam_set(case, +1, rng)
                yield N, ci, 'one spot', np.tile(np.array([[0.2093, 0.7317, 0.9991]])*L_BOX,
                                                 (3*CHUNK, 1))
                yield N, ci, 'switch points', gi.switch_set(case, +1, rng)
            for label, N_case, spans, origin in kick_limit_cases(diff):
                if N_case == N:
                    yield N, ci, label, gi.limit_set(case, +1, spans, origin, rng)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [64, 256])
@pytest.mark.parametrize('diff', DIFFS)
def test_gather_kick_chunks(diff, N):
    """Every scenario at one gridsize (256: the limit cases along a long axis), cell- and
    vertex-centred: against the reference, and compact against shuffled memory order."""
    rng = np.random.default_rng(300 + diff + N)
    worst = {}
    with gi.meshes() as get:
        fields = {}
        for si, (_, ci, label, pos) in enumerate(scenarios(diff, rng, (N,))):
            case = kick_cases(N, diff)[ci]
            mesh = get(case)
            if id(mesh) not in fields:
                fields[id(mesh)] = gi.random_field(mesh, N, rng)
            ratio = kick_both_orders(mesh, case, diff, fields[id(mesh)], pos, rng,
                                     FACTORS[si % 2], label)
            worst[label] = max(worst.get(label, 0.0), ratio)
    for label, ratio in worst.items():
        print(f'\ngather-kick diff={diff} N={N} {label}: error/bound {ratio:.3f}')


def test_limit_sets_are_at_the_limit():
    """the limit cases are what their labels say: span + W cells per axis"""
    for diff in DIFFS:
        W = 2 + 2*(diff//2)
        for label, N, spans, _ in kick_limit_cases(diff):
            e = [int(v) for v in label.split()[0].split('x')]
            assert [s + W for s in spans] == e, (diff, label)
            inside = e[0]*e[1]*e[2] <= 4096 and max(e) <= N
            assert inside == (label.endswith('axis') or label in ('16x16x16 cells',
                                                                  '6x6x113 cells')), label


@pytest.mark.parametrize('diff', DIFFS)
def test_reference_in_kernel_order_is_inside_the_bound(diff):
    """No GPU: the formulas in float64, in the kernel's order of operations, against the
    longdouble reference on every scenario at gridsize 64 — the bound holds for a correct
    kernel."""
    rng = np.random.default_rng(400 + diff)
    field = rng.normal(0, 1, (64, 64, 64))
    worst = 0.0
    for _, ci, label, pos in scenarios(diff, rng, (64,)):
        case = kick_cases(64, diff)[ci]
        mom = rng.normal(0, 1, pos.shape)
        for factor in FACTORS:
            expected, bound = ref_kick(case, diff, pos, mom, field, factor)
            emulated, _ = ref_kick(case, diff, pos, mom, field, factor, dtype=np.float64)
            err = np.abs(emulated.astype(np.longdouble) - expected)
            ratio, at = gi.worst_ratio(err.reshape(-1), bound.reshape(-1))
            assert ratio <= 1, (label, case, factor, at, ratio)
            worst = max(worst, ratio)
    print(f'\ngather-kick diff={diff} float64 in kernel order: error/bound {worst:.3f}')
