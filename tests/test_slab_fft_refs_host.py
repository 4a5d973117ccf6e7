"""The references of the slab transform tests (tests/slab_fft_refs.py) checked on the CPU:
they agree with each other and with numpy's rfftn of the whole field, the stored deviation of
the float64 k-space factor from its long-double value is what a new measurement gives, and every
(shape, pass) of the shape table takes, at 256 compute units, the kernel form the table names
— asked of concept_amd/csrc/cg_fft_plan.h through tests/fft_plan_print.cpp, with the pencil
maps fft_dist builds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import slab_fft_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'concept_amd', 'csrc')
SENT = 1e150*(1 + 1j)


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    cxx = shutil.which('g++') or next(
        (p for p in ('/opt/rocm/llvm/bin/clang++',) if os.path.exists(p)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('slab_plan')/'fft_plan_print')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I' + CSRC,
                    os.path.join(HERE, 'fft_plan_print.cpp'), '-o', exe], check=True)

    def ask(*requests):
        text = '\n'.join(' '.join(str(v) for v in r) for r in requests) + '\n'
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True)
        lines = [ln.split() for ln in out.stdout.decode().splitlines()]
        assert len(lines) == len(requests) and all(ln[0] == r[0] for ln, r in zip(lines, requests))
        return [ln[1:] for ln in lines]
    return ask


# ---------------------------------------------------------------------------------------------
# 1. ZY per slab -> exchange by hand -> X  ==  rfftn of the whole field, and the way back
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pieces', ['whole', 'two pieces'])
@pytest.mark.parametrize('P,N', R.HOST_CHAIN)
def test_references_chain_equals_rfftn(P, N, pieces):
    g = R.geometry(N, P)
    field = np.random.default_rng(100*P + N).normal(0, 1, (N, N, N))
    full = np.fft.rfftn(field)
    tol = 1e-13*np.sqrt((np.abs(full)**2).mean())*np.log2(N)**2

    def swap(send):
        recv = [np.full_like(s, SENT) for s in send]
        if pieces == 'whole':
            R.exchange(send, recv)
        else:  # as Comm.all_to_all_layers: two layer ranges, the later one first
            h = g.nxl//2
            R.exchange(send, recv, h, g.nxl - h)
            R.exchange(send, recv, 0, h)
        return recv

    send = [R.pack_blocked(R.zy_forward(field[r*g.nxl:(r + 1)*g.nxl]), g, SENT) for r in range(P)]
    for r in range(P):   # pack and unpack are inverses; everything else keeps the fill
        assert np.array_equal(R.unpack_blocked(send[r], g),
                              R.zy_forward(field[r*g.nxl:(r + 1)*g.nxl]))
        assert (send[r][~R.live_blocked(g)] == SENT).all()
    recv = swap(send)
    back = []
    for r in range(P):
        four = R.fourier_view(recv[r], g)
        assert four.shape == (N, g.JB + 1, g.cp)
        assert (four[:, g.JB] == SENT).all() and (four[:, :, g.nk:] == SENT).all()
        X = R.x_forward(four[:, :g.JB, :g.nk])
        assert np.abs(X - R.rfftn_slab(field, g, r)).max() <= tol
        assert np.abs(X - full[:, r*g.JB:(r + 1)*g.JB]).max() <= tol
        out = np.full((P, g.nxl, g.JB + 1, g.cp), SENT)
        R.fourier_view(out, g)[:, :g.JB, :g.nk] = R.x_backward(X)
        back.append(out)
    home = swap(back)
    for r in range(P):
        real = R.zy_backward(R.unpack_blocked(home[r], g), N)
        own = field[r*g.nxl:(r + 1)*g.nxl]
        assert np.abs(real - float(N)**3*own).max() <= 1e-13*N**3*np.abs(field).max()


def test_exchange_moves_only_its_layers():
    g = R.geometry(16, 4)
    rng = np.random.default_rng(3)
    send = [rng.normal(0, 1, (4, g.nxl, g.JB + 1, g.cp)) + 0j for _ in range(4)]
    recv = [np.full_like(s, SENT) for s in send]
    R.exchange(send, recv, 1, 2)
    for q in range(4):
        for r in range(4):
            assert np.array_equal(recv[q][r, 1:3], send[r][q, 1:3])
        assert (recv[q][:, 0] == SENT).all() and (recv[q][:, 3] == SENT).all()


def test_layer_pieces_cover_the_owned_layers():
    for s in R.SHAPES + R.ROCFFT_SHAPES:
        nxl = s.N//s.P
        seen = sorted(l for a, n in R.layer_pieces(nxl) for l in range(a, a + n))
        assert seen == list(range(nxl)) and all(n >= 1 for _, n in R.layer_pieces(nxl))


# ---------------------------------------------------------------------------------------------
# 2. the k-space factor: float64 restatement against long double
# ---------------------------------------------------------------------------------------------
def test_factor_restates_the_header():
    """spot values by hand: the nullified planes, the symmetry in (a, b), and one mode written
    out operation by operation"""
    N = 16
    n, s = R.kspace_tables(N, np.float64)
    a, b, kk = 3, 13, 5      # ka = 3, kb = -3
    q = ((n[a]*n[b])*n[kk])/((s[a]*s[b])*s[kk])
    k2 = 9 + 9 + 25
    want = (q**4)*((R.C_TEST/k2)*np.exp(k2*R.E_TEST))
    assert R.kspace_factor(N, a, b, kk, 4, R.C_TEST, 1, R.E_TEST) == want
    assert R.kspace_factor(N, b, a, kk, 4, R.C_TEST, 1, R.E_TEST) == want
    assert R.kspace_factor(N, a, b, kk, 0, R.C_TEST, 0, R.E_TEST) == R.C_TEST/k2
    for dead in ((8, 1, 1), (1, 8, 1), (1, 1, 8), (0, 0, 0)):
        for dtype in (np.float64, R.LD):
            assert R.kspace_factor(N, *dead, 2, R.C_TEST, 1, R.E_TEST, dtype) == 0
    assert R.kspace_factor(N, 0, 0, 1, 2, R.C_TEST, 0, R.E_TEST) != 0


@pytest.mark.parametrize('N,P,rank', [(16, 4, 0), (16, 2, 1), (64, 8, 4), (36, 3, 1), (48, 2, 1)])
def test_separable_long_double_factor(N, P, rank):
    """slab_factor_ld (what the GPU tests compare with at size) is the operation-order long-double
    form up to long double's own rounding: a dozen operations of 2**-64 each"""
    g = R.geometry(N, P)
    for order in R.ORDERS:
        for lr in R.LONG_RANGES:
            fast = R.slab_factor_ld(g, rank, order, R.C_TEST, lr, R.E_TEST)
            slow = R.slab_factor(g, rank, order, R.C_TEST, lr, R.E_TEST, R.LD)
            assert fast.dtype == slow.dtype == R.LD and fast.shape == (N, g.JB, g.nk)
            assert np.array_equal(fast == 0, slow == 0)
            assert (np.abs(fast - slow) <= 2.0**-58*np.abs(slow)).all()


def _sample_rows(g, rank):
    """every row of the small slabs; of those from 256 points on the first two, the middle and
    the last, and any row next to or on a nullified plane (long-double numpy over all
    N*JB*(N/2 + 1) modes of a 1024 slab takes minutes)"""
    if g.N < 256:
        return None
    rows = {0, 1, g.JB//2, g.JB - 1}
    return sorted(rows)


def test_factor_deviation_constants():
    """the stored table is what is measured: nothing beyond it, and the worst within 10 % of it
    (sampled rows at the large sizes can only find less than the full sweep that set it)"""
    worst = R.measure_factor_dev(R.all_cases(), _sample_rows)
    print('measured worst deviation per deconv_order [eps*|F|]:',
          {o: round(v, 3) for o, v in worst.items()})
    assert sorted(worst) == list(R.ORDERS) == sorted(R.FACTOR_DEV_EPS)
    for order in R.ORDERS:
        assert 0.9*R.FACTOR_DEV_EPS[order] <= worst[order] <= R.FACTOR_DEV_EPS[order], (
            order, worst[order], R.FACTOR_DEV_EPS[order])


# ---------------------------------------------------------------------------------------------
# 3. every (shape, pass) reaches the form the table names at 256 compute units
# ---------------------------------------------------------------------------------------------
def pass_requests(s, nouter_y):
    g = R.geometry(s.N, s.P)
    logn, sh = s.N.bit_length() - 1, g.JB.bit_length() - 1
    assert 1 << logn == s.N and 1 << sh == g.JB
    split = 1 if s.split is None else s.split
    head = ('choice', logn)
    tail = (s.N, g.pad, R.NCU, split)
    y, blocked, x = (g.cp, 31), (g.cp, sh), ((g.JB + 1)*g.cp, 31)
    return {
        'y_fwd': head + (0,) + tail + (nouter_y,) + y + blocked,
        'y_inv': head + (1,) + tail + (nouter_y,) + blocked + y,
        'x_fwd': head + (0,) + tail + (g.JB,) + x + x,
        'x_inv': head + (1,) + tail + (g.JB,) + x + x,
        'x_fused': head + (2,) + tail + (g.JB,) + x + x,
    }


@pytest.mark.parametrize('s', R.SHAPES, ids=lambda s: f'{s.N}-{s.P}-split{s.split}')
def test_shape_reaches_its_forms(plans, s):
    g = R.geometry(s.N, s.P)
    out = [int(v) for v in plans(('chunk', s.N, g.ny, g.pad, R.NCU, g.nxl))[0]]
    begin = out[4:]
    chunks = tuple(b - a for a, b in zip(begin, begin[1:]))
    assert chunks == s.chunks
    for nouter_y in sorted(set(chunks)):
        req = pass_requests(s, nouter_y)
        got = {name: ans[0] for name, ans in zip(req, plans(*req.values()))}
        assert got == s.forms, (s, nouter_y)
    # the table holds what it is there for
    forms = {(t.N, t.P, t.split): t.forms for t in R.SHAPES}
    assert forms[256, 4, None]['x_fused'] == 'Persistent'
    assert forms[512, 8, 2]['y_fwd'] == forms[512, 16, 2]['y_inv'] == 'SplitBlocked'
    assert forms[512, 32, 2]['y_fwd'] == 'Plain'
    assert forms[1024, 16, None]['y_fwd'] == 'SplitBlocked' and len(s.chunks) in (1, 2)
