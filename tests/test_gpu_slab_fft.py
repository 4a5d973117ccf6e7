"""The passes of the x-slab transform one by one, in ONE process: fft_dist (cg_fft.hip) and
cgk_libfft_dist with k_dist_rows (cg_rocfft.hip) through the raw entries
cg_dist_fft_forward[_layers], cg_dist_fft_x, cg_dist_fft_xsolve, cg_dist_fft_backward[_layers]
and cg_poisson_kernel on a bound Fourier slab, each against the plain numpy references of
tests/slab_fft_refs.py.

A slab's passes are local operations on one context, so PotentialMesh(N, L, nprocs=P, rank=r)
without a comm (the pattern of test_gpu_slab_handover.py) with caller-owned buffers of
transpose_doubles doubles runs a pass at production size without the other P - 1 slabs.  The
shapes, ranks and switches are the table of slab_fft_refs.py (SHAPES, ROCFFT_SHAPES); what form
of kernel each pass takes there at 256 compute units is asserted on the CPU by
test_slab_fft_refs_host.py.  This module prints the device's compute-unit count and a case whose
table entry names another form than Plain fails, saying so, when the count is not 256 (it would
silently test another kernel).  Every power-of-two shape up to 256 runs twice, hand-written and
with CONCEPT_GPU_FFT=rocfft: same contract, same reference.

The mesh, the stage buffer and the Fourier buffer hold the finite sentinel 1e150 before data
goes in (finite: the split forms read and write the row padding).  What a pass may not touch
must keep it bit for bit: row JB of every (q, layer) block, the ghost layers of the mesh, the
layers a _layers call was not given, and the columns kk > N/2 wherever the store is guarded
with kk < nk (k_fft_strided, k_dist_rows, k_kspace); the persistent and split forms and rocFFT's
x plan write whole rows or 8-wide tiles, there the columns must stay finite.

Bars (none is made from what the code under test gives):
  forward passes   1e-13*rms(ref)*log2(N)**2, round trips 1e-13*N**d*max: those of
                   test_handwritten_fft_vs_numpy_and_rocfft
  xsolve           1e-12*max|ref| against N*ifft(F*fft(x)) with the long-double F (rounded to
                   double before the product: 1 eps per mode); 1e-13*max against x_forward +
                   cg_poisson_kernel + x_backward of the same context
  kernel alone     per mode 2*FACTOR_DEV_EPS[order]*eps*|F|*|A| in long double (the factor 2 as
                   in test_gpu_general_kernels.py: repeated multiplication instead of pow, the
                   device's exp)
  _layers          bit equality with the one-call form on the hand-written backend, in every
                   layer whose piece runs the same kernel form as the one call.  A pencil's
                   arithmetic does not depend on its tile only within a form: under the split
                   forms a piece of fewer than 2*256 tiles is given the whole-pencil kernel
                   (strided_choice), so at 512 points with the switch at 2 layer 0 (P = 8) or
                   the layers 0..15 (P = 16), and at 1024 layer 0, differ from the one call by
                   rounding — measured 4.6e-13, 5.1e-13 and 1.0e-12 against bars of 4.1e-9 and
                   1.0e-8.  Those layers, known from the plan and not from the output, get the
                   forward bar against the one call and against numpy.

What these tests found: with CONCEPT_GPU_FFT=rocfft the slabs of 16 and 64 points stopped in
plans_2d (then dist_plans_2d) — rocfft_plan_create of the in-place 2-D real inverse plan answers
rocfft_status_failure for 16 x 16 and 64 x 64 in rows of N + 16 doubles (256 and 48 with
N + 16, 24 and 36 with N + 2 are planned both ways).  cgk_libfft_dist now transforms such layers
with two 1-D plans per layer (layers_1d); the rocFFT cases at 16 and 64 run that path.

Zeros: the planes b == N/2 and kk == N/2 are whole pencils of the x pass and come out of xsolve
as exact zeros, directly and after a forward pass of the result (`== 0` without a tolerance:
the fused passes multiply by the factor 0.0, which IEEE signs -0.0 for a negative operand, so
the sign bit is not asked).  The single modes a == N/2 and
the origin lie inside a pencil: a transform of rounded data returns them as rounding noise, not
as 0.0, so after the forward pass they are held to the forward bar around zero; by bits they are
checked where they are written as zeros, in the stand-alone kernel.

Left out on purpose: 2048 points on slabs — one slab that reaches SplitBlocked there (JB >= 128)
costs 9 GB and a reference of 128 layers of 2048^2; its even/odd kernel is covered on one domain
by test_fft_2048_known_answer — and the transports themselves (gloo, RCCL, the piece pipeline of
mesh.py), which stay with test_gpu_distributed.py: the exchange here is torch indexing."""
import contextlib

import numpy as np
import pytest

import slab_fft_refs as R

pytestmark = pytest.mark.gpu

BOX = 64.0
FSENT = 1e150
C, E = R.C_TEST, R.E_TEST


def _cases():
    out = []
    for s in R.SHAPES:
        for r in s.ranks:
            out.append((s, r, 'own'))
            if s.N <= 256:
                out.append((s, r, 'rocfft'))
    return out + [(s, r, 'rocfft') for s in R.ROCFFT_SHAPES for r in s.ranks]


def _case_id(c):
    s, r, backend = c
    return f'{s.N}-P{s.P}-r{r}-split{s.split}-{backend}'


CASES = _cases()
SOLVES = [(o, lr) for o in R.ORDERS for lr in R.LONG_RANGES]
case_param = pytest.mark.parametrize('case', CASES, ids=_case_id)
solve_param = pytest.mark.parametrize('order,lr', SOLVES)


class Gpu:
    """the module's handles and the references shared among its tests (computed once, never
    written again)"""

    def __init__(self, torch):
        from concept_amd import lib
        from concept_amd.mesh import PotentialMesh
        self.torch, self.lib, self.L, self.Mesh = torch, lib, lib.raw(), PotentialMesh
        self.check, self.ptr = lib.check, lib._ptr
        self.ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        self._fields, self._rows = {}, {}

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def devc(self, a):
        """a complex numpy array as a complex tensor on the device"""
        return self.dev(np.ascontiguousarray(a, dtype=np.complex128))

    def field(self, N, P, rank):
        """(real[nxl][N][N], its ZY transform complex[nxl][N][nk]) of a slab"""
        key = (N, P, rank)
        if key not in self._fields:
            g = R.geometry(N, P)
            gen = self.torch.Generator(device='cuda').manual_seed(1000*N + 10*P + rank)
            f = self.torch.randn((g.nxl, N, N), dtype=self.torch.float64, device='cuda',
                                 generator=gen).cpu().numpy()
            self._fields[key] = (f, R.zy_forward(f))
        return self._fields[key]

    def rows(self, N, JB):
        """random complex[N][JB][nk] and its forward and backward x transforms"""
        key = (N, JB)
        if key not in self._rows:
            gen = self.torch.Generator(device='cuda').manual_seed(7*N + JB)
            x = self.torch.randn((N, JB, N//2 + 1, 2), dtype=self.torch.float64, device='cuda',
                                 generator=gen).cpu().numpy().view(np.complex128)[..., 0]
            self._rows[key] = (x, R.x_forward(x), R.x_backward(x))
        return self._rows[key]


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    g = Gpu(torch)
    print(f'\ntest_gpu_slab_fft: the device has {g.ncu} compute units '
          f'(the forms of the shape table are those of {R.NCU})')
    return g


class Slab:
    """one slab context of rank r among P with caller-owned stage and Fourier buffers"""

    def __init__(self, gpu, N, P, rank):
        self.gpu, self.g, self.rank = gpu, R.geometry(N, P), rank
        self.m = gpu.Mesh(N, BOX, nprocs=P, rank=rank)
        g, m = self.g, self.m
        assert (m.nxl, m.pad, m.layer_doubles, m.transpose_doubles) == (
            g.nxl, g.pad, g.ny*g.pad, 2*N*(g.JB + 1)*g.cp)
        self.G = m.ghost_layers
        self.stage, self.four = self.buffer(), self.buffer()

    def close(self):
        self.m.close()

    def buffer(self):
        return self.gpu.torch.full((self.m.transpose_doubles,), FSENT,
                                   dtype=self.gpu.torch.float64, device='cuda')

    # the mesh: double[nxl + 2 G][ny][pad]
    def fill_mesh(self, field=None):
        """the sentinel in every double of the local mesh, `field` in the owned cells"""
        g, t = self.g, self.gpu.torch
        n = g.nxl + 2*self.G
        whole = t.full((n, g.ny, g.pad), FSENT, dtype=t.float64, device='cuda')
        if field is not None:
            whole[self.G:self.G + g.nxl, :g.N, :g.N] = field
        self.m.layers_write(-self.G, n, whole)

    def read_mesh(self):
        g, t = self.g, self.gpu.torch
        n = g.nxl + 2*self.G
        out = t.empty((n, g.ny, g.pad), dtype=t.float64, device='cuda')
        self.m.layers_read(-self.G, n, out)
        return out

    def ghosts_kept(self, mesh):
        return bool((mesh[:self.G] == FSENT).all()) and bool((mesh[self.G + self.g.nxl:] == FSENT).all())

    # views of a buffer
    def blocked(self, buf):
        g = self.g
        return buf.view(g.P, g.nxl, g.JB + 1, g.cp, 2)

    def fourier(self, buf):
        g = self.g
        return buf.view(g.N, g.JB + 1, g.cp, 2)

    def live(self, view):
        """the live elements of a blocked or Fourier view, complex"""
        return self.gpu.torch.view_as_complex(view[..., :self.g.JB, :self.g.nk, :])

    def load_rows(self, buf, x):
        """complex[N][JB][nk] into the live part of a Fourier buffer, the sentinel elsewhere"""
        buf.fill_(FSENT)
        self.live(self.fourier(buf)).copy_(self.gpu.devc(x))

    def dead_kept(self, view, guarded):
        """row JB keeps the sentinel; the columns kk > N/2 keep it where the store is guarded,
        and stay finite elsewhere"""
        g, t = self.g, self.gpu.torch
        assert bool((view[..., g.JB, :, :] == FSENT).all()), 'row JB was written'
        cols = view[..., :g.JB, g.nk:, :]
        if guarded:
            assert bool((cols == FSENT).all()), 'a column kk > N/2 was written'
        else:
            assert bool(t.isfinite(cols).all()), 'a column kk > N/2 is not finite'

    # the raw entries
    def call(self, name, *args):
        self.gpu.check(getattr(self.gpu.L, name)(self.m._ctx, *args))

    def zy_forward(self, buf, piece=None):
        if piece is None:
            self.call('cg_dist_fft_forward', self.gpu.ptr(buf))
        else:
            self.call('cg_dist_fft_forward_layers', self.gpu.ptr(buf), int(piece[0]), int(piece[1]))

    def zy_backward(self, buf, piece=None):
        if piece is None:
            self.call('cg_dist_fft_backward', self.gpu.ptr(buf))
        else:
            self.call('cg_dist_fft_backward_layers', self.gpu.ptr(buf), int(piece[0]), int(piece[1]))

    def x(self, buf, inverse):
        self.call('cg_dist_fft_x', self.gpu.ptr(buf), int(inverse))

    def xsolve(self, buf, order, lr):
        self.call('cg_dist_fft_xsolve', self.gpu.ptr(buf), int(order), float(C), int(lr), float(E))

    def kernel(self, buf, order, lr):
        self.call('cg_dist_bind_fourier', self.gpu.ptr(buf))
        self.call('cg_poisson_kernel', int(order), float(C), int(lr), float(E))


def set_backend(gpu, monkeypatch, N, split, backend, forms):
    pow2 = N & (N - 1) == 0
    if backend == 'rocfft' and pow2:
        monkeypatch.setenv('CONCEPT_GPU_FFT', 'rocfft')
    else:
        assert backend == ('own' if pow2 else 'rocfft')
        monkeypatch.delenv('CONCEPT_GPU_FFT', raising=False)
    monkeypatch.setenv('CONCEPT_GPU_FFT_SPLIT', str(1 if split is None else split))
    if backend == 'own' and any(f != 'Plain' for f in forms.values()):
        assert gpu.ncu == R.NCU, (
            f'this case is there for the forms {forms} at {R.NCU} compute units; the device has '
            f'{gpu.ncu}, where strided_choice may pick others: nothing was tested')


@contextlib.contextmanager
def slab_of(gpu, monkeypatch, case):
    s, rank, backend = case
    set_backend(gpu, monkeypatch, s.N, s.split, backend, s.forms or {})
    c = Slab(gpu, s.N, s.P, rank)
    try:
        yield c
    finally:
        c.close()


def guarded(case, which):
    """does the store of pass `which` ('y' or 'x') leave the columns kk > N/2 alone?  y:
    k_fft_strided and k_dist_rows do, the split form writes whole tiles.  x: only k_fft_strided;
    the persistent and split forms write whole tiles and rocFFT's plan transforms JB*cp columns"""
    s, _, backend = case
    if backend == 'rocfft':
        return which == 'y'
    return s.forms['y_fwd' if which == 'y' else 'x_fwd'] == 'Plain'


def rms(a):
    return float(np.sqrt((np.abs(a)**2).mean()))


def maxerr(gpu, got, ref):
    return float((got - gpu.devc(ref)).abs().max())


def same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def fwd_bar(ref, N):
    return 1e-13*rms(ref)*np.log2(N)**2


# ---------------------------------------------------------------------------------------------
# z and y passes: mesh -> blocked buffer and back
# ---------------------------------------------------------------------------------------------
@case_param
def test_zy_forward(gpu, monkeypatch, case):
    s, rank, _ = case
    field, Y = gpu.field(s.N, s.P, rank)
    with slab_of(gpu, monkeypatch, case) as c:
        c.fill_mesh(gpu.dev(field))
        c.zy_forward(c.stage)
        B = c.blocked(c.stage)
        err, bar = maxerr(gpu, c.live(B), R.blocked_live(Y, c.g)), fwd_bar(Y, s.N)
        print(f'zy_forward {_case_id(case)}: max deviation {err:.3e}, bar {bar:.3e}')
        assert err <= bar
        c.dead_kept(B, guarded(case, 'y'))
        assert c.ghosts_kept(c.read_mesh()), 'a ghost layer of the mesh was written'


@case_param
def test_zy_forward_layers(gpu, monkeypatch, case):
    s, rank, backend = case
    torch = gpu.torch
    field, Y = gpu.field(s.N, s.P, rank)
    with slab_of(gpu, monkeypatch, case) as c:
        g = c.g
        f = gpu.dev(field)
        c.fill_mesh(f)
        c.zy_forward(c.stage)
        c.fill_mesh(f)
        B, done = c.blocked(c.four), np.zeros(g.nxl, dtype=bool)
        for l0, nl in R.layer_pieces(g.nxl):
            c.zy_forward(c.four, (l0, nl))
            done[l0:l0 + nl] = True
            rest = gpu.dev(np.flatnonzero(~done))
            assert bool((B[:, rest] == FSENT).all()), f'piece {(l0, nl)} wrote other layers'
            assert not bool((c.live(B)[:, l0:l0 + nl] == complex(FSENT, FSENT)).any()), (
                f'piece {(l0, nl)} left its own layers unwritten')
            c.dead_kept(B, guarded(case, 'y'))
        assert done.all()
        one, pieces = c.live(c.blocked(c.stage)), c.live(B)
        if backend == 'own':
            # a pencil's arithmetic does not depend on its tile — within one kernel form.  A
            # piece of fewer than 2*ncu tiles of a shape whose one-call pass splits is given
            # the whole-pencil kernel by strided_choice (known from the plan, not from the
            # output): its layers hold another algorithm's rounding and get the forward bar
            nkb = -(-g.nk//8)
            same_form = np.zeros(g.nxl, dtype=bool)
            for l0, nl in R.layer_pieces(g.nxl):
                same_form[l0:l0 + nl] = s.forms['y_fwd'] == 'Plain' or nl*nkb >= 2*R.NCU
            keep, other = gpu.dev(np.flatnonzero(same_form)), gpu.dev(np.flatnonzero(~same_form))
            a, b = torch.view_as_real(one), torch.view_as_real(pieces)
            differ = (a[:, keep] != b[:, keep]).any(-1)
            assert same_bits(torch, a[:, keep], b[:, keep]), (
                f'{int(differ.sum())} elements differ from the one-call form in layers that '
                f'take the same kernel, by at most {float((one - pieces)[:, keep].abs().max()):.3e}')
            if (~same_form).any():
                err = float((one - pieces)[:, other].abs().max())
                print(f'layers {np.flatnonzero(~same_form).tolist()} in the other form: max '
                      f'deviation {err:.3e}, bar {fwd_bar(Y, s.N):.3e}')
                assert err <= fwd_bar(Y, s.N)
                assert maxerr(gpu, pieces, R.blocked_live(Y, g)) <= fwd_bar(Y, s.N)
        else:                 # rocFFT's plans differ by layer count
            assert float((one - pieces).abs().max()) <= fwd_bar(Y, s.N)
        assert c.ghosts_kept(c.read_mesh())


@case_param
def test_zy_backward_and_layers(gpu, monkeypatch, case):
    s, rank, _ = case
    torch = gpu.torch
    field, Y = gpu.field(s.N, s.P, rank)
    N = s.N
    bar = 1e-13*N*N*float(np.abs(field).max())
    with slab_of(gpu, monkeypatch, case) as c:
        g, G = c.g, c.G
        c.stage.copy_(gpu.dev(R.pack_blocked(Y, g, complex(FSENT, FSENT)).view(np.float64).reshape(-1)))
        before = c.stage.clone()
        want = gpu.dev(field)*float(N*N)
        for pieces in (None, R.layer_pieces(g.nxl)):
            c.fill_mesh()
            done = np.zeros(g.nxl, dtype=bool)
            for piece in [None] if pieces is None else pieces:
                c.zy_backward(c.stage, piece)
                if piece is not None:
                    done[piece[0]:piece[0] + piece[1]] = True
                    rest = gpu.dev(G + np.flatnonzero(~done))
                    assert bool((c.read_mesh()[rest] == FSENT).all()), (
                        f'piece {piece} wrote other layers')
            mesh = c.read_mesh()
            err = float((mesh[G:G + g.nxl, :N, :N] - want).abs().max())
            print(f'zy_backward {_case_id(case)} {"layers" if pieces else "whole"}: '
                  f'max deviation {err:.3e}, bar {bar:.3e}')
            assert err <= bar
            assert c.ghosts_kept(mesh), 'a ghost layer of the mesh was written'
            assert same_bits(torch, c.stage, before), 'the stage buffer was written'


# ---------------------------------------------------------------------------------------------
# x passes on the Fourier slab
# ---------------------------------------------------------------------------------------------
@case_param
def test_x_forward_backward(gpu, monkeypatch, case):
    s, rank, _ = case
    N = s.N
    with slab_of(gpu, monkeypatch, case) as c:
        x, xf, xb = gpu.rows(N, c.g.JB)
        F = c.fourier(c.four)
        c.load_rows(c.four, x)
        c.x(c.four, 0)
        err, bar = maxerr(gpu, c.live(F), xf), fwd_bar(xf, N)
        print(f'x_forward {_case_id(case)}: max deviation {err:.3e}, bar {bar:.3e}')
        assert err <= bar
        c.dead_kept(F, guarded(case, 'x'))
        c.x(c.four, 1)    # forward then backward: N times the identity
        err, bar = maxerr(gpu, c.live(F), N*x), 1e-13*N*float(np.abs(x).max())
        print(f'x round trip: max deviation {err:.3e}, bar {bar:.3e}')
        assert err <= bar
        c.dead_kept(F, guarded(case, 'x'))
        c.load_rows(c.four, x)
        c.x(c.four, 1)
        err, bar = maxerr(gpu, c.live(F), xb), fwd_bar(xb, N)
        print(f'x_backward: max deviation {err:.3e}, bar {bar:.3e}')
        assert err <= bar
        c.dead_kept(F, guarded(case, 'x'))


@solve_param
@case_param
def test_xsolve(gpu, monkeypatch, case, order, lr):
    s, rank, _ = case
    N, nyq = s.N, s.N//2
    torch = gpu.torch
    with slab_of(gpu, monkeypatch, case) as c:
        g = c.g
        x, xf, _ = gpu.rows(N, g.JB)
        Fk = R.slab_factor_ld(g, rank, order, C, lr, E).astype(np.float64)
        spectrum = Fk*xf
        ref = R.x_backward(spectrum)
        top = float(np.abs(ref).max())
        # fused
        c.load_rows(c.four, x)
        c.xsolve(c.four, order, lr)
        F = c.fourier(c.four)
        got = c.live(F)
        err = maxerr(gpu, got, ref)
        print(f'xsolve {_case_id(case)} order {order} long_range {lr}: max deviation {err:.3e}, '
              f'bar {1e-12*top:.3e}')
        assert err <= 1e-12*top
        c.dead_kept(F, guarded(case, 'x'))
        # the same in three steps on the same context
        c.load_rows(c.stage, x)
        c.x(c.stage, 0)
        c.kernel(c.stage, order, lr)
        c.x(c.stage, 1)
        steps = c.live(c.fourier(c.stage))
        err = float((got - steps).abs().max())
        print(f'fused against three steps: max deviation {err:.3e}, bar {1e-13*top:.3e}')
        assert err <= 1e-13*float(steps.abs().max())
        # the nullified planes are whole pencils: 0.0 by bits, before and after a forward pass
        jl = nyq - rank*g.JB
        for when in ('result', 'forward pass of the result'):
            # (exact zeros of either sign: the fused pass multiplies by the factor 0.0, and
            # IEEE gives -0.0 for a negative operand; nothing else passes `== 0`)
            r = torch.view_as_real(c.live(F))
            assert bool((r[:, :, nyq] == 0).all()), f'{when}: plane kk == N/2 is not 0.0'
            if 0 <= jl < g.JB:
                assert bool((r[:, jl] == 0).all()), f'{when}: row b == N/2 is not 0.0'
            if when == 'result':
                c.x(c.four, 0)
        # ... the single modes a == N/2 and the origin come back as rounding noise around zero
        back = c.live(F)
        bar = fwd_bar(N*spectrum, N)
        assert float(back[nyq].abs().max()) <= bar, 'plane a == N/2 after the forward pass'
        if rank == 0:
            assert abs(complex(back[0, 0, 0])) <= bar, 'the origin after the forward pass'
        assert maxerr(gpu, back, N*spectrum) <= bar


@solve_param
@case_param
def test_kernel_alone(gpu, monkeypatch, case, order, lr):
    s, rank, _ = case
    N = s.N
    with slab_of(gpu, monkeypatch, case) as c:
        g = c.g
        A = gpu.rows(N, g.JB)[0]
        c.load_rows(c.four, A)
        c.kernel(c.four, order, lr)
        F = c.fourier(c.four)
        c.dead_kept(F, True)
        got = c.live(F).cpu().numpy()
    Fk = R.slab_factor_ld(g, rank, order, C, lr, E)
    dead = Fk == 0
    assert dead[N//2].all() and dead[:, :, N//2].all()
    assert not got[dead].view(np.int64).any(), 'a nullified mode is not 0.0'
    err = np.abs(got.astype(R.CLD) - Fk*A.astype(R.CLD)).astype(np.float64)
    bar = 2*R.FACTOR_DEV_EPS[order]*R.EPS*np.abs(Fk).astype(np.float64)*np.abs(A)
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    print(f'kernel alone {_case_id(case)} order {order} long_range {lr}: worst mode '
          f'[a, jl, kk] = {worst}: {err[worst]:.3e}, bar {bar[worst]:.3e}')
    assert (err <= bar).all(), (worst, err[worst], bar[worst])


# ---------------------------------------------------------------------------------------------
# all P slabs side by side: ZY forward, exchange by hand, xsolve, exchange back, ZY backward
# ---------------------------------------------------------------------------------------------
def swap(torch, slabs, src, dst, pieces):
    """the all-to-all on the device: block q of rank r's `src` buffer -> block r of rank q's
    `dst` buffer, whole or in two layer ranges (the later one first)"""
    nxl = slabs[0].g.nxl
    ranges = [(0, nxl)] if pieces == 'whole' else [(nxl//2, nxl), (0, nxl//2)]
    for lo, hi in ranges:
        for r, a in enumerate(slabs):
            for q, b in enumerate(slabs):
                b.blocked(getattr(b, dst))[r, lo:hi] = a.blocked(getattr(a, src))[q, lo:hi]


@pytest.mark.parametrize('pieces', ['whole', 'two pieces'])
@pytest.mark.parametrize('P,N', R.CHAIN)
def test_chain_of_all_slabs(gpu, monkeypatch, P, N, pieces):
    torch = gpu.torch
    order, lr = 2, 1
    pow2 = N & (N - 1) == 0
    set_backend(gpu, monkeypatch, N, None, 'own' if pow2 else 'rocfft', {})
    g = R.geometry(N, P)
    field = np.random.default_rng(31*N + P).normal(0, 1, (N, N, N))
    full = np.fft.rfftn(field)
    single = gpu.Mesh(N, BOX)
    slabs = [Slab(gpu, N, P, r) for r in range(P)]
    try:
        whole = torch.zeros((N, g.ny, g.pad), dtype=torch.float64, device='cuda')
        whole[:, :N, :N] = gpu.dev(field)
        single.layers_write(0, N, whole)
        single.poisson_solve(order, C, bool(lr), E)
        single.layers_read(0, N, whole)
        phi = whole[:, :N, :N]
        for r, c in enumerate(slabs):
            c.fill_mesh(gpu.dev(field[r*g.nxl:(r + 1)*g.nxl]))
            c.zy_forward(c.stage)
        swap(torch, slabs, 'stage', 'four', pieces)
        for r, c in enumerate(slabs):
            c.dead_kept(c.fourier(c.four), True)   # the exchange moved whole rows of sentinels
            probe = c.four.clone()
            c.x(probe, 0)
            err = maxerr(gpu, c.live(c.fourier(probe)), R.rfftn_slab(field, g, r))
            assert err <= fwd_bar(full, N), (r, err)
            c.xsolve(c.four, order, lr)
            c.stage.fill_(FSENT)
        swap(torch, slabs, 'four', 'stage', pieces)
        for r, c in enumerate(slabs):
            c.fill_mesh()
            c.zy_backward(c.stage)
            mesh = c.read_mesh()
            want = phi[r*g.nxl:(r + 1)*g.nxl]
            err = float((mesh[c.G:c.G + g.nxl, :N, :N] - want).abs().max())
            print(f'chain P = {P}, N = {N}, rank {r}: max deviation {err:.3e} of '
                  f'{float(phi.abs().max()):.3e}')
            assert err <= 1e-12*float(phi.abs().max()), r
            assert c.ghosts_kept(mesh)
    finally:
        single.close()
        for c in slabs:
            c.close()


# ---------------------------------------------------------------------------------------------
# refusals: non-zero with a message, nothing launched, the stage untouched
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('backend', ['own', 'rocfft'])
def test_refusals(gpu, monkeypatch, backend):
    set_backend(gpu, monkeypatch, 16, None, backend, {})
    c = Slab(gpu, 16, 4, 1)
    try:
        L, ctx, p = gpu.L, c.m._ctx, gpu.ptr(c.stage)
        nxl = c.g.nxl
        calls = {
            'forward: layer0 + nlayers > nxl': lambda: L.cg_dist_fft_forward_layers(ctx, p, nxl - 1, 2),
            'backward: layer0 + nlayers > nxl': lambda: L.cg_dist_fft_backward_layers(ctx, p, nxl - 1, 2),
            'forward: layer0 = nxl': lambda: L.cg_dist_fft_forward_layers(ctx, p, nxl, 1),
            'forward: nlayers = 0': lambda: L.cg_dist_fft_forward_layers(ctx, p, 0, 0),
            'backward: nlayers = 0': lambda: L.cg_dist_fft_backward_layers(ctx, p, 0, 0),
            'forward: layer0 < 0': lambda: L.cg_dist_fft_forward_layers(ctx, p, -1, 1),
            'backward: layer0 < 0': lambda: L.cg_dist_fft_backward_layers(ctx, p, -1, 2),
            'forward: null buffer': lambda: L.cg_dist_fft_forward(ctx, None),
            'forward_layers: null buffer': lambda: L.cg_dist_fft_forward_layers(ctx, None, 0, 1),
            'backward: null buffer': lambda: L.cg_dist_fft_backward(ctx, None),
            'backward_layers: null buffer': lambda: L.cg_dist_fft_backward_layers(ctx, None, 0, 1),
            'x: null buffer': lambda: L.cg_dist_fft_x(ctx, None, 0),
            'xsolve: null buffer': lambda: L.cg_dist_fft_xsolve(ctx, None, 2, C, 0, E),
            'xsolve: deconv_order = 9': lambda: L.cg_dist_fft_xsolve(ctx, p, 9, C, 0, E),
            'xsolve: deconv_order = -1': lambda: L.cg_dist_fft_xsolve(ctx, p, -1, C, 0, E),
        }
        c.fill_mesh()
        for what, call in calls.items():
            assert call() != 0, what
            message = gpu.lib.last_error()
            assert message.startswith('cg_dist_fft_'), (what, message)
            assert bool((c.stage == FSENT).all()), what
        assert bool((c.read_mesh() == FSENT).all())
        gpu.torch.cuda.synchronize()
    finally:
        c.close()
