"""Who owns what in the rocFFT backend (concept_amd/csrc/cg_rocfft.hip): contexts that are made,
used, destroyed and made again in one process, and one context whose single work buffer and
execution info serve plans of different needs in turn.  What the transforms compute is the
business of test_gpu_pm.py and test_gpu_slab_fft.py; here every result is still compared with
numpy, so that a plan or a buffer that did not survive its neighbours shows as a wrong number.

Bars (none is made from what the code under test gives):
  single domain  1e-12*max|phi|: the rocFFT leg of test_gpu_pm.py's
                 test_handwritten_fft_vs_numpy_and_rocfft
  slab pieces    those of test_gpu_slab_fft.py for the same pieces against the references of
                 slab_fft_refs.py: forward 1e-13*rms(ref)*log2(N)**2, round trips
                 1e-13*N**d*max, xsolve 1e-12*max|ref|"""
import numpy as np
import pytest

import slab_fft_refs as R
from test_gpu_slab_fft import BOX, C, E, FSENT, Gpu, Slab, fwd_bar, maxerr, set_backend

pytestmark = pytest.mark.gpu

ORDER, LR = 2, 1


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return Gpu(torch)


@pytest.mark.parametrize('N,backend', [(16, 'rocfft'), (24, 'rocfft')],
                         ids=['16-forced', '24-unset'])
def test_single_domain_twice(gpu, monkeypatch, N, backend):
    """create, forward, kernel, backward, destroy — twice, against numpy on the same density"""
    torch = gpu.torch
    set_backend(gpu, monkeypatch, N, None, backend, {})   # (24: the variable is unset)
    g = R.geometry(N, 1)
    dens = np.random.default_rng(17*N).normal(0, 1, (N, N, N))
    F = R.slab_factor(g, 0, ORDER, C, LR, E)              # [a][b][kk], all rows b on one domain
    phi = float(N**3)*np.fft.irfftn(F*np.fft.rfftn(dens), s=(N, N, N), axes=(0, 1, 2))
    bar = 1e-12*float(np.abs(phi).max())  # test_handwritten_fft_vs_numpy_and_rocfft, rocFFT leg
    sizes = []
    for attempt in range(2):
        mesh = gpu.Mesh(N, BOX)
        try:
            whole = torch.zeros((N, g.ny, g.pad), dtype=torch.float64, device='cuda')
            whole[:, :N, :N] = gpu.dev(dens)
            mesh.layers_write(0, N, whole)
            mesh.poisson_forward(ORDER, C, bool(LR), E, apply_kernel=False)
            mesh.poisson_kernel(ORDER, C, bool(LR), E)
            mesh.poisson_backward()
            mesh.layers_read(0, N, whole)
            err = float((whole[:, :N, :N] - gpu.dev(phi)).abs().max())
            print(f'single domain N = {N}, attempt {attempt}: max deviation {err:.3e}, bar {bar:.3e}')
            assert err <= bar
            sizes.append(mesh.device_bytes)
        finally:
            mesh.close()
    # the mesh, the tile tables and the work buffer of the 3-D plans: the same answer each time,
    # and no less than the mesh
    assert sizes[0] == sizes[1] >= 8*N*g.ny*g.pad


@pytest.mark.parametrize('N,P,rank,backend', [(24, 2, 1, 'rocfft'), (16, 4, 2, 'rocfft')],
                         ids=['24-P2-r1', '16-P4-r2-forced'])
def test_slab_pieces_share_one_work_buffer(gpu, monkeypatch, N, P, rank, backend):
    """ZYForward on two layer ranges of different size (two 2-D plans; at 16 points the inverse
    2-D plan is refused and ZYBackward takes the 1-D pair), XForward, XBackward, XSolve,
    ZYBackward on one context; then the context is destroyed and all of it runs on a new one"""
    set_backend(gpu, monkeypatch, N, None, backend, {})
    field, Y = gpu.field(N, P, rank)
    for attempt in range(2):
        c = Slab(gpu, N, P, rank)
        try:
            g = c.g
            x, xf, _ = gpu.rows(N, g.JB)
            # 1. z and y forward, in two pieces
            c.fill_mesh(gpu.dev(field))
            for piece in ((0, g.nxl//2 - 1), (g.nxl//2 - 1, g.nxl - g.nxl//2 + 1)):
                c.zy_forward(c.stage, piece)
            B = c.blocked(c.stage)
            assert maxerr(gpu, c.live(B), R.blocked_live(Y, g)) <= fwd_bar(Y, N)
            c.dead_kept(B, True)
            # 2. x forward, 3. x backward: N times the identity
            F = c.fourier(c.four)
            c.load_rows(c.four, x)
            c.x(c.four, 0)
            assert maxerr(gpu, c.live(F), xf) <= fwd_bar(xf, N)
            c.x(c.four, 1)
            assert maxerr(gpu, c.live(F), N*x) <= 1e-13*N*float(np.abs(x).max())
            # 4. the fused x pass
            ref = R.x_backward(R.slab_factor_ld(g, rank, ORDER, C, LR, E).astype(np.float64)*xf)
            c.load_rows(c.four, x)
            c.xsolve(c.four, ORDER, LR)
            assert maxerr(gpu, c.live(F), ref) <= 1e-12*float(np.abs(ref).max())
            c.dead_kept(F, False)
            # 5. y and z backward of all layers
            c.stage.copy_(gpu.dev(R.pack_blocked(Y, g, complex(FSENT, FSENT)).view(np.float64).reshape(-1)))
            c.fill_mesh()
            c.zy_backward(c.stage)
            mesh = c.read_mesh()
            err = float((mesh[c.G:c.G + g.nxl, :N, :N] - gpu.dev(field)*float(N*N)).abs().max())
            print(f'slab N = {N}, P = {P}, attempt {attempt}: zy_backward max deviation {err:.3e}')
            assert err <= 1e-13*N*N*float(np.abs(field).max())
            assert c.ghosts_kept(mesh)
        finally:
            c.close()


def test_timed_solve_refused_on_rocfft(gpu, monkeypatch):
    """cg_poisson_solve_timed times the passes of the hand-written solve: a rocFFT context is
    refused with the reason, before any event is made"""
    set_backend(gpu, monkeypatch, 16, None, 'rocfft', {})
    mesh = gpu.Mesh(16, BOX)
    try:
        with pytest.raises(gpu.lib.ConceptGPUError, match='cg_poisson_solve_timed: hand-written'):
            mesh.poisson_solve_timed(ORDER, C, bool(LR), E)
        mesh.zero()
        mesh.poisson_solve(ORDER, C, bool(LR), E)   # (the context is as usable as before)
        mesh.synchronize()
    finally:
        mesh.close()
