"""The kernels of the general particle_mesh() (concept_amd/csrc/cg_general.hip), one by one:
k_nullify_nyquist, k_fourier_operate, k_copy_modes, k_cm_pack / k_cm_unpack, k_fluid_add,
k_mesh_diff and k_fluid_kick, each against a plain reference of the same operation
(tests/general_kernel_refs.py) instead of through a whole deposit -> FFT -> k-space -> FFT ->
gather pipeline.

One domain: a random real field goes in with fluid_add('=') (itself checked bit for bit against
fetch_real()), fft_forward() makes it a spectrum whose Nyquist planes hold data, fetch_fourier()
gives the input modes A; the operation runs and the slab is fetched again.  The expectation is
the long-double value M*A [+ previous]; the FFT is not under test.
x-slab domains: PotentialMesh(N, L, nprocs=P, rank=r) without a comm, all P side by side on one
GPU (the pattern of test_gpu_slab_handover.py).  Each context gets a caller-owned torch buffer
bound with cg_dist_bind_fourier and filled with its rows of a full host slab; row JB of every
layer and the columns kk > nyq hold a sentinel that must survive; the exchange of
copy_modes_pack / _unpack is done by hand from a row plan derived here from the header's rule.

Bar of every k-space comparison, per mode:
    |got - ref| <= 2*ORACLE_DEV_EPS[deconv_order]*eps*|M|*|A|   (+ 2*eps*|previous| with '+=')
ORACLE_DEV_EPS is the float64 oracle's own deviation from the long-double value, measured and
asserted by test_general_oracle_host.py; the factor 2 is for the kernel's repeated multiplication
instead of pow and the device's sin / cos.  Elements documented as untouched must keep their
bits, elements documented as zeroed must be 0.0.  The stencils are compiled with contraction
off: float64 numpy in the order of fd_value() gives the same bits, and bit equality is asked.

Grids: 12 (pad N + 2) and 16 (pad N + 16, ny N + 1) carry the full cross product of options;
144 and 152 (one of each layout) take the 64-lane kk loops into a second trip (nyq 72 / 76) and
the row loops past the 16384 blocks of blocks_for (20736 / 23104 rows); 162 takes the cell loops
of the stencils past 16384*256 cells.  Left out on purpose: the 256-lane kk loop of
k_fourier_operate takes its second trip only from N = 514, a workload-sized mesh."""
import ctypes

import numpy as np
import pytest

import general_kernel_refs as R

pytestmark = pytest.mark.gpu

BOX = 64.0
FSENT = 1e150
MODES = ('inplace', 'copy=', 'copy+=')
SLAB_GEOMETRIES = [(2, 16), (4, 24), (4, 144)]
PACK_CASES = [(2, 16, 24), (2, 24, 16), (4, 16, 24), (4, 24, 16), (4, 144, 152), (4, 152, 144)]
COPY_DIRECTIONS = [p for pair in R.COPY_PAIRS_SMALL + (R.COPY_PAIR_LARGE,)
                   for p in (pair, pair[::-1])]


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def gpu(torch_cuda):
    """the contexts and spectra of the module: made once, closed at the end"""
    g = Gpu(torch_cuda)
    yield g
    g.close()


def sh3(shift):
    return (ctypes.c_double*3)(*[float(x) for x in shift])


class Spectrum:
    """three single-domain contexts of one grid size: a and b hold the transforms A and B of two
    random fields and are never written again, w is the one operated on"""

    def __init__(self, g, N):
        self.N = N
        self.a, self.b, self.w = (g.domain(N, t) for t in 'abw')
        rng = np.random.default_rng(N)
        for m in (self.a, self.b):
            m.fluid_add(g.dev(rng.normal(0, 1, (N, N, N))), 1.0, '=')
            m.fft_forward()
        self.A, self.B = (R.as_modes(m.fetch_fourier()).copy() for m in (self.a, self.b))
        live = R.live_mask(N)
        # not nullified: the Nyquist planes hold data that a wrong write or a missing zero shows
        assert (np.abs(self.A[~live]) > 0).mean() > 0.9 and (np.abs(self.B[~live]) > 0).mean() > 0.9

    def fetch(self):
        return R.as_modes(self.w.fetch_fourier())


class SlabView:
    """a slab context with a bound Fourier buffer complex[N][JB + 1][pad/2]"""

    def __init__(self, g, mesh):
        self.g, self.m = g, mesh
        self.N, self.JB, self.cp = mesh.gridsize, mesh.gridsize//mesh.nprocs, mesh.pad//2
        self.j0, self.nyq = self.JB*mesh.rank, mesh.gridsize//2
        assert mesh.transpose_doubles == self.N*(self.JB + 1)*self.cp*2
        self.buf = g.torch.empty(mesh.transpose_doubles, dtype=g.torch.float64, device='cuda')
        g.check(g.L.cg_dist_bind_fourier(mesh._ctx, g.ptr(self.buf)))
        self.sent = None

    def upload(self, S):
        """this domain's rows of the full slab S = complex[j][i][nyq + 1]; a sentinel in the
        unused row JB and in the columns kk > nyq"""
        h = np.full((self.N, self.JB + 1, self.cp), FSENT*(1 + 1j))
        h[:, :self.JB, :self.nyq + 1] = S[self.j0:self.j0 + self.JB].transpose(1, 0, 2)
        self.sent = h
        self.buf.copy_(self.g.torch.from_numpy(h.view(np.float64).reshape(-1)))

    def download(self):
        """the live rows as complex[JB][i][nyq + 1]; the sentinel must be intact"""
        h = self.buf.cpu().numpy().view(np.complex128).reshape(self.N, self.JB + 1, self.cp)
        dead = np.ones(h.shape, dtype=bool)
        dead[:, :self.JB, :self.nyq + 1] = False
        assert R.same_bits(h[dead], self.sent[dead]), 'row JB or a column kk > nyq was written'
        return h[:, :self.JB, :self.nyq + 1].transpose(1, 0, 2)


class Gpu:
    def __init__(self, torch):
        from concept_amd import lib
        from concept_amd.mesh import PotentialMesh
        self.torch, self.lib, self.L, self.Mesh = torch, lib, lib.raw(), PotentialMesh
        self.check, self.ptr = lib.check, lib._ptr
        self.domains, self.slab_sets, self.spectra, self.views = {}, {}, {}, {}

    def dev(self, a):
        return self.torch.tensor(np.ascontiguousarray(a), device='cuda')

    def domain(self, N, tag):
        if (N, tag) not in self.domains:
            # (nghosts = 4 on the smallest grid: a stencil of order 8 reaches four cells)
            self.domains[N, tag] = self.Mesh(N, BOX, nghosts=4 if N == 12 else 2)
        return self.domains[N, tag]

    def spectrum(self, N):
        if N not in self.spectra:
            self.spectra[N] = Spectrum(self, N)
        return self.spectra[N]

    def slabs(self, P, N, tag):
        if (P, N, tag) not in self.slab_sets:
            self.slab_sets[P, N, tag] = [self.Mesh(N, BOX, nprocs=P, rank=r) for r in range(P)]
        return self.slab_sets[P, N, tag]

    def slab_views(self, P, N, tag):
        if (P, N, tag) not in self.views:
            self.views[P, N, tag] = [SlabView(self, m) for m in self.slabs(P, N, tag)]
        return self.views[P, N, tag]

    def close(self):
        for m in list(self.domains.values()) + [m for s in self.slab_sets.values() for m in s]:
            m.close()

    # the C entries, called directly: the wrappers' early exits and zeroing stay out of the way
    def operate(self, onto, src, case, op_add):
        order, nl, shift, dd = case
        return self.L.cg_fourier_operate(onto._ctx, src._ctx, int(order), int(nl), sh3(shift),
                                         int(dd), int(op_add))

    def copy_modes(self, onto, src, case, op_add):
        order, nl, shift = case
        return self.L.cg_copy_modes(onto._ctx, src._ctx, int(order), int(nl), sh3(shift),
                                    int(op_add))

    def whole_layers(self, mesh):
        """every double of the local mesh buffer, ghost layers, row ny - 1 and padding included,
        as a (layers, ny, pad) tensor"""
        G, n = mesh.ghost_layers, mesh.nxl + 2*mesh.ghost_layers
        out = self.torch.empty(n*mesh.layer_doubles, dtype=self.torch.float64, device='cuda')
        mesh.layers_read(-G, n, out)
        return out.view(n, mesh.layer_doubles//mesh.pad, mesh.pad)

    def fill_layers(self, mesh, value):
        G, n = mesh.ghost_layers, mesh.nxl + 2*mesh.ghost_layers
        mesh.layers_write(-G, n, self.torch.full((n*mesh.layer_doubles,), value,
                                                 dtype=self.torch.float64, device='cuda'))

    def owned_is(self, mesh, ref, rest=FSENT):
        """the owned cells hold the bits of `ref`; ghost layers, the unused row and the padding
        columns hold `rest`"""
        torch, G, N = self.torch, mesh.ghost_layers, mesh.gridsize
        raw = self.whole_layers(mesh)
        owned = raw[G:G + mesh.nxl, :N, :N].contiguous().view(torch.int64)
        if not torch.equal(owned, self.dev(ref).view(torch.int64)):
            return False
        return (bool((raw[:G] == rest).all()) and bool((raw[G + mesh.nxl:] == rest).all())
                and bool((raw[:, N:, :] == rest).all()) and bool((raw[:, :, N:] == rest).all()))


def zero_bits(a):
    return not np.ascontiguousarray(a).view(np.int64).any()


# ---------------------------------------------------------------------------------------------
# 1. how the data gets in: fluid_add against fetch_real, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', R.GRIDS_SMALL + (162,))
def test_fluid_add_bit_for_bit(gpu, N):
    m = gpu.domain(N, 'w')
    rng = np.random.default_rng(N + 5)
    f, h = R.distinct_field(N, N), rng.normal(0, 1, (N, N, N))
    gpu.fill_layers(m, FSENT)
    m.fluid_add(gpu.dev(f), 1.0, '=')
    assert R.same_bits(m.fetch_real()[:, :, :N], f) and gpu.owned_is(m, f)
    m.fluid_add(gpu.dev(h), 0.37, '+=')       # mesh.py:1737-1751: value*factor, then the sum
    want = f + h*0.37
    assert gpu.owned_is(m, want)
    m.fluid_add(gpu.dev(h), 1.0, '+=')
    want = want + h
    assert gpu.owned_is(m, want)
    m.fluid_add(gpu.dev(h), 2.5, '=')
    assert R.same_bits(m.fetch_real()[:, :, :N], h*2.5) and gpu.owned_is(m, h*2.5)


# ---------------------------------------------------------------------------------------------
# 2. one domain: nullify_nyquist, fourier_operate, copy_modes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', R.GRIDS_SMALL + R.GRIDS_LARGE)
def test_nullify_nyquist_one_domain(gpu, N):
    s = gpu.spectrum(N)
    live = R.live_mask(N)
    s.w.copy_from(s.a)
    s.w.nullify_nyquist()
    got = s.fetch()
    assert zero_bits(got[~live]) and R.same_bits(got[live], s.A[live])


def operate_and_check(gpu, s, case, mode, live):
    op_add = mode == 'copy+='
    s.w.copy_from(s.a if mode == 'inplace' else s.b)
    gpu.check(gpu.operate(s.w, s.w if mode == 'inplace' else s.a, case, op_add))
    got = s.fetch()
    if mode == 'copy=':     # the reference's nullified target
        assert zero_bits(got[~live]), (case, 'the Nyquist planes are not 0.0')
    else:
        before = s.A if mode == 'inplace' else s.B
        assert R.same_bits(got[~live], before[~live]), (case, 'a Nyquist plane was written')
    M, ref = R.expect_operate(s.A, s.B, s.N, BOX, case, op_add)
    scale = np.abs(M).astype(np.float64)*np.abs(s.A)
    bar = R.mode_bar(case[0], scale, s.B if op_add else None)
    R.check_modes(got[live], ref[live], bar[live], f'N = {s.N}, {mode}, {case}')
    return got


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N', R.GRIDS_SMALL)
def test_fourier_operate_one_domain_full_cross(gpu, N, mode):
    s, live = gpu.spectrum(N), R.live_mask(N)
    for case in R.operate_cases():
        operate_and_check(gpu, s, case, mode, live)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N', R.GRIDS_LARGE)
def test_fourier_operate_one_domain_large(gpu, N, mode):
    s, live = gpu.spectrum(N), R.live_mask(N)
    cases = R.operate_cases_large()
    for case in cases if mode == 'inplace' else cases[:3]:
        operate_and_check(gpu, s, case, mode, live)


@pytest.mark.parametrize('N', R.GRIDS_SMALL + R.GRIDS_LARGE)
def test_fourier_differentiation_known_answer(gpu, N):
    """diff_dim = d and nothing else: every mode comes back as i*k_fundamental*k_d times itself,
    the float64 product, bit for bit (what mesh.py:3391-3392 computes)"""
    s, live = gpu.spectrum(N), R.live_mask(N)
    k = R.wave_numbers(N)
    kd = {0: k[None, :, None], 1: k[:, None, None], 2: np.arange(N//2 + 1)[None, None, :]}
    for dd in (0, 1, 2):
        s.w.copy_from(s.a)
        gpu.check(gpu.operate(s.w, s.w, (0, 1, (0.0, 0.0, 0.0), dd), False))
        got = s.fetch()
        f = 1.0*((2*np.pi/BOX)*kd[dd].astype(np.float64))
        want = np.empty_like(s.A)
        want.real, want.imag = (-s.A.imag)*f, s.A.real*f
        assert R.same_bits(got[live], want[live]), dd
        assert R.same_bits(got[~live], s.A[~live])


@pytest.mark.parametrize('op_add', [False, True])
@pytest.mark.parametrize('N_from,N_onto', COPY_DIRECTIONS)
def test_copy_modes_one_domain(gpu, N_from, N_onto, op_add):
    """the C entry itself, onto a mesh that holds another field's transform: the cube's modes
    within the bar, every other element of `onto` (the modes outside the cube, the Nyquist planes
    of both grids' index ranges) untouched"""
    sf, so = gpu.spectrum(N_from), gpu.spectrum(N_onto)
    large = max(N_from, N_onto) > 100
    for case in R.copy_cases_large() if large else R.copy_cases():
        so.w.copy_from(so.b)
        gpu.check(gpu.copy_modes(so.w, sf.a, case, op_add))
        got = so.fetch()
        cube, M, scale, ref = R.expect_copy(sf.A, so.B, N_from, N_onto, BOX, case, op_add)
        outside = np.ones(got.shape, dtype=bool)
        outside[cube] = False
        assert R.same_bits(got[outside], so.B[outside]), (case, 'a mode outside the cube changed')
        bar = R.mode_bar(case[0], scale, so.B[cube] if op_add else None)
        R.check_modes(got[cube], ref, bar, f'{N_from} -> {N_onto}, op_add {op_add}, {case}')


@pytest.mark.parametrize('N_from,N_onto', [(12, 16), (16, 12), (144, 152)])
def test_copy_modes_from_zeroes_first(gpu, N_from, N_onto):
    sf, so = gpu.spectrum(N_from), gpu.spectrum(N_onto)
    case = (4, 2, (-0.5, -0.5, -0.5))
    so.w.copy_from(so.b)
    so.w.copy_modes_from(sf.a, *case, operation='=')
    got = so.fetch()
    cube, M, scale, ref = R.expect_copy(sf.A, so.B, N_from, N_onto, BOX, case, False)
    outside = np.ones(got.shape, dtype=bool)
    outside[cube] = False
    assert zero_bits(got[outside])
    R.check_modes(got[cube], ref, R.mode_bar(case[0], scale), f'{N_from} -> {N_onto}')


@pytest.mark.parametrize('N', R.GRIDS_SMALL)
def test_copy_modes_of_equal_sizes_is_fourier_operate(gpu, N):
    s = gpu.spectrum(N)
    for case in R.copy_cases((0, 4, 8)):
        for op_add in (False, True):
            s.w.copy_from(s.b)
            gpu.check(gpu.copy_modes(s.w, s.a, case, op_add))
            one = s.fetch().copy()
            s.w.copy_from(s.b)
            gpu.check(gpu.operate(s.w, s.a, case + (-1,), op_add))
            assert R.same_bits(one, s.fetch()), (case, op_add)
            assert not R.same_bits(one, s.B)


# ---------------------------------------------------------------------------------------------
# 3. x-slab views in one process
# ---------------------------------------------------------------------------------------------
def random_modes(N, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (N, N, N//2 + 1)) + 1j*rng.normal(0, 1, (N, N, N//2 + 1))


@pytest.mark.parametrize('P,N', SLAB_GEOMETRIES)
def test_nullify_nyquist_on_slabs(gpu, P, N):
    S, live = random_modes(N, 11), R.live_mask(N)
    for v in gpu.slab_views(P, N, 'a'):
        v.upload(S)
        v.m.nullify_nyquist()
        got, rows = v.download(), slice(v.j0, v.j0 + v.JB)
        assert zero_bits(got[~live[rows]])
        assert R.same_bits(got[live[rows]], S[rows][live[rows]])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('P,N', SLAB_GEOMETRIES)
def test_fourier_operate_on_slabs(gpu, P, N, mode):
    """every rank's rows against the full-slab reference; two contexts per rank for from != onto"""
    va, vb = gpu.slab_views(P, N, 'a'), gpu.slab_views(P, N, 'b')
    Sa, Sb, live = random_modes(N, 21), random_modes(N, 22), R.live_mask(N)
    op_add = mode == 'copy+='
    cases = (R.operate_cases_large()[:4] if N > 100 else R.operate_cases(orders=(0, 8)))
    for case in cases:
        M, ref = R.expect_operate(Sa, Sb, N, BOX, case, op_add)
        scale = np.abs(M).astype(np.float64)*np.abs(Sa)
        bar = R.mode_bar(case[0], scale, Sb if op_add else None)
        for a, b in zip(va, vb):
            rows = slice(a.j0, a.j0 + a.JB)
            a.upload(Sa)
            if mode == 'inplace':
                gpu.check(gpu.operate(a.m, a.m, case, False))
                got, before = a.download(), Sa[rows]
            else:
                b.upload(Sb)
                gpu.check(gpu.operate(b.m, a.m, case, op_add))
                got, before = b.download(), Sb[rows]
                assert R.same_bits(a.download(), Sa[rows]), '`from` was written'
            lv = live[rows]
            if mode == 'copy=':
                assert zero_bits(got[~lv]), case
            else:
                assert R.same_bits(got[~lv], before[~lv]), case
            R.check_modes(got[lv], ref[rows][lv], bar[rows][lv],
                          f'P = {P}, N = {N}, rank {a.m.rank}, {mode}, {case}')


def test_differentiation_of_single_modes_on_slabs(gpu):
    """one non-zero mode at hand-picked (ki, kj, kk), negative ki and kj and kk = 0 among them:
    back comes i*k_fundamental*k_d times the mode, the float64 product; all else stays zero"""
    P, N = 2, 16
    views = gpu.slab_views(P, N, 'a')
    value = 0.75 - 1.25j
    for ki, kj, kk in [(-3, 2, 0), (5, -7, 3), (-1, -1, 7), (0, 4, 1), (2, 0, 5), (-7, 7, 6)]:
        S = np.zeros((N, N, N//2 + 1), dtype=np.complex128)
        S[kj % N, ki % N, kk] = value
        for dd, kd in enumerate((ki, kj, kk)):
            f = 1.0*((2*np.pi/BOX)*float(kd))
            want = np.zeros_like(S)
            want[kj % N, ki % N, kk] = complex((-value.imag)*f, value.real*f)
            for v in views:
                v.upload(S)
                gpu.check(gpu.operate(v.m, v.m, (0, 1, (0.0, 0.0, 0.0), dd), False))
                got, rows = v.download(), slice(v.j0, v.j0 + v.JB)
                assert np.array_equal(got, want[rows]), (ki, kj, kk, dd)
                if v.j0 <= kj % N < v.j0 + v.JB:
                    assert R.same_bits(got[kj % N - v.j0, ki % N, kk], want[kj % N, ki % N, kk])


def row_plan(NS, N_from, N_onto, P):
    """include/concept_gpu.h: row kb of the small cube belongs to rank (kb mod N)//(N/P) in each
    grid.  send[src][dst] / recv[dst][src]: row numbers inside the owner's block, in the order of
    kb; the rows of the small grid's Nyquist plane do not travel"""
    send = [[[] for _ in range(P)] for _ in range(P)]
    recv = [[[] for _ in range(P)] for _ in range(P)]
    for kb in range(-(NS//2 - 1), NS//2):
        bf, bo = kb % N_from, kb % N_onto
        src, dst = bf//(N_from//P), bo//(N_onto//P)
        send[src][dst].append(bf % (N_from//P))
        recv[dst][src].append(bo % (N_onto//P))
    return send, recv


@pytest.mark.parametrize('P,N_from,N_onto', PACK_CASES)
def test_copy_modes_pack_exchange_unpack(gpu, P, N_from, N_onto):
    torch = gpu.torch
    vf, vo = gpu.slab_views(P, N_from, 'a'), gpu.slab_views(P, N_onto, 'b')
    ctx_from = gpu.slabs(P, N_from, 'a')
    NS = min(N_from, N_onto)
    nyq, per_row = NS//2, NS*(NS//2)
    send, recv = row_plan(NS, N_from, N_onto, P)
    assert sum(len(q) for s in send for q in s) == NS - 1
    Sa, Sb = random_modes(N_from, 31), random_modes(N_onto, 32)
    ks, i_from = R.cube_index(NS, N_from)
    # pack, once: bit for bit the small-cube part of the listed rows; the row as == nyq of every
    # packed row and everything behind the last row keep the sentinel
    pieces = [[None]*P for _ in range(P)]
    for src, v in enumerate(vf):
        v.upload(Sa)
        rows = [r for q in send[src] for r in q]
        out = torch.full(((len(rows) + 2)*per_row,), FSENT*(1 + 1j), dtype=torch.complex128,
                         device='cuda')
        rows_t = torch.tensor(rows, dtype=torch.int32, device='cuda')
        if rows:
            gpu.check(gpu.L.cg_copy_modes_pack(v.m._ctx, NS, gpu.ptr(rows_t), len(rows),
                                               gpu.ptr(out)))
        assert R.same_bits(v.download(), Sa[v.j0:v.j0 + v.JB])
        h = out.cpu().numpy().reshape(len(rows) + 2, NS, nyq)
        want = np.full(h.shape, FSENT*(1 + 1j))
        for r, row in enumerate(rows):
            want[r, ks % NS] = Sa[v.j0 + row][i_from, :nyq]
        assert R.same_bits(h, want), f'pack on rank {src}'
        start = 0
        for dst in range(P):
            n = len(send[src][dst])
            pieces[src][dst] = out[start*per_row:(start + n)*per_row]
            start += n
    cases = R.copy_cases_large()[:3] if NS > 100 else R.copy_cases()
    for op_add in (False, True):
        for case in cases:
            order, nl, shift = case
            cube, M, scale, ref = R.expect_copy(Sa, Sb, N_from, N_onto, BOX, case, op_add)
            full, bar = Sb.astype(R.CLD), np.zeros(Sb.shape)
            full[cube] = ref
            bar[cube] = R.mode_bar(order, scale, Sb[cube] if op_add else None)
            outside = np.ones(Sb.shape, dtype=bool)
            outside[cube] = False
            for dst, v in enumerate(vo):
                v.upload(Sb)
                rows = [r for q in recv[dst] for r in q]
                rows_t = torch.tensor(rows, dtype=torch.int32, device='cuda')
                inc = torch.cat([pieces[src][dst] for src in range(P)]
                                + [torch.full((per_row,), FSENT*(1 + 1j), dtype=torch.complex128,
                                              device='cuda')])   # (the hand exchange)
                assert inc.numel() == (len(rows) + 1)*per_row
                if rows:
                    gpu.check(gpu.L.cg_copy_modes_unpack(
                        v.m._ctx, ctx_from[dst]._ctx, NS, gpu.ptr(rows_t), len(rows), gpu.ptr(inc),
                        int(order), int(nl), sh3(shift), int(op_add)))
                got, sl = v.download(), slice(v.j0, v.j0 + v.JB)
                assert R.same_bits(got[outside[sl]], Sb[sl][outside[sl]]), (dst, case, op_add)
                R.check_modes(got, full[sl], bar[sl],
                              f'{N_from} -> {N_onto}, P = {P}, rank {dst}, op_add {op_add}, {case}')


def test_pack_and_unpack_of_no_rows_do_nothing(gpu):
    P, N_from, N_onto = 2, 16, 24
    vf, vo = gpu.slab_views(P, N_from, 'a')[0], gpu.slab_views(P, N_onto, 'b')[0]
    Sa, Sb = random_modes(N_from, 41), random_modes(N_onto, 42)
    vf.upload(Sa)
    vo.upload(Sb)
    out = gpu.torch.full((64,), FSENT, dtype=gpu.torch.float64, device='cuda')
    assert gpu.L.cg_copy_modes_pack(vf.m._ctx, 16, None, 0, gpu.ptr(out)) == 0
    assert gpu.L.cg_copy_modes_unpack(vo.m._ctx, vf.m._ctx, 16, None, 0, gpu.ptr(out), 4, 2,
                                      sh3((0.5, 0.5, 0.5)), 0) == 0
    assert bool((out == FSENT).all())
    assert R.same_bits(vf.download(), Sa[:vf.JB]) and R.same_bits(vo.download(), Sb[:vo.JB])


def test_refusals_launch_nothing(gpu):
    P = 2
    v16, w16 = gpu.slab_views(P, 16, 'a')[1], gpu.slab_views(P, 16, 'b')[1]
    v24 = gpu.slab_views(P, 24, 'b')[1]
    S16, T16, S24 = random_modes(16, 51), random_modes(16, 52), random_modes(24, 53)
    v16.upload(S16)
    w16.upload(T16)
    v24.upload(S24)
    rows = gpu.torch.zeros(1, dtype=gpu.torch.int32, device='cuda')
    inc = gpu.torch.zeros(2*16*8, dtype=gpu.torch.float64, device='cuda')
    zero = sh3((0, 0, 0))
    L = gpu.L
    refused = [
        (lambda: L.cg_copy_modes(v24.m._ctx, v16.m._ctx, 0, 1, zero, 0), 'cg_copy_modes_pack'),
        (lambda: L.cg_copy_modes_unpack(v24.m._ctx, v16.m._ctx, 12, gpu.ptr(rows), 1,
                                        gpu.ptr(inc), 0, 1, zero, 0), 'n_small must be the smaller'),
        (lambda: L.cg_copy_modes_pack(v16.m._ctx, 18, gpu.ptr(rows), 1, gpu.ptr(inc)),
         'small grid size 18'),
        (lambda: L.cg_fourier_operate(w16.m._ctx, v16.m._ctx, 9, 1, zero, -1, 0), 'deconv_order 9'),
        (lambda: L.cg_fourier_operate(w16.m._ctx, v16.m._ctx, 2, 3, zero, -1, 0),
         'nlattice 3 not in'),
        (lambda: L.cg_copy_modes(w16.m._ctx, v16.m._ctx, 9, 1, zero, 0), 'deconv_order 9'),
        (lambda: L.cg_copy_modes(w16.m._ctx, v16.m._ctx, 2, 3, zero, 0), 'nlattice 3 not in'),
        (lambda: L.cg_copy_modes_unpack(v24.m._ctx, v16.m._ctx, 16, gpu.ptr(rows), 1,
                                        gpu.ptr(inc), 9, 1, zero, 0), 'deconv_order 9'),
        (lambda: L.cg_copy_modes_unpack(v24.m._ctx, v16.m._ctx, 16, gpu.ptr(rows), 1,
                                        gpu.ptr(inc), 2, 3, zero, 0), 'nlattice 3 not in'),
    ]
    for call, message in refused:
        assert call() != 0
        assert message in gpu.lib.last_error(), (message, gpu.lib.last_error())
    assert R.same_bits(v16.download(), S16[8:]) and R.same_bits(w16.download(), T16[8:])
    assert R.same_bits(v24.download(), S24[12:]) and not bool(inc.any())


# ---------------------------------------------------------------------------------------------
# 4. the stencils: cg_mesh_diff and cg_fluid_kick
# ---------------------------------------------------------------------------------------------
MINUS_DT, INV_C2 = -0.0173, 1.0/299.0


def kick_inputs(N, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (N, N, N)), rng.uniform(0.5, 1.5, (N, N, N)),
            rng.uniform(0, 0.3, (N, N, N)))


STENCIL_ONE_DOMAIN = [(N, o) for N in (12, 16) for o in (0, 1, 2, 4, 6, 8)] + [(162, 2), (162, 8)]


@pytest.mark.parametrize('N,order', STENCIL_ONE_DOMAIN)
def test_stencils_one_domain(gpu, N, order):
    src, dst = gpu.domain(N, 'a'), gpu.domain(N, 'w')
    f = R.distinct_field(N, 100 + N)
    if N < 100:
        assert np.unique(f).size == f.size
    J0, rho, P = kick_inputs(N, 200 + N)
    rho_d, P_d = gpu.dev(rho), gpu.dev(P)
    gpu.fill_layers(src, FSENT)
    src.fluid_add(gpu.dev(f), 1.0, '=')
    for dim in range(3):
        g = R.fd_reference(f, dim, order, BOX/N)
        if order:
            gpu.fill_layers(dst, FSENT)
            dst.diff_from(src, dim, order)
            assert gpu.owned_is(dst, g), f'mesh_diff order {order} dim {dim}'
        J = gpu.dev(J0)
        src.fluid_kick(J, rho_d, P_d, dim, order, MINUS_DT, INV_C2)
        want = R.kick_reference(J0, rho, P, g, MINUS_DT, INV_C2)
        assert R.same_bits(J.cpu().numpy(), want), f'fluid_kick order {order} dim {dim}'
        assert gpu.owned_is(src, f)


@pytest.mark.parametrize('P,N', [(2, 16), (4, 24)])
def test_stencils_on_slabs(gpu, P, N):
    """the x stencils read through the three halo layers, filled by hand from the neighbours'
    owned layers across the slab faces and the box face"""
    torch = gpu.torch
    srcs, dsts = gpu.slabs(P, N, 'a'), gpu.slabs(P, N, 'b')
    f = R.distinct_field(N, 300 + N)
    assert np.unique(f).size == f.size
    J0, rho, Pr = kick_inputs(N, 400 + N)
    for s in srcs:
        gpu.fill_layers(s, FSENT)
        s.fluid_add(gpu.dev(f[s.x0:s.x0 + s.nxl]), 1.0, '=')
    layer = torch.empty(srcs[0].layer_doubles, dtype=torch.float64, device='cuda')
    for s in srcs:
        G = s.ghost_layers
        assert G == 3
        for g in list(range(-G, 0)) + list(range(s.nxl, s.nxl + G)):
            x = (s.x0 + g) % N
            srcs[x//s.nxl].layers_read(x % s.nxl, 1, layer)
            s.layers_write(g, 1, layer)
    for s, d in zip(srcs, dsts):
        own = slice(s.x0, s.x0 + s.nxl)
        before = gpu.whole_layers(s).clone()
        for order in (0, 1, 2, 4, 6):
            for dim in range(3):
                g = R.fd_reference(f, dim, order, BOX/N)[own]
                if order:
                    gpu.fill_layers(d, FSENT)
                    d.diff_from(s, dim, order)
                    assert gpu.owned_is(d, g), f'rank {s.rank}: mesh_diff order {order} dim {dim}'
                J = gpu.dev(J0[own])
                s.fluid_kick(J, gpu.dev(rho[own]), gpu.dev(Pr[own]), dim, order, MINUS_DT, INV_C2)
                want = R.kick_reference(J0[own], rho[own], Pr[own], g, MINUS_DT, INV_C2)
                assert R.same_bits(J.cpu().numpy(), want), (s.rank, order, dim)
        # order 8 reaches four layers beyond a slab face, the halo holds three: refused
        gpu.fill_layers(d, FSENT)
        J = gpu.dev(J0[own])
        with pytest.raises(gpu.lib.ConceptGPUError, match='the halo holds 3'):
            d.diff_from(s, 0, 8)
        with pytest.raises(gpu.lib.ConceptGPUError, match='the halo holds 3'):
            s.fluid_kick(J, gpu.dev(rho[own]), gpu.dev(Pr[own]), 0, 8, MINUS_DT, INV_C2)
        assert R.same_bits(J.cpu().numpy(), J0[own]) and bool((gpu.whole_layers(d) == FSENT).all())
        assert torch.equal(gpu.whole_layers(s), before)
