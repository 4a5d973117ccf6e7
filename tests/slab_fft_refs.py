"""Plain numpy references for the passes of the x-slab transform (fft_dist in
concept_amd/csrc/cg_fft.hip, cgk_libfft_dist and k_dist_rows in cg_rocfft.hip), without a GPU:
the layouts, the exchange by hand, the expected values, the k-space factor in float64 and in
numpy.longdouble, and the table of shapes that tests/test_gpu_slab_fft.py runs.

Layouts (complex128; N points, P domains, JB = nxl = N/P, cp = pad/2, nk = N/2 + 1):
  slab       complex[layer (nxl)][j (N)][kk (nk)]: a domain's layers after the z and y passes
  blocked    complex[P][nxl][JB + 1][cp]: send[q][layer][j - q*JB][kk], the all-to-all buffer.
             Row JB of every (q, layer) and the columns kk >= nk are never data.
  Fourier    complex[N][JB + 1][cp]: a receive buffer, block q = the layers of domain q, so that
             i = q*nxl + layer runs over the whole x axis; rows b = rank*JB + jl of the y axis.
Everything is unnormalised, as the kernels are: forward then backward is N per dimension.

The k-space factor F(a, b, kk) restates kspace_factor (cg_kspace.h) in the reference's
operation order: n(k) = k*(pi/N) + machine epsilon by array index, s = sin n,
((n_a n_b) n_kk / ((s_a s_b) s_kk))**deconv_order, C/k2, times exp(k2*E) when long_range; zero
on the three Nyquist planes and at the origin.  Once in float64 (the tables rounded to double
as the library uploads them) and once in longdouble (pi, the sine, the power and the
exponential in 64-bit mantissa arithmetic).

FACTOR_DEV_EPS is the largest deviation of the float64 form from the long-double value in units
of eps*|F|, per deconv_order (the convention of ORACLE_DEV_EPS in general_kernel_refs.py),
over every mode (a, b, kk) of every (shape, rank) of the table below, long_range 0 and 1,
C = -3.7, E = -1e-4.  measure_factor_dev() is what measured it (`python tests/slab_fft_refs.py`
prints the table); test_slab_fft_refs_host.py measures again and asserts it.  The bar of the
stand-alone kernel on the GPU is made from it and from nothing else."""
import collections

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = float(np.finfo(np.float64).eps)
PI_LD = 4*np.arctan(LD(1))
C_TEST, E_TEST = -3.7, -1e-4          # the values of test_handwritten_fft_vs_numpy_and_rocfft
ORDERS, LONG_RANGES = (0, 2, 4), (0, 1)
NCU = 256                             # compute units the forms of the table are worked out for

# measured by measure_factor_dev() over all of SHAPES + ROCFFT_SHAPES (see the docstring):
# 32.76, 36.67, 41.53, all three on the slab of rank 8 of 16 at 1024 points with long_range.  The
# exponential sets them: k2*E reaches -78.6 there, and the half ulp of that product is a relative
# 39 eps of exp(k2*E); without long_range, and on the grids up to 64 points, the deviations are
# 1.1, 5.9 and 10.7 (one rounding of C/k2, then the tables of n and sin n times the order).
FACTOR_DEV_EPS = {0: 32.77, 2: 36.67, 4: 41.54}


Geometry = collections.namedtuple('Geometry', 'N P JB nxl pad cp ny nk')


def geometry(N, P):
    """the sizes of cg_create (ctx_init): grids that are a multiple of 16 pad a row by 16
    doubles and a layer by one row, the others pad a row by 2"""
    assert N % P == 0
    m16 = N % 16 == 0
    pad = N + 16 if m16 else N + 2
    return Geometry(N, P, N//P, N//P, pad, pad//2, N + 1 if m16 else N, N//2 + 1)


# ---------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------
def blocked_live(slab, g):
    """complex[nl][N][nk] -> complex[P][nl][JB][nk]: the live elements of the blocked buffer"""
    nl = slab.shape[0]
    assert slab.shape == (nl, g.N, g.nk)
    return slab.reshape(nl, g.P, g.JB, g.nk).transpose(1, 0, 2, 3)


def pack_blocked(slab, g, fill=0.0):
    """complex[nl][N][nk] -> complex[P][nl][JB + 1][cp]; `fill` everywhere else"""
    out = np.full((g.P, slab.shape[0], g.JB + 1, g.cp), fill, dtype=np.complex128)
    out[:, :, :g.JB, :g.nk] = blocked_live(slab, g)
    return out


def unpack_blocked(buf, g):
    """complex[P][nl][JB + 1][cp] -> complex[nl][N][nk]"""
    nl = buf.shape[1]
    assert buf.shape == (g.P, nl, g.JB + 1, g.cp)
    return buf[:, :, :g.JB, :g.nk].transpose(1, 0, 2, 3).reshape(nl, g.N, g.nk).copy()


def live_blocked(g, layers=None):
    """mask over complex[P][nxl][JB + 1][cp] of the elements a ZY pass of `layers` (a range,
    default all) may write: rows < JB, columns < nk"""
    m = np.zeros((g.P, g.nxl, g.JB + 1, g.cp), dtype=bool)
    lo, hi = (0, g.nxl) if layers is None else layers
    m[:, lo:hi, :g.JB, :g.nk] = True
    return m


def fourier_view(buf, g):
    """a receive buffer complex[P][nxl][JB + 1][cp] as the Fourier slab complex[N][JB + 1][cp]
    (a view: i = q*nxl + layer)"""
    return buf.reshape(g.N, g.JB + 1, g.cp)


def exchange(send, recv, layer0=0, nlayers=None):
    """the all-to-all by hand, as Comm.all_to_all_layers: the layers [layer0, layer0 + nlayers)
    of block q of rank r's send buffer become those of block r of rank q's receive buffer.
    send, recv: one complex[P][nxl][JB + 1][cp] per rank; whole rows travel, row JB and the
    padding columns included"""
    P = len(send)
    hi = send[0].shape[1] if nlayers is None else layer0 + nlayers
    for r in range(P):
        for q in range(P):
            recv[q][r, layer0:hi] = send[r][q, layer0:hi]


# ---------------------------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------------------------
def zy_forward(layers):
    """real[nl][j][k] -> complex[nl][j][kk]: rfft2 per layer, y on axis 0 of a layer and z the
    half dimension"""
    return np.fft.rfft2(layers, axes=(1, 2))


def zy_backward(slab, N):
    """complex[nl][j][kk] (the transform of real layers) -> N*N times the real layers"""
    return float(N*N)*np.fft.irfft2(slab, s=(N, N), axes=(1, 2))


def x_forward(four):
    return np.fft.fft(four, axis=0)


def x_backward(four):
    return four.shape[0]*np.fft.ifft(four, axis=0)


def rfftn_slab(field, g, rank):
    """np.fft.rfftn of the whole real field [i][j][k], rows b of `rank`, as complex[N][JB][nk]"""
    return np.fft.rfftn(field)[:, rank*g.JB:(rank + 1)*g.JB, :]


# ---------------------------------------------------------------------------------------------
# the k-space factor
# ---------------------------------------------------------------------------------------------
def _signed(idx, N):
    idx = np.asarray(idx, dtype=np.int64)
    return idx - np.where(idx >= N//2, N, 0)


def kspace_tables(N, dtype):
    """n(k) and sin n(k) by array index (cg_create; mesh.py:2775-2776)"""
    k = _signed(np.arange(N), N)
    if dtype is np.float64:
        pi_over_n = 3.141592653589793/float(N)
        n = k.astype(np.float64)*pi_over_n + EPS
    else:
        n = k.astype(LD)*(PI_LD/LD(N)) + LD(EPS)
    return n, np.sin(n)


def kspace_factor(N, a, b, kk, deconv_order, C, long_range, E, dtype=np.float64):
    """F for the broadcast of the index arrays a, b (full dimensions) and kk (half dimension)"""
    a, b, kk = (np.asarray(v, dtype=np.int64) for v in (a, b, kk))
    nyq = N//2
    ka, kb = _signed(a, N), _signed(b, N)
    kab2 = kb*kb + ka*ka
    k2 = kab2 + kk*kk
    dead = (a == nyq) | (b == nyq) | (kk == nyq) | ((kab2 == 0) & (kk == 0))
    k2s = np.where(k2 == 0, 1, k2).astype(dtype)
    factor = np.ones(k2.shape, dtype=dtype)
    if deconv_order:
        n, s = kspace_tables(N, dtype)
        dab_n, dab_d = n[a]*n[b], s[a]*s[b]
        factor = ((dab_n*n[kk])/(dab_d*s[kk]))**int(deconv_order)
    pk = dtype(C)/k2s
    if long_range:
        pk = pk*np.exp(k2s*dtype(E))
    return np.where(dead, dtype(0), factor*pk)


def slab_factor(g, rank, deconv_order, C, long_range, E, dtype=np.float64, rows=None):
    """F[a (N)][jl][kk (nk)] on the Fourier slab of `rank`: b = rank*JB + jl (rows: a subset of
    jl)"""
    jl = np.arange(g.JB) if rows is None else np.asarray(rows)
    return kspace_factor(g.N, np.arange(g.N)[:, None, None], (rank*g.JB + jl)[None, :, None],
                         np.arange(g.nk)[None, None, :], deconv_order, C, long_range, E, dtype)


def slab_factor_ld(g, rank, deconv_order, C, long_range, E):
    """the long-double F[a][jl][kk] of a whole slab, evaluated separably so that a slab of 1024
    points takes a second and not a minute: t(i) = (n_i/s_i)**order * exp(k_i**2 * E) per
    dimension, F = C * t_a t_b t_kk / k2.  The same value as slab_factor(..., LD) up to the
    rounding of long double (2**-11 of a double's; test_slab_fft_refs_host.py asserts it)"""
    N = g.N
    k = _signed(np.arange(N), N)
    t = np.ones(N, dtype=LD)
    if deconv_order:
        n, s = kspace_tables(N, LD)
        q = n/s
        for _ in range(int(deconv_order)):
            t = t*q
    if long_range:
        t = t*np.exp((k*k).astype(LD)*LD(E))
    b = rank*g.JB + np.arange(g.JB)
    kab2 = (k[b]**2)[None, :] + (k**2)[:, None]
    k2 = kab2[:, :, None] + (np.arange(g.nk)**2)[None, None, :]
    dead = ((np.arange(N) == N//2)[:, None, None] | (b == N//2)[None, :, None]
            | (np.arange(g.nk) == N//2)[None, None, :] | (k2 == 0))
    F = (LD(C)*(t[:, None]*t[b][None, :]))[:, :, None]*t[:g.nk][None, None, :]
    F = F/np.where(dead, 1, k2).astype(LD)
    F[dead] = 0
    return F


def factor_dev(g, rank, deconv_order, long_range, rows=None, block=8):
    """max |F64 - FLD| / (eps*|FLD|) over the modes of a slab, `block` rows at a time"""
    jl = np.arange(g.JB) if rows is None else np.asarray(rows)
    worst = 0.0
    for i in range(0, len(jl), block):
        r = jl[i:i + block]
        f64 = slab_factor(g, rank, deconv_order, C_TEST, long_range, E_TEST, np.float64, r)
        fld = slab_factor(g, rank, deconv_order, C_TEST, long_range, E_TEST, LD, r)
        nz = fld != 0
        assert not f64[~nz].any()
        worst = max(worst, float((np.abs(f64[nz].astype(LD) - fld[nz])/np.abs(fld[nz])).max())/EPS)
    return worst


def measure_factor_dev(cases, rows=None):
    """{order: worst deviation} over cases = [(N, P, rank)]; rows(g, rank) -> subset of jl or
    None for all"""
    out = {}
    for order in ORDERS:
        out[order] = max(factor_dev(geometry(N, P), r, order, lr,
                                    None if rows is None else rows(geometry(N, P), r))
                         for N, P, r in cases for lr in LONG_RANGES)
    return out


# ---------------------------------------------------------------------------------------------
# the shapes: one slab context of rank r among P each
# ---------------------------------------------------------------------------------------------
# split: the value of CONCEPT_GPU_FFT_SPLIT (None: unset, the library's default 1).
# forms: what strided_choice (cg_fft_plan.h) answers at 256 compute units for the five passes
#   y_fwd   mode 0, from the y map (cp, 31) into the blocked map (cp, log2 JB), per chunk
#   y_inv   mode 1, the other way round
#   x_fwd, x_inv, x_fused   modes 0, 1, 2 on the x map ((JB + 1)*cp, 31), JB outer indices
# chunks: the layers per chunk of the z / y walk over the nxl owned layers.
Shape = collections.namedtuple('Shape', 'N P ranks split forms chunks what')


def _forms(y, x):
    return {'y_fwd': y, 'y_inv': y, 'x_fwd': x, 'x_inv': x, 'x_fused': x}


SHAPES = (
    Shape(16, 4, (0, 2, 3), None, _forms('Plain', 'Plain'), (4,),
          'the smallest legal block (sh = 2); 8 tiles'),
    Shape(16, 2, (1,), None, _forms('Plain', 'Plain'), (8,), 'sh = 3; rank 1 holds row N/2'),
    Shape(64, 8, (4, 7), None, _forms('Plain', 'Plain'), (8,),
          'a second kk tile with a short tail'),
    Shape(256, 4, (1, 2), None, _forms('Plain', 'Persistent'), (64,),
          'blocked y pass of 1088 tiles; the persistent x kernel with o_off 64 / 128, rank 2 '
          'holds row N/2'),
    Shape(512, 8, (0, 4, 5), None, _forms('Plain', 'Persistent'), (64,),
          'the slab of the 4096^3 on 8 GPUs configuration at 1/8 linear size'),
    Shape(512, 8, (5,), 2, _forms('SplitBlocked', 'Split'), (64,),
          'k_fft_strided_h<9, ...> both ways, sh = 6'),
    Shape(512, 16, (9,), 2, _forms('SplitBlocked', 'Split'), (32,),
          'a block of exactly the 32 rows a lane spans, sh = 5'),
    # (the x passes of this shape: 16*33 = 528 tiles >= 2*256 on plain maps, so they split; only
    # the blocked y passes are refused)
    Shape(512, 32, (17,), 2, _forms('Plain', 'Split'), (16,),
          'blocks of 16 rows: blocks_ok refuses the split y pass'),
    Shape(1024, 16, (8, 11), None, _forms('SplitBlocked', 'Split'), (32, 32),
          'the production instantiation <10, ..., true>; the chunk walk with layer0 = 32'),
)
# grids that are no power of two: the rocFFT backend with k_dist_rows (pad N + 2, N + 2, N + 16)
ROCFFT_SHAPES = (
    Shape(24, 2, (1,), None, None, None, 'pad N + 2'),
    Shape(36, 3, (1,), None, None, None, 'three domains, pad N + 2'),
    Shape(48, 2, (1,), None, None, None, 'pad N + 16, ny N + 1'),
)
CHAIN = ((2, 16), (4, 16), (8, 64), (3, 36))     # (P, N) of the chain test, all ranks
HOST_CHAIN = ((2, 16), (4, 16), (3, 36))          # ... of the references' own consistency test


def layer_pieces(nxl):
    """the pieces of the _layers tests, in call order"""
    return ((nxl//2, nxl - nxl//2), (0, 1), (1, nxl//2 - 1))


def all_cases():
    return list(dict.fromkeys((s.N, s.P, r) for s in SHAPES + ROCFFT_SHAPES for r in s.ranks))


if __name__ == '__main__':
    for case in all_cases():
        print(case, measure_factor_dev([case]), flush=True)
    print(measure_factor_dev(all_cases()))
