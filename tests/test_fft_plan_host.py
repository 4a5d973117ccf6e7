"""The host-side arithmetic of the hand-written solve (concept_amd/csrc/cg_fft_plan.h), without
a GPU: tests/fft_plan_print.cpp includes only that header, is compiled with the host compiler
and prints the chunk plans and the strided passes' forms for the inputs below.

The expected values are literals.  The chunk sizes and ChunkPlans were computed with the
expressions cg_fft.hip held before the header existed (256 compute units, an MI355X); the pass
forms are worked out by hand from the launchers' rules of that file:
  whole pencils   W = 8 up to 1024 points, 4 at 2048; NT = N*W/16 in 64..1024; LDS 16*N*W bytes,
                  the persistent form 16*(N/2) (+ 8*N fused) on top, min(4, 160 KB / LDS)
                  workgroups per CU, only with plain maps and >= 4*ncu tiles
  split           W = 8, NT = N/4, LDS 16*(N/2)*8 + 16*(N/4) (+ 8*N fused) + 16*(NT/8),
                  160 KB / LDS workgroups per CU; from 1024 points (512 with the switch at 2)
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'concept_amd', 'csrc')
NCU = 256


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    cxx = shutil.which('g++') or next(
        (p for p in ('/opt/rocm/llvm/bin/clang++',) if os.path.exists(p)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('fft_plan')/'fft_plan_print')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I' + CSRC,
                    os.path.join(HERE, 'fft_plan_print.cpp'), '-o', exe], check=True)

    def ask(*requests):
        text = '\n'.join(' '.join(str(int(v)) if not isinstance(v, str) else v for v in r)
                         for r in requests) + '\n'
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True)
        lines = [ln.split() for ln in out.stdout.decode().splitlines()]
        assert len(lines) == len(requests) and all(ln[0] == r[0] for ln, r in zip(lines, requests))
        return [ln[1:] for ln in lines]
    return ask


# (N, layers to split) -> layers per chunk, (n, base, extra)
CHUNKS = [
    (16, 16, 17, (1, 16, 0)), (64, 64, 65, (1, 64, 0)), (128, 128, 129, (1, 128, 0)),
    (256, 256, 257, (1, 256, 0)),                 # the mesh fits the cache bound: no chunks
    (512, 512, 93, (6, 85, 2)),                   # 86, 86, 85, 85, 85, 85
    (1024, 1024, 31, (33, 31, 1)),
    (2048, 2048, 7, (293, 6, 290)),
    (1024, 256, 31, (8, 32, 0)),                  # a slab of 256 layers
]


@pytest.mark.parametrize('N,total,chunk,plan', CHUNKS)
def test_chunks(plans, N, total, chunk, plan):
    out = [int(v) for v in plans(('chunk', N, N + 1, N + 16, NCU, total))[0]]
    assert out[0] == chunk and tuple(out[1:4]) == plan
    begin = out[4:]
    n = plan[0]
    sizes = [b - a for a, b in zip(begin, begin[1:])]
    # the chunks tile [0, total) and differ in size by at most one
    assert len(begin) == n + 1 and begin[0] == 0 and begin[-1] == total
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
    if N == 512:
        assert sizes == [86, 86, 85, 85, 85, 85]


def _choice(logn, mode, nouter, split=1, pad=None, s=None, d=None):
    """request for a pass over `nouter` outer indices; s, d: (es, sh), default the y map"""
    N = 1 << logn
    pad = N + 16 if pad is None else pad
    y = (pad//2, 31)
    s, d = s or y, d or s or y
    return ('choice', logn, mode, N, pad, NCU, split, nouter, s[0], s[1], d[0], d[1])


def _xmap(logn):
    N = 1 << logn
    return ((N + 16)//2*(N + 1), 31)


# request -> form, W, NT, LDS bytes, workgroups
CHOICES = {
    # small meshes: one workgroup per tile
    'n16': (_choice(4, 0, 16), ('Plain', 8, 64, 2048, 32)),
    'n64': (_choice(6, 0, 64), ('Plain', 8, 64, 8192, 320)),
    # >= 4*ncu tiles: persistent, at most 4 workgroups per CU
    'n128': (_choice(7, 0, 128), ('Persistent', 8, 64, 17408, 1024)),
    'n256': (_choice(8, 0, 256), ('Persistent', 8, 128, 34816, 1024)),
    # 512^3, a chunk of 85 layers = 2805 tiles
    'n512_m0': (_choice(9, 0, 85), ('Persistent', 8, 256, 69632, 512)),
    'n512_m1': (_choice(9, 1, 85), ('Persistent', 8, 256, 69632, 512)),
    'n512_x': (_choice(9, 2, 512, s=_xmap(9)), ('Persistent', 8, 256, 73728, 512)),
    'n512_split2': (_choice(9, 0, 85, split=2), ('Split', 8, 128, 35072, 1024)),
    # 1024^3, 31 layers = 2015 tiles
    'n1024_m0': (_choice(10, 0, 31), ('Split', 8, 256, 70144, 512)),
    'n1024_m1': (_choice(10, 1, 31), ('Split', 8, 256, 70144, 512)),
    'n1024_x': (_choice(10, 2, 1024, s=_xmap(10)), ('Split', 8, 256, 78336, 512)),
    'n1024_off': (_choice(10, 0, 31, split=0), ('Persistent', 8, 512, 139264, 256)),
    # 2048^3, 7 layers = 903 tiles
    'n2048_m0': (_choice(11, 0, 7), ('Split', 8, 512, 140288, 256)),
    'n2048_x': (_choice(11, 2, 2048, s=_xmap(11)), ('Split', 8, 512, 156672, 256)),
    'n2048_off': (_choice(11, 0, 7, split=0), ('Persistent', 4, 512, 147456, 256)),
    'n2048_x_off': (_choice(11, 2, 2048, split=0, s=_xmap(11)),
                    ('Persistent', 4, 512, 163840, 256)),
    # blocked maps (the slabs' transpose buffers): blocks of >= 2*(NT/W) = 64 rows split ...
    'blocked_64': (_choice(10, 0, 31, d=(520, 6)), ('SplitBlocked', 8, 256, 70144, 512)),
    'blocked_64_src': (_choice(10, 1, 31, s=(520, 6), d=(520, 31)),
                       ('SplitBlocked', 8, 256, 70144, 512)),
    # ... smaller ones do not, and blocked maps are never persistent
    'refuse_blocks': (_choice(10, 0, 31, d=(520, 5)), ('Plain', 8, 512, 131072, 2015)),
    # fewer than 2*ncu = 512 tiles: 7 layers = 455 (8 layers = 520 split)
    'refuse_tiles': (_choice(10, 0, 7), ('Plain', 8, 512, 131072, 455)),
    'enough_tiles': (_choice(10, 0, 8), ('Split', 8, 256, 70144, 512)),
    # 32-bit reach at 2048 points: (126*es + 8)*16 bytes >= 2^32 from es = 2130441 on
    'reach_inside': (_choice(11, 0, 2048, s=(2130440, 31)), ('Split', 8, 512, 140288, 256)),
    'refuse_reach': (_choice(11, 0, 2048, s=(2130441, 31)),
                     ('Persistent', 4, 512, 147456, 256)),
    # the last tile's 8 columns beyond the row: nkb*W = 520 > pad/2 = 513
    'refuse_row': (_choice(10, 0, 31, pad=1026), ('Persistent', 8, 512, 139264, 256)),
    # whole pencils below 4*ncu = 1024 tiles: 15 layers = 975 (16 layers = 1040 persist)
    'whole_few': (_choice(10, 0, 15, split=0), ('Plain', 8, 512, 131072, 975)),
    'whole_many': (_choice(10, 0, 16, split=0), ('Persistent', 8, 512, 139264, 256)),
}


@pytest.mark.parametrize('name', sorted(CHOICES))
def test_pass_form(plans, name):
    request, (form, W, NT, lds, grid) = CHOICES[name]
    out = plans(request)[0]
    assert (out[0], int(out[1]), int(out[2]), int(out[3]), int(out[4])) == (form, W, NT, lds, grid)
    # tiles per outer index and in all: ceil((N/2 + 1)/W) * nouter
    N, nouter = request[3], request[7]
    assert int(out[5]) == -(-(N//2 + 1)//W) and int(out[6]) == int(out[5])*nouter
