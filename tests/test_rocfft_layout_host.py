"""The data layouts of the rocFFT backend's plans (concept_amd/csrc/cg_rocfft_layout.h), without a
GPU: tests/rocfft_layout_print.cpp includes only that header, is compiled with the host compiler
and prints the layouts for the shapes below.

The expected values are literals, worked out by hand from the functions cg_context.hip held
before the header existed (make_plans, dist_plans_2d, dist_layers_1d, dist_plans_x), never from
the header.  With P = pad, cp = P/2, JB = N/nprocs, lengths fastest first, those functions gave
rocFFT, in place and in double precision:
  3-D real      lengths {N, N, N}, batch 1; real strides {1, P, P*ny}, distance P*N*N;
                hermitian strides {1, cp, cp*ny}, distance cp*N*N
  2-D real      lengths {N, N}, batch nlayers; real strides {1, P}, distance P*ny; hermitian
                strides {1, cp}, distance cp*ny
  z rows        length {N}, batch N; real stride {1}, distance P; hermitian stride {1}, distance cp
  y columns     complex both sides: length {N}, batch N/2 + 1; stride {cp}, distance 1
  x             complex both sides: length {N}, batch JB*cp; stride {(JB + 1)*cp}, distance 1
A forward real plan reads the real side and writes the hermitian one, an inverse plan the other
way round.  pad and ny are those of cg_create: N + 16 and N + 1 when N is a multiple of 16,
else N + 2 and N.

The shapes are those of the GPU tests (slab_fft_refs.py ROCFFT_SHAPES, the forced-rocFFT slabs of
16 and 64 points, and 24 points on one domain), so that both branches of pad and ny are hit; the
2-D layouts at one layer and at the slab's full layer count."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'concept_amd', 'csrc')

# (N, domains) -> pad, ny, owned layers and the literals of the docstring's expressions
SHAPES = {
    (24, 1): dict(pad=26, ny=24, nxl=24, real3=((1, 26, 624), 14976), herm3=((1, 13, 312), 7488),
                  real2=((1, 26), 624), herm2=((1, 13), 312), z=(26, 13), y=(13, 13),
                  x=(325, 312)),
    (24, 2): dict(pad=26, ny=24, nxl=12, real3=((1, 26, 624), 14976), herm3=((1, 13, 312), 7488),
                  real2=((1, 26), 624), herm2=((1, 13), 312), z=(26, 13), y=(13, 13),
                  x=(169, 156)),
    (36, 3): dict(pad=38, ny=36, nxl=12, real3=((1, 38, 1368), 49248),
                  herm3=((1, 19, 684), 24624), real2=((1, 38), 1368), herm2=((1, 19), 684),
                  z=(38, 19), y=(19, 19), x=(247, 228)),
    (48, 2): dict(pad=64, ny=49, nxl=24, real3=((1, 64, 3136), 147456),
                  herm3=((1, 32, 1568), 73728), real2=((1, 64), 3136), herm2=((1, 32), 1568),
                  z=(64, 32), y=(32, 25), x=(800, 768)),
    (16, 4): dict(pad=32, ny=17, nxl=4, real3=((1, 32, 544), 8192), herm3=((1, 16, 272), 4096),
                  real2=((1, 32), 544), herm2=((1, 16), 272), z=(32, 16), y=(16, 9),
                  x=(80, 64)),
    (64, 8): dict(pad=80, ny=65, nxl=8, real3=((1, 80, 5200), 327680),
                  herm3=((1, 40, 2600), 163840), real2=((1, 80), 5200), herm2=((1, 40), 2600),
                  z=(80, 40), y=(40, 33), x=(360, 320)),
}


@pytest.fixture(scope='module')
def layouts(tmp_path_factory):
    cxx = shutil.which('g++') or next(
        (p for p in ('/opt/rocm/llvm/bin/clang++',) if os.path.exists(p)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('rocfft_layout')/'rocfft_layout_print')
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-I' + CSRC,
                    os.path.join(HERE, 'rocfft_layout_print.cpp'), '-o', exe], check=True)

    def ask(plan, inverse, N, P, nlayers=0):
        s = SHAPES[N, P]
        text = f"{plan} {int(inverse)} {N} {s['ny']} {s['pad']} {P} {nlayers}\n"
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True)
        words = out.stdout.decode().split()
        assert words[0] == plan
        kind, dims, batch, in_dist, out_dist = words[1], *(int(w) for w in words[2:6])
        per_dim = [int(w) for w in words[6:]]
        assert len(per_dim) == 3*dims
        return dict(kind=kind, dims=dims, batch=batch, in_dist=in_dist, out_dist=out_dist,
                    lengths=tuple(per_dim[0::3]), in_stride=tuple(per_dim[1::3]),
                    out_stride=tuple(per_dim[2::3]))
    return ask


def expect(kind, N, batch, src, dst):
    """a layout from (strides, distance) of the side read and of the side written"""
    return dict(kind=kind, dims=len(src[0]), batch=batch, in_dist=src[1], out_dist=dst[1],
                lengths=(N,)*len(src[0]), in_stride=tuple(src[0]), out_stride=tuple(dst[0]))


def real_pair(inverse, real, herm):
    return ('RealInverse', herm, real) if inverse else ('RealForward', real, herm)


shape_param = pytest.mark.parametrize('N,P', sorted(SHAPES))
inverse_param = pytest.mark.parametrize('inverse', [False, True], ids=['forward', 'inverse'])


@inverse_param
@shape_param
def test_3d(layouts, N, P, inverse):
    s = SHAPES[N, P]
    kind, src, dst = real_pair(inverse, s['real3'], s['herm3'])
    assert layouts('3d', inverse, N, P) == expect(kind, N, 1, src, dst)


@inverse_param
@shape_param
def test_2d_layers(layouts, N, P, inverse):
    s = SHAPES[N, P]
    kind, src, dst = real_pair(inverse, s['real2'], s['herm2'])
    for nlayers in (1, s['nxl']):
        assert layouts('2d', inverse, N, P, nlayers) == expect(kind, N, nlayers, src, dst)


@inverse_param
@shape_param
def test_1d_pair_of_a_layer(layouts, N, P, inverse):
    s = SHAPES[N, P]
    pad, cp = s['z']
    kind, src, dst = real_pair(inverse, ((1,), pad), ((1,), cp))
    assert layouts('z', inverse, N, P) == expect(kind, N, N, src, dst)
    stride, batch = s['y']
    columns = ((stride,), 1)
    assert layouts('y', inverse, N, P) == expect(
        'ComplexInverse' if inverse else 'ComplexForward', N, batch, columns, columns)


@inverse_param
@shape_param
def test_x_on_the_transpose_buffer(layouts, N, P, inverse):
    stride, batch = SHAPES[N, P]['x']
    columns = ((stride,), 1)
    assert layouts('x', inverse, N, P) == expect(
        'ComplexInverse' if inverse else 'ComplexForward', N, batch, columns, columns)


def test_the_library_is_named_in_one_source_file():
    """no other file of csrc includes the library's header or names one of its functions or types
    outside comments (the value `rocfft` of CONCEPT_GPU_FFT, which picks the backend, is no such
    name)"""
    from concept_amd import build
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')) and name != 'cg_rocfft.hip':
            with open(os.path.join(CSRC, name), encoding='utf-8') as f:
                code = build._code_only(f.read())
                assert 'rocfft_' not in code and 'rocfft/' not in code, name
    assert 'cg_rocfft.hip' in build.SOURCES
