"""The integer arithmetic of the chunk box (concept_amd/csrc/cg_chunk_box.h), without a GPU:
tests/chunk_box_print.cpp includes only that header, is compiled with the host compiler — once
plainly and once with -fsanitize=address,undefined, a stand-alone binary — and prints what the
header computes for the requests below.  Expected values are Python expressions:
  rel(cell, ref)      = (cell - ref + N//2) % N - N//2
  extents             e = hi - lo + W;  fits = e0*e1*e2 <= 4096 and every e <= N
  entry -> cell       (r + lo - H + (a, b, c)) % N  for entry (a*e1 + b)*e2 + c
  cell -> entry       a particle whose cell is (r + rel) % N has its first stencil cell, H below,
                      at entry ((rel0 - lo0)*e1 + (rel1 - lo1))*e2 + (rel2 - lo2)
W, H are the stencil's width and reach below the particle's cell: (ORDER, 0) for the deposit and
the scalar gather, (2 + 2*H, H) with H = diff_order/2 for the fused gather-kick."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'concept_amd', 'csrc')
WIDTHS = [(1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (6, 2)]


@pytest.fixture(scope='module', params=['plain', 'sanitized'])
def box(request, tmp_path_factory):
    cxx = shutil.which('g++') or next(
        (p for p in ('/opt/rocm/llvm/bin/clang++',) if os.path.exists(p)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('chunk_box')/f'chunk_box_print_{request.param}')
    extra = (['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g']
             if request.param == 'sanitized' else [])
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', *extra, '-I' + CSRC,
                    os.path.join(HERE, 'chunk_box_print.cpp'), '-o', exe], check=True)

    def ask(*words):
        text = ' '.join(str(int(w)) if not isinstance(w, str) else w for w in words) + '\n'
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE)
        assert out.returncode == 0, out.stderr.decode()
        line = out.stdout.decode().split()
        assert line[0] == words[0]
        return [int(v) for v in line[1:]]
    return ask


@pytest.mark.parametrize('N', [2, 4, 8, 64])
def test_rel(box, N):
    got = np.array(box('rel', N)).reshape(N, N)          # [ref][cell]
    ref, cell = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    np.testing.assert_array_equal(got, (cell - ref + N//2) % N - N//2)


# (label, N, r, lo, hi as functions of the width W where the box must end at a given extent)
def _geometries(W):
    yield 'inside the grid', 64, (20, 30, 40), (-3, 0, -5), (4, 6, 0)
    yield 'across the seam on every axis', 64, (1, 62, 0), (-4, -2, -3), (2, 3, 1)
    yield 'reference on the last cell', 64, (63, 63, 63), (0, 0, 0), (5, 1, 3)
    # the whole z axis: e2 = hi - lo + W = N
    if W <= 4:
        yield 'whole axis of 256', 256, (254, 7, 100), (0, 0, -128), (4 - W, 0, 128 - W)
    yield 'whole axis of 16', 16, (5, 11, 14), (0, -1, -8), (0, 0, 8 - W)


@pytest.mark.parametrize('W,H', WIDTHS)
def test_entry_and_cell_are_inverse(box, W, H):
    for label, N, r, lo, hi in _geometries(W):
        r, lo, hi = np.array(r), np.array(lo), np.array(hi)
        e = hi - lo + W
        out = box('box', W, H, N, *r, *lo, *hi)
        assert out[0] == 1 and tuple(out[1:4]) == tuple(e) and out[4] == e.prod(), (label, out[:5])
        cells = np.array(out[5:]).reshape(e.prod(), 3)
        abc = np.array(list(itertools.product(*(range(v) for v in e))))
        np.testing.assert_array_equal(cells, (r + lo - H + abc) % N, err_msg=label)
        # every particle cell of the box: -> entry -> cell is the first stencil cell, H below
        rel = np.array(list(itertools.product(*(range(a, b + 1) for a, b in zip(lo, hi)))))
        assert rel.min() >= -(N//2) and rel.max() < N - N//2
        pcell = (r + rel) % N
        entry = np.array(box('entries', W, H, N, *r, *lo, *hi, len(pcell), *pcell.reshape(-1)))
        d = rel - lo
        np.testing.assert_array_equal(entry, (d[:, 0]*e[1] + d[:, 1])*e[2] + d[:, 2],
                                      err_msg=label)
        np.testing.assert_array_equal(cells[entry], (pcell - H) % N, err_msg=label)
        # ... and the whole stencil stays inside the box
        top = entry + ((W - 1)*e[1] + (W - 1))*e[2] + (W - 1)
        assert entry.min() == 0 and top.max() == e.prod() - 1, label


@pytest.mark.parametrize('W,H', WIDTHS)
def test_fits(box, W, H):
    def fits(N, e):
        hi = [v - W for v in e]
        out = box('box', W, H, N, 3, 5, 7, 0, 0, 0, *hi)
        assert tuple(out[1:4]) == tuple(e)
        assert out[4] == (np.prod(e) if out[0] else 0)
        return bool(out[0])
    assert fits(64, (16, 16, 16))                  # exactly 4096
    assert not fits(64, (17, 16, 16)) and not fits(64, (16, 16, 17))
    assert fits(64, (W, W, 64))                    # a whole axis
    assert not fits(64, (W, W, 65))                # e == N + 1, far below 4096 cells
    if W <= 4:
        assert fits(256, (4, 4, 256))              # 4096 with a whole axis
        assert not fits(256, (4, 4, 257)) and not fits(512, (4, 4, 257)) and not fits(256, (5, 4, 256))
    if W == 1:
        assert not fits(256, (1, 17, 241))         # 4097 = 17*241: only NGP boxes can be 1 wide
    else:
        assert not fits(4200, (W, W, -(-4097//(W*W))))   # the first product past 4096 at W x W
        assert fits(4200, (W, W, 4096//(W*W)))
