"""``assemble_form`` (csrc/sbm_assemble.hpp) on the host: which instantiation of k_assemble launch_assemble takes for a
shape -- how many rows of J a thread of pass A keeps in registers (0: the trip through global memory; 4 or 12), whether
the postfix interpreter and the logarithmic loss are compiled in.  It is plain C++ beside AssembleLds, compiled here with
g++ and called through ctypes -- no GPU -- and checked against a table written out by hand.

A workgroup of 256 threads handles cw = min(q, 256) columns on rpp = 256 // cw row lanes; a thread's rows are
ceil(R / rpp).  The table has q = 1 (rpp 256), q = 40 (rpp 6, the headline's), q = 255, 256 (rpp 1) and 257 (several column
passes: never a tile); R = 0 and 1; R = rpp K - 1, rpp K and rpp K + 1 for both tiles K; the headline shape (64 rows,
40 parameters) and the 512 x 68 and 580 x 68 shapes of the larger benchmark project, which stay on the form through
global memory."""
import ctypes
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sysbio_modeling_amd', 'csrc')
NTHR = 256
SQUARE, LOG = 0, 1

HARNESS = r'''
#include "sbm_assemble.hpp"
extern "C" void form(int R, int q, int programs, int loss, int nthr, int* out) {
  const AssembleForm f = assemble_form(R, q, programs, loss, nthr);
  out[0] = f.rows; out[1] = f.prog; out[2] = f.log;
}
extern "C" void tiles(int* out) { out[0] = SBM_ASSEMBLE_TILE_SMALL; out[1] = SBM_ASSEMBLE_TILE_LARGE; }
'''

# (R, q, programs, loss) -> (rows, prog, log)
TABLE = [
    # q = 1: cw 1, rpp 256
    ((0, 1, 0, SQUARE), (0, 0, 0)),
    ((1, 1, 0, SQUARE), (4, 0, 0)),
    ((256, 1, 0, SQUARE), (4, 0, 0)),
    ((1023, 1, 0, SQUARE), (4, 0, 0)),
    ((1024, 1, 0, SQUARE), (4, 0, 0)),
    ((1025, 1, 0, SQUARE), (12, 0, 0)),
    ((3071, 1, 0, LOG), (12, 0, 1)),
    ((3072, 1, 0, LOG), (12, 0, 1)),
    ((3073, 1, 0, LOG), (0, 0, 1)),
    # q = 40: rpp 6
    ((0, 40, 0, SQUARE), (0, 0, 0)),
    ((1, 40, 0, SQUARE), (4, 0, 0)),
    ((23, 40, 0, SQUARE), (4, 0, 0)),
    ((24, 40, 0, SQUARE), (4, 0, 0)),
    ((25, 40, 0, SQUARE), (12, 0, 0)),
    ((64, 40, 0, SQUARE), (12, 0, 0)),          # the headline: 11 rows a thread
    ((71, 40, 0, SQUARE), (12, 0, 0)),
    ((72, 40, 0, SQUARE), (12, 0, 0)),
    ((73, 40, 0, SQUARE), (0, 0, 0)),
    # rpp 1: q = 255, 256; q = 257 takes two passes over the columns
    ((0, 255, 0, SQUARE), (0, 0, 0)),
    ((1, 255, 0, SQUARE), (4, 0, 0)),
    ((3, 255, 0, SQUARE), (4, 0, 0)),
    ((4, 255, 0, SQUARE), (4, 0, 0)),
    ((5, 255, 0, SQUARE), (12, 0, 0)),
    ((11, 255, 0, SQUARE), (12, 0, 0)),
    ((12, 255, 0, SQUARE), (12, 0, 0)),
    ((13, 255, 0, SQUARE), (0, 0, 0)),
    ((1, 256, 0, LOG), (4, 0, 1)),
    ((3, 256, 0, LOG), (4, 0, 1)),
    ((4, 256, 0, LOG), (4, 0, 1)),
    ((5, 256, 0, LOG), (12, 0, 1)),
    ((11, 256, 0, LOG), (12, 0, 1)),
    ((12, 256, 0, LOG), (12, 0, 1)),
    ((13, 256, 0, LOG), (0, 0, 1)),
    ((0, 257, 0, SQUARE), (0, 0, 0)),
    ((1, 257, 0, SQUARE), (0, 0, 0)),
    ((4, 257, 0, SQUARE), (0, 0, 0)),
    ((12, 257, 1, LOG), (0, 1, 1)),
    # rpp 2 (q = 128) and rpp 3 (q = 68)
    ((7, 128, 0, SQUARE), (4, 0, 0)),
    ((8, 128, 0, SQUARE), (4, 0, 0)),
    ((9, 128, 0, SQUARE), (12, 0, 0)),
    ((23, 128, 0, SQUARE), (12, 0, 0)),
    ((24, 128, 0, SQUARE), (12, 0, 0)),
    ((25, 128, 0, SQUARE), (0, 0, 0)),
    ((36, 68, 0, SQUARE), (12, 0, 0)),
    ((37, 68, 0, SQUARE), (0, 0, 0)),
    ((512, 68, 0, SQUARE), (0, 0, 0)),          # the larger benchmark project: 171 rows a thread
    ((580, 68, 0, SQUARE), (0, 0, 0)),          # ... with a prior on every parameter
    # the flags do not move the tile, and the tile does not move the flags
    ((64, 40, 1, SQUARE), (12, 1, 0)),
    ((64, 40, 0, LOG), (12, 0, 1)),
    ((64, 40, 7, LOG), (12, 1, 1)),
    ((24, 40, 1, LOG), (4, 1, 1)),
    ((73, 40, 1, SQUARE), (0, 1, 0)),
]


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('assemble_tile')
    src, so = d / 'harness.cpp', d / 'harness.so'
    src.write_text(HARNESS)
    subprocess.run(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wall', '-I', CSRC, str(src), '-o', str(so)], check=True,
                   capture_output=True)
    lib = ctypes.CDLL(str(so))
    lib.form.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    lib.tiles.argtypes = [ctypes.POINTER(ctypes.c_int)]
    return lib


def _form(lib, R, q, programs, loss):
    out = (ctypes.c_int * 3)()
    lib.form(R, q, programs, loss, NTHR, out)
    return tuple(out)


def test_instantiated_tiles(lib):
    out = (ctypes.c_int * 2)()
    lib.tiles(out)
    assert tuple(out) == (4, 12)


def test_table_covers_every_edge():
    shapes = [k for k, _ in TABLE]
    assert len(set(shapes)) == len(shapes)
    for q, rpp in ((1, 256), (40, 6), (255, 1), (256, 1), (128, 2)):
        assert NTHR // min(q, NTHR) == rpp
        for K in (4, 12):
            for R in (rpp * K - 1, rpp * K, rpp * K + 1):
                assert any(s[0] == R and s[1] == q for s in shapes), (q, K, R)
    for q in (1, 40, 255, 257):
        assert any(s[:2] == (0, q) for s in shapes) and any(s[:2] == (1, q) for s in shapes), q


@pytest.mark.parametrize('shape,want', TABLE, ids=['R%d-q%d-prog%d-loss%d' % s for s, _ in TABLE])
def test_form(lib, shape, want):
    assert _form(lib, *shape) == want


def test_form_is_the_smallest_tile_that_holds_the_rows(lib):
    """every (R, q) on a grid: the tile is the smallest instantiated one >= ceil(R / rpp), 0 beyond the largest, for
    R = 0 and for q > 256; prog and log are the two inputs and nothing else"""
    for q in list(range(1, 70)) + [85, 86, 127, 128, 129, 255, 256, 257, 300, 513]:
        rpp = NTHR // min(q, NTHR)
        for R in sorted(set(list(range(0, 40)) + [rpp * k + d for k in (3, 4, 5, 11, 12, 13) for d in (-1, 0, 1)])):
            per_thread = -(-R // rpp)
            want = 0 if (R == 0 or q > NTHR or per_thread > 12) else (4 if per_thread <= 4 else 12)
            for programs, loss in ((0, SQUARE), (3, LOG)):
                assert _form(lib, R, q, programs, loss) == (want, int(programs != 0), int(loss == LOG)), (R, q)
