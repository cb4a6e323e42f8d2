"""``AssembleLds`` (csrc/sbm_assemble.hpp) on the host: the one description of k_assemble's dynamic LDS, from which the
kernel takes its pointers and launch_assemble the size of the block.  The struct is plain C++, compiled here with g++ and
called through ctypes -- no GPU.  For every direct-mode shape of tests/support/assembly_cases.py, the sizes around the
64 KB attribute threshold and the workgroup limit (q = 1, G = 0, R = 1022, 1023, 2660, 2661) and shapes with custom-row
weights:

  * ``bytes()`` equals the size launch_assemble asked for before the struct existed, restated below (the generalisation
    of ``_lds_bytes`` in tests/test_gpu_assembly_edges.py to any q, G and weight count);
  * every region lies inside the block, no two overlap, every region of doubles starts on a multiple of 8;
  * ``part`` starts where ``dB`` ends (the kernel used to find it that way)."""
import ctypes
import os
import subprocess

import pytest

from tests.support import assembly_cases as ac

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sysbio_modeling_amd', 'csrc')
NTHR = 256
DOUBLES = ('sim', 'res', 'B', 'sde', 'sds', 'red', 'd', 'sg', 'w', 'dB', 'part')
INTS = ('roff', 'rexp', 'rv0', 'rnv', 'rvar', 'rsf', 'rw0')
ORDER = ('sim', 'res', 'B', 'sde', 'sds', 'red', 'd', 'sg') + INTS + ('w', 'dB', 'part')

HARNESS = r'''
#include "sbm_assemble.hpp"
extern "C" void lds_layout(int R, int G, int q, int NW, int nthr, long long* out) {
  const AssembleLds l(R, G, q, NW, nthr);
  const size_t off[] = {%s};
  int n = 0;
  for (size_t o : off) out[n++] = (long long)o;
  out[n++] = (long long)l.bytes();
  out[n++] = l.Gn; out[n++] = l.cw; out[n++] = l.rpp;
}
''' % ', '.join('l.' + nm for nm in ORDER)


@pytest.fixture(scope='module')
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp('assemble_lds')
    src, so = d / 'harness.cpp', d / 'harness.so'
    src.write_text(HARNESS)
    subprocess.run(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wall', '-I', CSRC, str(src), '-o', str(so)], check=True,
                   capture_output=True)
    lib = ctypes.CDLL(str(so))
    lib.lds_layout.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_longlong)]

    def get(R, G, q, NW):
        out = (ctypes.c_longlong * (len(ORDER) + 4))()
        lib.lds_layout(R, G, q, NW, NTHR, out)
        vals = list(out)
        off = dict(zip(ORDER, vals))
        return off, vals[len(ORDER)], vals[len(ORDER) + 1:]
    return get


def formula_bytes(R, G, q, NW):
    """what launch_assemble computed by hand: sims, residuals, B / sde / sds per group, 4 doubles of reduction scratch,
    dB [Gn][q] and the partial sums [2][Gn][rpp][q]; the staged row tables (2 R doubles, 7 R + 2 ints); the weights"""
    Gn = max(G, 1)
    rpp = NTHR // min(q, NTHR)
    return 8 * (2 * R + 3 * Gn + 4 + Gn * q + 2 * Gn * rpp * q) + 8 * 2 * R + 4 * (7 * R + 2) + 8 * NW


def region_counts(R, G, q, NW):
    """entries of every region, from the kernel's use of it"""
    Gn = max(G, 1)
    rpp = NTHR // min(q, NTHR)
    n = dict(sim=R, res=R, B=Gn, sde=Gn, sds=Gn, red=4, d=R, sg=R, w=NW, dB=Gn * q, part=2 * Gn * rpp * q)
    n.update({nm: R for nm in INTS})
    return n


SHAPES = [(s[1], s[2], s[0], 0) for s in ac.SHAPES] + \
    [(R, 0, 1, 0) for R in (1022, 1023, 2660, 2661)] + \
    [(4, 0, 3, 1), (5, 2, 7, 13), (86, 3, 3, 64), (257, 7, 300, 129), (1, 1, 1, 64)]     # custom-row weights


def test_shapes_cover_the_issue_list():
    assert len(SHAPES) == len(ac.SHAPES) + 9 and len(ac.SHAPES) == 34
    assert formula_bytes(0, 0, 1, 0) == 4168 and formula_bytes(1, 0, 1, 0) - formula_bytes(0, 0, 1, 0) == 60
    assert formula_bytes(1022, 0, 1, 0) <= 64 * 1024 < formula_bytes(1023, 0, 1, 0)
    assert formula_bytes(2660, 0, 1, 0) + 16 <= 160 * 1024 < formula_bytes(2661, 0, 1, 0) + 16


@pytest.mark.parametrize('R,G,q,NW', SHAPES, ids=['R%d-G%d-q%d-NW%d' % s for s in SHAPES])
def test_layout(layout, R, G, q, NW):
    off, total, (Gn, cw, rpp) = layout(R, G, q, NW)
    assert (Gn, cw, rpp) == (max(G, 1), min(q, NTHR), NTHR // min(q, NTHR))
    assert total == formula_bytes(R, G, q, NW)
    counts = region_counts(R, G, q, NW)
    spans = []
    for nm in ORDER:
        width = 8 if nm in DOUBLES else 4
        lo, hi = off[nm], off[nm] + width * counts[nm]
        assert 0 <= lo <= hi <= total, nm
        if nm in DOUBLES:
            assert lo % 8 == 0, nm
        else:
            assert lo % 4 == 0, nm
        spans.append((lo, hi, nm))
    spans.sort()
    for (lo0, hi0, a), (lo1, hi1, b) in zip(spans, spans[1:]):
        assert hi0 <= lo1, (a, b)
    assert off['part'] == off['dB'] + 8 * counts['dB']
    # the slack the size has always carried: the int tables are counted as 7 R + 2 entries
    assert total - (off['part'] + 8 * counts['part']) == 4 * (2 - R % 2)
