"""csrc/sbm_row_operands.hpp on the host: the row table and the row evaluation every row-class kernel shares, compiled with g++
(device qualifiers defined away as in tests/test_generated_header_host.py) and called through ctypes -- no GPU.

  * SBM_ROW_TABLE_LOAD fills a row of SbmRowTable with exactly SBM_RL_CLASS[row], SBM_RL_YS[slot][row] (+ the base the packed
    kernels add) and P[SBM_RL_PS[slot][row]], the tables read from the text of the header; a lane past the last row gets
    class -1; SbmRowTable::zero_operands (the row-group kernels' RL_F_ZERO_OFF_ROW option) leaves ps == 0 and every operand
    index at the slot's own place in Y;
  * sbm_row_eval returns BIT FOR BIT what a direct class_dispatch call on zeroed outputs returns, without the off-row select
    and with it (where a class of -1 must give f == 0 and nothing else may change);
  * SbmRowTable::exchange publishes the lane's components at lane + 64 r and gathers the operands through yidx."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from sysbio_modeling_amd import build

HARNESS = r'''
#include <cmath>
#define __device__
#define __forceinline__ inline
#define __constant__ static const
#define SBM_RCP(x) (1.0 / (x))
#define SBM_SEL(c, a, b) ((c) ? (a) : (b))
#define SBM_PICK(scol, c, v, otherwise) ((scol) == (c) ? (v) : (otherwise))
#define SBM_PICK_COL(col, c, v, otherwise) ((col) == (c) ? (v) : (otherwise))
#define SBM_LANE_BCAST(v, src) (v)
#define SBM_LDS_FENCE()
using std::fma;
#include "%(header)s"
#include "sbm_row_operands.hpp"
typedef SbmModel M;
constexpr int RPL = 2;
extern "C" {
int nv() { return M::NV; }
int np_() { return M::NP; }
int maxys() { return M::RL_MAXYS; }
int maxps() { return M::RL_MAXPS; }
int maxjy() { return M::RL_MAXJY; }
int maxjp() { return M::RL_MAXJP; }
// row r of a two-row table as the kernels fill it: lane `idx` of a trajectory with n rows
void load_row(int r, const double* P, int idx, int ybase, int zero_off_row, int own, int* cls, int* yidx, double* ps) {
  SbmRowTable<M, RPL> tab;
  for (int q = 0; q < RPL; ++q) {       // poison: whatever load leaves untouched shows
    tab.cls[q] = -77;
    for (int s = 0; s < M::RL_MAXYS; ++s) tab.yidx[q][s] = -77;
    for (int s = 0; s < M::RL_MAXPS; ++s) tab.ps[q][s] = -77.0;
  }
  const bool has_row = idx < M::NV;
  const int row = has_row ? idx : 0;
  SBM_ROW_TABLE_LOAD(M, tab, r, P, row, has_row, ybase)
  if (zero_off_row && !has_row) tab.zero_operands(r, own);
  for (int q = 0; q < RPL; ++q) {
    cls[q] = tab.cls[q];
    for (int s = 0; s < M::RL_MAXYS; ++s) yidx[q * M::RL_MAXYS + s] = tab.yidx[q][s];
    for (int s = 0; s < M::RL_MAXPS; ++s) ps[q * M::RL_MAXPS + s] = tab.ps[q][s];
  }
}
void eval_direct(int cls, double t, const double* ys_, const double* ps_, double* f, double* jy, double* jp) {
  double ys[M::RL_MAXYS], ps[M::RL_MAXPS], jyo[M::RL_MAXJY], jpo[M::RL_MAXJP], ff = 0.0;
  for (int s = 0; s < M::RL_MAXYS; ++s) ys[s] = ys_[s];
  for (int s = 0; s < M::RL_MAXPS; ++s) ps[s] = ps_[s];
  for (int s = 0; s < M::RL_MAXJY; ++s) jyo[s] = 0.0;
  for (int s = 0; s < M::RL_MAXJP; ++s) jpo[s] = 0.0;
  M::class_dispatch(cls, t, ys, ps, ff, jyo, jpo);
  *f = ff;
  for (int s = 0; s < M::RL_MAXJY; ++s) jy[s] = jyo[s];
  for (int s = 0; s < M::RL_MAXJP; ++s) jp[s] = jpo[s];
}
// through the table, outputs poisoned first: the helper does the zeroing
void eval_shared(int cls, double t, const double* ys_, const double* ps_, int select, double* f, double* jy, double* jp) {
  SbmRowTable<M, RPL> tab;
  SbmRowTable<M, RPL>::Operands ops;
  tab.cls[1] = cls;
  for (int s = 0; s < M::RL_MAXYS; ++s) ops.ys[1][s] = ys_[s];
  for (int s = 0; s < M::RL_MAXPS; ++s) tab.ps[1][s] = ps_[s];
  double jyo[M::RL_MAXJY], jpo[M::RL_MAXJP], ff = 1e300;
  for (int s = 0; s < M::RL_MAXJY; ++s) jyo[s] = 1e300;
  for (int s = 0; s < M::RL_MAXJP; ++s) jpo[s] = 1e300;
  if (select) tab.eval<true>(1, t, ops, ff, jyo, jpo);
  else tab.eval<false>(1, t, ops, ff, jyo, jpo);
  *f = ff;
  for (int s = 0; s < M::RL_MAXJY; ++s) jy[s] = jyo[s];
  for (int s = 0; s < M::RL_MAXJP; ++s) jp[s] = jpo[s];
}
// Y: 128 doubles; the lane's two components go to lane and lane + 64, the operands come back through yidx
void exchange(double* Y, int lane, const double* own, const int* yidx, double* ys) {
  SbmRowTable<M, RPL> tab;
  for (int q = 0; q < RPL; ++q)
    for (int s = 0; s < M::RL_MAXYS; ++s) tab.yidx[q][s] = yidx[q * M::RL_MAXYS + s];
  const auto ops = tab.exchange(Y, lane, own);
  for (int q = 0; q < RPL; ++q)
    for (int s = 0; s < M::RL_MAXYS; ++s) ys[q * M::RL_MAXYS + s] = ops.ys[q][s];
}
}
'''


def _table(text, name):
    m = re.search(r'__constant__ short %s\[(\d+)\] = \{([^}]*)\};' % name, text)
    vals = [int(v) for v in m.group(2).split(',')]
    assert len(vals) == int(m.group(1))
    return vals


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.fixture(scope='module', params=['simple', 'michaelis_menten'])
def model(request, tmp_path_factory):
    from sysbio_modeling_amd.symbolic import zoo_model
    gm = zoo_model(request.param)
    tmp = tmp_path_factory.mktemp(request.param)
    header = tmp / (gm.name + '.hpp')
    header.write_text(gm.hip_source)
    src = tmp / 'harness.cpp'
    src.write_text(HARNESS % dict(header=str(header)))
    so = tmp / 'harness.so'
    # -ffp-contract=off: only the fma() calls the generator wrote are fused, in both forms alike
    subprocess.run(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=off', '-Wno-unknown-pragmas',
                    '-I' + build.CSRC_DIR, str(src), '-o', str(so)], check=True, capture_output=True)
    lib = ctypes.CDLL(str(so))
    ip, dp, ci, cd = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double
    lib.load_row.argtypes = [ci, dp, ci, ci, ci, ci, ip, ip, dp]
    lib.eval_direct.argtypes = [ci, cd, dp, dp, dp, dp, dp]
    lib.eval_shared.argtypes = [ci, cd, dp, dp, ci, dp, dp, dp]
    lib.exchange.argtypes = [dp, ci, dp, ip, dp]
    return lib, gm.hip_source


def _load(lib, r, P, idx, ybase=0, zero=0, own=0):
    mys, mps = lib.maxys(), lib.maxps()
    cls, yidx, ps = np.zeros(2, np.int32), np.zeros(2 * mys, np.int32), np.zeros(2 * mps)
    lib.load_row(r, _dp(P), idx, ybase, zero, own, _ip(cls), _ip(yidx), _dp(ps))
    return cls, yidx.reshape(2, mys), ps.reshape(2, mps)


@pytest.mark.parametrize('r', [0, 1])
@pytest.mark.parametrize('ybase', [0, 16])
def test_load_gives_the_tables_of_the_header(model, r, ybase):
    lib, text = model
    nv, mys, mps = lib.nv(), lib.maxys(), lib.maxps()
    CLASS, YS, PS = _table(text, 'SBM_RL_CLASS'), _table(text, 'SBM_RL_YS'), _table(text, 'SBM_RL_PS')
    assert len(CLASS) == nv and len(YS) == mys * nv and len(PS) == mps * nv
    P = np.random.default_rng(5).uniform(0.5, 2.0, lib.np_())
    for row in range(nv):
        cls, yidx, ps = _load(lib, r, P, row, ybase)
        assert cls[r] == CLASS[row]
        assert list(yidx[r]) == [YS[s * nv + row] + ybase for s in range(mys)]
        assert list(ps[r]) == [P[PS[s * nv + row]] for s in range(mps)]
        # the other row of the table is not touched
        assert cls[1 - r] == -77 and (yidx[1 - r] == -77).all() and (ps[1 - r] == -77.0).all()


@pytest.mark.parametrize('idx_past', [0, 1, 62])
def test_a_lane_past_the_last_row_has_class_minus_one(model, idx_past):
    lib, text = model
    nv = lib.nv()
    P = np.random.default_rng(6).uniform(0.5, 2.0, lib.np_())
    cls, yidx, ps = _load(lib, 0, P, nv + idx_past, 16)
    assert cls[0] == -1
    # operands of row 0 (valid indices, finite values nobody uses)
    ref = _load(lib, 0, P, 0, 16)
    assert (yidx[0] == ref[1][0]).all() and (ps[0] == ref[2][0]).all()


def test_zero_off_row_option(model):
    lib, text = model
    nv = lib.nv()
    P = np.random.default_rng(7).uniform(0.5, 2.0, lib.np_())
    own = 64 + 37                                       # (lane 37, r = 1)
    cls, yidx, ps = _load(lib, 1, P, nv + 3, 0, zero=1, own=own)
    assert cls[1] == -1 and (yidx[1] == own).all() and (ps[1] == 0.0).all()
    # a lane WITH a row is left as loaded
    a, b = _load(lib, 1, P, nv - 1, 0, zero=1, own=own), _load(lib, 1, P, nv - 1, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('select', [0, 1])
def test_row_evaluation_equals_a_direct_class_dispatch_bit_for_bit(model, select):
    lib, text = model
    mys, mps, mjy, mjp = lib.maxys(), lib.maxps(), lib.maxjy(), lib.maxjp()
    n_classes = max(_table(text, 'SBM_RL_CLASS')) + 1
    rng = np.random.default_rng(11 + select)
    for trial in range(8):
        ys, ps, t = rng.uniform(0.1, 3.0, mys), rng.uniform(0.1, 3.0, mps), float(rng.uniform(0.0, 5.0))
        for cls in list(range(n_classes)) + [-1]:
            fd, jyd, jpd = np.zeros(1), np.zeros(mjy), np.zeros(mjp)
            fs, jys, jps = np.zeros(1), np.zeros(mjy), np.zeros(mjp)
            lib.eval_direct(cls, t, _dp(ys), _dp(ps), _dp(fd), _dp(jyd), _dp(jpd))
            lib.eval_shared(cls, t, _dp(ys), _dp(ps), select, _dp(fs), _dp(jys), _dp(jps))
            if select and cls < 0:
                assert fs[0] == 0.0
            else:
                assert fs.tobytes() == fd.tobytes(), (cls, fs, fd)
            assert jys.tobytes() == jyd.tobytes() and jps.tobytes() == jpd.tobytes(), cls
            if cls >= 0:
                assert fd[0] != 0.0                      # the operands did enter


def test_exchange_publishes_own_components_and_gathers_by_index(model):
    lib, text = model
    mys = lib.maxys()
    rng = np.random.default_rng(3)
    Y = rng.standard_normal(128)
    before = Y.copy()
    lane = 5
    own = np.array([1.25, -2.5])
    yidx = rng.integers(0, 128, size=2 * mys).astype(np.int32)
    yidx[0] = lane                                       # one operand is the lane's own, just published, component
    yidx[-1] = lane + 64
    ys = np.zeros(2 * mys)
    lib.exchange(_dp(Y), lane, _dp(own), _ip(yidx), _dp(ys))
    after = before.copy()
    after[lane], after[lane + 64] = own
    assert np.array_equal(Y, after)
    assert np.array_equal(ys, after[yidx])
