"""Operations shared between row-lane classes (emit_rowlane.py::_plan_hoist): ``class_dispatch`` evaluates every class body
on every lane, so an expensive operation all classes have in common -- the reciprocal of a saturation term, mostly -- is
emitted ONCE on operands selected by class.  rcp(sel(c, a, b)) and sel(c, rcp(a), rcp(b)) are the same value in every
lane, and the shared statement is each class's own text after substitution of its operands, so nothing may change: the
shared and the unshared form (``emit_hip(..., class_hoist=False)``) are built for the host and compared BIT FOR BIT, f and
every J_y / J_p slot of every row, at 1000 random points.  No GPU needed."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

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
typedef SbmModel M;
extern "C" {
int nv() { return M::NV; }
int np_() { return M::NP; }
int maxjy() { return M::RL_MAXJY; }
int maxjp() { return M::RL_MAXJP; }
// every row at n points: out[point][row][1 + MAXJY + MAXJP]
void eval_rows(int n, const double* y, const double* p, double t, double* out) {
  constexpr int W = 1 + M::RL_MAXJY + M::RL_MAXJP;
  for (int k = 0; k < n; ++k)
    for (int row = 0; row < M::NV; ++row) {
      double ys[M::RL_MAXYS], ps[M::RL_MAXPS], f = 0.0, jy[M::RL_MAXJY], jp[M::RL_MAXJP];
      for (int s = 0; s < M::RL_MAXYS; ++s) ys[s] = y[k * M::NV + M::rl_ys(s, row)];
      for (int s = 0; s < M::RL_MAXPS; ++s) ps[s] = p[k * M::NP + M::rl_ps(s, row)];
      for (int s = 0; s < M::RL_MAXJY; ++s) jy[s] = 0.0;
      for (int s = 0; s < M::RL_MAXJP; ++s) jp[s] = 0.0;
      M::class_dispatch(M::rl_class(row), t, ys, ps, f, jy, jp);
      double* o = out + ((size_t)k * M::NV + row) * W;
      o[0] = f;
      for (int s = 0; s < M::RL_MAXJY; ++s) o[1 + s] = jy[s];
      for (int s = 0; s < M::RL_MAXJP; ++s) o[1 + M::RL_MAXJY + s] = jp[s];
    }
}
}
'''


def _specs():
    from sysbio_modeling_amd import models_zoo
    from tests.test_gpu_user_models import _random_network
    return {'cascade20': models_zoo.cascade_spec, 'stiff50': models_zoo.stiff_spec,
            'michaelis_menten': models_zoo.michaelis_menten_spec, 'rand30_4': lambda: _random_network(4, 30)}


def _dispatch(src):
    return re.search(r'static void class_dispatch.*?\n  }\n', src, re.S).group(0)


def _library(src, tmp_path, tag):
    header = tmp_path / ('%s.hpp' % tag)
    header.write_text(src)
    cpp = tmp_path / ('%s.cpp' % tag)
    cpp.write_text(HARNESS % dict(header=str(header)))
    so = tmp_path / ('%s.so' % tag)
    # -ffp-contract=off: only the fma() calls the generator wrote are fused, in both forms alike
    subprocess.run(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=off', '-Wno-unknown-pragmas',
                    str(cpp), '-o', str(so)], check=True, capture_output=True)
    lib = ctypes.CDLL(str(so))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.eval_rows.argtypes = [ctypes.c_int, dp, dp, ctypes.c_double, dp]
    return lib


@pytest.fixture(scope='module')
def forms():
    from sysbio_modeling_amd.symbolic.emit import emit_hip, Derived
    out = {}
    for name, make in _specs().items():
        spec = make()
        d = Derived(spec)
        out[name] = (emit_hip(spec, d, class_hoist=True), emit_hip(spec, d, class_hoist=False))
    return out


# SBM_RCP in class_dispatch: (without sharing, with sharing).  cascade20 / michaelis_menten: both classes divide by one
# saturation term; stiff50: both by 2 y + 1; the random network: 7 classes, 14 reciprocals of 4 shapes
EXPECTED_RCP = {'cascade20': (2, 1), 'stiff50': (2, 1), 'michaelis_menten': (2, 1)}


@pytest.mark.parametrize('name', ['cascade20', 'stiff50', 'michaelis_menten', 'rand30_4'])
def test_one_reciprocal_per_shared_group(forms, name):
    shared, plain = (_dispatch(s) for s in forms[name])
    n_plain, n_shared = plain.count('SBM_RCP('), shared.count('SBM_RCP(')
    groups = re.findall(r'const double h\d+ = (.*);   // classes ([\d, ]+)', shared)
    assert groups, shared
    # every group replaces its reciprocals (a shared tree may hold more than one), once per participating class, by one set
    saved = sum(text.count('SBM_RCP(') * (len(cls.split(',')) - 1) for text, cls in groups)
    assert n_shared == n_plain - saved, (n_plain, n_shared, groups)
    assert n_shared < n_plain
    if name in EXPECTED_RCP:
        assert (n_plain, n_shared) == EXPECTED_RCP[name]
    # nothing outside class_dispatch changed
    a, b = forms[name]
    assert a.replace(_dispatch(a), '') == b.replace(_dispatch(b), '')


@pytest.mark.parametrize('name', ['cascade20', 'stiff50', 'michaelis_menten', 'rand30_4'])
def test_shared_form_is_bitwise_the_unshared_form(forms, tmp_path, name):
    shared, plain = forms[name]
    la, lb = _library(shared, tmp_path, 'shared'), _library(plain, tmp_path, 'plain')
    n, n_par = la.nv(), la.np_()
    width = 1 + la.maxjy() + la.maxjp()
    rng = np.random.default_rng(20)
    points = 1000
    y = rng.uniform(0.05, 3.0, (points, n))
    p = rng.uniform(0.1, 4.0, (points, n_par))
    outs = []
    for lib in (la, lb):
        out = np.zeros((points, n, width))
        dp = ctypes.POINTER(ctypes.c_double)
        lib.eval_rows(points, y.ctypes.data_as(dp), p.ctypes.data_as(dp), 0.7, out.ctypes.data_as(dp))
        outs.append(out)
    assert np.isfinite(outs[1]).all()
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    assert np.count_nonzero(outs[1]) > points * n


def test_committed_headers_carry_the_shared_form():
    from sysbio_modeling_amd.symbolic import zoo_model
    src = _dispatch(zoo_model('cascade20').hip_source)
    assert src.count('SBM_RCP(') == 1
