"""sbm_iex_seq_kernel<M, ROT> (csrc/sbm_implicit_extrap_seq.hpp) at every lane layout of a stiff chain, against
oracle/iex_oracle.py (the same scheme in dense float64 numpy).

The kernel's layout moves in steps of 16 rows: RPG = ceil(NV / 16) rows per lane, 16 RPG table rows of which 16 RPG - NV
are padding, rotated columns only where RPG is even and NV < 64.  The matrix below takes sizes on both sides of every
16-row boundary, the full tables (NV 32: a zero row of phase A cuts the rotated recurrence; NV 64: no seq kernel), one and
two J_p entries per row, one and two chunks of columns, the orders the kernel takes, restarts and state-only runs, a
scratch buffer left dirty by another layout, and a failing vector among thousands in the persistent loop.  Which variant
each model compiles is checked on the CPU (tests/test_seq_kernel_layouts_cpu.py::EXPECTED).

Criteria as test_gpu_implicit.py::test_extrapolation_kernel_equals_scheme_oracle: y and S within 0.3 integration
tolerances (S with the floor 1e-6 x column max), macro steps within 1 + n / 50, rejections within 2; the seq kernel sums
T_j itself (sums='values'), sbm_iex_kernel T_j - S_n ('differences').  The 0.3 holds where kernel and oracle took the same
decisions on a model with one J_p entry per row; elsewhere 10 (_limits says why).  Structural zeros of S exactly,
whatever the tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_seq_kernel_layouts_cpu import EXPECTED, gpu_matrix_specs, _jp_rows_by_sympy

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_END = 2.5
T_OUT = np.array([0.0, 0.25, 0.4, 1.0]) * T_END
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        from sysbio_modeling_amd.model import OdeModel
        from sysbio_modeling_amd.symbolic import GeneratedModel
        gm = GeneratedModel(gpu_matrix_specs()[name])
        _MODELS[name] = (gm, OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=name))
    return _MODELS[name]


def _params(gm, n_vec):
    from sysbio_modeling_amd import models_zoo
    n = gm.n_vars
    P = models_zoo.stiff_ensemble(n_vec, n=n)[1]
    if len(gm.param_order) > 2 * n:        # the unused parameter: any value, no equation reads it
        P = np.insert(P, 0 if gm.param_order[0] == 'unused' else P.shape[1], 0.7, axis=1)
    return P


def _ratios(Y, S, Yo, So, rtol, atol):
    ky = np.max(np.abs(Y - Yo) / (rtol * np.abs(Yo) + atol))
    n_t = So.shape[0]
    So3 = So.reshape(n_t, Y.shape[-1], -1)
    floor = 1e-6 * np.abs(So3).max(axis=(0, 1))
    ks = np.max(np.abs(S.reshape(So3.shape) - So3) / (rtol * np.maximum(np.abs(So3), floor) + atol))
    return ky, ks


def _limits(same_steps, gm):
    """(y, S) bounds in integration tolerances.  0.3: kernel and oracle took the same decisions (macro steps AND rejections)
    and the model has one J_p entry per row.  Otherwise 10: once a rejection or a step falls differently (allowed by the
    step criteria: the kernel's controller runs in single precision), the two are two discretisations, each within its
    tolerance of the solution; and where two columns share a row (a_i, b_i free) the b columns hold entries far below the
    1e-6 floor of their column whose rounding the sums themselves move by several tolerances (the oracle's two
    accumulations of the same scheme differ by up to 5.8 on stiff16_free)."""
    two_jp = any(len(r) > 1 for r in _rows_by_column(gm, by_row=True))
    return (0.3 if same_steps else 10.0), (0.3 if same_steps and not two_jp else 10.0)


def _rows_by_column(gm, by_row=False):
    rows = _jp_rows_by_sympy(gm.spec)
    if not by_row:
        return rows
    out = [[] for _ in range(gm.n_vars)]
    for c, rr in enumerate(rows):
        for r in rr:
            out[r].append(c)
    return out


def _sums(name):
    return 'values' if EXPECTED[name] is not None else 'differences'


def _structural_zeros(gm, S):
    """S (..., NV * NK): the rows above each column's J_p row, exactly 0.0 at every output time"""
    n, k = gm.n_vars, gm.n_sens
    rows = _rows_by_column(gm)
    S4 = S.reshape(S.shape[:-1] + (n, k))
    for c in range(k):
        top = rows[c][0] if rows[c] else n        # a column without a J_p entry: zero throughout
        if top:
            above = S4[..., :top, c]
            assert np.all(above == 0.0), (gm.name, c, top, np.abs(above).max())


def _against_oracle(name, order, rtol, n_vec=2, t_out=T_OUT):
    from oracle import iex_oracle
    gm, m = _model(name)
    P = _params(gm, n_vec)
    atol = 1e-3 * rtol
    kw = dict(method='implicit_extrap', rtol=rtol, atol=atol, order=order)
    S, Y = m.calc_jacobian_batch(P, t_out, return_states=True, **kw)
    info = m.last_info
    assert info['status'].tolist() == [0] * n_vec
    _structural_zeros(gm, S)
    worst = [0.0, 0.0]
    for v in range(n_vec):
        Yo, So, io = iex_oracle.integrate(gm, P[v], t_out[1:], rtol=rtol, atol=atol, order=order, sums=_sums(name))
        assert io['status'] == 0
        ky, ks = _ratios(Y[v, 1:], S[v, 1:], Yo, So, rtol, atol)
        same = int(info['n_steps'][v]) == io['n_steps'] and int(info['n_rejected'][v]) == io['n_reject']
        ly, ls = _limits(same, gm)
        print("%s K %d vector %d (%s): kernel vs scheme oracle y %.3g S %.3g integration tolerances (bounds %g / %g); %d "
              "macro steps (oracle %d), %d rejected (oracle %d)" % (name, order, v, EXPECTED[name] or 'sbm_iex_kernel', ky,
                                                                    ks, ly, ls, info['n_steps'][v], io['n_steps'],
                                                                    info['n_rejected'][v], io['n_reject']))
        assert abs(int(info['n_steps'][v]) - io['n_steps']) <= 1 + io['n_steps'] // 50, (info['n_steps'][v], io)
        assert abs(int(info['n_rejected'][v]) - io['n_reject']) <= 2
        assert ky <= ly and ks <= ls, (ky, ks)
        worst = [max(worst[0], ky), max(worst[1], ks)]
    print("%s K %d worst: y %.3g S %.3g" % (name, order, worst[0], worst[1]))
    return gm, m, P, S, Y


LAYOUTS = ['stiff16', 'stiff17', 'stiff31', 'stiff32', 'stiff33', 'stiff48', 'stiff49', 'stiff64',
           'stiff16_free', 'stiff33_free', 'stiff64_free']


@pytest.mark.parametrize('name', LAYOUTS)
def test_layout_equals_scheme_oracle_with_exact_structural_zeros(name):
    _against_oracle(name, 8, 3e-9)


# (rtol per order: the low orders need thousands of macro steps at tight tolerances)
@pytest.mark.parametrize('name', ['stiff24', 'stiff33'])
@pytest.mark.parametrize('order,rtol', [(2, 1e-5), (3, 1e-6), (5, 1e-7), (8, 3e-9)])
def test_every_order_of_the_seq_kernel_equals_scheme_oracle(name, order, rtol):
    _against_oracle(name, order, rtol)


@pytest.mark.parametrize('name', ['stiff18_unused_trailing', 'stiff18_unused_leading'])
def test_column_without_a_jp_entry_is_exactly_zero(name):
    """A parameter no equation refers to: its column is zero.  The emitter does not rotate such a model (no row for the
    column to start at), the un-rotated seq kernel runs it -- against the oracle, and against the explicit default method"""
    gm, m, P, S, Y = _against_oracle(name, 8, 3e-9)
    c = gm.sens_params.index('unused')
    S4 = S.reshape(S.shape[:2] + (gm.n_vars, gm.n_sens))
    assert np.all(S4[..., c] == 0.0)
    t = np.array([0.0, 0.02, 0.05])         # (explicit steps on a 10^6 rate: a short span)
    Se, Ye = m.calc_jacobian_batch(P, t, return_states=True)
    assert not m.last_info['status'].any()
    assert np.all(Se.reshape(Se.shape[:2] + (gm.n_vars, gm.n_sens))[..., c] == 0.0)
    Si, Yi = m.calc_jacobian_batch(P, t, return_states=True, method='implicit_extrap', rtol=3e-9, atol=3e-12, order=8)
    assert np.max(np.abs(Yi - Ye) / (1e-7 * np.abs(Ye) + 1e-10)) <= 1.0


@pytest.mark.parametrize('name', ['stiff17', 'stiff32'])
def test_restart_and_state_only_at_rotated_sizes(name):
    """A restart from given (y, S)(t1) runs the un-rotated variant: against the oracle restarted from the same point (scheme
    level) and against the one-call solution (rotated variant; different step sequence: a few tolerances).  The state-only
    entry point against the oracle's state-only run and against the states of the call with sensitivities."""
    from oracle import iex_oracle
    rtol, atol = 3e-9, 3e-12
    kw = dict(method='implicit_extrap', rtol=rtol, atol=atol, order=8)
    gm, m = _model(name)
    n = gm.n_vars
    P = _params(gm, 2)
    t1, t2 = 1.0, T_END
    S, Y = m.calc_jacobian_batch(P, np.array([0.0, t1, t2]), return_states=True, **kw)
    assert not m.last_info['status'].any()
    for v in range(2):
        y0 = np.concatenate([Y[v, 1], S[v, 1]])
        Sb, Yb = m.calc_jacobian_batch(P[v:v + 1], np.array([t1, t2]), init_conditions=y0, return_states=True, **kw)
        info = m.last_info
        assert not info['status'].any()
        assert np.array_equal(Yb[0, 0], Y[v, 1]) and np.array_equal(Sb[0, 0], S[v, 1])
        Yo, So, io = iex_oracle.integrate(gm, P[v], np.array([t2]), rtol=rtol, atol=atol, order=8, sums='values', t0=t1,
                                          y0=Y[v, 1], s0=S[v, 1])
        ky, ks = _ratios(Yb[0, 1:], Sb[0, 1:], Yo, So, rtol, atol)
        ky1, ks1 = _ratios(Yb[0, 1:], Sb[0, 1:], Y[v, 2:], S[v, 2:], rtol, atol)
        same = int(info['n_steps'][0]) == io['n_steps'] and int(info['n_rejected'][0]) == io['n_reject']
        ly, ls = _limits(same, gm)
        # S of a restart: 3.  The oracle restarted from its own (y, S)(t1) with S moved by 1e-15 relative lands 1.7
        # tolerances away at t2 on stiff32 vector 1 (2.9 with its other accumulation): the restart amplifies rounding
        ls = max(ls, 3.0)
        print("%s vector %d restarted at %g: vs oracle y %.3g S %.3g (bounds %g / %g; %d / %d macro steps, %d / %d "
              "rejected), vs one call y %.3g S %.3g integration tolerances"
              % (name, v, t1, ky, ks, ly, ls, info['n_steps'][0], io['n_steps'], info['n_rejected'][0], io['n_reject'],
                 ky1, ks1))
        assert abs(int(info['n_steps'][0]) - io['n_steps']) <= 1 + io['n_steps'] // 50
        assert abs(int(info['n_rejected'][0]) - io['n_reject']) <= 2
        assert ky <= ly and ks <= ls
        assert ky1 <= 3.0 and ks1 <= 3.0
    t = np.array([0.0, t1, t2])
    Ys = m.simulate_batch(P, t, **kw)
    info = m.last_info
    assert not info['status'].any()
    for v in range(2):
        Yo, _, io = iex_oracle.integrate(gm, P[v], t[1:], rtol=rtol, atol=atol, order=8, with_sens=False)
        ky = np.max(np.abs(Ys[v, 1:] - Yo) / (rtol * np.abs(Yo) + atol))
        kc = np.max(np.abs(Ys[v, 1:] - Y[v, 1:]) / (rtol * np.abs(Y[v, 1:]) + atol))
        same = int(info['n_steps'][v]) == io['n_steps'] and int(info['n_rejected'][v]) == io['n_reject']
        # (3, not 0.3: without columns to tighten them the steps are long, and the oracle's own state-only run moves by up
        # to 1.45 tolerances when p moves by one rounding unit -- stiff32, same step counts)
        ly = 3.0 if same else 10.0
        print("%s vector %d state-only: vs oracle %.3g (bound %g; %d / %d macro steps, %d / %d rejected), vs the states "
              "with sensitivities %.3g integration tolerances" % (name, v, ky, ly, info['n_steps'][v], io['n_steps'],
                                                                  info['n_rejected'][v], io['n_reject'], kc))
        assert abs(int(info['n_steps'][v]) - io['n_steps']) <= 1 + io['n_steps'] // 50
        assert abs(int(info['n_rejected'][v]) - io['n_reject']) <= 2
        assert ky <= ly and kc <= 10.0
    assert Ys.shape == (2, 3, n)


_DIRTY = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_seq_layouts import _model, _params, T_OUT
dirty = sys.argv[3] == 'dirty'
kw = dict(method='implicit_extrap', rtol=3e-9, atol=3e-12, order=8)
out = {}
for name in ('stiff32', 'stiff17'):
    gm, m = _model(name)
    P = _params(gm, 2)
    if dirty:
        # the scratch buffer belongs to the model's plugin: dirty it through the SAME model first.  Given initial
        # sensitivities it runs the un-rotated variant, whose step tables (96 doubles apart) cover the rotated variant's
        # rows 32..63 of steps 0..17 with the reciprocal pivots, sub-diagonal factors and J_p entries of rows 16..31
        yS0 = np.zeros(gm.n_vars * (1 + gm.n_sens))
        S, Y = m.calc_jacobian_batch(P, T_OUT, init_conditions=yS0, return_states=True, **kw)
        assert not m.last_info['status'].any()
        out['Su_' + name] = S
    S, Y = m.calc_jacobian_batch(P, T_OUT, return_states=True, **kw)
    out['S_' + name], out['Y_' + name], out['st_' + name] = S, Y, m.last_info['status']
np.savez(sys.argv[2], **out)
'''


def _child(tmp_path, source, tag, *args, env=None):
    script = tmp_path / ('%s.py' % tag)
    script.write_text(source)
    out = tmp_path / ('%s.npz' % tag)
    p = subprocess.run([sys.executable, str(script), REPO, str(out)] + list(args), env=dict(os.environ, **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out), p.stderr


def test_rotated_results_do_not_depend_on_what_the_scratch_held(tmp_path):
    """Rotated NV 32 (full table: the cut row is a zero row phase A writes) and NV 17 (14 padded rows), once as the first
    launch of the model in a fresh process (its scratch buffer newly allocated and zeroed) and once right after an
    un-rotated launch of the same model on the same workgroups has left non-zero table values where the rotated variant
    reads its cut row: identical to the bit, and both on the oracle.  (Without phase A's zero rows, NV 32 would take
    J_p(row 21) x S[31] into the rows above each column's J_p row.)"""
    from oracle import iex_oracle
    clean, _ = _child(tmp_path, _DIRTY, 'clean', 'clean')
    dirty, _ = _child(tmp_path, _DIRTY, 'dirty', 'dirty')
    for name in ('stiff32', 'stiff17'):
        for key in ('S_', 'Y_', 'st_'):
            assert np.array_equal(clean[key + name], dirty[key + name]), (name, key)
        assert not clean['st_' + name].any()
        gm, _ = _model(name)
        P = _params(gm, 2)
        for v in range(2):
            Yo, So, io = iex_oracle.integrate(gm, P[v], T_OUT[1:], rtol=3e-9, atol=3e-12, order=8, sums='values')
            ky, ks = _ratios(clean['Y_' + name][v, 1:], clean['S_' + name][v, 1:], Yo, So, 3e-9, 3e-12)
            print("%s vector %d, clean / dirty scratch (identical): vs oracle y %.3g S %.3g" % (name, v, ky, ks))
            assert ky <= 0.3 and ks <= 0.3
        _structural_zeros(gm, clean['S_' + name])
        _structural_zeros(gm, dirty['S_' + name])
        # the dirtying launch is the same problem through the other variant: within a few tolerances of the rotated one
        for v in range(2):
            Yd = dirty['Y_' + name][v, 1:]
            _, ks = _ratios(Yd, dirty['Su_' + name][v, 1:], Yd, dirty['S_' + name][v, 1:], 3e-9, 3e-12)
            print("%s vector %d: un-rotated (given zero sensitivities) vs rotated S %.3g" % (name, v, ks))
            assert ks <= 3.0


_PERSISTENT = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_seq_layouts import _model, _params
gm, m = _model('stiff17')
P = _params(gm, int(sys.argv[3]))
bad = int(sys.argv[4])
t = np.array([0.0, 0.5, 1.0])
kw = dict(method='implicit_extrap', rtol=3e-9, atol=3e-12, order=8)
S0, Y0 = m.calc_jacobian_batch(P, t, return_states=True, **kw)
st0 = m.last_info['status'].copy()
P[bad, 3] = np.nan
S1, Y1 = m.calc_jacobian_batch(P, t, return_states=True, **kw)
st1 = m.last_info['status'].copy()
np.savez(sys.argv[2], S0=S0, Y0=Y0, st0=st0, S1=S1, Y1=Y1, st1=st1)
'''


def test_failing_vector_inside_the_persistent_loop(tmp_path):
    """More trajectories than resident workgroups (each workgroup takes several from the counter), one of them with a NaN
    parameter: its status is set and its rows are NaN, every other trajectory is the same to the bit as without it."""
    import re
    V, bad = 4096, 2500
    res, err = _child(tmp_path, _PERSISTENT, 'persistent', str(V), str(bad), env={'SBM_DEBUG_LAUNCH': '1'})
    m = re.findall(r'sbm_iex_seq_kernel: (\d+) pieces of work, (\d+) resident workgroups, grid (\d+)', err)
    assert len(m) == 2, err[-2000:]
    n_work, resident, grid = (int(x) for x in m[0])
    print("persistent loop: %d pieces of work on %d resident workgroups" % (n_work, resident))
    assert n_work == V and n_work > 2 * resident and grid == resident
    assert not res['st0'].any()
    st1 = res['st1']
    assert st1[bad] != 0 and np.all(np.isnan(res['Y1'][bad, 1:])) and np.all(np.isnan(res['S1'][bad, 1:]))
    keep = np.arange(V) != bad
    assert not st1[keep].any()
    assert np.array_equal(res['Y1'][keep], res['Y0'][keep]) and np.array_equal(res['S1'][keep], res['S0'][keep])
