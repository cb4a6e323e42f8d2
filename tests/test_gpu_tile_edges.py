"""sbm_sens_mfma_kernel (csrc/sbm_sens_mfma.hpp) and sbm_sens_packed_kernel (csrc/sbm_kernels_rowlane.hpp) at every tile and
segment edge: the ten models of models_zoo.tile_edge_specs(), each forced onto every one of the two kernels that takes
it.  Which instantiation a model compiles -- RT, CT, NCH, LDJ, LDA; SEG and trajectories per wavefront -- is computed
and held against a literal table on the CPU (tests/test_tile_edge_layouts_cpu.py::EXPECTED).

Fixed-step RK4 is one scheme whatever the lane layout: the kernels are compared with oracle/rk4_oracle.py (plain float64
RK4 on the oracle's C right-hand side, the step partition of include/sbm.h) entry by entry, relative to the column's
largest entry, at the ROUNDING level of the problem.  rho = the same oracle on the C against the Python right-hand side
(tests/test_tile_edge_layouts_cpu.py, measured per model in its docstring; largest RHO_MAX); the bound is 8 rho: the kernels
contract FMAs and sum a row's products in tile order where the CPU sums five non-zeros.  The row-lane kernel goes through
the same check: the bound is one a correct kernel meets.

  rho per model (five vectors, 128 steps per interval to t = 1, 2, 3):
    tile7_16 1.64e-16   tile16_15 2.08e-16   tile7_32 1.99e-16   tile17_14 1.15e-16   tile16_17 2.18e-16
    tile15_33 2.02e-16  tile16_49 2.18e-16   tile33_17 1.61e-16  tile49_17 1.41e-16   tile64_16 1.88e-16
  bound: 8 x 2.2e-16 = 1.76e-15.  Measured on an MI355X, worst over models, from zero / from given (y0, S0):
    MFMA 4.48e-16 / 3.46e-16, packed 3.95e-16 / 3.46e-16, row-lane 4.22e-16 / 4.45e-16.

A forced variant the launcher does not accept falls back to the row kernels without a word (csrc/sbm_kernel_choice.hpp,
row_choice_free): every forced MFMA result here must differ in some bit from the row-lane kernel's and from packed's, and
under SBM_DEBUG_LAUNCH the launcher must name the forced kernel, with the plan of the CPU table (the packed kernel evaluates
the row-lane kernel's own FMA chains: its RK4 result is the row-lane kernel's to the bit, so only the launcher can tell).

DOPRI45 / DOP853 against the reference's LSODA with a tight solution as arbiter (check_parity), two vectors per model.
Initial conditions, independence of wavefront mates and batch size, failures: bit for bit."""
import warnings

import numpy as np
import pytest

from tests.conftest import check_parity
from tests.test_tile_edge_layouts_cpu import EXPECTED, NAMES, PACKED, T_OUT, H0, RK4_BOUND, generated, params_of

pytestmark = pytest.mark.gpu

CASES = [(n, 'mfma') for n in NAMES] + [(n, 'packed') for n in PACKED]
IDS = ['%s-%s' % c for c in CASES]
GRID = np.linspace(0.0, 3.0, 97)          # the reference's grid; T_OUT[1:] = GRID[IDX] exactly (dyadic)
IDX = np.array([32, 64, 96])
_MODELS, _RUNS, _ORACLE = {}, {}, {}


def _model(name):
    if name not in _MODELS:
        from sysbio_modeling_amd.model import OdeModel
        gm = generated(name)
        _MODELS[name] = (gm, OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=name))
    return _MODELS[name]


def _run(name, variant, method, n_vec=5, init=None, P=None, **kw):
    """(S, Y, status, n_steps) of one call; calls on the standard vectors are computed once"""
    key = (name, variant, method, n_vec) if init is None and P is None and not kw else None
    if key in _RUNS:
        return _RUNS[key]
    gm, m = _model(name)
    if P is None:
        P = params_of(name, n_vec)
    if method == 'rk4':
        kw = dict(kw, h0=H0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        S, Y = m.calc_jacobian_batch(P, T_OUT, init, return_states=True, method=method, variant=variant, **kw)
    out = (S, Y, m.last_info['status'].copy(), m.last_info['n_steps'].copy())
    assert out[2].shape == (len(P),) and out[3].shape == (len(P),)
    if key is not None:
        _RUNS[key] = out
    return out


def _rk4_oracle(name, v, init=None):
    from oracle import rk4_oracle
    key = (name, v, None if init is None else init.tobytes())
    if key not in _ORACLE:
        gm = generated(name)
        _ORACLE[key] = rk4_oracle.integrate(gm, params_of(name, 5)[v], T_OUT, H0, init_conditions=init, use_c=True)
    return _ORACLE[key]


def _rk4_err(name, S, Y, init=None, vectors=(0, 1, 2, 3, 4)):
    from oracle import rk4_oracle
    gm = generated(name)
    return max(rk4_oracle.colmax_err(np.concatenate([Y[v], S[v]], axis=1), _rk4_oracle(name, v, init), gm.n_vars, gm.n_sens)
               for v in vectors)


def _init(name, seed=3):
    gm = generated(name)
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0.0, 0.5, gm.n_vars), 1e-2 * rng.standard_normal(gm.n_vars * gm.n_sens)])


# ---- fixed-step RK4 at the rounding level ----
@pytest.mark.parametrize('name,variant', CASES + [(n, 'row_lane') for n in NAMES],
                         ids=IDS + ['%s-row_lane' % n for n in NAMES])
def test_rk4_equals_the_cpu_rk4_to_rounding(name, variant):
    S, Y, st, ns = _run(name, variant, 'rk4')
    assert st.tolist() == [0] * 5 and ns.tolist() == [384] * 5
    e = _rk4_err(name, S, Y)
    print("%s %s: RK4 vs CPU RK4, worst entry relative to its column maximum %.3g (bound %.3g)" % (name, variant, e, RK4_BOUND))
    assert e <= RK4_BOUND
    # from given initial conditions: the element-to-(row, column) map of the load, against the same oracle
    init = _init(name)
    S, Y, st, _ = _run(name, variant, 'rk4', n_vec=2, init=init)
    assert st.tolist() == [0, 0]
    e = _rk4_err(name, S, Y, init=init, vectors=(0, 1))
    print("%s %s: RK4 from given (y0, S0) vs CPU RK4 %.3g (bound %.3g)" % (name, variant, e, RK4_BOUND))
    assert e <= RK4_BOUND


@pytest.mark.parametrize('name,variant', CASES, ids=IDS)
def test_the_forced_result_is_not_the_row_kernels(name, variant):
    """The matrix-core kernel sums a row's products in tile order: a forced MFMA result identical to the bit to the row-lane
    kernel's, or to the packed kernel's, would say the launcher fell back.  The packed kernel cannot be told from the
    row-lane kernel this way: it evaluates the very FMA chains of the row-lane kernel (the emitter's apply_lds and
    apply_rowlane sum in one order, J_y read from an LDS table instead of the row lane's register), so its RK4 result IS
    the row-lane kernel's, bit for bit -- asserted as such, at SEG 16 and 32; that the packed kernel ran is read off the
    launcher itself (test_the_launcher_names_the_forced_kernel_and_its_plan)."""
    S, Y, _, _ = _run(name, variant, 'rk4')
    Sr, Yr, _, _ = _run(name, 'row_lane', 'rk4')
    # "differs" must mean another finite number, not a NaN somewhere
    assert np.isfinite(S).all() and np.isfinite(Y).all() and np.isfinite(Sr).all() and np.isfinite(Yr).all()
    if variant == 'mfma':
        assert not np.array_equal(S, Sr)
    else:
        assert np.array_equal(S, Sr) and np.array_equal(Y, Yr), (
            "%s: packed and row-lane RK4 results differ in some bit.  They are the same only because the emitter's "
            "apply_lds and apply_rowlane sum a row's products in one order: a deliberate change to the order of either "
            "ends that identity without either kernel being wrong.  If test_rk4_equals_the_cpu_rk4_to_rounding still "
            "passes for both, replace this assertion by 'not bit-identical' (what the launcher ran is checked by "
            "test_the_launcher_names_the_forced_kernel_and_its_plan); if not, the kernel that fails there is wrong."
            % name)
        Sm, _, _, _ = _run(name, 'mfma', 'rk4')
        assert np.isfinite(Sm).all() and not np.array_equal(S, Sm)
    # (and to rounding they are the same numbers: all passed the check against the CPU RK4)


_LAUNCHES = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_tile_edges import CASES, _run
for name, variant in CASES:
    sys.stderr.write('CASE %s %s\n' % (name, variant))
    sys.stderr.flush()
    S, Y, st, ns = _run(name, variant, 'rk4', n_vec=5)
    assert not st.any()
sys.stderr.write('CASE end\n')
'''


def test_the_launcher_names_the_forced_kernel_and_its_plan():
    """A forced variant the launcher does not accept falls through to the row kernels without a word.  Under
    SBM_DEBUG_LAUNCH the launcher names the matrix-core / packed kernel a call runs, with the plan it was compiled with:
    one call per (model, forced variant) in a child process, each followed by exactly the line of the kernel it names and
    the plan of tests/test_tile_edge_layouts_cpu.py::EXPECTED (the Python restatement of the plan is the compiled one)."""
    import os
    import re
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the child's program is the string above (python -c): nothing is written or read outside the repository tree
    p = subprocess.run([sys.executable, '-c', _LAUNCHES, repo], cwd=repo, env=dict(os.environ, SBM_DEBUG_LAUNCH='1'),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    blocks = re.split(r'^CASE ', p.stderr, flags=re.M)[1:]
    assert [b.split('\n')[0] for b in blocks] == ['%s %s' % c for c in CASES] + ['end']
    for (name, variant), block in zip(CASES, blocks):
        nv, nk, packed, rt, ct, nch, ldj, lda, _ = EXPECTED[name]
        lines = [ln for ln in block.split('\n')[1:] if ln.startswith('sbm_')]
        if variant == 'mfma':
            want = 'sbm_sens_mfma_kernel: RT %d CT %d NCH %d LDJ %d LDA %d, 5 trajectories' % (rt, ct, nch, ldj, lda)
        else:
            want = 'sbm_sens_packed_kernel: SEG %d, 5 trajectories, grid %d' % (packed[0], (5 + packed[1] - 1) // packed[1])
        assert lines == [want], (name, variant, lines)


# ---- the adaptive methods against the reference ----
def _parity(name, variant, method, S, Y):
    from oracle import odeint_oracle as oo
    gm = generated(name)
    gm.c_library()
    P = params_of(name, 5)
    for v in (0, 4):
        key = (name, v, 'lsoda')
        if key not in _ORACLE:
            _ORACLE[key] = oo.calc_jacobian(gm, P[v], GRID, use_c=True, return_states=True)
        Sr, Yr = _ORACLE[key]
        tight = lambda v=v: oo.tight_solution(gm, P[v], T_OUT, use_c=True, atol=1e-30)[1:]
        check_parity(np.concatenate([Y[v, 1:], S[v, 1:]], axis=1), np.concatenate([Yr[IDX], Sr[IDX]], axis=1), tight,
                     what='%s %s %s vector %d' % (name, variant, method, v))


@pytest.mark.parametrize('name,variant', CASES, ids=IDS)
def test_dopri45_parity_statuses_and_step_counts(name, variant):
    assert np.array_equal(GRID[IDX], T_OUT[1:])
    S, Y, st, ns = _run(name, variant, 'dopri45')
    _, _, _, na = _run(name, 'row_lane', 'dopri45')
    assert st.tolist() == [0] * 5
    print("%s %s: DOPRI45 steps %s, row-lane kernel %s" % (name, variant, ns.tolist(), na.tolist()))
    if variant == 'mfma':
        # per-chunk error norms: a few per cent fewer steps than the norm over all columns, never more than + 2
        assert np.all(ns <= na + 2) and np.all(ns >= 0.9 * na)
    else:
        assert np.all(np.abs(ns - na) <= 2)
    _parity(name, variant, 'dopri45', S, Y)


@pytest.mark.parametrize('name,variant', [('tile15_33', 'mfma'), ('tile49_17', 'mfma'), ('tile7_16', 'packed'),
                                          ('tile17_14', 'packed')])
def test_dop853_parity(name, variant):
    """the launcher builds DOP853 for the matrix-core kernel (RT 1 with three column tiles, RT 4) but keeps AUTO away from
    it; packed at SEG 16 and SEG 32"""
    S, Y, st, ns = _run(name, variant, 'dop853')
    assert st.tolist() == [0] * 5
    _parity(name, variant, 'dop853', S, Y)


# ---- initial conditions ----
@pytest.mark.parametrize('name,variant', CASES, ids=IDS)
@pytest.mark.parametrize('method', ['dopri45', 'rk4'])
def test_initial_conditions_come_back_bit_for_bit(name, variant, method):
    """t_out[0] = t0: row 0 of Y and S is what the kernel loaded into its lane layout and stored from it -- padded rows,
    padded columns and empty tiles included (test_rk4_equals_the_cpu_rk4_to_rounding checks where they went in between)"""
    gm = generated(name)
    init = _init(name, seed=11)
    S, Y, st, _ = _run(name, variant, method, n_vec=3, init=init)
    assert st.tolist() == [0, 0, 0]
    for v in range(3):
        assert np.array_equal(Y[v, 0], init[:gm.n_vars]) and np.array_equal(S[v, 0], init[gm.n_vars:])


# ---- packed: neither wavefront mates nor the size of the batch ----
@pytest.mark.parametrize('name', PACKED)
@pytest.mark.parametrize('method', ['dopri45', 'rk4'])
def test_packed_rows_do_not_depend_on_mates_or_batch_size(name, method):
    """V on both sides of the trajectories per wavefront (a ragged last wavefront's idle segments integrate a copy of the
    last trajectory and must leave nothing behind), and a trajectory among other mates"""
    tpw = EXPECTED[name][2][1]
    sizes = (1, 4, 5, 7) if tpw == 4 else (1, 2, 3)
    P = params_of(name, 7)
    S7, Y7, st7, ns7 = _run(name, 'packed', method, P=P)
    assert st7.tolist() == [0] * 7
    for V in sizes:
        S, Y, st, ns = _run(name, 'packed', method, P=P[:V])
        assert S.shape[0] == V and st.tolist() == [0] * V
        assert np.array_equal(S, S7[:V]) and np.array_equal(Y, Y7[:V]) and np.array_equal(ns, ns7[:V]), (name, method, V)
    pick = np.array([6, 2, 2, 0, 5, 2])
    S, Y, st, ns = _run(name, 'packed', method, P=P[pick])
    assert np.array_equal(S, S7[pick]) and np.array_equal(Y, Y7[pick]) and np.array_equal(ns, ns7[pick])


# ---- failures stay where they are ----
@pytest.mark.parametrize('name,variant', [(n, 'packed') for n in PACKED] +
                         [(n, 'mfma') for n in ('tile7_32', 'tile16_49', 'tile33_17', 'tile49_17')])
@pytest.mark.parametrize('method', ['dopri45', 'rk4'])
def test_a_failing_vector_keeps_to_itself(name, variant, method):
    """One vector with a NaN parameter, in the middle of the batch and as its last vector (packed: the last live segment of a
    ragged wavefront, whose idle segments copy it): non-zero status and NaN rows for it, reported once per trajectory
    (MFMA, NCH = 2: the worst status over its chunks); its neighbours as in the clean run, bit for bit."""
    gm = generated(name)
    tpw = EXPECTED[name][2][1] if variant == 'packed' else 1
    V = tpw + 1 if variant == 'packed' else 3
    P = params_of(name, 7)[:V]
    S0, Y0, st0, ns0 = _run(name, variant, method, P=P)
    assert st0.tolist() == [0] * V
    col = gm.param_order.index('k0')
    for bad in (1 if V > 2 else 0, V - 1):
        Pb = P.copy()
        Pb[bad, col] = np.nan
        S, Y, st, ns = _run(name, variant, method, P=Pb)
        assert st.shape == (V,) and st[bad] != 0
        assert np.all(np.isnan(Y[bad, -1])) and np.all(np.isnan(S[bad, -1]))
        if method == 'dopri45':
            assert np.all(np.isnan(Y[bad, 1:])) and np.all(np.isnan(S[bad, 1:]))
        keep = np.arange(V) != bad
        assert not st[keep].any()
        assert np.array_equal(S[keep], S0[keep]) and np.array_equal(Y[keep], Y0[keep]) and np.array_equal(ns[keep], ns0[keep])
