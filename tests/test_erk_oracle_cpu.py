"""oracle/erk_oracle.py -- the restatement of sbm_dopri45 / sbm_dop853 that tests/test_gpu_adaptive_scheme.py holds every
kernel to -- pinned on the CPU, and the inputs of those GPU tests chosen.  No GPU needed.

  * the tableaus in csrc/sbm_rk_drivers.hpp (namespace dp: 30 entries, namespace dp8: 85) are SciPy's, bit for bit, and
    what the header leaves out is zero there (the header's dp::E is minus SciPy's E: the norm does not see the sign);
  * one step of each pair is SciPy's (rk_step and the solvers' own error norm), to rounding;
  * the oracle meets the parity criterion (check_parity) on the goldens' vectors, and its error falls with rtol as the
    order of the pair says;
  * every input of the GPU tests (tests/support/erk_cases.py::PROBLEMS, literal indices into the ensembles) qualifies:
    error margin >= 0.01, landing margin >= 1e-4 -- so no rounding flips a decision and step counts are exact;
  * s of every problem (oracle against oracle under the noise model, three seeds) is the literal the GPU bound 8 s is
    taken from, the counts do not move under the noise, and 8 s <= 1e-3 x the run's truncation error;
  * the bound bites: the oracle with ONE deliberate error changes a count or leaves the bound.

s per problem (worst over its vectors and seeds 1, 2, 3; rounded up in PROBLEMS), smallest distance to the tight solution:

  c20-d45-all 1.02e-15 / 8.9e-10       c20-d853-all 3.49e-14 / 5.4e-09      c20-d853-rg2 2.59e-14 / 5.4e-09
  c20-d45-rg1 1.27e-15 / 9.5e-10       c20-d853-rg1 9.26e-14 / 9.9e-10      c20-d45-mfma 1.78e-15 / 9.9e-10
  c20-d853-mfma 6.43e-14 / 5.5e-09     c20-d45-all-h0 1.53e-15 / 8.9e-10    c20-d853-rg2-h0 6.90e-14 / 4.7e-09
  c20-d45-all-r5 2.06e-13 / 5.8e-08    c20-d853-rg2-r5 1.53e-13 / 4.1e-08   c20-d45-mfma-init 2.54e-15 / 4.5e-09
  c20-d45-rg1-init 7.54e-15 / 4.8e-09  c20-d853-rg2-init 1.68e-14 / 1.9e-10 mm-d45 5.12e-15 / 6.1e-09
  mm-d853 1.04e-14 / 2.3e-09           simple-d45 2.83e-14 / 1.2e-08        simple-d853 1.80e-14 / 3.8e-09
  mm-d45-h0 4.07e-15 / 6.0e-09         mm-d45-r5 3.51e-12 / 4.7e-07         t49-d45-all 5.15e-15 / 3.0e-09
  t49-d853-all 2.91e-15 / 1.2e-09      t49-d45-mfma 3.48e-15 / 5.1e-09      t49-d853-mfma 2.88e-15 / 1.2e-09
  t49-d45-mfma-h0 3.99e-15 / 5.1e-09   t49-d45-mfma-r5 7.13e-13 / 5.0e-07   t49-d45-mfma-init 1.04e-15 / 1.4e-09
  c40-d45-all 3.28e-14 / 6.4e-09       s-c20-d45 1.92e-14 / 9.8e-09         s-c20-d853 3.95e-14 / 4.2e-09
  s-c20-d45-h0 8.21e-14 / 9.8e-09      s-c20-d45-r5 3.33e-12 / 8.4e-07      s-c20-d45-70 1.52e-14 / 9.8e-09
  s-c20-d45-2049 5.14e-15 / 3.9e-09    s-c20-d853-2049 1.22e-14 / 5.3e-09   s-mm-d45-2049 1.77e-14 / 3.8e-09
  s-mm-d853-2049 1.04e-14 / 1.1e-09"""
import os
import re

import numpy as np
import pytest

from tests.conftest import GOLDEN, REPO, check_parity
from tests.support import erk_cases as ec

HEADER = os.path.join(REPO, 'sysbio_modeling_amd', 'csrc', 'sbm_rk_drivers.hpp')
NAMES = list(ec.PROBLEMS)


# ---- the header's tableaus ----
def _namespace(name):
    """{constant: value} of ``namespace <name> { ... }`` in the header; the initialisers are literals and quotients of them"""
    text = open(HEADER).read()
    body = re.search(r'namespace %s \{(.*?)\}  // namespace %s' % (name, name), text, re.S).group(1)
    out = {}
    for key, expr in re.findall(r'(\w+) = ([^,;]+)[,;]', body):
        assert re.fullmatch(r'[-0-9.e/ ]+', expr), (key, expr)
        assert key not in out
        out[key] = float(eval(expr))
    return out


def test_dopri45_tableau_in_the_header_is_scipys():
    from scipy.integrate._ivp.rk import RK45
    h = _namespace('dp')
    want = {}
    for i in range(2, 6):
        want['C%d' % i] = RK45.C[i - 1]
    for i in range(2, 7):
        for j in range(1, i):
            want['A%d%d' % (i, j)] = RK45.A[i - 1][j - 1]
    for j in range(1, 7):
        want['A7%d' % j] = RK45.B[j - 1]          # the seventh stage's argument is the new value
    for j in range(1, 8):
        want['E%d' % j] = -RK45.E[j - 1]
    assert RK45.C[5] == 1.0 and RK45.C[0] == 0.0  # the header writes t + hs for stages 6 and 7
    zero = {k for k, v in want.items() if v == 0.0}
    assert zero == {'A72', 'E2'} and not zero & set(h)
    assert set(h) == set(want) - zero and len(h) == 30
    for k, v in h.items():
        assert v == want[k], (k, v, want[k])


def test_dop853_tableau_in_the_header_is_scipys():
    from scipy.integrate._ivp import dop853_coefficients as d
    h = _namespace('dp8')
    want = {}
    for i in range(2, 13):
        want['C%d' % i] = d.C[i - 1]
        for j in range(1, i):
            want['A%d_%d' % (i, j)] = d.A[i - 1, j - 1]
    for j in range(1, 13):
        want['B%d' % j] = d.B[j - 1]
        want['E5_%d' % j] = d.E5[j - 1]
        want['E3_%d' % j] = d.E3[j - 1]
    assert d.E5[12] == 0.0 and d.E3[12] == 0.0    # nothing for the new value's derivative
    assert np.array_equal(d.A[12, :12], d.B)      # (SciPy's thirteenth row is B)
    zero = {k for k, v in want.items() if v == 0.0}
    assert not zero & set(h)
    assert set(h) == set(want) - zero and len(h) == 85
    for k, v in h.items():
        assert v == want[k], (k, v, want[k])


# ---- one step ----
@pytest.mark.parametrize('method', ['dopri45', 'dop853'])
def test_one_step_is_scipys(method):
    """t_out = (0, h) with h0 = h: one clipped attempt of size h.  State only, so that the oracle's norm is SciPy's RMS norm."""
    from scipy.integrate import RK45, DOP853
    from scipy.integrate._ivp.rk import rk_step
    from oracle import erk_oracle as eo, odeint_oracle as oo
    gm = ec.gm_of('cascade20')
    p = ec.ensemble('cascade20', 4)[1]
    y0 = ec.init_of('cascade20')[:gm.n_vars]
    h, rtol, atol = 0.37, 1e-6, 1e-9
    r = eo.integrate(gm, p, np.array([0.0, h]), method=method, rtol=rtol, atol=atol, h0=h, sens=False, init_conditions=y0)
    assert r['n_try'] == 1 and len(r['errs']) == 1
    fw = oo._wrap_c(gm.c_library().sbm_rhs, gm.n_vars, p)
    fun = lambda t, y: fw(y, t).copy()
    solver = (RK45 if method == 'dopri45' else DOP853)(fun, 0.0, y0, 10.0, rtol=rtol, atol=atol)
    y_new, f_new = rk_step(fun, 0.0, y0, fun(0.0, y0), h, solver.A, solver.B, solver.C, solver.K)
    scale = atol + np.maximum(np.abs(y0), np.abs(y_new)) * rtol
    err = solver._estimate_error_norm(solver.K, h, scale)
    print("%s: one step, err %.9g (SciPy %.9g)" % (method, r['errs'][0], err))
    assert abs(r['errs'][0] - err) <= 4e-6 * err            # float32 ratios, sums and norm
    if r['errs'][0] <= 1.0:
        assert r['n_acc'] == 1 and np.abs(r['Z'][1] - y_new).max() <= 8 * np.finfo(float).eps * np.abs(y_new).max()
    else:
        assert r['n_rej'] == 1
    # with sensitivities: the same tableau on [y | S], the value after an ACCEPTED step of a tenth the size
    hs = h / 10
    N = gm.n_vars * (1 + gm.n_sens)
    z0 = ec.init_of('cascade20')
    fs = oo._wrap_c(gm.c_library().sbm_sens_rhs, N, p)
    funs = lambda t, z: fs(z, t).copy()
    K = np.empty((solver.K.shape[0], N))
    z_new, _ = rk_step(funs, 0.0, z0, funs(0.0, z0), hs, solver.A, solver.B, solver.C, K)
    r = eo.integrate(gm, p, np.array([0.0, hs]), method=method, rtol=1e-3, atol=1e-6, h0=hs, init_conditions=z0)
    assert (r['n_acc'], r['n_rej']) == (1, 0)
    assert np.abs(r['Z'][1] - z_new).max() <= 8 * np.finfo(float).eps * np.abs(z_new).max()


# ---- parity and order ----
@pytest.mark.parametrize('method', ['dopri45', 'dop853'])
def test_oracle_meets_the_parity_criterion_on_the_golden_vectors(method):
    from oracle import erk_oracle as eo, odeint_oracle as oo
    g = np.load(os.path.join(GOLDEN, 'cascade20_ref.npz'))
    gm = ec.gm_of('cascade20')
    t_out = np.concatenate([[0.0], g['t'][g['idx']]])
    for v in (0, 3):
        r = eo.integrate(gm, g['P'][v], t_out, method=method, rtol=1e-9, atol=1e-18)
        assert r['status'] == 0
        tight = lambda v=v: oo.tight_solution(gm, g['P'][v], t_out, use_c=True, atol=1e-30)[1:]
        e = check_parity(r['Z'][1:], np.concatenate([g['Y'][v], g['S'][v]], axis=1), tight, what='%s oracle, vector %d' % (method, v))
        print("%s golden vector %d: %d steps, %d rejected, parity %s" % (method, v, r['n_acc'], r['n_rej'], e))


@pytest.mark.parametrize('method,q', [('dopri45', 5), ('dop853', 8)])
def test_error_falls_with_rtol_as_the_order_says(method, q):
    """Error per step is held at rtol: h ~ rtol^(1/q), and the result of order q (DOPRI45 advances with the fifth-order
    value, DOP853 with the eighth-order one) moves by h^q ~ rtol: halving rtol is 2^(1/q) times the steps and half the
    error.  One halving drowns in the cancellations of a single run's error (DOP853: 70 steps); measured end to end over
    rtol 1e-4 .. 1e-8 the exponents are 1.06 / 0.18 (DOPRI45) and 0.80 / 0.10 (DOP853) -- the steps of the start-up and the
    clipped landings do not scale."""
    from oracle import erk_oracle as eo, odeint_oracle as oo
    gm = ec.gm_of('cascade20')
    p = ec.ensemble('cascade20', 4)[0]
    t_out = ec.T_CASCADE
    tight = oo.tight_solution(gm, p, t_out, use_c=True, atol=1e-30)
    runs = [eo.integrate(gm, p, t_out, method=method, rtol=rt, atol=1e-18) for rt in (1e-4, 1e-6, 1e-8)]
    err = [ec.distance('c20-d45-all', r['Z'], tight) for r in runs]
    steps = [r['n_acc'] for r in runs]
    e_slope = np.log(err[0] / err[2]) / np.log(1e4)
    s_slope = np.log(steps[2] / steps[0]) / np.log(1e4)
    print("%s: steps %s, error %s: error ~ rtol^%.2f, steps ~ rtol^-%.3f" % (method, steps, ['%.3g' % e for e in err], e_slope, s_slope))
    assert err[0] > err[1] > err[2] > 1e-11
    assert 0.75 <= e_slope <= 1.25
    assert 0.75 / q <= s_slope <= 1.1 / q


def test_column_chunks_of_every_kernel():
    from oracle import erk_oracle as eo
    gm = ec.gm_of('cascade20')
    assert [len(c) for c in eo.chunk_columns(gm, 'RG0')] == [40] and gm.rowgroup_chunks() == {'RG0': 1, 'RG1': 5, 'RG2': 2}
    assert [len(c) for c in eo.chunk_columns(gm, 'RG1')] == [8] * 5
    assert [len(c) for c in eo.chunk_columns(gm, 'RG2')] == [20, 20]
    assert [len(c) for c in eo.chunk_columns(gm, 'mfma')] == [16, 16, 8]
    assert [len(c) for c in eo.chunk_columns(ec.gm_of('tile49_17'), 'mfma')] == [16, 1]
    assert [len(c) for c in eo.chunk_columns(ec.gm_of('michaelis_menten'), 'RG2')] == [5]
    assert eo.chunk_columns(gm, 'per_wave') == [list(range(40))]
    # the ensembles' first members do not depend on how many are drawn
    for model in ('cascade20', 'michaelis_menten'):
        assert np.array_equal(ec.ensemble(model, 64), ec.ensemble(model, 2049)[:64])
    # every problem of the GPU tests is used, every case names a problem
    used = {c[0] for c in ec.SENS_CASES + ec.STATE_CASES + ec.BUDGET_CASES}
    assert used == set(ec.PROBLEMS)


# ---- the inputs ----
@pytest.mark.parametrize('name', NAMES)
def test_inputs_qualify_and_the_bound_is_the_noise_models(name):
    """Conditions on the inputs, on the oracle alone; no vector is skipped on the GPU side."""
    pr = ec.PROBLEMS[name]
    assert 4 <= len(pr['vectors']) <= 8 and len(pr['t_out']) == 5
    s, trunc = 0.0, np.inf
    for v in pr['vectors']:
        r = ec.oracle_run(name, v)
        assert r['status'] == 0 and r['n_acc'] > 0
        assert r['err_margin'] >= ec.ERR_MARGIN, (name, v, r['err_margin'])
        assert r['land_margin'] >= ec.LAND_MARGIN, (name, v, r['land_margin'])
        for seed in ec.SEEDS:
            rn = ec.oracle_run(name, v, noise=(seed, ec.NOISE_RHS, ec.NOISE_ERR))
            assert (rn['status'], rn['n_acc'], rn['n_rej'], rn['n_try']) == (0, r['n_acc'], r['n_rej'], r['n_try']), (name, v, seed)
            s = max(s, ec.distance(name, rn['Z'], r['Z']))
        trunc = min(trunc, ec.distance(name, r['Z'], ec.tight(name, v)))
    print("%s: s = %.3g (literal %.3g), bound %.3g, truncation %.3g" % (name, s, pr['S'], 8 * pr['S'], trunc))
    # S is a measurement rounded up (module docstring), not a property of the project: it depends on numpy's random
    # streams and libm.  A failure of the next line alone says nothing about the kernels: measure again, for all problems.
    assert s <= pr['S'] <= 1.5 * s, (name, s, pr['S'])
    assert 8.0 * pr['S'] <= 1e-3 * trunc, (name, pr['S'], trunc)


def test_h0_cases_open_with_rejections():
    for name in ('c20-d45-all-h0', 'c20-d853-rg2-h0', 'mm-d45-h0', 't49-d45-mfma-h0', 's-c20-d45-h0'):
        for v in ec.vectors_of(name):
            r = ec.oracle_run(name, v)
            first = (r['runs'][0] if 'runs' in r else r)['errs']
            k = int(np.argmax(first <= 1.0))
            assert k >= 4 and np.all(first[:k] > 1.0), (name, v, k)


# ---- the bound bites ----
# (mutation, problem, caught on every vector / on one at least: the landing rule and the state's share of the norm decide
#  something on few runs only -- 16 landings per problem; the sensitivities nearly always carry the largest error)
MUTANTS = [('A65', 'c20-d45-all', all), ('A65', 'c20-d853-all', all), ('E5', 'c20-d45-all', all), ('E5', 'c20-d853-all', all),
           ('E3', 'c20-d853-all', all), ('landing', 'c20-d853-all', any), ('clip_max', 'c20-d45-rg1-init', all),
           ('clip_max', 'c20-d853-all', all), ('fac_max', 'c20-d45-all', all), ('state_norm', 'mm-d45', any),
           ('state_norm', 's-c20-d45', all), ('hinit_all', 'c20-d45-rg1-init', all), ('hinit_all', 'c20-d853-rg2-init', all)]


@pytest.mark.parametrize('mutation,name,quant', MUTANTS, ids=['%s-%s' % m[:2] for m in MUTANTS])
def test_one_error_in_the_oracle_leaves_the_bound(mutation, name, quant):
    caught = []
    for v in ec.vectors_of(name):
        r = ec.oracle_run(name, v)
        m = ec.oracle_run(name, v, mutate=mutation, max_steps=4000)     # (a wrong error weight can stall a run: capped)
        counts = (m['status'], m['n_acc'], m['n_rej']) != (0, r['n_acc'], r['n_rej'])
        d = ec.distance(name, m['Z'], r['Z'])
        caught.append(counts or d > 8.0 * ec.PROBLEMS[name]['S'])
        print("%s on %s vector %d: counts %s, distance %.3g bounds" % (mutation, name, v, 'change' if counts else 'same',
                                                                        d / (8.0 * ec.PROBLEMS[name]['S'])))
    assert quant(caught), (mutation, name, caught)


def test_budget_compared_with_greater_than_is_caught():
    """n_try > budget instead of >=: one attempt too many.  With a budget of the run's attempts less one the driver fails in
    the last interval; the mutant finishes."""
    for name in ('c20-d45-all', 's-c20-d45'):
        v = ec.vectors_of(name)[0]
        r = ec.oracle_run(name, v)
        n_try = r['n_try'][0] if isinstance(r['n_try'], list) else r['n_try']
        same = ec.oracle_run(name, v, max_steps=n_try)
        assert same['status'] == 0 and np.array_equal(same['Z'], r['Z'])
        short = ec.oracle_run(name, v, max_steps=n_try - 1)
        assert short['status'] == 1 and short['n_acc'] == r['n_acc'] - 1
        assert np.isnan(short['Z'][-1]).all() and np.array_equal(short['Z'][:-1], r['Z'][:-1])
        mutant = ec.oracle_run(name, v, mutate='budget', max_steps=n_try - 1)
        assert (mutant['status'], mutant['n_acc']) == (0, r['n_acc'])


def test_early_exit_rule_of_the_oracle():
    """max_steps < 0 on a stiff system (stiff50, state only): the step size is pinned by stability, the check at attempt 768
    finds it neither growing nor free of rejections and the horizon out of reach: SBM_MAX_STEPS there, not at the budget.
    (No GPU case is built on it: some err of such a run is within 0.004 of 1, so the input does not qualify.)"""
    from sysbio_modeling_amd import models_zoo
    from sysbio_modeling_amd.symbolic import zoo_model
    from oracle import erk_oracle as eo
    gm = zoo_model('stiff50')
    p = models_zoo.stiff_ensemble(4)[1][0]
    t_out = np.array([0.0, 2.5, 5.0, 7.5, 10.0])
    r = eo.integrate(gm, p, t_out, method='dopri45', rtol=1e-7, atol=1e-18, sens=False, max_steps=-1000)
    assert (r['status'], r['n_try']) == (1, 768) and r['n_acc'] + r['n_rej'] == 768 and r['n_rej'] >= 3
    assert np.isnan(r['Z'][1:]).all() and not np.isnan(r['Z'][0]).any()
    growing, smooth, horizon = r['exit_margins']
    assert growing > 1.05 and smooth >= 1.2 and horizon > 1.05
    assert r['err_margin'] < ec.ERR_MARGIN
    # the same budget without the early exit runs to its end
    full = eo.integrate(gm, p, t_out, method='dopri45', rtol=1e-7, atol=1e-18, sens=False, max_steps=1000)
    assert (full['status'], full['n_try']) == (1, 1000) and full['exit_margins'] is None
