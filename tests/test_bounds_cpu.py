"""The parts of the box-constrained fits that need no GPU: the normaliser of fit_batch's ``bounds`` argument, the
declaration / binding of sbm_lm_trust_step_bounded, and the algorithm itself -- tests/support/bounded_lm_oracle.py, the
numpy statement of the bounded step and its loop -- against scipy.optimize.least_squares(method='trf', bounds=...)."""
import os
import re

import numpy as np
import pytest

from oracle import lmder_oracle as lo
from sysbio_modeling_amd.project.fitting import normalize_bounds
from tests.support import bounded_lm_oracle as bo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


class _Names:
    """What normalize_bounds needs of a project: get_param_index."""
    idx = {'k_synt': {'Global': 2}, 'Group_1': {('High',): 0, ('Low',): 1}}

    def get_param_index(self, group, settings='all'):
        return self.idx[group] if isinstance(settings, str) and settings == 'all' else self.idx[group][settings]


def test_every_form_of_bounds_gives_the_same_arrays():
    V, q = 4, 3
    lo_row, hi_row = np.array([-1.0, -INF, 0.5]), np.array([2.0, 3.0, INF])
    want = np.tile(lo_row, (V, 1)), np.tile(hi_row, (V, 1))
    forms = [(lo_row, hi_row), (want[0].copy(), want[1].copy()), (lo_row.tolist(), hi_row), (lo_row, want[1].copy()),
             [lo_row, hi_row],
             {('Group_1', ('High',)): (-1.0, 2.0), ('Group_1', ('Low',)): (-INF, 3.0), ('k_synt', 'Global'): (0.5, INF)}]
    for form in forms:
        got = normalize_bounds(form, V, q, _Names())
        for g, w in zip(got, want):
            assert g.dtype == np.float64 and g.shape == (V, q) and g.flags['C_CONTIGUOUS'] and g.flags['WRITEABLE'], form
            assert np.array_equal(g, w), form
    # scalars; a dict with 'all'; a dict that names nothing
    a, b = normalize_bounds((-50, 50.0), V, q)
    assert np.all(a == -50.0) and np.all(b == 50.0) and a.shape == b.shape == (V, q)
    a, b = normalize_bounds({('Group_1', 'all'): (-2.0, 2.0)}, V, q, _Names())
    assert np.array_equal(a, np.tile([-2.0, -2.0, -INF], (V, 1))) and np.array_equal(b, np.tile([2.0, 2.0, INF], (V, 1)))
    a, b = normalize_bounds({}, V, q, _Names())
    assert np.all(a == -INF) and np.all(b == INF)
    # lower == upper is a box
    a, b = normalize_bounds((1.0, 1.0), V, q, thetas0=np.ones((V, q)))
    assert np.array_equal(a, b)


@pytest.mark.parametrize('bad', [
    (np.zeros(4), np.ones(3)), (np.zeros(3), np.ones((3, 3))), (np.zeros((4, 3, 1)), 1.0), (0.0, 1.0, 2.0), 5.0, None,
    (np.array([0.0, np.nan, 0.0]), 1.0), (0.0, np.nan), (1.0, 0.0), (np.zeros(3), np.array([1.0, -1e-300, 1.0])),
    {('Group_1', ('Medium',)): (0.0, 1.0)}, {('nothing', 'Global'): (0.0, 1.0)}, {('k_synt', 'Global'): (1.0, 0.0)},
    {('k_synt', 'Global'): 1.0}, {2: (0.0, 1.0)}, ('a', 'b')])
def test_bad_bounds_raise(bad):
    with pytest.raises(ValueError):
        normalize_bounds(bad, 4, 3, _Names())


def test_an_infeasible_start_is_refused_unless_its_column_is_held():
    V, q = 2, 3
    x0 = np.array([[0.0, 0.5, 1.0], [0.0, 2.5, 1.0]])
    bounds = (np.array([-1.0, 0.0, -1.0]), np.array([1.0, 2.0, 1.0]))
    with pytest.raises(ValueError, match='infeasible'):
        normalize_bounds(bounds, V, q, thetas0=x0)
    with pytest.raises(ValueError, match='infeasible'):
        normalize_bounds(bounds, V, q, thetas0=-x0)
    held = np.zeros((V, q), dtype=bool)
    held[1, 1] = True
    a, b = normalize_bounds(bounds, V, q, thetas0=x0, held=held)
    # the held column is exempt altogether: it comes back unbounded; a start ON its bound is feasible
    assert a[1, 1] == -INF and b[1, 1] == INF and a[0, 1] == 0.0 and b[0, 1] == 2.0 and b[1, 2] == 1.0
    # lower > upper in a held column does not count either
    a, b = normalize_bounds((np.array([0.0, 3.0, 0.0]), np.array([1.0, 2.0, 1.0])), 1, 3, held=np.array([[False, True, False]]))
    assert a[0, 1] == -INF and b[0, 1] == INF
    with pytest.raises(ValueError, match='names need the project'):
        normalize_bounds({('k_synt', 'Global'): (0.0, 1.0)}, V, q)


def test_header_declares_the_bounded_step_and_the_binding_has_four_more_pointers():
    import ctypes
    from sysbio_modeling_amd import _lib
    with open(os.path.join(REPO, 'include', 'sbm.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+SBM_ABI_VERSION\s+4\b', header) and _lib.ABI_VERSION == 4
    decl = re.search(r'int\s+sbm_lm_trust_step_bounded\s*\(([^;]*)\)\s*;', header)
    decl_held = re.search(r'int\s+sbm_lm_trust_step_held\s*\(([^;]*)\)\s*;', header)
    assert decl and decl_held
    args, args_held = [a.strip() for a in decl.group(1).split(',')], [a.strip() for a in decl_held.group(1).split(',')]
    assert args[:-3] == args_held
    assert re.fullmatch(r'const\s+double\s*\*\s*lower_dev', args[-3]) and re.fullmatch(r'const\s+double\s*\*\s*upper_dev', args[-2])
    assert re.fullmatch(r'int32_t\s*\*\s*active_out_dev', args[-1])
    sig = _lib.SIGNATURES
    res, b_args = sig['sbm_lm_trust_step_bounded']
    res_held, held_args = sig['sbm_lm_trust_step_held']
    assert res is res_held is ctypes.c_int
    assert list(b_args[:-3]) == list(held_args) and all(a is ctypes.c_void_p for a in b_args[-3:]) and len(b_args) == len(args)
    # the wrapper and the kernel exist where the header says they do
    with open(os.path.join(REPO, 'sysbio_modeling_amd', 'csrc', 'sbm_core.hip')) as fh:
        assert re.search(r'extern\s+"C"\s+int\s+sbm_lm_trust_step_bounded\s*\(', fh.read())
    with open(os.path.join(REPO, 'sysbio_modeling_amd', 'csrc', 'sbm_lm.hpp')) as fh:
        assert re.search(r'__global__[^;{]*k_lm_trust_bounded\s*\(', fh.read())


@pytest.fixture(scope='module')
def baseline():
    probs = lo.problems()
    ref, w = bo.scipy_bounded_baseline(probs)
    return probs, ref, w


def test_the_bounds_cut_off_the_unconstrained_optimum(baseline):
    """What the loop test below rests on: in every problem scipy's constrained solution has parameters 1 and 2 (and 7 of the
    12-parameter problem) on their bounds and a cost above the unconstrained one; the loose interval of parameter 0 is not
    reached."""
    probs, ref, w = baseline
    for pb, rf in zip(probs, ref):
        xs = bo.unconstrained_optimum(pb)
        assert rf['at_bound'][1] == 1 and rf['at_bound'][2] == -1 and rf['at_bound'][0] == 0, (pb.name, rf['at_bound'])
        if pb.q == 12:
            assert rf['at_bound'][7] == 1
        assert rf['cstar'] > 0.5 * float(pb.fun(xs) @ pb.fun(xs)) * (1 + 1e-6)
        assert np.all(rf['starts'] >= rf['lower']) and np.all(rf['starts'] <= rf['upper'])


def test_bounded_oracle_loop_reaches_scipys_constrained_minimum(baseline):
    """tests/support/bounded_lm_oracle.py's loop on the three problems x eight starts, bounds from each problem's
    unconstrained optimum, starts clipped into the box.  Every start converges within 100 iterations; its excess over c*
    (scipy's least_squares 'trf' at 1e-14) is at most ten times w, scipy's own worst excess at default tolerances, in units
    of ftol c* (the rule of tests/test_gpu_lm_held.py's loop; w is computed here and printed); the parameters on bounds are
    scipy's; every trial point lies in the box bit for bit."""
    probs, ref, w = baseline
    print('scipy least_squares(trf, bounds): worst excess at default tolerances w = %.3g ftol c*' % w)
    assert w > 0.0
    worst, most_iter, fours = -np.inf, 0, 0
    for pb, rf in zip(probs, ref):
        for s, x0 in enumerate(rf['starts']):
            fit = bo.bounded_fit(pb.fun, pb.jac, x0, rf['lower'], rf['upper'], max_iter=100)
            assert fit['done'] == 1, ('not converged in 100 iterations', pb.name, s)
            most_iter, fours = max(most_iter, fit['n_iter']), fours + fit['statuses'].count(4)
            for t in fit['trials']:
                assert np.all(t >= rf['lower']) and np.all(t <= rf['upper']), (pb.name, s)
            excess = (fit['cost'] - rf['cstar']) / (lo.FTOL * rf['cstar'])
            worst = max(worst, excess)
            assert excess <= 10.0 * w, (pb.name, s, excess, w)
            at = (fit['x'] == rf['upper']).astype(int) - (fit['x'] == rf['lower']).astype(int)
            assert np.array_equal(at, rf['at_bound']), (pb.name, s, at, rf['at_bound'])
    print('bounded oracle loop: worst excess %.3g ftol c* (bound %.3g), at most %d iterations, %d steps of status 4 in 24 fits'
          % (worst, 10.0 * w, most_iter, fours))


def test_oracle_step_statuses():
    """Steps 2, 5 and 6 on two-parameter systems small enough to work by hand.  J = I, r = (1, -1): g = (1, -1), the
    Gauss-Newton step is (-1, 1)."""
    J, r, z = np.eye(2), np.array([1.0, -1.0]), np.zeros(2)
    free = bo.bounded_step(J, r, z, 1e3, 0.0, z, np.full(2, -INF), np.full(2, INF))
    assert free['status'] == 0 and np.allclose(free['delta'], [-1.0, 1.0]) and free['active'].tolist() == [0, 0]
    # both on a bound with the gradient pushing outward: status 3; the caller holding both: status 2
    s3 = bo.bounded_step(J, r, z, 1e3, 0.0, z, np.array([0.0, -INF]), np.array([INF, 0.0]))
    assert s3['status'] == 3 and s3['active'].tolist() == [2, 3] and np.all(s3['delta'] == 0) and np.all(s3['dscale'] == 0)
    assert bo.bounded_step(J, r, z, 1e3, 0.0, z, np.full(2, -INF), np.full(2, INF), held=[1, 1])['status'] == 2
    # on the bounds with the gradient pushing INWARD: free
    inward = bo.bounded_step(J, r, z, 1e3, 0.0, z, np.array([-INF, 0.0]), np.array([0.0, INF]))
    assert inward['active'].tolist() == [0, 0] and inward['status'] == 0 and not inward['projected'].any()
    # projection: the first component stops on its bound, bit for bit
    pj = bo.bounded_step(J, r, z, 1e3, 0.0, z, np.array([-0.25, -INF]), np.full(2, INF))
    assert pj['status'] == 0 and pj['projected'].tolist() == [True, False] and pj['trial'][0] == -0.25
    assert pj['gtx'] == pytest.approx(-1.25) and pj['pred'] == pytest.approx(1.25 - 0.5 * (0.0625 + 1.0))
