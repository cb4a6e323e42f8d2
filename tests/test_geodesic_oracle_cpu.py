"""tests/support/geodesic_oracle.py -- the reference of sbm_lm_geodesic and of fit_batch(geodesic=...) -- checked on the
CPU: its second derivative against an analytic one, its loop against oracle/lmder_oracle.py's with the gate shut, and
against MINPACK's minima with the gate open."""
import numpy as np

from oracle import lmder_oracle as lo
from tests.support import geodesic_oracle as go

EPS = np.finfo(np.float64).eps


def test_second_derivative_of_a_quadratic_residual_is_exact_to_the_rounding_of_the_difference_quotient():
    """lo.problems()[2]: r = A x + 0.1 (B x)^2 - b is quadratic in x, so the second directional derivative along v is
    0.2 (B v)^2 whatever h, and the difference quotient has no truncation error.  The two ends of the probe and J are
    evaluated in longdouble at the exact points and rounded to float64 -- the oracle's inputs --, so what is left is that
    rounding: eps (|r_probe| + |r_base|) 2 / h^2 per row, plus eps (2 / h) |J| |v| for J v."""
    pb = lo.problems()[2]
    c = {k: np.asarray(a, dtype=go.LD) for k, a in pb.consts.items()}
    rng = np.random.default_rng(5)
    worst = 0.0
    for x0 in pb.starts:
        for h in (go.H, 0.5, 1.0e-2):
            v = rng.standard_normal(pb.q)
            x, hv = np.asarray(x0, dtype=go.LD), go.LD(h) * np.asarray(v, dtype=go.LD)
            r_base = pb._r(c, x[None])[0].astype(np.float64)
            r_probe = pb._r(c, (x + hv)[None])[0].astype(np.float64)
            J = pb._J(c, x[None])[0].astype(np.float64)
            got = go.rvv_reference(J, r_base, r_probe, v, h)
            Bv = c['B'] @ np.asarray(v, dtype=go.LD)
            want = go.LD(0.2) * Bv * Bv
            bound = EPS * (np.abs(r_probe) + np.abs(r_base)) * 2.0 / h ** 2 + EPS * (2.0 / h) * (np.abs(J) @ np.abs(v))
            err = np.abs(got - want).astype(np.float64)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (h, float(np.max(err / bound)))
    print('r_vv of the quadratic problem: worst error %.3g of the bound' % worst)


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_with_the_gate_shut_the_loop_is_lmder_oracles_loop():
    """alpha = 0: no acceleration passes the gate, and every argument and result of lm_update_reference, iteration by
    iteration, is lo.fit_reference's exactly."""
    for pb in lo.problems():
        for x0 in pb.starts:
            want = lo.fit_reference(pb.fun, pb.jac, x0)
            got = go.geodesic_fit_reference(pb.fun, pb.jac, x0, alpha=0.0)
            assert got['n_accel'] == 0 and go.APPLIED not in got['accel_status']
            assert len(got['trace']) == len(want['trace'])
            for (ga, gout), (wa, wout) in zip(got['trace'], want['trace']):
                assert all(same(a, b) for a, b in zip(ga, wa))
                assert gout == wout
            assert np.array_equal(got['x'], want['x']) and got['cost'] == want['cost'] and got['n_iter'] == want['n_iter']


def test_with_the_defaults_every_start_reaches_minpacks_minimum():
    """h = 0.1, alpha = 0.75: every start lo.minpack_baseline keeps converges, within ten times MINPACK's own worst excess
    over c* at default tolerances (the criterion of tests/test_lmder_oracle.py).  Printed: the excess per problem, the
    iterations and the accelerated steps beside lo.fit_reference's iterations."""
    probs = lo.problems()
    cstar, keep, minpack_worst = lo.minpack_baseline(probs)
    assert keep.sum() >= 20
    for i, pb in enumerate(probs):
        worst, iters, plain, acc = 0.0, [], [], []
        for s, x0 in enumerate(pb.starts):
            fit = go.geodesic_fit_reference(pb.fun, pb.jac, x0)
            iters.append(fit['n_iter'])
            acc.append(fit['n_accel'])
            plain.append(lo.fit_reference(pb.fun, pb.jac, x0)['n_iter'])
            if keep[i, s]:
                assert fit['done'] == 1, (pb.name, s)
                excess = (fit['cost'] - cstar[i]) / (lo.FTOL * cstar[i])
                worst = max(worst, excess)
                assert excess <= 10.0 * minpack_worst, (pb.name, s, excess, minpack_worst)
        print('%s: worst excess %.3g ftol c* (MINPACK %.3g); iterations %s (plain lmder %s), accelerated %s'
              % (pb.name, worst, minpack_worst, iters, plain, acc))
