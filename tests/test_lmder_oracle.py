"""The lmder oracle itself (oracle/lmder_oracle.py), on the CPU: hand-worked cases of every branch, a complete loop built
on it against real MINPACK (scipy.optimize.leastsq), and the coverage of the random sweep the GPU tests run
(tests/test_gpu_lm_bookkeeping.py)."""
import collections

import numpy as np
import pytest

from oracle import lmder_oracle as lo



def check_update(out, label, want, what=''):
    """Every output of an LmUpdate-like record against the literals of a named case."""
    for key in ('radius', 'lam', 'done', 'accept', 'n_iter', 'ratio', 'live', 'accepted'):
        assert getattr(out, key) == want[key], '%s%s: %s = %r, expected %r' % (what, label, key, getattr(out, key), want[key])


def test_named_cases_one_per_branch():
    """The hand-worked cases (the arithmetic is in the comments of lmder_oracle.NAMED_CASES): every output literally, and
    the branch label and flags the case is named for.  None of them sits on a threshold."""
    d, first, expected = lo.named_cases()
    seen = set()
    for v, (label, want) in enumerate(expected):
        args = lo.update_args(d, v, lo.NAMED_FTOL, lo.NAMED_XTOL, lo.NAMED_ITERATION, first[v])
        out = lo.lm_update_reference(*args)
        check_update(out, label, want)
        assert out.branch == '+'.join((label,) + tuple(want.get('flags', ()))), (label, out.branch)
        assert not lo.lm_update_is_marginal(*args), label
        seen |= lo.labels(out.branch)
    assert seen == set(lo.BRANCHES) | set(lo.FLAGS)


def test_departures_from_lmder_and_the_parabola_guard():
    """What the oracle documents as deliberate: cost == 0 divides by 1 (and is always 'ten times worse': 0.1 |r_t| >= 0),
    pred <= 0 gives ratio 0 and no acceptance, and a positive directional derivative is refused rather than divided by."""
    th, D = [3.0, 4.0], [1.0, 1.0]
    # cost 0, trial 0.5: actred = -1, prered = 2 / 1: ratio -0.5; radius 0.1 min(8, 10)
    out = lo.lm_update_reference(0.0, 1.0, 0, 2.0, 1.0, -3.0, 0, th, D, 1e-8, 1e-8, 0, 0, 8.0, 0.5, 0, 99)
    assert (out.ratio, out.radius, out.lam, out.accept, out.branch) == (-0.5, 0.1 * 8.0, 0.5 / 0.1, 0, 'ten_x_worse')
    # pred < 0 with a worse trial point (lmder's formula would give ratio = +0.25 / 0.5 > 1e-4 and take it)
    out = lo.lm_update_reference(2.0, 5.0, 0, -1.0, 1.0, -1.0, 0, th, D, 1e-8, 1e-8, 0, 0, 8.0, 0.5, 0, 99)
    assert (out.ratio, out.accept) == (0.0, 0) and out.branch == 'shrink_parabola'
    with pytest.raises(AssertionError):
        lo.lm_update_reference(2.0, 5.0, 0, 1.0, 1.0, +1.0, 0, th, D, 1e-8, 1e-8, 0, 0, 8.0, 0.5, 0, 99)


def test_accept_reference_copies_rows():
    rng = np.random.default_rng(1)
    V, M, q = 3, 4, 2
    th, r, J, c = rng.random((V, q)), rng.random((V, M)), rng.random((V, M, q)), rng.random(V)
    tt, rt, Jt, nt = rng.random((V, q)), rng.random((V, M)), rng.random((V, M, q)), rng.random(V)
    th2, r2, J2, c2 = lo.lm_accept_reference([1, 0, 5], tt, rt, Jt, nt, th, r, J, c)
    for v, a in enumerate((1, 0, 1)):
        src = (tt, rt, Jt, 0.5 * nt) if a else (th, r, J, c)
        assert all(np.array_equal(x[v], y[v]) for x, y in zip((th2, r2, J2, c2), src))


@pytest.fixture(scope='module')
def baseline():
    return lo.minpack_baseline()


def test_fit_reference_reaches_minpack_minima(baseline):
    """fit_reference (lmpar by bisection + the oracle's bookkeeping) at the default ftol = xtol = 1.49012e-8 against
    scipy.optimize.leastsq = MINPACK on three nonzero-residual problems from eight starts each.  c* is MINPACK's minimum at
    ftol = xtol = 1e-14.  lmder's info 1 bounds the remaining relative excess by the order of ftol, so the assertion is
    cost - c* <= K ftol c* with K ten times MINPACK's own worst excess at default tolerances (ten, because lmpar's 10 %
    tolerance makes the two paths differ step by step).

    Measured (units of ftol c*): MINPACK at default tolerances 6.2e-4 at worst, the oracle loop 7.1e-4, the device loop of
    tests/test_gpu_lm_bookkeeping.py 6.2e-4; all 24 starts reach the common minimum (20 are required); 0 of the 125
    (start, iteration) pairs of these fits are marginal (2 % allowed)."""
    cstar, keep, worst = baseline
    assert keep.sum() >= 20
    assert 0.0 <= worst < 1.0
    ours, marginal, total = 0.0, 0, 0
    for i, pb in enumerate(lo.problems()):
        for j, x0 in enumerate(pb.starts):
            if not keep[i, j]:
                continue
            fit = lo.fit_reference(pb.fun, pb.jac, x0)
            assert fit['done'] == 1, (pb.name, j)
            excess = (fit['cost'] - cstar[i]) / (lo.FTOL * cstar[i])
            ours = max(ours, excess)
            assert excess <= 10.0 * worst, (pb.name, j, excess, worst)
            total += len(fit['trace'])
            marginal += sum(lo.lm_update_is_marginal(*a) for a, _ in fit['trace'])
    print('excess over c* in units of ftol c*: MINPACK %.3g, oracle loop %.3g; marginal %d of %d' % (worst, ours, marginal, total))
    assert marginal <= 0.02 * total


def test_sweep_covers_every_branch():
    """4096 draws of the sweep generator, both values of `first`: after the marginal ones are dropped (at most 5 %) every
    branch label and flag occurs at least 20 times -- and so do the cases the mutations of the kernel hinge on."""
    n = 4096
    d = lo.draw_update_inputs(n, lo.SWEEP_Q, lo.SWEEP_SEED)
    count, dropped = collections.Counter(), 0
    for first in (0, 1):
        for v in range(n):
            args = lo.update_args(d, v, lo.FTOL, lo.XTOL, 3, first)
            if lo.lm_update_is_marginal(*args):
                dropped += 1
                continue
            out = lo.lm_update_reference(*args)
            tags = lo.labels(out.branch)
            count.update(tags)
            if out.ratio is not None and 'step_failed' not in tags:
                count['ratio in (0, 1e-4)'] += 0.0 < out.ratio < 1.0e-4
                count['grow by lam == 0'] += 'grow' in tags and out.ratio < 0.75
                count['zero cost'] += d['cost'][v] == 0.0
    assert dropped <= 0.05 * 2 * n
    for tag in lo.BRANCHES + lo.FLAGS + ('ratio in (0, 1e-4)', 'grow by lam == 0', 'zero cost'):
        assert count[tag] >= 20, (tag, count[tag])
