"""fit_batch(bounds=...) and profile_likelihood_batch(bounds=...) on the noisy one-state project of
tests/test_gpu_profiles.py: a bound that cuts off the unconstrained optimum ends on the bound bit for bit, at the cost of
scipy.optimize.leastsq on the host functions with that parameter fixed there; bounds nobody reaches change nothing."""
import numpy as np
import pytest

from tests.test_gpu_profiles import COST_RTOL, Q, _noisy_simple_project, host_fit

pytestmark = pytest.mark.gpu

V = 16


@pytest.fixture(scope='module')
def noisy(gpu_models):
    proj, truth = _noisy_simple_project(gpu_models('simple'))
    fit = proj.fit_batch(truth[None, :], max_iter=60)
    assert fit['converged'].all() and fit['cost'][0] > 1e-3
    return proj, truth, fit['theta'][0]


def _starts(truth, seed):
    return truth[None, :] + np.random.default_rng(seed).uniform(-0.5, 0.5, (V, Q))


@pytest.mark.parametrize('i', range(Q))
def test_an_upper_bound_that_cuts_off_the_optimum_is_where_the_fit_ends(noisy, i):
    """upper[i] = truth[i] - 0.3, the others unbounded, 16 starts clipped into the box: at least 12 converge; those end with
    theta[:, i] == upper[i] bit for bit and at_bound +1 there, at the cost of leastsq on the host functions with
    parameter i fixed at the bound (from the same start), within 100 ftol."""
    proj, truth, _ = noisy
    upper = np.full(Q, np.inf)
    upper[i] = truth[i] - 0.3
    starts = np.minimum(_starts(truth, 60 + i), upper[None, :])
    fit = proj.fit_batch(starts, bounds=(-np.inf, upper), max_iter=60)
    conv = fit['converged']
    assert fit['at_bound'].shape == (V, Q) and fit['at_bound'].dtype == np.int8
    assert np.all(fit['theta'] <= upper[None, :])
    assert conv.sum() >= 12
    assert np.all(fit['theta'][conv, i] == upper[i]) and np.all(fit['at_bound'][conv, i] == 1)
    assert np.all(fit['at_bound'][:, [c for c in range(Q) if c != i]] == 0)
    worst = 0.0
    for v in np.nonzero(conv)[0]:
        x0 = starts[v].copy()
        x0[i] = upper[i]
        _, c = host_fit(proj, x0, i)
        worst = max(worst, abs(fit['cost'][v] - c) / c)
    print('upper bound on parameter %d: %d of 16 converged, worst |cost - leastsq at the bound| / leastsq = %.3g (bound %.3g)'
          % (i, conv.sum(), worst, COST_RTOL))
    assert worst <= COST_RTOL


def test_the_forms_of_bounds_agree(noisy):
    proj, truth, _ = noisy
    i_low = proj.get_param_index('Group_1', ('Low',))
    lower, upper = np.full(Q, -np.inf), np.full(Q, np.inf)
    lower[i_low], upper[i_low] = truth[i_low] - 2.0, truth[i_low] - 0.3
    starts = np.clip(_starts(truth, 70), lower[None, :], upper[None, :])
    a = proj.fit_batch(starts, bounds={('Group_1', ('Low',)): (truth[i_low] - 2.0, truth[i_low] - 0.3)}, max_iter=30)
    assert a['converged'].sum() >= 12 and np.all(a['at_bound'][a['converged'], i_low] == 1)
    for form in ((lower, upper), (np.tile(lower, (V, 1)), np.tile(upper, (V, 1))), (lower.tolist(), np.tile(upper, (V, 1)))):
        b = proj.fit_batch(starts, bounds=form, max_iter=30)
        for k in ('theta', 'cost', 'n_iter', 'converged', 'at_bound'):
            assert np.array_equal(a[k], b[k]), k
    assert 'at_bound' not in proj.fit_batch(starts[:2], max_iter=2)


def test_unsupported_combinations_and_bad_bounds_raise(noisy):
    proj, truth, _ = noisy
    starts = np.tile(truth, (2, 1))
    for kw in (dict(algorithm='marquardt'), dict(algorithm='trust_region_torch'), dict(method='auto')):
        with pytest.raises(ValueError, match='trust_region'):
            proj.fit_batch(starts, bounds=(-50.0, 50.0), max_iter=2, **kw)
    with pytest.raises(ValueError, match='infeasible'):
        proj.fit_batch(starts, bounds=(-50.0, truth - 0.1), max_iter=2)
    with pytest.raises(ValueError, match='lower > upper'):
        proj.fit_batch(starts, bounds=(truth + 1.0, truth - 1.0), max_iter=2)
    with pytest.raises(ValueError):
        proj.fit_batch(starts, bounds=(np.zeros(Q + 1), 50.0), max_iter=2)
    # a held column is exempt: the same box with its infeasible column held is accepted
    fit = proj.fit_batch(starts, bounds=(-50.0, np.array([truth[0] - 0.1, 50.0, 50.0])), held=[0], max_iter=2)
    assert np.array_equal(fit['theta'][:, 0], starts[:, 0]) and np.all(fit['at_bound'] == 0)


def test_bounds_that_no_iterate_reaches_leave_the_fit_where_it_was(noisy):
    """bounds = (-50, 50) with max_step = 0.5: the starts lie within 5 of the origin and 60 iterations move a parameter by
    at most 30, so no trial point or iterate can reach a bound (asserted as arithmetic, and on the result).  at_bound is
    zero, and every start converged in both fits is within 100 ftol of the unbounded fit's cost."""
    proj, truth, _ = noisy
    starts = _starts(truth, 80)
    max_iter, max_step = 60, 0.5
    assert np.abs(starts).max() + max_iter * max_step < 50.0
    free = proj.fit_batch(starts, max_iter=max_iter, max_step=max_step)
    box = proj.fit_batch(starts, bounds=(-50.0, 50.0), max_iter=max_iter, max_step=max_step)
    assert np.all(np.abs(box['theta']) < 50.0) and np.all(box['at_bound'] == 0)
    both = free['converged'] & box['converged']
    assert box['converged'].sum() >= 12 and both.sum() >= 12
    rel = np.abs(box['cost'][both] - free['cost'][both]) / free['cost'][both]
    print('loose bounds: %d of 16 converged in both fits, worst relative cost difference %.3g (bound %.3g)'
          % (both.sum(), rel.max(), COST_RTOL))
    assert rel.max() <= COST_RTOL


def test_profile_with_bounds_on_the_other_parameters(noisy):
    """profile_likelihood_batch for parameter 0 with three offsets, bounds on parameters 1 and 2 in the (q,) and the dict
    form (parameter 0, profiled and so held, gets a box its grid leaves: it is exempt).  It runs; the free parameters stay
    in the box; the held grid values are untouched; both forms give the same profile."""
    proj, truth, theta_hat = noisy
    offsets = [0.1, 0.2, 0.3]
    lower = np.array([theta_hat[0] - 0.05, theta_hat[1] - 0.02, theta_hat[2] - 1.0])
    upper = np.array([theta_hat[0] + 0.05, theta_hat[1] + 1.0, theta_hat[2] + 0.01])
    prof = proj.profile_likelihood_batch(theta_hat, params=[0], offsets=offsets, bounds=(lower, upper))
    assert prof['theta'].shape == (1, 7, Q) and np.all(np.isfinite(prof['cost']))
    assert np.array_equal(prof['theta'][0, :, 0], prof['value'][0])
    assert np.array_equal(prof['value'][0], np.concatenate([theta_hat[0] - np.array(offsets[::-1]), theta_hat[:1],
                                                            theta_hat[0] + np.array(offsets)]))
    th = prof['theta'][0]
    assert np.all(th[:, 1:] >= lower[None, 1:]) and np.all(th[:, 1:] <= upper[None, 1:])
    print('profile inside a box: %d of 6 points converged, %d of their 12 free coordinates on a bound'
          % (prof['converged'][0].sum() - 1, int(((th[:, 1:] == lower[1:]) | (th[:, 1:] == upper[1:])).sum())))
    names = {}
    for group, slots in proj.project_param_idx.items():
        for key, gi in slots.items():
            names[(group, key)] = (lower[gi], upper[gi])
    again = proj.profile_likelihood_batch(theta_hat, params=[0], offsets=offsets, bounds=names)
    for k in ('theta', 'cost', 'converged', 'value'):
        assert np.array_equal(prof[k], again[k]), k
