"""fit_batch(geodesic=...) on the noisy one-state project of tests/test_gpu_profiles.py: 16 starts, max_iter = 60."""
import numpy as np
import pytest

from tests.test_gpu_profiles import COST_RTOL, Q, _noisy_simple_project

pytestmark = pytest.mark.gpu

V, MAX_ITER = 16, 60


@pytest.fixture(scope='module')
def fits(gpu_models):
    """The project, the 16 starts, and the plain fit of them that every test compares with -- computed once"""
    proj, truth = _noisy_simple_project(gpu_models('simple'))
    starts = truth[None, :] + np.random.default_rng(60).uniform(-0.5, 0.5, (V, Q))
    return proj, starts, proj.fit_batch(starts, max_iter=MAX_ITER)


def test_geodesic_fit_converges_to_the_plain_fits_costs_and_counts_its_probes(fits):
    """geodesic=True: at least as many starts converge as without it; every start that converges in both fits has the plain
    fit's cost within COST_RTOL; steps were accelerated; n_evaluations = the plain count + 2 V probe vectors per iteration
    run."""
    proj, starts, plain = fits
    geo = proj.fit_batch(starts, max_iter=MAX_ITER, geodesic=True, trace=True)
    assert 'n_accelerated' not in plain
    assert geo['n_accelerated'].shape == (V,) and geo['n_accelerated'].sum() > 0
    assert np.all(geo['n_accelerated'] <= geo['n_iter'])
    assert geo['converged'].sum() >= plain['converged'].sum()
    both = geo['converged'] & plain['converged']
    assert both.sum() >= 1
    worst = float(np.max(np.abs(geo['cost'][both] - plain['cost'][both]) / plain['cost'][both]))
    iterations = len(geo['history'])
    print('geodesic: %d of %d converged (plain %d), worst |cost - plain| / plain = %.3g (bound %.3g); iterations per start %s '
          '(plain %s), accelerated %s' % (geo['converged'].sum(), V, plain['converged'].sum(), worst, COST_RTOL,
                                          geo['n_iter'].tolist(), plain['n_iter'].tolist(), geo['n_accelerated'].tolist()))
    assert worst <= COST_RTOL
    assert geo['n_evaluations'] == V + 3 * V * iterations and geo['n_jacobian_evaluations'] == V + V * iterations
    for entry in geo['history']:
        assert 0 <= entry['accelerated'] <= V and 'rho_median' in entry
    assert sum(entry['accelerated'] for entry in geo['history']) == geo['n_accelerated'].sum()


def test_a_shut_gate_is_the_fit_as_it_was_bit_for_bit(fits):
    """alpha = 0: the probes are integrated, nothing passes the gate, and theta, cost and n_iter are those of geodesic=None"""
    proj, starts, plain = fits
    shut = proj.fit_batch(starts, max_iter=MAX_ITER, geodesic=dict(alpha=0.0))
    for k in ('theta', 'cost', 'n_iter', 'converged'):
        assert np.array_equal(shut[k], plain[k]), k
    assert np.all(shut['n_accelerated'] == 0)
    assert shut['n_evaluations'] == plain['n_evaluations'] + 2 * (plain['n_evaluations'] - V)          # 2 V per iteration
    again = proj.fit_batch(starts, max_iter=MAX_ITER, geodesic=None)
    for k in ('theta', 'cost', 'n_iter', 'converged'):
        assert np.array_equal(again[k], plain[k]), k
    assert again['n_evaluations'] == plain['n_evaluations'] and 'n_accelerated' not in again


def test_a_held_parameter_stays_where_it_started_under_geodesic_steps(fits):
    proj, starts, _ = fits
    geo = proj.fit_batch(starts, max_iter=MAX_ITER, geodesic=True, held=[0])
    assert np.array_equal(geo['theta'][:, 0], starts[:, 0])
    assert geo['held'][:, 0].all() and geo['n_accelerated'].sum() > 0
    plain = proj.fit_batch(starts, max_iter=MAX_ITER, held=[0])
    both = geo['converged'] & plain['converged']
    assert geo['converged'].sum() >= plain['converged'].sum() and both.sum() >= 1
    assert np.max(np.abs(geo['cost'][both] - plain['cost'][both]) / plain['cost'][both]) <= COST_RTOL


def test_unsupported_combinations_with_geodesic_raise(fits):
    proj, starts, _ = fits
    for kw in (dict(algorithm='marquardt'), dict(algorithm='trust_region_torch'), dict(method='auto'),
               dict(method='implicit_romberg')):
        with pytest.raises(ValueError, match='trust_region'):
            proj.fit_batch(starts[:2], geodesic=True, max_iter=2, **kw)
    with pytest.raises(ValueError, match='bounds'):
        proj.fit_batch(starts[:2], geodesic=True, max_iter=2, bounds=(-20.0, 20.0))
    with pytest.raises(ValueError, match='bounds'):
        proj.profile_likelihood_batch(starts[0], params=[0], offsets=[0.1], geodesic=True, bounds=(-20.0, 20.0), max_iter=2)
    for bad in (False, 0.5, 'yes', dict(beta=1.0), dict(h=0.0), dict(h=-1.0), dict(alpha=-0.1), dict(h='x')):
        with pytest.raises(ValueError, match='geodesic'):
            proj.fit_batch(starts[:2], geodesic=bad, max_iter=2)
