"""fit_batch(held=...) and Project.profile_likelihood_batch against the reference's way of fitting,
scipy.optimize.leastsq(proj.residuals, x0, Dfun=proj.calc_project_jacobian), on the REDUCED host functions: the held
entry fixed and its column dropped."""
import warnings

import numpy as np
import pytest
from scipy.optimize import leastsq

pytestmark = pytest.mark.gpu

# both sides are lmder at ftol = 1.49e-8 on the same function, and each stops within ~0.5 ftol c* of the minimum
# (tests/test_gpu_lm_held.py measures the excesses): 100 ftol leaves room for the integrator's own tolerance
COST_RTOL = 100 * 1.49012e-8
Q = 3


def _noisy_simple_project(m):
    """The one-state project of tests/test_gpu_fitting.py::_exact_simple_project (two experiments, shared k_synt, one k_deg
    each), rebuilt here, with 2 % Gaussian noise (fixed seed) on the data: the minimum has a non-zero cost."""
    from sysbio_modeling_amd.experiment import Experiment
    from sysbio_modeling_amd.measurement import TimecourseMeasurement
    from sysbio_modeling_amd.project import Project
    theta_true = np.log([0.05, 0.02, 0.3])
    t = np.linspace(5.0, 100.0, 20)
    grid = np.linspace(0, 100.0, 1000)
    t_on_grid = grid[np.searchsorted(grid, t)]
    rng = np.random.default_rng(2024)
    exps = []
    for name, kd in (('Low', theta_true[1]), ('High', theta_true[0])):
        y = m.simulate(np.exp([kd, theta_true[2]]), np.concatenate([[0.0], t_on_grid]))[1:, 0]
        y = y * (1.0 + 0.02 * rng.standard_normal(y.size))
        exps.append(Experiment('%s_Deg_Exp' % name, TimecourseMeasurement('Variable_1', y, t),
                               experiment_settings={'Deg_Rate': name}))
    settings = {'Global': ['k_synt'], 'Shared': {'Group_1': {'k_deg': ('Deg_Rate',)}}}
    proj = Project(m, exps, settings, {'Variable_1': ('direct', 0)}, reference_compat=False)
    truth = np.zeros(Q)
    truth[proj.get_param_index('Group_1', ('High',))] = theta_true[0]
    truth[proj.get_param_index('Group_1', ('Low',))] = theta_true[1]
    truth[proj.get_param_index('k_synt', 'Global')] = theta_true[2]
    return proj, truth


def host_cost(proj, x):
    r = proj.residuals(x)
    return 0.5 * float(r @ r)


def host_fit(proj, x0, i):
    """leastsq at default tolerances on the reduced host functions: entry i fixed at x0[i], its column dropped."""
    free = [c for c in range(len(x0)) if c != i]

    def full(z):
        x = np.array(x0, dtype=np.float64)
        x[free] = z
        return x
    z = leastsq(lambda z: proj.residuals(full(z)), np.asarray(x0)[free], Dfun=lambda z: proj.calc_project_jacobian(full(z))[:, free])[0]
    x = full(z)
    return x, host_cost(proj, x)


@pytest.fixture(scope='module')
def noisy(gpu_models):
    proj, truth = _noisy_simple_project(gpu_models('simple'))
    fit = proj.fit_batch(truth[None, :], max_iter=60)
    assert fit['converged'].all() and fit['cost'][0] > 1e-3          # the noise leaves a cost
    return proj, truth, fit['theta'][0]


@pytest.mark.parametrize('i', range(Q))
def test_fit_with_a_held_parameter_matches_leastsq_on_the_reduced_problem(noisy, i):
    """16 starts, parameter i held at truth + 0.3: every converged start's cost against leastsq on the reduced host
    functions from the same start, within 100 ftol; the held column comes back untouched."""
    proj, truth, _ = noisy
    rng = np.random.default_rng(40 + i)
    starts = truth[None, :] + rng.uniform(-0.5, 0.5, (16, Q))
    starts[:, i] = truth[i] + 0.3
    fit = proj.fit_batch(starts, held=[i], max_iter=60)
    assert np.array_equal(fit['theta'][:, i], starts[:, i])
    assert fit['held'].shape == (16, Q) and fit['held'][:, i].all() and fit['held'].sum() == 16
    assert fit['converged'].sum() >= 12
    worst = 0.0
    for v in np.nonzero(fit['converged'])[0]:
        _, c = host_fit(proj, starts[v], i)
        worst = max(worst, abs(fit['cost'][v] - c) / c)
    print('parameter %d held: %d of 16 converged, worst |cost - leastsq| / leastsq = %.3g (bound %.3g)'
          % (i, fit['converged'].sum(), worst, COST_RTOL))
    assert worst <= COST_RTOL


def test_held_forms_agree_and_none_is_the_fit_as_it_was(noisy):
    proj, truth, _ = noisy
    rng = np.random.default_rng(50)
    V = 6
    starts = truth[None, :] + rng.uniform(-0.5, 0.5, (V, Q))
    mask = np.array([False, True, False])
    a = proj.fit_batch(starts, held=[1], max_iter=30)
    for form in (mask, np.tile(mask, (V, 1)), [-2]):
        b = proj.fit_batch(starts, held=form, max_iter=30)
        for k in ('theta', 'cost', 'n_iter', 'converged', 'held'):
            assert np.array_equal(a[k], b[k]), (form, k)
    i_low = proj.get_param_index('Group_1', ('Low',))
    b = proj.fit_batch(starts, held=[('Group_1', ('Low',))], max_iter=30)
    assert b['held'][:, i_low].all() and b['held'].sum() == V and np.array_equal(b['theta'][:, i_low], starts[:, i_low])
    # a different parameter per start, one start with nothing free: it comes back as it came, converged
    per = np.zeros((V, Q), dtype=bool)
    per[np.arange(V), np.arange(V) % Q] = True
    per[4] = True
    c = proj.fit_batch(starts, held=per, max_iter=30)
    assert np.array_equal(c['theta'][per], starts[per]) and c['converged'][4] and c['n_iter'][4] == 0
    assert np.array_equal(c['held'], per) and c['converged'].sum() >= V - 1
    # held=None: today's call, twice
    x = proj.fit_batch(starts, max_iter=30)
    y = proj.fit_batch(starts, max_iter=30, held=None)
    assert 'held' not in x and 'held' not in y
    for k in ('theta', 'cost', 'n_iter', 'converged'):
        assert np.array_equal(x[k], y[k]), k
    assert x['n_evaluations'] == y['n_evaluations']


def test_unsupported_combinations_with_held_raise(noisy):
    proj, truth, _ = noisy
    starts = np.tile(truth, (2, 1))
    for kw in (dict(algorithm='marquardt'), dict(algorithm='trust_region_torch'), dict(method='auto'),
               dict(method='implicit_romberg')):
        with pytest.raises(ValueError, match='trust_region'):
            proj.fit_batch(starts, held=[0], max_iter=2, **kw)
    for bad in (np.zeros(Q + 1, dtype=bool), np.zeros((3, Q), dtype=bool), [Q], [0.5]):
        with pytest.raises(ValueError):
            proj.fit_batch(starts, held=bad, max_iter=2)


@pytest.fixture(scope='module')
def profiled(noisy):
    proj, truth, theta_hat = noisy
    prof = proj.profile_likelihood_batch(theta_hat, offsets=[0.1, 0.2, 0.3])
    return prof


def test_profile_structure_and_costs_against_serial_host_fits(noisy, profiled):
    """Shapes, centre, ascending grid, held entries exactly on the grid; every converged point's cost against the serial
    host profile -- leastsq on the reduced functions, started from the previous point's host optimum (18 host fits)."""
    proj, truth, theta_hat = noisy
    prof, K = profiled, 3
    assert prof['param_index'].tolist() == [0, 1, 2]
    assert prof['value'].shape == prof['cost'].shape == prof['converged'].shape == prof['delta_chi2'].shape == (Q, 2 * K + 1)
    assert prof['theta'].shape == (Q, 2 * K + 1, Q)
    assert np.all(np.diff(prof['value'], axis=1) > 0)
    assert np.array_equal(prof['value'][:, K], theta_hat) and np.all(prof['cost'][:, K] == prof['cost_hat'])
    assert np.all(prof['theta'][:, K] == theta_hat[None, :]) and prof['converged'][:, K].all()
    assert prof['cost_hat'] == pytest.approx(host_cost(proj, theta_hat), rel=COST_RTOL)
    assert np.array_equal(prof['delta_chi2'], 2.0 * (prof['cost'] - prof['cost_hat']))
    for j in range(Q):
        assert np.array_equal(prof['theta'][j, :, j], prof['value'][j])
    assert np.all(np.isfinite(prof['cost'])) and prof['converged'].sum() >= 0.8 * prof['converged'].size
    assert np.all(prof['delta_chi2'] >= -1e-6 * prof['cost_hat'])
    assert prof['n_evaluations'] > 3 * 6
    worst = 0.0
    for j in range(Q):
        for step in (-1, 1):
            x = theta_hat.copy()
            for k in range(1, K + 1):
                x[j] = prof['value'][j, K + step * k]
                x, c = host_fit(proj, x, j)
                if prof['converged'][j, K + step * k]:
                    worst = max(worst, abs(prof['cost'][j, K + step * k] - c) / c)
    print('profile: worst |cost - serial host leastsq| / leastsq = %.3g (bound %.3g); delta_chi2 at +-0.3: %s'
          % (worst, COST_RTOL, prof['delta_chi2'][:, [0, -1]].round(3).tolist()))
    assert worst <= COST_RTOL


def test_profile_without_continuation_and_with_a_stop(noisy, profiled):
    proj, truth, theta_hat = noisy
    prof, K = profiled, 3
    flat = proj.profile_likelihood_batch(theta_hat, offsets=[0.1, 0.2, 0.3], continuation=False)
    both = prof['converged'] & flat['converged']
    assert both.sum() >= 0.8 * both.size
    rel = np.abs(flat['cost'][both] - prof['cost'][both]) / prof['cost'][both]
    print('continuation=False against continuation=True: worst relative cost difference %.3g' % rel.max())
    assert rel.max() <= COST_RTOL
    assert np.array_equal(flat['value'], prof['value'])
    # stop at the smallest positive delta_chi2 seen at offset 0.2
    at02 = prof['delta_chi2'][:, [K - 2, K + 2]]
    stop = float(at02[at02 > 0].min())
    cut = proj.profile_likelihood_batch(theta_hat, offsets=[0.1, 0.2, 0.3], stop_delta_chi2=stop)
    ended_early = 0
    for j in range(Q):
        for step in (-1, 1):
            over = False
            for k in range(1, K + 1):
                c = K + step * k
                if over:                         # after the point that exceeded: NaN, not converged
                    assert np.isnan(cut['cost'][j, c]) and np.all(np.isnan(cut['theta'][j, c])) and not cut['converged'][j, c]
                    assert np.isnan(cut['delta_chi2'][j, c])
                    continue
                # up to and including the point that exceeds: kept, and the point of the full profile
                assert cut['cost'][j, c] == pytest.approx(prof['cost'][j, c], rel=COST_RTOL)
                assert cut['theta'][j, c, j] == cut['value'][j, c]
                if cut['delta_chi2'][j, c] > stop:
                    over = True
                    ended_early += k < K
    assert np.array_equal(cut['value'], prof['value'])
    assert ended_early >= 4, ended_early                 # every branch but the marginal one(s) is over the smallest by offset 0.2
    assert cut['n_evaluations'] < prof['n_evaluations']
    # the same ends without continuation, after the fact
    cut_flat = proj.profile_likelihood_batch(theta_hat, offsets=[0.1, 0.2, 0.3], stop_delta_chi2=stop, continuation=False)
    assert np.isnan(cut_flat['cost']).sum() >= 4 and not cut_flat['converged'][np.isnan(cut_flat['cost'])].any()


def test_profile_batch_on_the_sloppy_cascade_project(gpu_models, golden):
    """One pass where per-start masks differ at scale: the 44-parameter config-4 project with two experiments, six
    parameters, two grid steps, 15 iterations per fit.  Structure and monotone sanity only: the problem is sloppy.

    theta_hat is a fixture (tests/golden/cascade_config4_n2_theta_hat.npy, make_golden_cascade_theta_hat.py): the point
    where lmder, from the nominal parameters, meets its DEFAULT tolerances -- the tolerances the profile fits stop by --
    after 1293 iterations (8 s: too long for a test), cost 39.77174.  From it 5 of the 24 profile points converge within
    15 iterations, all of them above cost_hat (by 6.6e-6 cost_hat and more); points that did not converge come out up to
    1.8e-5 cost_hat below, the valley floor being flatter than ftol resolves (6000 more iterations at ftol = 1e-13 reach
    39.77000 and still descend), so the inequality is asked of converged points only -- and of at least one.  A theta_hat
    fitted here in 100 iterations (cost 39.8805) lets converged points come out 3e-4 below cost_hat: the check fails
    there, as it should."""
    from sysbio_modeling_amd import models_zoo
    m = gpu_models('cascade20')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        proj, th0 = models_zoo.cascade_config4_project(m, n_exp=2, reference_compat=False)
        theta_hat = golden('cascade_config4_n2_theta_hat.npy')
        assert theta_hat.shape == th0.shape
        prof = proj.profile_likelihood_batch(theta_hat, params=range(6), offsets=[0.1, 0.2], max_iter=15)
    q = th0.size
    assert prof['param_index'].tolist() == list(range(6))
    assert prof['cost'].shape == (6, 5) and prof['theta'].shape == (6, 5, q)
    assert np.all(np.isfinite(prof['cost']))
    assert prof['cost_hat'] == pytest.approx(39.77174, rel=1e-5)          # the fixture is the point it claims to be
    for j in range(6):
        assert np.array_equal(prof['theta'][j, :, j], prof['value'][j])
        assert np.array_equal(prof['value'][j], theta_hat[j] + np.array([-0.2, -0.1, 0.0, 0.1, 0.2]))
    conv = prof['converged']
    print('cascade profile: cost_hat %.8g; %d of %d points converged, delta_chi2 / cost_hat from %.3g to %.3g, %d evaluations'
          % (prof['cost_hat'], conv.sum() - 6, conv.size - 6, (prof['delta_chi2'] / prof['cost_hat']).min(),
             (prof['delta_chi2'] / prof['cost_hat']).max(), prof['n_evaluations']))
    assert conv.sum() - 6 >= 1                       # beside the six centres: the inequality below is about something
    assert np.all(prof['cost'][conv] >= prof['cost_hat'] - 1e-6 * prof['cost_hat'])
