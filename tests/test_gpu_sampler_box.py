"""``ensemble_log_params_batch(held=, bounds=)`` on the device: 'device' and 'device_recalc' with ``draws=`` against a host
replay of the same rule with the same draws, a held and bounded run on the 68-parameter cascade project, and the two
samplers without the keywords."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CUTOFF = 1e-4


@pytest.fixture(scope='module')
def sf_project(gpu_models):
    """The scale-factor project of the samplers' replay tests (tests/test_gpu_sampler_device.py): model 'simple', one
    measure with a scale factor, a log prior (0.1, 1.0) on it, 5 % error bars; q = 2.  (project, truth, J^T J at the truth)"""
    from sysbio_modeling_amd.experiment import Experiment
    from sysbio_modeling_amd.measurement import TimecourseMeasurement
    from sysbio_modeling_amd.project import Project
    m = gpu_models('simple')
    t = np.linspace(5.0, 100.0, 20)
    grid = np.linspace(0, 100.0, 1000)
    y = m.simulate(np.array([0.05, 0.3]), np.concatenate([[0.0], grid[np.searchsorted(grid, t)]]))[1:, 0]
    exp = Experiment('E', TimecourseMeasurement('Variable_1', y, t, 0.05 * y))
    proj = Project(m, [exp], {'Global': ['k_deg', 'k_synt']}, {'Variable_1': ('direct', 0)}, reference_compat=False,
                   sf_groups=[frozenset(['Variable_1'])])
    proj.set_scale_factor_log_prior('Variable_1', 0.1, 1.0)
    truth = np.zeros(2)
    truth[proj.get_param_index('k_deg', 'Global')] = np.log(0.05)
    truth[proj.get_param_index('k_synt', 'Global')] = np.log(0.3)
    J = proj.calc_project_jacobian(truth)
    return proj, truth, J.T @ J


def _kernel_signs(V):
    """the sign convention of sbm_sampling_axes on (padded) axes: the component of largest magnitude positive"""
    idx = np.argmax(np.abs(V), axis=-2)
    sign = np.sign(np.take_along_axis(V, idx[..., None, :], axis=-2))
    return V * np.where(sign == 0.0, 1.0, sign)


def _host_replay(proj, starts, hess, z, log_u, T, energy, recalc, held, lower, upper):
    """The rule of ``ensemble_log_params_batch(held=, bounds=)`` with given draws, in numpy: held components stay, a
    candidate with a free component outside the box is rejected and its chain's current point evaluated in its place.
    Returns the record, the acceptance ratio, the number of candidates that left the box, and the smallest
    |log u - log ratio| over the decisions that were taken by the ratio."""
    from sysbio_modeling_amd.project.ensembles import _log_candidate_density, sampling_axes
    C, q = starts.shape

    def evaluate(th):
        # (the integration the sampler itself runs: with sensitivities only where their Jacobians are used)
        res = proj.evaluate_batch(th, jacobian=recalc, want=('sims', 'norms', 'status') + (('jacobian',) if recalc else ()))
        out = 0.5 * res['norms']
        if energy == 'free_energy':
            out = out - np.array([proj.calc_scale_factors_entropy(T, sims=s) for s in res['sims']])
        H = np.einsum('crj,crk->cjk', res['jacobian'], res['jacobian']) if recalc else None
        return np.where(np.isfinite(out) & (res['status'] == 0), out, np.inf), H

    def axes(H):
        V, s = sampling_axes(H, CUTOFF, T, 1.0, held=held)
        return (_kernel_signs(V) if recalc else V), s          # ('device' takes its matrix from the host's eigh as it comes)

    curr = starts.copy()
    Fc, H = evaluate(curr)
    V, s = axes(np.broadcast_to(hess, (C, q, q)) if (hess is not None or not recalc) else H)
    ens, ens_F, n_acc, n_out, margin = [curr.copy()], [Fc.copy()], np.zeros(C), 0, np.inf
    for n in range(len(z)):
        delta = np.where(held, 0.0, np.einsum('cij,cj->ci', V, s * z[n]))
        trial = curr + delta
        outside = (~((trial >= lower) & (trial <= upper)) & ~held).any(axis=1) | held.all(axis=1)
        n_out += int(outside.sum())
        trial = np.where(outside[:, None], curr, trial)
        Ft, Ht = evaluate(trial)
        assert np.all(np.isfinite(Ft))
        ratio = -(Ft - Fc) / T
        if recalc:
            Vn, sn = axes(Ht)
            ratio = ratio + _log_candidate_density(-delta, Vn, sn) - _log_candidate_density(delta, V, s)
        margin = min(margin, float(np.min(np.abs(log_u[n] - ratio)[~outside], initial=np.inf)))
        acc = ~outside & (log_u[n] < ratio)
        curr, Fc = np.where(acc[:, None], trial, curr), np.where(acc, Ft, Fc)
        if recalc:
            V, s = np.where(acc[:, None, None], Vn, V), np.where(acc[:, None], sn, s)
        n_acc += acc
        ens.append(curr.copy())
        ens_F.append(Fc.copy())
    return np.stack(ens), np.stack(ens_F), n_acc / len(z), n_out, margin


@pytest.mark.parametrize('case', ['bounds', 'bounds_held', 'bounds_free_energy'])
@pytest.mark.parametrize('sampler', ['device', 'device_recalc'])
def test_device_samplers_walk_the_host_chain_inside_the_box(sf_project, sampler, case):
    """4 chains x 30 steps with the same draws on both sides.  The box is the truth +- one standard deviation of the first
    candidate in either parameter, so candidates of the replay leave it (asserted); 'bounds_held' holds parameter 1.
    Acceptance counts equal exactly; positions within 1e-12 ('device') and 1e-10 ('device_recalc'), energies within
    1e-12 / 1e-8 max(1, |F|), the bounds of the replay tests without a box.  With the free energy the host's entropy is
    scipy's quadrature: there the energies are held to a fresh free_energy_batch of the recorded points instead (the
    device rule on both sides), and the counts and positions to the replay as before."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch, sampling_matrix
    proj, truth, hess = sf_project
    C, steps, T = 4, 30, 1.5
    recalc = sampler == 'device_recalc'
    energy = 'free_energy' if case == 'bounds_free_energy' else 'rss'
    held = np.broadcast_to(np.array([False, case == 'bounds_held']), (C, 2))
    rng = np.random.default_rng(300 + len(case))
    M = sampling_matrix(hess, CUTOFF, T, 1.0)
    width = np.sqrt(np.diag(M @ M.T))
    lower, upper = np.tile(truth - width, (C, 1)), np.tile(truth + width, (C, 1))
    starts = truth[None, :] + 0.5 * width * rng.uniform(-1.0, 1.0, (C, 2))
    z, log_u = rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C)))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ens_h, F_h, ratio_h, n_out, margin = _host_replay(proj, starts, hess, z, log_u, T, energy, recalc, held, lower, upper)
        ens_d, F_d, ratio_d = ensemble_log_params_batch(proj, starts, hess=hess, steps=steps, temperature=T, sing_val_cutoff=CUTOFF,
                                                        energy=energy, sampler=sampler, draws=(z, log_u),
                                                        held=held[0] if case == 'bounds_held' else None, bounds=(lower, upper))
        fresh = proj.free_energy_batch(ens_d.reshape(-1, 2), T).reshape(F_d.shape) if energy == 'free_energy' else None
    dx = np.max(np.abs(ens_d - ens_h))
    print("%s %s: %d of %d candidates outside, margin %.3e, max |dF| %.3e, max |dx| %.3e, acceptance %.2f"
          % (sampler, case, n_out, steps * C, margin, np.max(np.abs(F_d - F_h)), dx, ratio_h.mean()))
    assert n_out >= 1 and margin > 1e-6 and 0.05 < ratio_h.mean() < 0.95
    assert ens_d.shape == ens_h.shape == (steps + 1, C, 2)
    assert np.array_equal(ratio_d, ratio_h)
    assert dx <= (1e-10 if recalc else 1e-12)
    assert np.all((ens_d >= lower) & (ens_d <= upper))
    if case == 'bounds_held':
        assert np.array_equal(ens_d[:, :, 1], np.broadcast_to(starts[:, 1], (steps + 1, C)))
    if energy == 'free_energy':
        # ('device_recalc' integrates with sensitivities, free_energy_batch without: the 1e-8 of its replay test)
        assert np.all(np.abs(F_d - fresh) <= (1e-8 if recalc else 1e-12) * np.maximum(1.0, np.abs(fresh)))
    else:
        assert np.all(np.abs(F_d - F_h) <= (1e-8 if recalc else 1e-12) * np.maximum(1.0, np.abs(F_h)))


def test_device_recalc_held_and_bounded_on_the_cascade_project(gpu_models):
    """The 8-experiment cascade project (q = 68) with a log prior on each scale factor: 60 parameters held, another 60 in
    chain 3, the free ones confined to start +- 0.05; 4 chains x 10 steps of 'device_recalc' (axes of 8 x 8 problems).  Steps
    a tenth of the recipe's with a cutoff of 1e-2: the clipped directions' steps are then about the width of the box, so that
    candidates both leave it and stay (with the recipe's own length every candidate leaves it and nothing is accepted)."""
    from sysbio_modeling_amd import models_zoo
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    m = gpu_models('cascade20')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        proj, th0 = models_zoo.cascade_config4_project(m, reference_compat=False)
        for v in models_zoo.CASCADE_MEASURED_SPECIES:
            proj.set_scale_factor_log_prior('s%d' % v, 0.0, 1.0)
        q = th0.size
        assert q == 68
        C, steps = 4, 10
        held = np.ones((C, q), dtype=bool)
        held[:, np.arange(3, q, 9)[:8]] = False
        held[3] = True
        held[3, np.arange(5, q, 8)[:8]] = False
        assert np.all(held.sum(axis=1) == 60) and not np.array_equal(held[3], held[0])
        starts = np.tile(th0, (C, 1))
        lower, upper = starts - 0.05, starts + 0.05
        ens, ens_F, ratio = ensemble_log_params_batch(proj, starts, steps=steps, seeds=3, sing_val_cutoff=1e-2, step_scale=0.1,
                                                      sampler='device_recalc', held=held, bounds=(lower, upper))
        fresh = proj.free_energy_batch(ens.reshape(-1, q), 1.0).reshape(ens_F.shape)
    print("cascade, 60 of 68 held: accepted per chain %s of %d" % ((ratio * steps).round().astype(int), steps))
    assert ens.shape == (steps + 1, C, q) and ens_F.shape == (steps + 1, C)
    assert np.array_equal(ens[:, held], np.broadcast_to(starts[held], (steps + 1, held.sum())))
    assert np.all((ens >= lower) & (ens <= upper))
    assert np.all(np.isfinite(ens_F)) and np.all(np.abs(ens_F - fresh) <= 1e-8 * np.abs(fresh))
    n_acc = (ratio * steps).round().sum()
    assert 1 <= n_acc <= C * steps - 1
    moved = np.any(ens != ens[0], axis=0)
    assert np.array_equal(moved & held, np.zeros_like(held)) and moved.any()


@pytest.mark.parametrize('sampler', ['device', 'device_recalc'])
def test_without_the_keywords_nothing_changes(sf_project, sampler):
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    proj, truth, hess = sf_project
    C, steps = 4, 12
    rng = np.random.default_rng(9)
    starts = truth[None, :] + 0.01 * rng.standard_normal((C, 2))
    draws = (rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C))))
    kw = dict(hess=hess, steps=steps, temperature=1.5, sing_val_cutoff=CUTOFF, sampler=sampler, draws=draws)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = ensemble_log_params_batch(proj, starts, **kw)
        b = ensemble_log_params_batch(proj, starts, held=None, bounds=None, **kw)
        # an empty box is the same chain too: nothing held, every bound open (the box kernels instead of the plain ones)
        c = ensemble_log_params_batch(proj, starts, held=np.zeros(2, bool), bounds=(-np.inf, np.inf), **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    assert a[2].mean() > 0.0
