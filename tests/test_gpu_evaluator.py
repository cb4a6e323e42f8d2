"""DeviceEvaluator (project/_evaluation.py), the one place the Python layer calls sbm_residuals_batch / sbm_jacobian_batch
from: its buffer set against what ``Project.evaluate_batch`` returns at the same points, byte for byte, on the project
forms at which a shape rule of the set can go wrong -- no scale factor (G = 0, a null pointer), one scale-factor group,
and a parameter prior (RT = R + 1 rows)."""
import numpy as np
import pytest

from tests.test_gpu_fitting import _exact_simple_project

pytestmark = pytest.mark.gpu

TRUTH = np.log([0.05, 0.02, 0.3])
R = 40                # measurement rows: two experiments of 20
FORMS = ('plain', 'scale_factor', 'prior')
EXTRA = ('model_jacobian', 'gradient', 'sf_gradient')


@pytest.fixture(scope='module')
def projects(gpu_models):
    """The one-state two-experiment project (two experiments of 20 rows, q = 3) in the three forms:
    {form: (project, G, RT)}"""
    m = gpu_models('simple')
    out = {'plain': (_exact_simple_project(m, TRUTH), 0, R),
           'scale_factor': (_exact_simple_project(m, TRUTH, sf_groups=[frozenset(['Variable_1'])]), 1, R)}
    prior = _exact_simple_project(m, TRUTH)
    prior.set_parameter_log_prior('k_synt', 'Global', np.log(0.25), 0.5)
    out['prior'] = (prior, 0, R + 1)
    return out


def _points(V, seed):
    return TRUTH[None, :] + np.random.default_rng(seed).uniform(-0.5, 0.5, (V, 3))


def _same_bytes(buf, ref):
    assert list(buf) == list(ref)
    for key in ref:
        a, b = buf[key].cpu().numpy(), ref[key].cpu().numpy()
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), key


@pytest.mark.parametrize('V', [1, 3])
@pytest.mark.parametrize('form', FORMS)
def test_run_into_buffers_equals_evaluate_batch(projects, form, V):
    import torch
    from sysbio_modeling_amd.project._evaluation import DeviceEvaluator
    proj, G, RT = projects[form]
    ev = DeviceEvaluator(proj)
    assert (ev.R, ev.RT, ev.G, ev.q) == (R, RT, G, 3)
    th = torch.from_numpy(_points(V, 7)).cuda()
    for jacobian in (False, True):
        buf = ev.buffers(V, jacobian=jacobian, model_jacobian=jacobian, gradient=jacobian, sf_gradient=jacobian)
        shapes = {'residuals': (V, RT), 'sims': (V, R), 'sf': (V, G), 'norms': (V,), 'status': (V,), 'n_steps': (V,)}
        if jacobian:
            shapes.update({'jacobian': (V, RT, 3), 'model_jacobian': (V, R, 3), 'gradient': (V, 3)})
            if G:
                shapes['sf_gradient'] = (V, G, 3)
        assert {k: tuple(v.shape) for k, v in buf.items()} == shapes
        ev.run(th, proj._opts(), buf, jacobian)
        ref = proj.evaluate_batch(th, jacobian=jacobian, want=EXTRA if jacobian else ())
        torch.cuda.synchronize()
        assert int(ref['status'].abs().sum()) == 0 and bool(torch.isfinite(ref['norms']).all())
        _same_bytes(buf, ref)


def test_buffers_are_reusable(projects):
    """A second run into the same buffers, from other points, leaves what a fresh call returns."""
    import torch
    from sysbio_modeling_amd.project._evaluation import DeviceEvaluator
    proj = projects['scale_factor'][0]
    ev = DeviceEvaluator(proj)
    first, second = (torch.from_numpy(_points(3, seed)).cuda() for seed in (1, 2))
    for jacobian in (False, True):
        buf = ev.buffers(3, jacobian=jacobian)
        ev.run(first, proj._opts(), buf, jacobian)
        ev.run(second, proj._opts(), buf, jacobian)
        ref = proj.evaluate_batch(second, jacobian=jacobian)
        torch.cuda.synchronize()
        _same_bytes(buf, ref)
        assert not np.array_equal(ref['norms'].cpu().numpy(), proj.evaluate_batch(first)['norms'].cpu().numpy())


def test_reference_compat_fit_agrees_with_the_tensor_select_loop(gpu_models):
    """reference_compat=True: the Jacobian comes undivided by sigma and every loop scales it by the shared
    ``inverse_row_sigma`` -- the fused loop inside the step kernel, the tensor-select loop on the host.  The bound is that
    of tests/test_gpu_fitting.py::test_fused_trust_region_loop_equals_the_tensor_select_loop for its reference_compat
    project: costs within 1e-3, three quarters of the starts equal to rounding (1e-9).  Error bars of 5 % of the data, so that
    1 / sigma is not 1."""
    from sysbio_modeling_amd.experiment import Experiment
    from sysbio_modeling_amd.measurement import TimecourseMeasurement
    from sysbio_modeling_amd.project import Project
    m = gpu_models('simple')
    t = np.linspace(5.0, 100.0, 20)
    grid = np.linspace(0, 100.0, 1000)
    t_sim = np.concatenate([[0.0], grid[np.searchsorted(grid, t)]])
    exps = []
    for name, kd in (('Low', TRUTH[1]), ('High', TRUTH[0])):
        y = m.simulate(np.exp([kd, TRUTH[2]]), t_sim)[1:, 0]
        exps.append(Experiment('%s_Deg_Exp' % name, TimecourseMeasurement('Variable_1', y, t, 0.05 * y),
                               experiment_settings={'Deg_Rate': name}))
    proj = Project(m, exps, {'Global': ['k_synt'], 'Shared': {'Group_1': {'k_deg': ('Deg_Rate',)}}},
                   {'Variable_1': ('direct', 0)}, reference_compat=True)
    starts = _points(8, 3)
    a = proj.fit_batch(starts, max_iter=3)
    b = proj.fit_batch(starts, max_iter=3, algorithm='trust_region_torch')
    c0 = 0.5 * proj.evaluate_batch(starts)['norms']
    print('cost fused', a['cost'], 'tensor-select', b['cost'], 'starts', c0)
    assert np.median(a['cost']) < np.median(c0)
    assert np.allclose(a['cost'], b['cost'], rtol=1e-3) and np.sum(np.abs(a['cost'] / b['cost'] - 1) <= 1e-9) >= 6
