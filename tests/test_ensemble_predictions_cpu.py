"""Host side of the ensemble predictions: the theta -> model-parameter gather against ``Project.get_experiment_parameters``,
argument checks, and the new entry point in header and binding."""
import os
import re

import numpy as np
import pytest

from sysbio_modeling_amd import _lib
from sysbio_modeling_amd.model import OdeModel
from sysbio_modeling_amd.project import ensembles
from tests import ensemble_cases as ec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def project(zoo):
    gm = zoo('cascade20')
    model = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, use_jit=False)
    return ec.prediction_project(model)


def test_gather_matches_get_experiment_parameters(project):
    """experiment_parameters_batch is the vectorised restatement of the reference's gather: bit for bit the host loop, fixed
    (per-experiment values) and shared (one slot, two experiments) parameters included."""
    proj, theta = project
    ens = ec.ensemble_around(theta, V=9)
    exps = list(proj.experiments)
    assert len(exps) == 3
    saved = proj.project_param_vector
    try:
        for e, exp in enumerate(exps):
            P = ensembles.experiment_parameters_batch(proj, ens, e)
            for v in range(ens.shape[0]):
                proj._project_param_vector = ens[v].copy()
                assert np.array_equal(P[v], proj.get_experiment_parameters(exp)), (e, v)
            assert np.all(P[:, 21] == ec.FIXED_D1[e])
    finally:
        proj._project_param_vector = saved
    P0, P1, P2 = (ensembles.experiment_parameters_batch(proj, ens, e) for e in range(3))
    assert np.array_equal(P0[:, 20], P2[:, 20]) and not np.array_equal(P0[:, 20], P1[:, 20])      # the shared slot
    # the sampler's (n_kept, C, q) is the flattened ensemble
    P3 = ensembles.experiment_parameters_batch(proj, ens.reshape(3, 3, -1), 1)
    assert np.array_equal(P3, P1)


def test_argument_checks(project):
    proj, theta = project
    ens = ec.ensemble_around(theta, V=4)
    t = np.linspace(0, 50, 5)
    with pytest.raises(ValueError, match='ensemble must have shape'):
        ensembles.ensemble_trajs(proj, t, ens[:, :-1])
    with pytest.raises(ValueError, match='ensemble must have shape'):
        ensembles.ensemble_predictions(proj, t, np.zeros((2, 2, 2, theta.size)))
    with pytest.raises(ValueError, match='non-decreasing'):
        ensembles.ensemble_trajs(proj, t[::-1], ens)
    with pytest.raises(ValueError, match='non-decreasing'):
        ensembles.ensemble_predictions(proj, [0.0, 2.0, 1.0], ens)
    with pytest.raises(ValueError, match='negative'):
        ensembles.ensemble_trajs(proj, [-1.0, 2.0], ens)
    with pytest.raises(ValueError, match='non-empty'):
        ensembles.ensemble_trajs(proj, [], ens)
    for bad in ((0.5, 1.01), (-1e-9,), (float('nan'),)):
        with pytest.raises(ValueError, match=r'\[0, 1\]'):
            ensembles.ensemble_predictions(proj, t, ens, quantiles=bad)
    with pytest.raises(ValueError, match='16385 ensemble members'):
        ensembles.ensemble_predictions(proj, t, np.zeros((16385, theta.size)))
    with pytest.raises(KeyError):
        ensembles.ensemble_trajs(proj, t, ens, experiments=['nope'])


def test_entry_point_declared_and_bound():
    with open(os.path.join(REPO, 'include', 'sbm.h')) as fh:
        text = fh.read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+sbm_ensemble_stats\s*\(', code)
    assert re.search(r'#define\s+SBM_ENSEMBLE_MAX_MEMBERS\s+16384\b', text)
    assert re.search(r'#define\s+SBM_ABI_VERSION\s+4\b', text)
    res, args = _lib.SIGNATURES['sbm_ensemble_stats']
    assert len(args) == 12 and _lib.ENSEMBLE_MAX_MEMBERS == 16384
    lib = _lib.load_library()
    assert hasattr(lib, 'sbm_ensemble_stats')


def test_exports():
    import sysbio_modeling_amd.project as p
    for name in ('ensemble_trajs', 'traj_ensemble_stats', 'traj_ensemble_quantiles', 'net_ensemble_trajs',
                 'ensemble_predictions', 'EnsembleTrajectories'):
        assert hasattr(p, name) and name in p.__all__
