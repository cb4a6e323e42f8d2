"""tests/golden/cascade_config4_n2_theta_hat.npy: the point where lmder meets its default tolerances on the two-experiment
config-4 cascade project, from the nominal parameters (tests/test_gpu_profiles.py profiles around it).  Needs a GPU;
about ten seconds, ~1300 iterations.

    python tests/golden/make_golden_cascade_theta_hat.py

Also prints how far the valley floor still is: 6000 iterations more at ftol = xtol = 1e-13 lower the cost in the fifth
digit (that point is not stored)."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from sysbio_modeling_amd import models_zoo
from sysbio_modeling_amd.model import OdeModel
from sysbio_modeling_amd.symbolic import zoo_model


def main():
    warnings.simplefilter('ignore')
    gm = zoo_model('cascade20')
    m = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name='cascade20')
    proj, th0 = models_zoo.cascade_config4_project(m, n_exp=2, reference_compat=False)
    fit = proj.fit_batch(th0[None, :], max_iter=2000)
    print('default tolerances: converged %s after %d iterations, cost %.10g' % (fit['converged'][0], fit['n_iter'][0], fit['cost'][0]))
    assert fit['converged'][0]
    np.save(os.path.join(HERE, 'cascade_config4_n2_theta_hat.npy'), fit['theta'][0])
    tight = proj.fit_batch(fit['theta'], max_iter=6000, ftol=1e-13, xtol=1e-13)
    print('6000 iterations more at 1e-13: cost %.10g' % tight['cost'][0])


if __name__ == '__main__':
    main()
