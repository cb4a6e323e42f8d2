"""Profile likelihoods of the 8-experiment cascade project (BASELINE configs[3], 68 parameters) on one GPU.

    python examples/profile_likelihood.py [n_params] [--loose] [--host]

Fits the project from scattered starts, takes the best fit as theta_hat and profiles the first n_params parameters
(default: all 68) over +-1 log unit in ten steps: each profile point is a fit with that parameter held and all the
others free, and the 2 x n_params branches of a grid step are the starts of ONE fit_batch(held=...) call
(Project.profile_likelihood_batch).  Prints the 95 % likelihood-based confidence interval of every profiled parameter
(+-inf: the profile never reaches the chi^2 quantile on this grid -- the data do not determine the parameter), next
to the sampler's view of the same question in examples/fit_cascade.py.  The project is sloppy: within 60 iterations
few of the fits meet lmder's default tolerances (1.5e-8, relative), and only converged points count for an interval --
``--loose`` fits the profile points with ftol = xtol = 1e-6, ample against a chi^2 quantile of 3.84.  ``--host``: also times the same points of ONE
parameter done the serial way, scipy.optimize.leastsq on the host functions with the held column dropped."""
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sysbio_modeling_amd import models_zoo
from sysbio_modeling_amd.model import OdeModel
from sysbio_modeling_amd.project import profile_confidence_intervals
from sysbio_modeling_amd.symbolic import zoo_model


def host_profile(proj, theta_hat, i, offsets):
    """The serial counterpart: leastsq per point on the reduced functions, each branch continued from its last optimum."""
    from scipy.optimize import leastsq
    free = [c for c in range(theta_hat.size) if c != i]
    n_fev = 0
    for sign in (-1.0, 1.0):
        x = theta_hat.copy()
        for off in offsets:
            x[i] = theta_hat[i] + sign * off

            def full(z, x=x):
                y = x.copy()
                y[free] = z
                return y
            z, _, info, _, _ = leastsq(lambda z: proj.residuals(full(z)), x[free],
                                       Dfun=lambda z: proj.calc_project_jacobian(full(z))[:, free], full_output=True)
            n_fev += info['nfev']
            x = full(z)
    return n_fev


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    warnings.simplefilter('ignore')
    gm = zoo_model('cascade20')
    model = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order)
    proj, theta_true = models_zoo.cascade_config4_project(model, noise=0.05, reference_compat=False)
    q = proj.n_project_params
    n_params = int(args[0]) if args else q
    rng = np.random.default_rng(0)
    starts = theta_true[None, :] + 0.1 * rng.standard_normal((64, q))
    fit = proj.fit_batch(starts, max_iter=150)
    theta_hat = fit['theta'][int(np.argmin(fit['cost']))]
    # polish: the profile measures against the cost at theta_hat as given
    theta_hat = proj.fit_batch(theta_hat[None, :], max_iter=200)['theta'][0]
    offsets = np.linspace(0.1, 1.0, 10)
    proj.profile_likelihood_batch(theta_hat, params=range(2), offsets=offsets[:1], max_iter=2)      # warm-up
    t0 = time.time()
    tol = dict(ftol=1e-6, xtol=1e-6) if '--loose' in sys.argv else {}
    prof = proj.profile_likelihood_batch(theta_hat, params=range(n_params), offsets=offsets, max_iter=60, **tol)
    dt = time.time() - t0
    conv = prof['converged']
    print("profiles: %d parameters x %d points in %.2f s, %d starts x trial points integrated (%d of %d points converged), "
          "cost_hat %.3f" % (n_params, 2 * offsets.size, dt, prof['n_evaluations'], conv.sum() - n_params, conv.size - n_params,
                             prof['cost_hat']))
    ci = profile_confidence_intervals(prof, level=0.95)
    names = [n for n, _ in proj.get_ordered_project_params()]
    for j, i in enumerate(prof['param_index']):
        d = prof['delta_chi2'][j]
        print("    %-24s theta_hat %7.3f   95 %% interval [%7.3f, %7.3f]   delta_chi2 %.2g .. %.2g (converged points: up to %.2g)"
              % (names[i], theta_hat[i], ci[j, 0], ci[j, 1], np.nanmin(d), np.nanmax(d), np.nanmax(np.where(conv[j], d, np.nan))))
    print("    identifiable on this grid (both ends finite): %d of %d" % (int(np.isfinite(ci).all(axis=1).sum()), n_params))
    if '--host' in sys.argv:
        t0 = time.time()
        n_fev = host_profile(proj, theta_hat, 0, offsets)
        dt_h = time.time() - t0
        print("host: the %d points of ONE parameter, serial leastsq on the reduced functions: %.2f s (%d function evaluations); "
              "scaled by %d parameters: %.0f s" % (2 * offsets.size, dt_h, n_fev, n_params, dt_h * n_params))


if __name__ == '__main__':
    main()
