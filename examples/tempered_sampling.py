"""Parallel tempering of the 8-experiment cascade project (BASELINE configs[3]) on one GPU.

    python examples/tempered_sampling.py [t_max]

64 chains of the device sampler, free energy with a log prior on every scale factor, started at the nominal parameters:
once all at T = 1, once as 8 ladders of 8 temperatures 1 ... t_max (default 8) that exchange replicas every 5 steps, and once
as the same ladders without exchanges (what the hot replicas' longer trajectories alone cost).  Then what the ladder buys:
integrated autocorrelation time and effective sample size of the T = 1 chains, with the ladder and without it in the same
wall-clock time."""
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sysbio_modeling_amd import models_zoo
from sysbio_modeling_amd.model import OdeModel
from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch, temperature_ladder
from sysbio_modeling_amd.symbolic import zoo_model


def timed(run, repeats=3):
    best, out = np.inf, None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = run()
        best = min(best, time.perf_counter() - t0)
    return best, out


def report(label, diag):
    print("    %s: tau median %.1f (max %.1f) kept steps, ess summed over the chains: min %.0f, median %.0f; max r_hat %.2f, "
          "%d of %d windows truncated" % (label, np.nanmedian(diag['tau']), np.nanmax(diag['tau']), np.nanmin(diag['ess']),
                                          np.nanmedian(diag['ess']), np.nanmax(diag['r_hat']), int(diag['truncated'].sum()),
                                          diag['tau'].size))


def main():
    t_max = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
    warnings.simplefilter('ignore')
    gm = zoo_model('cascade20')
    model = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order)
    proj, th0 = models_zoo.cascade_config4_project(model, reference_compat=False)
    for v in models_zoo.CASCADE_MEASURED_SPECIES:
        proj.set_scale_factor_log_prior('s%d' % v, 0.0, 1.0)
    K, steps = 8, 200
    start = np.tile(th0, (64, 1))
    chains = dict(seeds=1, sing_val_cutoff=1e-4, step_scale=0.3, energy='free_energy', sampler='device')
    ladder = temperature_ladder(K, t_max)
    ensemble_log_params_batch(proj, start, steps=2, **chains)                                   # warm-up: no timing pays it
    ensemble_log_params_batch(proj, start, steps=10, temperature=ladder, swap_every=5, **chains)
    t_one, (_, _, ratio) = timed(lambda: ensemble_log_params_batch(proj, start, steps=steps, **chains))
    print("T = 1: 64 chains x %d steps in %.4f s, acceptance %.2f" % (steps, t_one, ratio.mean()))
    t_flat, _ = timed(lambda: ensemble_log_params_batch(proj, start, steps=steps, temperature=ladder, **chains))
    t_pt, out = timed(lambda: ensemble_log_params_batch(proj, start, steps=steps, temperature=ladder, swap_every=5, diagnostics=True,
                                                        **chains))
    ens, ens_F, ratio, diag, info = out
    pairs = info['rung'] < K - 1
    swap = (info['swap_accepted'][pairs] / info['swap_attempted'][pairs]).reshape(-1, K - 1).mean(axis=0)
    print("ladder 1 ... %g, %d ladders x %d rungs, swaps every 5 steps: %.4f s = %.2f x (estimate from the launches: 1.2); without "
          "swaps %.4f s = %.2f x" % (t_max, 64 // K, K, t_pt, t_pt / t_one, t_flat, t_flat / t_one))
    print("    acceptance per rung %s" % np.round(ratio.reshape(-1, K).mean(axis=0), 2))
    print("    swap ratio per pair of rungs %s" % np.round(swap, 2))
    report("rung 0 with the ladder (%d chains x %d steps)" % (64 // K, steps), diag)
    # the same wall-clock time spent on 64 chains at T = 1
    n_equal = int(round(steps * t_pt / t_one))
    out = ensemble_log_params_batch(proj, start, steps=n_equal, diagnostics=True, **chains)
    report("T = 1 alone in the same time (64 chains x %d steps)" % n_equal, out[3])


if __name__ == '__main__':
    main()
