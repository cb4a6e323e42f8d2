"""The calls of tests/test_gpu_rowgroup_handover.py: the smallest shapes that reach every path of the row-group kernels'
stage hand-over (RowGroupSystem::eval_stage / finish).  ``run(name)`` returns what one call hands back; run as a program,

    SBM_PLUGIN_FLAGS=-DSBM_RG_EARLY_STAGES=0 python -m tests.support.rowgroup_handover_cases OUT.npz

it runs every case on the plugins compiled with those flags and writes the arrays to OUT.npz (the test starts it as a
child process: two builds of one model's plugin are not loaded into one process)."""
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SPAN = np.array([0.0, 1.5, 4.0])           # t_out[0] = t0: the first row is the initial condition


def _cascade20():
    from sysbio_modeling_amd import models_zoo
    _, P = models_zoo.cascade_ensemble(3)
    P[1] *= 3.0                            # faster rates: more steps than its neighbours
    P[2] *= 0.3
    return 'cascade20', P


def _stiff50():
    from sysbio_modeling_amd import models_zoo
    return 'stiff50', models_zoo.stiff_ensemble(2)[1]


def _cascade70():
    from sysbio_modeling_amd import models_zoo
    rng = np.random.default_rng(2026)
    return 'cascade70', models_zoo.cascade_nominal_params(70)[None, :] * np.exp(0.3 * rng.standard_normal((2, 140)))


# name -> (model and vectors, output times, integrator overrides)
CASES = {
    # one chunk, the halo term, the padded row of group 2, idle lanes 60-63
    'cascade20_rg0': (_cascade20, SPAN, dict(variant='row_group', method='dopri45')),
    # the first attempt spans everything: rejected, the reject path re-evaluates through the unnumbered rhs
    'cascade20_rg0_rejected_first_step': (_cascade20, SPAN, dict(variant='row_group', method='dopri45', h0=4.0)),
    # SBM_MAX_STEPS and NaN rows
    'cascade20_rg0_step_budget': (_cascade20, SPAN, dict(variant='row_group', method='dopri45', max_steps=5)),
    # RG1: five chunks of eight columns
    'cascade20_small_batch_one_vector': (lambda: (_cascade20()[0], _cascade20()[1][:1]), SPAN,
                                         dict(variant='small_batch', method='dopri45')),
    # five chunks; the system is stiff (rates up to 1e6), so a short span from its quasi-steady start (about ten steps)
    # and a budget in case a change makes it hit the stability limit
    'stiff50_dopri45': (_stiff50, np.array([0.0, 0.002, 0.005]), dict(variant='row_group', method='dopri45', max_steps=20000)),
    # two state rows per lane, 14 chunks
    'cascade70': (_cascade70, SPAN, dict(method='dopri45')),
}


def _model(name):
    from sysbio_modeling_amd import models_zoo
    from sysbio_modeling_amd.model import OdeModel
    from sysbio_modeling_amd.symbolic import GeneratedModel, zoo_model
    gm = GeneratedModel(models_zoo.cascade_spec(70, name='cascade70')) if name == 'cascade70' else zoo_model(name)
    return OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=name)


_MODELS = {}


def run(case):
    make, t_out, overrides = CASES[case]
    name, P = make()
    if name not in _MODELS:
        _MODELS[name] = _model(name)
    m = _MODELS[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # (the step-budget case reports failed vectors)
        S, Y = m.calc_jacobian_batch(P, t_out, return_states=True, **overrides)
    info = m.last_info
    return dict(Y=Y, S=S, status=np.asarray(info['status']), n_steps=np.asarray(info['n_steps']),
                n_reject=np.asarray(info['n_rejected']))


if __name__ == '__main__':
    out = {}
    for case in CASES:
        for key, a in run(case).items():
            out['%s.%s' % (case, key)] = a
    np.savez(sys.argv[1], **out)
