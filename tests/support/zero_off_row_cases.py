"""The calls of tests/test_gpu_rowgroup_zero_off_row.py: the smallest shapes that reach every path of the row-group
kernels on which lanes without a row matter (RL_F_ZERO_OFF_ROW: all-zero operands instead of a select).  ``run(name)`` returns what
one call hands back; run as a program,

    SBM_PLUGIN_FLAGS=-DSBM_RG_KEEP_F_SELECT=1 python -m tests.support.zero_off_row_cases OUT.npz

it runs every case on the plugins compiled with those flags and writes the arrays to OUT.npz (as in
tests/support/rowgroup_handover_cases.py: two builds of one model's plugin are not loaded into one process)."""
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

TWIN_FLAGS = '-DSBM_RG_KEEP_F_SELECT=1'


def _cascade20():
    """the nominal vector and three of the ensemble"""
    from sysbio_modeling_amd import models_zoo
    _, P = models_zoo.cascade_ensemble(3)
    return 'cascade20', np.vstack([models_zoo.cascade_nominal_params()[None, :], P])


def _michaelis_menten():
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'mm_ref.npz'))
    return 'michaelis_menten', np.vstack([g['P'], g['P']])


RG0 = dict(variant='row_group', method='dopri45')
SPAN = np.array([0.0, 1.5, 4.0])           # t_out[0] = t0: the first row is the initial condition

# name -> (model and vectors, output times, integrator overrides)
CASES = {
    # number of output times: the initial condition alone (no attempt at all), one landing, seventeen
    'n_t_1': (_cascade20, np.array([0.0]), RG0),
    'n_t_2': (_cascade20, np.array([0.0, 4.0]), RG0),
    'n_t_17': (_cascade20, np.linspace(0.0, 8.0, 17), RG0),
    # few steps, odd and even counts of them
    'rtol_1e-3': (_cascade20, SPAN, dict(RG0, rtol=1e-3)),
    # the first attempt spans everything: rejected attempts, the reject path's evaluation
    'rejected_attempts': (_cascade20, SPAN, dict(RG0, h0=4.0)),
    # SBM_MAX_STEPS on an odd and on an even attempt: NaN rows from the failing output on
    'max_steps_5': (_cascade20, SPAN, dict(RG0, max_steps=5)),
    'max_steps_6': (_cascade20, SPAN, dict(RG0, max_steps=6)),
    # the other row-group layouts: RG1 (five chunks of eight columns) under DOPRI45 -- the launcher starts RG2 under
    # DOP853 only, where the zero operands are what changed
    'rg1_dopri45': (lambda: (_cascade20()[0], _cascade20()[1][:1]), SPAN, dict(variant='small_batch', method='dopri45')),
    'rg2_dop853': (_cascade20, SPAN, dict(variant='row_group', method='dop853')),
    # a model whose class bodies do not vanish on zero operands (RL_F_ZERO_OFF_ROW false): the select stays
    'michaelis_menten': (_michaelis_menten, np.array([0.0, 0.5, 2.0]), RG0),
}


def _model(name):
    from sysbio_modeling_amd.model import OdeModel
    from sysbio_modeling_amd.symbolic import zoo_model
    gm = zoo_model(name)
    return OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=name)


_MODELS = {}


def run(case):
    make, t_out, overrides = CASES[case]
    name, P = make()
    if name not in _MODELS:
        _MODELS[name] = _model(name)
    m = _MODELS[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # (the step-budget cases report failed vectors)
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
