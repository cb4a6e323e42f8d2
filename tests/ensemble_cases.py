"""The small project the ensemble-prediction tests share: cascade20 with three experiments that differ in a FIXED
parameter (d1), share d0 through a 'Shared' group keyed on the experiments' ``cond`` setting -- experiments 0 and 2 carry
the same ``cond``, so one project slot feeds two experiments -- and keep everything else Global.  Measures: s4 ('direct')
and tot ('sum' of two species) in one scale-factor group, s19 ('direct') without a scale factor; experiment 1 lacks s19
and measures at other times."""
import numpy as np

from sysbio_modeling_amd import models_zoo
from sysbio_modeling_amd.experiment import Experiment
from sysbio_modeling_amd.measurement import TimecourseMeasurement
from sysbio_modeling_amd.project import Project

FIXED_D1 = (0.08, 0.105, 0.14)
COND = ('a', 'b', 'a')
MEASURE_TIMES = (np.linspace(10.0, 100.0, 7), np.linspace(5.0, 60.0, 5), np.linspace(10.0, 100.0, 7))
MAPPING = {'s4': ('direct', 4), 's19': ('direct', 19), 'tot': ('sum', [9, 14])}


def nominal_params(e):
    p = models_zoo.cascade_nominal_params()
    p[20] *= 1.0 + 0.3 * (COND[e] == 'b')
    p[21] = FIXED_D1[e]
    return p


def prediction_project(model, simulate=None, extra_mapping=None):
    """(project, theta at the parameters the data were generated with).  ``simulate(p, t) -> (len(t), 20)`` gives the data
    (scaled by 2.5 where the measure has a scale factor); without it the data are ones (index arrays only)."""
    names = list(model.param_order)
    mapping = dict(MAPPING)
    mapping.update(extra_mapping or {})
    exps = []
    for e in range(3):
        t = MEASURE_TIMES[e]
        grid = np.linspace(0, t[-1], 1000)
        y = simulate(nominal_params(e), np.concatenate([[0.0], grid[np.searchsorted(grid, t)]]))[1:] if simulate else np.ones((len(t), 20))
        ms = [TimecourseMeasurement('s4', 2.5 * y[:, 4], t.copy(), 0.05 * np.abs(y[:, 4]) + 0.01),
              TimecourseMeasurement('tot', 2.5 * (y[:, 9] + y[:, 14]), t.copy(), 0.05 * np.abs(y[:, 9] + y[:, 14]) + 0.01)]
        if e != 1:
            ms.append(TimecourseMeasurement('s19', y[:, 19], t.copy(), 0.05 * np.abs(y[:, 19]) + 0.01))
        for nm in (extra_mapping or {}):
            ms.append(TimecourseMeasurement(nm, np.ones(len(t)), t.copy(), np.ones(len(t))))
        exps.append(Experiment('exp_%d' % e, ms, fixed_parameters={'d1': FIXED_D1[e]}, experiment_settings={'cond': COND[e]}))
    settings = {'Fixed': ['d1'], 'Shared': {'deg': {'d0': ('cond',)}}, 'Global': [n for n in names if n not in ('d0', 'd1')]}
    proj = Project(model, exps, settings, mapping, sf_groups=[frozenset(['s4', 'tot'])], reference_compat=False)
    theta = np.zeros(proj.n_project_params)
    for g, slots in proj.project_param_idx.items():
        for key, gi in slots.items():
            if g == 'deg':
                theta[gi] = np.log(models_zoo.cascade_nominal_params()[20] * (1.0 + 0.3 * (key[0] == 'b')))
            else:
                theta[gi] = np.log(models_zoo.cascade_nominal_params()[names.index(g)])
    return proj, theta


def ensemble_around(theta, V=48, seed=3, spread=0.05):
    return theta[None, :] + spread * np.random.default_rng(seed).standard_normal((V, theta.size))
