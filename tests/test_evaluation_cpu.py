"""The parts of project/_evaluation.py and of the (p_group, settings) resolver that need no GPU."""
import numpy as np
import pytest
import torch

from sysbio_modeling_amd.project._evaluation import finite_cost, usable
from sysbio_modeling_amd.project.fitting import normalize_held
from sysbio_modeling_amd.project.profiles import param_indices

INF = float('inf')


def test_finite_cost_is_half_the_norm_where_usable_and_inf_elsewhere():
    norms = torch.tensor([3.0, 3.0, float('nan'), INF, 0.0, 1e-300], dtype=torch.float64)
    status = torch.tensor([0, 3, 0, 0, 0, 0], dtype=torch.int32)
    cost = finite_cost(norms, status)
    assert cost.dtype == torch.float64
    # the ordinary case is exact: 0.5 * x is
    assert cost.tolist() == [1.5, INF, INF, INF, 0.0, 0.5e-300]
    assert usable(norms, status).tolist() == [True, False, False, False, True, True]


def test_finite_cost_with_an_entropy():
    norms = torch.tensor([3.0, 3.0, 3.0, 3.0, float('nan')], dtype=torch.float64)
    status = torch.tensor([0, 0, 0, 2, 0], dtype=torch.int32)
    entropy = torch.tensor([0.25, -INF, float('nan'), 0.25, 0.25], dtype=torch.float64)
    assert finite_cost(norms, status, entropy).tolist() == [1.25, INF, INF, INF, INF]
    # +inf entropy would be a free energy of -inf: not finite, so not usable either
    assert finite_cost(norms[:1], status[:1], torch.tensor([INF], dtype=torch.float64)).tolist() == [INF]


class _Names:
    """What the resolver needs of a project: get_param_index."""
    idx = {'k_synt': {'Global': 2}, 'Group_1': {('High',): 0, ('Low',): 1}}

    def get_param_index(self, group, settings='all'):
        return self.idx[group] if isinstance(settings, str) and settings == 'all' else self.idx[group][settings]


def test_pairs_resolve_the_same_through_both_callers():
    names, V, q = _Names(), 2, 3
    # a known pair
    assert param_indices(names, [('Group_1', ('Low',))], q).tolist() == [1]
    assert normalize_held([('Group_1', ('Low',))], V, q, names).tolist() == [[False, True, False]] * V
    # 'all': get_param_index returns the group's dict, every index of it is meant
    assert param_indices(names, [('Group_1', 'all'), ('k_synt', 'Global')], q).tolist() == [0, 1, 2]
    assert normalize_held([('Group_1', 'all')], V, q, names).tolist() == [[True, True, False]] * V


@pytest.mark.parametrize('pair', [('Group_1', ('Medium',)), ('nothing', 'Global'), ('Group_1', ['High'])])
def test_an_unknown_pair_is_refused_with_the_callers_prefix(pair):
    with pytest.raises(ValueError, match=r"^held: the project has no parameter "):
        normalize_held([pair], 2, 3, _Names())
    with pytest.raises(ValueError, match=r"^params: the project has no parameter "):
        param_indices(_Names(), [pair], 3)
