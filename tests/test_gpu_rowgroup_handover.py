"""The per-stage operand hand-over of the row-group kernels (RowGroupSystem::eval_stage, SBM_RG_EARLY_STAGES) moves LDS
loads and changes no arithmetic: a plugin built with -DSBM_RG_EARLY_STAGES=0 (every stage fetches its operands in finish,
the schedule before the switch existed) and the default build return the same BITS for Y, S, status, n_steps and n_reject,
NaN rows included.  The cases (tests/support/rowgroup_handover_cases.py) are the smallest that reach every path the
switch touches.  The mask-0 plugins are compiled by build(); they run in one child process, the default build here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import rowgroup_handover_cases as cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK0 = '-DSBM_RG_EARLY_STAGES=0'
SBM_MAX_STEPS = 1


@pytest.fixture(scope='module')
def mask0(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('handover') / 'mask0.npz')
    env = dict(os.environ, SBM_PLUGIN_FLAGS=MASK0)
    subprocess.run([sys.executable, cases.__file__, out], check=True, env=env, cwd=REPO, timeout=600)
    return np.load(out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize('case', list(cases.CASES))
def test_default_build_equals_mask_0_bit_for_bit(mask0, case):
    assert MASK0 not in os.environ.get('SBM_PLUGIN_FLAGS', '')
    got = cases.run(case)
    print(case, 'status', got['status'], 'n_steps', got['n_steps'], 'n_reject', got['n_reject'])
    for key, a in got.items():
        ref = mask0['%s.%s' % (case, key)]
        assert a.shape == ref.shape and a.dtype == ref.dtype, key
        assert np.array_equal(_bits(a), _bits(ref)), '%s: %s differs in %d entries' % (
            case, key, int((_bits(a) != _bits(ref)).sum()))
    # what each case is there for
    if case == 'cascade20_rg0':
        assert not got['status'].any() and len(set(got['n_steps'].tolist())) == 3
        assert np.all(np.isfinite(got['S']))
    elif case == 'cascade20_rg0_rejected_first_step':
        assert not got['status'].any() and np.all(got['n_reject'] > 0)
    elif case == 'cascade20_rg0_step_budget':
        assert np.all(got['status'] == SBM_MAX_STEPS) and np.all(np.isnan(got['S'][:, -1]))
    else:
        assert not got['status'].any() and np.all(np.isfinite(got['S']))
