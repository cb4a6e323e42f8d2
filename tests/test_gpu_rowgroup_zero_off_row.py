"""Lanes of the row-group kernels that evaluate no row get all-zero operands instead of a select behind every row evaluation
where the model's class bodies vanish on them (RL_F_ZERO_OFF_ROW, csrc/sbm_kernels_rowgroup.hpp RowGroupSystem::kZeroOffRow).
That changes no floating-point operation of any lane with a row: the default build returns the same BITS for Y, S,
n_steps, n_reject and status as the plugin built with -DSBM_RG_KEEP_F_SELECT=1 (the select: the code before), NaN rows
included.  The cases are in tests/support/zero_off_row_cases.py.  The twin plugins are compiled by build(); they run in
one child process, the default build here (two builds of one model's plugin are not loaded into one process:
tests/test_gpu_rowgroup_handover.py).

The launcher starts layout RG2 under DOP853 only, so the second layout under DOPRI45 is RG1 (variant small_batch); RG2
runs under its own method."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import zero_off_row_cases as cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SBM_MAX_STEPS = 1


@pytest.fixture(scope='module')
def twin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('zero_off_row') / 'twin.npz')
    env = dict(os.environ, SBM_PLUGIN_FLAGS=cases.TWIN_FLAGS)
    subprocess.run([sys.executable, cases.__file__, out], check=True, env=env, cwd=REPO, timeout=600)
    return np.load(out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize('case', list(cases.CASES))
def test_default_build_equals_the_select_twin_bit_for_bit(twin, case):
    assert 'SBM_PLUGIN_FLAGS' not in os.environ
    got = cases.run(case)
    ref = {key: twin['%s.%s' % (case, key)] for key in got}
    print(case, 'status', got['status'], 'n_steps', got['n_steps'], 'n_reject', got['n_reject'], '; twin n_steps',
          ref['n_steps'], 'n_reject', ref['n_reject'])
    for key, a in got.items():
        assert a.shape == ref[key].shape and a.dtype == ref[key].dtype, key
        assert np.array_equal(_bits(a), _bits(ref[key])), '%s: %s differs in %d entries' % (
            case, key, int((_bits(a) != _bits(ref[key])).sum()))
    # what each case is there for, asserted on the TWIN's counts where it is about the path taken
    if case == 'n_t_1':
        assert not got['status'].any() and not ref['n_steps'].any()
    elif case == 'rtol_1e-3':
        assert not got['status'].any()
        assert (ref['n_steps'] % 2 == 0).any() and (ref['n_steps'] % 2 == 1).any(), ref['n_steps']
    elif case == 'rejected_attempts':
        assert not got['status'].any() and np.all(ref['n_reject'] > 0)
    elif case in ('max_steps_5', 'max_steps_6'):
        assert np.all(got['status'] == SBM_MAX_STEPS)
        assert np.all(np.isnan(got['S'][:, -1])) and np.all(np.isnan(got['Y'][:, -1]))
        assert np.all(np.isfinite(got['S'][:, 0])) and np.all(np.isfinite(got['Y'][:, 0]))
    else:
        assert not got['status'].any() and np.all(np.isfinite(got['S'])) and np.all(np.isfinite(got['Y']))
