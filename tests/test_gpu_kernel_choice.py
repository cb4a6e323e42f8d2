"""The launcher runs the kernel sbm_choose_kernel names.  Under SBM_DEBUG_LAUNCH every launch of a model plugin prints
``launch choice: <kernel> method <m> nch <chunks> SEG <lanes>, <n> trajectories`` (csrc/sbm_launch.hpp, directly after the
decision); the line of each call below must be the one the host harness of tests/test_kernel_choice_cpu.py computes from
the hand-written traits of the model, and every trajectory must report status 0: the kernel the decision names exists in
the plugin and integrates.

michaelis_menten and cascade20 on a 3-point grid: sensitivity calls with five vectors, every variant x {rk4, dopri45,
dop853}; state calls with 5 and 2049 vectors (both sides of the packed state kernel's threshold)."""
import os
import re
import subprocess
import sys

import pytest

from tests.test_kernel_choice_cpu import EXPLICIT, SENS, STATE, VARIANTS, build_harness, launch_line

pytestmark = pytest.mark.gpu

MODELS = ('michaelis_menten', 'cascade20')
CALLS = [(model, SENS, method, variant, 5) for model in MODELS for variant in VARIANTS for method in EXPLICIT] + \
    [(model, STATE, method, 'auto', n) for model in MODELS for n in (5, 2049) for method in EXPLICIT]

_CHILD = r'''
import sys
import warnings
import numpy as np
sys.path.insert(0, sys.argv[1])
from sysbio_modeling_amd.model import OdeModel
from sysbio_modeling_amd.symbolic import zoo_model
from tests.support.erk_cases import ensemble
from tests.test_gpu_kernel_choice import CALLS, SENS
models = {}
for i, (name, kind, method, variant, n) in enumerate(CALLS):
    if name not in models:
        gm = zoo_model(name)
        models[name] = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=name)
    m = models[name]
    P = ensemble(name, n)
    t_out = np.array([0.0, 1.0, 2.0])
    kw = dict(method=method, variant=variant)
    if method == 'rk4':
        kw['h0'] = 1.0 / 16.0
    sys.stderr.write('CALL %d\n' % i)
    sys.stderr.flush()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if kind == SENS:
            m.calc_jacobian_batch(P, t_out, **kw)
        else:
            m.simulate_batch(P, t_out, **kw)
    st = m.last_info['status']
    assert st.shape == (n,) and not st.any(), (name, kind, method, variant, n, st)
sys.stderr.write('CALL end\n')
'''


def test_every_call_runs_the_kernel_the_host_decision_names(tmp_path):
    lib = build_harness(tmp_path)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the child's program is the string above (python -c): nothing is written or read outside the repository tree
    p = subprocess.run([sys.executable, '-c', _CHILD, repo], cwd=repo, env=dict(os.environ, SBM_DEBUG_LAUNCH='1'),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    blocks = re.split(r'^CALL ', p.stderr, flags=re.M)[1:]
    assert [b.split('\n')[0] for b in blocks] == [str(i) for i in range(len(CALLS))] + ['end']
    for call, block in zip(CALLS, blocks):
        lines = [ln for ln in block.split('\n')[1:] if ln.startswith('launch choice:')]
        assert lines == [launch_line(lib, *call)], (call, lines)
