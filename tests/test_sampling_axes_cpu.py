"""Host side of the sampler's second algorithm on the device: ``sbm_sampling_axes`` / ``sbm_mh_accept_hastings`` are declared,
bound and exported, the limit is the same number everywhere, and ``ensemble_log_params_batch`` refuses what it has to refuse
before it touches a device."""
import os
import re

import numpy as np
import pytest

from sysbio_modeling_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, 'include', 'sbm.h')) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _declared_arg_count(code, name):
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, code)
    assert m, "%s is not declared in include/sbm.h" % name
    return len([a for a in m.group(1).split(',') if a.strip()])


def test_entries_declared_and_bound():
    text, code = _header()
    for name, n_args in (('sbm_sampling_axes', 16), ('sbm_mh_accept_hastings', 21)):
        assert _declared_arg_count(code, name) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    # the Hastings entry takes the arguments of sbm_mh_accept and seven more
    assert _declared_arg_count(code, 'sbm_mh_accept') + 7 == 21
    assert _lib.SIGNATURES['sbm_mh_accept_hastings'][1][:14] == _lib.SIGNATURES['sbm_mh_accept'][1]
    assert re.search(r'#define\s+SBM_SAMPLING_AXES_MAX_Q\s+96\b', text) and _lib.SAMPLING_AXES_MAX_Q == 96
    assert re.search(r'#define\s+SBM_ABI_VERSION\s+4\b', text) and _lib.ABI_VERSION == 4
    # the sign convention is part of the interface
    doc = text[text.index('Axes of the Gaussian candidate density'):text.index('int sbm_sampling_axes')]
    assert 'largest magnitude is positive' in doc and 'lowest index' in doc


def test_library_exports_the_entries():
    lib = _lib.load_library()
    assert hasattr(lib, 'sbm_sampling_axes') and hasattr(lib, 'sbm_mh_accept_hastings')


def test_header_is_a_build_source():
    from sysbio_modeling_amd import build
    assert any(s.endswith('sbm_sampling_axes.hpp') for s in build._core_sources())


def test_exports():
    import sysbio_modeling_amd.project as p
    for name in ('pca_eig', 'pca_eig_log_params'):
        assert hasattr(p, name) and name in p.__all__


def test_sampler_argument_checks_need_no_device():
    """These are decided from the arguments alone (the project is not looked at): 'device' stays the first algorithm and
    names the new value, the new value names its limit, draws= is for the device samplers."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    with pytest.raises(ValueError, match='device_recalc'):
        ensemble_log_params_batch(None, np.zeros(2), steps=2, sampler='device', recalc_hess_alg=True)
    with pytest.raises(ValueError, match='96'):
        ensemble_log_params_batch(None, np.zeros((3, 97)), steps=2, sampler='device_recalc')
    with pytest.raises(ValueError, match='draws'):
        ensemble_log_params_batch(None, np.zeros(2), steps=2, sampler='host', draws=(np.zeros((2, 1, 2)), np.zeros((2, 1))))
    with pytest.raises(ValueError, match='sampler'):
        ensemble_log_params_batch(None, np.zeros(2), steps=2, sampler='gpu_recalc')
