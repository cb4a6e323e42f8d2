"""The scale-factor entropy quadrature rule (csrc/sbm_sf_quadrature.hpp), compiled for the host, against mpmath; and the
C ABI of the device sampler: declared in include/sbm.h, bound in _lib, exported by the library (CPU)."""
import os
import re
import warnings

import numpy as np
import pytest

from sysbio_modeling_amd import _lib
from tests import sf_entropy_cases as sfc

# What the rule can deliver in the logarithm, from its construction (header comment): the integrand is dropped below
# exp(-40) = 4e-18 of its maximum, a 16-point Gauss-Legendre panel integrates a Gaussian over four standard deviations
# to 5e-18, and what remains is the rounding of ~2000 terms of exp(f - max), |f - max| <= 40 + the rounding of f
# itself, ~1e-14 (1e-16 |f| for an integrand as low as exp(-1000)).  1e-10 leaves four digits over that.
RULE_TOL = 1e-10


@pytest.fixture(scope='module')
def rule(tmp_path_factory):
    return sfc.host_rule(tmp_path_factory.mktemp('sfq'))


def _cases():
    rng = np.random.default_rng(7)
    out = []
    for sigma in (0.1, 0.35, 0.9, 3.0):                                   # the sampler's regime: prior within 3 sigma
        for X in 10.0 ** rng.uniform(-2, 8, 4):
            out.append((X, rng.uniform(-3, 3) * sigma, sigma, float(rng.choice([1.0, 2.5]))))
    for sigma, X in ((0.5, 1.0), (1.0, 0.8), (3.0, 1.2), (2.0, 6.0)):      # two maxima: a B*^2 / T ~ 1, prior 3 sigma below
        out.append((X, -3.0 * sigma, sigma, 1.0))
    out += [(1.0e4, -4.0, 0.1, 1.0), (1.0e6, -8.0, 0.2, 2.5),              # integrand below exp(-745) everywhere
            (30.0, 12.0, 2.0, 1.0), (0.02, 9.0, 3.0, 1.0), (5.0e3, -20.0, 2.0, 1.0), (40.0, -0.7, 0.05, 2.5)]
    return out


def test_rule_against_mpmath(rule):
    worst = 0.0
    for X, c, sigma, T in _cases():
        # a B*^2 = X with B* = 1: a = b = X, mu = c
        got = rule.sfq_log_integral(X / (2.0 * T), c, sigma)
        ref = sfc.mp_log_integral(X, X, c, sigma, T)
        err = abs(got - ref)
        worst = max(worst, err)
        assert np.isfinite(got) and err <= RULE_TOL, (X, c, sigma, T, got, ref, err)
        assert 0 < rule.sfq_panels(X / (2.0 * T), c, sigma) <= 128
    print("sf quadrature rule: worst |log I - mpmath| = %.2e over %d cases" % (worst, len(_cases())))


def test_rule_is_finite_where_the_host_quadrature_underflows(rule):
    """An integrand whose maximum is below exp(-745): scipy's quad integrates zeros and the host method returns
    log 0 = -inf; the rule returns the logarithm."""
    from sysbio_modeling_amd.project.loss_functions.squared_loss.linear_scale_factor import scale_factor_entropy
    X, c, sigma = 1.0e4, -4.0, 0.1
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert scale_factor_entropy(X, X, c, sigma, 1.0) == -np.inf
    got = rule.sfq_log_integral(X / 2.0, c, sigma)
    assert got < -745.0 and abs(got - sfc.mp_log_integral(X, X, c, sigma, 1.0)) <= RULE_TOL


def test_rule_refuses_a_scale_factor_that_is_not_positive(rule):
    import ctypes
    out = ctypes.c_double(0.0)
    assert rule.sfq_from_sums(2.0, 3.0, 0.1, 0.5, 1.0, ctypes.byref(out)) == 1 and np.isfinite(out.value)
    for a, b in ((2.0, -3.0), (2.0, 0.0), (0.0, 0.0), (float('nan'), 1.0), (1.0, float('inf'))):
        assert rule.sfq_from_sums(a, b, 0.1, 0.5, 1.0, ctypes.byref(out)) == 0


def test_sampler_symbols_are_declared_bound_and_exported():
    """The pattern of test_host_boundary.test_library_exports_every_declared_symbol for the sampler's three calls."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, 'include', 'sbm.h')) as fh:
        text = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    declared = set(re.findall(r'\b(sbm_[a-z_0-9]+)\s*\(', text))
    lib = _lib.load_library()
    for name, n_args in (('sbm_project_sf_entropy', 6), ('sbm_mh_propose', 8), ('sbm_mh_accept', 14)):
        assert name in declared, "include/sbm.h does not declare %s" % name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name), "libsbm_hip.so does not export %s" % name
    assert lib.sbm_abi_version() == _lib.ABI_VERSION == 4
