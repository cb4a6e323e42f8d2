"""The parts of the held-parameter fits and profile likelihoods that need no GPU: profile_confidence_intervals on synthetic
profiles, the normaliser of fit_batch's ``held`` argument, and the declaration / binding of sbm_lm_trust_step_held."""
import os
import re

import numpy as np
import pytest
from scipy.stats import chi2

from sysbio_modeling_amd.project.fitting import normalize_held
from sysbio_modeling_amd.project.profiles import param_indices, profile_confidence_intervals

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_profile(value, delta_chi2, converged=None):
    value, d = np.atleast_2d(np.asarray(value, dtype=float)), np.atleast_2d(np.asarray(delta_chi2, dtype=float))
    conv = np.ones(d.shape, dtype=bool) if converged is None else np.atleast_2d(converged)
    return {'param_index': np.arange(value.shape[0]), 'value': value, 'delta_chi2': d, 'converged': conv, 'cost_hat': 1.0,
            'cost': 1.0 + 0.5 * d}


def test_interval_of_an_exact_parabola():
    """delta_chi2 = (v - v_hat)^2 / sigma^2 on a uniform grid of spacing h.  Linear interpolation of f = u^2 (u in units of
    sigma) between two grid points is off by at most (h / sigma)^2 / 4 in f (the chord of a parabola at mid-interval), and
    a value error of that size in f moves the crossing by (h / sigma)^2 / 4 / f'(u*) = (h / sigma)^2 / (8 u*) in u, with
    u* = sqrt(chi2.ppf(0.95, 1)) = 1.96: below 1e-3 sigma needs (h / sigma)^2 <= 8 * 1.96 * 1e-3, h <= 0.125 sigma.
    h = 0.1 sigma is used: error <= 6.4e-4 sigma."""
    v_hat, sigma, K = 0.7, 0.25, 30
    h = 0.1 * sigma
    assert h <= np.sqrt(8 * 1.96 * 1e-3) * sigma
    value = v_hat + h * np.arange(-K, K + 1)
    prof = synthetic_profile(value, ((value - v_hat) / sigma) ** 2)
    lo, hi = profile_confidence_intervals(prof)[0]
    half = sigma * np.sqrt(chi2.ppf(0.95, 1))
    assert abs(lo - (v_hat - half)) <= 1e-3 * sigma and abs(hi - (v_hat + half)) <= 1e-3 * sigma
    # the chord lies above the parabola: the interpolated crossing is never outside the exact one
    assert lo >= v_hat - half and hi <= v_hat + half
    # another level
    lo68, hi68 = profile_confidence_intervals(prof, level=0.6827)[0]
    assert abs(hi68 - (v_hat + sigma)) <= 1e-3 * sigma and abs(lo68 - (v_hat - sigma)) <= 1e-3 * sigma


def test_flat_branches_are_not_identifiable():
    value = np.linspace(-1.0, 1.0, 9)
    flat = synthetic_profile(value, np.zeros(9))
    assert profile_confidence_intervals(flat).tolist() == [[-np.inf, np.inf]]
    # flat to the right only
    d = np.where(value < 0, (value / 0.2) ** 2, 0.01 * value)
    lo, hi = profile_confidence_intervals(synthetic_profile(value, d))[0]
    assert hi == np.inf and np.isfinite(lo)


def test_nan_and_unconverged_points_are_skipped():
    """The grid points next to the crossing are unusable: the crossing is interpolated between the usable points around
    them -- and a huge delta_chi2 at a point that did not converge is not a crossing."""
    value = np.arange(-4.0, 5.0)                    # centre 0, sigma = 1: exact crossing at +-1.96
    d = value ** 2
    conv = np.ones(9, dtype=bool)
    d[6] = np.nan                                   # v = 2
    conv[2] = False                                 # v = -2
    d[3] = 1e9                                      # v = -1: not converged, must not count
    conv[3] = False
    lo, hi = profile_confidence_intervals(synthetic_profile(value, d, conv))[0]
    thr = chi2.ppf(0.95, 1)
    assert hi == pytest.approx(1.0 + (thr - 1.0) * (3.0 - 1.0) / (9.0 - 1.0))          # between v = 1 and v = 3
    assert lo == pytest.approx(0.0 + (thr - 0.0) * (-3.0 - 0.0) / (9.0 - 0.0))         # between v = 0 and v = -3
    # everything beyond the centre unusable on one side
    conv2 = np.ones(9, dtype=bool)
    conv2[:4] = False
    lo2, _ = profile_confidence_intervals(synthetic_profile(value, value ** 2, conv2))[0]
    assert lo2 == -np.inf


def test_each_side_comes_from_its_own_branch():
    value = np.linspace(-2.0, 2.0, 41)
    d = np.where(value < 0, (value / 0.3) ** 2, (value / 0.6) ** 2)
    two = synthetic_profile(np.stack([value, value + 5.0]), np.stack([d, d[::-1]]))
    ci = profile_confidence_intervals(two)
    u = np.sqrt(chi2.ppf(0.95, 1))
    assert ci.shape == (2, 2)
    assert ci[0, 0] == pytest.approx(-0.3 * u, abs=2e-3) and ci[0, 1] == pytest.approx(0.6 * u, abs=2e-3)
    assert ci[1, 0] == pytest.approx(5.0 - 0.6 * u, abs=2e-3) and ci[1, 1] == pytest.approx(5.0 + 0.3 * u, abs=2e-3)


class _Names:
    """What normalize_held needs of a project: get_param_index."""
    idx = {'k_synt': {'Global': 2}, 'Group_1': {('High',): 0, ('Low',): 1}}

    def get_param_index(self, group, settings='all'):
        return self.idx[group] if isinstance(settings, str) and settings == 'all' else self.idx[group][settings]


def test_every_form_of_held_gives_the_same_mask():
    V, q = 4, 3
    want = np.tile([False, True, True], (V, 1))
    forms = [np.array([False, True, True]), want.copy(), [1, 2], (2, 1), np.array([1, 2]), [-1, 1], [1, 1, 2],
             [('Group_1', ('Low',)), ('k_synt', 'Global')]]
    for form in forms:
        got = normalize_held(form, V, q, _Names())
        assert got.dtype == np.bool_ and got.shape == (V, q) and got.flags['C_CONTIGUOUS'] and np.array_equal(got, want), form
    assert np.array_equal(normalize_held([('Group_1', 'all')], V, q, _Names()), np.tile([True, True, False], (V, 1)))
    assert not normalize_held([], V, q).any()
    per_start = np.eye(3, dtype=bool)
    assert np.array_equal(normalize_held(per_start, 3, 3), per_start)


@pytest.mark.parametrize('bad', [np.zeros(4, dtype=bool), np.zeros((3, 3), dtype=bool), np.zeros((4, 3, 1), dtype=bool), [3], [-4],
                                 [0.5], np.zeros((2, 2), dtype=int), [('Group_1', ('Medium',))], [('nothing', 'Global')]])
def test_bad_held_arguments_raise(bad):
    with pytest.raises(ValueError):
        normalize_held(bad, 4, 3, _Names())


def test_param_indices_of_a_profile():
    assert param_indices(_Names(), 'all', 3).tolist() == [0, 1, 2]
    assert param_indices(_Names(), range(2), 3).tolist() == [0, 1]
    assert param_indices(_Names(), [('k_synt', 'Global'), 0], 3).tolist() == [2, 0]
    for bad in ([3], [-1], [0, 0], 'some', [('Group_1', ('Medium',))]):
        with pytest.raises(ValueError):
            param_indices(_Names(), bad, 3)


def test_header_declares_the_held_step_and_the_binding_has_one_more_pointer():
    import ctypes
    from sysbio_modeling_amd import _lib
    with open(os.path.join(REPO, 'include', 'sbm.h')) as fh:
        header = fh.read()
    assert re.search(r'#define\s+SBM_ABI_VERSION\s+4\b', header) and _lib.ABI_VERSION == 4
    decl = re.search(r'int\s+sbm_lm_trust_step_held\s*\(([^;]*)\)\s*;', header)
    decl_ex = re.search(r'int\s+sbm_lm_trust_step_ex\s*\(([^;]*)\)\s*;', header)
    assert decl and decl_ex
    args, args_ex = [a.strip() for a in decl.group(1).split(',')], [a.strip() for a in decl_ex.group(1).split(',')]
    assert args[:-1] == args_ex and re.fullmatch(r'const\s+int32_t\s*\*\s*held_dev', args[-1])
    sig = _lib.SIGNATURES
    res, held_args = sig['sbm_lm_trust_step_held']
    res_ex, ex_args = sig['sbm_lm_trust_step_ex']
    assert res is res_ex is ctypes.c_int
    assert list(held_args[:-1]) == list(ex_args) and held_args[-1] is ctypes.c_void_p and len(held_args) == len(args)
