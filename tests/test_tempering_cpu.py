"""Parallel tempering (project/ensembles.py, ``temperature=`` a ladder and ``swap_every=``), the parts that run without a
device: the arguments, the C ABI of the three added entries, and the 'host' sampler on posteriors that are known -- a
Gaussian, whose rung k must come out sqrt(T_k) times as wide, and a double well, which a chain at T = 1 never crosses."""
import os
import re

import numpy as np
import pytest

from tests.support.sampler_stand_ins import QuadraticProject
from tests.support.tempering_oracle import DoubleWellProject, lower_chains, swap_step

from sysbio_modeling_amd import _lib
from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch, temperature_ladder

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gaussian():
    rng = np.random.default_rng(8)
    W = rng.standard_normal((12, 3)) * np.array([3.0, 1.0, 0.4])
    mu = np.array([0.3, -1.0, 2.0])
    return QuadraticProject(W, mu, 0.0), W, mu


def test_temperature_ladder_is_geometric():
    assert np.array_equal(temperature_ladder(4, 8.0), np.geomspace(1.0, 8.0, 4))
    assert np.allclose(temperature_ladder(4, 8.0), [1.0, 2.0, 4.0, 8.0], rtol=1e-15)


def test_arguments():
    proj, W, mu = _gaussian()
    starts = np.tile(mu, (8, 1))
    run = lambda **kw: ensemble_log_params_batch(proj, kw.pop('starts', starts), hess=W.T @ W, steps=4, energy='rss', **kw)     # noqa: E731
    with pytest.raises(ValueError, match='first algorithm'):
        run(temperature=[1.0, 2.0], recalc_hess_alg=True)
    with pytest.raises(ValueError, match='first algorithm'):
        run(temperature=[1.0, 2.0], sampler='device_recalc')
    with pytest.raises(ValueError, match='whole number of ladders'):
        run(temperature=[1.0, 2.0, 4.0])
    for bad in ([1.0, 0.0], [1.0, -2.0], [1.0, np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError, match='finite and > 0'):
            run(temperature=bad)
    with pytest.raises(ValueError, match='K >= 2'):
        run(temperature=[1.0])
    with pytest.raises(ValueError, match='swap_every'):
        run(temperature=1.0, swap_every=2)
    with pytest.raises(ValueError, match='positive whole number'):
        run(temperature=[1.0, 2.0], swap_every=0)
    with pytest.raises(ValueError, match='three arrays'):
        run(temperature=[1.0, 2.0], swap_every=2, sampler='device', draws=(np.zeros((4, 8, 3)), np.zeros((4, 8))))
    # what a swap would carry across must be the same on both sides: held mask, held values, box
    held = np.zeros((8, 3), dtype=bool)
    held[1, 2] = True
    with pytest.raises(ValueError, match='within every ladder'):
        run(temperature=[1.0, 2.0], swap_every=2, held=held)
    held[:, 2] = True
    moved = starts.copy()
    moved[3, 2] += 0.1
    with pytest.raises(ValueError, match='within every ladder'):
        run(temperature=[1.0, 2.0], swap_every=2, held=held, starts=moved)
    lo = np.full((8, 3), -50.0)
    lo[5, 0] = -40.0
    with pytest.raises(ValueError, match='within every ladder'):
        run(temperature=[1.0, 2.0], swap_every=2, bounds=(lo, np.full((8, 3), 50.0)))
    # equal within each ladder, different between ladders: legal; and without swaps the chains are independent
    moved = starts.copy()
    moved[2:4, 2] += 0.1
    out = run(temperature=[1.0, 2.0], swap_every=2, held=held, starts=moved, seeds=1)
    assert len(out) == 4 and np.array_equal(out[0][:, :, 2], np.broadcast_to(moved[:, 2], (5, 8)))
    held[1, 2] = False
    assert len(run(temperature=[1.0, 2.0], held=held, seeds=1)) == 4


def _declared_arity(name):
    """number of parameters of ``name`` in include/sbm.h, comments removed (as test_sf_quadrature_cpu.py reads the header)"""
    with open(os.path.join(REPO, 'include', 'sbm.h')) as fh:
        text = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, text)
    assert m, "include/sbm.h does not declare %s" % name
    return len(m.group(1).split(','))


def test_added_entries_are_declared_bound_and_exported():
    lib = _lib.load_library()
    for name, n_args in (('sbm_project_sf_entropy_pt', 6), ('sbm_mh_accept_pt', 15), ('sbm_pt_swap', 13)):
        assert _declared_arity(name) == n_args == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name), "libsbm_hip.so does not export %s" % name
    # the _pt entries take their scalar counterparts' arguments, a pointer where the temperature was
    for pt, scalar, at in (('sbm_project_sf_entropy_pt', 'sbm_project_sf_entropy', 3), ('sbm_mh_accept_pt', 'sbm_mh_accept_ex', 5)):
        a, b = _lib.SIGNATURES[pt][1], _lib.SIGNATURES[scalar][1]
        assert _declared_arity(scalar) == len(b) and a[:at] + a[at + 1:] == b[:at] + b[at + 1:]
        assert b[at] is _lib.ctypes.c_double and a[at] is _lib.ctypes.c_void_p
    assert lib.sbm_abi_version() == _lib.ABI_VERSION == 4


def test_return_value_of_a_ladder():
    """The last element: layout, attempts (they depend on the step count alone) and accepts at the lower chains only; the
    same seed gives the same run, and the move streams do not depend on the swaps."""
    proj, W, mu = _gaussian()
    T = [1.0, 4.0, 2.0]                     # need not be sorted
    kw = dict(hess=W.T @ W, steps=21, energy='rss', temperature=T, seeds=3)
    ens, ens_F, ratio, info = ensemble_log_params_batch(proj, np.tile(mu, (6, 1)), swap_every=2, **kw)
    assert ens.shape == (22, 6, 3) and ens_F.shape == (22, 6) and ratio.shape == (6,)
    assert np.array_equal(info['temperature'], [1.0, 4.0, 2.0] * 2) and np.array_equal(info['rung'], [0, 1, 2] * 2)
    assert np.array_equal(info['ladder'], [0, 0, 0, 1, 1, 1])
    # 10 swap steps: parities 0, 1, 0, ... -- five each; parity 0 pairs rungs (0, 1), parity 1 rungs (1, 2)
    assert np.array_equal(info['swap_attempted'], [5, 5, 0] * 2)
    assert np.all(info['swap_accepted'] <= info['swap_attempted']) and info['swap_accepted'].sum() > 0
    again = ensemble_log_params_batch(proj, np.tile(mu, (6, 1)), swap_every=2, **kw)
    assert len(again) == 4 and np.array_equal(again[0], ens) and np.array_equal(again[3]['swap_accepted'], info['swap_accepted'])
    # no swaps: the first step of every chain -- the first swap follows step 2 -- is that of the run with swaps, since the
    # swap numbers come from a stream of their own
    plain = ensemble_log_params_batch(proj, np.tile(mu, (6, 1)), **kw)
    assert np.array_equal(plain[0][:2], ens[:2]) and not plain[3]['swap_attempted'].any() and not plain[3]['swap_accepted'].any()
    # energies recorded are those of the recorded points
    assert np.allclose(ens_F, 0.5 * np.sum(np.einsum('rj,scj->scr', W, ens - mu) ** 2, axis=2), rtol=1e-12, atol=1e-12)


def test_host_swap_is_the_oracles_rule():
    """The numpy swap of the host sampler against the oracle's restatement, on random states with a cross energy"""
    from sysbio_modeling_amd.project.ensembles import _host_swap, _temperature_ladder_arguments
    rng = np.random.default_rng(12)
    C, K, q = 10, 5, 3
    T = np.array([1.0, 1.5, 2.0, 3.0, 5.0])
    starts = rng.standard_normal((C, q))
    ladder = _temperature_ladder_arguments(T, 1, starts, 4, 'host', False, None, None)
    for parity in (0, 1):
        assert np.array_equal(np.flatnonzero(ladder['lower'][parity]), lower_chains(C, K, parity))
        i = lower_chains(C, K, parity)
        want = ladder['chain_T'].copy()
        want[i], want[i + 1] = ladder['chain_T'][i + 1], ladder['chain_T'][i]
        assert np.array_equal(ladder['partner_T'][parity], want)
        F, X, log_u = rng.uniform(0, 5, C), rng.uniform(0, 5, C), np.log(rng.random(C))
        X[3] = np.inf
        n0 = np.arange(C)
        ref = swap_step(K, parity, ladder['chain_T'], X, log_u, starts, F, n0)
        n = n0.copy()
        curr, newF = _host_swap(ladder, parity, starts, F, X, log_u, n)
        assert np.array_equal(curr, ref[0]) and np.array_equal(newF, ref[1]) and np.array_equal(n, ref[2])
        assert 0 < len(ref[5]) < len(i)


def test_host_sampler_samples_every_rung_of_a_gaussian():
    """temperature_ladder(4, 4.0), 32 ladders, 400 steps, swaps every 2: rung k samples N(mu, T_k (W^T W)^-1).  Pooled over
    ens[100:, k::4]: standard deviations within rtol 0.15 of sqrt(T_k) x the exact ones (the tolerance of the Gaussian
    posterior tests of the samplers), means within 0.2 sqrt(T_k) sd (their 0.1, doubled: a rung holds a quarter of their
    samples).  A numpy prototype of the algorithm gave at worst 0.043 and 0.068 over 20 seeds; a rule that always swaps
    inflates the cold standard deviation to 1.45 x."""
    proj, W, mu = _gaussian()
    T = temperature_ladder(4, 4.0)
    ens, ens_F, ratio, info = ensemble_log_params_batch(proj, np.tile(mu, (128, 1)), steps=400, temperature=T, swap_every=2,
                                                        seeds=17, energy='rss')
    assert ens.shape == (401, 128, 3) and 0.3 < ratio.mean() < 0.8
    sd = np.sqrt(np.diag(np.linalg.inv(W.T @ W)))
    for k in range(4):
        pooled = ens[100:, k::4].reshape(-1, 3)
        dev_sd = np.max(np.abs(pooled.std(axis=0) / (np.sqrt(T[k]) * sd) - 1.0))
        dev_mean = np.max(np.abs(pooled.mean(axis=0) - mu) / (np.sqrt(T[k]) * sd))
        print("rung %d (T = %.3f): sd off by %.3f (rtol 0.15), mean off by %.3f sd (0.2)" % (k, T[k], dev_sd, dev_mean))
        assert np.allclose(pooled.std(axis=0), np.sqrt(T[k]) * sd, rtol=0.15)
        assert np.all(np.abs(pooled.mean(axis=0) - mu) < 0.2 * np.sqrt(T[k]) * sd)
    assert np.all(info['swap_accepted'][info['rung'] < 3] > 0) and not info['swap_accepted'][info['rung'] == 3].any()


def test_tempering_crosses_a_barrier_that_a_cold_chain_does_not():
    """r = ((theta_0^2 - 1) / 0.15, theta_1): two equal basins behind a barrier of 22 at T = 1.  All chains start in the left
    one, (-1, 0), with the Hessian at the start.  16 chains x 2000 steps at T = 1 never show theta_0 > 0 (the condition that
    makes this test mean something; a prototype gave exactly 0 over 10 runs).  With temperature_ladder(6, 32.0), 16 ladders and
    swaps every 5 steps, the share of rung-0 samples after step 500 with theta_0 > 0 lies in [0.35, 0.65] (prototype: 0.46 ...
    0.56 over 10 runs), the rung-0 standard deviation of theta_1 is within 0.15 of 1, and every adjacent pair's swap ratio is
    above 0.3 (prototype: 0.64 ... 0.74)."""
    proj = DoubleWellProject(0.15)
    start = np.array([-1.0, 0.0])
    J = proj.evaluate_batch(start[None], jacobian=True)['jacobian'][0]
    hess = J.T @ J
    cold, _, _ = ensemble_log_params_batch(proj, np.tile(start, (16, 1)), hess=hess, steps=2000, temperature=1.0, seeds=21,
                                           energy='rss')
    assert cold.shape == (2001, 16, 2) and not np.any(cold[:, :, 0] > 0.0)
    K = 6
    ens, ens_F, ratio, info = ensemble_log_params_batch(proj, np.tile(start, (16 * K, 1)), hess=hess, steps=2000,
                                                        temperature=temperature_ladder(K, 32.0), swap_every=5, seeds=22, energy='rss')
    rung0 = ens[501:, ::K]
    share = np.mean(rung0[:, :, 0] > 0.0)
    sd1 = rung0[:, :, 1].std()
    pairs = info['rung'] < K - 1
    swap_ratio = (info['swap_accepted'][pairs] / info['swap_attempted'][pairs]).reshape(16, K - 1)      # (ladder, pair of rungs)
    print("double well: share right of the barrier %.3f, sd(theta_1) %.3f, swap ratios per pair of rungs %s, lowest of a ladder %.3f"
          % (share, sd1, np.round(swap_ratio.mean(axis=0), 3), swap_ratio.min()))
    assert 0.35 <= share <= 0.65
    assert abs(sd1 - 1.0) <= 0.15
    assert np.all(info['swap_attempted'][pairs] == 200) and np.all(swap_ratio.mean(axis=0) > 0.3)
