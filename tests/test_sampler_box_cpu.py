"""``held=`` and ``bounds=`` of the samplers (project/ensembles.py), the parts that run without a device: the padded
layout of ``sampling_axes(held=)`` -- what ``sbm_sampling_axes_held`` returns (include/sbm.h) -- against the reduced problem,
the 'host' sampler on a posterior whose truncated form is known, and the arguments."""
import numpy as np
import pytest

from tests.support.sampler_stand_ins import QuadraticProject, conditional_gaussian

from sysbio_modeling_amd.project.ensembles import (_log_candidate_density, ensemble_log_params_batch, sampling_axes,
                                                   sampling_matrix)


def _spd(rng, q, decades=4.0):
    B = rng.standard_normal((q + 3, q)) * 10.0 ** rng.uniform(-decades / 2, 0.0, q)
    return B.T @ B


@pytest.mark.parametrize('cutoff, T, scale', [(0.0, 1.0, 1.0), (1e-2, 2.0, 0.7)])
def test_padded_axes_are_the_reduced_problem(cutoff, T, scale):
    rng = np.random.default_rng(3)
    q = 7
    H = _spd(rng, q)
    masks = [np.zeros(q, bool), np.eye(q, dtype=bool)[0], np.eye(q, dtype=bool)[q - 1], ~np.eye(q, dtype=bool)[3],
             np.ones(q, bool), rng.random(q) < 0.5]
    for mask in masks:
        free = np.flatnonzero(~mask)
        nf = free.size
        V, s = sampling_axes(H, cutoff, T, scale, held=mask)
        assert V.shape == (q, q) and s.shape == (q,)
        assert np.array_equal(V[mask], np.zeros((q - nf, q))) and np.array_equal(V[:, nf:], np.zeros((q, q - nf)))
        assert np.array_equal(s[nf:], np.ones(q - nf))
        M = sampling_matrix(H, cutoff, T, scale, held=mask)
        assert np.array_equal(M, V * s[None, :])
        if nf == 0:
            continue
        Vr, sr = sampling_axes(H[np.ix_(free, free)], cutoff, T, scale)
        assert np.array_equal(V[free][:, :nf], Vr) and np.array_equal(s[:nf], sr)
        # the candidate density of a move in the free subspace is the reduced problem's
        d_red = rng.standard_normal((5, nf)) * sr.max()
        d = np.zeros((5, q))
        d[:, free] = d_red
        full = _log_candidate_density(d, np.broadcast_to(V, (5, q, q)), np.broadcast_to(s, (5, q)))
        red = _log_candidate_density(d_red, np.broadcast_to(Vr, (5, nf, nf)), np.broadcast_to(sr, (5, nf)))
        assert np.allclose(full, red, rtol=1e-13, atol=0.0)
    # no mask: the output of before, to the bit; a mask per Hessian: each its own reduced problem
    assert all(np.array_equal(x, y) for x, y in zip(sampling_axes(H, cutoff, T, scale, held=None), sampling_axes(H, cutoff, T, scale)))
    Hs = np.stack([_spd(rng, q) for _ in range(len(masks))])
    Vb, sb = sampling_axes(Hs, cutoff, T, scale, held=np.stack(masks))
    for k, mask in enumerate(masks):
        V1, s1 = sampling_axes(Hs[k], cutoff, T, scale, held=mask)
        assert np.array_equal(Vb[k], V1) and np.array_equal(sb[k], s1)


@pytest.fixture(scope='module')
def gaussian():
    rng = np.random.default_rng(8)
    W = rng.standard_normal((12, 3)) * np.array([3.0, 1.0, 0.4])
    mu = np.array([0.3, -1.0, 2.0])
    held = np.array([False, False, True])
    value = mu[2] + 1.5
    m, c = conditional_gaussian(W, mu, held, [value])
    return W, mu, held, value, m, c


@pytest.mark.parametrize('recalc', [False, True])
@pytest.mark.parametrize('box', [(0.0, np.inf), (-0.5, 1.0)])
def test_host_sampler_reproduces_a_known_truncated_posterior(gaussian, box, recalc):
    """N(mu, (W^T W)^-1) with parameter 2 held at mu_2 + 1.5 and parameter 0 confined to m_0 + [a, b] sd_0 (m, sd: the
    Gaussian conditional on the held value): parameter 0 is a truncated normal, parameter 1 given parameter 0 is normal with
    mean m_1 + (c_01 / c_00) (x_0 - m_0).  Tolerances as in the known-posterior test of tests/test_control_loops.py: means
    within 0.06 of the exact standard deviation of the component, variances within 12 %."""
    from scipy.stats import truncnorm
    W, mu, held, value, m, c = gaussian
    sd0 = np.sqrt(c[0, 0])
    lo, hi = m[0] + box[0] * sd0, m[0] + box[1] * sd0
    lower = np.array([lo, -np.inf, -np.inf])
    upper = np.array([hi, np.inf, np.inf])
    start = np.array([m[0] + 0.25 * sd0, m[1], value])
    proj = QuadraticProject(W, mu)
    kw = dict(steps=300, seeds=5, energy='rss', recalc_hess_alg=recalc, held=held, bounds=(lower, upper))
    ens, ens_F, ratio = ensemble_log_params_batch(proj, np.tile(start, (256, 1)), **kw)
    assert ens.shape == (301, 256, 3) and ens_F.shape == (301, 256)
    assert np.array_equal(ens[:, :, 2], np.full((301, 256), value))
    assert np.all((ens[:, :, 0] >= lo) & (ens[:, :, 0] <= hi))
    # no point outside the box was ever evaluated, and the held parameter never anywhere else
    for th in proj.seen:
        assert np.all((th[:, 0] >= lo) & (th[:, 0] <= hi)) and np.all(th[:, 2] == value)
    assert np.allclose(ens_F, 0.5 * np.sum(((ens - mu) @ W.T) ** 2, axis=2), rtol=1e-12)
    x0, x1 = ens[60:, :, 0].ravel(), ens[60:, :, 1].ravel()
    tn = truncnorm(box[0], box[1], loc=m[0], scale=sd0)
    slope = c[0, 1] / c[0, 0]
    mean1 = m[1] + slope * (tn.mean() - m[0])
    var1 = c[1, 1] - c[0, 1] ** 2 / c[0, 0] + slope ** 2 * tn.var()
    print("box %s recalc %s: ratio %.3f, mean errors %.4f %.4f sd, variance errors %.4f %.4f"
          % (box, recalc, ratio.mean(), (x0.mean() - tn.mean()) / tn.std(), (x1.mean() - mean1) / np.sqrt(var1),
             x0.var() / tn.var() - 1.0, x1.var() / var1 - 1.0))
    assert 0.2 < ratio.mean() < 0.8
    assert abs(x0.mean() - tn.mean()) < 0.06 * tn.std()
    assert abs(x1.mean() - mean1) < 0.06 * np.sqrt(var1)
    assert abs(x0.var() / tn.var() - 1.0) < 0.12 and abs(x1.var() / var1 - 1.0) < 0.12
    again = ensemble_log_params_batch(proj, np.tile(start, (256, 1)), **kw)
    assert all(np.array_equal(x, y) for x, y in zip(again, (ens, ens_F, ratio)))


def test_everything_held_stays_put_and_masks_may_differ(gaussian):
    W, mu = gaussian[0], gaussian[1]
    masks = np.array([[True, True, True], [False, True, False], [False, False, False]])
    starts = mu + np.array([[0.1, 0.2, 0.3], [0.0, 0.5, 0.0], [0.0, 0.0, 0.0]])
    for recalc in (False, True):
        ens, ens_F, ratio = ensemble_log_params_batch(QuadraticProject(W, mu, 0.3), starts, steps=40, seeds=2, energy='rss',
                                                      recalc_hess_alg=recalc, held=masks)
        assert np.array_equal(ens[:, masks], np.broadcast_to(starts[masks], (41, masks.sum())))
        assert ratio[0] == 0.0 and np.all(ens_F[:, 0] == ens_F[0, 0]) and ratio[1] > 0.0 and ratio[2] > 0.0
        assert np.ptp(ens[:, 1, 0]) > 0.0 and np.ptp(ens[:, 2, 1]) > 0.0


def test_arguments(gaussian):
    W, mu = gaussian[0], gaussian[1]
    starts = np.tile(mu, (4, 1))
    for recalc in (False, True):
        kw = dict(steps=25, seeds=11, energy='rss', recalc_hess_alg=recalc)
        plain = ensemble_log_params_batch(QuadraticProject(W, mu, 0.2), starts, **kw)
        named = ensemble_log_params_batch(QuadraticProject(W, mu, 0.2), starts, held=None, bounds=None, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(plain, named))
    proj = QuadraticProject(W, mu)
    with pytest.raises(ValueError, match='infeasible'):
        ensemble_log_params_batch(proj, starts, steps=3, energy='rss', bounds=(mu + 0.1, mu + 1.0))
    # a held column is exempt from the bounds: the same box with its violated side held is a legal start
    ensemble_log_params_batch(proj, starts, steps=3, energy='rss', bounds=(mu + 0.1, mu + 1.0), held=np.ones(3, bool))
    with pytest.raises(ValueError, match='held'):
        ensemble_log_params_batch(proj, starts, steps=3, energy='rss', held=np.zeros(4, bool))
    with pytest.raises(ValueError, match='held'):
        ensemble_log_params_batch(proj, starts, steps=3, energy='rss', held=np.zeros((3, 3), bool))
    with pytest.raises(ValueError, match='held'):
        sampling_axes(W.T @ W, held=np.zeros(4, bool))
    with pytest.raises(ValueError, match='draws'):
        ensemble_log_params_batch(proj, starts, steps=3, energy='rss', held=[2], bounds=(-10.0, 10.0),
                                  draws=(np.zeros((3, 4, 3)), np.zeros((3, 4))))
