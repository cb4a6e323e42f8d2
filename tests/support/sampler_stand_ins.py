"""Stand-ins for Project in the samplers' tests: what ``ensemble_log_params_batch(sampler='host')`` asks of a project,
with a posterior that is known in closed form."""
import numpy as np


class QuadraticProject:
    """Residuals r = W (theta - mu) * g(theta), g = 1 + bend tanh(theta_0 - mu_0): for bend = 0 the posterior
    exp(-0.5 |r|^2) is the Gaussian N(mu, (W^T W)^-1); a bend makes the Gauss-Newton Hessian vary from point to point."""
    reference_compat = False
    scale_factors = None

    def __init__(self, W, mu, bend=0.0):
        self.W, self.mu, self.bend = np.asarray(W, dtype=float), np.asarray(mu, dtype=float), float(bend)
        self.n_calls = 0
        self.seen = []            # every batch of points that was evaluated

    def evaluate_batch(self, thetas, jacobian=False, want=(), **kw):
        self.n_calls += 1
        th = np.atleast_2d(thetas)
        self.seen.append(th.copy())
        d = th - self.mu
        stretch = 1.0 + self.bend * np.tanh(d[:, :1])                  # (C, 1)
        r = np.einsum('rj,cj->cr', self.W, d) * stretch
        out = {'residuals': r, 'norms': np.sum(r * r, axis=1), 'status': np.zeros(len(r), dtype=np.int32)}
        if jacobian:
            dstretch = np.zeros_like(d)
            dstretch[:, 0] = self.bend / np.cosh(d[:, 0]) ** 2
            out['jacobian'] = self.W[None] * stretch[:, :, None] + np.einsum('cr,cj->crj', r / stretch, dstretch)
        return out


def conditional_gaussian(W, mu, held, values):
    """Mean (nf,) and covariance (nf, nf) of the free parameters of N(mu, (W^T W)^-1) given theta[held] = values"""
    held = np.asarray(held, dtype=bool)
    P = W.T @ W
    cov = np.linalg.inv(P[~held][:, ~held])
    mean = mu[~held] - cov @ P[~held][:, held] @ (np.asarray(values, dtype=float) - mu[held])
    return mean, cov
