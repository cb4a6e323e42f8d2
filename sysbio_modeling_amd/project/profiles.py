"""Profile likelihoods on top of ``fit_batch(held=...)`` (project/fitting.py).

The standard identifiability analysis of a sloppy model: for a parameter theta_i, step it away from the optimum and
re-fit all the others at every step; where 2 (cost - cost_hat) crosses the chi^2_1 quantile is the end of the confidence
interval, and a profile that stays flat says the data do not determine the parameter.  Every profile point is an lmder
fit with one column removed, so the 2 P branches of P parameters (one per direction) are the starts of ONE
``fit_batch`` call per grid step, each start holding a different column (``sbm_lm_trust_step_held`` compacts every
start's system separately) -- where a host loop runs 2 P K serial ``leastsq`` calls.

Parameters are log-parameters, so the grid steps are log units.
"""
from __future__ import annotations

import numpy as np

from .fitting import is_param_pair, param_pair_indices

# what fit_batch itself consumes; everything else in **fit_options is an integrator override (method, rtol, ...)
_FIT_KEYS = ('max_iter', 'lambda0', 'lambda_up', 'lambda_down', 'ftol', 'xtol', 'max_step', 'trace', 'lazy_jacobian', 'algorithm',
             'factor', 'bounds', 'geodesic')


def param_indices(project, params, q):
    """``params`` of `profile_likelihood_batch` as an int array: 'all', parameter indices, or ``(p_group, settings)`` pairs
    as ``get_param_index`` takes them.  ValueError on an index outside [0, q), a repeated or an unknown parameter."""
    if isinstance(params, str):
        if params != 'all':
            raise ValueError("params: 'all', a list of indices or of (p_group, settings) pairs")
        return np.arange(q)
    out = []
    for it in params:
        if is_param_pair(it):
            out += param_pair_indices(project, it, 'params')
        else:
            out.append(int(it))
    idx = np.asarray(out, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= q):
        raise ValueError("params: parameter index out of range for %d parameters" % q)
    if len(set(idx.tolist())) != idx.size:
        raise ValueError("params: a parameter is named twice")
    return idx


def profile_likelihood_batch(project, theta_hat, params='all', offsets=np.linspace(0.1, 2.0, 20), continuation=True,
                             stop_delta_chi2=None, **fit_options):
    """Profiles of 0.5 |r|^2 along ``params`` around ``theta_hat`` (q,), an optimum found before (``fit_batch``).

    ``offsets`` (K,), strictly increasing and positive, are used in both directions: parameter i is held at
    ``theta_hat[i] - offsets[k]`` and ``theta_hat[i] + offsets[k]`` while all the others are fitted
    (``fit_batch(held=...)``; ``fit_options`` go there: max_iter, ftol, ..., integrator overrides).  ``bounds=`` among them
    keeps the fitted parameters in a box: a ``(lower, upper)`` pair of scalars or (q,) arrays, or a dict of
    ``(p_group, settings)`` names, the same box for every branch; the profiled parameter, being held, is exempt from it,
    and ``theta_hat`` has to lie inside.  ``geodesic=`` among them (``True`` or ``dict(h=..., alpha=...)``) turns on the
    geodesic acceleration of every branch's steps, as in ``fit_batch``; together with ``bounds`` it is refused there.

    ``continuation=True``: the 2 P branches are the starts of one ``fit_batch`` call per grid step k; a branch starts from
    its own optimum of step k - 1 (``theta_hat`` at k = 0) -- K calls.  ``continuation=False``: all 2 P K points start from
    ``theta_hat``, in one call.  A point whose fit did not converge is flagged (``converged`` False) and its branch goes on
    from where it stopped.  A branch ends where its cost is not finite, and -- with ``stop_delta_chi2`` -- after the first
    point whose 2 (cost - cost_hat) exceeds it (that point is kept): the points after the end are NaN with
    ``converged`` False, and with continuation an ended branch leaves the batch: it is not integrated again.

    Returns a dict: param_index (P,); value (P, 2K+1), the grid of the held parameter, ascending, ``theta_hat[i]`` at
    position K; cost (P, 2K+1) = 0.5 |r|^2; theta (P, 2K+1, q); converged (P, 2K+1); cost_hat; delta_chi2 =
    2 (cost - cost_hat); n_evaluations (trial points integrated, over all calls).

    ``cost_hat`` is the cost at ``theta_hat`` AS GIVEN (one integration with sensitivities, as the fit evaluates its
    points).  A profile point that comes out below it -- ``theta_hat`` was not quite the optimum -- is reported as it is,
    with a negative ``delta_chi2``: nothing is re-centred.
    """
    theta_hat = np.asarray(theta_hat, dtype=np.float64)
    q = int(project.n_project_params)
    if theta_hat.shape != (q,):
        raise ValueError("theta_hat has shape %s, the project has %d parameters" % (theta_hat.shape, q))
    idx = param_indices(project, params, q)
    off = np.asarray(offsets, dtype=np.float64)
    if off.ndim != 1 or off.size == 0 or not np.all(off > 0) or not np.all(np.diff(off) > 0):
        raise ValueError("offsets must be positive and strictly increasing")
    if fit_options.get('trace'):
        raise ValueError("profile_likelihood_batch: trace is an option of a single fit_batch call")
    P, K = idx.size, off.size
    overrides = {k: v for k, v in fit_options.items() if k not in _FIT_KEYS}
    at_hat = project.evaluate_batch(theta_hat[None, :], jacobian=True, want=('jacobian',), **overrides)
    cost_hat = 0.5 * float(np.asarray(_host(at_hat['norms']))[0])
    n_eval = 1

    B = 2 * P                                           # branch b = 2 j + s: parameter idx[j], direction -1 (s = 0) / +1
    b_par = np.repeat(idx, 2)
    b_sign = np.tile([-1.0, 1.0], P)
    cost = np.full((B, K), np.nan)
    theta = np.full((B, K, q), np.nan)
    conv = np.zeros((B, K), dtype=bool)
    target = theta_hat[b_par][:, None] + b_sign[:, None] * off[None, :]           # (B, K) the held values

    def held_rows(rows):
        m = np.zeros((len(rows), q), dtype=bool)
        m[np.arange(len(rows)), b_par[rows]] = True
        return m

    if continuation:
        cur = np.tile(theta_hat, (B, 1))
        alive = np.ones(B, dtype=bool)
        for k in range(K):
            rows = np.nonzero(alive)[0]
            if rows.size == 0:
                break
            starts = cur[rows].copy()
            starts[np.arange(rows.size), b_par[rows]] = target[rows, k]
            fit = project.fit_batch(starts, held=held_rows(rows), **fit_options)
            n_eval += int(fit['n_evaluations'])
            cost[rows, k], theta[rows, k], conv[rows, k] = fit['cost'], fit['theta'], fit['converged']
            cur[rows] = fit['theta']
            ended = ~np.isfinite(fit['cost'])
            if stop_delta_chi2 is not None:
                ended |= 2.0 * (fit['cost'] - cost_hat) > stop_delta_chi2
            alive[rows[ended]] = False
    elif P:
        rows = np.repeat(np.arange(B), K)
        starts = np.tile(theta_hat, (B * K, 1))
        starts[np.arange(B * K), b_par[rows]] = target.reshape(-1)
        fit = project.fit_batch(starts, held=held_rows(rows), **fit_options)
        n_eval += int(fit['n_evaluations'])
        cost, theta, conv = fit['cost'].reshape(B, K).copy(), fit['theta'].reshape(B, K, q).copy(), fit['converged'].reshape(B, K).copy()
        # the same ends, after the fact
        ended = ~np.isfinite(cost)
        if stop_delta_chi2 is not None:
            ended |= 2.0 * (cost - cost_hat) > stop_delta_chi2
        after = np.cumsum(ended, axis=1) - ended > 0                              # strictly after a branch's first end
        cost[after], theta[after], conv[after] = np.nan, np.nan, False
    conv &= np.isfinite(cost)

    # (P, 2K+1): the minus branch reversed, the centre, the plus branch
    def arrange(minus, centre, plus):
        return np.concatenate([minus[:, ::-1], centre, plus], axis=1)
    value = arrange(target[0::2], theta_hat[idx][:, None], target[1::2])
    cost_out = arrange(cost[0::2], np.full((P, 1), cost_hat), cost[1::2])
    theta_out = arrange(theta[0::2], np.tile(theta_hat, (P, 1, 1)), theta[1::2])
    conv_out = arrange(conv[0::2], np.ones((P, 1), dtype=bool), conv[1::2])
    return {'param_index': idx, 'value': value, 'cost': cost_out, 'theta': theta_out, 'converged': conv_out,
            'cost_hat': cost_hat, 'delta_chi2': 2.0 * (cost_out - cost_hat), 'n_evaluations': n_eval}


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else x


def profile_confidence_intervals(profile, level=0.95):
    """Likelihood-based confidence intervals from a profile dict: per parameter the (lower, upper) value of the held
    parameter where ``delta_chi2`` first reaches ``scipy.stats.chi2.ppf(level, 1)`` moving outwards from the centre,
    interpolated linearly between the two grid points around the crossing.  -inf / +inf where a branch never gets there:
    the parameter is not identifiable in that direction on this grid.  Points that are NaN or not converged are not used
    (the crossing is looked for between the usable points around them).  Pure numpy; returns an array (P, 2)."""
    from scipy.stats import chi2
    thr = float(chi2.ppf(level, 1))
    value, d = np.asarray(profile['value'], dtype=np.float64), np.asarray(profile['delta_chi2'], dtype=np.float64)
    ok = np.asarray(profile['converged'], dtype=bool) & np.isfinite(d) & np.isfinite(value)
    P, n = value.shape
    K = (n - 1) // 2
    out = np.empty((P, 2))
    for j in range(P):
        for side, step, never in ((0, -1, -np.inf), (1, 1, np.inf)):
            out[j, side] = never
            v0, d0 = value[j, K], d[j, K]
            for k in range(1, K + 1):
                c = K + step * k
                if not ok[j, c]:
                    continue
                if d[j, c] >= thr:
                    out[j, side] = value[j, c] if d[j, c] == d0 else v0 + (thr - d0) * (value[j, c] - v0) / (d[j, c] - d0)
                    break
                v0, d0 = value[j, c], d[j, c]
    return out
