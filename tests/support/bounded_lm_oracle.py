"""The bounded trust-region step (include/sbm.h: sbm_lm_trust_step_bounded, steps 1 - 6) and the fitting loop around it,
one start at a time in plain float64 numpy, on oracle/lmder_oracle.py's lmpar_reference and lm_update_reference.

Written from the contract in sbm.h, not from the kernel: the gradient is a matrix product, lmpar is the oracle's bisection
(another lambda within the 10 % MINPACK accepts than the kernel's Newton iteration finds), so single steps agree with the
device in what is decided -- the active set, what is projected, the status -- and loops agree in where they end.
"""
import math

import numpy as np

from oracle import lmder_oracle as lo

FREE, HELD, AT_LOWER, AT_UPPER = 0, 1, 2, 3


def active_set(J, r, theta, lower, upper, held=None, row_scale=None):
    """Steps 1 and 2: (codes (q,) int32, g (q,), gabs (q,) = sum_m |rs J r|, the scale a sign of g is to be judged by)."""
    Js = J if row_scale is None else J * np.asarray(row_scale)[:, None]
    terms = Js * np.asarray(r)[:, None]
    g = terms.sum(axis=0)
    code = np.zeros(J.shape[1], dtype=np.int32)
    code[(theta <= lower) & (g > 0.0)] = AT_LOWER
    code[(theta >= upper) & (g < 0.0)] = AT_UPPER
    if held is not None:
        code[np.asarray(held) != 0] = HELD
    return code, g, np.abs(terms).sum(axis=0)


def taken_step_quantities(Js, r, D, x):
    """pred = -g.x - |J x|^2 / 2, ||D x||, g.x of a step x as taken (clipped or projected)"""
    Jx = Js @ x
    gtx = float((Js.T @ r) @ x)
    return -gtx - 0.5 * float(Jx @ Jx), float(np.linalg.norm(D * x)), gtx


def bounded_step(J, r, dscale, radius, lam, theta, lower, upper, held=None, row_scale=None, max_step=0.0):
    """One start through steps 1 - 6.  Returns a dict: dscale, delta, trial (q,); lam, pred, dxnorm, gtx; status (0; 1 no
    system solved; 2 nothing free, all held by the caller; 3 nothing free because of bounds; 4 the projected step is no
    descent step); active (q,) codes; projected (q,) bool; raw: the step before the projection (after the clip)."""
    J, r, theta = np.asarray(J, dtype=np.float64), np.asarray(r, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    q = J.shape[1]
    code, _, _ = active_set(J, r, theta, lower, upper, held, row_scale)
    free = np.nonzero(code == FREE)[0]
    out = dict(dscale=np.zeros(q), delta=np.zeros(q), trial=theta.copy(), lam=float(lam), pred=0.0, dxnorm=0.0, gtx=0.0,
               active=code, projected=np.zeros(q, dtype=bool), raw=np.zeros(q))
    if free.size == 0:
        out['status'] = 3 if np.any(code >= AT_LOWER) else 2
        return out
    Js = (J if row_scale is None else J * np.asarray(row_scale)[:, None])[:, free]
    D, x, lam_new, pred, dxnorm, gtx, st = lo.lmpar_reference(Js, r, np.asarray(dscale, dtype=np.float64)[free], float(radius))
    out['dscale'][free] = D
    if st != 0:
        out['status'] = 1
        return out
    changed = False
    if max_step > 0.0:
        clipped = np.clip(x, -max_step, max_step)
        changed = bool(np.any(clipped != x))
        x = clipped
    out['raw'][free] = x
    s = theta[free] + x
    t = np.minimum(np.maximum(s, lower[free]), upper[free])
    proj = t != s
    x = np.where(proj, t - theta[free], x)
    if changed or proj.any():
        pred, dxnorm, gtx = taken_step_quantities(Js, r, D, x)
    if proj.any() and not (gtx < 0.0 and pred > 0.0):
        out['status'] = 4
        return out
    out['delta'][free] = x
    out['trial'][free] = np.where(proj, t, s)
    out['projected'][free] = proj
    out.update(lam=lam_new, pred=pred, dxnorm=dxnorm, gtx=gtx, status=0)
    return out


def bounded_fit(fun, jac, x0, lower, upper, held=None, ftol=lo.FTOL, xtol=lo.XTOL, max_iter=100, factor=100.0):
    """lmder inside the box, serially: bounded_step for the step, lm_update_reference / lm_accept_reference for the
    bookkeeping, status 3 ends the start (done, n_iter = iteration + 1, the radius untouched).  Returns dict(x, cost, n_iter,
    done, trials: every trial point in order, statuses: the step status of every iteration)."""
    x = np.array(x0, dtype=np.float64)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    r, J = np.asarray(fun(x), dtype=np.float64), np.asarray(jac(x), dtype=np.float64)
    cost = 0.5 * float(r @ r)
    col = np.sqrt((J * J).sum(axis=0))
    d0 = np.where(col > 0, col, 1.0)
    if held is not None:
        d0 = np.where(np.asarray(held) != 0, 0.0, d0)
    xn = float(np.linalg.norm(d0 * x))
    D = np.zeros(x.size)
    radius, lam, done, n_iter = (factor * xn if xn > 0 else factor), 0.0, 0, max_iter
    trials, statuses = [], []
    for it in range(max_iter):
        s = bounded_step(J, r, D, radius, lam, x, lower, upper, held)
        D, lam = s['dscale'], s['lam']
        trials.append(s['trial'])
        statuses.append(s['status'])
        if s['status'] == 3:
            done, n_iter = 1, it + 1
            break
        r_t = np.asarray(fun(s['trial']), dtype=np.float64)
        norms_t = float(r_t @ r_t)
        out = lo.lm_update_reference(cost, norms_t, 0 if math.isfinite(norms_t) else 1, s['pred'], s['dxnorm'], s['gtx'], s['status'],
                                     x.copy(), D.copy(), ftol, xtol, it, 1 if it == 0 else 0, radius, lam, done, n_iter)
        radius, lam, done, n_iter = out.radius, out.lam, out.done, out.n_iter
        if out.accept:
            x, r, J, cost = s['trial'], r_t, np.asarray(jac(s['trial']), dtype=np.float64), 0.5 * norms_t
        if done:
            break
    return dict(x=x, cost=cost, n_iter=n_iter, done=done, trials=trials, statuses=statuses)


def problem_bounds(pb, xstar):
    """The box of the bounded tests for one of lmder_oracle.problems(), from its unconstrained optimum x*: the optimum is
    cut off at an upper bound of parameter 1 and a lower bound of parameter 2; on the 12-parameter problem also at an upper
    bound of parameter 7, with a loose interval around parameter 0.  Returns (lower, upper)."""
    lower, upper = np.full(pb.q, -np.inf), np.full(pb.q, np.inf)
    upper[1] = xstar[1] - 0.3 * abs(xstar[1])
    lower[2] = xstar[2] + 0.2 * abs(xstar[2])
    if pb.q == 12:
        upper[7] = xstar[7] - 0.2
        lower[0], upper[0] = xstar[0] - 5.0, xstar[0] + 5.0
    return lower, upper


def unconstrained_optimum(pb):
    """x* of a problem: the best of scipy.optimize.leastsq at ftol = xtol = 1e-14 over its starts"""
    from scipy.optimize import leastsq
    best, best_cost = None, np.inf
    for x0 in pb.starts:
        x = leastsq(pb.fun, x0, Dfun=pb.jac, ftol=1e-14, xtol=1e-14, gtol=0.0, maxfev=5000)[0]
        c = 0.5 * float(pb.fun(x) @ pb.fun(x))
        if c < best_cost:
            best, best_cost = x, c
    return best


def scipy_bounded_baseline(probs):
    """scipy.optimize.least_squares(method='trf', bounds=...) on every (problem, start clipped into its box).  Returns a
    list per problem of dict(lower, upper, starts [8][q], cstar: the lowest cost of the runs at ftol = xtol = gtol = 1e-14,
    at_bound [q] int: -1 / 0 / +1 where that run's solution is within 1e-9 of a bound) and w: scipy's own worst excess
    (cost - c*) / (FTOL c*) at its default tolerances over all starts."""
    from scipy.optimize import least_squares
    half = lambda pb, x: 0.5 * float(pb.fun(x) @ pb.fun(x))          # noqa: E731
    out, w = [], 0.0
    for pb in probs:
        lower, upper = problem_bounds(pb, unconstrained_optimum(pb))
        starts = np.clip(pb.starts, lower, upper)
        tight = [least_squares(pb.fun, x0, jac=pb.jac, bounds=(lower, upper), method='trf', ftol=1e-14, xtol=1e-14, gtol=1e-14,
                               max_nfev=5000).x for x0 in starts]
        costs = [half(pb, x) for x in tight]
        xb = tight[int(np.argmin(costs))]
        cstar = min(costs)
        for x0 in starts:
            xd = least_squares(pb.fun, x0, jac=pb.jac, bounds=(lower, upper), method='trf').x
            w = max(w, (half(pb, xd) - cstar) / (lo.FTOL * cstar))
        at = np.where(np.abs(xb - upper) < 1e-9, 1, 0) - np.where(np.abs(xb - lower) < 1e-9, 1, 0)
        out.append(dict(lower=lower, upper=upper, starts=starts, cstar=cstar, at_bound=at))
    return out, w
