"""The geodesic acceleration of a Levenberg-Marquardt step (Transtrum and Sethna, "Improvements to the Levenberg-Marquardt
algorithm", 2012) as sbm_lm_geodesic is specified in include/sbm.h, one start at a time, in numpy with the linear algebra in
np.longdouble: the reference of the kernel and of the fitting loop with ``geodesic=``.  Written from the contract, not from
the kernel.

    r_vv = (2 / h) ((r_probe - r_base) / h - J~ v),        J~ = diag(row_scale) J
    (J~^T J~ + lam D^2) a = -J~^T r_vv                     (Cholesky)
    rho  = 2 ||D a|| / ||D v||;   applied iff ||D a|| > 0 and rho <= alpha
    x    = clip(v + a / 2, +-max_step);   dxnorm = ||D x||, gtx = g . x, pred = -gtx - x^T J~^T J~ x / 2
    not applied either if not (gtx < 0 and pred > 0)
"""
import math
from collections import namedtuple

import numpy as np

from oracle import lmder_oracle as lo

LD = np.longdouble
H, ALPHA = 0.1, 0.75          # the paper's defaults, and fit_batch's

APPLIED, NO_STEP, PROBE, SYSTEM, GATE, NO_DESCENT = range(6)

Accel = namedtuple('Accel', 'x status rho pred dxnorm gtx a')


def scaled_jacobian(J, row_scale=None):
    J = np.asarray(J, dtype=LD)
    return J if row_scale is None else np.asarray(row_scale, dtype=LD)[:, None] * J


def rvv_reference(J, r_base, r_probe, v, h, row_scale=None):
    """The second directional derivative of the residuals along v from the two ends of the probe, (M,) longdouble"""
    h = LD(h)
    Jv = scaled_jacobian(J, row_scale) @ np.asarray(v, dtype=LD)
    return (LD(2) / h) * ((np.asarray(r_probe, dtype=LD) - np.asarray(r_base, dtype=LD)) / h - Jv)


def cholesky_solve(A, b):
    """x with A x = b for a symmetric positive definite A (longdouble; numpy's LAPACK routines stop at double); None where a
    pivot is not positive."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for k in range(n):
        piv = A[k, k] - L[k, :k] @ L[k, :k]
        if not piv > 0 or not np.isfinite(piv):
            return None
        L[k, k] = np.sqrt(piv)
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def accel_reference(J, r, r_base, r_probe, D, lam, v, h, alpha, max_step, held=None, row_scale=None):
    """Items 2 - 6 of the algorithm for one start: J (M, q), r (M,), D and v (q,) as the trust step left them.  Returns
    Accel(x, status, rho, pred, dxnorm, gtx, a): x (q,) float64 is the step to take -- v itself wherever status != 0, with
    pred = dxnorm = gtx = None (the caller keeps the trust step's) --, rho NaN where it was not computed, a the acceleration
    (q,) longdouble (zero on held columns; None where no system was solved).  ``held`` (q,) bool: the system is that of the
    free columns."""
    q = len(v)
    v64 = np.array(v, dtype=np.float64)
    free = np.ones(q, dtype=bool) if held is None else ~np.asarray(held, dtype=bool)
    none = lambda status, rho=math.nan, a=None: Accel(v64, status, rho, None, None, None, a)          # noqa: E731
    if not free.any():
        return none(NO_STEP)
    r_base = r if r_base is None else r_base
    if not (np.all(np.isfinite(np.asarray(r_base, dtype=np.float64))) and np.all(np.isfinite(np.asarray(r_probe, dtype=np.float64)))):
        return none(PROBE)
    Jf = np.asarray(J, dtype=np.float64)[:, free]
    if not (np.all(np.isfinite(Jf)) and np.all(np.isfinite(np.asarray(r, dtype=np.float64))) and lam >= 0):
        return none(SYSTEM)
    Js = scaled_jacobian(Jf, row_scale)
    Df, vf = np.asarray(D, dtype=LD)[free], np.asarray(v, dtype=LD)[free]
    rvv = rvv_reference(Jf, r_base, r_probe, vf, h, row_scale)
    Hm = Js.T @ Js
    A = Hm + LD(lam) * np.diag(Df * Df)
    af = cholesky_solve(A, -(Js.T @ rvv))
    if af is None:
        return none(SYSTEM)
    a = np.zeros(q, dtype=LD)
    a[free] = af
    dan, dvn = np.sqrt(np.sum((Df * af) ** 2)), np.sqrt(np.sum((Df * vf) ** 2))
    with np.errstate(divide='ignore', invalid='ignore'):
        rho = float(LD(2) * dan / dvn)
    if not dan > 0 or not rho <= alpha:
        return none(GATE, rho, a)
    xf = vf + af / 2
    if max_step > 0:
        xf = np.clip(xf, -LD(max_step), LD(max_step))
    g = Js.T @ np.asarray(r, dtype=LD)
    gtx = g @ xf
    pred = -gtx - (xf @ (Hm @ xf)) / 2
    if not (gtx < 0 and pred > 0):
        return none(NO_DESCENT, rho, a)
    x = v64.copy()
    x[free] = xf.astype(np.float64)
    return Accel(x, APPLIED, rho, float(pred), float(np.sqrt(np.sum((Df * xf) ** 2))), float(gtx), a)


def geodesic_fit_reference(fun, jac, x0, h=H, alpha=ALPHA, ftol=lo.FTOL, xtol=lo.XTOL, max_iter=200, factor=100.0, lmpar=None):
    """``lo.fit_reference`` with the probe and `accel_reference` between lmpar and the trial point: r is evaluated once more
    at x + h p, and where the acceleration is applied the trial point, pred, dxnorm and gtx are those of p + a / 2.
    ``lmpar(J, r, D, radius, iteration)``: the trust step, ``lo.lmpar_reference`` by default.  Returns fit_reference's dict
    with 'n_accel', and per iteration 'accel_status' and 'rho'."""
    x = np.array(x0, dtype=np.float64)
    r, J = np.asarray(fun(x), dtype=np.float64), np.asarray(jac(x), dtype=np.float64)
    cost = 0.5 * float(r @ r)
    D = np.zeros(x.size)
    col = np.sqrt((J * J).sum(axis=0))
    xn = float(np.linalg.norm(np.where(col > 0, col, 1.0) * x))
    radius, lam, done, n_iter = (factor * xn if xn > 0 else factor), 0.0, 0, max_iter
    trace, statuses, rhos, n_accel = [], [], [], 0
    for it in range(max_iter):
        if lmpar is None:
            D, p, lam, pred, dxnorm, gtx, st = lo.lmpar_reference(J, r, D, radius)
        else:
            D, p, lam, pred, dxnorm, gtx, st = lmpar(J, r, D, radius, it)
        status, rho = NO_STEP, math.nan
        if st == 0:
            r_probe = np.asarray(fun(x + h * p), dtype=np.float64)
            acc = accel_reference(J, r, r, r_probe, D, lam, p, h, alpha, 0.0)
            status, rho = acc.status, acc.rho
            if status == APPLIED:
                p, pred, dxnorm, gtx = acc.x, acc.pred, acc.dxnorm, acc.gtx
                n_accel += 1
        statuses.append(status)
        rhos.append(rho)
        trial = x + p
        r_t = np.asarray(fun(trial), dtype=np.float64)
        norms_t = float(r_t @ r_t)
        status_t = 0 if math.isfinite(norms_t) else 1
        args = (cost, norms_t, status_t, pred, dxnorm, gtx, st, x.copy(), D.copy(), ftol, xtol, it, 1 if it == 0 else 0, radius,
                lam, done, n_iter)
        out = lo.lm_update_reference(*args)
        trace.append((args, out))
        radius, lam, done, n_iter = out.radius, out.lam, out.done, out.n_iter
        if out.accept:
            J_t = np.asarray(jac(trial), dtype=np.float64)
            xs, rs, Js, cs = lo.lm_accept_reference([1], [trial], [r_t], [J_t], [norms_t], [x], [r], [J], [cost])
            x, r, J, cost = xs[0], rs[0], Js[0], float(cs[0])
        if done:
            break
    return dict(x=x, cost=cost, n_iter=n_iter, done=done, trace=trace, n_accel=n_accel, accel_status=statuses, rho=rhos)
