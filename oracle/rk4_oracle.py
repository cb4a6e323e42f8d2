"""ORACLE (test infrastructure, not product code) -- classic fixed-step RK4 of the augmented system [y; S] in plain float64.

The fixed-step method of the GPU kernels (SBM_RK4_FIXED) evaluates one scheme whatever the lane layout: against this
restatement a kernel may differ in rounding only, so the comparison is at the rounding level of the problem instead of an
integration tolerance.  The step partition is the contract of include/sbm.h (sbm_integrator_opts.h0 / .step_mult): every
output interval is cut into step_mult * ceil(dt / h0) equal steps.  Nothing here is taken from the kernels.

The right-hand side is the oracle's compiled C one (gm.c_library().sbm_sens_rhs, ``use_c=True``) or the generated Python
callable (gm.sens_model): the same expressions evaluated by two compilers.  Their difference, relative to each column's
largest entry over the output times (``colmax_err``), is the rounding level rho of a problem.

PINNED: tests/test_tile_edge_layouts_cpu.py (fourth-order convergence to odeint_oracle.tight_solution, C against Python)."""
from __future__ import annotations

import math

import numpy as np

from .odeint_oracle import _wrap, _wrap_c


def steps_per_interval(t_out, h0, step_mult=0):
    """The partition of include/sbm.h: step_mult * ceil(dt / h0) equal steps for every output interval (step_mult 0 = 1)."""
    t_out = np.asarray(t_out, dtype=float)
    if not h0 > 0.0:
        raise ValueError("h0 must be positive")
    return [max(1, int(step_mult) if step_mult else 1) * max(1, int(math.ceil(dt / h0))) for dt in np.diff(t_out)]


def integrate(gm, params, t_out, h0, step_mult=0, init_conditions=None, use_c=True):
    """(len(t_out), n + n k): [y; S] at the output times, t_out[0] the time of the initial condition (zeros by default),
    S in the layout of calc_jacobian (column i * k + j = d y_i / d p_j)."""
    n, k = gm.n_vars, gm.n_sens
    N = n + n * k
    fw = _wrap_c(gm.c_library().sbm_sens_rhs, N, params) if use_c else _wrap(gm.sens_model, N, params)
    t_out = np.asarray(t_out, dtype=float)
    z = np.zeros(N) if init_conditions is None else np.array(init_conditions, dtype=float)
    out = [z.copy()]
    for a, dt, ns in zip(t_out[:-1], np.diff(t_out), steps_per_interval(t_out, h0, step_mult)):
        if dt > 0.0:
            h = dt / ns
            for s in range(ns):
                t = a + s * h
                k1 = fw(z, t).copy()
                k2 = fw(z + 0.5 * h * k1, t + 0.5 * h).copy()
                k3 = fw(z + 0.5 * h * k2, t + 0.5 * h).copy()
                k4 = fw(z + h * k3, t + h).copy()
                z = z + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        out.append(z.copy())
    return np.array(out)


def colmax_err(a, ref, n, k):
    """max |a - ref| entry by entry, each relative to the largest |ref| of its column over all output times and rows (a
    sensitivity column j: the entries n + i k + j; the state: one column).  A column that is zero throughout must match
    exactly (inf otherwise).  A NaN or inf anywhere in ``a`` -- state, sensitivity, a zero column -- gives inf, and so does
    one in ``ref``: nothing that is not a finite number is ever within a bound."""
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    if a.shape != ref.shape or a.ndim != 2 or a.shape[1] != n + n * k:
        raise ValueError("colmax_err: shapes %s and %s, expected (times, %d)" % (a.shape, ref.shape, n + n * k))
    if not (np.isfinite(a).all() and np.isfinite(ref).all()):
        return float('inf')
    ey = np.abs(a[:, :n] - ref[:, :n])
    es = np.abs(a[:, n:] - ref[:, n:]).reshape(-1, n, k)
    sy = np.abs(ref[:, :n]).max()
    ss = np.abs(ref[:, n:]).reshape(-1, n, k).max(axis=(0, 1))
    with np.errstate(divide='ignore', invalid='ignore'):
        ry = np.where(ey == 0.0, 0.0, ey / sy)
        rs = np.where(es == 0.0, 0.0, es / ss[None, None, :])
    # all entries are finite here; a non-zero error over a zero scale is inf, and np.max (unlike the builtin) keeps a NaN
    worst = float(np.max(np.concatenate([ry.ravel(), rs.ravel()])))
    return worst if worst == worst else float('inf')
