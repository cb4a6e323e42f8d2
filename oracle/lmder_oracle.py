"""MINPACK lmder's bookkeeping between two trust-region steps, one start at a time, in plain float64 Python: the
reference of sbm_lm_update / sbm_lm_accept (include/sbm.h) and of the fitting loop built on them.

Written from lmder.f (the inner loop after the call to lmpar) and from the contract in sbm.h, not from the kernel:

    actred = -1;  if (0.1 fnorm1 < fnorm) actred = 1 - (fnorm1 / fnorm)^2
    prered = (|J p|^2 + 2 par |D p|^2) / fnorm^2,   dirder = -(|J p|^2 + par |D p|^2) / fnorm^2
    ratio  = 0;   if (prered != 0) ratio = actred / prered
    if (ratio <= 1/4)   temp = 1/2 if actred >= 0 else dirder / 2 / (dirder + actred / 2)
                        if (0.1 fnorm1 >= fnorm or temp < 0.1) temp = 0.1
                        delta = temp min(delta, pnorm / 0.1);  par = par / temp
    else if (par == 0 or ratio >= 3/4)  delta = pnorm / 0.5;  par = par / 2
    if (ratio >= 1e-4)  the trial point is taken
    info 1: |actred| <= ftol and prered <= ftol and ratio / 2 <= 1;   info 2: delta <= xtol xnorm

With fnorm^2 = |r|^2 = 2 cost the package's arguments map to these as (sbm.h): fnorm1^2 = norms_trial,
prered = pred / cost, dirder = gtx / (2 cost), pnorm = dxnorm, par = lam, delta = radius.

Where the package departs from lmder, on purpose (sbm.h states each):
  * step status != 0 (lmpar solved no system, something MINPACK's QR cannot report): the radius is halved, lambda and
    the point stay, no convergence test is made and the start stays live.
  * cost == 0: the relative quantities are divided by 1 instead of by cost (lmder would divide by zero).
  * pred <= 0: ratio = 0.  lmder writes `prered .ne. zero`, but its prered is a sum of squares; the package's pred is
    that of a possibly clipped step and can be negative, and actred / prered with both negative would take an uphill step.
  * an unusable trial point (integration status != 0, or a cost that is not finite) counts as actred = -1 and is never
    taken: MINPACK has no notion of a residual function that fails.
  * ||D theta|| of info 2 is taken at the current point, before acceptance; lmder updates xnorm first on a successful
    iteration.
  * n_iter records iteration + 1 (lmder's iter counts from 1) for a start that converges in this call.
"""
import math
from collections import namedtuple

import numpy as np

FTOL = XTOL = 1.49012e-8          # scipy.optimize.leastsq's defaults (sqrt of the machine epsilon)
SWEEP_SEED, SWEEP_Q = 7, 7        # of the random sweep the CPU coverage test and the GPU test share

LmUpdate = namedtuple('LmUpdate', 'radius lam done accept n_iter ratio live accepted branch')

BRANCHES = ('done', 'step_failed', 'shrink_half', 'shrink_parabola', 'shrink_floor', 'ten_x_worse', 'trial_failed', 'grow',
            'keep')
FLAGS = ('conv_f', 'conv_x', 'first_rule')


def labels(branch):
    """The branch label and flags of an LmUpdate.branch ('grow+conv_x+first_rule') as a set."""
    return set(branch.split('+'))


def _close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def _update(cost, norms_trial, status_trial, pred, dxnorm, gtx, step_status, theta, dscale, ftol, xtol, iteration, first,
            radius, lam, done, n_iter, rel):
    """lm_update_reference and, second, whether a comparison that decides a branch is within relative `rel` of equality."""
    if done:
        return LmUpdate(radius, lam, 1, 0, n_iter, None, 0, 0, 'done'), False
    cost, norms_trial, pred, dxnorm, gtx = float(cost), float(norms_trial), float(pred), float(dxnorm), float(gtx)
    radius, lam = float(radius), float(lam)
    cost_t = 0.5 * norms_trial
    usable = status_trial == 0 and math.isfinite(cost_t)
    marginal = False
    flags = []
    if first and step_status == 0:                      # lmder: on the first iteration delta = min(delta, pnorm)
        radius = min(radius, dxnorm)
        flags.append('first_rule')
    scale = cost if cost > 0.0 else 1.0
    ten_x = (not usable) or 0.1 * math.sqrt(cost_t) >= math.sqrt(cost)
    if usable:
        marginal |= _close(0.1 * math.sqrt(cost_t), math.sqrt(cost), rel)
    actred = -1.0 if ten_x else 1.0 - cost_t / scale
    prered = pred / scale
    dirder = gtx / (2.0 * scale)
    ratio = actred / prered if prered > 0.0 else 0.0
    if step_status != 0:
        return LmUpdate(0.5 * radius, lam, 0, 0, n_iter, ratio, 1, 0, 'step_failed'), marginal
    marginal |= any(_close(ratio, t, rel) for t in (0.25, 0.75, 1.0e-4))
    if ratio <= 0.25:
        if not usable:
            temp, name = 0.1, 'trial_failed'
        elif ten_x:
            temp, name = 0.1, 'ten_x_worse'
        elif actred >= 0.0:
            temp, name = 0.5, 'shrink_half'
        else:
            # both terms of the denominator are negative: it cannot cancel, and temp is in (0, 1/2]
            assert dirder <= 0.0 and actred < 0.0, (dirder, actred)
            temp = 0.5 * dirder / (dirder + 0.5 * actred)
            marginal |= _close(temp, 0.1, rel)
            name = 'shrink_parabola'
            if temp < 0.1:
                temp, name = 0.1, 'shrink_floor'
        radius = temp * min(radius, dxnorm / 0.1)
        lam = lam / temp
    elif lam == 0.0 or ratio >= 0.75:
        radius = dxnorm / 0.5
        lam = 0.5 * lam
        name = 'grow'
    else:
        name = 'keep'
    accept = 1 if (ratio >= 1.0e-4 and usable) else 0
    xnorm = math.sqrt(sum((float(d) * float(t)) ** 2 for d, t in zip(dscale, theta)))
    conv_f = abs(actred) <= ftol and prered <= ftol and 0.5 * ratio <= 1.0
    conv_x = radius <= xtol * xnorm
    marginal |= _close(abs(actred), ftol, rel) or _close(prered, ftol, rel) or _close(0.5 * ratio, 1.0, rel)
    marginal |= _close(radius, xtol * xnorm, rel)
    if conv_f:
        flags.insert(0, 'conv_f')
    if conv_x:
        flags.insert(1 if conv_f else 0, 'conv_x')
    conv = conv_f or conv_x
    return LmUpdate(radius, lam, 1 if conv else 0, accept, iteration + 1 if conv else n_iter, ratio, 0 if conv else 1, accept,
                    '+'.join([name] + flags)), marginal


def lm_update_reference(cost, norms_trial, status_trial, pred, dxnorm, gtx, step_status, theta, dscale, ftol, xtol, iteration,
                        first, radius, lam, done, n_iter):
    """One start through lmder's bookkeeping.  Returns LmUpdate(radius, lam, done, accept, n_iter, ratio, live, accepted,
    branch): the updated state, the ratio of actual to predicted reduction (None for a start that was already done: the
    package leaves it untouched), this start's contribution to the two counters, and the label of the path taken."""
    return _update(cost, norms_trial, status_trial, pred, dxnorm, gtx, step_status, theta, dscale, ftol, xtol, iteration, first,
                   radius, lam, done, n_iter, 0.0)[0]


def lm_update_is_marginal(cost, norms_trial, status_trial, pred, dxnorm, gtx, step_status, theta, dscale, ftol, xtol, iteration,
                          first, radius, lam, done, n_iter, rel=1.0e-9):
    """True where one of the comparisons (ratio with 1/4, 3/4, 1e-4; temp with 1/10; the ten-times-worse test; the ftol and
    xtol tests) is within relative `rel` of equality: there an implementation that contracts a * b + c into an fma may
    decide the other way, and only the floating-point outputs can be demanded of it."""
    return _update(cost, norms_trial, status_trial, pred, dxnorm, gtx, step_status, theta, dscale, ftol, xtol, iteration, first,
                   radius, lam, done, n_iter, rel)[1]


def lm_accept_reference(accept, trial, r_trial, J_trial, norms_trial, theta, r, J, cost):
    """Rows with accept != 0 take the trial point's theta, residuals, Jacobian and cost = 0.5 norms_trial; the others stay.
    Arrays with a leading dimension V; returns new (theta, r, J, cost)."""
    theta, r, J, cost = (np.array(x, dtype=np.float64, copy=True) for x in (theta, r, J, cost))
    for v in range(len(accept)):
        if accept[v]:
            theta[v] = trial[v]
            r[v] = r_trial[v]
            J[v] = J_trial[v]
            cost[v] = 0.5 * norms_trial[v]
    return theta, r, J, cost


# ----------------------------------------------------------------------------------------------------------------------
# a complete serial lmder loop on the two functions above
# ----------------------------------------------------------------------------------------------------------------------
def lmpar_reference(J, r, dscale, radius):
    """A plain lmpar: D = max(D, column norms of J) (1 for a zero column), lam = 0 where the Gauss-Newton step is inside
    1.1 radius, else lam by bisection on ||D p(lam)|| = radius to the 10 % MINPACK accepts.  Returns D, p, lam, pred, dxnorm,
    gtx, status in the package's terms (pred = |J p|^2 / 2 + lam |D p|^2, gtx = g . p)."""
    q = J.shape[1]
    col = np.sqrt((J * J).sum(axis=0))
    D = np.maximum(dscale, col)
    D[D == 0.0] = 1.0
    if not (np.all(np.isfinite(J)) and np.all(np.isfinite(r))):
        return D, np.zeros(q), 0.0, 0.0, 0.0, 0.0, 1

    def step(lam):
        A = np.vstack([J, math.sqrt(lam) * np.diag(D)])
        b = np.concatenate([-r, np.zeros(q)])
        return np.linalg.lstsq(A, b, rcond=None)[0]

    p, lam = step(0.0), 0.0
    if np.linalg.norm(D * p) > 1.1 * radius:
        g = J.T @ r
        lo, hi = 0.0, np.linalg.norm(g / D) / radius          # ||D p(hi)|| <= ||D^-1 g|| / hi = radius
        for _ in range(200):
            lam = 0.5 * (lo + hi)
            p = step(lam)
            phi = np.linalg.norm(D * p) - radius
            if abs(phi) <= 0.1 * radius:
                break
            lo, hi = (lam, hi) if phi > 0 else (lo, lam)
    Jp, dxnorm = J @ p, float(np.linalg.norm(D * p))
    return D, p, lam, 0.5 * float(Jp @ Jp) + lam * dxnorm ** 2, dxnorm, float((J.T @ r) @ p), 0


def fit_reference(fun, jac, x0, ftol=FTOL, xtol=XTOL, max_iter=200, factor=100.0):
    """lmder, serially: lmpar_reference for the step, lm_update_reference / lm_accept_reference for everything else.
    Returns dict(x, cost, n_iter, done, trace); trace holds per iteration the arguments lm_update_reference was called with
    and what it returned."""
    x = np.array(x0, dtype=np.float64)
    r, J = np.asarray(fun(x), dtype=np.float64), np.asarray(jac(x), dtype=np.float64)
    cost = 0.5 * float(r @ r)
    D = np.zeros(x.size)
    col = np.sqrt((J * J).sum(axis=0))
    xn = float(np.linalg.norm(np.where(col > 0, col, 1.0) * x))
    radius, lam, done, n_iter = (factor * xn if xn > 0 else factor), 0.0, 0, max_iter
    trace = []
    for it in range(max_iter):
        D, p, lam, pred, dxnorm, gtx, st = lmpar_reference(J, r, D, radius)
        trial = x + p
        r_t = np.asarray(fun(trial), dtype=np.float64)
        norms_t = float(r_t @ r_t)
        status_t = 0 if math.isfinite(norms_t) else 1
        args = (cost, norms_t, status_t, pred, dxnorm, gtx, st, x.copy(), D.copy(), ftol, xtol, it, 1 if it == 0 else 0, radius,
                lam, done, n_iter)
        out = lm_update_reference(*args)
        trace.append((args, out))
        radius, lam, done, n_iter = out.radius, out.lam, out.done, out.n_iter
        if out.accept:
            J_t = np.asarray(jac(trial), dtype=np.float64)
            xs, rs, Js, cs = lm_accept_reference([1], [trial], [r_t], [J_t], [norms_t], [x], [r], [J], [cost])
            x, r, J, cost = xs[0], rs[0], Js[0], float(cs[0])
        if done:
            break
    return dict(x=x, cost=cost, n_iter=n_iter, done=done, trace=trace)


# ----------------------------------------------------------------------------------------------------------------------
# inputs: the random sweep of the update rule, the named cases, three small least-squares problems
# ----------------------------------------------------------------------------------------------------------------------
UPDATE_FIELDS = ('cost', 'norms_trial', 'status_trial', 'pred', 'dxnorm', 'gtx', 'step_status', 'theta', 'dscale', 'radius',
                 'lam', 'done', 'n_iter')


def draw_update_inputs(n, q, seed, xtol=XTOL):
    """n input sets of the update rule as a dict of arrays, log-uniform over many decades and arranged so that every branch
    is populated: zero costs, trial points from a thousand times better to a thousand times worse, just better, unusable;
    predictions tied to the actual reduction so that the ratio covers (0, 1e-4), 1/4 and 3/4; zero lambda; radii at the
    xtol test; starts already done."""
    rng = np.random.default_rng(seed)
    lu = lambda lo, hi, size=n: 10.0 ** rng.uniform(lo, hi, size)          # noqa: E731
    cost = lu(-12, 6)
    cost[rng.random(n) < 0.02] = 0.0
    kind = rng.random(n)
    f = lu(-3, 3)                                                          # trial |r|^2 over current |r|^2
    f = np.where(kind < 0.25, 1.0 - lu(-14, -1), f)                        # just under: tiny positive actred
    f = np.where((kind >= 0.25) & (kind < 0.40), 1.0 + lu(-6, 0.5), f)     # worse, less than tenfold: the parabola
    base = np.where(cost > 0, cost, lu(-6, 2))
    norms_trial = 2.0 * base * f
    special = rng.random(n)
    norms_trial[special < 0.01] = np.nan
    norms_trial[(special >= 0.01) & (special < 0.02)] = np.inf
    norms_trial[(special >= 0.02) & (special < 0.03)] = 1.0e301
    status_trial = np.where(rng.random(n) < 0.05, rng.integers(1, 4, n), 0).astype(np.int32)
    actred = np.abs(1.0 - f)
    mult = np.where(rng.random(n) < 0.85, lu(-1.5, 1.5), lu(1.5, 8))        # prered over |actred|
    pred = base * np.maximum(actred, 1.0e-300) * mult
    sign = rng.random(n)
    pred[sign < 0.02] = 0.0
    pred = np.where((sign >= 0.02) & (sign < 0.04), -pred, pred)
    gtx = -np.abs(pred) * rng.uniform(1.0, 2.0, n)                          # -g.p lies between pred and 2 pred
    gtx[rng.random(n) < 0.02] = 0.0
    step_status = (rng.random(n) < 0.08).astype(np.int32)
    theta = rng.standard_normal((n, q)) * lu(-2, 2, (n, 1))
    dscale = lu(-2, 2, (n, q))
    radius = lu(-6, 3)
    xnorm = np.sqrt(((dscale * theta) ** 2).sum(axis=1))
    at_xtol = rng.random(n) < 0.06
    radius = np.where(at_xtol, xtol * xnorm * lu(-3, -1), radius)
    dxnorm = radius * np.where(rng.random(n) < 0.8, lu(-1, 0.04), lu(0, 2))
    lam = np.where(rng.random(n) < 1.0 / 3.0, 0.0, lu(-8, 4))
    done = (rng.random(n) < 0.1).astype(np.int32)
    n_iter = np.full(n, 200, dtype=np.int32)
    return dict(cost=cost, norms_trial=norms_trial, status_trial=status_trial, pred=pred, dxnorm=dxnorm, gtx=gtx,
                step_status=step_status, theta=theta, dscale=dscale, radius=radius, lam=lam, done=done, n_iter=n_iter)


def update_args(d, v, ftol, xtol, iteration, first):
    """The argument tuple of lm_update_reference for row v of a dict of arrays (draw_update_inputs, named_cases)."""
    return (d['cost'][v], d['norms_trial'][v], int(d['status_trial'][v]), d['pred'][v], d['dxnorm'][v], d['gtx'][v],
            int(d['step_status'][v]), d['theta'][v], d['dscale'][v], ftol, xtol, iteration, first, d['radius'][v], d['lam'][v],
            int(d['done'][v]), int(d['n_iter'][v]))


# The named cases: one per branch label, q = 2, theta = (3, 4), D = (1, 1) so ||D theta|| = 5; ftol = xtol = 1e-8, iteration 6.
# Every number is a small binary fraction or is worked with the operations the rule itself uses, so that the expected
# values below are exact.  Only the two cases marked `first` have a step shorter than the radius, so the whole set gives the
# same numbers when it is run as ONE call with first = 1 (the device entry point takes `first` per call).  Columns: cost, norms_trial, status_trial, pred, dxnorm, gtx, step_status, radius, lam, done, first.
NAMED_FTOL = NAMED_XTOL = 1.0e-8
NAMED_ITERATION = 6
NAMED_N_ITER = 99
NAMED_CASES = (
    # done: nothing moves, the trial point is not taken
    ('done', (2.0, 1.0, 0, 1.0, 1.0, -1.5, 0, 8.0, 0.5, 1, 0),
     dict(radius=8.0, lam=0.5, done=1, accept=0, n_iter=99, ratio=None, live=0, accepted=0)),
    # step_failed: radius 8 -> 4, lambda kept, still live; ratio is still reported: actred = 1 - 0.5 / 2 = 0.75,
    # prered = 1 / 2 -> 1.5
    ('step_failed', (2.0, 1.0, 0, 1.0, 1.0, -1.5, 1, 8.0, 0.5, 0, 0),
     dict(radius=4.0, lam=0.5, done=0, accept=0, n_iter=99, ratio=1.5, live=1, accepted=0)),
    # shrink_half: cost 2 -> 1.75: actred = 1 - 1.75 / 2 = 0.125, prered = 2 / 2 = 1, ratio 0.125 <= 1/4, actred >= 0:
    # temp = 1/2, radius = 0.5 min(8, 16 / 0.1) = 4, lam = 0.5 / 0.5 = 1; ratio >= 1e-4: taken
    ('shrink_half', (2.0, 3.5, 0, 2.0, 16.0, -3.0, 0, 8.0, 0.5, 0, 0),
     dict(radius=4.0, lam=1.0, done=0, accept=1, n_iter=99, ratio=0.125, live=1, accepted=1)),
    # shrink_parabola: cost 2 -> 3: actred = 1 - 3 / 2 = -0.5, prered = 1, ratio = -0.5, dirder = -3 / 4 = -0.75,
    # temp = 0.5 (-0.75) / (-0.75 - 0.25) = 0.375, radius = 0.375 min(8, 160) = 3, lam = 0.75 / 0.375 = 2; not taken
    ('shrink_parabola', (2.0, 6.0, 0, 2.0, 16.0, -3.0, 0, 8.0, 0.75, 0, 0),
     dict(radius=3.0, lam=2.0, done=0, accept=0, n_iter=99, ratio=-0.5, live=1, accepted=0)),
    # shrink_floor: cost 2 -> 18 (3 times the norm: not ten times worse): actred = 1 - 9 = -8, prered = 1, ratio = -8,
    # dirder = -0.75, temp = 0.5 (-0.75) / (-0.75 - 4) = 0.0789 < 0.1 -> 0.1, radius = 0.1 min(0.25, 0.5 / 0.1) = 0.1 * 0.25,
    # lam = 0.75 / 0.1
    ('shrink_floor', (2.0, 36.0, 0, 2.0, 0.5, -3.0, 0, 0.25, 0.75, 0, 0),
     dict(radius=0.1 * 0.25, lam=0.75 / 0.1, done=0, accept=0, n_iter=99, ratio=-8.0, live=1, accepted=0)),
    # ten_x_worse: cost 2 -> 800 (twenty times the norm): actred = -1, prered = 1, ratio = -1, temp = 0.1,
    # radius = 0.1 min(8, 16 / 0.1) = 0.1 * 8, lam = 0.75 / 0.1; the parabola (0.5 (-0.75) / (-0.75 - 0.5) = 0.3) is not used
    ('ten_x_worse', (2.0, 1600.0, 0, 2.0, 16.0, -3.0, 0, 8.0, 0.75, 0, 0),
     dict(radius=0.1 * 8.0, lam=0.75 / 0.1, done=0, accept=0, n_iter=99, ratio=-1.0, live=1, accepted=0)),
    # trial_failed: a trial point that would have been a fine step (cost 2 -> 0.5) but whose integration failed:
    # actred = -1, prered = 0.5, ratio = -2, temp = 0.1, radius = 0.1 min(8, 160) = 0.1 * 8, lam = 0.75 / 0.1; not taken
    ('trial_failed', (2.0, 1.0, 3, 1.0, 16.0, -1.5, 0, 8.0, 0.75, 0, 0),
     dict(radius=0.1 * 8.0, lam=0.75 / 0.1, done=0, accept=0, n_iter=99, ratio=-2.0, live=1, accepted=0)),
    # grow, and the first-iteration rule: cost 2 -> 0.5: actred = 0.75, prered = 0.5, ratio = 1.5 >= 3/4:
    # radius = 1 / 0.5 = 2 (first: min(8, 1) = 1 before, which the grow branch overwrites), lam = 0.25; taken
    ('grow', (2.0, 1.0, 0, 1.0, 1.0, -1.5, 0, 8.0, 0.5, 0, 1),
     dict(radius=2.0, lam=0.25, done=0, accept=1, n_iter=99, ratio=1.5, live=1, accepted=1, flags=('first_rule',))),
    # keep, under the first-iteration rule: cost 2 -> 1: actred = 0.5, prered = 1, ratio = 0.5 in (1/4, 3/4), lam != 0:
    # lambda kept, radius = min(8, 1) = 1 from the first rule alone; taken
    ('keep', (2.0, 2.0, 0, 2.0, 1.0, -3.0, 0, 8.0, 0.5, 0, 1),
     dict(radius=1.0, lam=0.5, done=0, accept=1, n_iter=99, ratio=0.5, live=1, accepted=1, flags=('first_rule',))),
    # grow through lam == 0 with both convergence tests: cost 2 -> 2 (1 - 2^-30): actred = 2^-30 = 9.3e-10 <= ftol,
    # prered = 2^-29 = 1.9e-9 <= ftol, ratio = 0.5 with lam == 0: radius = 2 * 2^-26 = 2^-25 = 3.0e-8 <= xtol * 5 = 5e-8,
    # lam = 0; taken, done, n_iter = 6 + 1
    ('grow', (2.0, 4.0 * (1.0 - 2.0 ** -30), 0, 2.0 ** -28, 2.0 ** -26, -(2.0 ** -28), 0, 8.0, 0.0, 0, 0),
     dict(radius=2.0 ** -25, lam=0.0, done=1, accept=1, n_iter=7, ratio=0.5, live=0, accepted=1, flags=('conv_f', 'conv_x'))),
)


def named_cases():
    """NAMED_CASES as the dict of arrays the sweep uses (V = 10, q = 2), and the list of (label, expected) beside it."""
    rows = [c[1] for c in NAMED_CASES]
    col = lambda i, dt=np.float64: np.array([r[i] for r in rows], dtype=dt)          # noqa: E731
    V = len(rows)
    d = dict(cost=col(0), norms_trial=col(1), status_trial=col(2, np.int32), pred=col(3), dxnorm=col(4), gtx=col(5),
             step_status=col(6, np.int32), radius=col(7), lam=col(8), done=col(9, np.int32),
             theta=np.tile([3.0, 4.0], (V, 1)), dscale=np.ones((V, 2)), n_iter=np.full(V, NAMED_N_ITER, dtype=np.int32))
    return d, [r[10] for r in rows], [(c[0], c[2]) for c in NAMED_CASES]


class Problem:
    """A small least-squares problem whose residuals and Jacobian are written once for numpy and torch: X is [V][q]."""

    def __init__(self, name, q, M, consts, residuals, jacobian, starts):
        self.name, self.q, self.M, self.consts, self._r, self._J, self.starts = name, q, M, consts, residuals, jacobian, starts

    def to(self, device):
        import torch
        return Problem(self.name, self.q, self.M, {k: torch.from_numpy(v).to(device) for k, v in self.consts.items()}, self._r,
                       self._J, self.starts)

    def residuals(self, X):
        return self._r(self.consts, X)

    def jacobian(self, X):
        return self._J(self.consts, X)

    def fun(self, x):
        return self.residuals(np.asarray(x, dtype=np.float64)[None])[0]

    def jac(self, x):
        return self.jacobian(np.asarray(x, dtype=np.float64)[None])[0]


def _xp(X):
    if isinstance(X, np.ndarray):
        return np.exp, lambda cols: np.stack(cols, axis=-1), np.ones_like
    import torch
    return torch.exp, lambda cols: torch.stack(cols, dim=-1), torch.ones_like


def _decay_r(c, X):
    exp = _xp(X)[0]
    a, b, o = X[:, 0:1], X[:, 1:2], X[:, 2:3]
    return a * exp(-b * c['t'][None]) + o - c['y'][None]


def _decay_J(c, X):
    exp, stack, ones = _xp(X)
    a, b = X[:, 0:1], X[:, 1:2]
    e = exp(-b * c['t'][None])
    return stack([e, -a * c['t'][None] * e, ones(e)])


def _decay4_r(c, X):
    # the offset is split over two nearly collinear columns: 1 and 1 + 1e-3 t
    return _decay_r(c, X) + X[:, 3:4] * c['g'][None]


def _decay4_J(c, X):
    exp, stack, ones = _xp(X)
    a, b = X[:, 0:1], X[:, 1:2]
    e = exp(-b * c['t'][None])
    return stack([e, -a * c['t'][None] * e, ones(e), ones(e) * c['g'][None]])


def _quad_r(c, X):
    Bx = X @ c['B'].T
    return X @ c['A'].T + 0.1 * Bx * Bx - c['b'][None]


def _quad_J(c, X):
    Bx = X @ c['B'].T
    return c['A'][None] + 0.2 * Bx[:, :, None] * c['B'][None]


def problems():
    """The three nonzero-residual problems, each with eight starts (fixed seeds)."""
    rng = np.random.default_rng(20240611)
    t = np.linspace(0.0, 4.0, 20)
    y = 2.5 * np.exp(-1.3 * t) + 0.5 + 0.05 * rng.standard_normal(20)
    s3 = np.array([2.5, 1.3, 0.5]) * np.exp(rng.uniform(-0.7, 0.7, (8, 3)))
    s4 = np.concatenate([s3 * np.array([1.0, 1.0, 0.5]), 0.5 * s3[:, 2:3]], axis=1)
    A = rng.standard_normal((30, 12))
    B = rng.standard_normal((30, 12)) / math.sqrt(12.0)
    b = A @ rng.standard_normal(12) + 0.3 * rng.standard_normal(30)
    s12 = 0.5 * rng.standard_normal((8, 12))
    return [Problem('decay', 3, 20, dict(t=t, y=y), _decay_r, _decay_J, s3),
            Problem('decay_collinear', 4, 20, dict(t=t, y=y, g=1.0 + 1.0e-3 * t), _decay4_r, _decay4_J, s4),
            Problem('quadratic', 12, 30, dict(A=A, B=B, b=b), _quad_r, _quad_J, s12)]


def minpack_baseline(probs=None, ftol=FTOL):
    """scipy.optimize.leastsq = MINPACK lmder on the problems.  Per problem c* is the lowest cost any start reaches at
    ftol = xtol = 1e-14; a start whose own tight solution is another minimum is dropped.  Returns (cstar [P], keep [P][8],
    worst): worst is MINPACK's own largest excess (cost - c*) / (ftol c*) at DEFAULT tolerances over the starts kept."""
    from scipy.optimize import leastsq
    probs = probs or problems()
    cstar, keep, worst = [], [], 0.0
    half = lambda pb, x: 0.5 * float(pb.fun(x) @ pb.fun(x))          # noqa: E731
    for pb in probs:
        tight = [leastsq(pb.fun, x0, Dfun=pb.jac, ftol=1e-14, xtol=1e-14, gtol=0.0, maxfev=5000)[0] for x0 in pb.starts]
        costs = [half(pb, x) for x in tight]
        best = tight[int(np.argmin(costs))]
        c = min(costs)
        kp = [bool(np.linalg.norm(x - best) <= 1e-6 * (1.0 + np.linalg.norm(best))) for x in tight]
        for x0, k in zip(pb.starts, kp):
            if k:
                worst = max(worst, (half(pb, leastsq(pb.fun, x0, Dfun=pb.jac)[0]) - c) / (ftol * c))
        cstar.append(c)
        keep.append(kp)
    return np.array(cstar), np.array(keep), worst
