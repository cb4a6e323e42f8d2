"""Batched multi-start Levenberg-Marquardt on top of the device evaluator.

The reference fits one start at a time: ``scipy.optimize.leastsq(project.residuals, x0,
Dfun=project.calc_project_jacobian)`` (tests/test_Project.py:202-213, :352-357) -- every function and
Jacobian evaluation a serial LSODA run per experiment.  Here V starts advance together: one
``sbm_jacobian_batch`` call integrates all trial points (residuals AND Jacobians from the same augmented
integration), one ``sbm_lm_step`` call solves the V damped normal equations on the device, and the
accept / reject bookkeeping is a handful of tensor selects.  Nothing leaves the GPU inside the loop except
a convergence count per iteration.
"""
from __future__ import annotations


import numpy as np

from .. import _lib
from ._evaluation import (DeviceEvaluator, finite_cost, geodesic_step, inverse_row_sigma, one_device_call, trust_step,
                          usable)


def _trial_budget(project, th, integrator_overrides, n_steps_sum=None, status=None):
    """Step budget of the TRIAL integrations when the caller named none: three times what the slowest TRAJECTORY of the
    starting points needs (at least 300 attempts: DOP853 takes ~170 steps where DOPRI45 takes ~1000, and a floor of 2000 let its
    stiff trial points run twelve times the typical trajectory), with the early exit (negative ``max_steps``, include/sbm.h).  One
    launch lasts as long as its slowest trajectory, and an optimiser free to wander along unconstrained parameter
    directions finds regions where the model is stiff and a trajectory takes 20 times the usual steps: such a trial point
    is worth rejecting by its price alone -- the trust region then shrinks away from it.  (Measured on the sloppy
    configs[3] project, 256 starts x 100 iterations of the trust-region algorithm: 4.4 s with a budget of 20 000 attempts,
    1.7 s with 5 000, same costs.)

    The budget is per trajectory and so is the count it is derived from (``sbm_project_trajectory_steps``: round 2
    divided a vector's SUM over its experiments by their number -- with one slow experiment among eight the starts
    themselves ran out of budget).  The STARTING points are integrated with the caller's / the model's own budget
    before this is called (``n_steps_sum`` / ``status`` of that evaluation, if the caller has them); only trial points
    get the derived one.  Returns the budget set (None if the caller named one)."""
    import torch
    if 'max_steps' in integrator_overrides:
        return None
    if n_steps_sum is None:
        out = project.evaluate_batch(th, want=('n_steps',), **integrator_overrides)
        n_steps_sum, status = out['n_steps'], out['status']
    V = int(th.shape[0])
    E = max(1, len(project._experiments))
    worst = 0
    try:
        per = torch.empty((V, E), dtype=torch.int32, device=th.device)
        _lib.check(_lib.load_library().sbm_project_trajectory_steps(project._device(), V, _lib.dev_ptr(per)),
                   'sbm_project_trajectory_steps')
        ok = (status == 0) if status is not None else torch.ones((V,), dtype=torch.bool, device=th.device)
        if bool(ok.any()):
            worst = int(per[ok].max())
    except _lib.SbmError:
        worst = int(n_steps_sum.max()) if n_steps_sum.numel() else 0      # (an upper bound of every trajectory's count)
    # the same cost-quality trade-off for both pairs (scripts/dev_fit_budget.py, 256 starts x 100 iterations of the configs[3]
    # project: median cost 184.6 - 184.8 at 1.2 s with 3x for DOPRI45 (~3 900 attempts) and 6x for DOP853 (~1 200); half the
    # budget: 184.75 / 185.0 at 1.2 / 1.0 s, 185.6 at 0.8 s with 3x for DOP853; twice: 184.3 / 184.5 at 1.9 / 1.4 s)
    method = str(project._options(**integrator_overrides).get('method', 'dopri45')).lower()
    factor = 6.0 if method in _lib.DOP853 else 3.0
    budget = -max(300, int(factor * worst))
    integrator_overrides['max_steps'] = budget
    return budget


def is_param_pair(item):
    """Whether ``item`` names parameters as ``(p_group, settings)``, the way ``Project.get_param_index`` takes them"""
    return isinstance(item, (tuple, list)) and len(item) == 2 and isinstance(item[0], str)


def param_pair_indices(project, pair, what):
    """The parameter indices a ``(p_group, settings)`` pair names, as a list (every setting of the group with 'all').
    ValueError, its message starting with ``what`` (the argument the pair came in), for a name the project does not know."""
    group, settings = pair
    try:
        found = project.get_param_index(group, settings)
    except (KeyError, TypeError):
        raise ValueError("%s: the project has no parameter %r / %r" % (what, group, settings)) from None
    return list(found.values()) if isinstance(found, dict) else [found]


def normalize_held(held, V, q, project=None):
    """The ``held`` argument of ``fit_batch`` as a (V, q) bool array (True: the parameter stays where the start has it).
    Accepted: a bool array (q,) -- the same parameters in every start -- or (V, q); a list of parameter indices; a list of
    ``(p_group, settings)`` pairs, resolved with ``project.get_param_index``.  ValueError on any other shape, an index
    outside [-q, q) or a name the project does not know."""
    arr = held if isinstance(held, np.ndarray) else None
    if arr is None and hasattr(held, 'detach'):
        arr = held.detach().cpu().numpy()
    if arr is None:
        items = list(held)
        if items and all(is_param_pair(it) for it in items):
            if project is None:
                raise ValueError("held: (p_group, settings) pairs need the project that names them")
            arr = np.asarray([i for it in items for i in param_pair_indices(project, it, 'held')], dtype=np.int64)
        else:
            try:
                arr = np.asarray(items)
            except ValueError:
                raise ValueError("held: a bool array (q,) or (V, q), a list of indices or of (p_group, settings) pairs") from None
            if arr.size == 0:
                arr = arr.astype(np.int64)
    if arr.dtype == np.bool_:
        if arr.shape == (q,):
            return np.ascontiguousarray(np.broadcast_to(arr, (V, q)))
        if arr.shape == (V, q):
            return np.ascontiguousarray(arr)
        raise ValueError("held: a bool mask has shape (q,) = (%d,) or (V, q) = (%d, %d), not %s" % (q, V, q, arr.shape))
    if arr.ndim != 1 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("held: a bool array (q,) or (V, q), a list of indices or of (p_group, settings) pairs")
    if arr.size and (arr.min() < -q or arr.max() >= q):
        raise ValueError("held: parameter index out of range for %d parameters: %s" % (q, arr[(arr < -q) | (arr >= q)].tolist()))
    mask = np.zeros((q,), dtype=bool)
    mask[arr] = True
    return np.ascontiguousarray(np.broadcast_to(mask, (V, q)))


def _bound_array(x, V, q, what):
    """One side of ``bounds`` as a (V, q) array: a scalar, (q,) or (V, q)"""
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    try:
        arr = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("bounds: %s is a scalar or an array (q,) or (V, q)" % what) from None
    if arr.shape not in ((), (q,), (V, q)):
        raise ValueError("bounds: %s has shape %s; a scalar, (q,) = (%d,) or (V, q) = (%d, %d)" % (what, arr.shape, q, V, q))
    return np.array(np.broadcast_to(arr, (V, q)), dtype=np.float64, order='C')


def normalize_bounds(bounds, V, q, project=None, thetas0=None, held=None):
    """The ``bounds`` argument of ``fit_batch`` as two contiguous (V, q) float64 arrays (lower, upper), in the units of
    ``thetas0`` (log parameters); an infinite entry leaves that side open.  Accepted: ``(lower, upper)``, each a scalar, an
    array (q,) or (V, q); or a dict ``{(p_group, settings): (lo, hi)}`` resolved with ``project.get_param_index`` (every
    setting of the group with 'all'), parameters it does not name being unbounded.  ``held`` (V, q) bool: held columns are
    exempt from bounds altogether and come back unbounded.  ``thetas0`` (V, q): a start outside its box in a column that is
    not held is refused (scipy's "x0 is infeasible").  ValueError also on a wrong shape, a NaN, lower > upper anywhere and
    a name the project does not know."""
    if isinstance(bounds, dict):
        if project is None:
            raise ValueError("bounds: (p_group, settings) names need the project that resolves them")
        lower, upper = np.full((V, q), -np.inf), np.full((V, q), np.inf)
        for pair, lo_hi in bounds.items():
            if not is_param_pair(pair):
                raise ValueError("bounds: the keys of a dict are (p_group, settings) pairs, not %r" % (pair,))
            try:
                lo, hi = (float(x) for x in lo_hi)
            except (TypeError, ValueError):
                raise ValueError("bounds: the value of %r is a pair (lo, hi) of numbers" % (pair,)) from None
            for c in param_pair_indices(project, pair, 'bounds'):
                lower[:, c], upper[:, c] = lo, hi
    else:
        try:
            lo, hi = bounds
        except (TypeError, ValueError):
            raise ValueError("bounds: a pair (lower, upper) or a dict {(p_group, settings): (lo, hi)}") from None
        lower, upper = _bound_array(lo, V, q, 'lower'), _bound_array(hi, V, q, 'upper')
    if np.isnan(lower).any() or np.isnan(upper).any():
        raise ValueError("bounds: NaN among the bounds")
    if held is not None:
        held = np.asarray(held, dtype=bool)
        lower[held], upper[held] = -np.inf, np.inf
    if (lower > upper).any():
        v, c = np.argwhere(lower > upper)[0]
        raise ValueError("bounds: lower > upper (start %d, parameter %d: %r > %r)" % (v, c, lower[v, c], upper[v, c]))
    if thetas0 is not None:
        x0 = np.asarray(thetas0, dtype=np.float64).reshape(V, q)
        outside = (x0 < lower) | (x0 > upper)
        if outside.any():
            v, c = np.argwhere(outside)[0]
            raise ValueError("bounds: the start is infeasible (start %d, parameter %d: %r outside [%r, %r]); clip the starts "
                             "into the box first" % (v, c, x0[v, c], lower[v, c], upper[v, c]))
    return lower, upper


GEODESIC_H, GEODESIC_ALPHA = 0.1, 0.75          # Transtrum and Sethna's: the probe length and the gate on 2 |a| / |v|


def normalize_geodesic(geodesic):
    """The ``geodesic`` argument of ``fit_batch`` as (h, alpha), or None for the loop without it.  Accepted: None, True
    (the defaults h = 0.1, alpha = 0.75) or a dict with the keys 'h' and / or 'alpha'.  ValueError on anything else, on
    h <= 0 and on alpha < 0."""
    if geodesic is None:
        return None
    if geodesic is True:
        return GEODESIC_H, GEODESIC_ALPHA
    if not isinstance(geodesic, dict) or set(geodesic) - {'h', 'alpha'}:
        raise ValueError("geodesic: None, True or a dict with the keys 'h' and 'alpha', not %r" % (geodesic,))
    try:
        h, alpha = float(geodesic.get('h', GEODESIC_H)), float(geodesic.get('alpha', GEODESIC_ALPHA))
    except (TypeError, ValueError):
        raise ValueError("geodesic: h and alpha are numbers, not %r" % (geodesic,)) from None
    if not (0.0 < h < float('inf')) or not alpha >= 0.0:
        raise ValueError("geodesic: h > 0 and alpha >= 0 are needed, got h = %r, alpha = %r" % (h, alpha))
    return h, alpha


def _prepare(project, thetas0, lazy_jacobian):
    """What the three loops below begin with: the refusal of prior rows under ``reference_compat``, ``lazy_jacobian`` resolved,
    the library and the context (device, stream) the project's model lives on, and the starts staged on the device as a copy
    the loop may write to.  Returns (th (V, q), V, q, device, lib, ctx, lazy_jacobian)."""
    if project.reference_compat and project.n_total_rows != project.n_project_residuals:
        raise ValueError("fit_batch needs reference_compat=False when priors are set: the reference leaves the "
                         "prior rows of the Jacobian zero (SURVEY.md section 8a, quirk 4)")
    if lazy_jacobian == 'auto':
        lazy_jacobian = False        # (see levenberg_marquardt_batch: lazy is opt-in since round 3)
    th, _ = project._theta_dev(np.asarray(thetas0, dtype=np.float64) if not hasattr(thetas0, 'device') else thetas0)
    th = th.clone()
    V, q = th.shape
    return th, V, q, th.device, _lib.load_library(), project._model.device_model.ctx, lazy_jacobian


def _inv_sigma_dev(project, dev):
    """`inverse_row_sigma` on the device: reference_compat leaves J undivided by sigma (quirk 3) and the gradient needs
    d r / d theta"""
    import torch
    inv_sigma = inverse_row_sigma(project)
    return None if inv_sigma is None else torch.from_numpy(inv_sigma).to(dev)


def _warn_unusable_starts(bad):
    import warnings
    warnings.warn("fit_batch: %d of %d starting points could not be integrated; they are returned as they came"
                  % (int(bad.sum()), bad.numel()), stacklevel=2)


def _evaluated_starts(project, th, overrides, warn):
    """The start of the two tensor-select loops (the Marquardt loop, `_trust_region_batch`), which integrate through
    ``evaluate_batch`` so that the host control loops of _control.py can serve them: ``evaluate(t)`` -> (r, J, cost) from one
    state + sensitivity integration and ``cost_only(t)`` from a state-only one; the starts evaluated with the caller's / the
    model's own step budget; then the budget of the trial points (`_trial_budget`, into ``overrides``, which both closures
    read).  Returns (evaluate, cost_only, r, J, cost)."""
    import torch
    inv_sigma = _inv_sigma_dev(project, th.device)
    last = {}

    def evaluate(t):
        out = project.evaluate_batch(t, jacobian=True, want=('jacobian',), **overrides)
        last['n_steps'], last['status'] = out['n_steps'], out['status']
        J = out['jacobian']
        if inv_sigma is not None:
            J = J * inv_sigma[None, :, None]
        return out['residuals'], J, finite_cost(out['norms'], out['status'])

    def cost_only(t):
        out = project.evaluate_batch(t, **overrides)
        return finite_cost(out['norms'], out['status'])

    r, J, cost = evaluate(th)
    if warn and not bool(torch.isfinite(cost).all()):
        _warn_unusable_starts(~torch.isfinite(cost))
    _trial_budget(project, th, overrides, n_steps_sum=last['n_steps'], status=last['status'])
    return evaluate, cost_only, r, J, cost


def _finite_stand_ins(J, r, cost):
    """(J, r) with zeros where the current point is unusable (the steps of such starts are discarded), contiguous"""
    import torch
    fin = torch.isfinite(cost)
    return (torch.where(fin[:, None, None], J, torch.zeros_like(J)).contiguous(),
            torch.where(fin[:, None], r, torch.zeros_like(r)).contiguous())


def _reintegrate_accepted(evaluate, keep, ok, trial, th, r, J, cost):
    """``lazy_jacobian``: residuals and Jacobian of the accepted trial points ``ok``, from ONE integration each (so that
    J^T r is consistent).  The state-only and the state + sensitivity integrations agree to the integrator's tolerance, not
    to the bit: a point stays where it was unless ``keep(cost_a, cost_before)`` holds for its second cost.  Writes the
    points kept into ``th``, ``r`` and ``J``; returns (the mask of the points kept, the new cost vector, the number of points
    integrated)."""
    import torch
    sel = torch.nonzero(ok).flatten()
    ok = torch.zeros_like(ok)
    n = int(sel.numel())
    if n:
        r_a, J_a, cost_a = evaluate(trial[sel])
        good = keep(cost_a, cost[sel])
        sel, r_a, J_a, cost_a = sel[good], r_a[good], J_a[good], cost_a[good]
        th[sel] = trial[sel]
        r[sel] = r_a
        J[sel] = J_a
        cost = cost.clone()
        cost[sel] = cost_a
        ok[sel] = True
    return ok, cost, n


def _median_over(live):
    """t -> the median of ``t`` over the starts ``live`` as a float (0.0 when there are none): the entries of ``trace``"""
    some = bool(live.any())
    return lambda t: float(t[live].median()) if some else 0.0


def _timed(launch, dev):
    """``launch()`` between two synchronisations: milliseconds"""
    import time
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    launch()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


def _traced_launch(integrate_trial, project, ev, tr, done, st, bounded):
    """``trace`` of the fused loop: ``integrate_trial()`` between two synchronisations and the ``launch`` dict of the history entry,
    what the launch cost and why -- it lasts as long as its slowest trajectory (scripts/dev_fit_trace.py).  ``bounded``: ``st``
    is the step status of a bounded fit, which says what steps the bounds took away."""
    import time
    import torch
    torch.cuda.synchronize(ev.dev)
    t_launch = time.perf_counter()
    integrate_trial()
    torch.cuda.synchronize(ev.dev)
    t_launch = time.perf_counter() - t_launch
    V = int(done.shape[0])
    per = torch.empty((V, max(1, len(project._experiments))), dtype=torch.int32, device=ev.dev)
    _lib.check(ev.lib.sbm_project_trajectory_steps(ev.proj, V, _lib.dev_ptr(per)), 'sbm_project_trajectory_steps')
    launch = dict(ms=1e3 * t_launch, steps_max=int(per.max()), steps_mean=float(per.double().mean()),
                  steps_p99=float(per.double().flatten().quantile(0.99)), failed=int((tr['status'] != 0).sum()),
                  done=int((done != 0).sum()))
    if bounded:
        # projected steps that did not descend (status 4), each a spent iteration
        launch['no_descent'] = int(((st == 4) & (done == 0)).sum())
    return launch


def _result(th, cost, n_iter, done, n_eval, n_jac, history=None, held=None, bounds=None):
    """The dict `levenberg_marquardt_batch` returns, from the loop's device tensors"""
    import torch
    out = {'theta': th.cpu().numpy(), 'cost': cost.cpu().numpy(), 'n_iter': n_iter.cpu().numpy().astype(np.int64),
           'converged': (done.bool() & torch.isfinite(cost)).cpu().numpy(), 'n_evaluations': n_eval,
           'n_jacobian_evaluations': n_jac}
    if held is not None:
        out['held'] = held
    if bounds is not None:
        lower, upper = bounds
        out['at_bound'] = (out['theta'] == upper).astype(np.int8) - ((out['theta'] == lower) & (lower < upper)).astype(np.int8)
    if history is not None:
        out['history'] = history
    return out


def levenberg_marquardt_batch(project, thetas0, max_iter=60, lambda0=1e-2, lambda_up=4.0, lambda_down=3.0,
                              ftol=1.49012e-8, xtol=1.49012e-8, max_step=2.0, trace=False, lazy_jacobian='auto',
                              algorithm='trust_region', factor=100.0, held=None, bounds=None, geodesic=None,
                              **integrator_overrides):
    """Minimise 0.5 |r(theta)|^2 from every row of ``thetas0`` (V, q), independently.

    ``algorithm='trust_region'`` (default since round 2): MINPACK's lmder, batched (`_trust_region_batch` below) -- the
    damping of every step comes from a scaled trust region whose radius follows the ratio of actual to predicted
    reduction; ``factor`` is lmder's initial step bound (leastsq's default 100).  On the sloppy 68-parameter configs[3]
    project, 64 starts: median cost 185.8 / 184.5 / 184.0 after 50 / 100 / 200 iterations against 187.4 / 187.0 / 186.8
    for ``algorithm='marquardt'`` (round 1's loop, kept), and where leastsq itself stands at 186.2 after 52 Jacobian
    evaluations of the same start.  ``algorithm='marquardt'``:

    Marquardt damping per start: a step is accepted when the cost decreases (lambda /= lambda_down),
    rejected otherwise (lambda *= lambda_up).  (Nielsen's gain-ratio update was tried and did no better on
    the sloppy 68-parameter test problem.)  A start has converged when a lightly damped (lambda <= 1)
    accepted step lowers the cost by less than ftol * cost with a predicted decrease just as small, or
    changes no parameter by more than xtol * (|theta| + xtol); the defaults are scipy.optimize.leastsq's (the reference's
    optimiser, tests/test_Project.py:202-213).
    Failed integrations (inf cost) count as rejections.  Two safeguards keep wild trial points from
    stalling the whole batch (one launch waits for its slowest trajectory): every component of a step is
    clipped to ``max_step`` log-units, and trial integrations get a step budget
    (``max_steps``; default: three times -- six with DOP853 -- the attempts the slowest trajectory of the starting points
    needs, at least 300, `_trial_budget`) -- a trial that exhausts it is simply rejected.

    ``lazy_jacobian``: a trial point is first integrated WITHOUT sensitivities (the state-only kernels: a
    tenth of the cost) to get its residuals; the state + sensitivity system is integrated only at the trial points that
    were accepted -- MINPACK's economy (lmder evaluates the Jacobian once per successful step, the function once per
    trial), batched: about half of the trials are rejected on a sloppy problem.  ``False``: one state + sensitivity
    integration of every trial point per iteration.  'auto' (default) = ``False`` since round 3 (it was lazy from 8192
    trajectories per iteration on): a launch lasts as long as its slowest trajectory, so two launches per iteration cost
    more than one (256 starts x 8 experiments: 1.23 s eager, 1.74 s lazy per 100 iterations) -- and the cost the
    state-only kernel returns differs from the sensitivity kernel's by the integration tolerance (its steps are chosen by
    the state's error alone), which is what lmder's ftol = 1.5e-8 test resolves: with lazy trial points NO start is ever
    reported converged (costs and parameters are as good).  Pass ``lazy_jacobian=True`` together with looser
    ``ftol`` / tighter ``rtol`` where the saved sensitivity integrations matter.

    ``held``: parameters that stay where the start has them while the others are fitted -- a bool mask (q,) or (V, q)
    (a different set per start: the branches of a profile likelihood, project/profiles.py), a list of parameter indices, or
    a list of ``(p_group, settings)`` pairs as ``get_param_index`` takes them (`normalize_held`).  Every step is lmder's on
    the problem without the held columns (``sbm_lm_trust_step_held`` compacts the system per start: holding 60 of 68
    parameters costs an 8 x 8 factorisation); the returned ``theta[:, held]`` is ``thetas0[:, held]`` bit for bit, a start
    with nothing free comes back as it came, converged.  Supported with ``algorithm='trust_region'`` and an integration
    that is one device call; ``held=None`` is the loop as it was: the same kernels, the same bits.

    ``bounds``: a box the fitted parameters stay in, in the units of ``thetas0`` (log parameters) -- ``(lower, upper)``, each
    a scalar, an array (q,) or (V, q), infinite where a side is open; or a dict ``{(p_group, settings): (lo, hi)}`` whose
    unnamed parameters are unbounded (`normalize_bounds`).  Held parameters are exempt; a start outside its box is refused
    (clip the starts first), as scipy's ``least_squares`` refuses an infeasible x0.  The cost function is unchanged (a prior
    changes it): every step is an active-set step of ``sbm_lm_trust_step_bounded`` -- a parameter on a bound with the
    gradient pushing outward is held for that step, the step on the others is lmder's and is projected into the box, so an
    iterate that reaches a bound lies ON it bit for bit.  A projected step that no longer descends in the model is not taken
    and costs that iteration (the radius is halved); a start whose free parameters all sit on bounds with the gradient
    pushing outward has converged.  Same support as ``held``; ``bounds=None`` is the loop as it was: the same kernels, the same
    bits.

    ``geodesic``: the geodesic acceleration of every step (Transtrum and Sethna 2012), the remedy for the narrow curved
    canyons of sloppy models -- ``True``, or ``dict(h=..., alpha=...)`` (defaults 0.1 and 0.75, the paper's).  Per iteration
    the step v of the trust region is taken as a velocity: theta and theta + h v are integrated WITHOUT sensitivities in one
    call of 2 V vectors (both ends of the difference from the same kernel: the state-only and the sensitivity kernels differ
    by the integration tolerance, which a division by h^2 would magnify), ``sbm_lm_geodesic`` forms the second directional
    derivative r_vv of the residuals, solves the step's own damped system for the acceleration a = -(J^T J + lambda D^2)^-1
    J^T r_vv and replaces the step by v + a / 2 where 2 ||D a|| <= alpha ||D v|| and the new step still descends in the
    model; everywhere else the step stays lmder's, and lmder's acceptance logic is unchanged (no step is rejected on the
    gate).  It is an option and not the default: on Rosenbrock's function it doubles the iterations, and what it buys on
    the configs[3] project is in docs/history.md.  Supported where ``held`` is, with ``held`` and with ``lazy_jacobian``;
    not with ``bounds`` (the projection and the active set of an accelerated step are not built).  ``geodesic=None`` is the
    loop as it was: the same kernels, the same launches, the same bits; ``alpha=0`` pays for the probes and never applies
    the acceleration.

    With a handful of starts the chip is mostly empty: ``variant='small_batch'`` (an integrator override) lets the
    sensitivity kernel use its small-batch split while starts x experiments x chunks <= 2048.

    Returns a dict of numpy arrays: theta (V, q), cost (V,) = 0.5 |r|^2, n_iter (V,) iterations until
    convergence (max_iter if never), converged (V,) bool, n_evaluations (total trial points integrated),
    n_jacobian_evaluations (those integrated with sensitivities); with ``held``, 'held' (V, q) bool; with ``bounds``,
    'at_bound' (V, q) int8: -1 / +1 where the returned theta equals its lower / upper bound, else 0; with ``geodesic``,
    'n_accelerated' (V,): the iterations whose step was accelerated (``n_evaluations`` then counts the 2 V probe vectors
    of every iteration too); with
    ``trace=True`` also 'history': per iteration the number of accepted steps, starts still running, median cost,
    damping, relative decrease and largest step component (costs a device synchronisation per iteration); with
    ``geodesic`` also 'accelerated' (running starts whose step was accelerated), 'rho_median' (2 ||D a|| / ||D v|| over the
    starts where it was computed; 'rho_p10' and 'rho_p90' beside it) and 'probe_ms' / 'geodesic_ms', the two added launches.
    """
    # the loop's bookkeeping in two device launches per iteration (sbm_lm_update / sbm_lm_accept) whenever the integration is
    # ONE device call; the control loops of _control.py (method='auto', 'implicit_romberg') and algorithm='trust_region_torch'
    # (round 2's spelling in tensor selects, kept as the cross-check) take the other
    fused = algorithm in ('trust_region', 'lmder', 'minpack') and one_device_call(project, integrator_overrides)
    if (held is not None or bounds is not None) and not fused:
        raise ValueError("fit_batch: %s are supported by algorithm='trust_region' with an integration method "
                         "that is one device call (not method='auto' / the host-controlled implicit methods); got "
                         "algorithm=%r, method=%r" % ('held parameters' if held is not None else 'bounds', algorithm,
                                                      project._options(**integrator_overrides).get('method')))
    geodesic = normalize_geodesic(geodesic)
    if geodesic is not None and not fused:
        raise ValueError("fit_batch: %s are supported by algorithm='trust_region' with an integration method "
                         "that is one device call (not method='auto' / the host-controlled implicit methods); got "
                         "algorithm=%r, method=%r" % ('geodesic steps', algorithm,
                                                      project._options(**integrator_overrides).get('method')))
    if geodesic is not None and bounds is not None:
        raise ValueError("fit_batch: geodesic steps are not supported together with bounds (the projection and the "
                         "active set of an accelerated step are not built)")
    if algorithm in ('trust_region', 'lmder', 'minpack', 'trust_region_torch'):
        fit = dict(max_iter=max_iter, ftol=ftol, xtol=xtol, factor=factor, trace=trace, lazy_jacobian=lazy_jacobian,
                   max_step=max_step)
        if fused:
            return _trust_region_fused(project, thetas0, held=held, bounds=bounds, geodesic=geodesic, **fit,
                                       **integrator_overrides)
        return _trust_region_batch(project, thetas0, **fit, **integrator_overrides)
    if algorithm != 'marquardt':
        raise ValueError("fit_batch: unknown algorithm %r ('marquardt', 'trust_region' or 'trust_region_torch')" % (algorithm,))
    import torch
    th, V, q, dev, lib, ctx, lazy_jacobian = _prepare(project, thetas0, lazy_jacobian)
    f64, i32 = torch.float64, torch.int32
    evaluate, cost_only, r, J, cost = _evaluated_starts(project, th, integrator_overrides, warn=False)
    M = r.shape[1]
    lam = torch.full((V,), float(lambda0), dtype=f64, device=dev)
    delta = torch.empty((V, q), dtype=f64, device=dev)
    pred = torch.empty((V,), dtype=f64, device=dev)
    st = torch.empty((V,), dtype=i32, device=dev)
    done = ~torch.isfinite(cost)                      # a start that cannot be integrated stays where it is
    n_iter = torch.full((V,), int(max_iter), dtype=torch.int64, device=dev)
    n_eval = V
    n_jac = V                   # state + sensitivity integrations among them
    history = []
    p = _lib.dev_ptr
    for it in range(max_iter):
        Jc, rc = _finite_stand_ins(J, r, cost)
        _lib.check(lib.sbm_lm_step(ctx.handle, p(Jc), p(rc), p(lam), V, M, q, p(delta), p(pred), p(st)), 'sbm_lm_step')
        # per parameter, not by shrinking the whole step: a parameter the data barely constrain gets an
        # enormous (and harmless) Gauss-Newton step, which must not scale everybody else's down to nothing
        delta = delta.clamp(-max_step, max_step)
        trial = torch.where(done[:, None], th, th + delta)
        if lazy_jacobian:
            cost_t = cost_only(trial)
        else:
            r_t, J_t, cost_t = evaluate(trial)
        n_eval += V
        ok = (st == 0) & (cost_t < cost) & ~done
        # MINPACK-style tests, on lightly damped steps only: a heavily damped step is short whatever the
        # distance to the optimum
        free = lam <= 1.0
        small_f = ok & free & ((cost - cost_t) <= ftol * cost) & (pred <= ftol * cost)
        # a negligible step ends the search whether or not it still lowers the cost (at the rounding floor it does not)
        small_x = (st == 0) & ~done & free & (delta.abs() <= xtol * (th.abs() + xtol)).all(dim=1)
        cost_prev = cost
        if lazy_jacobian:
            # (a point whose second integration fails or no longer improves stays where it was)
            ok, cost, n = _reintegrate_accepted(evaluate, lambda c_a, c: torch.isfinite(c_a) & (c_a < c), ok, trial, th, r, J, cost)
            n_jac += n
        else:
            th = torch.where(ok[:, None], trial, th)
            r = torch.where(ok[:, None], r_t, r)
            J = torch.where(ok[:, None, None], J_t, J)
            cost = torch.where(ok, cost_t, cost)
            n_jac += V
        lam = torch.where(ok, lam / lambda_down, lam * lambda_up).clamp(1e-15, 1e15)
        newly = (small_f | small_x) & ~done
        if trace:
            live = ~done
            md = _median_over(live)
            history.append(dict(iteration=it, accepted=int((ok & live).sum()), live=int(live.sum()),
                                cost_median=float(cost.median()), lambda_median=md(lam),
                                rel_decrease_median=md((cost_prev - cost) / cost_prev),
                                step_max_median=md(delta.abs().max(dim=1).values)))
        n_iter = torch.where(newly, torch.full_like(n_iter, it + 1), n_iter)
        done = done | newly
        if bool(done.all()):
            break
    return _result(th, cost, n_iter, done, n_eval, n_jac, history if trace else None)


def _trust_region_batch(project, thetas0, max_iter=60, ftol=1.49012e-8, xtol=1.49012e-8, factor=100.0, trace=False,
                        lazy_jacobian='auto', max_step=2.0, **integrator_overrides):
    """MINPACK's lmder for V starts at once -- the optimiser behind the reference's ``scipy.optimize.leastsq`` calls
    (tests/test_Project.py:202-213, 351-357), with its bookkeeping as tensor selects and its inner problem (lmpar: the
    Levenberg-Marquardt parameter of a scaled trust region) solved per start on the device (``sbm_lm_trust_step``, one
    launch per iteration).

    Per start: D = the largest column norm of J seen so far; the step solves (J^T J + lambda D^2) delta = -J^T r with
    ||D delta|| within 10 % of the radius Delta (lambda = 0 if the Gauss-Newton step is inside); ratio = actual / predicted
    reduction of |r|^2; ratio <= 1/4 shrinks Delta (by 1/2, or by the parabola-fit factor down to 1/10 when the cost went
    up), ratio >= 3/4 or lambda = 0 sets Delta = 2 ||D delta||; the step is taken when ratio >= 1e-4.  Converged (lmder's
    info 1 / 2): actual and predicted relative reductions both <= ftol with ratio <= 2, or Delta <= xtol ||D theta||.
    Trial points are integrated as in the Marquardt loop (``lazy_jacobian``, the step budget with early exit); a trial
    that cannot be integrated counts as an increase of the cost.  ``max_step`` only keeps exp(theta) finite.
    """
    import torch
    th, V, q, dev, lib, ctx, lazy_jacobian = _prepare(project, thetas0, lazy_jacobian)
    f64, i32 = torch.float64, torch.int32
    evaluate, cost_only, r, J, cost = _evaluated_starts(project, th, integrator_overrides, warn=True)
    done = ~torch.isfinite(cost)
    dscale = torch.zeros((V, q), dtype=f64, device=dev)
    lam = torch.zeros((V,), dtype=f64, device=dev)
    radius = torch.full((V,), 1.0, dtype=f64, device=dev)        # set from ||D theta|| once D exists (first pass)
    delta = torch.empty((V, q), dtype=f64, device=dev)
    pred = torch.empty((V,), dtype=f64, device=dev)
    dxnorm = torch.empty((V,), dtype=f64, device=dev)
    st = torch.empty((V,), dtype=i32, device=dev)
    n_iter = torch.full((V,), int(max_iter), dtype=torch.int64, device=dev)
    n_eval, n_jac = V, V
    history = []
    first = True
    for it in range(max_iter):
        Jc, rc = _finite_stand_ins(J, r, cost)
        if first:
            # lmder: D from the first Jacobian, Delta = factor * ||D theta|| (factor itself where that is zero)
            col = torch.sqrt((Jc * Jc).sum(dim=1))
            d0 = torch.where(col > 0, col, torch.ones_like(col))
            xn = (d0 * th).norm(dim=1)
            radius = torch.where(xn > 0, factor * xn, torch.full_like(xn, float(factor)))
        trust_step(ctx, J=Jc, r=rc, dscale=dscale, radius=radius, lam=lam, delta=delta, pred=pred, dxnorm=dxnorm, status=st)
        step = delta.clamp(-max_step, max_step)
        clipped = (step != delta).any(dim=1)
        if bool(clipped.any()):
            # the quantities of the step TAKEN (round 2 judged the clipped step by the unclipped one's prediction):
            # pred = -g.x - x^T J^T J x / 2, ||D x||
            Jx = torch.einsum('vmq,vq->vm', Jc, step)
            gx = torch.einsum('vm,vm->v', rc, Jx)
            pred = torch.where(clipped, -gx - 0.5 * (Jx * Jx).sum(dim=1), pred)
            dxnorm = torch.where(clipped, (dscale * step).norm(dim=1), dxnorm)
        if first:
            # lmder: on the first iteration, Delta = min(Delta, ||D p||) -- of the step taken (the clipped one)
            radius = torch.where(st == 0, torch.minimum(radius, dxnorm), radius)
            first = False
        trial = torch.where(done[:, None], th, th + step)
        if lazy_jacobian:
            cost_t = cost_only(trial)
        else:
            r_t, J_t, cost_t = evaluate(trial)
        n_eval += V
        usable = (st == 0) & ~done
        # lmder's quantities, relative to |r|^2 = 2 cost:  prered = (|J p|^2 + 2 lam |D p|^2) / |r|^2 = pred / cost
        safe_cost = torch.where(cost > 0, cost, torch.ones_like(cost))
        actred = torch.where(0.1 * torch.sqrt(cost_t) < torch.sqrt(cost), 1.0 - cost_t / safe_cost, -torch.ones_like(cost))
        actred = torch.where(torch.isfinite(cost_t), actred, -torch.ones_like(cost))
        prered = pred / safe_cost
        # dirder = g . p / |r|^2  (= -(|J p|^2 + lam |D p|^2) / |r|^2 for an unclipped step: lmder's expression)
        dirder = torch.einsum('vm,vm->v', rc, torch.einsum('vmq,vq->vm', Jc, step)) / (2.0 * safe_cost)
        ratio = torch.where(prered > 0, actred / torch.where(prered > 0, prered, torch.ones_like(prered)), torch.zeros_like(prered))
        # radius update
        shrink = ratio <= 0.25
        temp = torch.where(actred >= 0, torch.full_like(actred, 0.5),
                           0.5 * dirder / torch.where((dirder + 0.5 * actred) != 0, dirder + 0.5 * actred, -torch.ones_like(dirder)))
        worse10 = ~(0.1 * torch.sqrt(cost_t) < torch.sqrt(cost)) | ~torch.isfinite(cost_t)
        temp = torch.where(worse10 | (temp < 0.1) | ~torch.isfinite(temp), torch.full_like(temp, 0.1), temp)
        new_radius = torch.where(shrink, temp * torch.minimum(radius, dxnorm / 0.1),
                                 torch.where((lam == 0) | (ratio >= 0.75), dxnorm / 0.5, radius))
        new_lam = torch.where(shrink, lam / temp, torch.where((lam == 0) | (ratio >= 0.75), 0.5 * lam, lam))
        # a system that could not be solved (status 1): halve the radius, keep the point
        new_radius = torch.where(st == 0, new_radius, 0.5 * radius)
        radius = torch.where(done, radius, new_radius)
        lam = torch.where(done | (st != 0), lam, new_lam)
        ok = usable & (ratio >= 1.0e-4) & torch.isfinite(cost_t)
        cost_prev = cost
        th_before = th.clone() if lazy_jacobian else th
        if lazy_jacobian:
            ok, cost, n = _reintegrate_accepted(evaluate, lambda c_a, c: torch.isfinite(c_a), ok, trial, th, r, J, cost)
            n_jac += n
        else:
            th = torch.where(ok[:, None], trial, th)
            r = torch.where(ok[:, None], r_t, r)
            J = torch.where(ok[:, None, None], J_t, J)
            cost = torch.where(ok, cost_t, cost)
            n_jac += V
        # lmder's convergence tests (info 1, 2); ||D theta|| of the point the iteration started from, as sbm_lm_update has it
        xnorm = (dscale * th_before).norm(dim=1)
        conv_f = usable & (actred.abs() <= ftol) & (prered <= ftol) & (0.5 * ratio <= 1.0)
        conv_x = usable & (radius <= xtol * xnorm)
        newly = (conv_f | conv_x) & ~done
        if trace:
            live = ~done
            md = _median_over(live)
            history.append(dict(iteration=it, accepted=int((ok & live).sum()), live=int(live.sum()), cost_median=float(cost.median()),
                                lambda_median=md(lam), radius_median=md(radius), ratio_median=md(ratio),
                                rel_decrease_median=md((cost_prev - cost) / cost_prev)))
        n_iter = torch.where(newly, torch.full_like(n_iter, it + 1), n_iter)
        done = done | newly
        if bool(done.all()):
            break
    return _result(th, cost, n_iter, done, n_eval, n_jac, history if trace else None)


def _trust_region_fused(project, thetas0, max_iter=60, ftol=1.49012e-8, xtol=1.49012e-8, factor=100.0, trace=False,
                        lazy_jacobian='auto', max_step=2.0, held=None, bounds=None, geodesic=None, **integrator_overrides):
    """`_trust_region_batch` with the bookkeeping on the device: per iteration ONE ``_evaluation.trust_step`` (lmpar, the
    clipped step and the trial point), the integration of the trial points (``sbm_jacobian_batch`` /
    ``sbm_residuals_batch`` into preallocated buffers), ONE ``sbm_lm_update`` (lmder's ratio / radius / acceptance /
    convergence logic) and ONE ``sbm_lm_accept`` (the accepted points' theta, r, J, cost) -- about eight launches and one
    4-byte read-back where round 2's loop issued ~70 tensor selects (68 000 micro-launches in a 100-iteration fit,
    profiles/r02/fit_kernel_stats.csv).  Same algorithm, same numbers up to the order of a few sums.

    ``held`` (see `levenberg_marquardt_batch`): ``trust_step`` gets the (V, q) mask (``sbm_lm_trust_step_held``), the
    initial radius factor * ||D theta|| is that of the free parameters, and a start with nothing free is done before the
    first step.  ``sbm_lm_update`` and ``sbm_lm_accept`` are called as ever: held columns have dscale = 0 and
    trial = theta.

    ``bounds``: ``trust_step`` gets the box (``sbm_lm_trust_step_bounded``, with the held mask or NULL), which chooses the active set
    from this iteration's gradient on the device: no read-back is added.  Its status 3 (a constrained stationary point)
    ends a start in ``sbm_lm_update``; its status 4 (a projected step that does not descend) halves the radius there.

    ``geodesic`` = (h, alpha) (`normalize_geodesic`): between ``trust_step`` and the trial integration the 2 V points
    [theta ; theta + h delta] are written into one preallocated buffer and integrated by ONE state-only call with the
    trial options and budget, and ``_evaluation.geodesic_step`` (``sbm_lm_geodesic``) replaces delta, trial, pred, dxnorm
    and gtx of the starts whose acceleration passes the gate.  A copy, an add, the integration and one kernel more, and no
    read-back: the iteration keeps its one 8-byte read of the counters."""
    import torch
    th, V, q, dev, lib, ctx, lazy_jacobian = _prepare(project, thetas0, lazy_jacobian)
    held_dev = None
    if held is not None:
        held = normalize_held(held, V, q, project)
        held_dev = torch.from_numpy(held).to(dev)
    lower_dev = upper_dev = None
    if bounds is not None:
        bounds = normalize_bounds(bounds, V, q, project, thetas0=th.cpu().numpy(), held=held)
        lower_dev, upper_dev = (torch.from_numpy(b).to(dev) for b in bounds)
    ev = DeviceEvaluator(project)
    M = ev.RT
    f64, i32 = torch.float64, torch.int32
    p = _lib.dev_ptr
    cur, tr = ev.buffers(V, jacobian=True), ev.buffers(V, jacobian=True)
    ev.run(th, project._opts(**integrator_overrides), cur, True)      # the starts: the caller's / the model's own budget
    cost = finite_cost(cur['norms'], cur['status'])
    bad = ~torch.isfinite(cost)
    cur_J, cur_r = cur['jacobian'], cur['residuals']
    if bool(bad.any()):
        _warn_unusable_starts(bad)
        cur_J[bad] = 0.0
        cur_r[bad] = 0.0
    _trial_budget(project, th, integrator_overrides, n_steps_sum=cur['n_steps'], status=cur['status'])
    opts_t = project._opts(**integrator_overrides)
    row_scale = _inv_sigma_dev(project, dev)
    done = bad.to(i32) if held_dev is None else (bad | held_dev.all(dim=1)).to(i32)
    dscale = torch.zeros((V, q), dtype=f64, device=dev)
    lam = torch.zeros((V,), dtype=f64, device=dev)
    # lmder: D from the first Jacobian, Delta = factor * ||D theta|| (factor itself where that is zero)
    Js = cur_J if row_scale is None else cur_J * row_scale[None, :, None]
    col = torch.sqrt((Js * Js).sum(dim=1))
    del Js
    d0 = torch.where(col > 0, col, torch.ones_like(col))
    if held_dev is not None:
        d0 = torch.where(held_dev, torch.zeros_like(d0), d0)
    xn = (d0 * th).norm(dim=1)
    del d0
    radius = torch.where(xn > 0, factor * xn, torch.full_like(xn, float(factor))).contiguous()
    delta = torch.empty((V, q), dtype=f64, device=dev)
    trial = torch.empty((V, q), dtype=f64, device=dev)
    pred, dxnorm, gtx = (torch.empty((V,), dtype=f64, device=dev) for _ in range(3))
    ratio = torch.empty((V,), dtype=f64, device=dev) if trace else None
    st = torch.empty((V,), dtype=i32, device=dev)
    accept = torch.zeros((V,), dtype=i32, device=dev)
    n_iter = torch.full((V,), int(max_iter), dtype=i32, device=dev)
    if held_dev is not None:
        n_iter[held_dev.all(dim=1) & ~bad] = 0
    counters = torch.zeros((2,), dtype=i32, device=dev)
    n_eval, n_jac = V, V
    history = []
    held_i32 = held_dev.to(i32).contiguous() if held_dev is not None else None
    if geodesic is not None:
        geo_h, geo_alpha = geodesic
        points = torch.empty((2 * V, q), dtype=f64, device=dev)         # [theta ; theta + h delta]
        probe = ev.buffers(2 * V)
        accel_st = torch.empty((V,), dtype=i32, device=dev)
        n_accel = torch.zeros((V,), dtype=i32, device=dev)
        rho = torch.empty((V,), dtype=f64, device=dev) if trace else None

    def integrate_trial():
        ev.run(trial, opts_t, tr, not lazy_jacobian)

    def integrate_probe():
        points[:V].copy_(th)
        torch.add(th, delta, alpha=geo_h, out=points[V:])
        ev.run(points, opts_t, probe, False)

    def accelerate():
        geodesic_step(ctx, J=cur_J, r=cur_r, r_base=probe['residuals'][:V], r_probe=probe['residuals'][V:],
                      status_base=probe['status'][:V], status_probe=probe['status'][V:], dscale=dscale, lam=lam,
                      row_scale=row_scale, skip=done, step_status=st, held=held_i32, h=geo_h, alpha=geo_alpha, max_step=max_step,
                      theta=th, delta=delta, trial=trial, pred=pred, dxnorm=dxnorm, gtx=gtx, accel_status=accel_st, ratio=rho,
                      n_accel=n_accel)

    for it in range(max_iter):
        trust_step(ctx, J=cur_J, r=cur_r, dscale=dscale, radius=radius, lam=lam, row_scale=row_scale, skip=done, max_step=max_step,
                   theta=th, trial=trial, delta=delta, pred=pred, dxnorm=dxnorm, gtx=gtx, status=st, held=held_i32,
                   lower=lower_dev, upper=upper_dev)
        geo_ms = None
        if geodesic is not None:
            if trace:
                # the two launches between synchronisations of their own, for the history entry
                geo_ms = (_timed(integrate_probe, dev), _timed(accelerate, dev))
            else:
                integrate_probe()
                accelerate()
            n_eval += 2 * V
        # the integration of the trial points (launch: the trace's record of it, None without trace)
        launch = _traced_launch(integrate_trial, project, ev, tr, done, st, lower_dev is not None) if trace else integrate_trial()
        n_eval += V
        cost_prev = cost.clone() if trace else None
        _lib.check(lib.sbm_lm_update(ctx.handle, p(cost), p(tr['norms']), p(tr['status']), p(pred), p(dxnorm), p(gtx), p(st),
                                     p(th), p(dscale), V, q, float(ftol), float(xtol), it, 1 if it == 0 else 0, p(radius),
                                     p(lam), p(done), p(accept), p(n_iter), p(counters), p(ratio)), 'sbm_lm_update')
        veto_live = 0
        if lazy_jacobian:
            # MINPACK's economy: the state + sensitivity system only at the trial points that were accepted
            sel = torch.nonzero(accept).flatten()
            if sel.numel():
                sub = ev.buffers(int(sel.numel()), jacobian=True)
                ev.run(trial[sel].contiguous(), opts_t, sub, True)
                n_jac += int(sel.numel())
                good = usable(sub['norms'], sub['status'])
                vetoed = sel[~good]
                accept[vetoed] = 0
                # sbm_lm_update ran BEFORE this re-integration: a start whose accepted step is vetoed here (the sensitivity
                # system could not be integrated at the trial point) has not moved, so it has not converged on that step
                # either -- it goes on from where it was
                veto_live = int(vetoed.numel())
                if veto_live:
                    done[vetoed] = 0
                    n_iter[vetoed] = int(max_iter)
                tr['residuals'][sel] = sub['residuals']
                tr['norms'][sel] = sub['norms']
                tr['jacobian'][sel] = sub['jacobian']
        else:
            n_jac += V
        _lib.check(lib.sbm_lm_accept(ctx.handle, p(accept), V, M, q, p(trial), p(tr['residuals']), p(tr['jacobian']), p(tr['norms']),
                                     p(th), p(cur_r), p(cur_J), p(cost)), 'sbm_lm_accept')
        live, n_acc = (int(x) for x in counters.cpu())          # (the one read-back of the iteration)
        if lazy_jacobian and veto_live:
            live, n_acc = int((done == 0).sum()), n_acc - veto_live
        if trace:
            md = _median_over(done == 0)
            history.append(dict(iteration=it, accepted=n_acc, live=live, launch=launch, cost_median=float(cost.median()),
                                lambda_median=md(lam), radius_median=md(radius), ratio_median=md(ratio),
                                rel_decrease_median=md((cost_prev - cost) / cost_prev)))
            if geodesic is not None:
                # (of the starts that were running when the step was made; rho is NaN where it was not computed)
                was_live = st != 2
                seen = was_live & ~torch.isnan(rho)
                lo_q, mid_q, hi_q = (rho[seen].quantile(torch.tensor([0.1, 0.5, 0.9], dtype=f64, device=dev)).tolist()
                                     if bool(seen.any()) else [float('nan')] * 3)
                history[-1].update(accelerated=int(((accel_st == 0) & was_live).sum()), rho_median=mid_q, rho_p10=lo_q,
                                   rho_p90=hi_q, probe_ms=geo_ms[0], geodesic_ms=geo_ms[1])
        if live == 0:
            break
    torch.cuda.synchronize(dev)
    out = _result(th, cost, n_iter, done, n_eval, n_jac, history if trace else None, held, bounds)
    if geodesic is not None:
        out['n_accelerated'] = n_accel.cpu().numpy().astype(np.int64)
    return out
