"""Multi-chain Metropolis sampling of the parameter posterior (a15).

The reference's sampler (project/Ensembles.py:55-178, taken from SloppyCell) walks ONE chain: a
candidate from a Gaussian whose axes come from the Hessian (``_sampling_matrix`` :226-258,
``_trial_move`` :260-264), one ``free_energy`` evaluation -- a full set of LSODA runs -- per step,
Metropolis acceptance ``rand < exp(-dF / T)`` (:193-198).  Here C chains take their steps together: the C
candidates of a step are ONE batched device evaluation (``Project.free_energy_batch`` or, without
scale-factor priors, 0.5 |r|^2 from ``sbm_residuals_batch``).  Same candidate density, same acceptance
rule, same outputs, with a leading chain axis.

The reference module itself cannot run (Python-2 ``print`` / ``cPickle``, and it calls
``Project.hessian``, which does not exist): the Hessian used here is the Gauss-Newton J^T J of the
project Jacobian, what SloppyCell's ``GetJandJtJInLogParameters`` -- the function the docstring names --
returns.

The second half of the module turns a sampled ensemble into predictions (reference Ensembles.py:277-361):
``ensemble_trajs`` integrates every member on a time grid of the caller's choice, ``traj_ensemble_stats`` /
``traj_ensemble_quantiles`` / ``net_ensemble_trajs`` reduce over the members with ``sbm_ensemble_stats`` on the device
(failed members left out, as ``few_ensemble_trajs`` drops NaN trajectories), ``ensemble_predictions`` does both
experiment by experiment and adds the bands of the scaled observables.

Between the two: has the ensemble converged?  ``autocorrelation`` (reference Ensembles.py:14-29) and
``ensemble_diagnostics`` (integrated autocorrelation time, effective sample size, split-R-hat) work on the record where the
device samplers leave it (``sbm_chain_autocorr``, ``sbm_chain_summary``).
"""
from __future__ import annotations

import numpy as np

from ._evaluation import DeviceEvaluator, finite_cost, inverse_row_sigma, one_device_call


def sampling_axes(hessian, cutoff=0.0, temperature=1.0, step_scale=1.0, held=None):
    """Principal axes V (q, q) and step lengths s (q,) of the candidate density: a move is V @ (s * z), z standard
    normal.  ``hessian`` may carry leading batch axes (one Hessian per chain).

    held : bool mask (q,), or (..., q) with batched Hessians (one mask per chain): the density lives in the subspace of the
    free parameters -- the recipe below applied to the free x free block of the Hessian, i.e. the density conditional on
    the held values -- and comes back in the padded full layout of ``sbm_sampling_axes_held`` (include/sbm.h): with nf free
    parameters f_0 < ... < f_{nf-1}, V[f_k, i] and s[i] are the reduced problem's for k, i < nf; the held rows of V and its
    columns from nf on are 0 and s = 1 there, so a move has no held component and ``_log_candidate_density`` is the reduced
    problem's.

    The recipe is SloppyCell's, as the reference carries it (_sampling_matrix, Ensembles.py:226-258): along each
    principal axis v_i of A = hessian / 2 (eigenvalue a_i) the step has standard deviation 1 / sqrt(max(a_i, c)) with
    c = cutoff * max a, so flat directions are not followed without bound; everything is then divided by
    sqrt(n_eff), n_eff = sum_i min(a_i / c, 1) (= the number of axes when nothing is clipped), which makes the
    expected quadratic cost increase of a move about 1, and multiplied by step_scale * sqrt(temperature).
    A is symmetric, so the axes come from ``eigh`` (the reference takes an SVD; the two agree up to the sign of each
    column, which a Gaussian candidate does not see)."""
    if held is not None:
        return _sampling_axes_held(np.asarray(hessian, dtype=float), cutoff, temperature, step_scale, held)
    A = 0.5 * np.asarray(hessian, dtype=float)
    a, V = np.linalg.eigh(0.5 * (A + np.swapaxes(A, -1, -2)))
    a = np.abs(a)                                   # singular values of a symmetric matrix
    c = cutoff * a.max(axis=-1, keepdims=True)
    stiffness = np.maximum(a, np.maximum(c, np.finfo(float).tiny))
    with np.errstate(divide='ignore', invalid='ignore'):
        n_eff = np.where(c > 0.0, np.minimum(a / np.where(c > 0.0, c, 1.0), 1.0), 1.0).sum(axis=-1, keepdims=True)
    return V, step_scale * np.sqrt(temperature / n_eff) / np.sqrt(stiffness)


def _sampling_axes_held(H, cutoff, temperature, step_scale, held):
    """``sampling_axes`` with a mask: one ``eigh`` per distinct mask, on the free blocks of the Hessians that carry it"""
    q = H.shape[-1]
    mask = np.asarray(held)
    if mask.dtype != np.bool_ or mask.shape[-1:] != (q,):
        raise ValueError("held: a bool mask (q,) = (%d,) or one per Hessian (..., %d), not %s %s" % (q, q, mask.dtype, mask.shape))
    try:
        batch = np.broadcast_shapes(H.shape[:-2], mask.shape[:-1])
    except ValueError:
        raise ValueError("held: mask of shape %s does not go with Hessians of shape %s" % (mask.shape, H.shape)) from None
    Hb = np.broadcast_to(H, batch + (q, q)).reshape(-1, q, q)
    mb = np.broadcast_to(mask, batch + (q,)).reshape(-1, q)
    V, s = np.zeros(Hb.shape), np.ones(mb.shape)
    for m in np.unique(mb, axis=0):
        rows = np.flatnonzero((mb == m).all(axis=1))
        free = np.flatnonzero(~m)
        nf = free.size
        if nf == 0:
            continue
        Vr, sr = sampling_axes(Hb[rows][:, free][:, :, free], cutoff, temperature, step_scale)
        V[rows[:, None, None], free[None, :, None], np.arange(nf)[None, None, :]] = Vr
        s[rows[:, None], np.arange(nf)[None, :]] = sr
    return V.reshape(batch + (q, q)), s.reshape(batch + (q,))


def sampling_matrix(hessian, cutoff=0.0, temperature=1.0, step_scale=1.0, held=None):
    """Candidate-move matrix M = V diag(s) of ``sampling_axes``: a move is M @ z, Gaussian with covariance M M^T
    (``held``: in the free subspace, the held rows and the columns behind the free ones zero)."""
    V, s = sampling_axes(hessian, cutoff, temperature, step_scale, held)
    return V * s[..., None, :]


def _gauss_newton_hessians(project, th, inv_sigma, overrides):
    """J^T J of the project Jacobian at every row of ``th``, (C, q, q)."""
    J = project.evaluate_batch(th, jacobian=True, want=('jacobian',), **overrides)['jacobian']
    if inv_sigma is not None:
        J = J.copy()
        J[:, :project.n_project_residuals] *= inv_sigma[None, :, None]
    return np.einsum('crj,crk->cjk', J, J)


def _log_candidate_density(step, V, s):
    """log of the Gaussian density N(0, V diag(s^2) V^T) at ``step`` up to the constant (2 pi)^(-q/2), per chain:
    -0.5 step^T Sigma^-1 step - 0.5 log det Sigma  (reference _accept_move_recalc_alg, Ensembles.py:200-224)."""
    u = np.einsum('cji,cj->ci', V, step) / s       # coordinates along the axes, in units of their step lengths
    return -0.5 * np.sum(u * u, axis=1) - np.sum(np.log(s), axis=1)


def ensemble_log_params_batch(project, params, hess=None, steps=1000, temperature=1.0, step_scale=1.0,
                              sing_val_cutoff=0.0, seeds=None, skip_elems=0, energy='auto', recalc_hess_alg=False,
                              sampler='host', draws=None, held=None, bounds=None, diagnostics=False, **integrator_overrides):
    """C Metropolis chains in log-parameter space, advanced together.

    params : (q,) start shared by all chains, or (C, q) one start per chain (``n_chains`` = C).
    hess   : (q, q) Hessian for the candidate density (default: J^T J at the first start).
    recalc_hess_alg : the reference's second algorithm (Ensembles.py:153-157, 200-224): every chain draws its
             candidate from the Gauss-Newton Hessian J^T J AT ITS CURRENT POINT and the move is accepted with the
             Metropolis-Hastings ratio pi(y) q(y -> x) / (pi(x) q(x -> y)) -- the candidate density now differs between
             the two ends of a move.  The Jacobians of all C trial points come from the same batched device call that
             integrates them.
    energy : 'free_energy' (rss - scale-factor entropy, needs a log prior on every scale factor, as the
             reference), 'rss' (0.5 |r|^2), or 'auto' (free energy when the priors are there).
    sampler : 'host' (default): candidates, energies' quadratures and acceptance in numpy / scipy around one batched
             device evaluation per step.  'device': the whole step is enqueued on the device -- ``sbm_mh_propose``,
             ``sbm_residuals_batch``, ``sbm_project_sf_entropy``, ``sbm_mh_accept`` -- with the random numbers drawn by
             torch on the device from a ``torch.Generator`` seeded with ``seeds``, and one synchronisation at the end.
             Same candidate density, same acceptance rule, same return shapes; another random stream, and the entropy
             by a fixed-node rule instead of ``scipy.integrate.quad``.  ``method='auto'`` / ``'implicit_controlled'``
             are host control loops: the integration then goes through ``evaluate_batch`` and the rest stays on the
             device.  ``sampler='device'`` is the first algorithm only: with ``recalc_hess_alg=True`` it raises ValueError
             and points at 'device_recalc'.
             'device_recalc': the second algorithm (``recalc_hess_alg`` is implied and ignored) with the whole step on
             the device -- ``sbm_mh_propose`` with one matrix per chain, ``sbm_jacobian_batch``, ``sbm_project_sf_entropy``,
             ``sbm_sampling_axes`` (the Gauss-Newton Hessian of every trial point, its eigen-decomposition and the
             clipping recipe in one launch), ``sbm_mh_accept_hastings`` -- no read-back, one synchronisation at the end.
             The first axes come from ``hess`` when given (the same for all chains), else from the Jacobian at the
             starts.  A trial point whose Jacobian is not finite is rejected.  At most ``_lib.SAMPLING_AXES_MAX_Q`` = 96
             parameters.
    draws : (z, log_u) of shapes (steps, C, q) and (steps, C): the standard normal and log-uniform numbers to use
             instead of drawing them (the two device samplers only).  With 'device_recalc' the move is V (s z) with the
             eigenvectors signed as ``sbm_sampling_axes`` signs them (include/sbm.h).
    held   : parameters that never move, in the forms of ``fit_batch(held=)`` (``fitting.normalize_held``: a bool mask (q,)
             or (C, q) -- masks may differ from chain to chain --, indices, or (p_group, settings) pairs): every kept point has
             the start's value there.  The candidate density lives in the free subspace (``sampling_axes(held=)``: the recipe
             on the free x free block of the Hessian, n_eff and the cutoff those of the reduced problem).  A chain with
             everything held is legal and stays put.  The samplers on the device compact every chain's eigen-problem to its
             free columns (``sbm_sampling_axes_held``).
    bounds : a box for the free parameters, in the forms of ``fit_batch(bounds=)`` (``fitting.normalize_bounds``; log units,
             held columns exempt, a start outside its box raises the "infeasible" ValueError), as a uniform prior: a
             candidate with a free component outside [lower, upper] (a bound itself is inside, a NaN is not) is rejected --
             the exact Metropolis rule for the symmetric candidate of the first algorithm and the exact Metropolis-Hastings
             rule for the second, the target being zero outside.  Such a chain evaluates its current point again in that
             step's batched call (on the device: ``sbm_mh_propose_box`` puts it there and vetoes the chain in
             ``sbm_mh_accept[_hastings]_ex``), so no launch waits for a trajectory outside the box and nothing is read back.
             With both None every sampler makes the calls it made before these arguments existed.
    diagnostics : True adds a fourth element, the dict of ``ensemble_diagnostics(ens, ens_Fs)`` (default lag window, no
             thinning).  The device samplers compute it from the record on the device, before the read-back they end with;
             ``sampler='host'`` uploads its record.  False (default): today's 3-tuple through today's calls.
    Returns (ens, ens_Fs, ratio): ens (n_kept, C, q) parameter sets including the starts, ens_Fs
    (n_kept, C) their energies, ratio (C,) accepted / attempted per chain.
    """
    starts = np.atleast_2d(np.asarray(params, dtype=float))
    C, q = starts.shape
    if diagnostics:       # a record the diagnostics cannot take is refused before the run, not after it
        _chain_steps(1 + int(steps) // (int(skip_elems) + 1), 1, 'ensemble_log_params_batch(diagnostics=True)')
    if sampler not in ('host', 'device', 'device_recalc'):
        raise ValueError("sampler must be 'host', 'device' or 'device_recalc', not %r" % (sampler,))
    if sampler == 'device' and recalc_hess_alg:
        raise ValueError("sampler='device' is the first algorithm (one Hessian for the whole run): for recalc_hess_alg=True "
                         "use sampler='device_recalc' (or sampler='host')")
    if draws is not None and sampler == 'host':
        raise ValueError("draws= is an argument of sampler='device' and sampler='device_recalc'")
    if sampler == 'device_recalc':
        from .. import _lib
        if q > _lib.SAMPLING_AXES_MAX_Q:
            raise ValueError("sampler='device_recalc': %d parameters; sbm_sampling_axes keeps the Hessian and its eigenvectors in "
                             "the LDS of one workgroup, which holds q <= %d (use sampler='host')" % (q, _lib.SAMPLING_AXES_MAX_Q))
    box = None
    if held is not None or bounds is not None:
        from .fitting import normalize_bounds, normalize_held
        held_m = normalize_held(held, C, q, project) if held is not None else np.zeros((C, q), dtype=bool)
        lower, upper = (normalize_bounds(bounds, C, q, project, thetas0=starts, held=held_m) if bounds is not None
                        else (np.full((C, q), -np.inf), np.full((C, q), np.inf)))
        box = dict(held=held_m, lower=lower, upper=upper, any_held=held is not None, bounded=bounds is not None)
    sfs = list(project.scale_factors.values()) if project.scale_factors is not None else []
    if energy == 'auto':
        energy = 'free_energy' if sfs and all(sf.log_prior is not None for sf in sfs) else 'rss'

    if sampler == 'device_recalc':
        recalc = dict(hess=None if hess is None else np.ascontiguousarray(hess, dtype=np.float64), cutoff=float(sing_val_cutoff),
                      step_scale=float(step_scale))
        if recalc['hess'] is not None and recalc['hess'].shape != (q, q):
            raise ValueError("hess must have shape (%d, %d), not %s" % (q, q, recalc['hess'].shape))
        return _device_chains(project, starts, None, int(steps), float(temperature), seeds, int(skip_elems), energy, draws,
                              integrator_overrides, recalc=recalc, box=box, diagnostics=diagnostics)
    if sampler == 'device':
        if hess is None:
            hess = _gauss_newton_hessians(project, starts[:1], inverse_row_sigma(project), integrator_overrides)[0]
        if box is not None and box['any_held']:       # one matrix per chain: the masks may differ
            samp = sampling_matrix(np.broadcast_to(np.asarray(hess, dtype=float), (C, q, q)), sing_val_cutoff, temperature,
                                   step_scale, held=box['held'])
        else:
            samp = sampling_matrix(hess, sing_val_cutoff, temperature, step_scale)
        return _device_chains(project, starts, samp, int(steps), float(temperature), seeds, int(skip_elems), energy, draws,
                              integrator_overrides, box=box, diagnostics=diagnostics)
    rng = np.random.default_rng(seeds)
    held_m = box['held'] if box is not None else None

    def F(th):
        if energy == 'free_energy':
            return project.free_energy_batch(th, temperature, **integrator_overrides)
        out = 0.5 * project.evaluate_batch(th, **integrator_overrides)['norms']
        return np.where(np.isfinite(out), out, np.inf)

    inv_sigma = inverse_row_sigma(project)

    def hessians(th):
        return _gauss_newton_hessians(project, th, inv_sigma, integrator_overrides)

    if hess is None and not recalc_hess_alg:
        hess = hessians(starts[:1])[0]
    curr = starts.copy()
    curr_F = F(curr)
    if recalc_hess_alg:
        V, sv = sampling_axes(hessians(curr) if hess is None else np.broadcast_to(hess, (C, q, q)),
                              sing_val_cutoff, temperature, step_scale, held=held_m)
    elif held_m is not None:
        V, sv = sampling_axes(np.broadcast_to(np.asarray(hess, dtype=float), (C, q, q)), sing_val_cutoff, temperature,
                              step_scale, held=held_m)
    else:
        V1, s1 = sampling_axes(hess, sing_val_cutoff, temperature, step_scale)
        V, sv = np.broadcast_to(V1, (C, q, q)), np.broadcast_to(s1, (C, q))
    ens, ens_F = [curr.copy()], [curr_F.copy()]
    accepted = np.zeros(C)
    for step in range(1, int(steps) + 1):
        delta = np.einsum('cij,cj->ci', V, sv * rng.standard_normal((C, q)))     # _trial_move, one per chain
        if box is not None:
            # held components stay; a candidate that left the box is rejected before F sees it: the chain's current
            # point stands in, so the batch keeps its shape
            delta = np.where(held_m, 0.0, delta)
            trial = np.where(held_m, curr, curr + delta)
            outside = (~((trial >= box['lower']) & (trial <= box['upper'])) & ~held_m).any(axis=1) | held_m.all(axis=1)
            trial = np.where(outside[:, None], curr, trial)
        else:
            trial = curr + delta
        next_F = F(trial)
        log_ratio = -(next_F - curr_F) / temperature                               # _accept_move
        if recalc_hess_alg:
            ok = np.isfinite(next_F)
            # chains whose trial point cannot be integrated are rejected anyway: their Hessian is not needed
            Vn, sn = sampling_axes(hessians(np.where(ok[:, None], trial, curr)), sing_val_cutoff, temperature, step_scale,
                                   held=held_m)
            log_ratio = log_ratio + _log_candidate_density(-delta, Vn, sn) - _log_candidate_density(delta, V, sv)
        with np.errstate(over='ignore', invalid='ignore'):
            acc = np.log(rng.random(C)) < log_ratio
        acc &= np.isfinite(next_F)
        if box is not None:
            acc &= ~outside
        curr = np.where(acc[:, None], trial, curr)
        curr_F = np.where(acc, next_F, curr_F)
        if recalc_hess_alg:
            V = np.where(acc[:, None, None], Vn, V)
            sv = np.where(acc[:, None], sn, sv)
        accepted += acc
        if step % (skip_elems + 1) == 0:
            ens.append(curr.copy())
            ens_F.append(curr_F.copy())
    if diagnostics:
        ens, ens_F = np.stack(ens), np.stack(ens_F)
        return ens, ens_F, accepted / max(int(steps), 1), ensemble_diagnostics(ens, ens_F)
    return np.stack(ens), np.stack(ens_F), accepted / max(int(steps), 1)


_DRAW_BLOCK = 256      # steps whose random numbers are drawn at once


def _device_chains(project, starts, samp, steps, temperature, seeds, skip_elems, energy, draws, overrides, recalc=None,
                   box=None, diagnostics=False):
    """The loop of ``ensemble_log_params_batch(sampler='device')``: per step four enqueues on the context's stream and
    no read-back; the record is a preallocated device array that ``sbm_mh_accept`` writes every (skip_elems + 1)-th
    step.

    With ``recalc`` = dict(hess, cutoff, step_scale) the loop of ``sampler='device_recalc'``: ``samp`` is not used, every
    chain keeps the axes (V, s, samp = V diag(s)) of its current point; per step five enqueues -- the evaluation is
    ``sbm_jacobian_batch``, ``sbm_sampling_axes`` turns the trial points' Jacobians into their axes, and
    ``sbm_mh_accept_hastings`` decides with the candidate density at both ends and moves the axes with the point.

    With ``box`` = dict(held, lower, upper, ...) (``held=`` / ``bounds=``) the same enqueues in their box forms:
    ``sbm_mh_propose_box`` (``samp`` (C, q, q) goes per chain), whose ``outside`` flags veto the chains in
    ``sbm_mh_accept_ex`` / ``sbm_mh_accept_hastings_ex``, and ``sbm_sampling_axes_held`` on every chain's free columns.

    With ``diagnostics`` the record goes through ``sbm_chain_autocorr`` / ``sbm_chain_summary`` where it lies, two more
    enqueues per record ahead of the one synchronisation, and the dict of ``ensemble_diagnostics`` is a fourth element."""
    import torch
    from .. import _lib
    ev = DeviceEvaluator(project)
    lib, proj, dev = ev.lib, ev.proj, ev.dev
    ctx = project._model.device_model.ctx
    p = _lib.dev_ptr
    f64, i32 = torch.float64, torch.int32
    C, q = starts.shape
    free = energy == 'free_energy'
    if free:
        project._require_scale_factor_priors()
    host_loop = not one_device_call(project, overrides)
    R, RT = ev.R, ev.RT
    curr = torch.from_numpy(np.ascontiguousarray(starts)).to(dev)
    trial = torch.empty_like(curr)
    if recalc is None:
        samp_d = torch.from_numpy(np.ascontiguousarray(samp, dtype=np.float64)).to(dev)
    else:
        # axes of the current points and of the trial points: V, s, samp
        ax_c = [torch.empty(sh, dtype=f64, device=dev) for sh in ((C, q, q), (C, q), (C, q, q))]
        ax_t = [torch.empty(sh, dtype=f64, device=dev) for sh in ((C, q, q), (C, q), (C, q, q))]
        ax_status = torch.empty((C,), dtype=i32, device=dev)
        row_scale = None
        inv_sigma = inverse_row_sigma(project)
        if inv_sigma is not None:       # the measurement rows of a reference_compat Jacobian come undivided by sigma
            row_scale = torch.ones((RT,), dtype=f64, device=dev)
            row_scale[:R] = torch.from_numpy(np.ascontiguousarray(inv_sigma, dtype=np.float64)).to(dev)
    buf = ev.buffers(C, jacobian=recalc is not None)
    jac = buf.get('jacobian')
    entropy = torch.empty((C,), dtype=f64, device=dev) if free else None
    n_acc = torch.zeros((C,), dtype=i32, device=dev)
    held_d = lower_d = upper_d = outside = None
    if box is not None:
        if box['any_held']:
            held_d = torch.from_numpy(np.ascontiguousarray(box['held'], dtype=np.int32)).to(dev)
        if box['bounded']:
            lower_d = torch.from_numpy(np.ascontiguousarray(box['lower'], dtype=np.float64)).to(dev)
            upper_d = torch.from_numpy(np.ascontiguousarray(box['upper'], dtype=np.float64)).to(dev)
        outside = torch.empty((C,), dtype=i32, device=dev)
    opts = None if host_loop else project._opts(**overrides)

    def evaluate(th):
        """norms, status (and sims) of the C points ``th``; entropy of their simulations; with ``recalc`` their Jacobians"""
        if host_loop:
            if recalc is not None:
                res = project.evaluate_batch(th, jacobian=True, want=('sims', 'norms', 'status', 'jacobian'), **overrides)
                jac.copy_(res['jacobian'])
            else:
                res = project.evaluate_batch(th, want=('sims', 'norms', 'status'), **overrides)
            nr, st, sm = res['norms'].contiguous(), res['status'].to(i32).contiguous(), res['sims'].contiguous()
        else:
            ev.run(th, opts, buf, recalc is not None)
            nr, st, sm = buf['norms'], buf['status'], buf['sims']
        if free:
            _lib.check(lib.sbm_project_sf_entropy(proj, p(sm), C, temperature, p(entropy), None), 'sbm_project_sf_entropy')
        return nr, st

    def axes(out, hess=None):
        """V, s, samp of the points whose Jacobians ``evaluate`` left in ``jac`` (or of one Hessian for all chains)"""
        H = None if hess is None else torch.from_numpy(hess).to(dev)
        if box is not None:
            _lib.check(lib.sbm_sampling_axes_held(ctx.handle, p(jac) if H is None else None, p(row_scale) if H is None else None,
                                                  p(H), 0, C, RT, q, recalc['cutoff'], temperature, recalc['step_scale'], None,
                                                  p(out[0]), p(out[1]), p(out[2]), p(ax_status), p(held_d)),
                       'sbm_sampling_axes_held')
            return
        _lib.check(lib.sbm_sampling_axes(ctx.handle, p(jac) if H is None else None, p(row_scale) if H is None else None, p(H), 0,
                                         C, RT, q, recalc['cutoff'], temperature, recalc['step_scale'], None, p(out[0]),
                                         p(out[1]), p(out[2]), p(ax_status)), 'sbm_sampling_axes')

    nr, st = evaluate(curr)
    if recalc is not None:
        axes(ax_c, recalc['hess'])
    F_curr = finite_cost(nr, st, entropy).contiguous()
    every = skip_elems + 1
    n_kept = 1 + steps // every
    ens = torch.empty((n_kept, C, q), dtype=f64, device=dev)
    ens_F = torch.empty((n_kept, C), dtype=f64, device=dev)
    ens[0].copy_(curr)
    ens_F[0].copy_(F_curr)
    if draws is not None:
        z_all = torch.as_tensor(np.asarray(draws[0], dtype=np.float64) if not isinstance(draws[0], torch.Tensor) else draws[0])
        u_all = torch.as_tensor(np.asarray(draws[1], dtype=np.float64) if not isinstance(draws[1], torch.Tensor) else draws[1])
        if tuple(z_all.shape) != (steps, C, q) or tuple(u_all.shape) != (steps, C):
            raise ValueError("draws must have shapes (steps, C, q) = %s and (steps, C) = %s" % ((steps, C, q), (steps, C)))
        z_all = z_all.to(device=dev, dtype=f64).contiguous()
        u_all = u_all.to(device=dev, dtype=f64).contiguous()
    else:
        gen = torch.Generator(device=dev)
        if seeds is None:
            gen.seed()
        else:
            gen.manual_seed(int(np.random.SeedSequence(seeds).generate_state(1, dtype=np.uint64)[0] >> np.uint64(1)))
    z_blk = u_blk = None
    for step in range(1, steps + 1):
        k = (step - 1) % _DRAW_BLOCK
        if draws is not None:
            z, log_u = z_all[step - 1], u_all[step - 1]
        else:
            if k == 0:
                n = min(_DRAW_BLOCK, steps - step + 1)
                z_blk = torch.randn((n, C, q), dtype=f64, device=dev, generator=gen)
                u_blk = torch.log(torch.rand((n, C), dtype=f64, device=dev, generator=gen))
            z, log_u = z_blk[k], u_blk[k]
        if box is not None:
            m, per_chain = (samp_d, int(samp_d.dim() == 3)) if recalc is None else (ax_c[2], 1)
            _lib.check(lib.sbm_mh_propose_box(ctx.handle, p(curr), p(m), per_chain, p(z), C, q, p(held_d), p(lower_d), p(upper_d),
                                              p(trial), p(outside)), 'sbm_mh_propose_box')
        elif recalc is None:
            _lib.check(lib.sbm_mh_propose(ctx.handle, p(curr), p(samp_d), 0, p(z), C, q, p(trial)), 'sbm_mh_propose')
        else:
            _lib.check(lib.sbm_mh_propose(ctx.handle, p(curr), p(ax_c[2]), 1, p(z), C, q, p(trial)), 'sbm_mh_propose')
        nr, st = evaluate(trial)
        slot = step // every if step % every == 0 else None
        if recalc is not None:
            axes(ax_t)
            if box is not None:
                _lib.check(lib.sbm_mh_accept_hastings_ex(ctx.handle, p(nr), p(st), p(entropy), p(log_u), temperature, C, q, p(trial),
                                                         p(curr), p(F_curr), p(n_acc), p(ens[slot]) if slot is not None else None,
                                                         p(ens_F[slot]) if slot is not None else None, p(ax_c[0]), p(ax_c[1]),
                                                         p(ax_c[2]), p(ax_t[0]), p(ax_t[1]), p(ax_t[2]), p(ax_status), p(outside)),
                           'sbm_mh_accept_hastings_ex')
                continue
            _lib.check(lib.sbm_mh_accept_hastings(ctx.handle, p(nr), p(st), p(entropy), p(log_u), temperature, C, q, p(trial), p(curr),
                                                  p(F_curr), p(n_acc), p(ens[slot]) if slot is not None else None,
                                                  p(ens_F[slot]) if slot is not None else None, p(ax_c[0]), p(ax_c[1]), p(ax_c[2]),
                                                  p(ax_t[0]), p(ax_t[1]), p(ax_t[2]), p(ax_status)), 'sbm_mh_accept_hastings')
            continue
        if box is not None:
            _lib.check(lib.sbm_mh_accept_ex(ctx.handle, p(nr), p(st), p(entropy), p(log_u), temperature, C, q, p(trial), p(curr),
                                            p(F_curr), p(n_acc), p(ens[slot]) if slot is not None else None,
                                            p(ens_F[slot]) if slot is not None else None, p(outside)), 'sbm_mh_accept_ex')
            continue
        _lib.check(lib.sbm_mh_accept(ctx.handle, p(nr), p(st), p(entropy), p(log_u), temperature, C, q, p(trial), p(curr),
                                     p(F_curr), p(n_acc), p(ens[slot]) if slot is not None else None,
                                     p(ens_F[slot]) if slot is not None else None), 'sbm_mh_accept')
    diag = _ensemble_diagnostics_dev(ctx, ens, ens_F, None, 1) if diagnostics else None
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    if diagnostics:
        return ens.cpu().numpy(), ens_F.cpu().numpy(), n_acc.cpu().numpy() / max(steps, 1), {k: v.cpu().numpy() for k, v in diag.items()}
    return ens.cpu().numpy(), ens_F.cpu().numpy(), n_acc.cpu().numpy() / max(steps, 1)


# ---------------------------------------------------------------------------------------------
# Convergence diagnostics of a sampled record (reference project/Ensembles.py:14-29 autocorrelation; tau, ESS and
# split-R-hat on top of it): sbm_chain_autocorr / sbm_chain_summary, kernels in csrc/sbm_chain_diagnostics.hpp
# ---------------------------------------------------------------------------------------------
DEFAULT_MAX_LAG = 1024


def _as_device_record(x, what):
    """(float64 device tensor, was_numpy) of a numpy array or a tensor on the device"""
    import torch
    from .. import _lib
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise ValueError("%s: a torch tensor must live on the device (pass numpy for host data)" % what)
        return x.to(torch.float64).contiguous(), False
    ctx = _lib.default_context()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.device('cuda', ctx.device)), True


def _chain_steps(n_kept, thin, what):
    """steps a record of ``n_kept`` offers at ``thin``; the ValueErrors of a record too long or too short"""
    from .. import _lib
    thin = int(thin)
    if thin < 1:
        raise ValueError("%s: thin must be >= 1, not %r" % (what, thin))
    N = -(-int(n_kept) // thin)
    if N > _lib.CHAIN_MAX_STEPS:
        raise ValueError("%s: %d steps after thinning; a series is kept in the LDS of one workgroup, which holds %d "
                         "(SBM_CHAIN_MAX_STEPS): pass thin= >= %d here, or record fewer steps with the sampler's skip_elems"
                         % (what, N, _lib.CHAIN_MAX_STEPS, -(-int(n_kept) // _lib.CHAIN_MAX_STEPS)))
    if N < 2:
        raise ValueError("%s: %d steps after thinning; a series needs at least 2" % (what, N))
    return N, thin


def _chain_autocorr_dev(ctx, rec, N, S, stride, K, summary=None):
    """Enqueue ``sbm_chain_autocorr`` on the device tensor ``rec`` (steps slowest, ``stride`` doubles between the steps
    used) and, with ``summary`` = (C, q), ``sbm_chain_summary``.  Device tensors ac (S, K), tau (S,), moments (S, 4),
    flags (S,), r_hat (q,) and ess (q,) (None without ``summary``); nothing is synchronised."""
    import torch
    from .. import _lib
    lib, p = ctx.lib, _lib.dev_ptr
    dev, f64 = rec.device, torch.float64
    ac = torch.empty((S, K), dtype=f64, device=dev)
    tau = torch.empty((S,), dtype=f64, device=dev)
    mom = torch.empty((S, 4), dtype=f64, device=dev)
    flags = torch.empty((S,), dtype=torch.int32, device=dev)
    _lib.check(lib.sbm_chain_autocorr(ctx.handle, p(rec), N, S, stride, K, p(ac), p(tau), p(mom), p(flags)), 'sbm_chain_autocorr')
    rhat = ess = None
    if summary is not None:
        C, q = summary
        rhat = torch.empty((q,), dtype=f64, device=dev)
        ess = torch.empty((q,), dtype=f64, device=dev)
        _lib.check(lib.sbm_chain_summary(ctx.handle, p(mom), p(tau), N, C, q, p(rhat), p(ess)), 'sbm_chain_summary')
    return ac, tau, mom, flags, rhat, ess


def autocorrelation(series, max_lag=None):
    """Normalised autocorrelation along axis 0 (reference ``autocorrelation``, Ensembles.py:14-29: de-meaned, zero-padded,
    every lag divided by the number of its terms and by lag 0), by direct lag sums on the device (``sbm_chain_autocorr``).

    series  : (N,) or (N, ...), a numpy array or a torch tensor on the device; 2 <= N <= 16384 (``SBM_CHAIN_MAX_STEPS``).
    max_lag : number of lags K <= N; None = all N, as in the reference.
    Returns (K, ...) of the kind that came in.  A constant series gives NaN at every lag, as the reference's 0 / 0 does."""
    import torch
    from .. import _lib
    rec, was_numpy = _as_device_record(series, 'autocorrelation')
    if rec.dim() < 1:
        raise ValueError("autocorrelation: series must have at least one axis")
    N, _ = _chain_steps(rec.shape[0], 1, 'autocorrelation')
    K = N if max_lag is None else int(max_lag)
    if not 1 <= K <= N:
        raise ValueError("autocorrelation: max_lag must be in [1, N = %d], not %r" % (N, max_lag))
    shape = tuple(rec.shape[1:])
    S = int(rec.numel() // N)
    ctx = _lib.default_context(rec.device.index)
    if S == 0:
        out = torch.empty((K,) + shape, dtype=torch.float64, device=rec.device)
    else:
        out = _chain_autocorr_dev(ctx, rec, N, S, S, K)[0].t().reshape((K,) + shape)
    if was_numpy:
        ctx.synchronize()
        return out.cpu().numpy()
    return out


def _ensemble_diagnostics_dev(ctx, ens, ens_Fs, max_lag, thin):
    """``ensemble_diagnostics`` on device tensors, nothing synchronised: a dict of device tensors"""
    import torch
    if ens.dim() != 3:
        raise ValueError("ensemble_diagnostics: ens must have shape (n_kept, C, q), not %s" % (tuple(ens.shape),))
    n_kept, C, q = (int(v) for v in ens.shape)
    N, thin = _chain_steps(n_kept, thin, 'ensemble_diagnostics')
    K = min(N - 1, DEFAULT_MAX_LAG) if max_lag is None else int(max_lag)
    if not 1 <= K <= N:
        raise ValueError("ensemble_diagnostics: max_lag must be in [1, %d] (the steps after thinning), not %r" % (N, max_lag))
    if C < 1 or q < 1:
        raise ValueError("ensemble_diagnostics: an ensemble needs chains and parameters, not shape %s" % (tuple(ens.shape),))
    ac, tau, _, flags, rhat, ess = _chain_autocorr_dev(ctx, ens, N, C * q, thin * C * q, K, (C, q))
    out = {'autocorrelation': ac.t().reshape(K, C, q), 'tau': tau.reshape(C, q), 'ess_chain': (float(N) / tau).reshape(C, q),
           'ess': ess, 'r_hat': rhat, 'constant': (flags & 1).bool().reshape(C, q), 'truncated': (flags & 2).bool().reshape(C, q)}
    if ens_Fs is not None:
        if tuple(ens_Fs.shape) != (n_kept, C):
            raise ValueError("ensemble_diagnostics: ens_Fs must have shape (n_kept, C) = %s, not %s" % ((n_kept, C), tuple(ens_Fs.shape)))
        acF, tauF, _, _, rhatF, essF = _chain_autocorr_dev(ctx, ens_Fs, N, C, thin * C, K, (C, 1))
        out.update({'autocorrelation_F': acF.t().reshape(K, C), 'tau_F': tauF, 'ess_F': essF.reshape(()), 'r_hat_F': rhatF.reshape(())})
    return out


def ensemble_diagnostics(ens, ens_Fs=None, max_lag=None, thin=1):
    """Convergence diagnostics of a sampled ensemble, computed on the device in one pass per record (``sbm_chain_autocorr``,
    ``sbm_chain_summary``; include/sbm.h has the definitions).

    ens     : (n_kept, C, q) as ``ensemble_log_params_batch`` returns it, a numpy array or a torch tensor on the device.
    ens_Fs  : (n_kept, C) energies of the same kind, optional.
    max_lag : lags K of the autocorrelation; None = min(N - 1, 1024) with N the steps after thinning.
    thin    : use every thin-th kept step (the step stride of the kernel: no copy is made).
    Returns a dict of arrays of the kind that came in:
      'autocorrelation' (K, C, q)   lag first, ``autocorrelation``'s normalisation
      'tau'             (C, q)      integrated autocorrelation time, Geyer's initial positive sequence
      'ess_chain'       (C, q)      N / tau
      'ess'             (q,)        sum over the chains of N / tau, chains without a tau left out.  The sum treats the chains
                                    as samples of one distribution: it means something only where 'r_hat' is close to 1.
      'r_hat'           (q,)        split-R-hat over the 2C half-chains
      'constant'        (C, q) bool the series never moved (a held parameter, a chain that accepted nothing): its
                                    autocorrelation and tau are NaN
      'truncated'       (C, q) bool the window did not close within K lags: tau is a lower bound
      with ens_Fs: 'autocorrelation_F' (K, C), 'tau_F' (C,), 'ess_F' and 'r_hat_F' (scalars)
    More than 16384 steps (``SBM_CHAIN_MAX_STEPS``) after thinning raise ValueError."""
    from .. import _lib
    rec, was_numpy = _as_device_record(ens, 'ensemble_diagnostics')
    F = None if ens_Fs is None else _as_device_record(ens_Fs, 'ensemble_diagnostics')[0]
    ctx = _lib.default_context(rec.device.index)
    out = _ensemble_diagnostics_dev(ctx, rec, F, max_lag, thin)
    if was_numpy:
        ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    return out


# ---------------------------------------------------------------------------------------------
# Principal components of an ensemble (reference project/Ensembles.py:363-382)
# ---------------------------------------------------------------------------------------------
def pca_eig(ens):
    """Principal component analysis of an ensemble (reference PCA_eig): (values (q,), vectors (q, q)), scaled and ordered
    so that they can be set beside the eigen-system of J^T J -- values n / sigma_i^2 with sigma_i the singular values of
    the centred (n, q) ensemble, largest value (tightest direction) first, the vectors in the columns.  ``ens`` is
    (n, q) or the sampler's (n_kept, C, q), which is flattened; it is not modified (the reference centres in place and
    adds the mean back).  One ``sbm_sampling_axes`` call on the centred ensemble as the 'Jacobian' of a single chain:
    the eigenvalues a of X^T X / 2, ascending, are sigma^2 / 2, so the values are n / (2 a) and the vectors come signed
    by that entry's convention.  q <= 96."""
    import torch
    from .. import _lib
    X = np.array(ens, dtype=np.float64)
    if X.ndim == 3:
        X = X.reshape(-1, X.shape[-1])
    if X.ndim != 2 or X.shape[0] == 0:
        raise ValueError("ensemble must have shape (n, q) or (n_kept, C, q), not %s" % (np.shape(ens),))
    n, q = X.shape
    if q > _lib.SAMPLING_AXES_MAX_Q:
        raise ValueError("pca_eig: %d parameters; sbm_sampling_axes holds q <= %d" % (q, _lib.SAMPLING_AXES_MAX_Q))
    X -= X.mean(axis=0)
    lib = _lib.load_library()
    ctx = _lib.default_context()
    dev = torch.device('cuda', ctx.device)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    eig = torch.empty((q,), dtype=torch.float64, device=dev)
    V = torch.empty((q, q), dtype=torch.float64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    p = _lib.dev_ptr
    _lib.check(lib.sbm_sampling_axes(ctx.handle, p(Xd), None, None, 0, 1, n, q, 0.0, 1.0, 1.0, p(eig), p(V), None, None,
                                     p(status)), 'sbm_sampling_axes')
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    if int(status.item()) != 0:
        raise ValueError("pca_eig: the ensemble has entries that are not finite")
    with np.errstate(divide='ignore'):
        return n / (2.0 * eig.cpu().numpy()), V.cpu().numpy()


def pca_eig_log_params(ens):
    """``pca_eig`` of the logarithms of an ensemble of (positive) parameters (reference PCA_eig_log_params)."""
    return pca_eig(np.log(np.asarray(ens, dtype=np.float64)))


# ---------------------------------------------------------------------------------------------
# Ensemble predictions: from a sampled ensemble to trajectories with uncertainty bands
# (reference project/Ensembles.py:277-361; ``project`` stands where SloppyCell's ``net`` stood)
# ---------------------------------------------------------------------------------------------
DEFAULT_QUANTILES = (0.025, 0.5, 0.975)


def _ensemble_2d(project, ensemble):
    """(V, q) project vectors from (V, q), (q,) or the sampler's (n_kept, C, q)."""
    ens = np.asarray(ensemble, dtype=np.float64)
    q = project.n_project_params
    if ens.ndim == 1:
        ens = ens[None, :]
    if ens.ndim not in (2, 3) or ens.shape[-1] != q:
        raise ValueError("ensemble must have shape (V, %d) or (n_kept, C, %d), not %s" % (q, q, ens.shape))
    ens = np.ascontiguousarray(ens.reshape(-1, q))
    if ens.shape[0] == 0:
        raise ValueError("ensemble holds no parameter vector")
    return ens


def _check_members(V):
    from .. import _lib
    if V > _lib.ENSEMBLE_MAX_MEMBERS:
        raise ValueError("%d ensemble members: a column is sorted in the LDS of one workgroup, which holds %d "
                         "(thin the ensemble, e.g. ensemble[::2])" % (V, _lib.ENSEMBLE_MAX_MEMBERS))


def _check_times(times):
    t = np.ascontiguousarray(times, dtype=np.float64)
    if t.ndim != 1 or t.size == 0:
        raise ValueError("times must be a non-empty 1-d array")
    if not np.all(np.isfinite(t)) or np.any(np.diff(t) < 0):
        raise ValueError("times must be finite and non-decreasing")
    if t[0] < 0.0:
        raise ValueError("times must not be negative: a project integrates from t = 0")
    return t


def _check_levels(quantiles):
    lv = np.atleast_1d(np.asarray(quantiles, dtype=np.float64)).ravel()
    if lv.size and not np.all((lv >= 0.0) & (lv <= 1.0)):
        raise ValueError("quantile levels must lie in [0, 1]: %s" % (lv,))
    return np.ascontiguousarray(lv)


def experiment_parameters_batch(project, ensemble, exp_idx):
    """Model parameter vectors (V, n_params) of experiment ``exp_idx`` for every member: the gather of
    ``Project.get_experiment_parameters`` (reference base_project.py:343-363) from the descriptor's index arrays,
    p = exp(theta[pmap]) where pmap >= 0, the experiment's fixed value elsewhere."""
    a = project.descriptor_arrays()
    ens = _ensemble_2d(project, ensemble)
    pmap, pfixed = a['pmap'][exp_idx], a['pfixed'][exp_idx]
    free = pmap >= 0
    P = np.empty((ens.shape[0], pmap.shape[0]))
    P[:, free] = np.exp(ens[:, pmap[free]])
    P[:, ~free] = pfixed[~free]
    return P


def _experiment_indices(project, experiments):
    exps = list(project.experiments)
    if isinstance(experiments, str) and experiments == 'all':
        return list(range(len(exps)))
    if isinstance(experiments, (str, int, np.integer)):
        experiments = [experiments]
    out = []
    for e in experiments:
        out.append(project.get_experiment_index(e) if isinstance(e, str) else int(e))
        if not 0 <= out[-1] < len(exps):
            raise ValueError("experiment index %d of %d" % (out[-1], len(exps)))
    return out


def _variable_names(model):
    gm = getattr(model, 'generated', None)
    return list(gm.spec.variables) if gm is not None else ['y%d' % i for i in range(model.n_vars)]


class EnsembleTrajectories(object):
    """Member trajectories of an ensemble on one time grid, on the device.  Per requested experiment (position ``i`` or
    its name): ``Y[i]`` torch tensor (V, n_t, n_vars), ``status[i]`` torch int32 (V,) -- the integrator's status word, 0
    = the member is usable; shared: ``times`` (n_t,), ``variables`` (names), ``names`` (experiments), ``ensemble`` (V, q)."""

    def __init__(self, project, names, times, variables, ensemble, Y, status):
        self.project, self.names, self.times, self.variables, self.ensemble = project, list(names), times, list(variables), ensemble
        self.Y, self.status = list(Y), list(status)

    def __len__(self):
        return len(self.names)

    def index(self, experiment):
        return self.names.index(experiment) if isinstance(experiment, str) else int(experiment)

    @property
    def n_members(self):
        return self.ensemble.shape[0]


def _integrate_members(project, P, times, overrides):
    """(Y (V, n_t, n_vars), status (V,)) on the device for the parameter vectors P, from t = 0: one ``simulate_dev`` call, or
    the model's host control loop (method='auto' / 'implicit_romberg' / extrapolate=...) with the result uploaded."""
    import torch
    from .. import _control
    model = project._model
    dm = model.device_model
    dev = torch.device('cuda', dm.ctx.device)
    o = project._options(**overrides)
    named = dict(project.integrator_options)
    named.update(overrides)
    method = str(o.get('method', 'dopri45')).lower()
    V, n_t = P.shape[0], times.shape[0]
    if method in _control.IMPLICIT_CONTROLLED + _control.AUTO or model._extrapolated(named):
        t_sim = times if times[0] == 0.0 else np.concatenate([[0.0], times])      # the model takes t_sim[0] for t0
        Y = model.simulate_batch(P, t_sim, **named)
        st = np.asarray(model.last_info['status'], dtype=np.int32)
        Y = np.ascontiguousarray(Y[:, t_sim.shape[0] - n_t:])
        return torch.from_numpy(Y).to(dev), torch.from_numpy(st).to(dev)
    opts = model._opts(times, **named)
    opts.t0 = 0.0
    Pd = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
    td = torch.from_numpy(times).to(dev)
    Y = torch.empty((V, n_t, model.n_vars), dtype=torch.float64, device=dev)
    st = torch.empty((V,), dtype=torch.int32, device=dev)
    dm.simulate_dev(Pd, td, None, opts, Y, st)
    return Y, st


def ensemble_trajs(project, times, ensemble, experiments='all', **integrator_overrides):
    """Trajectories of every member of ``ensemble`` at ``times`` for the requested experiments (reference ensemble_trajs /
    few_ensemble_trajs, Ensembles.py:295-327): per experiment the members' model parameters are gathered from the project
    vectors and integrated from t = 0 in one device call.  Members that fail are not dropped here -- their status word
    is kept and the statistics leave them out.  Integrator options: the project's, then ``integrator_overrides``."""
    ens = _ensemble_2d(project, ensemble)
    t = _check_times(times)
    idx = _experiment_indices(project, experiments)
    exps = list(project.experiments)
    Y, status = [], []
    for e in idx:
        y, st = _integrate_members(project, experiment_parameters_batch(project, ens, e), t, integrator_overrides)
        Y.append(y)
        status.append(st)
    return EnsembleTrajectories(project, [exps[e].name for e in idx], t, _variable_names(project._model), ens, Y, status)


def ensemble_stats_dev(ctx, values, status=None, quantiles=(), want_moments=True):
    """``sbm_ensemble_stats`` on a device tensor ``values`` (V, ...): statistics over the first axis.  Returns numpy arrays
    (mean, std, quantiles (Q, ...), used (V,) bool, n_used); mean and std are None with ``want_moments=False``."""
    import ctypes
    import torch
    from .. import _lib
    lib = _lib.load_library()
    lv = _check_levels(quantiles)
    V = int(values.shape[0])
    _check_members(V)
    shape = tuple(values.shape[1:])
    vals = values.contiguous()
    L = int(vals.numel() // V)
    dev = vals.device
    f64 = torch.float64
    mean = torch.empty((L,), dtype=f64, device=dev) if want_moments else None
    sd = torch.empty((L,), dtype=f64, device=dev) if want_moments else None
    quant = torch.empty((lv.size, L), dtype=f64, device=dev) if lv.size else None
    used = torch.empty((V,), dtype=torch.int32, device=dev)
    n_used = torch.empty((1,), dtype=torch.int32, device=dev)
    st = None if status is None else status.to(torch.int32).contiguous()
    p = _lib.dev_ptr
    step = _lib.ENSEMBLE_MAX_LEVELS
    blocks = list(range(0, lv.size, step)) or [0]
    for k, q0 in enumerate(blocks):
        part = np.ascontiguousarray(lv[q0:q0 + step])
        first = k == 0
        _lib.check(lib.sbm_ensemble_stats(ctx.handle, p(vals), p(st), V, L, _lib.np_ptr(part) if part.size else None, int(part.size),
                                          p(mean) if first else None, p(sd) if first else None,
                                          p(quant[q0:q0 + step]) if part.size else None, p(used), p(n_used)), 'sbm_ensemble_stats')
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    back = lambda x: None if x is None else x.cpu().numpy().reshape(shape)
    qn = quant.cpu().numpy().reshape((lv.size,) + shape) if lv.size else np.zeros((0,) + shape)
    return back(mean), back(sd), qn, used.cpu().numpy().astype(bool), int(n_used.item())


def _ctx(project):
    return project._model.device_model.ctx


def _per_experiment(traj_set, fn):
    out = [fn(i) for i in range(len(traj_set))]
    return out[0] if len(out) == 1 else out


def traj_ensemble_stats(traj_set):
    """(mean, std) over the usable members, numpy (n_t, n_vars) each (population std, as scipy.std in the reference,
    Ensembles.py:277-293); for a trajectory set of several experiments a list of such pairs."""
    ctx = _ctx(traj_set.project)
    return _per_experiment(traj_set, lambda i: ensemble_stats_dev(ctx, traj_set.Y[i], traj_set.status[i])[:2])


def traj_ensemble_quantiles(traj_set, quantiles=DEFAULT_QUANTILES):
    """Quantile trajectories (Q, n_t, n_vars) over the usable members, linearly interpolated between order statistics
    (reference Ensembles.py:335-361); for a trajectory set of several experiments a list of them."""
    ctx = _ctx(traj_set.project)
    return _per_experiment(traj_set, lambda i: ensemble_stats_dev(ctx, traj_set.Y[i], traj_set.status[i], quantiles,
                                                                  want_moments=False)[2])


def net_ensemble_trajs(project, times, ensemble, experiments='all', **integrator_overrides):
    """(best, mean, std): ``best`` is the trajectory of member 0, as in the reference (Ensembles.py:329-333); numpy
    (n_t, n_vars) each, or lists of them for several experiments."""
    ts = ensemble_trajs(project, times, ensemble, experiments, **integrator_overrides)
    ctx = _ctx(project)

    def one(i):
        mean, sd = ensemble_stats_dev(ctx, ts.Y[i], ts.status[i])[:2]
        return ts.Y[i][0].cpu().numpy(), mean, sd
    out = [one(i) for i in range(len(ts))]
    return tuple(out[0]) if len(out) == 1 else tuple(list(x) for x in zip(*out))


def _custom_measures(project):
    return sorted(nm for nm, m in project._measurement_to_model_map.items() if m['type'] == 'custom')


def _experiment_measures(project, exp_idx):
    """[(measure name, variable indices, scale-factor group or -1)] of the measures experiment ``exp_idx`` carries"""
    exp = list(project.experiments)[exp_idx]
    out = []
    for nm in dict.fromkeys(m.variable_name for m in exp.measurements):
        mp = project._measurement_to_model_map[nm]
        out.append((nm, list(mp['variables']), int(project._sf_group_of(nm))))
    return out


def scaled_observables(project, Y, status, exp_idx, sf, eval_status):
    """Scaled observables of every member BEFORE any reduction: Z (V, n_t, M) = B_g(member) * sum of the measure's
    variables, for the M 'direct' / 'sum' measures of the experiment (B = 1 without a scale-factor group), and the status
    that leaves a member out of them (its trajectory's, or its project evaluation's).  Device tensors."""
    import torch
    meas = _experiment_measures(project, exp_idx)
    Z = torch.empty((Y.shape[0], Y.shape[1], len(meas)), dtype=Y.dtype, device=Y.device)
    for k, (nm, variables, g) in enumerate(meas):
        z = Y[:, :, variables].sum(dim=2)
        Z[:, :, k] = z * sf[:, g:g + 1] if g >= 0 else z
    return [nm for nm, _, _ in meas], Z, torch.maximum(status, eval_status.to(status.dtype))


def ensemble_predictions(project, times, ensemble, quantiles=DEFAULT_QUANTILES, measures=True, experiments='all',
                         **integrator_overrides):
    """Prediction bands of an ensemble, experiment by experiment: integrate the members, reduce on the device, keep the
    statistics, free the trajectories -- the memory-lean path from a sampled ensemble to what is plotted over the data.

    Returns {experiment name: {'times', 'variables', 'mean' (n_t, n_vars), 'std', 'quantiles' (Q, n_t, n_vars), 'n_used',
    'levels'}}; with ``measures=True`` also 'measures' = {'names', 'mean' (n_t, M), 'std', 'quantiles' (Q, n_t, M),
    'n_used'}: bands of the SCALED observables B_g * sum(variables) of the experiment's 'direct' / 'sum' measures.  The
    product is formed per member before the reduction (quantiles of a product are not products of quantiles); B comes
    from one ``evaluate_batch`` of the ensemble, and a member whose project evaluation failed is left out of the
    measures.  'custom' measures are not built: with ``measures=True`` a project that has one raises ValueError."""
    import torch
    ens = _ensemble_2d(project, ensemble)
    _check_members(ens.shape[0])
    t = _check_times(times)
    lv = _check_levels(quantiles)
    idx = _experiment_indices(project, experiments)
    if measures and _custom_measures(project):
        raise ValueError("ensemble_predictions(measures=True): 'custom' mapped measures are not supported (%s); "
                         "pass measures=False for the state bands" % ", ".join(_custom_measures(project)))
    ctx = _ctx(project)
    dev = torch.device('cuda', ctx.device)
    sf = eval_status = None
    if measures:
        res = project.evaluate_batch(torch.from_numpy(ens).to(dev), want=('sf', 'status'), **integrator_overrides)
        sf, eval_status = res['sf'], res['status'].to(torch.int32)
    exps = list(project.experiments)
    variables = _variable_names(project._model)
    out = {}
    for e in idx:
        Y, st = _integrate_members(project, experiment_parameters_batch(project, ens, e), t, integrator_overrides)
        mean, sd, qn, _, n_used = ensemble_stats_dev(ctx, Y, st, lv)
        entry = dict(times=t, variables=variables, levels=lv, mean=mean, std=sd, quantiles=qn, n_used=n_used)
        if measures:
            names, Z, zst = scaled_observables(project, Y, st, e, sf, eval_status)
            zm, zs, zq, _, zn = ensemble_stats_dev(ctx, Z, zst, lv)
            entry['measures'] = dict(names=names, mean=zm, std=zs, quantiles=zq, n_used=zn)
            del Z
        del Y
        out[exps[e].name] = entry
    return out
