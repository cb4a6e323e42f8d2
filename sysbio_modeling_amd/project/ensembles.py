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
"""
from __future__ import annotations

import numpy as np


def sampling_axes(hessian, cutoff=0.0, temperature=1.0, step_scale=1.0):
    """Principal axes V (q, q) and step lengths s (q,) of the candidate density: a move is V @ (s * z), z standard
    normal.  ``hessian`` may carry leading batch axes (one Hessian per chain).

    The recipe is SloppyCell's, as the reference carries it (_sampling_matrix, Ensembles.py:226-258): along each
    principal axis v_i of A = hessian / 2 (eigenvalue a_i) the step has standard deviation 1 / sqrt(max(a_i, c)) with
    c = cutoff * max a, so flat directions are not followed without bound; everything is then divided by
    sqrt(n_eff), n_eff = sum_i min(a_i / c, 1) (= the number of axes when nothing is clipped), which makes the
    expected quadratic cost increase of a move about 1, and multiplied by step_scale * sqrt(temperature).
    A is symmetric, so the axes come from ``eigh`` (the reference takes an SVD; the two agree up to the sign of each
    column, which a Gaussian candidate does not see)."""
    A = 0.5 * np.asarray(hessian, dtype=float)
    a, V = np.linalg.eigh(0.5 * (A + np.swapaxes(A, -1, -2)))
    a = np.abs(a)                                   # singular values of a symmetric matrix
    c = cutoff * a.max(axis=-1, keepdims=True)
    stiffness = np.maximum(a, np.maximum(c, np.finfo(float).tiny))
    with np.errstate(divide='ignore', invalid='ignore'):
        n_eff = np.where(c > 0.0, np.minimum(a / np.where(c > 0.0, c, 1.0), 1.0), 1.0).sum(axis=-1, keepdims=True)
    return V, step_scale * np.sqrt(temperature / n_eff) / np.sqrt(stiffness)


def sampling_matrix(hessian, cutoff=0.0, temperature=1.0, step_scale=1.0):
    """Candidate-move matrix M = V diag(s) of ``sampling_axes``: a move is M @ z, Gaussian with covariance M M^T."""
    V, s = sampling_axes(hessian, cutoff, temperature, step_scale)
    return V * s[..., None, :]


def _inv_sigma(project):
    """1 / sigma per measurement row where the project's Jacobian comes undivided by it, else None"""
    return 1.0 / project.descriptor_arrays()['row_sigma'] if project.reference_compat else None


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
                              sampler='host', draws=None, **integrator_overrides):
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
             device.  ``recalc_hess_alg=True`` needs an eigen-decomposition per chain and step, which stays on the host
             path: with ``sampler='device'`` it raises ValueError.
    draws : (z, log_u) of shapes (steps, C, q) and (steps, C): the standard normal and log-uniform numbers to use
             instead of drawing them (``sampler='device'`` only).
    Returns (ens, ens_Fs, ratio): ens (n_kept, C, q) parameter sets including the starts, ens_Fs
    (n_kept, C) their energies, ratio (C,) accepted / attempted per chain.
    """
    starts = np.atleast_2d(np.asarray(params, dtype=float))
    C, q = starts.shape
    if sampler not in ('host', 'device'):
        raise ValueError("sampler must be 'host' or 'device', not %r" % (sampler,))
    if sampler == 'device' and recalc_hess_alg:
        raise ValueError("recalc_hess_alg=True takes an eigen-decomposition per chain and step on the host: use sampler='host'")
    if draws is not None and sampler != 'device':
        raise ValueError("draws= is an argument of sampler='device'")
    sfs = list(project.scale_factors.values()) if project.scale_factors is not None else []
    if energy == 'auto':
        energy = 'free_energy' if sfs and all(sf.log_prior is not None for sf in sfs) else 'rss'

    if sampler == 'device':
        if hess is None:
            hess = _gauss_newton_hessians(project, starts[:1], _inv_sigma(project), integrator_overrides)[0]
        return _device_chains(project, starts, sampling_matrix(hess, sing_val_cutoff, temperature, step_scale), int(steps),
                              float(temperature), seeds, int(skip_elems), energy, draws, integrator_overrides)
    rng = np.random.default_rng(seeds)

    def F(th):
        if energy == 'free_energy':
            return project.free_energy_batch(th, temperature, **integrator_overrides)
        out = 0.5 * project.evaluate_batch(th, **integrator_overrides)['norms']
        return np.where(np.isfinite(out), out, np.inf)

    inv_sigma = _inv_sigma(project)

    def hessians(th):
        return _gauss_newton_hessians(project, th, inv_sigma, integrator_overrides)

    if hess is None and not recalc_hess_alg:
        hess = hessians(starts[:1])[0]
    curr = starts.copy()
    curr_F = F(curr)
    if recalc_hess_alg:
        V, sv = sampling_axes(hessians(curr) if hess is None else np.broadcast_to(hess, (C, q, q)),
                              sing_val_cutoff, temperature, step_scale)
    else:
        V1, s1 = sampling_axes(hess, sing_val_cutoff, temperature, step_scale)
        V, sv = np.broadcast_to(V1, (C, q, q)), np.broadcast_to(s1, (C, q))
    ens, ens_F = [curr.copy()], [curr_F.copy()]
    accepted = np.zeros(C)
    for step in range(1, int(steps) + 1):
        delta = np.einsum('cij,cj->ci', V, sv * rng.standard_normal((C, q)))     # _trial_move, one per chain
        trial = curr + delta
        next_F = F(trial)
        log_ratio = -(next_F - curr_F) / temperature                               # _accept_move
        if recalc_hess_alg:
            ok = np.isfinite(next_F)
            # chains whose trial point cannot be integrated are rejected anyway: their Hessian is not needed
            Vn, sn = sampling_axes(hessians(np.where(ok[:, None], trial, curr)), sing_val_cutoff, temperature, step_scale)
            log_ratio = log_ratio + _log_candidate_density(-delta, Vn, sn) - _log_candidate_density(delta, V, sv)
        with np.errstate(over='ignore', invalid='ignore'):
            acc = np.log(rng.random(C)) < log_ratio
        acc &= np.isfinite(next_F)
        curr = np.where(acc[:, None], trial, curr)
        curr_F = np.where(acc, next_F, curr_F)
        if recalc_hess_alg:
            V = np.where(acc[:, None, None], Vn, V)
            sv = np.where(acc[:, None], sn, sv)
        accepted += acc
        if step % (skip_elems + 1) == 0:
            ens.append(curr.copy())
            ens_F.append(curr_F.copy())
    return np.stack(ens), np.stack(ens_F), accepted / max(int(steps), 1)


_DRAW_BLOCK = 256      # steps whose random numbers are drawn at once


def _device_chains(project, starts, samp, steps, temperature, seeds, skip_elems, energy, draws, overrides):
    """The loop of ``ensemble_log_params_batch(sampler='device')``: per step four enqueues on the context's stream and
    no read-back; the record is a preallocated device array that ``sbm_mh_accept`` writes every (skip_elems + 1)-th
    step."""
    import ctypes
    import torch
    from .. import _control, _lib
    lib = _lib.load_library()
    ctx = project._model.device_model.ctx
    dev = torch.device('cuda', ctx.device)
    proj = project._device()
    p = _lib.dev_ptr
    f64, i32 = torch.float64, torch.int32
    C, q = starts.shape
    free = energy == 'free_energy'
    if free:
        project._require_scale_factor_priors()
    o = project._options(**overrides)
    host_loop = str(o.get('method', 'dopri45')).lower() in _control.IMPLICIT_CONTROLLED + _control.AUTO
    R, RT = project.n_project_residuals, project.n_total_rows
    G = project._n_sf_groups()
    curr = torch.from_numpy(np.ascontiguousarray(starts)).to(dev)
    trial = torch.empty_like(curr)
    samp_d = torch.from_numpy(np.ascontiguousarray(samp, dtype=np.float64)).to(dev)
    sims = torch.empty((C, R), dtype=f64, device=dev)
    resid = torch.empty((C, RT), dtype=f64, device=dev)
    sf = torch.empty((C, G), dtype=f64, device=dev) if G else None
    norms = torch.empty((C,), dtype=f64, device=dev)
    status = torch.empty((C,), dtype=i32, device=dev)
    n_steps = torch.empty((C,), dtype=i32, device=dev)
    entropy = torch.empty((C,), dtype=f64, device=dev) if free else None
    n_acc = torch.zeros((C,), dtype=i32, device=dev)
    opts = None if host_loop else project._opts(**overrides)

    def evaluate(th):
        """norms, status (and sims) of the C points ``th``; entropy of their simulations"""
        if host_loop:
            res = project.evaluate_batch(th, want=('sims', 'norms', 'status'), **overrides)
            nr, st, sm = res['norms'].contiguous(), res['status'].to(i32).contiguous(), res['sims'].contiguous()
        else:
            _lib.check(lib.sbm_residuals_batch(proj, p(th), C, ctypes.byref(opts), p(sims), p(resid), p(sf), p(norms),
                                               p(status), p(n_steps)), 'sbm_residuals_batch')
            nr, st, sm = norms, status, sims
        if free:
            _lib.check(lib.sbm_project_sf_entropy(proj, p(sm), C, temperature, p(entropy), None), 'sbm_project_sf_entropy')
        return nr, st

    nr, st = evaluate(curr)
    F = 0.5 * nr - entropy if free else 0.5 * nr
    F_curr = torch.where(torch.isfinite(F) & (st == 0), F, torch.full_like(F, float('inf'))).contiguous()
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
        _lib.check(lib.sbm_mh_propose(ctx.handle, p(curr), p(samp_d), 0, p(z), C, q, p(trial)), 'sbm_mh_propose')
        nr, st = evaluate(trial)
        slot = step // every if step % every == 0 else None
        _lib.check(lib.sbm_mh_accept(ctx.handle, p(nr), p(st), p(entropy), p(log_u), temperature, C, q, p(trial), p(curr),
                                     p(F_curr), p(n_acc), p(ens[slot]) if slot is not None else None,
                                     p(ens_F[slot]) if slot is not None else None), 'sbm_mh_accept')
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    return ens.cpu().numpy(), ens_F.cpu().numpy(), n_acc.cpu().numpy() / max(steps, 1)
