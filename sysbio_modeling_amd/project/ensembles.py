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

What becomes of a sampled ensemble lives next door and keeps its names here: has it converged (project/chain_diagnostics.py),
and its predictions (project/predictions.py, reference Ensembles.py:277-361).
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ._evaluation import (DeviceEvaluator, finite_cost, inverse_row_sigma, mh_accept, mh_propose, one_device_call,
                          pt_swap, sampling_axes as device_sampling_axes)
from .chain_diagnostics import (DEFAULT_MAX_LAG, _chain_steps, _ensemble_diagnostics_dev, autocorrelation,  # noqa: F401
                                ensemble_diagnostics)
from .predictions import (DEFAULT_QUANTILES, EnsembleTrajectories, _experiment_measures, ensemble_predictions,  # noqa: F401
                          ensemble_stats_dev, ensemble_trajs, experiment_parameters_batch, net_ensemble_trajs,
                          scaled_observables, traj_ensemble_quantiles, traj_ensemble_stats)


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


def temperature_ladder(K, t_max):
    """The geometric temperature ladder of K rungs from 1 to ``t_max``, ``np.geomspace(1, t_max, K)``: equal ratios between
    neighbours, which gives equal swap rates between them where the heat capacity is constant (a Gaussian posterior)."""
    return np.geomspace(1.0, float(t_max), int(K))


def ensemble_log_params_batch(project, params, hess=None, steps=1000, temperature=1.0, step_scale=1.0,
                              sing_val_cutoff=0.0, seeds=None, skip_elems=0, energy='auto', recalc_hess_alg=False,
                              sampler='host', draws=None, held=None, bounds=None, diagnostics=False, swap_every=None,
                              **integrator_overrides):
    """C Metropolis chains in log-parameter space, advanced together.

    params : (q,) start shared by all chains, or (C, q) one start per chain (``n_chains`` = C).
    temperature : a number -- every chain samples exp(-F / T) --, or a ladder (T_0, ..., T_{K-1}) of K >= 2 positive
             temperatures, in any order, for parallel tempering (replica exchange): C must be a multiple of K, chain c
             is rung c % K of ladder c // K (the rungs of a ladder are neighbours) and samples exp(-F(theta; T_k) / T_k) for
             the whole run, with its own candidate density ``sampling_matrix(hess, cutoff, T_k, step_scale)``.  So
             ``ens[:, c]`` is a sample at T[c % K] and ``ens[:, ::K]`` are the chains of rung 0; ``ens_Fs[:, c]`` holds
             F(x_c; T_c).  The first algorithm only, with ``sampler='host'`` or ``'device'``.
    swap_every : with a ladder, a replica-exchange step after the acceptance of every ``swap_every``-th step.  The n-th of
             them (from 0) proposes, in every ladder, the pairs of rungs (k, k + 1) with k % 2 == n % 2; with i the lower
             chain, j = i + 1 and F_cross[c] = F(x_c; T of c's partner) the two chains exchange their POINTS -- a chain
             keeps its temperature -- iff both cross energies are finite and
             log u < (F[i] - F_cross[j]) / T[i] + (F[j] - F_cross[i]) / T[j]  (for 'rss', whose energy does not depend on T:
             (F_i - F_j) (1 / T_i - 1 / T_j)).  With 'free_energy' a swap step evaluates the current points once more
             (state only) for the cross energies; on the device that is one ``sbm_residuals_batch``, one
             ``sbm_project_sf_entropy_pt`` and one ``sbm_pt_swap``, still without a read-back.  Whole rows are exchanged, so
             ``held`` masks, the start values of held columns and ``bounds`` must be equal within a ladder (ValueError).
             None with a ladder is legal: independent chains at different temperatures.  With a scalar temperature it must
             be None (ValueError), and every sampler then enqueues the kernels it enqueued before ladders existed.
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
             eigenvectors signed as ``sbm_sampling_axes`` signs them (include/sbm.h).  With ``swap_every`` a third array is
             required, (z, log_u, log_u_swap): log_u_swap (steps // swap_every, C), of which a swap step reads the entry of
             each pair's lower chain.  Without ``draws`` the swap numbers come from a second generator derived from
             ``seeds``; the two existing streams deliver the numbers they delivered before.
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
             With both None every sampler launches the kernels it launched before these arguments existed: the same bits.
    diagnostics : True adds a fourth element, the dict of ``ensemble_diagnostics(ens, ens_Fs)`` (default lag window, no
             thinning).  The device samplers compute it from the record on the device, before the read-back they end with;
             ``sampler='host'`` uploads its record.  False (default): today's 3-tuple through today's calls.  With a ladder
             the diagnostics cover the chains of rung 0 only, through a contiguous copy of ``ens[:, ::K]`` (C / K chains):
             R-hat across chains that sample different temperatures means nothing.
    Returns (ens, ens_Fs, ratio): ens (n_kept, C, q) parameter sets including the starts, ens_Fs
    (n_kept, C) their energies, ratio (C,) accepted / attempted per chain.  With a ladder one more element comes last, the
    dict temperature (C,), rung (C,), ladder (C,), swap_attempted (C,), swap_accepted (C,) -- the last two counted at the
    lower chain of each pair (0 at the top rung): swap_accepted / swap_attempted of chain c is the swap ratio between the
    rungs c % K and c % K + 1 of its ladder.
    """
    starts = np.atleast_2d(np.asarray(params, dtype=float))
    C, q = starts.shape
    _check_sampler_arguments(sampler, recalc_hess_alg, draws, diagnostics, steps, skip_elems, q)
    box = _sampler_box(project, starts, held, bounds)
    ladder = _temperature_ladder_arguments(temperature, swap_every, starts, int(steps), sampler, recalc_hess_alg, draws, box)
    sfs = list(project.scale_factors.values()) if project.scale_factors is not None else []
    if energy == 'auto':
        energy = 'free_energy' if sfs and all(sf.log_prior is not None for sf in sfs) else 'rss'
    if sampler == 'host':
        return _host_chains(project, starts, hess, int(steps), temperature, step_scale, sing_val_cutoff, seeds, skip_elems, energy,
                            recalc_hess_alg, integrator_overrides, box, diagnostics, ladder)
    samp = recalc = None
    if sampler == 'device_recalc':
        recalc = dict(hess=None if hess is None else np.ascontiguousarray(hess, dtype=np.float64), cutoff=float(sing_val_cutoff),
                      step_scale=float(step_scale))
        if recalc['hess'] is not None and recalc['hess'].shape != (q, q):
            raise ValueError("hess must have shape (%d, %d), not %s" % (q, q, recalc['hess'].shape))
    else:
        if hess is None:
            hess = _gauss_newton_hessians(project, starts[:1], inverse_row_sigma(project), integrator_overrides)[0]
        if ladder is not None:                         # one matrix per chain: that of its rung
            V, s = _ladder_axes(hess, sing_val_cutoff, ladder, step_scale, box['held'] if box is not None and box['any_held'] else None, C)
            samp = V * s[..., None, :]
        elif box is not None and box['any_held']:     # one matrix per chain: the masks may differ
            samp = sampling_matrix(np.broadcast_to(np.asarray(hess, dtype=float), (C, q, q)), sing_val_cutoff, temperature,
                                   step_scale, held=box['held'])
        else:
            samp = sampling_matrix(hess, sing_val_cutoff, temperature, step_scale)
    return _device_chains(project, starts, samp, int(steps), None if ladder is not None else float(temperature), seeds,
                          int(skip_elems), energy, draws, integrator_overrides, recalc=recalc, box=box, diagnostics=diagnostics,
                          ladder=ladder)


def _temperature_ladder_arguments(temperature, swap_every, starts, steps, sampler, recalc_hess_alg, draws, box):
    """``temperature=`` / ``swap_every=`` of ``ensemble_log_params_batch`` checked and laid out for the C chains: None for a
    scalar temperature, else the dict below.  Everything a swap step needs that depends only on the arguments is made here,
    once: per parity the mask of the lower chains and every chain's partner temperature (its own where it has no partner)."""
    if np.ndim(temperature) == 0:
        if swap_every is not None:
            raise ValueError("swap_every= exchanges replicas between the rungs of a temperature ladder: give temperature= as a "
                             "sequence (temperature_ladder(K, t_max)), not the number %r" % (temperature,))
        return None
    C, q = starts.shape
    T = np.asarray(temperature, dtype=float)
    if T.ndim != 1 or T.size < 2:
        raise ValueError("temperature: a number or a ladder of K >= 2 temperatures, not an array of shape %s" % (T.shape,))
    if not np.all(np.isfinite(T) & (T > 0.0)):
        raise ValueError("temperature: every rung of the ladder must be finite and > 0, not %s" % (T,))
    K = T.size
    if C % K:
        raise ValueError("%d chains are not a whole number of ladders of %d rungs" % (C, K))
    if recalc_hess_alg or sampler == 'device_recalc':
        raise ValueError("a temperature ladder goes with the first algorithm only: the axes of the second one scale with sqrt(T) "
                         "and would have to travel with a swap (recalc_hess_alg=False, sampler='host' or 'device')")
    rung, chain_T = np.arange(C) % K, np.tile(T, C // K)
    out = dict(T=T, K=K, chain_T=chain_T, rung=rung, ladder=np.arange(C) // K, swap_every=None, n_swaps=0)
    if swap_every is None:
        return out
    if int(swap_every) != swap_every or int(swap_every) < 1:
        raise ValueError("swap_every must be a positive whole number of steps, not %r" % (swap_every,))
    out['swap_every'], out['n_swaps'] = int(swap_every), steps // int(swap_every)
    if draws is not None and (len(draws) != 3 or draws[2] is None):
        raise ValueError("draws= with swap_every= takes three arrays, (z, log_u, log_u_swap): log_u_swap of shape "
                         "(steps // swap_every, C) = %s" % ((out['n_swaps'], C),))
    if box is not None:       # a swap exchanges whole rows: what is fixed or bounded has to be the same on both sides
        first = lambda a: np.repeat(a.reshape(C // K, K, q)[:, :1], K, axis=1).reshape(C, q)      # noqa: E731
        same = (np.array_equal(box['held'], first(box['held'])) and np.array_equal(box['lower'], first(box['lower']))
                and np.array_equal(box['upper'], first(box['upper']))
                and np.array_equal(np.where(box['held'], starts, 0.0), np.where(box['held'], first(starts), 0.0)))
        if not same:
            raise ValueError("swap_every=: a swap exchanges whole parameter rows, so the held mask, the start values of the "
                             "held columns and the bounds must be equal within every ladder")
    lower = np.stack([(rung % 2 == parity) & (rung + 1 < K) for parity in (0, 1)])                 # (2, C)
    partner = np.where(lower, np.arange(C) + 1, np.where(np.roll(lower, 1, axis=1), np.arange(C) - 1, np.arange(C)))
    out.update(lower=lower, partner_T=chain_T[partner])
    return out


def _ladder_axes(hess, cutoff, ladder, step_scale, held_m, C):
    """``sampling_axes`` of the C chains of temperature ladders, V (C, q, q) and s (C, q): chain c gets the axes of
    ``hess`` (q, q) at its rung's temperature (and with its own held mask, ``held_m`` (C, q) or None)."""
    hess = np.asarray(hess, dtype=float)
    q, K = hess.shape[-1], ladder['K']
    V, s = np.empty((C, q, q)), np.empty((C, q))
    for k, T in enumerate(ladder['T']):
        if held_m is None:
            V[k::K], s[k::K] = sampling_axes(hess, cutoff, T, step_scale)
        else:
            V[k::K], s[k::K] = sampling_axes(np.broadcast_to(hess, (C // K, q, q)), cutoff, T, step_scale, held=held_m[k::K])
    return V, s


def _ladder_summary(ladder, n_swapped):
    """The last element of a tempered run's return value (``ensemble_log_params_batch``); attempts depend only on the number
    of swap steps, so they are counted here"""
    n = ladder['n_swaps']
    attempted = np.zeros(ladder['chain_T'].shape, dtype=np.int64)
    if n:
        attempted = (n + 1) // 2 * ladder['lower'][0].astype(np.int64) + n // 2 * ladder['lower'][1].astype(np.int64)
    return dict(temperature=ladder['chain_T'].copy(), rung=ladder['rung'].copy(), ladder=ladder['ladder'].copy(),
                swap_attempted=attempted, swap_accepted=np.asarray(n_swapped, dtype=np.int64))


def _check_sampler_arguments(sampler, recalc_hess_alg, draws, diagnostics, steps, skip_elems, q):
    """The ValueErrors of ``ensemble_log_params_batch`` that need nothing but its arguments"""
    if diagnostics:       # a record the diagnostics cannot take is refused before the run, not after it
        _chain_steps(1 + int(steps) // (int(skip_elems) + 1), 1, 'ensemble_log_params_batch(diagnostics=True)')
    if sampler not in ('host', 'device', 'device_recalc'):
        raise ValueError("sampler must be 'host', 'device' or 'device_recalc', not %r" % (sampler,))
    if sampler == 'device' and recalc_hess_alg:
        raise ValueError("sampler='device' is the first algorithm (one Hessian for the whole run): for recalc_hess_alg=True "
                         "use sampler='device_recalc' (or sampler='host')")
    if draws is not None and sampler == 'host':
        raise ValueError("draws= is an argument of sampler='device' and sampler='device_recalc'")
    if sampler == 'device_recalc' and q > _lib.SAMPLING_AXES_MAX_Q:
        raise ValueError("sampler='device_recalc': %d parameters; sbm_sampling_axes keeps the Hessian and its eigenvectors in "
                         "the LDS of one workgroup, which holds q <= %d (use sampler='host')" % (q, _lib.SAMPLING_AXES_MAX_Q))


def _sampler_box(project, starts, held, bounds):
    """``held=`` / ``bounds=`` normalised for the C chains: None without either, else the dict below ((C, q) arrays, two flags)"""
    if held is None and bounds is None:
        return None
    from .fitting import normalize_bounds, normalize_held
    C, q = starts.shape
    held_m = normalize_held(held, C, q, project) if held is not None else np.zeros((C, q), dtype=bool)
    lower, upper = (normalize_bounds(bounds, C, q, project, thetas0=starts, held=held_m) if bounds is not None
                    else (np.full((C, q), -np.inf), np.full((C, q), np.inf)))
    return dict(held=held_m, lower=lower, upper=upper, any_held=held is not None, bounded=bounds is not None)


def _host_chains(project, starts, hess, steps, temperature, step_scale, sing_val_cutoff, seeds, skip_elems, energy,
                 recalc_hess_alg, integrator_overrides, box, diagnostics, ladder=None):
    """The loop of ``ensemble_log_params_batch(sampler='host')``: candidates, acceptance and the record in numpy around one
    batched device evaluation per step (two with ``recalc_hess_alg``: the Jacobians of the trial points).  ``ladder``
    (``_temperature_ladder_arguments``): ``temperature`` becomes the chains' own (C,), and every ``swap_every``-th step ends
    with a replica exchange (``_host_swap``), for 'free_energy' after one more evaluation of the current points at the
    partners' temperatures."""
    C, q = starts.shape
    rng = np.random.default_rng(seeds)
    held_m = box['held'] if box is not None else None
    if ladder is not None:
        temperature = ladder['chain_T']
        # a second stream for the swaps, a child of the first one's seed: the first delivers the numbers it always did
        swap_rng = np.random.default_rng(rng.bit_generator.seed_seq.spawn(1)[0])
        n_swapped, n_swaps = np.zeros(C, dtype=np.int64), 0

    def F(th, T=temperature):
        if energy == 'free_energy':
            return project.free_energy_batch(th, T, **integrator_overrides)
        out = 0.5 * project.evaluate_batch(th, **integrator_overrides)['norms']
        return np.where(np.isfinite(out), out, np.inf)

    inv_sigma = inverse_row_sigma(project)
    hessians = lambda th: _gauss_newton_hessians(project, th, inv_sigma, integrator_overrides)      # noqa: E731

    if hess is None and not recalc_hess_alg:
        hess = hessians(starts[:1])[0]
    curr = starts.copy()
    curr_F = F(curr)
    if ladder is not None:
        V, sv = _ladder_axes(hess, sing_val_cutoff, ladder, step_scale, held_m, C)
    else:
        # one Hessian per chain, the given one broadcast: numpy's batched eigh takes the matrices one by one
        V, sv = sampling_axes(hessians(curr) if hess is None else np.broadcast_to(np.asarray(hess, dtype=float), (C, q, q)),
                              sing_val_cutoff, temperature, step_scale, held=held_m)
    ens, ens_F = [curr.copy()], [curr_F.copy()]
    accepted = np.zeros(C)
    for step in range(1, steps + 1):
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
        if ladder is not None and ladder['swap_every'] and step % ladder['swap_every'] == 0:
            parity = n_swaps % 2
            F_cross = F(curr, ladder['partner_T'][parity]) if energy == 'free_energy' else curr_F
            curr, curr_F = _host_swap(ladder, parity, curr, curr_F, F_cross, np.log(swap_rng.random(C)), n_swapped)
            n_swaps += 1
        if step % (skip_elems + 1) == 0:
            ens.append(curr.copy())
            ens_F.append(curr_F.copy())
    out = np.stack(ens), np.stack(ens_F), accepted / max(steps, 1)
    if ladder is not None:      # convergence is a question to the chains of one temperature: rung 0
        K = ladder['K']
        diag = (ensemble_diagnostics(np.ascontiguousarray(out[0][:, ::K]), np.ascontiguousarray(out[1][:, ::K])),) if diagnostics else ()
        return out + diag + (_ladder_summary(ladder, n_swapped),)
    return out + (ensemble_diagnostics(out[0], out[1]),) if diagnostics else out


def _host_swap(ladder, parity, curr, curr_F, F_cross, log_u, n_swapped):
    """One replica-exchange step in numpy (``ensemble_log_params_batch``, ``swap_every``): new (curr, curr_F); ``n_swapped``
    is counted in place at the lower chains.  The rule and its order of evaluation are those of ``sbm_pt_swap``."""
    i = np.flatnonzero(ladder['lower'][parity])
    j, T = i + 1, ladder['chain_T']
    with np.errstate(over='ignore', invalid='ignore'):
        bound = (curr_F[i] - F_cross[j]) / T[i] + (curr_F[j] - F_cross[i]) / T[j]
        take = np.isfinite(F_cross[i]) & np.isfinite(F_cross[j]) & (log_u[i] < bound)
    i, j = i[take], j[take]
    curr, new_F = curr.copy(), curr_F.copy()
    curr[i], curr[j] = curr[j].copy(), curr[i].copy()
    new_F[i], new_F[j] = F_cross[j], F_cross[i]
    n_swapped[i] += 1
    return curr, new_F


_DRAW_BLOCK = 256      # steps whose random numbers are drawn at once


def _swap_draws(draws, seeds, n_swaps, C, dev):
    """The log-uniform numbers of the device loop's swap steps, (n_swaps, C) on the device: ``draws[2]`` when given, else from
    a second ``torch.Generator``, seeded with a child of ``seeds`` -- the generator of ``_step_draws`` is not touched."""
    import torch
    if draws is not None:
        u = torch.as_tensor(draws[2] if isinstance(draws[2], torch.Tensor) else np.asarray(draws[2], dtype=np.float64))
        u = u.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(u.shape) != (n_swaps, C):
            raise ValueError("draws: log_u_swap must have shape (steps // swap_every, C) = %s, not %s" % ((n_swaps, C), tuple(u.shape)))
        return u
    gen = torch.Generator(device=dev)
    if seeds is None:
        gen.seed()
    else:
        child = np.random.SeedSequence(seeds).spawn(1)[0]
        gen.manual_seed(int(child.generate_state(1, dtype=np.uint64)[0] >> np.uint64(1)))
    return torch.log(torch.rand((n_swaps, C), dtype=torch.float64, device=dev, generator=gen))


def _step_draws(draws, seeds, steps, C, q, dev):
    """The random numbers of the device loops, step by step, (z (C, q), log_u (C,)) on the device: ``draws`` when given, else from
    a ``torch.Generator`` seeded with ``seeds``, in blocks of ``_DRAW_BLOCK`` steps -- in a block ``randn`` first, then ``log(rand)``."""
    import torch
    f64 = torch.float64
    if draws is not None:
        z_all, u_all = (torch.as_tensor(d if isinstance(d, torch.Tensor) else np.asarray(d, dtype=np.float64))
                        .to(device=dev, dtype=f64).contiguous() for d in (draws[0], draws[1]))
        if tuple(z_all.shape) != (steps, C, q) or tuple(u_all.shape) != (steps, C):
            raise ValueError("draws must have shapes (steps, C, q) = %s and (steps, C) = %s" % ((steps, C, q), (steps, C)))
        for k in range(steps):
            yield z_all[k], u_all[k]
        return
    gen = torch.Generator(device=dev)
    if seeds is None:
        gen.seed()
    else:
        gen.manual_seed(int(np.random.SeedSequence(seeds).generate_state(1, dtype=np.uint64)[0] >> np.uint64(1)))
    for first in range(0, steps, _DRAW_BLOCK):
        n = min(_DRAW_BLOCK, steps - first)
        z_blk = torch.randn((n, C, q), dtype=f64, device=dev, generator=gen)
        u_blk = torch.log(torch.rand((n, C), dtype=f64, device=dev, generator=gen))
        for k in range(n):
            yield z_blk[k], u_blk[k]


def _device_chains(project, starts, samp, steps, temperature, seeds, skip_elems, energy, draws, overrides, recalc=None,
                   box=None, diagnostics=False, ladder=None):
    """The loop of ``ensemble_log_params_batch(sampler='device')``: per step ``mh_propose``, the evaluation and ``mh_accept``
    (project/_evaluation.py) enqueued on the context's stream and no read-back; the record is a preallocated device array
    that the acceptance writes every (skip_elems + 1)-th step.
    ``recalc`` = dict(hess, cutoff, step_scale): the loop of ``sampler='device_recalc'``.  ``samp`` is not used, every chain
    keeps the axes (V, s, samp = V diag(s)) of its current point; the evaluation is ``sbm_jacobian_batch``, one more enqueue
    (``_evaluation.sampling_axes``) turns the trial points' Jacobians into axes, and the acceptance is the Hastings rule.
    ``box`` = dict(held, lower, upper, ...) (``held=`` / ``bounds=``): the proposal is ``sbm_mh_propose_box`` (``samp`` (C, q, q)
    goes per chain), its ``outside`` flags veto the chains in the acceptance, the axes are those of the free columns.  What
    is absent is None and reaches the library as NULL: without a box, the kernels and the bits of the loop before it had one.
    ``diagnostics``: two more enqueues per record (``_ensemble_diagnostics_dev``) ahead of the one synchronisation.
    ``ladder`` (``_temperature_ladder_arguments``; ``temperature`` is then None): the chains' temperatures are a device array
    and the entropy and the acceptance the ``_pt`` entries; a swap step is ``pt_swap`` after, for 'free_energy', one more
    state-only evaluation of ``curr`` and the entropy at the partners' temperatures -- enqueued like the rest."""
    import torch
    ev = DeviceEvaluator(project)
    dev = ev.dev
    ctx = project._model.device_model.ctx
    f64, i32 = torch.float64, torch.int32
    C, q = starts.shape
    free = energy == 'free_energy'
    if free:
        project._require_scale_factor_priors()
    host_loop = not one_device_call(project, overrides)

    to_dev = lambda a, dtype=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)      # noqa: E731
    curr = to_dev(starts)
    trial = torch.empty_like(curr)
    ax_c = ax_t = ax_status = row_scale = None
    if recalc is None:
        samp_c = to_dev(samp)
    else:
        # axes of the current points and of the trial points: V, s, samp
        ax_c, ax_t = ([torch.empty(sh, dtype=f64, device=dev) for sh in ((C, q, q), (C, q), (C, q, q))] for _ in range(2))
        ax_status = torch.empty((C,), dtype=i32, device=dev)
        samp_c = ax_c[2]
        inv_sigma = inverse_row_sigma(project)
        if inv_sigma is not None:       # the measurement rows of a reference_compat Jacobian come undivided by sigma
            row_scale = torch.ones((ev.RT,), dtype=f64, device=dev)
            row_scale[:ev.R] = to_dev(inv_sigma)
    buf = ev.buffers(C, jacobian=recalc is not None)
    jac = buf.get('jacobian')
    entropy = torch.empty((C,), dtype=f64, device=dev) if free else None
    n_acc = torch.zeros((C,), dtype=i32, device=dev)
    # the box on the device: only what was asked for -- the rest stays None, the library's NULL
    held_d = to_dev(box['held'], np.int32) if box is not None and box['any_held'] else None
    lower_d, upper_d = (to_dev(box['lower']), to_dev(box['upper'])) if box is not None and box['bounded'] else (None, None)
    outside = torch.empty((C,), dtype=i32, device=dev) if box is not None else None
    opts = None if host_loop else project._opts(**overrides)
    swaps = partner_T = entropy_x = n_swapped = None
    if ladder is not None:
        temperature = to_dev(ladder['chain_T'])
        if ladder['n_swaps']:
            swaps = _swap_draws(draws, seeds, ladder['n_swaps'], C, dev)
            n_swapped = torch.zeros((C,), dtype=i32, device=dev)
            if free:
                partner_T = [to_dev(t) for t in ladder['partner_T']]
                entropy_x = torch.empty((C,), dtype=f64, device=dev)

    def evaluate(th, T=temperature, entropy=entropy):
        """norms, status (and sims) of the C points ``th``; entropy of their simulations at ``T``, a number or one per chain;
        with ``recalc`` their Jacobians"""
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
        if free and ladder is not None:
            _lib.check(ev.lib.sbm_project_sf_entropy_pt(ev.proj, _lib.dev_ptr(sm), C, _lib.dev_ptr(T), _lib.dev_ptr(entropy), None),
                       'sbm_project_sf_entropy_pt')
        elif free:
            _lib.check(ev.lib.sbm_project_sf_entropy(ev.proj, _lib.dev_ptr(sm), C, T, _lib.dev_ptr(entropy), None),
                       'sbm_project_sf_entropy')
        return nr, st

    def axes(out, hess=None):
        """V, s, samp of the points whose Jacobians ``evaluate`` left in ``jac`` (or of one Hessian for all chains)"""
        source = dict(J=jac, row_scale=row_scale) if hess is None else dict(H=to_dev(hess))
        device_sampling_axes(ctx, cutoff=recalc['cutoff'], temperature=temperature, step_scale=recalc['step_scale'],
                             V=out[0], s=out[1], samp=out[2], status=ax_status, held=held_d, **source)

    nr, st = evaluate(curr)
    if recalc is not None:
        axes(ax_c, recalc['hess'])
    F_curr = finite_cost(nr, st, entropy).contiguous()
    every = skip_elems + 1
    ens = torch.empty((1 + steps // every, C, q), dtype=f64, device=dev)
    ens_F = torch.empty(ens.shape[:2], dtype=f64, device=dev)
    ens[0].copy_(curr)
    ens_F[0].copy_(F_curr)
    for step, (z, log_u) in enumerate(_step_draws(draws, seeds, steps, C, q, dev), 1):
        mh_propose(ctx, curr=curr, samp=samp_c, z=z, trial=trial, held=held_d, lower=lower_d, upper=upper_d, outside=outside)
        nr, st = evaluate(trial)
        if recalc is not None:
            axes(ax_t)
        kept = step % every == 0
        mh_accept(ctx, norms=nr, status=st, entropy=entropy, log_u=log_u, temperature=temperature, trial=trial, curr=curr,
                  F_curr=F_curr, n_accepted=n_acc, ens_slot=ens[step // every] if kept else None,
                  ens_F_slot=ens_F[step // every] if kept else None, veto=outside, axes_curr=ax_c, axes_trial=ax_t,
                  axes_status=ax_status)
        if swaps is not None and step % ladder['swap_every'] == 0:
            n = step // ladder['swap_every'] - 1                   # the n-th swap step, from 0
            F_cross = None
            if free:
                nr, st = evaluate(curr, partner_T[n % 2], entropy_x)
                F_cross = finite_cost(nr, st, entropy_x).contiguous()
            pt_swap(ctx, K=ladder['K'], parity=n % 2, temperature=temperature, F_cross=F_cross, log_u=swaps[n], curr=curr,
                    F_curr=F_curr, n_swapped=n_swapped, ens_slot=ens[step // every] if kept else None,
                    ens_F_slot=ens_F[step // every] if kept else None)
    if ladder is not None and diagnostics:      # the chains of rung 0: one temperature
        K = ladder['K']
        diag = _ensemble_diagnostics_dev(ctx, ens[:, ::K].contiguous(), ens_F[:, ::K].contiguous(), None, 1)
    else:
        diag = _ensemble_diagnostics_dev(ctx, ens, ens_F, None, 1) if diagnostics else None
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    out = ens.cpu().numpy(), ens_F.cpu().numpy(), n_acc.cpu().numpy() / max(steps, 1)
    if diagnostics:
        out += ({k: v.cpu().numpy() for k, v in diag.items()},)
    if ladder is not None:
        out += (_ladder_summary(ladder, n_swapped.cpu().numpy() if n_swapped is not None else np.zeros(C, dtype=np.int64)),)
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
    X = np.array(ens, dtype=np.float64)
    if X.ndim == 3:
        X = X.reshape(-1, X.shape[-1])
    if X.ndim != 2 or X.shape[0] == 0:
        raise ValueError("ensemble must have shape (n, q) or (n_kept, C, q), not %s" % (np.shape(ens),))
    n, q = X.shape
    if q > _lib.SAMPLING_AXES_MAX_Q:
        raise ValueError("pca_eig: %d parameters; sbm_sampling_axes holds q <= %d" % (q, _lib.SAMPLING_AXES_MAX_Q))
    X -= X.mean(axis=0)
    ctx = _lib.default_context()
    dev = torch.device('cuda', ctx.device)
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    eig = torch.empty((q,), dtype=torch.float64, device=dev)
    V = torch.empty((q, q), dtype=torch.float64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    device_sampling_axes(ctx, J=Xd, cutoff=0.0, temperature=1.0, step_scale=1.0, eig=eig, V=V, status=status)
    ctx.synchronize()
    torch.cuda.synchronize(dev)
    if int(status.item()) != 0:
        raise ValueError("pca_eig: the ensemble has entries that are not finite")
    with np.errstate(divide='ignore'):
        return n / (2.0 * eig.cpu().numpy()), V.cpu().numpy()


def pca_eig_log_params(ens):
    """``pca_eig`` of the logarithms of an ensemble of (positive) parameters (reference PCA_eig_log_params)."""
    return pca_eig(np.log(np.asarray(ens, dtype=np.float64)))
