"""From a sampled ensemble (project/ensembles.py) to trajectories with uncertainty bands (reference project/Ensembles.py:277-361;
``project`` stands where SloppyCell's ``net`` stood): ``ensemble_trajs`` integrates every member on a time grid of the caller's
choice, ``traj_ensemble_stats`` / ``traj_ensemble_quantiles`` / ``net_ensemble_trajs`` reduce over the members with
``sbm_ensemble_stats`` on the device (failed members left out, as ``few_ensemble_trajs`` drops NaN trajectories),
``ensemble_predictions`` does both experiment by experiment and adds the bands of the scaled observables."""
import numpy as np

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
