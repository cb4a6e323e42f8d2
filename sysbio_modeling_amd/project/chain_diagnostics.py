"""Has a sampled ensemble converged?  ``autocorrelation`` (reference project/Ensembles.py:14-29) and ``ensemble_diagnostics``
(integrated autocorrelation time, effective sample size, split-R-hat) work on the record where the device samplers of
project/ensembles.py leave it (``sbm_chain_autocorr``, ``sbm_chain_summary``; kernels in csrc/sbm_chain_diagnostics.hpp)."""
import numpy as np

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
