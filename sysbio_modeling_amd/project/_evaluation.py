"""What every host loop around the project kernels shares (project/fitting.py, project/ensembles.py, base_project.py): the
one place that calls ``sbm_residuals_batch`` / ``sbm_jacobian_batch``, the output set those calls fill, the three small
rules the loops apply to what comes back, and the other per-step device calls of the loops (``trust_step``, ``geodesic_step``, ``mh_propose``,
``mh_accept``, ``pt_swap``, ``sampling_axes``), each written once.  torch is imported inside the functions: it loads without a GPU."""
from __future__ import annotations

import ctypes

from .. import _control, _lib

p = _lib.dev_ptr          # void* of a device tensor; None is NULL


class DeviceEvaluator(object):
    """The project on its device, ready to be evaluated into buffers the caller keeps: handle, library, device and the
    sizes R (measurement rows), RT (rows with the prior rows), G (scale-factor groups) and q, read once.  Build one per
    call of a public entry point: setting a prior changes RT and reloads the project."""

    def __init__(self, project):
        import torch
        self.proj = project._device()
        self.lib = _lib.load_library()
        self.dev = torch.device('cuda', project._model.device_model.ctx.device)
        self.R, self.RT = project.n_project_residuals, project.n_total_rows
        self.G, self.q = project._n_sf_groups(), project.n_project_params

    def buffers(self, n, jacobian=False, model_jacobian=False, gradient=False, sf_gradient=False):
        """Uninitialised outputs for ``n`` project vectors, under the names ``evaluate_batch`` returns them by:
        residuals (n, RT), sims (n, R), sf (n, G) -- no bytes without scale factors --, norms (n,), status and n_steps
        (n,) int32; on request jacobian (n, RT, q), model_jacobian (n, R, q), gradient (n, q) and, where there are scale
        factors, sf_gradient (n, G, q)."""
        import torch
        f64, i32, dev = torch.float64, torch.int32, self.dev
        buf = {'residuals': torch.empty((n, self.RT), dtype=f64, device=dev),
               'sims': torch.empty((n, self.R), dtype=f64, device=dev),
               'sf': torch.empty((n, self.G), dtype=f64, device=dev),
               'norms': torch.empty((n,), dtype=f64, device=dev),
               'status': torch.empty((n,), dtype=i32, device=dev),
               'n_steps': torch.empty((n,), dtype=i32, device=dev)}
        if jacobian:
            buf['jacobian'] = torch.empty((n, self.RT, self.q), dtype=f64, device=dev)
        if model_jacobian:
            buf['model_jacobian'] = torch.empty((n, self.R, self.q), dtype=f64, device=dev)
        if gradient:
            buf['gradient'] = torch.empty((n, self.q), dtype=f64, device=dev)
        if sf_gradient and self.G:
            buf['sf_gradient'] = torch.empty((n, self.G, self.q), dtype=f64, device=dev)
        return buf

    def run(self, theta, opts, buf, jacobian):
        """Integrate the rows of ``theta`` (n, q), float64 and contiguous on the device, with the options ``opts``
        (``Project._opts``) into ``buf``: ``sbm_jacobian_batch`` with ``jacobian``, else ``sbm_residuals_batch``.  An
        output ``buf`` does not hold is not computed.  Enqueues only."""
        n = int(theta.shape[0])
        sf = p(buf['sf']) if self.G else None
        if jacobian:
            _lib.check(self.lib.sbm_jacobian_batch(self.proj, p(theta), n, ctypes.byref(opts), p(buf['sims']), p(buf['residuals']),
                                                   p(buf['jacobian']), p(buf.get('model_jacobian')), sf, p(buf.get('sf_gradient')),
                                                   p(buf['norms']), p(buf.get('gradient')), p(buf['status']), p(buf['n_steps'])),
                       'sbm_jacobian_batch')
        else:
            _lib.check(self.lib.sbm_residuals_batch(self.proj, p(theta), n, ctypes.byref(opts), p(buf['sims']), p(buf['residuals']),
                                                    sf, p(buf['norms']), p(buf['status']), p(buf['n_steps'])), 'sbm_residuals_batch')


def usable(values, status):
    """Mask of the vectors whose ``values`` (norms, costs, energies) count: finite, from an integration that ended with
    status 0."""
    import torch
    return torch.isfinite(values) & (status == 0)


def finite_cost(norms, status, entropy=None):
    """0.5 * norms (less ``entropy``, for a free energy) where that is `usable`, +inf elsewhere."""
    import torch
    cost = 0.5 * norms if entropy is None else 0.5 * norms - entropy
    return torch.where(usable(cost, status), cost, torch.full_like(cost, float('inf')))


def one_device_call(project, overrides):
    """Whether an evaluation with these integrator overrides is one device call -- not one of the host control loops of
    ``_control.py`` (method='auto', the host-controlled implicit methods)."""
    method = str(project._options(**overrides).get('method', 'dopri45')).lower()
    return method not in _control.IMPLICIT_CONTROLLED + _control.AUTO


def inverse_row_sigma(project):
    """1 / sigma per measurement row (numpy) where the project's Jacobian comes undivided by it (``reference_compat``,
    SURVEY 8a quirk 3), else None."""
    return 1.0 / project.descriptor_arrays()['row_sigma'] if project.reference_compat else None


# ---------------------------------------------------------------------------------------------
# The per-step device calls of the fit and sampler loops.  Every pointer of the C ABI is a void*: the order of the
# tensors is checked here and nowhere else (tests/test_gpu_device_steps.py), so the loops pass them by name.  ``ctx`` is
# the ``_lib.Context`` whose stream the launch goes to; sizes are read from the shapes; None is NULL; enqueue only.
# ---------------------------------------------------------------------------------------------
def trust_step(ctx, *, J, r, dscale, radius, lam, delta, pred, dxnorm, status, row_scale=None, skip=None, max_step=0.0,
               theta=None, trial=None, gtx=None, held=None, lower=None, upper=None):
    """One trust-region step per start from J (V, M, q) and r (V, M): ``sbm_lm_trust_step_bounded`` with ``lower`` /
    ``upper`` (V, q), else ``sbm_lm_trust_step_held`` with the int32 mask ``held`` (V, q) or NULL, which is
    ``sbm_lm_trust_step_ex`` -- the same kernel, the same bits.  Without ``theta`` / ``trial`` / ``gtx`` / ``skip`` /
    ``row_scale`` it is ``sbm_lm_trust_step``.  include/sbm.h says what each tensor holds."""
    V, M, q = J.shape
    args = (ctx.handle, p(J), p(r), p(dscale), p(radius), p(lam), V, M, q, p(row_scale), p(skip), float(max_step), p(theta),
            p(trial), p(delta), p(pred), p(dxnorm), p(gtx), p(status), p(held))
    if lower is not None or upper is not None:
        _lib.check(ctx.lib.sbm_lm_trust_step_bounded(*args, p(lower), p(upper), None), 'sbm_lm_trust_step_bounded')
    else:
        _lib.check(ctx.lib.sbm_lm_trust_step_held(*args), 'sbm_lm_trust_step_held')


def geodesic_step(ctx, *, J, r, r_probe, dscale, lam, step_status, theta, delta, trial, pred, dxnorm, gtx, accel_status, h, alpha,
                  r_base=None, status_base=None, status_probe=None, row_scale=None, skip=None, held=None, max_step=0.0,
                  ratio=None, n_accel=None):
    """``sbm_lm_geodesic``: the geodesic acceleration of the steps `trust_step` just wrote into ``delta`` / ``trial`` /
    ``pred`` / ``dxnorm`` / ``gtx`` (with the same J, r, row_scale, skip, held, max_step and theta; ``dscale`` and ``lam`` as
    it left them, ``step_status`` its status).  ``r_base`` / ``r_probe`` (V, M): the residuals at theta and theta + h delta
    from one state-only integration, ``status_base`` / ``status_probe`` its statuses.  include/sbm.h says what each tensor
    holds and what ``accel_status`` means."""
    V, M, q = J.shape
    _lib.check(ctx.lib.sbm_lm_geodesic(ctx.handle, p(J), p(r), p(r_base), p(r_probe), p(status_base), p(status_probe), p(dscale),
                                       p(lam), V, M, q, p(row_scale), p(skip), p(step_status), p(held), float(h), float(alpha),
                                       float(max_step), p(theta), p(delta), p(trial), p(pred), p(dxnorm), p(gtx),
                                       p(accel_status), p(ratio), p(n_accel)), 'sbm_lm_geodesic')


def mh_propose(ctx, *, curr, samp, z, trial, held=None, lower=None, upper=None, outside=None):
    """trial = curr + samp z for C chains: ``samp`` (q, q) shared or (C, q, q) one matrix per chain.  With the int32 flags
    ``outside`` (C,) ``sbm_mh_propose_box`` (``held`` int32 (C, q), ``lower`` / ``upper`` (C, q), each nullable), else
    ``sbm_mh_propose``: two kernels, so the choice is made here."""
    C, q = curr.shape
    per_chain = int(samp.dim() == 3)
    if outside is not None:
        _lib.check(ctx.lib.sbm_mh_propose_box(ctx.handle, p(curr), p(samp), per_chain, p(z), C, q, p(held), p(lower), p(upper),
                                              p(trial), p(outside)), 'sbm_mh_propose_box')
    else:
        _lib.check(ctx.lib.sbm_mh_propose(ctx.handle, p(curr), p(samp), per_chain, p(z), C, q, p(trial)), 'sbm_mh_propose')


def mh_accept(ctx, *, norms, status, log_u, temperature, trial, curr, F_curr, n_accepted, entropy=None, ens_slot=None,
              ens_F_slot=None, veto=None, axes_curr=None, axes_trial=None, axes_status=None):
    """Accept or reject the C trial points and move ``curr`` / ``F_curr`` / ``n_accepted`` (and the record slots, when
    given): ``sbm_mh_accept_ex``, or with ``axes_curr`` / ``axes_trial`` = (V, s, samp) of the candidate density at the two
    ends and the trial axes' ``axes_status`` ``sbm_mh_accept_hastings_ex``, which moves the axes with the point.  ``veto``
    int32 (C,) or NULL: the unsuffixed entry points are these with NULL.  ``temperature``: a number, or a float64 device
    tensor (C,) with one temperature per chain -- ``sbm_mh_accept_pt``, the Metropolis rule only."""
    C, q = curr.shape
    if hasattr(temperature, 'data_ptr'):
        if axes_curr is not None:
            raise ValueError("mh_accept: one temperature per chain goes with the Metropolis rule, not with axes")
        if tuple(temperature.shape) != (C,):
            raise ValueError("mh_accept: temperature must be a number or have shape (%d,), not %s" % (C, tuple(temperature.shape)))
        _lib.check(ctx.lib.sbm_mh_accept_pt(ctx.handle, p(norms), p(status), p(entropy), p(log_u), p(temperature), C, q, p(trial),
                                            p(curr), p(F_curr), p(n_accepted), p(ens_slot), p(ens_F_slot), p(veto)),
                   'sbm_mh_accept_pt')
        return
    args = (ctx.handle, p(norms), p(status), p(entropy), p(log_u), float(temperature), C, q, p(trial), p(curr), p(F_curr),
            p(n_accepted), p(ens_slot), p(ens_F_slot))
    if axes_curr is not None:
        _lib.check(ctx.lib.sbm_mh_accept_hastings_ex(*args, *(p(a) for a in axes_curr), *(p(a) for a in axes_trial),
                                                     p(axes_status), p(veto)), 'sbm_mh_accept_hastings_ex')
    else:
        _lib.check(ctx.lib.sbm_mh_accept_ex(*args, p(veto)), 'sbm_mh_accept_ex')


def pt_swap(ctx, *, K, parity, temperature, log_u, curr, F_curr, n_swapped, F_cross=None, ens_slot=None, ens_F_slot=None):
    """``sbm_pt_swap``: one replica-exchange step of the C / K temperature ladders in ``curr`` (C, q) -- the pairs of rungs
    (k, k + 1) with k % 2 == ``parity``.  ``temperature`` (C,) the chains' own, ``F_cross`` (C,) the energies of their points
    at the partners' temperatures (None: ``F_curr``), ``log_u`` (C,) read at the lower chain of a pair, ``n_swapped`` int32
    (C,) counted there; the record slots of a kept step, when given, get the exchanged rows."""
    C, q = curr.shape
    _lib.check(ctx.lib.sbm_pt_swap(ctx.handle, C, q, int(K), int(parity), p(temperature), p(F_cross), p(log_u), p(curr), p(F_curr),
                                   p(n_swapped), p(ens_slot), p(ens_F_slot)), 'sbm_pt_swap')


def sampling_axes(ctx, *, status, cutoff, temperature, step_scale, J=None, row_scale=None, H=None, eig=None, V=None, s=None,
                  samp=None, held=None):
    """Axes of the candidate density of the C = len(status) chains, ``sbm_sampling_axes_held`` (``held`` int32 (C, q) or
    NULL, which is ``sbm_sampling_axes``): from exactly one of the Jacobians ``J`` (C, M, q) (with ``row_scale`` (M,) or
    NULL) and the Hessian ``H`` (q, q) for all chains or (C, q, q); the outputs ``eig``, ``V``, ``s``, ``samp`` as given."""
    _lib.check(ctx.lib.sbm_sampling_axes_held(ctx.handle, p(J), p(row_scale), p(H), int(H is not None and H.dim() == 3),
                                              int(status.shape[0]), int(J.shape[-2]) if J is not None else 0,
                                              int((J if J is not None else H).shape[-1]),
                                              float(cutoff), float(temperature), float(step_scale), p(eig), p(V), p(s), p(samp),
                                              p(status), p(held)), 'sbm_sampling_axes_held')
