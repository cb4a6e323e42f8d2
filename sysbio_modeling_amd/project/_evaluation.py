"""What every host loop around the project kernels shares (project/fitting.py, project/ensembles.py, base_project.py): the
one place that calls ``sbm_residuals_batch`` / ``sbm_jacobian_batch``, the output set those calls fill, and the three small
rules the loops apply to what comes back.  torch is imported inside the functions: the module loads without a GPU."""
from __future__ import annotations

import ctypes

from .. import _control, _lib


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
        p = _lib.dev_ptr
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
