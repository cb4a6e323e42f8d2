"""fit_batch(geodesic=...) on the configs[3] project, 256 starts x 100 iterations, beside the plain fit of the same starts:
median cost after 25 / 50 / 100 iterations, starts converged, accepted steps, the share of running starts accelerated by
iteration, the time of an iteration split into probe launch, geodesic kernel and trial launch, the slowest trajectory of
the trial launches, rho by iteration; wall time of both fits without trace; the probe's noise floor; and sbm_lm_geodesic
alone beside sbm_lm_trust_step_ex at 256 x 512 x 68 (docs/history.md, "Geodesic acceleration")."""
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from sysbio_modeling_amd import _lib, models_zoo  # noqa: E402
from sysbio_modeling_amd.model import OdeModel  # noqa: E402
from sysbio_modeling_amd.project._evaluation import geodesic_step, trust_step  # noqa: E402
from sysbio_modeling_amd.symbolic import zoo_model  # noqa: E402

TOL = dict(ftol=1.49012e-8, xtol=1.49012e-8)


def kernels_alone(V=256, M=512, q=68, reps=20):
    """Both kernels on the same random J, r; radii that leave half of the starts damped.  Median of `reps` launches after
    three warm-up launches, timed with events on the context's stream."""
    dev, f64, i32 = 'cuda', torch.float64, torch.int32
    g = torch.Generator(device=dev).manual_seed(3)
    J = torch.randn((V, M, q), dtype=f64, device=dev, generator=g)
    r = torch.randn((V, M), dtype=f64, device=dev, generator=g)
    theta = torch.randn((V, q), dtype=f64, device=dev, generator=g)
    radius = torch.where(torch.arange(V, device=dev) % 2 == 0, 1e6, 0.3).to(f64).contiguous()
    ctx = _lib.default_context()
    z = lambda *s, dt=f64: torch.zeros(s, dtype=dt, device=dev)          # noqa: E731
    D, lam, delta, trial, pred, dxn, gtx, st = z(V, q), z(V), z(V, q), z(V, q), z(V), z(V), z(V), z(V, dt=i32)

    def step():
        D.zero_()
        lam.zero_()
        trust_step(ctx, J=J, r=r, dscale=D, radius=radius, lam=lam, delta=delta, pred=pred, dxnorm=dxn, status=st, max_step=2.0,
                   theta=theta, trial=trial, gtx=gtx)
    step()
    r_probe = r + 0.1 * torch.einsum('vmq,vq->vm', J, delta) + 0.005 * 0.05 * torch.randn((V, M), dtype=f64, device=dev, generator=g)
    kept = [t.clone() for t in (delta, trial, pred, dxn, gtx)]
    acc, rho, n_acc = z(V, dt=i32), z(V), z(V, dt=i32)

    def timed(launch, prepare):
        times = []
        for i in range(reps + 3):
            prepare()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                times.append(1e3 * a.elapsed_time(b))
        return np.median(times), np.min(times), np.max(times)
    restore = lambda: [t.copy_(k) for t, k in zip((delta, trial, pred, dxn, gtx), kept)]          # noqa: E731
    t_geo = timed(lambda: geodesic_step(ctx, J=J, r=r, r_probe=r_probe, dscale=D, lam=lam, step_status=st, theta=theta, delta=delta,
                                        trial=trial, pred=pred, dxnorm=dxn, gtx=gtx, accel_status=acc, h=0.1, alpha=0.75,
                                        max_step=2.0, ratio=rho, n_accel=n_acc), restore)
    t_step = timed(lambda: trust_step(ctx, J=J, r=r, dscale=D, radius=radius, lam=lam, delta=delta, pred=pred, dxnorm=dxn, status=st,
                                      max_step=2.0, theta=theta, trial=trial, gtx=gtx), lambda: (D.zero_(), lam.zero_()))
    print('kernels alone at %d x %d x %d, us (median, min, max of %d): sbm_lm_geodesic %.0f %.0f %.0f; sbm_lm_trust_step_ex '
          '%.0f %.0f %.0f; statuses of the geodesic launch %s; damped starts %d'
          % (V, M, q, reps, *t_geo, *t_step, np.bincount(acc.cpu().numpy(), minlength=6).tolist(), int((lam > 0).sum())), flush=True)


def main():
    method = sys.argv[1] if len(sys.argv) > 1 else 'dopri45'
    gm = zoo_model('cascade20')
    m = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        proj, th0 = models_zoo.cascade_config4_project(m, reference_compat=False)
    starts = th0[None, :] + 0.15 * np.random.default_rng(1).standard_normal((256, th0.size))
    V = starts.shape[0]
    for geo in (None, True):
        proj.fit_batch(starts[:8], max_iter=3, method=method, geodesic=geo)          # warm-up: plugin, buffers, first launches
    # the probe's noise floor: the state-only kernel's residuals against the sensitivity kernel's at the same points
    a = proj.evaluate_batch(starts, jacobian=True, want=('jacobian',), method=method)
    b = proj.evaluate_batch(starts, method=method)
    ra, rb = (np.asarray(x['residuals'].cpu() if hasattr(x['residuals'], 'cpu') else x['residuals']) for x in (a, b))
    noise = np.linalg.norm(rb - ra, axis=1) / np.linalg.norm(ra, axis=1)
    print('noise floor |r_base - r| / |r| over the %d starts: median %.3g, 90 %% %.3g, max %.3g'
          % (V, np.median(noise), np.quantile(noise, 0.9), noise.max()), flush=True)
    traced = {}
    for geo in (None, True):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            fit = proj.fit_batch(starts, max_iter=100, method=method, trace=True, geodesic=geo, **TOL)
        traced[geo] = fit
        hist = fit['history']
        med = {n: hist[min(n, len(hist)) - 1]['cost_median'] for n in (25, 50, 100)}
        print('geodesic=%s: iterations %d, median cost after 25 / 50 / 100: %.3f / %.3f / %.3f, final min %.3f median %.3f; '
              'converged %d of %d; accepted steps %d; trial launches: %.1f ms in all, slowest trajectory max %d median %d'
              % (geo, len(hist), med[25], med[50], med[100], fit['cost'].min(), np.median(fit['cost']), fit['converged'].sum(), V,
                 sum(h['accepted'] for h in hist), sum(h['launch']['ms'] for h in hist),
                 max(h['launch']['steps_max'] for h in hist), int(np.median([h['launch']['steps_max'] for h in hist]))), flush=True)
        if geo:
            print('  probe launches %.1f ms, geodesic kernel %.2f ms in all (per iteration: probe median %.2f ms, kernel median '
                  '%.3f ms, trial median %.2f ms); accelerated steps per start: median %d, max %d'
                  % (sum(h['probe_ms'] for h in hist), sum(h['geodesic_ms'] for h in hist), np.median([h['probe_ms'] for h in hist]),
                     np.median([h['geodesic_ms'] for h in hist]), np.median([h['launch']['ms'] for h in hist]),
                     np.median(fit['n_accelerated']), fit['n_accelerated'].max()))
            for lo in range(0, len(hist), 10):
                blk = hist[lo:lo + 10]
                print('  iterations %3d-%3d: accelerated %5.1f %% of the running starts, accepted %5.1f %%, rho p10 / median / p90 '
                      '%.3g / %.3g / %.3g' % (lo, lo + len(blk) - 1, 100.0 * sum(h['accelerated'] for h in blk) / max(1, sum(h['live'] for h in blk)),
                                              100.0 * sum(h['accepted'] for h in blk) / max(1, sum(h['live'] for h in blk)),
                                              np.nanmedian([h['rho_p10'] for h in blk]), np.nanmedian([h['rho_median'] for h in blk]),
                                              np.nanmedian([h['rho_p90'] for h in blk])), flush=True)
    # wall time without trace: three runs each, alternating
    wall = {None: [], True: []}
    for _ in range(3):
        for geo in (None, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                f = proj.fit_batch(starts, max_iter=100, method=method, geodesic=geo, **TOL)
            torch.cuda.synchronize()
            wall[geo].append(time.perf_counter() - t0)
        last = f
    print('wall time of the fit, 3 runs each: plain %s s, geodesic %s s (median cost of the last geodesic run %.3f, evaluations %d)'
          % (np.round(wall[None], 3).tolist(), np.round(wall[True], 3).tolist(), np.median(last['cost']), last['n_evaluations']),
          flush=True)
    kernels_alone()


if __name__ == '__main__':
    main()
