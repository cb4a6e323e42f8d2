"""sbm_lm_trust_step_held -- the trust-region step over the free parameters of every start only -- against
sbm_lm_trust_step_ex on the problem with the held columns deleted (the kernel compacts the system, so the two do the same
arithmetic: bitwise equality is expected and printed, 1e-13 asserted), and the loop built from it (step, residuals and
Jacobian in torch, sbm_lm_update, sbm_lm_accept) against MINPACK on reduced problems."""
import numpy as np
import pytest

from oracle import lmder_oracle as lo

pytestmark = pytest.mark.gpu

REL = 1.0e-13          # the float bound of tests/test_gpu_lm_bookkeeping.py for these kernels


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return np.inf
    if np.array_equal(got, want):
        return 0.0
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 5e-324)))


def trust_step(J, r, dscale, radius, lam, theta, row_scale=None, skip=None, max_step=0.0, held='ex'):
    """One launch on numpy inputs.  ``held='ex'``: sbm_lm_trust_step_ex; otherwise sbm_lm_trust_step_held with that mask
    (None: a NULL pointer).  Returns the outputs as numpy arrays (dscale and lam are the in / out arrays after the call)."""
    import torch
    from sysbio_modeling_amd import _lib
    dev, f64, i32 = 'cuda', torch.float64, torch.int32
    V, M, q = J.shape
    t = lambda x, dt=f64: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)     # noqa: E731
    Jd, rd, Dd, Rd, Ld, thd, rsd, skd = t(J), t(r), t(dscale), t(radius), t(lam), t(theta), t(row_scale), t(skip, i32)
    delta, trial = (torch.full((V, q), -77.0, dtype=f64, device=dev) for _ in range(2))
    pred, dxn, gtx = (torch.full((V,), -77.0, dtype=f64, device=dev) for _ in range(3))
    st = torch.full((V,), -7, dtype=i32, device=dev)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    args = (ctx.handle, p(Jd), p(rd), p(Dd), p(Rd), p(Ld), V, M, q, p(rsd), p(skd), float(max_step), p(thd), p(trial), p(delta),
            p(pred), p(dxn), p(gtx), p(st))
    if isinstance(held, str):
        _lib.check(ctx.lib.sbm_lm_trust_step_ex(*args), 'sbm_lm_trust_step_ex')
    else:
        hd = t(np.asarray(held, dtype=np.int32), i32) if held is not None else None
        _lib.check(ctx.lib.sbm_lm_trust_step_held(*args, p(hd)), 'sbm_lm_trust_step_held')
    torch.cuda.synchronize()
    return dict(delta=delta.cpu().numpy(), trial=trial.cpu().numpy(), pred=pred.cpu().numpy(), dxnorm=dxn.cpu().numpy(),
                gtx=gtx.cpu().numpy(), status=st.cpu().numpy(), dscale=Dd.cpu().numpy(), lam=Ld.cpu().numpy())


def lmpar_accepts(out, v, radius, cols):
    """lmpar's own acceptance condition for start v of a launch: | ||D x|| - Delta | <= 0.1 Delta, or lambda = 0 with the
    step inside."""
    dxn = np.linalg.norm(out['dscale'][v][cols] * out['delta'][v][cols])
    return abs(dxn - radius) <= 0.1 * radius * (1 + 1e-12) or (out['lam'][v] == 0.0 and dxn <= 1.1 * radius)


def compare_with_reduced(J, r, dscale, radius, lam, theta, held, row_scale=None, max_step=0.0, what=''):
    """The held call on the full arrays (ONE launch, every mask in it) against one sbm_lm_trust_step_ex call per start on
    the arrays with that start's held columns deleted.  Returns the held call's outputs."""
    V, M, q = J.shape
    held = np.asarray(held, dtype=bool)
    full = trust_step(J, r, dscale, radius, lam, theta, row_scale, None, max_step, held=held.astype(np.int32))
    bitwise, aside, compared, worst = True, 0, 0, 0.0
    for v in range(V):
        free = np.nonzero(~held[v])[0]
        hv = np.nonzero(held[v])[0]
        where = '%sstart %d (%d free)' % (what, v, free.size)
        # held columns: exactly 0 / theta / 0, whatever else happens
        assert np.all(full['delta'][v, hv] == 0.0) and np.array_equal(full['trial'][v, hv], theta[v, hv]), where
        assert np.all(full['dscale'][v, hv] == 0.0), where
        if free.size == 0:
            assert full['status'][v] == 2 and full['pred'][v] == 0.0 and full['dxnorm'][v] == 0.0 and full['gtx'][v] == 0.0, where
            assert full['lam'][v] == lam[v], where
            continue
        red = trust_step(J[v:v + 1][:, :, free], r[v:v + 1], dscale[v:v + 1, free], radius[v:v + 1], lam[v:v + 1],
                         theta[v:v + 1, free], row_scale, None, max_step, held='ex')
        compared += 1
        assert full['status'][v] == red['status'][0], (where, full['status'][v], red['status'][0])
        if rel_err(full['lam'][v], red['lam'][0]) > REL:
            # another lambda: tolerable only if both are answers lmpar itself would accept (none expected with compaction)
            assert full['status'][v] == 0 and lmpar_accepts(full, v, radius[v], free) and \
                lmpar_accepts(red, 0, radius[v], np.arange(free.size)), (where, full['lam'][v], red['lam'][0])
            aside += 1
            continue
        pairs = [(full[k][v, free], red[k][0]) for k in ('delta', 'trial', 'dscale')] + \
                [(full[k][v], red[k][0]) for k in ('pred', 'dxnorm', 'gtx', 'lam')]
        errs = [rel_err(a, b) for a, b in pairs]
        worst = max([worst] + errs)
        bitwise = bitwise and all(np.array_equal(a, b) for a, b in pairs)
        assert max(errs) <= REL, (where, errs)
    print('%s%d starts against the reduced problem: bitwise equal: %s, worst relative error %.3g, set aside %d'
          % (what, compared, bitwise, worst, aside))
    assert aside <= 0.02 * compared, (aside, compared)
    return full


def test_held_step_equals_the_step_on_the_reduced_problem_every_mask_in_one_launch():
    """(V, M, q) = (8, 30, 12): one triangle entry per thread, one row tile.  Eight masks in ONE launch: none held, the
    first column, the last, two adjacent, all but one (nf = 1), all (nf = 0: status 2), two random.  Radii from far
    inside to far outside the Gauss-Newton step, so that lambda = 0 and lambda > 0 both occur; a scaling and a poor lambda
    carried in."""
    rng = np.random.default_rng(11)
    V, M, q = 8, 30, 12
    J = rng.standard_normal((V, M, q))
    r = rng.standard_normal((V, M))
    theta = rng.standard_normal((V, q))
    radius = np.array([1e3, 1e-2, 5.0, 1e6, 1.0, 1e8, 0.3, 2e-1])
    dscale = np.zeros((V, q))
    dscale[2] = 3.0 * np.linalg.norm(J[2], axis=0)
    lam = np.zeros(V)
    lam[6] = 7.0
    held = np.zeros((V, q), dtype=bool)
    held[1, 0] = True
    held[2, q - 1] = True
    held[3, 5:7] = True
    held[4] = True
    held[4, 7] = False
    held[5] = True
    held[6] = rng.random(q) < 0.4
    held[7] = rng.random(q) < 0.6
    assert 0 < held[6].sum() < q and 0 < held[7].sum() < q
    full = compare_with_reduced(J, r, dscale, radius, lam, theta, held)
    solved = full['status'] == 0
    assert solved.sum() == 7 and full['status'][5] == 2
    assert np.any(full['lam'][solved] == 0.0) and np.any(full['lam'][solved] > 0.0)      # both branches of lmpar


def test_held_step_with_row_scale_and_a_clip_that_binds_several_entries_per_thread():
    """(6, 45, 40): 820 triangle entries over 256 threads, two row tiles with a remainder (32 + 13).  1 held and 17 held;
    row_scale, and a max_step that clips."""
    rng = np.random.default_rng(12)
    V, M, q = 6, 45, 40
    J = rng.standard_normal((V, M, q))
    r = rng.standard_normal((V, M))
    rs = rng.uniform(0.5, 2.0, M)
    theta = rng.standard_normal((V, q))
    radius = np.array([1e3, 1e-2, 5.0, 1e6, 0.3, 1e3])
    held = np.zeros((V, q), dtype=bool)
    for v, c in ((0, 0), (1, q - 1), (2, 20)):
        held[v, c] = True
    for v in (3, 4, 5):
        held[v, rng.choice(q, 17, replace=False)] = True
    assert held.sum(axis=1).tolist() == [1, 1, 1, 17, 17, 17]
    max_step = 0.05
    full = compare_with_reduced(J, r, np.zeros((V, q)), radius, np.zeros(V), theta, held, row_scale=rs, max_step=max_step)
    assert np.all(full['status'] == 0)
    assert np.any(np.abs(full['delta']) == max_step) and np.all(np.abs(full['delta']) <= max_step)      # the clip binds


def test_held_step_at_the_largest_q():
    """(2, 20, 128), 1 held: the LDS budget at the largest q the entry point admits (16-row tile + the index list): the
    launch succeeds, and equals the 127-column problem."""
    rng = np.random.default_rng(13)
    V, M, q = 2, 20, 128
    J = rng.standard_normal((V, M, q))
    r = rng.standard_normal((V, M))
    theta = rng.standard_normal((V, q))
    held = np.zeros((V, q), dtype=bool)
    held[0, 127] = True
    held[1, 64] = True
    full = compare_with_reduced(J, r, np.zeros((V, q)), np.array([1.0, 1e-2]), np.zeros(V), theta, held)
    assert np.all(full['status'] == 0)


def test_held_null_is_the_ex_entry_point_and_a_skipped_start_is_left_alone():
    """held = NULL: every output array_equal to sbm_lm_trust_step_ex on the same inputs.  skip together with a mask: the
    skipped start keeps its dscale and lambda, delta = 0, trial = theta, status 2."""
    rng = np.random.default_rng(14)
    V, M, q = 5, 33, 23
    J = rng.standard_normal((V, M, q))
    r = rng.standard_normal((V, M))
    rs = rng.uniform(0.5, 2.0, M)
    theta = rng.standard_normal((V, q))
    radius = np.array([1e3, 1e-2, 5.0, 0.3, 1.0])
    dscale = rng.uniform(0.0, 2.0, (V, q))
    lam = np.array([0.0, 0.5, 0.0, 2.0, 0.0])
    skip = np.array([0, 0, 1, 0, 0], dtype=np.int32)
    a = trust_step(J, r, dscale, radius, lam, theta, rs, skip, 0.05, held=None)
    b = trust_step(J, r, dscale, radius, lam, theta, rs, skip, 0.05, held='ex')
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    held = rng.random((V, q)) < 0.3
    held[2, 3] = True
    c = trust_step(J, r, dscale, radius, lam, theta, rs, skip, 0.05, held=held.astype(np.int32))
    assert c['status'].tolist() == [0, 0, 2, 0, 0]
    assert np.array_equal(c['dscale'][2], dscale[2]) and c['lam'][2] == lam[2]
    assert np.all(c['delta'][2] == 0.0) and np.array_equal(c['trial'][2], theta[2]) and c['pred'][2] == 0.0
    for v in (0, 1, 3, 4):
        assert np.all(c['delta'][v, held[v]] == 0.0) and np.all(c['dscale'][v, held[v]] == 0.0)
        assert np.all(c['dscale'][v, ~held[v]] > 0.0)


def reduced_minpack_baseline(probs, held_col):
    """scipy.optimize.leastsq on every (problem, start) with parameter held_col(pb, s) fixed at its starting value: c* per
    start from ftol = xtol = 1e-14, taken both from the start and from the default-tolerance solution; a start whose two
    tight solutions differ by more than 1e-6 relative is dropped.  Returns (cstar [P][8], keep [P][8], MINPACK's worst excess
    (cost - c*) / (ftol c*) at default tolerances over the kept starts)."""
    from scipy.optimize import leastsq
    cstar, keep, worst = np.zeros((len(probs), 8)), np.zeros((len(probs), 8), dtype=bool), 0.0
    for i, pb in enumerate(probs):
        for s, x0 in enumerate(pb.starts):
            free = np.array([c for c in range(pb.q) if c != held_col(pb, s)])

            def full(z, x0=x0, free=free):
                x = x0.copy()
                x[free] = z
                return x
            fun = lambda z: pb.fun(full(z))                      # noqa: E731
            jac = lambda z: pb.jac(full(z))[:, free]             # noqa: E731
            half = lambda z: 0.5 * float(fun(z) @ fun(z))        # noqa: E731
            z0 = x0[free]
            zt = leastsq(fun, z0, Dfun=jac, ftol=1e-14, xtol=1e-14, gtol=0.0, maxfev=5000)[0]
            zd = leastsq(fun, z0, Dfun=jac)[0]
            zt2 = leastsq(fun, zd, Dfun=jac, ftol=1e-14, xtol=1e-14, gtol=0.0, maxfev=5000)[0]
            cstar[i, s] = min(half(zt), half(zt2))
            keep[i, s] = np.linalg.norm(zt - zt2) <= 1e-6 * (1 + np.linalg.norm(zt))
            if keep[i, s]:
                worst = max(worst, (half(zd) - cstar[i, s]) / (lo.FTOL * cstar[i, s]))
    return cstar, keep, worst


def test_held_loop_reaches_minpacks_minimum_of_the_reduced_problems():
    """The fitting loop with held parameters, without an ODE: sbm_lm_trust_step_held, residuals and Jacobian of the trial
    points in torch, sbm_lm_update, sbm_lm_accept, on the three problems of oracle/lmder_oracle.py padded to one batch
    (V = 24, M = 30, q = 12, a padding parameter gets a residual row of its own) -- start s of a problem holds its
    parameter s % q at the starting value.  Every kept start converges within 100 iterations to MINPACK's minimum of ITS
    reduced problem within ten times MINPACK's own worst excess at default tolerances, and its held coordinate is the
    start's bit for bit.  The baseline is computed here and printed (on the CPU: 23 of 24 starts kept, MINPACK's worst
    excess 0.17 ftol c*)."""
    import torch
    from sysbio_modeling_amd import _lib
    dev, f64, i32 = 'cuda', torch.float64, torch.int32
    probs = lo.problems()
    held_col = lambda pb, s: s % pb.q          # noqa: E731
    cstar, keep, minpack_worst = reduced_minpack_baseline(probs, held_col)
    print('reduced problems: %d of 24 starts kept, MINPACK worst excess %.3g ftol c*' % (keep.sum(), minpack_worst))
    assert keep.sum() >= 20
    dprobs = [pb.to(dev) for pb in probs]
    V, M, q, max_iter = 24, max(pb.M for pb in probs), max(pb.q for pb in probs), 100
    assert all(pb.M + q - pb.q <= M for pb in probs)
    x0 = np.zeros((V, q))
    held = np.zeros((V, q), dtype=np.int32)
    for i, pb in enumerate(probs):
        x0[8 * i:8 * i + 8, :pb.q] = pb.starts
        for s in range(8):
            held[8 * i + s, held_col(pb, s)] = 1

    def evaluate(X):
        r, J = torch.zeros((V, M), dtype=f64, device=dev), torch.zeros((V, M, q), dtype=f64, device=dev)
        for i, pb in enumerate(dprobs):
            rows = slice(8 * i, 8 * i + 8)
            r[rows, :pb.M] = pb.residuals(X[rows, :pb.q])
            J[rows, :pb.M, :pb.q] = pb.jacobian(X[rows, :pb.q])
            for k in range(pb.q, q):
                r[rows, pb.M + k - pb.q] = X[rows, k]
                J[rows, pb.M + k - pb.q, k] = 1.0
        return r, J, (r * r).sum(dim=1)

    th = torch.from_numpy(x0).to(dev)
    held_d = torch.from_numpy(held).to(dev)
    r, J, norms = evaluate(th)
    cost = 0.5 * norms
    # lmder: D from the first Jacobian, Delta = 100 ||D theta|| -- over the free parameters
    col = torch.sqrt((J * J).sum(dim=1))
    d0 = torch.where(held_d != 0, torch.zeros_like(col), torch.where(col > 0, col, torch.ones_like(col)))
    xn = (d0 * th).norm(dim=1)
    radius = torch.where(xn > 0, 100.0 * xn, torch.full_like(xn, 100.0)).contiguous()
    dscale = torch.zeros((V, q), dtype=f64, device=dev)
    lam = torch.zeros((V,), dtype=f64, device=dev)
    done, accept = torch.zeros((V,), dtype=i32, device=dev), torch.zeros((V,), dtype=i32, device=dev)
    n_iter = torch.full((V,), max_iter, dtype=i32, device=dev)
    status_t = torch.zeros((V,), dtype=i32, device=dev)
    counters = torch.zeros((2,), dtype=i32, device=dev)
    delta, trial = (torch.empty((V, q), dtype=f64, device=dev) for _ in range(2))
    pred, dxnorm, gtx = (torch.empty((V,), dtype=f64, device=dev) for _ in range(3))
    st = torch.empty((V,), dtype=i32, device=dev)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    live = V
    for it in range(max_iter):
        _lib.check(ctx.lib.sbm_lm_trust_step_held(ctx.handle, p(J), p(r), p(dscale), p(radius), p(lam), V, M, q, None, p(done), 0.0,
                                                  p(th), p(trial), p(delta), p(pred), p(dxnorm), p(gtx), p(st), p(held_d)),
                   'sbm_lm_trust_step_held')
        r_t, J_t, norms_t = evaluate(trial)
        _lib.check(ctx.lib.sbm_lm_update(ctx.handle, p(cost), p(norms_t), p(status_t), p(pred), p(dxnorm), p(gtx), p(st), p(th),
                                         p(dscale), V, q, lo.FTOL, lo.XTOL, it, 1 if it == 0 else 0, p(radius), p(lam), p(done),
                                         p(accept), p(n_iter), p(counters), None), 'sbm_lm_update')
        _lib.check(ctx.lib.sbm_lm_accept(ctx.handle, p(accept), V, M, q, p(trial), p(r_t), p(J_t), p(norms_t), p(th), p(r), p(J),
                                         p(cost)), 'sbm_lm_accept')
        live = int(counters.cpu()[0])
        if live == 0:
            break
    final, theta, done_h = cost.cpu().numpy(), th.cpu().numpy(), done.cpu().numpy()
    assert np.array_equal(theta[held != 0], x0[held != 0])                 # the held coordinates: bit for bit, every start
    assert np.all(dscale.cpu().numpy()[held != 0] == 0.0)
    ours = -np.inf
    for i, pb in enumerate(probs):
        for s in range(8):
            if keep[i, s]:
                v = 8 * i + s
                assert done_h[v] == 1, ('not converged in %d iterations' % max_iter, pb.name, s)
                excess = (final[v] - cstar[i, s]) / (lo.FTOL * cstar[i, s])
                ours = max(ours, excess)
                assert excess <= 10.0 * minpack_worst, (pb.name, s, excess, minpack_worst)
    print('held device loop: %d iterations, %d starts still running; excess over c* in units of ftol c*: MINPACK %.3g, '
          'device loop %.3g' % (it + 1, live, minpack_worst, ours))
