"""sbm_lm_trust_step_bounded -- the active-set trust-region step inside a box -- against sbm_lm_trust_step_held on the mask
the bounds imply (the kernel compacts by that mask, so the two do the same arithmetic: bitwise equality is expected and
printed, 1e-13 asserted), its projection against numpy, and the loop built from it (step, residuals and Jacobian in torch,
sbm_lm_update, sbm_lm_accept) against scipy.optimize.least_squares(method='trf', bounds=...)."""
import numpy as np
import pytest

from oracle import lmder_oracle as lo
from tests.support import bounded_lm_oracle as bo
from tests.test_gpu_lm_held import REL, rel_err, trust_step

pytestmark = pytest.mark.gpu

INF = np.inf
EPS = np.finfo(np.float64).eps
SHAPES = [(8, 30, 12),      # one triangle entry per thread, one row tile
          (4, 75, 70),      # the ballot spans two waves, several row tiles and a remainder row count
          (3, 40, 128)]     # LM_MAX_Q
OUTPUTS = ('delta', 'trial', 'dscale', 'pred', 'dxnorm', 'gtx', 'lam')


def bounded_step(J, r, dscale, radius, lam, theta, lower, upper, held=None, row_scale=None, skip=None, max_step=0.0):
    """One sbm_lm_trust_step_bounded launch on numpy inputs (``held=None``: a NULL pointer).  Returns the outputs as numpy
    arrays (dscale and lam are the in / out arrays after the call), 'active' being active_out."""
    import torch
    from sysbio_modeling_amd import _lib
    dev, f64, i32 = 'cuda', torch.float64, torch.int32
    V, M, q = J.shape
    t = lambda x, dt=f64: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)     # noqa: E731
    Jd, rd, Dd, Rd, Ld, thd, rsd, skd = t(J), t(r), t(dscale), t(radius), t(lam), t(theta), t(row_scale), t(skip, i32)
    lod, upd = t(np.array(np.broadcast_to(lower, (V, q)))), t(np.array(np.broadcast_to(upper, (V, q))))
    hd = t(np.asarray(held, dtype=np.int32), i32) if held is not None else None
    delta, trial = (torch.full((V, q), -77.0, dtype=f64, device=dev) for _ in range(2))
    pred, dxn, gtx = (torch.full((V,), -77.0, dtype=f64, device=dev) for _ in range(3))
    st = torch.full((V,), -7, dtype=i32, device=dev)
    active = torch.full((V, q), -7, dtype=i32, device=dev)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    _lib.check(ctx.lib.sbm_lm_trust_step_bounded(ctx.handle, p(Jd), p(rd), p(Dd), p(Rd), p(Ld), V, M, q, p(rsd), p(skd),
                                                 float(max_step), p(thd), p(trial), p(delta), p(pred), p(dxn), p(gtx), p(st), p(hd),
                                                 p(lod), p(upd), p(active)), 'sbm_lm_trust_step_bounded')
    torch.cuda.synchronize()
    return dict(delta=delta.cpu().numpy(), trial=trial.cpu().numpy(), pred=pred.cpu().numpy(), dxnorm=dxn.cpu().numpy(),
                gtx=gtx.cpu().numpy(), status=st.cpu().numpy(), dscale=Dd.cpu().numpy(), lam=Ld.cpu().numpy(),
                active=active.cpu().numpy())


def expected_codes(J, r, theta, lower, upper, held, row_scale):
    """The active-set codes of every start in numpy.  No sign may be decided by rounding: at every column that sits on a
    bound, |g_c| > 1e-9 sum_m |rs J r| is asserted -- no entry of the mask is set aside."""
    V, M, q = J.shape
    codes = np.zeros((V, q), dtype=np.int32)
    for v in range(V):
        codes[v], g, gabs = bo.active_set(J[v], r[v], theta[v], lower[v], upper[v], None if held is None else held[v], row_scale)
        on = (theta[v] <= lower[v]) | (theta[v] >= upper[v])
        assert np.all(np.abs(g[on]) > 1e-9 * gabs[on]), ('a sign that rounding decides', v, np.nonzero(on)[0])
    return codes


def compare_with_held(got, want, codes, lam_in, what):
    """Every output of the bounded launch ``got`` against the held launch ``want`` on the mask codes != 0; status 3 where
    the bounds (not the caller alone) leave nothing free.  Returns whether everything was bitwise equal."""
    V = codes.shape[0]
    nothing_free = np.all(codes != 0, axis=1)
    by_bounds = nothing_free & np.any(codes >= 2, axis=1)
    want_status = np.where(by_bounds, 3, want['status'])
    assert np.array_equal(want['status'][nothing_free], np.full(nothing_free.sum(), 2))
    assert np.array_equal(got['status'], want_status), (what, got['status'], want_status)
    assert np.array_equal(got['active'], codes), what
    assert np.array_equal(got['lam'][nothing_free], lam_in[nothing_free]), what          # lambda untouched
    errs = {k: rel_err(got[k], want[k]) for k in OUTPUTS}
    bitwise = all(np.array_equal(got[k], want[k]) for k in OUTPUTS)
    print('%s: %d starts against the held step on the effective mask: bitwise equal: %s, worst relative error %.3g'
          % (what, V, bitwise, max(errs.values())))
    assert max(errs.values()) <= REL, (what, errs)
    return bitwise


def effective_mask_case(V, M, q, seed):
    """The inputs of the effective-mask test for one shape.  Start 0 has, in columns 0 .. 5: theta on a lower bound with
    g > 0 (held at it) and with g < 0 (free); on an upper bound with g < 0 (held) and g > 0 (free); a column the caller
    holds that also sits on a bound with the gradient pushing outward; and a column on a lower bound whose sum rs J r is
    positive while its sum J r is negative.  Its radius is small, so that the step is close to a scaled gradient step and
    the free columns on bounds move inward.  Start 1: every column on a bound with the gradient pushing outward.  Start 2:
    infinite bounds, nothing held.  Further starts: random columns held by bounds or by the caller, radii from far inside
    to far outside the Gauss-Newton step."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((V, M, q))
    r = rng.standard_normal((V, M))
    rs = rng.uniform(0.5, 1.5, M)
    rs[0] = 8.0
    theta = rng.standard_normal((V, q))
    lower, upper = theta - 1.0e6, theta + 1.0e6
    held = np.zeros((V, q), dtype=np.int32)
    radius = np.array([1e-3, 1.0, 5.0, 1e3, 1e-2, 1e6, 0.3, 2e-1])[:V].copy()
    lam = np.zeros(V)
    lam[1] = 7.0
    g = lambda v: np.einsum('m,mc,m->c', rs, J[v], r[v])          # noqa: E731

    def orient(v, c, sign):          # make g_c of start v have that sign
        if np.sign(g(v)[c]) != sign:
            J[v, :, c] *= -1.0

    # start 0
    for c, sign in ((0, 1), (1, -1), (2, -1), (3, 1), (4, 1)):
        orient(0, c, sign)
    lower[0, [0, 1, 4]] = theta[0, [0, 1, 4]]
    upper[0, [2, 3]] = theta[0, [2, 3]]
    held[0, 4] = 1
    # column 5: a_0 + rest < 0 < rs_0 a_0 + rest_rs with a_m = J_m5 r_m -- row 0 carries the weight 8
    a = J[0, :, 5] * r[0]
    if a[1:].sum() > 0:
        J[0, :, 5] *= -1.0
        a = -a
    rest, rest_rs = a[1:].sum(), (rs[1:] * a[1:]).sum()
    assert rest < 0 and -rest_rs / rs[0] < -rest
    a0 = 0.5 * (-rest_rs / rs[0] - rest)
    J[0, 0, 5] = a0 / r[0, 0]
    assert (J[0, :, 5] * r[0]).sum() < 0 < (rs * J[0, :, 5] * r[0]).sum()
    lower[0, 5] = theta[0, 5]
    # start 1: everything bound-active
    g1 = g(1)
    lower[1] = np.where(g1 > 0, theta[1], -INF)
    upper[1] = np.where(g1 < 0, theta[1], INF)
    # start 2: no bounds at all
    lower[2], upper[2] = -INF, INF
    for v in range(3, V):
        gv = g(v)
        pick = rng.random(q) < 0.3
        lower[v] = np.where(pick & (gv > 0), theta[v], lower[v])
        upper[v] = np.where(pick & (gv < 0), theta[v], upper[v])
        held[v] = (rng.random(q) < 0.2).astype(np.int32)
    return dict(J=J, r=r, rs=rs, theta=theta, lower=lower, upper=upper, held=held, radius=radius, lam=lam)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'V%d_M%d_q%d' % s)
def test_bounded_step_equals_the_held_step_on_the_effective_mask(shape):
    """Every start in one launch (the cases: effective_mask_case), with a row_scale; then the same bounds with
    held = NULL, where the start with infinite bounds is also compared with sbm_lm_trust_step_ex.  The expected mask comes
    from numpy (no sign decided by rounding, no entry set aside); all outputs against sbm_lm_trust_step_held on that mask
    at 1e-13, active_out exactly.  The other bounds are wide enough that nothing is projected, asserted on the held step."""
    V, M, q = shape
    c = effective_mask_case(V, M, q, 21 + q)
    J, r, rs, theta, lower, upper, radius, lam = (c[k] for k in ('J', 'r', 'rs', 'theta', 'lower', 'upper', 'radius', 'lam'))
    dscale = np.zeros((V, q))
    for held, what in ((c['held'], 'held mask'), (None, 'held = NULL')):
        codes = expected_codes(J, r, theta, lower, upper, held, rs)
        if held is not None:
            assert codes[0, :6].tolist() == [2, 0, 3, 0, 1, 2] and np.all(codes[1] >= 2) and np.all(codes[2] == 0)
            assert set(np.unique(codes)) == {0, 1, 2, 3}
        else:
            assert codes[0, :6].tolist() == [2, 0, 3, 0, 2, 2] and not np.any(codes == 1)
        want = trust_step(J, r, dscale, radius, lam, theta, rs, None, 0.0, held=(codes != 0).astype(np.int32))
        # nothing is projected: the held step stays strictly inside the box in every free column
        free = codes == 0
        assert np.all((want['trial'] >= lower)[free]) and np.all((want['trial'] <= upper)[free])
        assert np.all(want['status'][[0] + list(range(2, V))] == 0)
        got = bounded_step(J, r, dscale, radius, lam, theta, lower, upper, held, rs)
        compare_with_held(got, want, codes, lam, '%s, %s' % (shape, what))
        assert got['status'][1] == 3 and got['pred'][1] == 0.0 and got['dxnorm'][1] == 0.0 and got['gtx'][1] == 0.0
        assert np.all(got['delta'][1] == 0.0) and np.array_equal(got['trial'][1], theta[1]) and np.all(got['dscale'][1] == 0.0)
        if held is None:
            ex = trust_step(J, r, dscale, radius, lam, theta, rs, None, 0.0, held='ex')
            errs = [rel_err(got[k][2], ex[k][2]) for k in OUTPUTS]
            print('%s: infinite bounds, held = NULL against sbm_lm_trust_step_ex: bitwise equal: %s, worst relative error %.3g'
                  % (shape, all(np.array_equal(got[k][2], ex[k][2]) for k in OUTPUTS), max(errs)))
            assert max(errs) <= REL and got['status'][2] == ex['status'][2] == 0


def sums_of_the_step_taken(J, r, rs, D, x):
    """pred, dxnorm, gtx of the step x in numpy, each with the summation bound of the test: 4 (M + q) eps times the sum of
    the absolute values of the terms of its sum (the factor 4 for the order of the sums and the fmas)."""
    M, q = J.shape
    Js = J * rs[:, None]
    k = 4.0 * (M + q) * EPS
    gterms = Js * r[:, None] * x[None, :]
    gtx = gterms.sum()
    Jx = Js @ x
    quad_abs = ((np.abs(Js) * np.abs(x)[None, :]).sum(axis=1) ** 2).sum()
    pred = -gtx - 0.5 * float(Jx @ Jx)
    dxn = float(np.linalg.norm(D * x))
    return (pred, k * (np.abs(gterms).sum() + 0.5 * quad_abs)), (dxn, k * dxn), (gtx, k * np.abs(gterms).sum())


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'V%d_M%d_q%d' % s)
def test_projection_ends_on_the_bound_and_reports_the_step_taken(shape):
    """Bounds a fraction of the unprojected step away in a third of the columns of every start (theta strictly inside: the
    active set is the caller's mask, so the unprojected step is sbm_lm_trust_step_held's, bit for bit).  trial ==
    clip(theta + x_held, lower, upper) bitwise; delta == trial - theta bitwise where a component was projected, x_held
    bitwise where not; pred, dxnorm, gtx against numpy from delta within the summation bound.  The last start is one whose
    projected step is no descent step: status 4, zeros, trial = theta -- checked on the CPU, with the oracle, to be such a
    case."""
    V, M, q = shape
    rng = np.random.default_rng(31 + q)
    J = rng.standard_normal((V, M, q))
    r = rng.standard_normal((V, M))
    rs = rng.uniform(0.5, 2.0, M)
    theta = rng.standard_normal((V, q))
    radius = np.array([1e3, 1e-1, 5.0, 1e6, 1.0, 1e2, 0.3, 1e3])[:V].copy()
    radius[V - 1] = 1e3 if q <= M else 3.0      # (q > M: a damped step, as the oracle's lmpar would take too)
    held = (rng.random((V, q)) < 0.15).astype(np.int32)
    held[V - 1] = 0
    dscale, lam = np.zeros((V, q)), np.zeros(V)
    ref = trust_step(J, r, dscale, radius, lam, theta, rs, None, 0.0, held=held)
    assert np.all(ref['status'] == 0)
    x = ref['delta']
    lower, upper = np.full((V, q), -INF), np.full((V, q), INF)
    frac = rng.uniform(0.1, 0.9, (V, q))
    pick = (rng.random((V, q)) < 1.0 / 3.0) & (held == 0) & (x != 0.0)
    pick[:, 0] |= (held[:, 0] == 0)
    upper[pick & (x > 0)] = (theta + frac * x)[pick & (x > 0)]
    lower[pick & (x < 0)] = (theta + frac * x)[pick & (x < 0)]
    # the last start: every component of the unprojected step that descends (g_c x_c < 0) is stopped after a thousandth of
    # its way; what is left goes uphill.  Checked on the CPU: the oracle's sums of the projected step say "no descent" with
    # room to spare, and where J has full column rank (the oracle's lmpar and the kernel's then both return the
    # Gauss-Newton step) the oracle's own bounded step ends with status 4
    v4 = V - 1
    gv = np.einsum('m,mc,m->c', rs, J[v4], r[v4])
    down = gv * x[v4] < 0
    assert down.any() and not down.all()
    lower[v4], upper[v4] = -INF, INF
    upper[v4, down & (x[v4] > 0)] = (theta[v4] + 1e-3 * x[v4])[down & (x[v4] > 0)]
    lower[v4, down & (x[v4] < 0)] = (theta[v4] + 1e-3 * x[v4])[down & (x[v4] < 0)]
    xp = np.clip(theta[v4] + x[v4], lower[v4], upper[v4]) - theta[v4]
    assert np.any(xp != x[v4])
    pred4, _, gtx4 = bo.taken_step_quantities(J[v4] * rs[:, None], r[v4], ref['dscale'][v4], xp)
    (_, pred4_tol), _, (_, gtx4_tol) = sums_of_the_step_taken(J[v4], r[v4], rs, ref['dscale'][v4], xp)
    assert gtx4 > gtx4_tol or pred4 < -pred4_tol, (gtx4, gtx4_tol, pred4, pred4_tol)
    if q <= M:
        oracle = bo.bounded_step(J[v4], r[v4], dscale[v4], radius[v4], 0.0, theta[v4], lower[v4], upper[v4], row_scale=rs)
        assert oracle['status'] == 4 and np.all(oracle['active'] == 0), oracle['status']

    assert np.all((theta > lower) & (theta < upper))                       # strictly inside: nothing is bound-active
    got = bounded_step(J, r, dscale, radius, lam, theta, lower, upper, held, rs)
    assert np.array_equal(got['active'], held)
    want_trial = np.clip(theta + x, lower, upper)
    projected = want_trial != theta + x
    assert projected[:v4].any(axis=1).all() and np.all(want_trial[projected] == np.where(x > 0, upper, lower)[projected])
    assert got['status'].tolist() == [0] * v4 + [4]
    # status 4: zeros, trial = theta, the scaling written as for any solved system, lambda kept
    assert np.all(got['delta'][v4] == 0.0) and np.array_equal(got['trial'][v4], theta[v4])
    assert got['pred'][v4] == 0.0 and got['dxnorm'][v4] == 0.0 and got['gtx'][v4] == 0.0 and got['lam'][v4] == lam[v4]
    assert np.array_equal(got['dscale'][v4], ref['dscale'][v4])
    worst = 0.0
    for v in range(v4):
        assert np.array_equal(got['trial'][v], want_trial[v]), v
        pv = projected[v]
        assert np.array_equal(got['delta'][v, pv], (want_trial[v] - theta[v])[pv]) and np.array_equal(got['delta'][v, ~pv], x[v, ~pv]), v
        assert np.array_equal(got['dscale'][v], ref['dscale'][v]) and got['lam'][v] == ref['lam'][v], v
        sums = sums_of_the_step_taken(J[v], r[v], rs, got['dscale'][v], got['delta'][v])
        for name, (want, tol) in zip(('pred', 'dxnorm', 'gtx'), sums):
            err = abs(got[name][v] - want)
            worst = max(worst, err / tol)
            assert err <= tol, (name, v, got[name][v], want, tol)
    print('%s: projection: trial on the bounds bitwise; pred, dxnorm, gtx within %.3g of their summation bounds' % (shape, worst))


def test_bounded_loop_reaches_scipys_constrained_minimum():
    """The fitting loop inside a box, without an ODE: sbm_lm_trust_step_bounded (held = NULL), residuals and Jacobian of
    the trial points in torch, sbm_lm_update, sbm_lm_accept, on the three problems of oracle/lmder_oracle.py padded to one
    batch (V = 24, M = 30, q = 12; a padding parameter gets a residual row of its own and the bounds [-1, 1]) with the
    bounds of tests/test_bounds_cpu.py.  Every start ends done within 100 iterations, at most 10 w above scipy's c* (w:
    scipy's own worst excess at default tolerances, computed here and printed); theta stays in the box at every iteration;
    the parameters on bounds are scipy's."""
    import torch
    from sysbio_modeling_amd import _lib
    dev, f64, i32 = 'cuda', torch.float64, torch.int32
    probs = lo.problems()
    ref, w = bo.scipy_bounded_baseline(probs)
    print('scipy least_squares(trf, bounds): worst excess at default tolerances w = %.3g ftol c*' % w)
    dprobs = [pb.to(dev) for pb in probs]
    V, M, q, max_iter = 24, max(pb.M for pb in probs), max(pb.q for pb in probs), 100
    assert all(pb.M + q - pb.q <= M for pb in probs)
    x0 = np.zeros((V, q))
    lower, upper = np.full((V, q), -1.0), np.full((V, q), 1.0)
    for i, (pb, rf) in enumerate(zip(probs, ref)):
        x0[8 * i:8 * i + 8, :pb.q] = rf['starts']
        lower[8 * i:8 * i + 8, :pb.q], upper[8 * i:8 * i + 8, :pb.q] = rf['lower'], rf['upper']

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
    lo_d, up_d = torch.from_numpy(lower).to(dev), torch.from_numpy(upper).to(dev)
    r, J, norms = evaluate(th)
    cost = 0.5 * norms
    col = torch.sqrt((J * J).sum(dim=1))
    xn = (torch.where(col > 0, col, torch.ones_like(col)) * th).norm(dim=1)
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
    inside = torch.ones((), dtype=torch.bool, device=dev)
    fours = torch.zeros((), dtype=torch.int64, device=dev)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    live = V
    for it in range(max_iter):
        _lib.check(ctx.lib.sbm_lm_trust_step_bounded(ctx.handle, p(J), p(r), p(dscale), p(radius), p(lam), V, M, q, None, p(done),
                                                     0.0, p(th), p(trial), p(delta), p(pred), p(dxnorm), p(gtx), p(st), None,
                                                     p(lo_d), p(up_d), None), 'sbm_lm_trust_step_bounded')
        inside &= ((trial >= lo_d) & (trial <= up_d)).all()
        fours += ((st == 4) & (done == 0)).sum()
        r_t, J_t, norms_t = evaluate(trial)
        _lib.check(ctx.lib.sbm_lm_update(ctx.handle, p(cost), p(norms_t), p(status_t), p(pred), p(dxnorm), p(gtx), p(st), p(th),
                                         p(dscale), V, q, lo.FTOL, lo.XTOL, it, 1 if it == 0 else 0, p(radius), p(lam), p(done),
                                         p(accept), p(n_iter), p(counters), None), 'sbm_lm_update')
        _lib.check(ctx.lib.sbm_lm_accept(ctx.handle, p(accept), V, M, q, p(trial), p(r_t), p(J_t), p(norms_t), p(th), p(r), p(J),
                                         p(cost)), 'sbm_lm_accept')
        inside &= ((th >= lo_d) & (th <= up_d)).all()
        live = int(counters.cpu()[0])
        if live == 0:
            break
    final, theta, done_h = cost.cpu().numpy(), th.cpu().numpy(), done.cpu().numpy()
    assert bool(inside), 'a trial point or an iterate left the box'
    assert np.all(done_h == 1), ('not converged in %d iterations' % max_iter, np.nonzero(done_h != 1)[0])
    ours = -np.inf
    for i, (pb, rf) in enumerate(zip(probs, ref)):
        for s in range(8):
            v = 8 * i + s
            excess = (final[v] - rf['cstar']) / (lo.FTOL * rf['cstar'])
            ours = max(ours, excess)
            assert excess <= 10.0 * w, (pb.name, s, excess, w)
            at = (theta[v, :pb.q] == rf['upper']).astype(int) - (theta[v, :pb.q] == rf['lower']).astype(int)
            assert np.array_equal(at, rf['at_bound']), (pb.name, s, at, rf['at_bound'])
            assert np.all(np.abs(theta[v, pb.q:]) < 1.0)                      # the padding parameters end at 0, inside [-1, 1]
    print('bounded device loop: %d iterations, %d starts still running, %d steps of status 4; excess over c* in units of ftol c*: '
          'scipy %.3g, device loop %.3g' % (it + 1, live, int(fours), w, ours))
