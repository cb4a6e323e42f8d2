"""sbm_lm_geodesic -- the geodesic acceleration of the trust-region step -- against tests/support/geodesic_oracle.py.
Inputs come from sbm_lm_trust_step_ex / _held on random J and r, with radii from far inside to far outside the Gauss-Newton
step; the probe is synthesised as r_probe = r_base + h J~ v + h^2 c / 2 with c chosen per start, so that the second
derivative the kernel extracts is c up to rounding and the gate can be aimed at."""
import numpy as np
import pytest

from oracle import lmder_oracle as lo
from tests.support import geodesic_oracle as go
from tests.test_gpu_lm_held import REL, rel_err, trust_step

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = go.LD
GUARD_F, GUARD_I = 7.25, -91
INOUT = ('delta', 'trial', 'pred', 'dxnorm', 'gtx')


def guarded(arr, dtype):
    """A device copy of ``arr`` as a view two elements into a flat tensor, two sentinel elements on each side"""
    import torch
    arr = np.ascontiguousarray(arr)
    flat = torch.full((arr.size + 4,), GUARD_F if dtype.is_floating_point else GUARD_I, dtype=dtype, device='cuda')
    view = flat[2:2 + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(arr).to('cuda').to(dtype))
    return flat, view


def guards_intact(flat):
    g = GUARD_F if flat.dtype.is_floating_point else GUARD_I
    return bool((flat[:2] == g).all()) and bool((flat[-2:] == g).all())


def geodesic(J, r, r_base, r_probe, step, theta, *, h=go.H, alpha=go.ALPHA, max_step=0.0, row_scale=None, skip=None, held=None,
             status_base=None, status_probe=None, step_status=None, n_accel0=None):
    """One sbm_lm_geodesic launch on numpy inputs: ``step`` is the dict tests.test_gpu_lm_held.trust_step returned for the same
    J, r, row_scale, max_step, theta (its delta, trial, pred, dxnorm, gtx, dscale, lam, status go in).  Every output sits
    between sentinel elements.  Returns the arrays after the call; asserts the guards, lambda and dscale."""
    import torch
    from sysbio_modeling_amd import _lib
    f64, i32 = torch.float64, torch.int32
    V, M, q = J.shape
    t = lambda x, dt=f64: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to('cuda').to(dt)     # noqa: E731
    ins = dict(J=t(J), r=t(r), r_base=t(r_base), r_probe=t(r_probe), sb=t(status_base, i32), sp=t(status_probe, i32),
               D=t(step['dscale']), lam=t(step['lam']), rs=t(row_scale), skip=t(skip, i32),
               st=t(step['status'] if step_status is None else step_status, i32), held=t(held, i32), theta=t(theta))
    kept = {k: ins[k].clone() for k in ('D', 'lam')}
    out = {k: guarded(step[k], f64) for k in INOUT}
    out['accel_status'] = guarded(np.full(V, -7), i32)
    out['ratio'] = guarded(np.full(V, -77.0), f64)
    out['n_accel'] = guarded(np.arange(V) + 5 if n_accel0 is None else n_accel0, i32)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    _lib.check(ctx.lib.sbm_lm_geodesic(ctx.handle, p(ins['J']), p(ins['r']), p(ins['r_base']), p(ins['r_probe']), p(ins['sb']),
                                       p(ins['sp']), p(ins['D']), p(ins['lam']), V, M, q, p(ins['rs']), p(ins['skip']), p(ins['st']),
                                       p(ins['held']), float(h), float(alpha), float(max_step), p(ins['theta']),
                                       *(p(out[k][1]) for k in INOUT), p(out['accel_status'][1]), p(out['ratio'][1]),
                                       p(out['n_accel'][1])), 'sbm_lm_geodesic')
    torch.cuda.synchronize()
    for k, (flat, _) in out.items():
        assert guards_intact(flat), 'guard elements of %s' % k
    for k in kept:
        assert torch.equal(kept[k], ins[k]), '%s was written' % k
    return {k: view.cpu().numpy() for k, (_, view) in out.items()}


def scaled(J, row_scale):
    return J if row_scale is None else row_scale[None, :, None] * J


def accel_of(Jv, D, lam, c, free):
    """-(J^T J + lam D^2)^-1 J^T c on the free columns, float64: good enough to aim c at a rho"""
    Jf = Jv[:, free]
    return np.linalg.lstsq(np.vstack([Jf, np.sqrt(lam) * np.diag(D[free])]), np.concatenate([-c, np.zeros(free.sum())]), rcond=None)[0]


def aim(Js, step, v, c0, rho, free=None):
    """c0 scaled so that the acceleration of start v has 2 ||D a|| / ||D v|| = rho"""
    q = Js.shape[2]
    free = np.ones(q, dtype=bool) if free is None else free
    D, vel = step['dscale'][v], step['delta'][v]
    a = accel_of(Js[v], D, step['lam'][v], c0, free)
    rho0 = 2.0 * np.linalg.norm(D[free] * a) / np.linalg.norm(D[free] * vel[free])
    return c0 * (rho / rho0)


def probe_of(Js, r_base, step, c, h):
    """r_probe = r_base + h J~ v + h^2 c / 2, in float64 as a state-only integration would return it"""
    return r_base + h * np.einsum('vmq,vq->vm', Js, step['delta']) + 0.5 * h * h * c


def c_q(M, q):
    """The constant of the backward error of a Cholesky solve of normal equations that were formed in floating point, in
    units of the unit roundoff (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.: (3.5) gamma_M for the dot
    products of length M behind every entry of J^T J and of the right-hand side; Theorem 10.4 gamma_{3 q + 1} |R^T| |R| for
    the factorisation and the two triangular solves, with || |R^T| |R| || <= q ||A|| (10.7)); the q + 6 are the row's
    J v (a dot product of length q), the four operations of r_vv, the product with row_scale and the damping."""
    return M + q + 6 + q * (3 * q + 1)


def backward_error_ratio(Js_v, r_base, r_probe, D, lam, vel, a, h, free):
    """|| D^-1 (A a + J~^T r_vv) || in longdouble over the bound eps c_q (|| D^-1 |A| D^-1 || ||D a|| + || D^-1 |J~|^T t ||),
    t = (2 / h^2) (|r_probe| + |r_base|) + (2 / h) |J~| |v|; the bound itself; D^-1 A D^-1"""
    Jf = np.asarray(Js_v[:, free], dtype=LD)
    Df, vf, af = np.asarray(D[free], dtype=LD), np.asarray(vel[free], dtype=LD), np.asarray(a[free], dtype=LD)
    rvv = go.rvv_reference(Jf, r_base, r_probe, vf, h)
    A = Jf.T @ Jf + LD(lam) * np.diag(Df * Df)
    res = (A @ af + Jf.T @ rvv) / Df
    t = (2.0 / h ** 2) * (np.abs(r_probe) + np.abs(r_base)) + (2.0 / h) * (np.abs(Jf).astype(np.float64) @ np.abs(vel[free]))
    scale = np.linalg.norm((np.abs(A) / np.outer(Df, Df)).astype(np.float64), 2) * float(np.sqrt(np.sum((Df * af) ** 2))) + \
        np.linalg.norm((np.abs(Jf).astype(np.float64).T @ t) / D[free])
    bound = EPS * c_q(Js_v.shape[0], int(free.sum())) * scale
    return float(np.sqrt(np.sum(res * res))) / bound, bound, (A / np.outer(Df, Df)).astype(np.float64)


def rho_tolerance(Js_v, r_base, r_probe, D, lam, vel, a, h, free):
    """What the backward-error bound allows rho = 2 ||D a|| / ||D v|| to differ from the oracle's by: a perturbation of the
    scaled system within the bound moves D a by at most || (D^-1 A D^-1)^-1 || times it."""
    _, bound, As = backward_error_ratio(Js_v, r_base, r_probe, D, lam, vel, a, h, free)
    smallest = float(np.linalg.svd(As, compute_uv=False)[-1])
    return 2.0 * bound / (smallest * float(np.linalg.norm(D[free] * vel[free]))) if smallest > 0.0 else np.inf


def check_launch(J, r, r_base, r_probe, step, theta, out, *, h=go.H, alpha=go.ALPHA, max_step=0.0, row_scale=None, held=None,
                 want=None, what=''):
    """Everything one launch owes the oracle, start by start: the status (``want[v]`` if given and not None, else the oracle's); where
    the acceleration was applied, its backward error and the quantities of the step taken, recomputed from the device's
    own delta; where it was not, the five in / out arrays bit for bit as the trust step wrote them; n_accel.  Returns the
    worst backward-error ratio."""
    V, M, q = J.shape
    Js = scaled(J, row_scale)
    worst = 0.0
    for v in range(V):
        where = '%sstart %d' % (what, v)
        free = np.ones(q, dtype=bool) if held is None else ~np.asarray(held[v], dtype=bool)
        ref = go.accel_reference(J[v], r[v], r_base[v], r_probe[v], step['dscale'][v], step['lam'][v], step['delta'][v], h, alpha,
                                 max_step, held=None if held is None else ~free, row_scale=row_scale)
        status = out['accel_status'][v]
        assert status == (ref.status if want is None or want[v] is None else want[v]), (where, status, ref.status, ref.rho)
        assert out['n_accel'][v] == v + 5 + (1 if status == 0 else 0), where
        if status in (4, 5):
            # (an applied step's rho is checked below against the device's own delta, to 1e-13)
            tol = rho_tolerance(Js[v], r_base[v], r_probe[v], step['dscale'][v], step['lam'][v], step['delta'][v], ref.a, h, free)
            assert abs(out['ratio'][v] - ref.rho) <= tol, (where, out['ratio'][v], ref.rho, tol)
        elif status != 0:
            assert np.isnan(out['ratio'][v]), where
        if status != 0:
            for k in INOUT:
                assert np.array_equal(out[k][v], step[k][v]), (where, k)
            continue
        D, vel, x = step['dscale'][v], step['delta'][v], out['delta'][v]
        assert np.array_equal(x[~free], vel[~free]) and np.array_equal(out['trial'][v][~free], step['trial'][v][~free]), where
        assert np.array_equal(out['trial'][v][free], (theta[v] + x)[free]), where                       # bit for bit
        clipped = max_step > 0.0 and bool(np.any(np.abs(x) >= max_step))
        if max_step > 0.0:
            assert np.all(np.abs(x) <= max_step), where
        xl, Dl, Jl = np.asarray(x, dtype=LD)[free], np.asarray(D, dtype=LD)[free], np.asarray(Js[v], dtype=LD)[:, free]
        g = Jl.T @ np.asarray(r[v], dtype=LD)
        gtx, Jx = g @ xl, Jl @ xl
        assert rel_err(out['dxnorm'][v], float(np.sqrt(np.sum((Dl * xl) ** 2)))) <= REL, where
        assert rel_err(out['gtx'][v], float(gtx)) <= REL, (where, out['gtx'][v], float(gtx))
        assert abs(out['pred'][v] - float(-gtx - (Jx @ Jx) / 2)) <= REL * float(abs(gtx) + (Jx @ Jx) / 2), where
        assert out['gtx'][v] < 0.0 and out['pred'][v] > 0.0, where
        if not clipped:
            a = np.zeros(q, dtype=LD)
            a[free] = 2 * (xl - np.asarray(vel, dtype=LD)[free])
            rho = 2.0 * float(np.sqrt(np.sum((Dl * a[free]) ** 2)) / np.sqrt(np.sum((Dl * np.asarray(vel, dtype=LD)[free]) ** 2)))
            assert rel_err(out['ratio'][v], rho) <= REL, (where, out['ratio'][v], rho)
            ratio = backward_error_ratio(Js[v], r_base[v], r_probe[v], D, step['lam'][v], vel, a, h, free)[0]
            worst = max(worst, ratio)
            assert ratio <= 1.0, (where, ratio)
    return worst


def random_case(seed, V, M, q, radii=None, row_scale=False):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((V, M, q))
    r = rng.standard_normal((V, M))
    theta = rng.standard_normal((V, q))
    radius = np.resize(np.array([1e3, 1e-2, 5.0, 1e6, 1.0, 1e8, 0.3, 2e-1]) if radii is None else radii, V).astype(np.float64)
    rs = rng.uniform(0.5, 2.0, M) if row_scale else None
    return rng, J, r, theta, radius, rs


SHAPES = [(8, 30, 12)] + [(4, M, 5) for M in (1, 7, 8, 9, 31, 32, 33, 65)] + [(4, q + 3, q) for q in (1, 2, 63, 64, 65)] + \
    [(2, 140, 128),            # the largest q, the 16-row tile: nine tiles with a remainder
     (4, 6, 9)]                # M < q: J^T J is singular and every step is damped


@pytest.mark.parametrize('V,M,q', SHAPES, ids=['%dx%dx%d' % s for s in SHAPES])
def test_acceleration_against_the_oracle_at_every_shape(V, M, q):
    """Even starts are aimed at rho = alpha / 2 (applied), odd ones at 2 alpha (the gate), half of the launches with a
    row_scale.  M in {1, 7, 8, 9, 31, 32, 33, 65} at q = 5: the edges of the 32-row tile, the eight lanes of a row and a single
    row; q in {1, 2, 63, 64, 65} at M = q + 3: the wave edge and the ownership of the triangle; (2, 140, 128): the largest
    q and the shrunk tile; (4, 6, 9): M < q, lambda > 0 everywhere.  The acceleration is checked as a backward error: with
    the device's a = 2 (delta - v), || D^-1 (A a + J~^T r_vv) || in longdouble stays below
    eps c_q (|| D^-1 |A| D^-1 || ||D a|| + || D^-1 |J~|^T t ||), c_q = M + q + 6 + q (3 q + 1) (see c_q; recovering a from
    delta costs eps ||D^-1 A |delta| || more, which at rho = alpha / 2 is below 6.3 eps lambda ||D a|| + eps || D^-1 |J~|^T t ||
    and inside the factor two between eps and the unit roundoff the constants are stated in).

    Worst measured ratio to that bound over the sixteen shapes: 8.3e-4 (at 4 x 4 x 1; 2.0e-5 at 8 x 30 x 12, 1.5e-7 at
    2 x 140 x 128 -- the bound's second term carries the 2 / h^2 = 200 of the difference quotient, which the synthetic probe's
    rounding does not exhaust)."""
    rng, J, r, theta, radius, rs = random_case(100 + M * 131 + q, V, M, q, row_scale=(M + q) % 2 == 0)
    if M < q:
        radius = np.resize([1.0, 1e-2, 0.3, 5.0], V).astype(np.float64)
    step = trust_step(J, r, np.zeros((V, q)), radius, np.zeros(V), theta, rs, None, 0.0)
    solved = step['status'] == 0
    assert solved.sum() >= V - 1
    if M < q:
        assert np.all(step['lam'][solved] > 0.0)
    elif V >= 4:
        assert np.any(step['lam'] == 0.0) and np.any(step['lam'] > 0.0)
    Js = scaled(J, rs)
    c = np.stack([aim(Js, step, v, rng.standard_normal(M), go.ALPHA / 2 if v % 2 == 0 else 2 * go.ALPHA) if solved[v]
                  else np.zeros(M) for v in range(V)])
    r_base = r + 1e-9 * rng.standard_normal((V, M))          # the two kernels differ by the integration tolerance
    r_probe = probe_of(Js, r_base, step, c, go.H)
    out = geodesic(J, r, r_base, r_probe, step, theta, row_scale=rs)
    # an odd start stops at the gate; whether an even one descends in the model (status 0 or 5) the oracle decides, and at
    # least one start of every launch is accelerated
    want = [1 if not solved[v] else 4 if v % 2 else None for v in range(V)]
    worst = check_launch(J, r, r_base, r_probe, step, theta, out, row_scale=rs, want=want)
    print('%d x %d x %d: statuses %s, worst backward error %.3g of the bound' % (V, M, q, out['accel_status'].tolist(), worst))
    assert np.sum(out['accel_status'] == 0) >= 1


def test_every_status_lands_in_its_own_code_and_nothing_else_is_written():
    """One launch of fourteen starts at (14, 30, 12), one scenario each: rho inside the gate (0) and a factor two outside
    (4); a probe status != 0 at either end (2); NaN and inf in r_probe and in r_base (2); NaN in J (3); skip (1); a trust
    step with status 1 (1); max_step clipping the accelerated step (0, with entries of delta at the bound); a constructed step
    that does not descend in the model (5: the velocity along the soft direction of two nearly collinear columns, the
    acceleration along the stiff one).  In every case that is not applied the five in / out arrays keep the trust step's bits;
    lambda and dscale always (asserted in `geodesic`); n_accel moves exactly where the status is 0."""
    V, M, q = 14, 30, 12
    rng, J, r, theta, radius, _ = random_case(31, V, M, q, radii=[1e3, 1e-2, 5.0, 1e6, 1.0, 0.3, 1e3])
    CLIP, NODESC = 12, 13
    r[CLIP] *= 10.0
    radius[CLIP] = 1e6                          # the Gauss-Newton step, the longest of the launch
    J[NODESC, :, 1] = J[NODESC, :, 0] + 1e-2 * rng.standard_normal(M)
    soft, stiff = np.zeros(q), np.zeros(q)
    soft[0], soft[1], stiff[0], stiff[1] = 1.0, -1.0, 1.0, 1.0
    r[NODESC] = -J[NODESC] @ (0.1 * soft)       # the Gauss-Newton step is 0.1 (e0 - e1)
    radius[NODESC] = 1e6
    first = trust_step(J, r, np.zeros((V, q)), radius, np.zeros(V), theta, None, None, 0.0)
    max_step = (1.0 + 1e-3) * np.abs(first['delta']).max()
    assert np.abs(first['delta'][CLIP]).max() == np.abs(first['delta']).max()
    step = trust_step(J, r, np.zeros((V, q)), radius, np.zeros(V), theta, None, None, max_step)
    assert np.all(step['status'] == 0) and np.array_equal(step['delta'], first['delta'])          # nothing clipped yet
    c = np.stack([aim(J, step, v, rng.standard_normal(M), go.ALPHA / 2) for v in range(V)])
    c[1] = aim(J, step, 1, c[1], 2 * go.ALPHA)
    # the clipped one: 0.9 alpha, its sign such that the longest component grows
    c[CLIP] = aim(J, step, CLIP, c[CLIP], 0.9 * go.ALPHA)
    top = int(np.argmax(np.abs(step['delta'][CLIP])))
    a_clip = accel_of(J[CLIP], step['dscale'][CLIP], step['lam'][CLIP], c[CLIP], np.ones(q, dtype=bool))
    if a_clip[top] * step['delta'][CLIP][top] < 0:
        c[CLIP] = -c[CLIP]
    assert abs(0.5 * a_clip[top]) > 2e-3 * abs(step['delta'][CLIP][top])
    c[NODESC] = aim(J, step, NODESC, -J[NODESC] @ stiff, go.ALPHA / 2)
    r_base = r.copy()
    r_probe = probe_of(J, r_base, step, c, go.H)
    status_base, status_probe = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
    status_probe[2], status_base[3] = 4, 1
    r_probe[4, 7], r_probe[5, 0], r_base[6, M - 1], r_base[7, 3] = np.nan, np.inf, np.nan, -np.inf
    Jbad = J.copy()
    Jbad[8, 17, 5] = np.nan
    skip = np.zeros(V, dtype=np.int32)
    skip[9] = 1
    step_status = step['status'].copy()
    step_status[10] = 1
    want = [0, 4, 2, 2, 2, 2, 2, 2, 3, 1, 1, 0, 0, 5]
    out = geodesic(Jbad, r, r_base, r_probe, step, theta, max_step=max_step, skip=skip, status_base=status_base,
                   status_probe=status_probe, step_status=step_status)
    assert out['accel_status'].tolist() == want
    # the oracle on the starts it can be asked about as they are (skip and step_status are the caller's)
    ask = [v for v in range(V) if v not in (2, 3, 9, 10)]
    sub = lambda d: {k: a[ask] for k, a in d.items()}          # noqa: E731
    sub_out = sub(out)
    sub_out['n_accel'] = sub_out['n_accel'] - np.array(ask) + np.arange(len(ask))
    check_launch(Jbad[ask], r[ask], r_base[ask], r_probe[ask], sub(step), theta[ask], sub_out, max_step=max_step,
                 want=[want[v] for v in ask])
    for v in (2, 3, 9, 10):
        assert np.isnan(out['ratio'][v]) and out['n_accel'][v] == v + 5
        for k in INOUT:
            assert np.array_equal(out[k][v], step[k][v]), (v, k)
    assert np.sum(np.abs(out['delta'][CLIP]) == max_step) >= 1 and np.all(np.abs(out['delta']) <= max_step)
    assert out['n_accel'].tolist() == [v + 5 + (1 if want[v] == 0 else 0) for v in range(V)]


def test_a_probe_without_curvature_is_stopped_by_the_gate():
    """c = 0 in exact arithmetic: J = diag(1, 2, 4, 8), dyadic r and h = 1 / 8, so that the Gauss-Newton step, J v and the probe
    are exact and r_vv = 0 bit for bit: a = 0, status 4, rho = 0, nothing written.  The same launch with r_base = NULL."""
    V, M, q = 2, 4, 4
    J = np.tile(np.diag([1.0, 2.0, 4.0, 8.0]), (V, 1, 1))
    r = np.array([[0.5, -1.5, 3.0, 0.25], [1.0, 1.0, -2.0, 4.0]])
    theta = np.ones((V, q))
    step = trust_step(J, r, np.zeros((V, q)), np.full(V, 1e6), np.zeros(V), theta, None, None, 0.0)
    assert np.all(step['status'] == 0) and np.all(step['lam'] == 0.0)
    assert np.array_equal(step['delta'], -r / np.array([1.0, 2.0, 4.0, 8.0]))
    h = 0.125
    r_probe = probe_of(J, r, step, np.zeros((V, M)), h)
    assert np.array_equal(r_probe, r * (1.0 - h))
    for r_base in (r, None):
        out = geodesic(J, r, r_base, r_probe, step, theta, h=h)
        assert out['accel_status'].tolist() == [4, 4] and np.all(out['ratio'] == 0.0)
        assert out['n_accel'].tolist() == [5, 6]
        for k in INOUT:
            assert np.array_equal(out[k], step[k]), k


def test_arguments_are_checked():
    """h <= 0, alpha < 0 (and NaN), q > LM_MAX_Q and a NULL output are refused with SBM_E_ARG before anything is launched; V = 0
    is accepted."""
    import torch
    from sysbio_modeling_amd import _lib
    V, M, q = 2, 3, 2
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device='cuda')          # noqa: E731
    i32 = torch.int32
    ctx, p = _lib.default_context(), _lib.dev_ptr
    J, r, D, lam, th, delta, trial = z(V, M, q), z(V, M), z(V, q), z(V), z(V, q), z(V, q), z(V, q)
    pred, dxn, gtx, st, acc = z(V), z(V), z(V), z(V, dt=i32), z(V, dt=i32)

    def call(h=0.1, alpha=0.75, q_=q, V_=V, acc_=acc):
        return ctx.lib.sbm_lm_geodesic(ctx.handle, p(J), p(r), None, p(r), None, None, p(D), p(lam), V_, M, q_, None, None, p(st), None,
                                       h, alpha, 0.0, p(th), p(delta), p(trial), p(pred), p(dxn), p(gtx), p(acc_), None, None)
    assert call() == 0 and call(V_=0) == 0
    for bad in (dict(h=0.0), dict(h=-0.1), dict(h=float('nan')), dict(alpha=-1e-300), dict(alpha=float('nan')), dict(q_=129),
                dict(acc_=None)):
        assert call(**bad) == -1, bad          # SBM_E_ARG
    torch.cuda.synchronize()


def test_held_acceleration_equals_the_acceleration_of_the_reduced_problem_every_mask_in_one_launch():
    """(8, 70, 66), eight masks in ONE launch: none held, the first column, the last, two adjacent, all but one, all (status
    1), two random, and free columns on both sides of columns 63 / 64 only.  Each start against the unheld call on the arrays
    with its held columns deleted (the trust step's outputs included): the kernel compacts, so bitwise equality is expected
    and printed, 1e-13 asserted; the columns that are not free keep the trust step's bits."""
    rng, J, r, theta, radius, rs = random_case(41, 8, 70, 66, row_scale=True)
    V, M, q = J.shape
    held = np.zeros((V, q), dtype=bool)
    held[1, 0] = True
    held[2, q - 1] = True
    held[3, 30:32] = True
    held[4] = True
    held[4, 40] = False
    held[5] = True
    held[6, rng.choice(q, 2, replace=False)] = True
    held[7] = True
    held[7, [3, 62, 63, 64, 65]] = False
    step = trust_step(J, r, np.zeros((V, q)), radius, np.zeros(V), theta, rs, None, 0.0, held=held.astype(np.int32))
    assert step['status'].tolist() == [0, 0, 0, 0, 0, 2, 0, 0]
    Js = scaled(J, rs)
    c = np.zeros((V, M))
    for v in range(V):
        if v != 5:
            c[v] = aim(Js, step, v, rng.standard_normal(M), go.ALPHA / 2 if v != 3 else 2 * go.ALPHA, free=~held[v])
    r_base = r + 1e-9 * rng.standard_normal((V, M))
    r_probe = probe_of(Js, r_base, step, c, go.H)
    out = geodesic(J, r, r_base, r_probe, step, theta, row_scale=rs, held=held.astype(np.int32))
    want = [0, 0, 0, 4, 0, 1, 0, 0]
    check_launch(J, r, r_base, r_probe, step, theta, out, row_scale=rs, held=held, want=want, what='held, ')
    bitwise, worst = True, 0.0
    for v in range(V):
        free = ~held[v]
        for k in ('delta', 'trial'):
            assert np.array_equal(out[k][v][~free], step[k][v][~free]), (v, k)
        if not free.any():
            continue
        one = lambda a: a[v:v + 1]          # noqa: E731
        red_step = {k: (one(step[k])[:, free] if step[k].ndim == 2 else one(step[k])) for k in step}
        red = geodesic(one(J)[:, :, free], one(r), one(r_base), one(r_probe), red_step, one(theta)[:, free], row_scale=rs,
                       n_accel0=np.array([v + 5]))
        assert red['accel_status'][0] == out['accel_status'][v], v
        pairs = [(out[k][v][free], red[k][0]) for k in ('delta', 'trial')] + \
                [(out[k][v], red[k][0]) for k in ('pred', 'dxnorm', 'gtx', 'ratio', 'n_accel')]
        errs = [rel_err(a, b) for a, b in pairs]
        worst = max([worst] + errs)
        bitwise = bitwise and all(np.array_equal(a, b) for a, b in pairs)
        assert max(errs) <= REL, (v, errs)
    print('held acceleration against the reduced problem: bitwise equal: %s, worst relative error %.3g' % (bitwise, worst))


def replayed_lmpar(steps):
    """The trust steps a device loop recorded for one start (a list of (D, p, lam, pred, dxnorm, gtx, status) per iteration) as
    the ``lmpar`` of go.geodesic_fit_reference; past the record it is lo.lmpar_reference"""
    def lmpar(J, r, D, radius, it):
        return steps[it] if it < len(steps) else lo.lmpar_reference(J, r, D, radius)
    return lmpar


def test_device_loop_with_geodesic_steps_reaches_minpacks_minima_and_counts_as_the_oracle():
    """The loop of tests/test_gpu_lm_bookkeeping.py::test_device_loop_follows_the_oracle_at_every_step (no ODE: residuals
    and Jacobians of the three problems of oracle/lmder_oracle.py in torch, padded to V = 24, M = 30, q = 12) with the
    probe r(theta + h delta) evaluated in torch and sbm_lm_geodesic between the trust step and the trial point.  Every
    start lo.minpack_baseline keeps converges within ten times MINPACK's worst excess over c*.  The number of accelerated
    iterations per start is go.geodesic_fit_reference's, on the starts whose gates are not marginal (rho further than 1e-9
    alpha from alpha at every iteration); at most 2 of the 24 may be set aside.

    The reference loop is given the device's trust steps (`replayed_lmpar`): the kernel's lmpar is More's Newton
    iteration and lo.lmpar_reference a bisection, both stop anywhere within 10 % of the radius, so on a damped step the two
    loops legitimately hold different lambdas and walk different paths.  With the steps replayed everything the issue is
    about -- probe, acceleration, gate, the quantities of the step taken, lmder's bookkeeping -- is the oracle's own.  The
    count against the free-running reference is printed beside it."""
    import torch
    from sysbio_modeling_amd import _lib
    dev, f64, i32 = 'cuda', torch.float64, torch.int32
    probs = lo.problems()
    cstar, keep, minpack_worst = lo.minpack_baseline(probs)
    assert keep.sum() >= 20
    dprobs = [pb.to(dev) for pb in probs]
    V, M, q, max_iter = 24, max(pb.M for pb in probs), max(pb.q for pb in probs), 100
    x0 = np.zeros((V, q))
    for i, pb in enumerate(probs):
        x0[8 * i:8 * i + 8, :pb.q] = pb.starts

    def residuals(X):
        r = torch.zeros((V, M), dtype=f64, device=dev)
        for i, pb in enumerate(dprobs):
            rows = slice(8 * i, 8 * i + 8)
            r[rows, :pb.M] = pb.residuals(X[rows, :pb.q])
            for k in range(pb.q, q):
                r[rows, pb.M + k - pb.q] = X[rows, k]
        return r

    def evaluate(X):
        J = torch.zeros((V, M, q), dtype=f64, device=dev)
        for i, pb in enumerate(dprobs):
            rows = slice(8 * i, 8 * i + 8)
            J[rows, :pb.M, :pb.q] = pb.jacobian(X[rows, :pb.q])
            for k in range(pb.q, q):
                J[rows, pb.M + k - pb.q, k] = 1.0
        r = residuals(X)
        return r, J, (r * r).sum(dim=1)

    th = torch.from_numpy(x0).to(dev)
    r, J, norms = evaluate(th)
    cost = 0.5 * norms
    col = torch.sqrt((J * J).sum(dim=1))
    radius = (100.0 * (torch.where(col > 0, col, torch.ones_like(col)) * th).norm(dim=1)).contiguous()
    dscale = torch.zeros((V, q), dtype=f64, device=dev)
    lam = torch.zeros((V,), dtype=f64, device=dev)
    done, accept = torch.zeros((V,), dtype=i32, device=dev), torch.zeros((V,), dtype=i32, device=dev)
    n_iter = torch.full((V,), max_iter, dtype=i32, device=dev)
    status_t = torch.zeros((V,), dtype=i32, device=dev)
    counters = torch.zeros((2,), dtype=i32, device=dev)
    delta, trial = (torch.empty((V, q), dtype=f64, device=dev) for _ in range(2))
    pred, dxnorm, gtx, rho = (torch.empty((V,), dtype=f64, device=dev) for _ in range(4))
    st, accel_st = torch.empty((V,), dtype=i32, device=dev), torch.empty((V,), dtype=i32, device=dev)
    n_accel = torch.zeros((V,), dtype=i32, device=dev)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    host = lambda *ts: [t.cpu().numpy().copy() for t in ts]          # noqa: E731
    record, rhos = [], []
    live = V
    for it in range(max_iter):
        _lib.check(ctx.lib.sbm_lm_trust_step_ex(ctx.handle, p(J), p(r), p(dscale), p(radius), p(lam), V, M, q, None, p(done), 0.0,
                                                p(th), p(trial), p(delta), p(pred), p(dxnorm), p(gtx), p(st)), 'sbm_lm_trust_step_ex')
        record.append(host(dscale, delta, lam, pred, dxnorm, gtx, st, done))
        r_probe = residuals(th + go.H * delta)
        _lib.check(ctx.lib.sbm_lm_geodesic(ctx.handle, p(J), p(r), None, p(r_probe), None, None, p(dscale), p(lam), V, M, q, None,
                                           p(done), p(st), None, go.H, go.ALPHA, 0.0, p(th), p(delta), p(trial), p(pred),
                                           p(dxnorm), p(gtx), p(accel_st), p(rho), p(n_accel)), 'sbm_lm_geodesic')
        rhos.append(host(rho)[0])
        r_t, J_t, norms_t = evaluate(trial)
        _lib.check(ctx.lib.sbm_lm_update(ctx.handle, p(cost), p(norms_t), p(status_t), p(pred), p(dxnorm), p(gtx), p(st), p(th),
                                         p(dscale), V, q, lo.FTOL, lo.XTOL, it, 1 if it == 0 else 0, p(radius), p(lam), p(done),
                                         p(accept), p(n_iter), p(counters), None), 'sbm_lm_update')
        _lib.check(ctx.lib.sbm_lm_accept(ctx.handle, p(accept), V, M, q, p(trial), p(r_t), p(J_t), p(norms_t), p(th), p(r), p(J),
                                         p(cost)), 'sbm_lm_accept')
        live = int(counters.cpu()[0])
        if live == 0:
            break
    assert live == 0, 'not converged in %d iterations' % max_iter
    final, counts, iters = cost.cpu().numpy(), n_accel.cpu().numpy(), n_iter.cpu().numpy()
    ours = 0.0
    for i in range(len(probs)):
        for j in range(8):
            if keep[i, j]:
                excess = (final[8 * i + j] - cstar[i]) / (lo.FTOL * cstar[i])
                ours = max(ours, excess)
                assert excess <= 10.0 * minpack_worst, (probs[i].name, j, excess, minpack_worst)
    rhos = np.array(rhos)                                   # [iterations][V]
    aside, free_running_differs, wrong = [], [], []
    for i, pb in enumerate(probs):
        for j in range(8):
            v = 8 * i + j
            steps = [(rec[0][v, :pb.q], rec[1][v, :pb.q], float(rec[2][v]), float(rec[3][v]), float(rec[4][v]), float(rec[5][v]),
                      int(rec[6][v])) for rec in record if not rec[7][v]]
            ref = go.geodesic_fit_reference(pb.fun, pb.jac, pb.starts[j], lmpar=replayed_lmpar(steps))
            seen = rhos[:iters[v], v]
            marginal = bool(np.any(np.abs(seen[~np.isnan(seen)] - go.ALPHA) <= 1e-9 * go.ALPHA)) or \
                any(abs(x - go.ALPHA) <= 1e-9 * go.ALPHA for x in ref['rho'] if x == x)
            if marginal:
                aside.append(v)
            elif counts[v] != ref['n_accel']:
                wrong.append((pb.name, j, int(counts[v]), ref['n_accel']))
            if counts[v] != go.geodesic_fit_reference(pb.fun, pb.jac, pb.starts[j])['n_accel']:
                free_running_differs.append(v)
    print('geodesic device loop: %d iterations; accelerated per start %s; excess over c* in units of ftol c*: MINPACK %.3g, '
          'device loop %.3g; set aside (marginal gate) %s; starts whose count differs from the free-running reference: %s'
          % (it + 1, counts.tolist(), minpack_worst, ours, aside, free_running_differs))
    assert not wrong, wrong
    assert len(aside) <= 2, aside
    assert counts.min() >= 1


def test_geodesic_step_orders_the_pointers():
    """project/_evaluation.py::geodesic_step, the one place that orders the tensors of the C call, against the call spelled out
    in `geodesic` above: every output equal bit for bit, with a row_scale, a skip flag, a held mask and probe statuses in."""
    import torch
    from sysbio_modeling_amd import _lib
    from sysbio_modeling_amd.project._evaluation import geodesic_step
    rng, J, r, theta, radius, rs = random_case(77, 6, 20, 7, row_scale=True)
    V, M, q = J.shape
    held = np.zeros((V, q), dtype=np.int32)
    held[1, 2] = held[4, 0] = 1
    skip = np.array([0, 0, 1, 0, 0, 0], dtype=np.int32)
    status_base, status_probe = np.array([0, 0, 0, 2, 0, 0], dtype=np.int32), np.array([0, 0, 0, 0, 0, 1], dtype=np.int32)
    max_step = 0.7
    step = trust_step(J, r, np.zeros((V, q)), radius, np.zeros(V), theta, rs, None, max_step, held=held)
    Js = scaled(J, rs)
    c = np.stack([aim(Js, step, v, rng.standard_normal(M), go.ALPHA / 2, free=held[v] == 0) for v in range(V)])
    r_base = r + 1e-9 * rng.standard_normal((V, M))
    r_probe = probe_of(Js, r_base, step, c, go.H)
    kw = dict(max_step=max_step, row_scale=rs, skip=skip, held=held, status_base=status_base, status_probe=status_probe)
    want = geodesic(J, r, r_base, r_probe, step, theta, **kw)
    assert want['accel_status'].tolist()[2:] == [1, 2, 0, 2] and 0 in want['accel_status'][:2]
    f64, i32 = torch.float64, torch.int32
    t = lambda x, dt=f64: torch.from_numpy(np.ascontiguousarray(x)).to('cuda').to(dt)          # noqa: E731
    got = {k: t(step[k]) for k in INOUT}
    got.update(accel_status=t(np.full(V, -7), i32), ratio=t(np.full(V, -77.0)), n_accel=t(np.arange(V) + 5, i32))
    geodesic_step(_lib.default_context(), J=t(J), r=t(r), r_base=t(r_base), r_probe=t(r_probe), status_base=t(status_base, i32),
                  status_probe=t(status_probe, i32), dscale=t(step['dscale']), lam=t(step['lam']), row_scale=t(rs), skip=t(skip, i32),
                  step_status=t(step['status'], i32), held=t(held, i32), h=go.H, alpha=go.ALPHA, max_step=max_step, theta=t(theta),
                  delta=got['delta'], trial=got['trial'], pred=got['pred'], dxnorm=got['dxnorm'], gtx=got['gtx'],
                  accel_status=got['accel_status'], ratio=got['ratio'], n_accel=got['n_accel'])
    torch.cuda.synchronize()
    for k, a in want.items():
        assert np.array_equal(got[k].cpu().numpy(), a, equal_nan=True), k
