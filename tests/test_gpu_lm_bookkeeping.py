"""sbm_lm_update and sbm_lm_accept -- lmder's bookkeeping of fit_batch(algorithm='trust_region') -- against the MINPACK
oracle of oracle/lmder_oracle.py (written from lmder.f and the contract in sbm.h, tested on the CPU against real MINPACK in
tests/test_lmder_oracle.py): a random sweep over every branch, the hand-worked cases, the composed loop on the device
held to the oracle at every step, and every copy path of the accept kernel."""
import numpy as np
import pytest

from oracle import lmder_oracle as lo

pytestmark = pytest.mark.gpu

REL = 1.0e-13          # radius, lambda, ratio: at most a dozen correctly rounded operations on same-signed terms
SENTINEL = -123.456


def rel_err(got, want):
    if got == want:
        return 0.0
    return abs(got - want) / max(abs(want), 5e-324)


class UpdateCall:
    """One sbm_lm_update launch on V starts of a dict of arrays.  Every buffer carries one more element than V: valid
    inputs of a start that is not done, outputs prefilled -- a thread that runs past V shows in them instead of writing
    out of bounds."""

    def __init__(self, d, V, q, ftol, xtol, iteration, first, with_ratio=True, counters=(0, 0)):
        import torch
        from sysbio_modeling_amd import _lib
        dev = 'cuda'

        def padded(a, guard):
            a = np.asarray(a)
            tail = np.full((1,) + a.shape[1:], guard, dtype=a.dtype)
            return torch.from_numpy(np.ascontiguousarray(np.concatenate([a[:V], tail]))).to(dev)
        # the guard start: an ordinary good step (the 'grow' case), not done
        g = dict(cost=2.0, norms_trial=1.0, status_trial=0, pred=1.0, dxnorm=1.0, gtx=-1.5, step_status=0, theta=1.0, dscale=1.0,
                 radius=8.0, lam=0.5, done=0, n_iter=-5)
        self.t = {k: padded(d[k], g[k]) for k in lo.UPDATE_FIELDS}
        self.t['accept'] = torch.full((V + 1,), -7, dtype=torch.int32, device=dev)
        self.t['ratio'] = torch.full((V + 1,), SENTINEL, dtype=torch.float64, device=dev)
        self.t['counters'] = torch.tensor(list(counters), dtype=torch.int32, device=dev)
        t, p, ctx = self.t, _lib.dev_ptr, _lib.default_context()
        _lib.check(ctx.lib.sbm_lm_update(ctx.handle, p(t['cost']), p(t['norms_trial']), p(t['status_trial']), p(t['pred']),
                                         p(t['dxnorm']), p(t['gtx']), p(t['step_status']), p(t['theta']), p(t['dscale']), V, q,
                                         float(ftol), float(xtol), int(iteration), int(first), p(t['radius']), p(t['lam']),
                                         p(t['done']), p(t['accept']), p(t['n_iter']), p(t['counters']),
                                         p(t['ratio']) if with_ratio else None), 'sbm_lm_update')
        torch.cuda.synchronize()
        self.out = {k: t[k].cpu().numpy() for k in ('radius', 'lam', 'done', 'accept', 'n_iter', 'ratio', 'counters')}
        self.V, self.guard = V, g

    def guard_untouched(self):
        o, V, g = self.out, self.V, self.guard
        return (o['accept'][V] == -7 and o['ratio'][V] == SENTINEL and o['radius'][V] == g['radius'] and o['lam'][V] == g['lam']
                and o['done'][V] == 0 and o['n_iter'][V] == -5)


def compare_with_oracle(d, out, V, ftol, xtol, iteration, first, marginal=None, what=''):
    """Rows 0..V-1 of a launch's outputs against lm_update_reference.  Returns (live, accepted, worst relative error)."""
    live = accepted = 0
    worst = 0.0
    for v in range(V):
        args = lo.update_args(d, v, ftol, xtol, iteration, first)
        ref = lo.lm_update_reference(*args)
        where = '%sstart %d (%s)' % (what, v, ref.branch)
        if ref.branch == 'done':
            # untouched, bit for bit; the trial point is not taken
            assert out['radius'][v] == d['radius'][v] and out['lam'][v] == d['lam'][v] and out['n_iter'][v] == d['n_iter'][v], where
            assert out['done'][v] == 1 and out['accept'][v] == 0, where
            if 'ratio' in out:
                assert out['ratio'][v] == SENTINEL, where
            continue
        errs = [rel_err(out['radius'][v], ref.radius), rel_err(out['lam'][v], ref.lam)]
        if 'ratio' in out:
            errs.append(rel_err(out['ratio'][v], ref.ratio))
        worst = max([worst] + errs)
        if marginal is not None and marginal[v]:
            # on a threshold either side may be taken: the integer outputs (and what follows from them) are not demanded
            live += 1 - int(out['done'][v])
            accepted += int(out['accept'][v])
            continue
        assert max(errs) <= REL, (where, errs, out['radius'][v], ref.radius, out['lam'][v], ref.lam)
        assert (out['accept'][v], out['done'][v], out['n_iter'][v]) == (ref.accept, ref.done, ref.n_iter), where
        live += ref.live
        accepted += ref.accepted
    return live, accepted, worst


def test_update_random_sweep_matches_the_oracle():
    """V = 1000 (four blocks, the last ragged), q = 7, log-uniform inputs over many decades arranged to populate every branch
    (tests/test_lmder_oracle.py checks the coverage), both values of `first`.  Draws on a threshold are removed first.
    accept, done, n_iter and both counters exactly; radius, lambda, ratio to 1e-13; starts already done come back bit
    for bit; nothing is written past V."""
    q = lo.SWEEP_Q
    d = lo.draw_update_inputs(1000, q, lo.SWEEP_SEED)
    keep = np.array([not any(lo.lm_update_is_marginal(*lo.update_args(d, v, lo.FTOL, lo.XTOL, 3, f)) for f in (0, 1))
                     for v in range(1000)])
    assert keep.sum() >= 950
    d = {k: np.ascontiguousarray(a[keep]) for k, a in d.items()}
    V = int(keep.sum())
    was_done = d['done'] != 0
    assert 50 <= was_done.sum() <= 150
    d['radius'][was_done] = SENTINEL
    d['lam'][was_done] = SENTINEL
    d['n_iter'][was_done] = -5
    assert (V + 255) // 256 == 4 and V % 256 != 0
    for first in (0, 1):
        call = UpdateCall(d, V, q, lo.FTOL, lo.XTOL, 3, first, counters=(-7, -7))
        live, accepted, worst = compare_with_oracle(d, call.out, V, lo.FTOL, lo.XTOL, 3, first, what='first = %d, ' % first)
        print('first = %d: worst relative error of radius / lambda / ratio %.3g; live %d, accepted %d' % (first, worst, live, accepted))
        assert call.out['counters'].tolist() == [live, accepted]
        assert call.guard_untouched()
    # ratio_out = NULL is accepted and changes nothing else
    no_ratio = UpdateCall(d, V, q, lo.FTOL, lo.XTOL, 3, 1, with_ratio=False)
    for k in ('radius', 'lam', 'done', 'accept', 'n_iter', 'counters'):
        assert np.array_equal(no_ratio.out[k], call.out[k]), k
    assert np.all(no_ratio.out['ratio'] == SENTINEL)
    # V = 0: the counters are zeroed, nothing else is touched
    empty = UpdateCall(d, 0, q, lo.FTOL, lo.XTOL, 3, 1, counters=(-7, -7))
    assert empty.out['counters'].tolist() == [0, 0] and empty.guard_untouched()


def test_update_named_cases():
    """The hand-worked cases of tests/test_lmder_oracle.py as one V = 10 launch (first = 1: only the two first-rule cases
    have a step shorter than the radius), against the same literals."""
    d, _, expected = lo.named_cases()
    V = len(expected)
    call = UpdateCall(d, V, 2, lo.NAMED_FTOL, lo.NAMED_XTOL, lo.NAMED_ITERATION, 1)
    o = call.out
    for v, (label, want) in enumerate(expected):
        got = dict(radius=o['radius'][v], lam=o['lam'][v], done=o['done'][v], accept=o['accept'][v], n_iter=o['n_iter'][v],
                   ratio=o['ratio'][v] if want['ratio'] is not None else None)
        for key, val in got.items():
            assert val == want[key], 'case %d, branch %s: %s = %r, expected %r' % (v, label, key, val, want[key])
        if want['ratio'] is None:
            assert o['ratio'][v] == SENTINEL, label
    assert o['counters'].tolist() == [sum(w['live'] for _, w in expected), sum(w['accepted'] for _, w in expected)]
    assert call.guard_untouched()


def test_device_loop_follows_the_oracle_at_every_step():
    """The default fitting loop without an ODE: sbm_lm_trust_step_ex, residuals and Jacobian of the trial points in torch,
    sbm_lm_update, sbm_lm_accept, on the three problems of tests/test_lmder_oracle.py -- 3 x 8 starts padded to one batch of
    V = 24, M = 30, q = 12: a padding parameter gets a residual row of its own, r = theta_k, zero at the start and at the
    minimum, so that every Jacobian keeps full column rank and no cost changes; the remaining rows are zero.  After every sbm_lm_update its inputs and outputs are checked against
    lm_update_reference (integers exactly away from the thresholds, floats to 1e-13), after every sbm_lm_accept the four
    arrays against lm_accept_reference bit for bit; at the end every start has converged to MINPACK's minimum c*
    (leastsq at ftol = xtol = 1e-14) within the bound of the CPU test: ten times MINPACK's own worst excess at default
    tolerances.

    Measured excess over c* in units of ftol c*: MINPACK 6.2e-4, the oracle loop 7.1e-4, this loop 6.2e-4."""
    import torch
    from sysbio_modeling_amd import _lib
    dev, f64, i32 = 'cuda', torch.float64, torch.int32
    probs = lo.problems()
    cstar, keep, minpack_worst = lo.minpack_baseline(probs)
    assert keep.sum() >= 20
    dprobs = [pb.to(dev) for pb in probs]
    V, M, q, max_iter = 24, max(pb.M for pb in probs), max(pb.q for pb in probs), 100
    assert all(pb.M + q - pb.q <= M for pb in probs)
    x0 = np.zeros((V, q))
    for i, pb in enumerate(probs):
        x0[8 * i:8 * i + 8, :pb.q] = pb.starts

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
    r, J, norms = evaluate(th)
    cost = 0.5 * norms
    # lmder: D from the first Jacobian, Delta = 100 ||D theta||
    col = torch.sqrt((J * J).sum(dim=1))
    radius = (100.0 * (torch.where(col > 0, col, torch.ones_like(col)) * th).norm(dim=1)).contiguous()
    dscale = torch.zeros((V, q), dtype=f64, device=dev)
    lam = torch.zeros((V,), dtype=f64, device=dev)
    done, accept = torch.zeros((V,), dtype=i32, device=dev), torch.zeros((V,), dtype=i32, device=dev)
    n_iter = torch.full((V,), max_iter, dtype=i32, device=dev)
    status_t = torch.zeros((V,), dtype=i32, device=dev)
    counters = torch.zeros((2,), dtype=i32, device=dev)
    delta, trial = (torch.empty((V, q), dtype=f64, device=dev) for _ in range(2))
    pred, dxnorm, gtx, ratio = (torch.empty((V,), dtype=f64, device=dev) for _ in range(4))
    st = torch.empty((V,), dtype=i32, device=dev)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    host = lambda *ts: [t.cpu().numpy().copy() for t in ts]          # noqa: E731
    pairs = n_marginal = 0
    worst = 0.0
    for it in range(max_iter):
        _lib.check(ctx.lib.sbm_lm_trust_step_ex(ctx.handle, p(J), p(r), p(dscale), p(radius), p(lam), V, M, q, None, p(done), 0.0,
                                                p(th), p(trial), p(delta), p(pred), p(dxnorm), p(gtx), p(st)), 'sbm_lm_trust_step_ex')
        r_t, J_t, norms_t = evaluate(trial)
        ratio.fill_(SENTINEL)
        keys = ('cost', 'norms_trial', 'status_trial', 'pred', 'dxnorm', 'gtx', 'step_status', 'theta', 'dscale', 'radius', 'lam',
                'done', 'n_iter')
        d = dict(zip(keys, host(cost, norms_t, status_t, pred, dxnorm, gtx, st, th, dscale, radius, lam, done, n_iter)))
        first = 1 if it == 0 else 0
        _lib.check(ctx.lib.sbm_lm_update(ctx.handle, p(cost), p(norms_t), p(status_t), p(pred), p(dxnorm), p(gtx), p(st), p(th),
                                         p(dscale), V, q, lo.FTOL, lo.XTOL, it, first, p(radius), p(lam), p(done), p(accept),
                                         p(n_iter), p(counters), p(ratio)), 'sbm_lm_update')
        out = dict(zip(('radius', 'lam', 'done', 'accept', 'n_iter', 'ratio', 'counters'),
                       host(radius, lam, done, accept, n_iter, ratio, counters)))
        marginal = [lo.lm_update_is_marginal(*lo.update_args(d, v, lo.FTOL, lo.XTOL, it, first)) for v in range(V)]
        running = int((d['done'] == 0).sum())
        pairs += running
        n_marginal += sum(marginal)
        live, accepted, w = compare_with_oracle(d, out, V, lo.FTOL, lo.XTOL, it, first, marginal, what='iteration %d, ' % it)
        worst = max(worst, w)
        assert out['counters'].tolist() == [live, accepted], it
        before = host(th, r, J, cost)
        sources = host(trial, r_t, J_t, norms_t)
        _lib.check(ctx.lib.sbm_lm_accept(ctx.handle, p(accept), V, M, q, p(trial), p(r_t), p(J_t), p(norms_t), p(th), p(r), p(J),
                                         p(cost)), 'sbm_lm_accept')
        want = lo.lm_accept_reference(out['accept'], *sources, *before)
        for name, got, ref in zip(('theta', 'r', 'J', 'cost'), host(th, r, J, cost), want):
            assert np.array_equal(got, ref), (it, name)
        if live == 0:
            break
    assert live == 0, 'not converged in %d iterations' % max_iter
    assert n_marginal <= 0.02 * pairs, (n_marginal, pairs)
    final = cost.cpu().numpy()
    ours = 0.0
    for i in range(len(probs)):
        for j in range(8):
            if keep[i, j]:
                excess = (final[8 * i + j] - cstar[i]) / (lo.FTOL * cstar[i])
                ours = max(ours, excess)
                assert excess <= 10.0 * minpack_worst, (probs[i].name, j, excess, minpack_worst)
    print('device loop: %d iterations, %d (start, iteration) pairs, %d marginal, worst float error %.3g; excess over c* in '
          'units of ftol c*: MINPACK %.3g, device loop %.3g' % (it + 1, pairs, n_marginal, worst, minpack_worst, ours))


ACCEPT_SHAPES = [(5, 9, 7),          # M q odd: odd rows take the scalar path, even rows the 16-byte one
                 (4, 10, 6),         # even, one block in y
                 (3, 70, 68),        # gridDim.y = 2
                 (2, 2100, 128)]     # 66 blocks' worth in y, capped at 64: the grid-stride loop wraps


def guarded(n, fill, offset=2):
    """A view of n doubles starting `offset` doubles into a flat tensor (2: 16-byte aligned, 1: only 8-byte aligned), one
    guard element on each side."""
    import torch
    flat = torch.full((n + 4,), 7.25, dtype=torch.float64, device='cuda')
    view = flat[offset:offset + n]
    view.copy_(fill)
    assert view.data_ptr() % 16 == (0 if offset % 2 == 0 else 8)
    return flat, view


def run_accept(V, M, q, accept, j_offset=2):
    import torch
    from sysbio_modeling_amd import _lib
    dev = 'cuda'
    sizes = dict(theta=V * q, r=V * M, J=V * M * q, cost=V)
    dst, src, before = {}, {}, {}
    for k, n in sizes.items():
        ramp = torch.arange(n, dtype=torch.float64, device=dev)          # distinct per element, and between the buffers
        off = j_offset if k == 'J' else 2
        dst[k] = guarded(n, ramp + 0.25, off)
        src[k] = guarded(n, -ramp - 0.5, off)
        before[k] = dst[k][1].clone()
    acc = torch.tensor(accept, dtype=torch.int32, device=dev)
    ctx, p = _lib.default_context(), _lib.dev_ptr
    _lib.check(ctx.lib.sbm_lm_accept(ctx.handle, p(acc), V, M, q, p(src['theta'][1]), p(src['r'][1]), p(src['J'][1]),
                                     p(src['cost'][1]), p(dst['theta'][1]), p(dst['r'][1]), p(dst['J'][1]), p(dst['cost'][1])),
               'sbm_lm_accept')
    torch.cuda.synchronize()
    for k, n in sizes.items():
        flat, view = dst[k]
        off = j_offset if k == 'J' else 2
        assert flat[off - 1].item() == 7.25 and flat[off + n].item() == 7.25, 'guard of %s' % k
        got, old, new = view.view(V, -1), before[k].view(V, -1), src[k][1].view(V, -1)
        if k == 'cost':
            new = 0.5 * new
        for v in range(V):
            assert torch.equal(got[v], new[v] if accept[v] else old[v]), '%s, row %d, accept %d' % (k, v, accept[v])
        sflat = src[k][0]
        assert sflat[off - 1].item() == 7.25 and sflat[off + n].item() == 7.25 and torch.equal(src[k][1], -torch.arange(
            n, dtype=torch.float64, device=dev) - 0.5), 'source %s changed' % k


@pytest.mark.parametrize('V,M,q', ACCEPT_SHAPES)
def test_accept_every_copy_path(V, M, q):
    """Accepted rows of theta, r, J equal the trial arrays bit for bit and cost = 0.5 norms_trial, rejected rows keep what
    they held, one guard element on each side of every buffer stays: all, none, alternating, only the last row."""
    for accept in ([1] * V, [0] * V, [v % 2 for v in range(V)], [0] * (V - 1) + [1]):
        run_accept(V, M, q, accept)


def test_accept_with_jacobians_that_are_only_8_byte_aligned():
    """Even M q, but J and J_trial are views that start one double into their allocations: the 16-byte copy path must not
    be taken on the strength of the element offset alone."""
    for accept in ([1, 1, 1, 1], [0, 1, 0, 1]):
        run_accept(4, 10, 6, accept, j_offset=1)
