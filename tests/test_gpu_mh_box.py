"""The box forms of the sampler's step kernels: ``sbm_mh_propose_box`` against numpy and ``sbm_mh_propose``, and the veto of
``sbm_mh_accept_ex`` / ``sbm_mh_accept_hastings_ex`` against the host rule and the entries without it (include/sbm.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _propose_box(curr, samp, z, held=None, lower=None, upper=None):
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    p = _lib.dev_ptr
    C, q = curr.shape
    trial = torch.full((C, q), 7.0, dtype=torch.float64, device='cuda')
    outside = torch.full((C,), 7, dtype=torch.int32, device='cuda')
    t = [_dev(curr), _dev(samp), _dev(z), _dev(held, torch.int32), _dev(lower), _dev(upper)]
    _lib.check(ctx.lib.sbm_mh_propose_box(ctx.handle, p(t[0]), p(t[1]), int(samp.ndim == 3), p(t[2]), C, q, p(t[3]), p(t[4]), p(t[5]),
                                          p(trial), p(outside)), 'sbm_mh_propose_box')
    torch.cuda.synchronize()
    return trial.cpu().numpy(), outside.cpu().numpy()


def _propose(curr, samp, z):
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    p = _lib.dev_ptr
    C, q = curr.shape
    trial = torch.full((C, q), 7.0, dtype=torch.float64, device='cuda')
    t = [_dev(curr), _dev(samp), _dev(z)]
    _lib.check(ctx.lib.sbm_mh_propose(ctx.handle, p(t[0]), p(t[1]), int(samp.ndim == 3), p(t[2]), C, q, p(trial)), 'sbm_mh_propose')
    torch.cuda.synchronize()
    return trial.cpu().numpy()


@pytest.mark.parametrize('per_chain', [0, 1])
@pytest.mark.parametrize('C, q', [(9, 5), (3, 70)])
def test_propose_box_against_numpy(C, q, per_chain):
    """q = 70 takes two passes of the lanes, C = 9 three workgroups with a last one of one chain.  Chain 0 leaves the box
    through its last free component, chain 1 lands exactly on an upper bound (z a unit vector: the sum is one product, so
    numpy's candidate has the kernel's bits) and counts as inside, chain 2 stays inside with full draws; with more chains,
    chain 3 has everything held (no candidate: outside), chain 4 is outside below a lower bound, chain 5 has a NaN draw, the
    others stay inside."""
    rng = np.random.default_rng(100 * C + q + per_chain)
    curr = rng.standard_normal((C, q))
    samp = rng.standard_normal((C, q, q) if per_chain else (q, q)) * 0.3
    z = rng.standard_normal((C, q))
    held = rng.random((C, q)) < 0.3
    held[:, 0] = False                       # (something free in every chain ...)
    z[1] = 0.0
    z[1, q - 2] = 1.0
    if C > 3:
        held[3] = True                       # (... but this one)
    S = np.broadcast_to(samp, (C, q, q))
    terms = S * z[:, None, :]
    cand = curr + terms.sum(axis=2)
    mag = np.abs(curr) + np.abs(terms).sum(axis=2)
    lower, upper = cand - 1.0, cand + 1.0
    lower[rng.random((C, q)) < 0.2] = -np.inf
    upper[rng.random((C, q)) < 0.2] = np.inf
    last_free = [int(np.flatnonzero(~held[c])[-1]) for c in range(C) if not held[c].all()]
    upper[0, last_free[0]] = cand[0, last_free[0]] - 0.1
    upper[1, 0] = cand[1, 0]                 # = fl(curr + samp[0][q - 2]): exact on both sides
    want_out = np.zeros(C, dtype=np.int32)
    want_out[0] = 1
    if C > 3:
        lower[4, 0] = cand[4, 0] + 1e-9
        z[5, q // 2] = np.nan
        want_out[[3, 4, 5]] = 1
    # held columns are exempt: bounds that exclude them change nothing
    lower[held], upper[held] = 50.0, 60.0
    trial, outside = _propose_box(curr, samp, z, held, lower, upper)
    assert np.array_equal(outside, want_out)
    out = want_out.astype(bool)
    assert np.array_equal(trial[out], curr[out])
    assert np.array_equal(trial[held], curr[held])
    moved = ~out[:, None] & ~held
    assert moved[1].any() and moved[2].sum() > q // 2
    assert np.all(np.abs(trial - cand)[moved] <= 4 * q * EPS * mag[moved])
    assert trial[1, 0] == upper[1, 0]
    assert np.all((trial >= lower)[moved] & (trial <= upper)[moved])


@pytest.mark.parametrize('per_chain', [0, 1])
@pytest.mark.parametrize('C, q', [(9, 5), (3, 70)])
def test_propose_box_without_a_box_is_propose(C, q, per_chain):
    rng = np.random.default_rng(7 * C + q)
    curr = rng.standard_normal((C, q))
    samp = rng.standard_normal((C, q, q) if per_chain else (q, q))
    z = rng.standard_normal((C, q))
    ref = _propose(curr, samp, z)
    inf = np.full((C, q), np.inf)
    for held, lower, upper in ((None, None, None), (np.zeros((C, q), bool), -inf, inf), (None, -inf, inf),
                               (np.zeros((C, q), bool), None, None)):
        trial, outside = _propose_box(curr, samp, z, held, lower, upper)
        assert np.array_equal(trial, ref) and np.array_equal(outside, np.zeros(C, dtype=np.int32))
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    t = _dev(curr)
    o = _dev(np.zeros(C, dtype=np.int32))
    p = _lib.dev_ptr
    assert ctx.lib.sbm_mh_propose_box(ctx.handle, p(t), p(t), 0, p(t), C, q, None, p(t), None, p(_dev(curr)), p(o)) == -1   # lower alone
    assert ctx.lib.sbm_mh_propose_box(ctx.handle, p(t), p(t), 0, p(t), C, q, None, None, None, p(t), p(o)) == -1           # trial is curr


def _signed(V):
    idx = np.argmax(np.abs(V), axis=-2)
    sign = np.sign(np.take_along_axis(V, idx[..., None, :], axis=-2))
    return V * np.where(sign == 0.0, 1.0, sign)


def _spd(rng, C, q):
    B = rng.standard_normal((C, q, q + 2)) * 10.0 ** rng.uniform(-1.0, 1.0, (C, q, 1))
    return np.einsum('cik,cjk->cij', B, B)


def _accept(entry, st, veto):
    """One acceptance call on copies of the state ``st``; every array afterwards"""
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    p = _lib.dev_ptr
    C, q = st['curr'].shape
    i32 = torch.int32
    t = {k: _dev(st[k]) for k in ('norms', 'entropy', 'log_u', 'trial', 'curr', 'F', 'Vc', 'sc', 'Mc', 'Vt', 'st', 'Mt')}
    t.update(status=_dev(st['status'], i32), n=_dev(st['n'], i32), ax=_dev(st['ax'], i32), veto=_dev(veto, i32),
             slot=torch.full((C, q), 7.0, dtype=torch.float64, device='cuda'), slot_F=torch.full((C,), 7.0, dtype=torch.float64, device='cuda'))
    head = (ctx.handle, p(t['norms']), p(t['status']), p(t['entropy']), p(t['log_u']), st['T'], C, q, p(t['trial']), p(t['curr']),
            p(t['F']), p(t['n']), p(t['slot']), p(t['slot_F']))
    axes = (p(t['Vc']), p(t['sc']), p(t['Mc']), p(t['Vt']), p(t['st']), p(t['Mt']), p(t['ax']))
    if entry == 'accept':
        rc = ctx.lib.sbm_mh_accept(*head)
    elif entry == 'accept_ex':
        rc = ctx.lib.sbm_mh_accept_ex(*head, p(t['veto']))
    elif entry == 'hastings':
        rc = ctx.lib.sbm_mh_accept_hastings(*head, *axes)
    else:
        rc = ctx.lib.sbm_mh_accept_hastings_ex(*head, *axes, p(t['veto']))
    assert rc == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items() if v is not None}


def _state(rng, C, q, held=None):
    """Chains, trial points and axes at both ends (padded for ``held``), with log_u placed at least 1e-5 from the ratio of
    either rule.  Returns the state and the two ratios."""
    from sysbio_modeling_amd.project.ensembles import _log_candidate_density, sampling_axes
    T = 1.5
    axes = [sampling_axes(_spd(rng, C, q), 1e-4, T, 1.0, held=held) for _ in range(2)]
    (Vc, sc), (Vt, st) = [(_signed(V), s) for V, s in axes]
    Mc, Mt = Vc * sc[:, None, :], Vt * st[:, None, :]
    curr = rng.standard_normal((C, q))
    delta = np.einsum('cij,cj->ci', Mc, rng.standard_normal((C, q)))
    if held is not None:
        delta[np.broadcast_to(held, (C, q))] = 0.0
    trial = curr + delta
    delta = trial - curr
    F = rng.uniform(1.0, 5.0, C)
    norms = 2.0 * (F + rng.uniform(-2.0, 2.0, C))
    entropy = rng.uniform(-0.5, 0.5, C)
    status, ax = np.zeros(C, dtype=np.int32), np.zeros(C, dtype=np.int32)
    status[5] = 2
    ax[6] = 1
    Ft = 0.5 * norms - entropy
    plain = -(Ft - F) / T
    hastings = plain + _log_candidate_density(-delta, Vt, st) - _log_candidate_density(delta, Vc, sc)
    st_ = dict(T=T, norms=norms, entropy=entropy, trial=trial, curr=curr, F=F, Vc=Vc, sc=sc, Mc=Mc, Vt=Vt, st=st, Mt=Mt,
               status=status, ax=ax, n=rng.integers(0, 4, C).astype(np.int32), Ft=Ft, delta=delta)
    return st_, plain, hastings


def _log_u(rng, ratio, below):
    """below: chains whose log_u sits under the ratio (they would be accepted), the others above; 1e-5 to 1 away"""
    off = 10.0 ** rng.uniform(-5.0, 0.0, len(ratio))
    log_u = np.where(below, ratio - off, ratio + off)
    assert np.all(np.abs(log_u - ratio) > 1e-6)
    return log_u


VETO = np.array([1, 0, 3, 0, -1, 0, 0, 1], dtype=np.int32)         # half of the chains, any non-zero value
BELOW = np.array([1, 1, 1, 0, 0, 1, 1, 0], dtype=bool)              # vetoed chains 0 and 2 would be accepted


def _check(got, st, acc, hastings):
    assert np.array_equal(got['n'], st['n'] + acc)
    assert np.array_equal(got['curr'], np.where(acc[:, None], st['trial'], st['curr']))
    assert np.array_equal(got['F'], np.where(acc, st['Ft'], st['F']))
    assert np.array_equal(got['slot'], got['curr']) and np.array_equal(got['slot_F'], got['F'])
    for now, t, c in (('Vc', 'Vt', 'Vc'), ('sc', 'st', 'sc'), ('Mc', 'Mt', 'Mc')):
        a = acc.reshape((-1,) + (1,) * (st[c].ndim - 1)) if hastings else np.zeros_like(acc).reshape((-1,) + (1,) * (st[c].ndim - 1))
        assert np.array_equal(got[now], np.where(a, st[t], st[c]))
    for k in ('trial', 'Vt', 'st', 'Mt'):
        assert np.array_equal(got[k], st[k])


def test_accept_ex_veto_against_the_host_rule():
    rng = np.random.default_rng(83)
    C, q = 8, 3
    st, plain, hastings = _state(rng, C, q)
    ok = (st['status'] == 0) & np.isfinite(st['Ft'])
    for entry, old, ratio, extra in (('accept_ex', 'accept', plain, ok), ('hastings_ex', 'hastings', hastings, ok & (st['ax'] == 0))):
        st['log_u'] = _log_u(rng, ratio, BELOW)
        free_acc = extra & (st['log_u'] < ratio)
        acc = free_acc & (VETO == 0)
        assert acc.any() and (free_acc & (VETO != 0)).sum() >= 2
        _check(_accept(entry, st, VETO), st, acc, entry == 'hastings_ex')
        # no veto: the entry of before, to the bit
        a, b = _accept(entry, st, None), _accept(old, st, None)
        _check(a, st, free_acc, entry == 'hastings_ex')
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        z = _accept(entry, st, np.zeros(C, dtype=np.int32))
        assert all(np.array_equal(a[k], z[k]) for k in a)


def test_hastings_on_padded_axes_decides_as_the_reduced_problem():
    """nf = 2 of 3: the padded axes of sampling_axes(held=) at both ends of moves without a held component.  The ratio of the
    reduced problem -- the density of the 2 x 2 blocks alone -- decides, and the kernel decides alike on the padded arrays."""
    from sysbio_modeling_amd.project.ensembles import _log_candidate_density
    rng = np.random.default_rng(84)
    C, q = 8, 3
    held = np.array([False, True, False])
    st, plain, hastings = _state(rng, C, q, held=held)
    free = np.flatnonzero(~held)
    assert np.all(st['delta'][:, held] == 0.0) and np.all(st['sc'][:, 2] == 1.0) and np.all(st['Vc'][:, held] == 0.0)
    d = st['delta'][:, free]
    red = plain + _log_candidate_density(-d, st['Vt'][:, free][:, :, :2], st['st'][:, :2]) \
        - _log_candidate_density(d, st['Vc'][:, free][:, :, :2], st['sc'][:, :2])
    assert np.allclose(red, hastings, rtol=1e-12, atol=1e-12)
    st['log_u'] = _log_u(rng, red, BELOW)
    ok = (st['status'] == 0) & np.isfinite(st['Ft']) & (st['ax'] == 0)
    acc = ok & (st['log_u'] < red)
    assert 0 < acc.sum() < C
    _check(_accept('hastings_ex', st, None), st, acc, True)
    _check(_accept('hastings_ex', st, VETO), st, acc & (VETO == 0), True)
