"""The per-step functions of project/_evaluation.py (``trust_step``, ``mh_propose``, ``mh_accept``, ``sampling_axes``) against
the direct ctypes call each stands for, on the raw bytes of every tensor of the call.  Every pointer of the C ABI is a void*,
so this is where the order of the tensors is checked: the shapes are the smallest at which two tensors of one shape cannot
be exchanged unseen (every tensor holds values of its own), and reference and wrapper write into separate outputs
prefilled with a sentinel, so that an output nobody wrote shows as well."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -77


def both(arrays, direct, wrapped):
    """``arrays``: name -> numpy array or None (inputs, in / out tensors with their start values, outputs via `out`).  Each of
    the two callables gets device copies of its own, ``call(t, ctx, p)``.  Every tensor is compared on bytes after the calls;
    returns the reference's arrays."""
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    sets = []
    for call in (direct, wrapped):
        t = {k: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda') for k, a in arrays.items()}
        call(t, ctx, _lib.dev_ptr)
        ctx.synchronize()
        torch.cuda.synchronize()
        sets.append({k: v.cpu().numpy() for k, v in t.items() if v is not None})
    ref, got = sets
    for k in ref:
        assert ref[k].tobytes() == got[k].tobytes(), (k, ref[k], got[k])
    return ref


def out(shape, dtype=np.float64):
    return np.full(shape, SENTINEL, dtype=dtype)


def written(a):
    return not np.any(a == SENTINEL)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['plain', 'held', 'bounded', 'bounded_held'])
def test_trust_step(case):
    """V = 3, M = 5, q = 3; start 1 is skipped; with ``held`` start 2 has nothing free and start 0 holds one column; with
    bounds column 2 of start 0 sits in a box of +-1e-3 that its step (of order 1) leaves, so that component ends on a bound."""
    from sysbio_modeling_amd.project._evaluation import trust_step
    V, M, q = 3, 5, 3
    rng = np.random.default_rng(11)
    theta = rng.standard_normal((V, q))
    a = dict(J=rng.standard_normal((V, M, q)), r=rng.standard_normal((V, M)), dscale=rng.uniform(0.5, 2.0, (V, q)),
             radius=rng.uniform(5.0, 9.0, V), lam=rng.uniform(0.1, 0.2, V), row_scale=rng.uniform(0.5, 1.5, M),
             skip=np.array([0, 1, 0], dtype=np.int32), theta=theta, trial=out((V, q)), delta=out((V, q)), pred=out(V),
             dxnorm=out(V), gtx=out(V), status=out(V, np.int32), held=None, lower=None, upper=None)
    # start 0: the columns of the row-scaled Jacobian are orthogonal, so its normal equations are diagonal and a step with one
    # component cut short by a bound still descends (the bounded step takes it: status 0, not 4)
    a['J'][0] = np.linalg.qr(a['J'][0])[0] * np.array([1.0, 1.5, 2.0]) / a['row_scale'][:, None]
    if 'held' in case:
        a['held'] = np.array([[0, 1, 0], [0, 0, 0], [1, 1, 1]], dtype=np.int32)
    if 'bounded' in case:
        a['lower'], a['upper'] = theta - 3.0, theta + 3.0
        a['lower'][0, 2], a['upper'][0, 2] = theta[0, 2] - 1e-3, theta[0, 2] + 1e-3
    max_step = 0.7

    def direct(t, ctx, p):
        from sysbio_modeling_amd import _lib
        head = (ctx.handle, p(t['J']), p(t['r']), p(t['dscale']), p(t['radius']), p(t['lam']), V, M, q, p(t['row_scale']),
                p(t['skip']), max_step, p(t['theta']), p(t['trial']), p(t['delta']), p(t['pred']), p(t['dxnorm']), p(t['gtx']),
                p(t['status']))
        if 'bounded' in case:
            _lib.check(ctx.lib.sbm_lm_trust_step_bounded(*head, p(t['held']), p(t['lower']), p(t['upper']), None))
        elif case == 'held':
            _lib.check(ctx.lib.sbm_lm_trust_step_held(*head, p(t['held'])))
        else:
            _lib.check(ctx.lib.sbm_lm_trust_step_ex(*head))

    def wrapped(t, ctx, p):
        trust_step(ctx, J=t['J'], r=t['r'], dscale=t['dscale'], radius=t['radius'], lam=t['lam'], row_scale=t['row_scale'],
                   skip=t['skip'], max_step=max_step, theta=t['theta'], trial=t['trial'], delta=t['delta'], pred=t['pred'],
                   dxnorm=t['dxnorm'], gtx=t['gtx'], status=t['status'], held=t['held'], lower=t['lower'], upper=t['upper'])

    ref = both(a, direct, wrapped)
    for k in ('trial', 'delta', 'pred', 'dxnorm', 'gtx', 'status'):
        assert written(ref[k][0]), (k, ref[k])
    assert written(ref['status'][2])
    assert not np.array_equal(ref['dscale'], a['dscale'])          # the in / out tensors moved: the comparison saw them
    if 'held' in case:
        assert np.array_equal(ref['trial'][2], theta[2]) and ref['trial'][0, 1] == theta[0, 1]
    if 'bounded' in case:
        assert ref['status'][0] == 0 and ref['trial'][0, 2] in (a['lower'][0, 2], a['upper'][0, 2]), (ref['trial'][0], ref['status'])


def test_trust_step_without_the_optional_tensors_is_sbm_lm_trust_step():
    """The call of the tensor-select loop: no row scale, skip list, clip, theta / trial or gtx."""
    from sysbio_modeling_amd.project._evaluation import trust_step
    V, M, q = 3, 5, 3
    rng = np.random.default_rng(12)
    a = dict(J=rng.standard_normal((V, M, q)), r=rng.standard_normal((V, M)), dscale=rng.uniform(0.5, 2.0, (V, q)),
             radius=rng.uniform(0.1, 0.2, V), lam=rng.uniform(0.1, 0.2, V), delta=out((V, q)), pred=out(V), dxnorm=out(V),
             status=out(V, np.int32))

    def direct(t, ctx, p):
        from sysbio_modeling_amd import _lib
        _lib.check(ctx.lib.sbm_lm_trust_step(ctx.handle, p(t['J']), p(t['r']), p(t['dscale']), p(t['radius']), p(t['lam']), V, M,
                                             q, p(t['delta']), p(t['pred']), p(t['dxnorm']), p(t['status'])))

    ref = both(a, direct, lambda t, ctx, p: trust_step(ctx, **t))
    assert all(written(ref[k]) for k in ('delta', 'pred', 'dxnorm', 'status'))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('box', ['plain', 'held', 'bounds', 'held_bounds'])
@pytest.mark.parametrize('per_chain', [False, True])
@pytest.mark.parametrize('q', [3, 65])
def test_mh_propose(q, per_chain, box):
    """C = 5; q = 65 crosses one lane stride of k_mh_propose_box.  Chain 1 sits in a box of +-1e-9 (its candidate is outside),
    chain 3 has every component held."""
    from sysbio_modeling_amd.project._evaluation import mh_propose
    C = 5
    rng = np.random.default_rng(q)
    curr = rng.standard_normal((C, q))
    a = dict(curr=curr, samp=0.1 * rng.standard_normal((C, q, q) if per_chain else (q, q)), z=rng.standard_normal((C, q)),
             trial=out((C, q)), held=None, lower=None, upper=None, outside=None)
    if box != 'plain':
        a['outside'] = out(C, np.int32)
    if 'held' in box:
        a['held'] = ((np.arange(C)[:, None] + np.arange(q)[None, :]) % 3 == 0).astype(np.int32)      # some held, some free
        a['held'][3] = 1
    if 'bounds' in box:
        a['lower'], a['upper'] = curr - 50.0, curr + 50.0
        a['lower'][1], a['upper'][1] = curr[1] - 1e-9, curr[1] + 1e-9

    def direct(t, ctx, p):
        from sysbio_modeling_amd import _lib
        if box == 'plain':
            _lib.check(ctx.lib.sbm_mh_propose(ctx.handle, p(t['curr']), p(t['samp']), int(per_chain), p(t['z']), C, q, p(t['trial'])))
        else:
            _lib.check(ctx.lib.sbm_mh_propose_box(ctx.handle, p(t['curr']), p(t['samp']), int(per_chain), p(t['z']), C, q, p(t['held']),
                                                  p(t['lower']), p(t['upper']), p(t['trial']), p(t['outside'])))

    ref = both(a, direct, lambda t, ctx, p: mh_propose(ctx, **t))
    assert written(ref['trial']) and not np.array_equal(ref['trial'][0], curr[0])
    if box != 'plain':
        want = np.zeros(C, dtype=np.int32)
        want[1] = 'bounds' in box
        want[3] = 'held' in box
        assert np.array_equal(ref['outside'], want), ref['outside']


# ---------------------------------------------------------------------------------------------------------------------
def _accept_case(rng, C, q, T, entropy, axes):
    """Inputs of an acceptance: log_u is placed 0.5 from the ratio of every chain (computed here as include/sbm.h states
    it), below it in chains 0, 2, 4 and above it in 1, 3: no decision hangs on a rounding."""
    from sysbio_modeling_amd.project.ensembles import _log_candidate_density
    curr = rng.standard_normal((C, q))
    trial = curr + 0.1 * rng.standard_normal((C, q))
    norms = rng.uniform(1.0, 2.0, C)
    F_curr = rng.uniform(0.3, 0.9, C)
    ent = rng.uniform(0.1, 0.2, C) if entropy else None
    ratio = -((0.5 * norms - (ent if entropy else 0.0)) - F_curr) / T
    a = dict(norms=norms, status=np.zeros(C, dtype=np.int32), entropy=ent, trial=trial, curr=curr, F_curr=F_curr,
             n_accepted=np.arange(10, 10 + C, dtype=np.int32))
    if axes:
        def one():
            V = np.linalg.qr(rng.standard_normal((C, q, q)))[0]
            s = rng.uniform(0.5, 1.5, (C, q))
            return [V, s, V * s[:, None, :]]
        a['axes_curr'], a['axes_trial'] = one(), one()
        a['axes_status'] = np.zeros(C, dtype=np.int32)
        ratio = ratio + _log_candidate_density(curr - trial, *a['axes_trial'][:2]) - _log_candidate_density(trial - curr, *a['axes_curr'][:2])
    a['log_u'] = ratio + np.where(np.arange(C) % 2 == 0, -0.5, 0.5)
    return a


@pytest.mark.parametrize('entropy', [False, True])
@pytest.mark.parametrize('slot', [False, True])
@pytest.mark.parametrize('veto', [False, True])
def test_mh_accept(veto, slot, entropy):
    """C = 5, q = 3 against sbm_mh_accept_ex: chains 0, 2, 4 accept, 1 and 3 reject; the veto takes chain 2 back."""
    from sysbio_modeling_amd.project._evaluation import mh_accept
    C, q, T = 5, 3, 1.5
    a = _accept_case(np.random.default_rng(21), C, q, T, entropy, False)
    a.update(ens_slot=out((C, q)) if slot else None, ens_F_slot=out(C) if slot else None,
             veto=np.array([0, 0, 1, 0, 0], dtype=np.int32) if veto else None)

    def direct(t, ctx, p):
        from sysbio_modeling_amd import _lib
        _lib.check(ctx.lib.sbm_mh_accept_ex(ctx.handle, p(t['norms']), p(t['status']), p(t['entropy']), p(t['log_u']), T, C, q,
                                            p(t['trial']), p(t['curr']), p(t['F_curr']), p(t['n_accepted']), p(t['ens_slot']),
                                            p(t['ens_F_slot']), p(t['veto'])))

    ref = both(a, direct, lambda t, ctx, p: mh_accept(ctx, temperature=T, **t))
    taken = np.array([1, 0, 0 if veto else 1, 0, 1])
    assert np.array_equal(ref['n_accepted'] - a['n_accepted'], taken), ref['n_accepted']
    assert np.array_equal(ref['curr'], np.where(taken[:, None] == 1, a['trial'], a['curr']))
    if slot:
        assert np.array_equal(ref['ens_slot'], ref['curr']) and np.array_equal(ref['ens_F_slot'], ref['F_curr'])


@pytest.mark.parametrize('veto', [False, True])
def test_mh_accept_with_axes(veto):
    """C = 5, q = 3 against sbm_mh_accept_hastings_ex, the six axes tensors all different: chains 0, 2, 4 accept and take the
    trial axes with them; chain 4's trial axes have status 1 (rejected), the veto takes chain 2 back."""
    from sysbio_modeling_amd.project._evaluation import mh_accept
    C, q, T = 5, 3, 1.5
    a = _accept_case(np.random.default_rng(22), C, q, T, True, True)
    a['axes_status'][4] = 1
    a.update(ens_slot=out((C, q)), ens_F_slot=out(C), veto=np.array([0, 0, 1, 0, 0], dtype=np.int32) if veto else None)
    flat = dict(a)
    for end in ('axes_curr', 'axes_trial'):
        for name, arr in zip(('V', 's', 'samp'), flat.pop(end)):
            flat['%s_%s' % (end, name)] = arr
    axes = lambda t, end: [t['%s_%s' % (end, name)] for name in ('V', 's', 'samp')]          # noqa: E731

    def direct(t, ctx, p):
        from sysbio_modeling_amd import _lib
        _lib.check(ctx.lib.sbm_mh_accept_hastings_ex(ctx.handle, p(t['norms']), p(t['status']), p(t['entropy']), p(t['log_u']), T, C, q,
                                                     p(t['trial']), p(t['curr']), p(t['F_curr']), p(t['n_accepted']), p(t['ens_slot']),
                                                     p(t['ens_F_slot']), *(p(x) for x in axes(t, 'axes_curr')),
                                                     *(p(x) for x in axes(t, 'axes_trial')), p(t['axes_status']), p(t['veto'])))

    def wrapped(t, ctx, p):
        mh_accept(ctx, temperature=T, axes_curr=axes(t, 'axes_curr'), axes_trial=axes(t, 'axes_trial'),
                  **{k: v for k, v in t.items() if not k.startswith(('axes_curr', 'axes_trial'))})

    ref = both(flat, direct, wrapped)
    taken = np.array([1, 0, 0 if veto else 1, 0, 0])
    assert np.array_equal(ref['n_accepted'] - a['n_accepted'], taken), ref['n_accepted']
    for k, name in enumerate(('V', 's', 'samp')):
        moved = np.where(taken.reshape((C,) + (1,) * (a['axes_curr'][k].ndim - 1)) == 1, a['axes_trial'][k], a['axes_curr'][k])
        assert np.array_equal(ref['axes_curr_' + name], moved), name


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('held', [False, True])
@pytest.mark.parametrize('source', ['J', 'J_row_scale', 'H', 'H_per_chain'])
def test_sampling_axes(source, held):
    """q = 7, C = 3, M = 9 against sbm_sampling_axes_held; with ``held`` chain 0 holds two columns, chain 2 all of them."""
    from sysbio_modeling_amd.project._evaluation import sampling_axes
    C, M, q = 3, 9, 7
    rng = np.random.default_rng(31)
    a = dict(J=None, row_scale=None, H=None, eig=out((C, q)), V=out((C, q, q)), s=out((C, q)), samp=out((C, q, q)),
             status=out(C, np.int32), held=None)
    if source.startswith('J'):
        a['J'] = rng.standard_normal((C, M, q))
        if source == 'J_row_scale':
            a['row_scale'] = rng.uniform(0.5, 1.5, M)
    else:
        B = rng.standard_normal((C, M, q))
        H = np.einsum('cmj,cmk->cjk', B, B)
        a['H'] = H if source == 'H_per_chain' else H[0]
    if held:
        a['held'] = np.zeros((C, q), dtype=np.int32)
        a['held'][0, [1, 4]] = 1
        a['held'][2] = 1
    cutoff, T, step_scale = 1e-2, 1.5, 0.3

    def direct(t, ctx, p):
        from sysbio_modeling_amd import _lib
        _lib.check(ctx.lib.sbm_sampling_axes_held(ctx.handle, p(t['J']), p(t['row_scale']), p(t['H']), int(source == 'H_per_chain'), C,
                                                  M if t['J'] is not None else 0, q, cutoff, T, step_scale, p(t['eig']), p(t['V']),
                                                  p(t['s']), p(t['samp']), p(t['status']), p(t['held'])))

    ref = both(a, direct, lambda t, ctx, p: sampling_axes(ctx, cutoff=cutoff, temperature=T, step_scale=step_scale, **t))
    assert all(written(ref[k]) for k in ('eig', 'V', 's', 'samp', 'status')) and not ref['status'].any()
    assert np.allclose(ref['samp'], ref['V'] * ref['s'][:, None, :], rtol=1e-14, atol=0)
    if source == 'H':
        assert held or np.array_equal(ref['V'][0], ref['V'][1])          # one Hessian for all chains
    else:
        assert not np.array_equal(ref['V'][0], ref['V'][1])
