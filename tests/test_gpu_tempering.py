"""Parallel tempering on the device: ``sbm_project_sf_entropy_pt`` and ``sbm_mh_accept_pt`` against their scalar entries,
``sbm_pt_swap`` against the numpy rule (tests/support/tempering_oracle.py), ``ensemble_log_params_batch(sampler='device')``
with a temperature ladder against a replay with the same draws, and the statistics of every rung."""
import numpy as np
import pytest

from tests.support import tempering_oracle as po
from tests.test_gpu_sampler_device import _Synthetic, _gaussian_posterior_project, _targets

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------
# sbm_project_sf_entropy_pt
# ---------------------------------------------------------------------------
def _entropy_pt(proj, sims, T):
    """(rc, entropy (V,), group_entropy (V, G)) of sbm_project_sf_entropy_pt, outputs pre-filled with 7; T None is NULL"""
    import torch
    from sysbio_modeling_amd import _lib
    sd = _dev(sims)
    V = sd.shape[0]
    ent = torch.full((V,), 7.0, dtype=torch.float64, device='cuda')
    grp = torch.full((V, proj.G), 7.0, dtype=torch.float64, device='cuda')
    rc = proj.lib.sbm_project_sf_entropy_pt(proj.handle, _lib.dev_ptr(sd), V, _lib.dev_ptr(None if T is None else _dev(T)),
                                            _lib.dev_ptr(ent), _lib.dev_ptr(grp))
    torch.cuda.synchronize()
    return rc, ent.cpu().numpy(), grp.cpu().numpy()


@pytest.mark.parametrize('sizes, V', [((7,), 5), ((70,), 67), ((1, 7, 70, 3, 12), 67), ((1, 7, 70, 3, 12), 5)])
def test_entropy_pt_is_the_scalar_entry_vector_by_vector(gpu_models, sizes, V):
    """Groups of 1, 7 and 70 rows (70: two passes of rows over the lanes), G = 1 and G = 5 (wavefront 0 takes a second
    group), V = 5 and 67.  All temperatures 1.5: the bits of sbm_project_sf_entropy(..., 1.5, ...).  One temperature per
    vector in [1, 2.5]: row v is the scalar entry's row v at T[v], to the bit.  A NULL temperature pointer: -1."""
    G = len(sizes)
    rng = np.random.default_rng(40 + G + V)
    proj = _Synthetic(gpu_models('simple'), sizes, 9, D=10.0 ** rng.uniform(0.0, 4.0, G), mu=rng.uniform(-0.5, 0.5, G),
                      prior_sigma=rng.uniform(0.2, 2.0, G), seed=50 + G)
    try:
        X, bstar = _targets(rng, proj, V)
        sims = proj.sims(rng, X, bstar)
        rc, ent, grp = _entropy_pt(proj, sims, np.full(V, 1.5))
        rc1, ent1, grp1 = proj.entropy(sims, 1.5)
        assert rc == 0 and rc1 == 0 and np.all(np.isfinite(grp1))
        assert np.array_equal(ent, ent1) and np.array_equal(grp, grp1)
        T = rng.uniform(1.0, 2.5, V)
        T[0], T[-1] = 1.0, 2.5
        rc, ent, grp = _entropy_pt(proj, sims, T)
        assert rc == 0
        for v in range(V):
            _, ent_v, grp_v = proj.entropy(sims, T[v])
            assert ent[v] == ent_v[v] and np.array_equal(grp[v], grp_v[v]), v
        assert len(np.unique(ent)) == V
        # a temperature that is not positive: that vector's entropy is -inf, the others keep their bits
        bad = T.copy()
        bad[1] = 0.0
        rc, ent_b, grp_b = _entropy_pt(proj, sims, bad)
        assert rc == 0 and ent_b[1] == -np.inf and np.all(grp_b[1] == -np.inf)
        assert np.array_equal(np.delete(ent_b, 1), np.delete(ent, 1)) and np.array_equal(np.delete(grp_b, 1, 0), np.delete(grp, 1, 0))
        rc, ent_n, _ = _entropy_pt(proj, sims, None)
        assert rc == -1 and np.all(ent_n == 7.0) and b'NULL' in proj.lib.sbm_last_error()
    finally:
        proj.close()


# ---------------------------------------------------------------------------
# sbm_mh_accept_pt
# ---------------------------------------------------------------------------
def _accept(st, T, veto, slots, entropy):
    """One acceptance on copies of ``st``: sbm_mh_accept_ex for a number ``T``, sbm_mh_accept_pt for an array; every output"""
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    p = _lib.dev_ptr
    C, q = st['curr'].shape
    t = dict(norms=_dev(st['norms']), status=_dev(st['status'], torch.int32), entropy=_dev(st['entropy']) if entropy else None,
             log_u=_dev(st['log_u']), trial=_dev(st['trial']), curr=_dev(st['curr']), F=_dev(st['F']), n=_dev(st['n'], torch.int32),
             slot=torch.full((C, q), 7.0, dtype=torch.float64, device='cuda') if slots else None,
             slot_F=torch.full((C,), 7.0, dtype=torch.float64, device='cuda') if slots else None,
             veto=_dev(st['veto'], torch.int32) if veto else None)
    head = (ctx.handle, p(t['norms']), p(t['status']), p(t['entropy']), p(t['log_u']))
    tail = (C, q, p(t['trial']), p(t['curr']), p(t['F']), p(t['n']), p(t['slot']), p(t['slot_F']), p(t['veto']))
    if np.ndim(T) == 0:
        rc = ctx.lib.sbm_mh_accept_ex(*head, float(T), *tail)
    else:
        Td = _dev(T)
        rc = ctx.lib.sbm_mh_accept_pt(*head, p(Td), *tail)
    assert rc == 0, ctx.lib.sbm_last_error()
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in ('curr', 'F', 'n', 'slot', 'slot_F') if t[k] is not None}


def _accept_state(rng, C, q):
    F = rng.uniform(1.0, 5.0, C)
    st = dict(curr=rng.standard_normal((C, q)), trial=rng.standard_normal((C, q)), F=F, norms=2.0 * (F + rng.uniform(-2.0, 2.0, C)),
              entropy=rng.uniform(-0.5, 0.5, C), log_u=np.log(rng.random(C)), status=np.zeros(C, dtype=np.int32),
              n=np.arange(C, dtype=np.int32), veto=(np.arange(C) % 4 == 1).astype(np.int32))
    st['status'][C - 1] = 2                 # the last chain cannot move,
    st['log_u'][0] = -50.0                  # the first one does
    return st


@pytest.mark.parametrize('entropy', [False, True])
@pytest.mark.parametrize('slots', [False, True])
@pytest.mark.parametrize('veto', [False, True])
def test_accept_pt_with_equal_temperatures_is_accept_ex(veto, slots, entropy):
    rng = np.random.default_rng(5)
    for C, q in ((9, 5), (3, 70)):
        st = _accept_state(rng, C, q)
        ref = _accept(st, 1.5, veto, slots, entropy)
        got = _accept(st, np.full(C, 1.5), veto, slots, entropy)
        assert sorted(ref) == sorted(got) and all(np.array_equal(ref[k], got[k]) for k in ref)
        assert 0 < (ref['n'] - st['n']).sum() < C


@pytest.mark.parametrize('C, q', [(9, 5), (3, 70)])
def test_accept_pt_rule_with_one_temperature_per_chain(C, q):
    """Against the numpy rule, temperatures powers of two and energies small integers, so that -(Ft - Fc) / T is exact: chain
    0 has log_u equal to the bound -- strict <, it stays --, chain 1 one ulp below it and moves, chain 2 one ulp above."""
    rng = np.random.default_rng(6 + C)
    T = 2.0 ** rng.integers(-1, 4, C)
    T[:3] = (4.0, 0.5, 2.0)
    Fc = rng.integers(1, 9, C).astype(float)
    Ft = Fc + rng.integers(1, 6, C)                                   # uphill: the bound is negative
    bound = -(Ft - Fc) / T
    log_u = bound + rng.choice([-0.75, 0.75], C)
    log_u[:3] = bound[0], np.nextafter(bound[1], -np.inf), np.nextafter(bound[2], np.inf)
    st = dict(curr=rng.standard_normal((C, q)), trial=rng.standard_normal((C, q)), F=Fc, norms=2.0 * Ft, entropy=np.zeros(C),
              log_u=log_u, status=np.zeros(C, dtype=np.int32), n=np.zeros(C, dtype=np.int32), veto=np.zeros(C, dtype=np.int32))
    acc = log_u < bound
    assert acc[:3].tolist() == [False, True, False]
    got = _accept(st, T, False, True, False)
    assert np.array_equal(got['n'], acc.astype(np.int32))
    assert np.array_equal(got['curr'], np.where(acc[:, None], st['trial'], st['curr'])) and np.array_equal(got['slot'], got['curr'])
    assert np.array_equal(got['F'], np.where(acc, Ft, Fc)) and np.array_equal(got['slot_F'], got['F'])
    # a chain whose temperature is not positive stays
    T2 = T.copy()
    T2[1] = 0.0
    assert _accept(st, T2, False, False, False)['n'][1] == 0


def test_accept_pt_through_the_step_function():
    """``_evaluation.mh_accept`` with a temperature tensor is sbm_mh_accept_pt, tensor for tensor"""
    import torch
    from sysbio_modeling_amd import _lib
    from sysbio_modeling_amd.project._evaluation import mh_accept
    rng = np.random.default_rng(7)
    C, q = 5, 3
    st = _accept_state(rng, C, q)
    T = rng.uniform(1.0, 3.0, C)
    ref = _accept(st, T, True, True, True)
    t = dict(norms=_dev(st['norms']), status=_dev(st['status'], torch.int32), entropy=_dev(st['entropy']), log_u=_dev(st['log_u']),
             trial=_dev(st['trial']), curr=_dev(st['curr']), F_curr=_dev(st['F']), n_accepted=_dev(st['n'], torch.int32),
             ens_slot=torch.full((C, q), 7.0, dtype=torch.float64, device='cuda'),
             ens_F_slot=torch.full((C,), 7.0, dtype=torch.float64, device='cuda'), veto=_dev(st['veto'], torch.int32))
    mh_accept(_lib.default_context(), temperature=_dev(T), **t)
    torch.cuda.synchronize()
    for k, name in (('curr', 'curr'), ('F', 'F_curr'), ('n', 'n_accepted'), ('slot', 'ens_slot'), ('slot_F', 'ens_F_slot')):
        assert np.array_equal(ref[k], t[name].cpu().numpy())
    with pytest.raises(ValueError):
        mh_accept(_lib.default_context(), temperature=_dev(T[:2]), **t)


# ---------------------------------------------------------------------------
# sbm_pt_swap
# ---------------------------------------------------------------------------
def _swap(st, K, parity, cross, slots, null=None):
    """sbm_pt_swap on copies of ``st``: (rc, every array afterwards).  ``null``: the name of an argument to pass as NULL."""
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    p = _lib.dev_ptr
    C, q = st['curr'].shape
    t = dict(T=_dev(st['T']), X=_dev(st['X']) if cross else None, log_u=_dev(st['log_u']), curr=_dev(st['curr']), F=_dev(st['F']),
             n=_dev(st['n'], torch.int32), slot=_dev(st['slot']) if slots else None, slot_F=_dev(st['slot_F']) if slots else None)
    a = {k: (None if k == null else v) for k, v in t.items()}
    rc = ctx.lib.sbm_pt_swap(ctx.handle, C, q, K, parity, p(a['T']), p(a['X']), p(a['log_u']), p(a['curr']), p(a['F']), p(a['n']),
                             p(a['slot']), p(a['slot_F']))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items() if v is not None}


def _swap_state(rng, C, K, q, parity, offset, cross, spoil=None):
    """Chains whose swap bounds are exact (temperatures powers of two, energies small integers): the pairs of this parity
    cycle through accept (log_u one ulp below the bound), reject (one ulp above) and the tie (log_u == bound), starting at
    ``offset``.  ``spoil`` = inf or nan: the cross energy of one member of every pair that would be accepted is that.  Every
    array that the kernel may write is pre-filled with something it must keep; one entry of curr per chain is a NaN with a
    payload, and log_u of the chains that are not a lower chain is NaN: it is not to be looked at."""
    T = np.tile(2.0 ** np.arange(K), C // K)
    F = rng.integers(1, 20, C).astype(float)
    X = F + rng.integers(-3, 4, C) if cross else F.copy()
    curr = rng.standard_normal((C, q))
    nan_bits = np.uint64(0x7FF8000000000000) + np.arange(1, C + 1, dtype=np.uint64)
    curr[np.arange(C), np.arange(C) % q] = nan_bits.view(np.float64)
    i = po.lower_chains(C, K, parity)
    kind = (np.arange(len(i)) + offset) % 3                          # 0 accept, 1 reject, 2 tie
    bound = po.swap_bound(T, F, X, i)
    log_u = np.full(C, np.nan)
    log_u[i] = np.where(kind == 0, np.nextafter(bound, -np.inf), np.where(kind == 1, np.nextafter(bound, np.inf), bound))
    want = i[kind == 0]
    if spoil is not None:
        X = X.copy()
        X[want[0::2]] = spoil                                        # the lower member of one pair, the upper of the next
        X[want[1::2] + 1] = spoil
        want = want[:0]
    st = dict(T=T, F=F, X=X, curr=curr, log_u=log_u, n=np.arange(10, 10 + C, dtype=np.int32), slot=np.full((C, q), 7.0),
              slot_F=np.full(C, 7.0))
    return st, want


@pytest.mark.parametrize('parity', [0, 1])
@pytest.mark.parametrize('C, K, q', [(8, 4, 5), (66, 3, 70), (6, 2, 1), (5, 5, 3)])
def test_pt_swap_against_the_oracle(C, K, q, parity):
    """(8, 4, 5) baseline; (66, 3, 70): pairs straddle workgroups (four chains each) and q takes two lane passes; (6, 2, 1):
    q = 1, and parity 1 has no pair at all; (5, 5, 3): odd K -- the top rung is idle on parity 0, the bottom one on parity 1.
    Per shape and parity: accepted, rejected and exact-tie pairs (each pair is each in turn), a cross energy of +inf and of
    NaN, F_cross NULL, slots NULL and given.  Everything is compared bit for bit with the oracle's step on the same arrays:
    rows outside an exchanged pair -- all rows, where nothing swaps -- keep their bits, NaN payloads included, and n_swapped
    counts at the lower chains only."""
    rng = np.random.default_rng(1000 * C + 10 * q + parity)
    n_taken = 0
    cases = [(offset, cross, slots, None) for offset in range(3) for cross in (True, False) for slots in (True, False)]
    cases += [(0, True, True, np.inf), (0, True, False, np.nan)]
    for offset, cross, slots, spoil in cases:
        st, want = _swap_state(rng, C, K, q, parity, offset, cross, spoil)
        ref = po.swap_step(K, parity, st['T'], st['X'] if cross else None, st['log_u'], st['curr'], st['F'], st['n'],
                           st['slot'] if slots else None, st['slot_F'] if slots else None)
        assert np.array_equal(ref[5], want)                           # the oracle takes the pairs the state was built for
        rc, got = _swap(st, K, parity, cross, slots)
        assert rc == 0
        assert np.array_equal(_bits(got['curr']), _bits(ref[0])) and np.array_equal(_bits(got['F']), _bits(ref[1]))
        assert np.array_equal(got['n'], ref[2]) and np.array_equal(got['n'] - st['n'], np.isin(np.arange(C), want).astype(np.int32))
        if slots:
            assert np.array_equal(_bits(got['slot']), _bits(ref[3])) and np.array_equal(_bits(got['slot_F']), _bits(ref[4]))
            untouched = ~np.isin(np.arange(C), np.concatenate([want, want + 1]))
            assert np.all(got['slot'][untouched] == 7.0) and np.all(got['slot_F'][untouched] == 7.0)
        assert np.array_equal(_bits(got['log_u']), _bits(st['log_u'])) and np.array_equal(got['T'], st['T'])
        if len(want) == 0:
            assert np.array_equal(_bits(got['curr']), _bits(st['curr'])) and np.array_equal(_bits(got['F']), _bits(st['F']))
        n_taken += len(want)
    pairs = len(po.lower_chains(C, K, parity))
    assert (n_taken > 0) == (pairs > 0)
    assert pairs == {(8, 4, 5): (4, 2), (66, 3, 70): (22, 22), (6, 2, 1): (3, 0), (5, 5, 3): (2, 2)}[(C, K, q)][parity]


def test_pt_swap_refuses_bad_arguments():
    from sysbio_modeling_amd import _lib
    rng = np.random.default_rng(3)
    st, _ = _swap_state(rng, 8, 4, 5, 0, 0, True)
    lib = _lib.default_context().lib
    for K, parity, null, word in ((3, 0, None, b'ladders'), (1, 0, None, b'ladders'), (4, 2, None, b'parity'), (4, -1, None, b'parity'),
                                  (4, 0, 'T', b'NULL'), (4, 0, 'log_u', b'NULL'), (4, 0, 'curr', b'NULL'), (4, 0, 'F', b'NULL'),
                                  (4, 0, 'n', b'NULL')):
        rc, got = _swap(st, K, parity, True, True, null=null)
        assert rc == -1 and word in lib.sbm_last_error(), (K, parity, null)
        assert np.array_equal(_bits(got['curr']), _bits(st['curr'])) and np.array_equal(got['n'], st['n'])


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
LADDER = np.array([1.0, 1.5, 2.25])       # inside the temperatures the entropy bound was measured on (1 ... 2.5)


@pytest.fixture(scope='module')
def sf_project(gpu_models):
    """(project, truth, J^T J): the scale-factor project of tests/test_gpu_sampler_device.py"""
    proj, truth = _gaussian_posterior_project(gpu_models, True)
    J = proj.calc_project_jacobian(truth)
    return proj, truth, J.T @ J


def _energies(proj, energy, T, **overrides):
    """energies(theta) -> (K, C) for the oracle's replay: row k is ``free_energy_batch(theta, T_k, device=True)`` -- the scalar
    entropy entry, one call per temperature on the whole batch --, or, for 'rss', 0.5 |r|^2 in every row"""
    def rss(th):
        res = proj.evaluate_batch(th, want=('norms', 'status'), **overrides)
        out = 0.5 * res['norms']
        return np.broadcast_to(np.where(np.isfinite(out) & (res['status'] == 0), out, np.inf), (len(T), len(th)))

    def free(th):
        return np.stack([proj.free_energy_batch(th, float(Tk), device=True, **overrides) for Tk in T])
    return free if energy == 'free_energy' else rss


def _samp(hess, T, C, held=None):
    from sysbio_modeling_amd.project.ensembles import sampling_matrix
    return np.stack([sampling_matrix(hess, 1e-4, T[c % len(T)], 1.0, held=None if held is None else held[c]) for c in range(C)])


_replays = {}


def _replay(proj, truth, hess, C, energy):
    """The replay of the (C, energy) case, every step recorded -- made once, shared by the skip_elems cases and left as it is"""
    if (C, energy) not in _replays:
        steps = 30
        rng = np.random.default_rng(100 + C)
        starts = truth[None, :] + 0.01 * rng.standard_normal((C, 2))
        draws = (rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C))), np.log(rng.random((steps // 3, C))))
        ref = po.replay(_energies(proj, energy, LADDER), starts, _samp(hess, LADDER, C), LADDER, *draws, swap_every=3)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _replays[(C, energy)] = starts, draws, ref
    return _replays[(C, energy)]


def _compare(out, ref, steps, every=1):
    """acceptance and swap counts equal, positions to 1e-12, energies to 1e-12 max(1, |F|) -- the bounds of the scalar
    sampler's replay test without its quadrature term: both sides take the entropy from the same kernel body"""
    ens, ens_F, ratio, info = out
    assert ens.shape == ref['ens'][::every].shape and ens_F.shape == ref['ens_F'][::every].shape
    assert np.array_equal(ratio, ref['n_accepted'] / steps)
    assert np.array_equal(info['swap_accepted'], ref['n_swapped'])
    assert np.max(np.abs(ens - ref['ens'][::every])) <= 1e-12
    assert np.all(np.abs(ens_F - ref['ens_F'][::every]) <= 1e-12 * np.maximum(1.0, np.abs(ref['ens_F'][::every])))


@pytest.mark.parametrize('energy', ['rss', 'free_energy'])
@pytest.mark.parametrize('skip_elems', [0, 2])
@pytest.mark.parametrize('C', [6, 66])
def test_tempered_device_sampler_walks_the_replay(sf_project, C, skip_elems, energy):
    """T = (1, 1.5, 2.25), 30 steps, swaps every 3, with the three arrays of draws: the same move and swap decisions as the
    replay, whose energies come from free_energy_batch(theta, T_k, device=True) per temperature.  On the replay alone, first:
    no move and no swap decision is closer than 1e-6 to its bound, and moves and swaps both happen."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    proj, truth, hess = sf_project
    steps = 30
    starts, draws, ref = _replay(proj, truth, hess, C, energy)
    print("C=%d %s: move margin %.3e, swap margin %.3e, accepted %d of %d, swapped %d of %d"
          % (C, energy, ref['move_margin'], ref['swap_margin'], ref['n_accepted'].sum(), steps * C, ref['n_swapped'].sum(),
             10 * C // 3))
    assert ref['move_margin'] > 1e-6 and ref['swap_margin'] > 1e-6
    assert 0.05 < ref['n_accepted'].mean() / steps < 0.95 and ref['n_swapped'].sum() > 0
    out = ensemble_log_params_batch(proj, starts, hess=hess, steps=steps, temperature=LADDER, swap_every=3, sing_val_cutoff=1e-4,
                                    skip_elems=skip_elems, energy=energy, sampler='device', draws=draws)
    assert len(out) == 4 and np.array_equal(out[3]['temperature'], np.tile(LADDER, C // 3))
    assert np.array_equal(out[3]['swap_attempted'], np.tile([5, 5, 0], C // 3))
    _compare(out, ref, steps, skip_elems + 1)


def test_tempered_device_sampler_with_a_host_control_loop_integrator(sf_project):
    """method='auto': the integration goes through evaluate_batch, at the swap steps too (C = 4, K = 2, 6 steps, swaps every 2)"""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    proj, truth, hess = sf_project
    T, C, steps = np.array([1.0, 2.0]), 4, 6
    rng = np.random.default_rng(32)
    starts = truth[None, :] + 0.01 * rng.standard_normal((C, 2))
    draws = (rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C))), np.log(rng.random((3, C))))
    ref = po.replay(_energies(proj, 'free_energy', T, method='auto'), starts, _samp(hess, T, C), T, *draws, swap_every=2)
    assert ref['move_margin'] > 1e-6 and ref['swap_margin'] > 1e-6
    out = ensemble_log_params_batch(proj, starts, hess=hess, steps=steps, temperature=T, swap_every=2, sing_val_cutoff=1e-4,
                                    energy='free_energy', sampler='device', draws=draws, method='auto')
    _compare(out, ref, steps)


def test_tempered_device_sampler_with_a_shared_held_column_and_box(sf_project):
    """One parameter held at a value per ladder and one box for all chains: the proposal is sbm_mh_propose_box, its veto goes
    to sbm_mh_accept_pt, and a swap carries the held value to a chain that holds the same one."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    proj, truth, hess = sf_project
    C, steps = 6, 30
    rng = np.random.default_rng(33)
    sd0 = 1.0 / np.sqrt(hess[0, 0])                                                 # the free parameter's conditional width
    starts = np.empty((C, 2))
    starts[:, 0] = truth[0] + sd0 * rng.uniform(-1.0, 1.0, C)
    starts[:, 1] = np.repeat(truth[1] + np.array([0.002, -0.003]), 3)             # the held column: one value per ladder
    held = np.zeros((C, 2), dtype=bool)
    held[:, 1] = True
    lower, upper = np.tile(truth - [1.5 * sd0, 1.0], (C, 1)), np.tile(truth + [1.5 * sd0, 1.0], (C, 1))
    draws = (rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C))), np.log(rng.random((steps // 3, C))))
    ref = po.replay(_energies(proj, 'free_energy', LADDER), starts, _samp(hess, LADDER, C, held), LADDER, *draws, swap_every=3,
                    held=held, lower=lower, upper=upper)
    assert ref['move_margin'] > 1e-6 and ref['swap_margin'] > 1e-6
    out = ensemble_log_params_batch(proj, starts, hess=hess, steps=steps, temperature=LADDER, swap_every=3, sing_val_cutoff=1e-4,
                                    energy='free_energy', sampler='device', draws=draws, held=held, bounds=(lower, upper))
    _compare(out, ref, steps)
    assert np.array_equal(out[0][:, :, 1], np.broadcast_to(starts[:, 1], (steps + 1, C)))
    assert np.all(out[0] >= lower) and np.all(out[0] <= upper)


@pytest.mark.parametrize('energy', ['rss', 'free_energy'])
def test_a_flat_ladder_without_swaps_is_the_scalar_run(sf_project, energy):
    """temperature=[1.5, 1.5, 1.5] with the same draws: the record of temperature=1.5, to the bit -- the _pt entries and one
    candidate matrix per chain change nothing where the temperatures are equal"""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    proj, truth, hess = sf_project
    C, steps = 6, 20
    rng = np.random.default_rng(34)
    starts = truth[None, :] + 0.01 * rng.standard_normal((C, 2))
    draws = (rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C))))
    kw = dict(hess=hess, steps=steps, sing_val_cutoff=1e-4, energy=energy, sampler='device', draws=draws)
    scalar = ensemble_log_params_batch(proj, starts, temperature=1.5, **kw)
    flat = ensemble_log_params_batch(proj, starts, temperature=[1.5, 1.5, 1.5], **kw)
    assert len(scalar) == 3 and len(flat) == 4
    assert all(np.array_equal(a, b) for a, b in zip(scalar, flat[:3])) and 0 < scalar[2].mean() < 1
    assert not flat[3]['swap_attempted'].any() and not flat[3]['swap_accepted'].any()


def test_energies_with_one_temperature_per_vector(sf_project):
    """free_energy_batch and scale_factors_entropy_batch with a (V,) temperature: vector v as from the scalar call at T[v] --
    to the bit on the device, and the host path loops over the temperatures"""
    import warnings
    proj, truth, hess = sf_project
    th = truth[None, :] + 0.02 * np.random.default_rng(2).standard_normal((5, 2))
    T = np.array([1.0, 1.5, 2.25, 1.5, 2.5])
    got = proj.free_energy_batch(th, T, device=True)
    sims = proj.evaluate_batch(th, want=('sims',))['sims']
    ent = proj.scale_factors_entropy_batch(sims, T)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        host = proj.free_energy_batch(th, T)
        for v in range(5):
            assert got[v] == proj.free_energy_batch(th, T[v], device=True)[v]
            assert ent[v] == proj.scale_factors_entropy_batch(sims, T[v])[v]
            assert host[v] == proj.free_energy_batch(th, T[v])[v]
    with pytest.raises(ValueError):
        proj.scale_factors_entropy_batch(sims, T[:3])


def test_tempered_device_sampler_samples_every_rung(gpu_models):
    """The Gaussian-posterior project (1 % error bars, 'rss') with temperature_ladder(4, 4.0), 32 ladders, 400 steps, swaps
    every 2, random numbers drawn on the device: per rung, pooled over ens[100:, k::4], standard deviations within rtol 0.15
    of sqrt(T_k) sd and means within 0.2 sqrt(T_k) sd, sd from (J^T J)^-1 at the truth -- the bounds of the CPU test
    (tests/test_tempering_cpu.py says where they come from).  The test prints the deviations of its run.  The diagnostics of
    a tempered run are those of its 32 rung-0 chains."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch, temperature_ladder
    proj, truth = _gaussian_posterior_project(gpu_models, False)
    J = proj.calc_project_jacobian(truth)
    sd = np.sqrt(np.diag(np.linalg.inv(J.T @ J)))
    T = temperature_ladder(4, 4.0)
    ens, ens_F, ratio, diag, info = ensemble_log_params_batch(proj, np.tile(truth, (128, 1)), steps=400, temperature=T, swap_every=2,
                                                              seeds=11, sampler='device', energy='rss', diagnostics=True)
    assert ens.shape == (401, 128, 2) and ens_F.shape == (401, 128) and ratio.shape == (128,)
    assert 0.3 < ratio.mean() < 0.75
    for k in range(4):
        pooled = ens[100:, k::4].reshape(-1, 2)
        print("rung %d (T = %.3f): sd off by %.3f (rtol 0.15), mean off by %.3f sd (0.2)"
              % (k, T[k], np.max(np.abs(pooled.std(axis=0) / (np.sqrt(T[k]) * sd) - 1.0)),
                 np.max(np.abs(pooled.mean(axis=0) - truth) / (np.sqrt(T[k]) * sd))))
    for k in range(4):
        pooled = ens[100:, k::4].reshape(-1, 2)
        assert np.allclose(pooled.std(axis=0), np.sqrt(T[k]) * sd, rtol=0.15)
        assert np.all(np.abs(pooled.mean(axis=0) - truth) < 0.2 * np.sqrt(T[k]) * sd)
    pairs = info['rung'] < 3
    assert np.all(info['swap_attempted'][pairs] == 100) and np.all(info['swap_accepted'][pairs] > 0)
    assert not info['swap_attempted'][~pairs].any() and not info['swap_accepted'][~pairs].any()
    assert diag['tau'].shape == (32, 2) and diag['ess'].shape == (2,)
    # the same seed gives the same run; the move streams are those of the run without swaps (its first step is the same)
    kw = dict(steps=4, temperature=T, seeds=5, sampler='device', energy='rss')
    a, b = (ensemble_log_params_batch(proj, np.tile(truth, (8, 1)), swap_every=2, **kw) for _ in range(2))
    c = ensemble_log_params_batch(proj, np.tile(truth, (8, 1)), **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3]['swap_accepted'], b[3]['swap_accepted'])
    assert np.array_equal(a[0][:2], c[0][:2])
