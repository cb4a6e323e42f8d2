"""``sbm_chain_autocorr`` / ``sbm_chain_summary`` through the C ABI with device pointers, and their Python surface
(``autocorrelation``, ``ensemble_diagnostics``, ``ensemble_log_params_batch(diagnostics=True)``).

Oracle: tests/support/chain_diagnostics_oracle.py (``np.longdouble``; tests/test_chain_diagnostics_cpu.py holds it to the
reference's FFT formula).  Bounds, u = 2^-53:
  autocorrelation   tol_k = 8 N u [(sum_i |d_i d_{i+k}| / (N - k) + max|d|^2) / c_0 + |ac_k|] at every lag
  moments           64 n u relative, n = N // 2
  tau               4 K u sum|ac| against the window rule on the kernel's own ac; 2 sum_{k < 2M} tol_k against the oracle's tau
  r_hat, ess        64 N u relative
Figures of the runs this file was written with (MI355X): docs/history.md, "Chain diagnostics"."""
import numpy as np
import pytest

from tests.support import chain_diagnostics_oracle as co

pytestmark = pytest.mark.gpu

U = co.U
SBM_E_ARG = -1


def _call(values, N, S, stride, K, want=('tau', 'moments', 'flags')):
    """(rc, dict of numpy outputs) of one sbm_chain_autocorr call on cuda:0 on the flat record ``values``; outputs not in
    ``want`` are passed as NULL.  Outputs are pre-filled with 7 (flags -1)."""
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    vd = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).cuda()
    out = {'ac': torch.full((S, K), 7.0, dtype=torch.float64, device='cuda')}
    if 'tau' in want:
        out['tau'] = torch.full((S,), 7.0, dtype=torch.float64, device='cuda')
    if 'moments' in want:
        out['moments'] = torch.full((S, 4), 7.0, dtype=torch.float64, device='cuda')
    if 'flags' in want:
        out['flags'] = torch.full((S,), -1, dtype=torch.int32, device='cuda')
    p = _lib.dev_ptr
    rc = ctx.lib.sbm_chain_autocorr(ctx.handle, p(vd), N, S, stride, K, p(out['ac']), p(out.get('tau')), p(out.get('moments')),
                                    p(out.get('flags')))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _summary(moments, tau, N, C, q):
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    md, td = torch.from_numpy(np.ascontiguousarray(moments)).cuda(), torch.from_numpy(np.ascontiguousarray(tau)).cuda()
    rhat = torch.full((q,), 7.0, dtype=torch.float64, device='cuda')
    ess = torch.full((q,), 7.0, dtype=torch.float64, device='cuda')
    p = _lib.dev_ptr
    rc = ctx.lib.sbm_chain_summary(ctx.handle, p(md), p(td), N, C, q, p(rhat), p(ess))
    torch.cuda.synchronize()
    return rc, rhat.cpu().numpy(), ess.cpu().numpy()


_oracle_cache = {}


def _oracle(key, x, K):
    """(ac, tol) of series ``x`` with K lags, float64 and float64; computed once per key"""
    if key not in _oracle_cache:
        _oracle_cache[key] = (np.asarray(co.autocorrelation(x, K), dtype=np.float64), co.tolerance(x, K))
    return _oracle_cache[key]


def _check_ac(rec, res, K, what):
    """every series of the record (N, S) at every lag, and the flags of a record without constant series"""
    N, S = rec.shape
    worst = 0.0
    for s in range(S):
        ac, tol = _oracle((what, s), rec[:, s], K)
        ratio = np.abs(res['ac'][s] - ac) / tol
        assert np.all(np.isfinite(res['ac'][s])), (what, s)
        worst = max(worst, ratio.max())
        assert ratio.max() <= 1.0, (what, s, int(ratio.argmax()), ratio.max())
        assert res['ac'][s, 0] == 1.0
    print('%s: worst |ac - oracle| / tol = %.3g' % (what, worst))
    return worst


def _check_moments(rec, res, what):
    N, S = rec.shape
    n = N // 2
    for s in range(S):
        ref = co.half_moments(rec[:, s])
        got = res['moments'][s]
        for i in range(4):
            if np.isnan(ref[i]):
                assert np.isnan(got[i]), (what, s, i)
            else:
                assert abs(got[i] - ref[i]) <= 64 * n * U * abs(ref[i]), (what, s, i, got[i], float(ref[i]))


def _check_tau_own(res, K, what):
    """tau against the window rule applied to the kernel's own ac, and the truncated flag with it"""
    for s in range(res['ac'].shape[0]):
        tau, M, truncated = co.geyer(res['ac'][s].astype(co.LD))
        assert abs(res['tau'][s] - tau) <= 4 * K * U * np.abs(res['ac'][s]).sum(), (what, s, res['tau'][s], float(tau))
        assert res['flags'][s] == (co.FLAG_TRUNCATED if truncated else 0), (what, s)


@pytest.mark.parametrize('S', [1, 5, 33])
@pytest.mark.parametrize('N', [2, 3, 63, 64, 65, 1025])
def test_autocorrelation_all_lags(N, S):
    """K = N, the reference's semantics; S = 5 and 33 leave the last packed workgroup ragged (and S = 1 nearly empty)"""
    rec = co.random_record(N, S, seed=1000 * N + S)
    rc, res = _call(rec, N, S, S, N)
    assert rc == 0
    _check_ac(rec, res, N, 'N=%d S=%d' % (N, S))
    _check_moments(rec, res, 'N=%d S=%d' % (N, S))
    _check_tau_own(res, N, 'N=%d S=%d' % (N, S))


@pytest.mark.parametrize('K', [1, 2, 64])
def test_autocorrelation_few_lags(K):
    """K = 1, 2 and N - 1 at N = 65: the i range split over the lanes of a lag block, and nearly all lags"""
    N, S = 65, 5
    rec = co.random_record(N, S, seed=77)
    rc, res = _call(rec, N, S, S, K)
    assert rc == 0
    _check_ac(rec, res, K, 'N=65 K=%d' % K)
    _check_tau_own(res, K, 'N=65 K=%d' % K)
    if K == 1:
        assert np.all(res['tau'] == -1.0) and np.all(res['flags'] == co.FLAG_TRUNCATED)      # no complete pair


def test_step_stride_skips_steps():
    """step_stride = 3 S: every third step of the record is used; the others hold NaN"""
    N, S = 65, 5
    rec = co.random_record(N, S, seed=78)
    full = np.full((3 * N, S), np.nan)
    full[::3] = rec
    rc, res = _call(full, N, S, 3 * S, N)
    assert rc == 0
    _check_ac(rec, res, N, 'stride')
    _check_moments(rec, res, 'stride')
    dense = _call(rec, N, S, S, N)[1]
    for k in res:
        assert np.array_equal(res[k], dense[k], equal_nan=True), k


def test_full_lds_budget_and_the_limit():
    """N = SBM_CHAIN_MAX_STEPS keeps a series in 128 KiB of LDS; one more step is refused with an error"""
    from sysbio_modeling_amd import _lib
    N, S, K = _lib.CHAIN_MAX_STEPS, 2, 64
    assert N == 16384
    rec = co.random_record(N, S, seed=79)
    rc, res = _call(rec, N, S, S, K)
    assert rc == 0
    _check_ac(rec, res, K, 'N=16384')
    _check_moments(rec, res, 'N=16384')
    _check_tau_own(res, K, 'N=16384')
    rc, res = _call(np.zeros(8), N + 1, 1, 1, 4)
    assert rc == SBM_E_ARG
    msg = _lib.load_library().sbm_last_error().decode()
    assert '16385' in msg and 'SBM_CHAIN_MAX_STEPS' in msg
    assert np.all(res['ac'] == 7.0)


def test_argument_checks():
    from sysbio_modeling_amd import _lib
    import torch
    ctx = _lib.default_context()
    lib, p = ctx.lib, _lib.dev_ptr
    v = torch.zeros(64, dtype=torch.float64, device='cuda')
    ac = torch.zeros(64, dtype=torch.float64, device='cuda')
    err = lambda: lib.sbm_last_error().decode()
    assert lib.sbm_chain_autocorr(ctx.handle, p(v), 1, 1, 1, 1, p(ac), None, None, None) == SBM_E_ARG and 'N >= 2' in err()
    assert lib.sbm_chain_autocorr(ctx.handle, p(v), 8, 1, 1, 0, p(ac), None, None, None) == SBM_E_ARG and 'K' in err()
    assert lib.sbm_chain_autocorr(ctx.handle, p(v), 8, 1, 1, 9, p(ac), None, None, None) == SBM_E_ARG and 'K' in err()
    assert lib.sbm_chain_autocorr(ctx.handle, p(v), 8, 4, 3, 2, p(ac), None, None, None) == SBM_E_ARG and 'step_stride' in err()
    assert lib.sbm_chain_autocorr(ctx.handle, None, 8, 1, 1, 2, p(ac), None, None, None) == SBM_E_ARG and 'NULL' in err()
    assert lib.sbm_chain_autocorr(ctx.handle, p(v), 8, 1, 1, 2, None, None, None, None) == SBM_E_ARG and 'NULL' in err()
    assert lib.sbm_chain_autocorr(None, p(v), 8, 1, 1, 2, p(ac), None, None, None) == SBM_E_ARG and 'NULL' in err()
    assert lib.sbm_chain_autocorr(ctx.handle, None, 8, 0, 0, 2, None, None, None, None) == 0       # S == 0: nothing to do
    assert lib.sbm_chain_summary(ctx.handle, p(v), p(v), 8, 0, 1, p(ac), p(ac)) == SBM_E_ARG and 'C=0' in err()
    assert lib.sbm_chain_summary(ctx.handle, p(v), p(v), 8, 1, 0, p(ac), p(ac)) == SBM_E_ARG and 'q=0' in err()
    assert lib.sbm_chain_summary(ctx.handle, p(v), None, 8, 1, 1, p(ac), p(ac)) == SBM_E_ARG and 'NULL' in err()
    assert lib.sbm_chain_summary(ctx.handle, p(v), p(v), 1, 1, 1, p(ac), p(ac)) == SBM_E_ARG
    torch.cuda.synchronize()


def test_offset_series():
    """x + 1e6 with unit spread: the shifted two-pass mean keeps the deviations; the bound is the offset series' own"""
    N, S = 1025, 3
    rec = co.random_record(N, S, seed=80, offset=1e6)
    rc, res = _call(rec, N, S, S, N)
    assert rc == 0
    _check_ac(rec, res, N, 'offset 1e6')
    _check_moments(rec, res, 'offset 1e6')


@pytest.mark.parametrize('N', [65, 1025])
def test_constant_series(N):
    """N copies of 0.1 (whose computed mean need not be 0.1) among varying series: flagged, NaN in ac and tau, mean 0.1 and
    variance 0; the neighbours in the same workgroup are what they are without it"""
    S, K = 5, 32
    rec = co.random_record(N, S, seed=81)
    rec[:, 2] = 0.1
    rc, res = _call(rec, N, S, S, K)
    assert rc == 0
    assert res['flags'][2] == co.FLAG_CONSTANT and np.all(np.isnan(res['ac'][2])) and np.isnan(res['tau'][2])
    assert np.array_equal(res['moments'][2], [0.1, 0.0, 0.1, 0.0])
    others = [0, 1, 3, 4]
    alone = _call(rec[:, others], N, 4, 4, K)[1]
    for k in res:
        assert np.array_equal(res[k][others], alone[k]), k
    _check_ac(rec[:, others], alone, K, 'beside a constant series N=%d' % N)
    assert not np.any(alone['flags'] & co.FLAG_CONSTANT)


@pytest.mark.parametrize('phi', sorted(co.AR1_SEEDS))
def test_tau_against_the_oracle(phi):
    x = co.ar1_case(phi)
    N, K = co.AR1_N, co.AR1_K
    rc, res = _call(x, N, 1, 1, K)
    assert rc == 0
    ac, tol = _oracle(('ar1', phi), x, K)
    assert np.all(np.abs(res['ac'][0] - ac) <= tol)
    _check_tau_own(res, K, 'ar1 %g' % phi)
    tau, M, truncated = co.geyer(co.autocorrelation(x, K))
    bound = 2.0 * tol[:2 * M].sum()
    print('phi = %g: tau %.6f, oracle %.6f, |diff| = %.3g, bound %.3g, M = %d' % (phi, res['tau'][0], float(tau),
                                                                                abs(res['tau'][0] - float(tau)), bound, M))
    assert abs(res['tau'][0] - float(tau)) <= bound
    assert not truncated and res['flags'][0] == 0


def test_truncated_window():
    """K = 4 at phi = 0.9 cuts the window: the sum over both pairs, and the flag"""
    x = co.ar1_case(0.9)
    rc, res = _call(x, co.AR1_N, 1, 1, 4)
    assert rc == 0
    ac, tol = _oracle(('ar1 K=4', 0.9), x, 4)
    tau, M, truncated = co.geyer(co.autocorrelation(x, 4))
    assert truncated and M == 2
    assert res['flags'][0] == co.FLAG_TRUNCATED
    assert abs(res['tau'][0] - float(tau)) <= 2.0 * tol.sum()


def _summary_case(shift):
    """(N, C = 4, q = 3) AR(1) chains around 3; ``shift`` moves chain 1 of every parameter by that many standard deviations"""
    N, C, q = 1000, 4, 3
    ens = co.random_record(N, C * q, seed=90).reshape(N, C, q)
    ens[:, 1, :] += shift * ens[:, 1, :].std(axis=0)
    return ens


@pytest.mark.parametrize('shift', [0.0, 5.0])
def test_summary(shift):
    ens = _summary_case(shift)
    N, C, q = ens.shape
    K = 256
    rc, res = _call(ens, N, C * q, C * q, K)
    assert rc == 0
    rc, rhat, ess = _summary(res['moments'], res['tau'], N, C, q)
    assert rc == 0
    ref_rhat, ref_ess, ref_tau = co.summary(ens, K)
    print('shift %g: r_hat %s (oracle %s), ess %s (oracle %s)' % (shift, rhat, np.asarray(ref_rhat, dtype=float), ess,
                                                                  np.asarray(ref_ess, dtype=float)))
    if shift:
        assert np.all(ref_rhat > 1.5)
    else:
        assert np.all(ref_rhat < 1.1)
    assert np.all(np.abs(rhat - ref_rhat) <= 64 * N * U * np.abs(ref_rhat))
    assert np.all(np.abs(ess - ref_ess) <= 64 * N * U * np.abs(ref_ess))


def test_summary_nan_rules():
    """parameter 0 constant in every chain: r_hat and ess NaN; parameter 1 constant in chain 2 only: r_hat from all eight
    half-chains (two of variance 0), ess from the three chains that have a tau"""
    ens = _summary_case(0.0)
    N, C, q = ens.shape
    K = 256
    ens[:, :, 0] = 0.1
    ens[:, 2, 1] = ens[0, 2, 1]
    rc, res = _call(ens, N, C * q, C * q, K)
    assert rc == 0
    const = (res['flags'] & co.FLAG_CONSTANT).astype(bool).reshape(C, q)
    assert np.all(const[:, 0]) and const[2, 1] and const.sum() == C + 1
    rc, rhat, ess = _summary(res['moments'], res['tau'], N, C, q)
    assert rc == 0
    ref_rhat, ref_ess, _ = co.summary(ens, K)
    assert np.isnan(rhat[0]) and np.isnan(ess[0]) and np.isnan(ref_rhat[0]) and np.isnan(ref_ess[0])
    for j in (1, 2):
        assert abs(rhat[j] - ref_rhat[j]) <= 64 * N * U * abs(ref_rhat[j])
        assert abs(ess[j] - ref_ess[j]) <= 64 * N * U * abs(ref_ess[j])


def test_two_calls_give_the_same_bits():
    for N, S, K in ((1025, 3, 1025), (65, 33, 65), (4096, 2, 16)):
        rec = co.random_record(N, S, seed=91)
        a, b = _call(rec, N, S, S, K)[1], _call(rec, N, S, S, K)[1]
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (N, k)


# ---------------------------------------------------------------------------------------------
# Python surface
# ---------------------------------------------------------------------------------------------
def test_autocorrelation_function():
    import torch
    from sysbio_modeling_amd.project import autocorrelation
    x = co.random_record(200, 6, seed=92)
    one = autocorrelation(x[:, 0])
    assert isinstance(one, np.ndarray) and one.shape == (200,)
    ac, tol = _oracle(('py', 0), x[:, 0], 200)
    assert np.all(np.abs(one - ac) <= tol)
    cube = autocorrelation(x.reshape(200, 2, 3), max_lag=17)
    assert isinstance(cube, np.ndarray) and cube.shape == (17, 2, 3)
    for c in range(2):
        for j in range(3):
            a, t = _oracle(('py', 3 * c + j), x[:, 3 * c + j], 200)
            assert np.all(np.abs(cube[:, c, j] - a[:17]) <= t[:17])
    xt = torch.from_numpy(x).cuda()
    dev1 = autocorrelation(xt[:, 0])
    dev3 = autocorrelation(xt.reshape(200, 2, 3), max_lag=17)
    assert isinstance(dev1, torch.Tensor) and dev1.is_cuda and tuple(dev1.shape) == (200,)
    assert isinstance(dev3, torch.Tensor) and dev3.is_cuda and tuple(dev3.shape) == (17, 2, 3)
    assert np.array_equal(dev1.cpu().numpy(), one) and np.array_equal(dev3.cpu().numpy(), cube)
    with pytest.raises(ValueError, match='max_lag'):
        autocorrelation(x[:, 0], max_lag=201)


def test_ensemble_diagnostics_function():
    import torch
    from sysbio_modeling_amd.project import ensemble_diagnostics
    N, C, q = 301, 4, 3
    ens = co.random_record(N, C * q, seed=93).reshape(N, C, q)
    ens[:, :, 2] = ens[0, :, 2]                          # a held parameter
    F = co.random_record(N, C, seed=94)
    d = ensemble_diagnostics(ens, F)
    K = 300
    shapes = {'autocorrelation': (K, C, q), 'tau': (C, q), 'ess_chain': (C, q), 'ess': (q,), 'r_hat': (q,), 'constant': (C, q),
              'truncated': (C, q), 'autocorrelation_F': (K, C), 'tau_F': (C,), 'ess_F': (), 'r_hat_F': ()}
    assert set(d) == set(shapes)
    for k, sh in shapes.items():
        assert isinstance(d[k], np.ndarray) and d[k].shape == sh, k
    assert d['constant'].dtype == np.bool_ and d['truncated'].dtype == np.bool_
    assert np.all(d['constant'][:, 2]) and not np.any(d['constant'][:, :2]) and np.all(np.isnan(d['tau'][:, 2]))
    assert np.isnan(d['ess'][2]) and np.isnan(d['r_hat'][2]) and np.all(np.isfinite(d['ess'][:2]))
    # N / tau by torch on the device, which may divide by multiplying with a rounded reciprocal: two roundings
    ok = ~np.isnan(d['tau'])
    assert np.array_equal(np.isnan(d['ess_chain']), ~ok)
    assert np.all(np.abs(d['ess_chain'][ok] - N / d['tau'][ok]) <= 4 * U * np.abs(N / d['tau'][ok]))
    ref_rhat, ref_ess, ref_tau = co.summary(ens[:, :, :2], K)
    assert np.all(np.abs(d['r_hat'][:2] - ref_rhat) <= 64 * N * U * np.abs(ref_rhat))
    assert np.all(np.abs(d['ess'][:2] - ref_ess) <= 64 * N * U * np.abs(ref_ess))
    rF, eF, _ = co.summary(F[:, :, None], K)
    assert abs(d['r_hat_F'] - rF[0]) <= 64 * N * U * abs(rF[0]) and abs(d['ess_F'] - eF[0]) <= 64 * N * U * abs(eF[0])
    # thin = 2 is the diagnostics of every second step, without a copy
    thin = ensemble_diagnostics(ens, F, thin=2)
    copy = ensemble_diagnostics(ens[::2].copy(), F[::2].copy())
    assert thin['autocorrelation'].shape == (150, C, q)
    for k in thin:
        assert np.array_equal(thin[k], copy[k], equal_nan=True), k
    # device tensors in, device tensors out
    dev = ensemble_diagnostics(torch.from_numpy(ens).cuda(), torch.from_numpy(F).cuda(), max_lag=40)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values())
    assert tuple(dev['autocorrelation'].shape) == (40, C, q)
    host = ensemble_diagnostics(ens, F, max_lag=40)
    for k in host:
        assert np.array_equal(dev[k].cpu().numpy(), host[k], equal_nan=True), k
    # too many steps: the message says what to do
    long = np.zeros((16386, 1, 1))
    with pytest.raises(ValueError, match=r'thin=.*skip_elems'):
        ensemble_diagnostics(long)
    assert ensemble_diagnostics(long, thin=2)['tau'].shape == (1, 1)


def test_sampler_returns_the_diagnostics_of_its_record(gpu_models):
    from sysbio_modeling_amd.project.ensembles import ensemble_diagnostics, ensemble_log_params_batch
    from tests.test_gpu_sampler_device import _gaussian_posterior_project
    proj, truth = _gaussian_posterior_project(gpu_models, False)
    starts = np.tile(truth, (4, 1)) + 0.01 * np.arange(4)[:, None]
    kw = dict(steps=40, seeds=7, sampler='device', held=[1])
    ens, ens_F, ratio, diag = ensemble_log_params_batch(proj, starts, diagnostics=True, **kw)
    plain = ensemble_log_params_batch(proj, starts, **kw)
    assert len(plain) == 3
    for a, b in zip((ens, ens_F, ratio), plain):
        assert np.array_equal(a, b)
    again = ensemble_diagnostics(ens, ens_F)
    assert set(diag) == set(again)
    for k in diag:
        assert isinstance(diag[k], np.ndarray) and np.array_equal(diag[k], again[k], equal_nan=True), k
    assert diag['autocorrelation'].shape == (40, 4, 2)
    assert np.all(diag['constant'][:, 1]) and np.all(ens[:, :, 1] == starts[None, :, 1])
    assert not np.any(diag['constant'][:, 0])
    # without held parameters, and the host sampler on its uploaded record
    out = ensemble_log_params_batch(proj, starts, steps=12, seeds=7, sampler='host', diagnostics=True)
    assert len(out) == 4
    again = ensemble_diagnostics(out[0], out[1])
    for k in again:
        assert np.array_equal(out[3][k], again[k], equal_nan=True), k
    with pytest.raises(ValueError, match='skip_elems'):
        ensemble_log_params_batch(proj, starts, steps=20000, sampler='device', diagnostics=True)
