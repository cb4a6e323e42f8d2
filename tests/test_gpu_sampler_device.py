"""The Metropolis sampler's step on the device: ``sbm_project_sf_entropy`` against mpmath, ``sbm_mh_propose`` /
``sbm_mh_accept`` and ``ensemble_log_params_batch(sampler='device')`` against a host replay with the same draws, and the
statistics of the chains."""
import ctypes
import warnings

import numpy as np
import pytest

from tests import sf_entropy_cases as sfc

pytestmark = pytest.mark.gpu

# The device rule's own floor in the logarithm (tests/test_sf_quadrature_cpu.py derives it from the rule's construction).
RULE_TOL = 1e-10


# ---------------------------------------------------------------------------
# synthetic projects through sbm_project_load: only the row tables matter to the entropy kernel
# ---------------------------------------------------------------------------
class _Synthetic(object):
    """Rows of ``sizes[k]`` measurements per scale-factor group k plus ``n_plain`` rows without one, shuffled; group k
    has D_k = sum d^2 / sigma^2 = ``D[k]`` and the log prior (mu[k], prior_sigma[k]); loaded on the 'simple' model."""

    def __init__(self, model, sizes, n_plain, D, mu, prior_sigma, seed, with_priors=None):
        from sysbio_modeling_amd import _lib
        rng = np.random.default_rng(seed)
        G = len(sizes)
        sf = np.concatenate([np.full(n, k) for k, n in enumerate(sizes)] + [np.full(n_plain, -1)]).astype(np.int32)
        rng.shuffle(sf)
        R = len(sf)
        data = rng.uniform(1.0, 2.0, R)
        sigma = rng.uniform(0.05, 0.2, R)
        for k in range(G):
            sel = sf == k
            sigma[sel] *= np.sqrt(np.sum(data[sel] ** 2 / sigma[sel] ** 2) / D[k])
        self.G, self.R, self.sf, self.data, self.sigma = G, R, sf, data, sigma
        self.mu, self.prior_sigma = np.asarray(mu, dtype=float), np.asarray(prior_sigma, dtype=float)
        groups = list(range(G)) if with_priors is None else list(with_priors)
        nv, npar = model.n_vars, len(model.param_order)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        a = dict(pmap=i32(np.arange(npar)[None, :]), pfixed=f64(np.zeros((1, npar))), sens_col=i32(np.arange(npar)),
                 tgrid_off=i32([0, 2]), tgrid=f64([0.0, 1.0]), row_exp=i32(np.zeros(R)), row_tidx=i32(np.ones(R)),
                 row_var_off=i32(np.arange(R + 1)), row_vars=i32(np.zeros(R)), row_data=f64(data), row_sigma=f64(sigma),
                 row_sf=i32(sf), sfg=i32(groups), sfm=f64(self.mu[groups]), sfs=f64(self.prior_sigma[groups]))
        self._keep = a
        ip = lambda x: x.ctypes.data_as(_lib.c_int32_p) if x.size else ctypes.cast(None, _lib.c_int32_p)
        dp = lambda x: x.ctypes.data_as(_lib.c_double_p) if x.size else ctypes.cast(None, _lib.c_double_p)
        nil_i, nil_d = ctypes.cast(None, _lib.c_int32_p), ctypes.cast(None, _lib.c_double_p)
        assert nv >= 1
        desc = _lib.ProjectDesc(1, npar, R, G, 0, len(groups), ip(a['pmap']), dp(a['pfixed']), ip(a['sens_col']),
                                ip(a['tgrid_off']), dp(a['tgrid']), ip(a['row_exp']), ip(a['row_tidx']),
                                ip(a['row_var_off']), ip(a['row_vars']), dp(a['row_data']), dp(a['row_sigma']),
                                ip(a['row_sf']), nil_i, nil_d, nil_d, ip(a['sfg']), dp(a['sfm']), dp(a['sfs']), 0, 0,
                                0, 0, 0, nil_i, nil_i, nil_i, nil_i, nil_d, nil_d)
        self.lib = _lib.load_library()
        h = ctypes.c_void_p()
        _lib.check(self.lib.sbm_project_load(model.device_model.handle, ctypes.byref(desc), ctypes.byref(h)), 'sbm_project_load')
        self.handle = h

    def close(self):
        self.lib.sbm_project_unload(self.handle)

    def sims(self, rng, X, bstar):
        """(V, R) simulations with a B*^2 = X[v, k] and B* = bstar[v, k]; the rows without a scale factor random."""
        V = X.shape[0]
        out = rng.uniform(0.5, 3.0, (V, self.R))
        for v in range(V):
            for k in range(self.G):
                sel = self.sf == k
                out[v, sel] = sfc.group_sims(rng, self.data[sel], self.sigma[sel], X[v, k], bstar[v, k])
        return out

    def entropy(self, sims, T):
        """(rc, entropy (V,), group_entropy (V, G)) of sbm_project_sf_entropy"""
        import torch
        from sysbio_modeling_amd import _lib
        sd = torch.from_numpy(np.ascontiguousarray(sims)).cuda()
        V = sd.shape[0]
        ent = torch.full((V,), 7.0, dtype=torch.float64, device='cuda')
        grp = torch.full((V, self.G), 7.0, dtype=torch.float64, device='cuda')
        rc = self.lib.sbm_project_sf_entropy(self.handle, _lib.dev_ptr(sd), V, float(T), _lib.dev_ptr(ent), _lib.dev_ptr(grp))
        torch.cuda.synchronize()
        return rc, ent.cpu().numpy(), grp.cpu().numpy()

    def host_group(self, sims_v, k, T):
        """the host path's value for one (vector, group): scale_factor_entropy on numpy's row sums"""
        from sysbio_modeling_amd.project.loss_functions.squared_loss.linear_scale_factor import scale_factor_entropy
        sel = self.sf == k
        w = 1.0 / self.sigma[sel] ** 2
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return scale_factor_entropy(np.sum(sims_v[sel] ** 2 * w), np.sum(sims_v[sel] * self.data[sel] * w),
                                        self.mu[k], self.prior_sigma[k], T)

    def mp_group(self, sims_v, k, T):
        sel = self.sf == k
        a, b = sfc.mp_row_sums(sims_v[sel], self.data[sel], self.sigma[sel])
        return sfc.mp_log_integral(a, b, self.mu[k], self.prior_sigma[k], T)


def _targets(rng, proj, V, cos2_range=(-2.0, 0.0)):
    """a B*^2 = D cos^2, cos^2 log-uniform (the angle between simulations and data: a B*^2 does not change when the
    simulations are scaled), and B* such that the prior's centre is up to 3 prior sigmas from log B*."""
    D = np.array([np.sum(proj.data[proj.sf == k] ** 2 / proj.sigma[proj.sf == k] ** 2) for k in range(proj.G)])
    X = D[None, :] * 10.0 ** rng.uniform(cos2_range[0], cos2_range[1], (V, proj.G))
    X = np.minimum(X, D[None, :])
    bstar = np.exp(proj.mu[None, :] - rng.uniform(-3.0, 3.0, (V, proj.G)) * proj.prior_sigma[None, :])
    return X, bstar


_measured = {}


def _entropy_errors(model):
    """Test 1's measurement, made once per session: the device's and the host's error against mpmath, and the largest
    device-host difference over every (vector, group, T) of the runs.

    Ranges.  Prior sigma 0.1 ... 3, prior centre up to 3 sigma from log B*, T = 1 and 2.5, groups of 1, 7 and 70 rows
    (the last over two wavefront passes of rows) among rows without a scale factor, V = 5 (G = 1) and V = 67 (G = 3).
    a B*^2 spans 1e-2 ... 1e6 in the host comparison, not 1e8: over 1e-2 ... 1e8, scipy's quad on (-inf, inf) misses the
    narrow likelihood peak in 36 of 400 trial cases and returns FINITE values that are wrong by 10 ... 100 in the
    logarithm (none of 400 up to 1e6; checked on the CPU with the host-compiled rule, which agrees with mpmath to
    2e-15).  1e6 ... 1e8 is covered against mpmath alone, with the rule's floor as the bound."""
    if _measured:
        return _measured
    rng = np.random.default_rng(2024)
    # D per group: with cos^2 in [1e-2, 1] the two G = 3 projects cover a B*^2 = 1e-2 ... 1e6
    lo = _Synthetic(model, (1, 7, 70), 9, D=(1.0e-2, 1.0, 1.0e2), mu=(0.3, -0.5, 1.0), prior_sigma=(0.1, 0.9, 3.0), seed=1)
    hi = _Synthetic(model, (1, 7, 70), 9, D=(1.0e3, 1.0e6, 1.0e4), mu=(-0.2, 0.4, 0.0), prior_sigma=(3.0, 0.1, 0.35), seed=2)
    one = _Synthetic(model, (7,), 3, D=(30.0,), mu=(0.1,), prior_sigma=(1.7,), seed=3)
    top = _Synthetic(model, (7,), 3, D=(1.0e8,), mu=(0.1,), prior_sigma=(0.6,), seed=4)     # 1e6 ... 1e8: mpmath only
    dev_err, host_err, dev_host, left_out, n_pairs, n_mp = 0.0, 0.0, 0.0, 0, 0, 0
    try:
        for proj, V, n_check in ((lo, 67, 3), (hi, 67, 3), (one, 5, 1)):
            X, bstar = _targets(rng, proj, V)
            sims = proj.sims(rng, X, bstar)
            for T in (1.0, 2.5):
                rc, ent, grp = proj.entropy(sims, T)
                assert rc == 0
                assert np.allclose(ent, T * grp.sum(axis=1), rtol=1e-14, atol=0)
                host = np.array([[proj.host_group(sims[v], k, T) for k in range(proj.G)] for v in range(V)])
                ok = np.isfinite(host)
                left_out += int((~ok).sum())
                n_pairs += ok.size
                # quad stops when its error estimate is below max(epsabs, epsrel |I|), both 1.49e-8: in the logarithm
                # that is 1.5e-8 max(1, 1 / I)
                tol = RULE_TOL + 1.5e-8 * np.maximum(1.0, np.exp(-grp))
                assert np.all(np.isfinite(grp))
                assert np.all(np.abs(grp - host)[ok] <= tol[ok]), np.max((np.abs(grp - host) / tol)[ok])
                dev_host = max(dev_host, float(np.max(np.abs(grp - host)[ok])))
                # mpmath on a spread of (vector, group) pairs that includes the last vector and every group, and on the
                # pairs where device and host disagree most: whose error that is, is the question
                pairs = [(int(v), int(k)) for v, k in zip(np.linspace(0, V - 1, n_check).round(), np.arange(n_check) % proj.G)]
                diff = np.where(ok, np.abs(grp - host), -1.0)
                pairs += [tuple(int(i) for i in np.unravel_index(j, diff.shape)) for j in np.argsort(diff, axis=None)[-3:]]
                pairs = sorted(set(pairs))[:n_check + 3]
                for v, k in pairs:
                    ref = proj.mp_group(sims[v], k, T)
                    n_mp += 1
                    dev_err = max(dev_err, abs(grp[v, k] - ref))
                    if ok[v, k]:
                        host_err = max(host_err, abs(host[v, k] - ref))
        # beyond the host's reach
        X, bstar = _targets(rng, top, 5)
        sims = top.sims(rng, X, bstar)
        rc, ent, grp = top.entropy(sims, 1.0)
        assert rc == 0
        top_err = max(abs(grp[v, 0] - top.mp_group(sims[v], 0, 1.0)) for v in (0, 4))
        n_mp += 2
    finally:
        for proj in (lo, hi, one, top):
            proj.close()
    _measured.update(dev_err=dev_err, host_err=host_err, dev_host=dev_host, left_out=left_out, n_pairs=n_pairs, n_mp=n_mp,
                     top_err=top_err, bound=max(host_err, RULE_TOL))
    print("sf entropy: device max |err| %.3e, host max |err| %.3e (mpmath, %d cases); device-host max %.3e over %d pairs, "
          "%d left out; a B*^2 1e6..1e8: device %.3e" % (dev_err, host_err, n_mp, dev_host, n_pairs, left_out, top_err))
    return _measured


def test_entropy_kernel_against_mpmath(gpu_models):
    """sbm_project_sf_entropy against mpmath.quad at 25 digits (34 cases with the special ones below, none stored), and
    against the host path it replaces: the device error must be at most the larger of the host path's error against the
    same mpmath values and 1e-10 absolute in the logarithm.

    Measured on an MI355X: device 3.1e-15, host (scipy quad) 9.2e-10 over 31 cases -- the pairs where the two disagree
    most are among them, and the disagreement is the host's; largest device-host difference 9.2e-10 over 814 (vector,
    group, T) pairs, none left out; a B*^2 1e6 ... 1e8: device 1.8e-15.  The test prints the figures of its run."""
    m = _entropy_errors(gpu_models('simple'))
    assert m['n_mp'] <= 34                     # (+ 3 in the two-bump test: 40 at most)
    assert m['left_out'] <= 0.02 * m['n_pairs']
    assert m['dev_err'] <= max(m['host_err'], RULE_TOL)
    assert m['top_err'] <= RULE_TOL


def test_entropy_kernel_two_bumps_and_underflow(gpu_models):
    """Two deliberate two-maxima cases (a B*^2 / T ~ 1, prior centre 3 sigma below log B*: one bump at u ~ 0, one at
    the prior's centre) and one whose integrand stays below exp(-745): the host returns -inf there, the device the
    logarithm.  All against mpmath."""
    model = gpu_models('simple')
    bound = _entropy_errors(model)['bound']
    proj = _Synthetic(model, (1, 7, 70), 9, D=(1.0e4, 50.0, 50.0), mu=(0.0, 0.2, -0.3), prior_sigma=(0.1, 0.9, 3.0), seed=5)
    try:
        rng = np.random.default_rng(8)
        T = 1.0
        X = np.array([[1.0e4, 1.0 * T, 1.2 * T]])
        # group 0: prior centre 40 prior sigmas below log B*: max of the integrand ~ exp(-800)
        bstar = np.exp(proj.mu[None, :] - np.array([[-40.0, -3.0, -3.0]]) * proj.prior_sigma[None, :])
        sims = proj.sims(rng, X, bstar)
        rc, ent, grp = proj.entropy(sims, T)
        assert rc == 0
        host = [proj.host_group(sims[0], k, T) for k in range(3)]
        ref = [proj.mp_group(sims[0], k, T) for k in range(3)]
        assert host[0] == -np.inf and np.isfinite(grp[0, 0]) and ref[0] < -745.0
        for k in range(3):
            assert abs(grp[0, k] - ref[k]) <= (bound if k else RULE_TOL), (k, grp[0, k], ref[k], host[k])
        assert np.isfinite(ent[0])
    finally:
        proj.close()


def test_entropy_kernel_degenerate_inputs(gpu_models):
    """A NaN simulation (in a row WITHOUT a scale factor) in vector 2 and b <= 0 for one group in vector 4 give
    entropy -inf there and leave the other vectors alone; sbm_mh_accept then keeps those chains where they were; a
    project without a prior on one group is refused with SBM_E_ARG."""
    import torch
    from sysbio_modeling_amd import _lib
    model = gpu_models('simple')
    proj = _Synthetic(model, (1, 7, 70), 9, D=(10.0, 20.0, 30.0), mu=(0.0, 0.2, -0.3), prior_sigma=(0.5, 0.9, 2.0), seed=6)
    nopr = _Synthetic(model, (1, 7, 70), 9, D=(10.0, 20.0, 30.0), mu=(0.0, 0.2, -0.3), prior_sigma=(0.5, 0.9, 2.0), seed=6,
                      with_priors=(0, 2))
    try:
        rng = np.random.default_rng(9)
        V = 6
        X, bstar = _targets(rng, proj, V)
        sims = proj.sims(rng, X, bstar)
        clean = proj.entropy(sims, 1.0)[1]
        assert np.all(np.isfinite(clean))
        sims[2, np.flatnonzero(proj.sf == -1)[0]] = np.nan
        sims[4, proj.sf == 1] *= -1.0
        rc, ent, grp = proj.entropy(sims, 1.0)
        assert rc == 0
        assert ent[2] == -np.inf and ent[4] == -np.inf and grp[4, 1] == -np.inf and np.isfinite(grp[4, 0])
        keep = [0, 1, 3, 5]
        assert np.array_equal(ent[keep], clean[keep])
        # the acceptance rule on these entropies: chains 2 and 4 stay, the others (log_u = -inf, finite energies) move
        ctx = _lib.default_context()
        q = 3
        dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
        trial, curr0 = rng.standard_normal((V, q)), rng.standard_normal((V, q))
        curr, F = dev(curr0), dev(np.full(V, 5.0))
        norms_d, st_d, ent_d, lu_d, trial_d = (dev(np.ones(V)), dev(np.zeros(V), torch.int32), dev(ent), dev(np.full(V, -np.inf)),
                                               dev(trial))
        n_acc = torch.zeros(V, dtype=torch.int32, device='cuda')
        slot, slot_F = torch.zeros((V, q), dtype=torch.float64, device='cuda'), torch.zeros(V, dtype=torch.float64, device='cuda')
        p = _lib.dev_ptr
        _lib.check(ctx.lib.sbm_mh_accept(ctx.handle, p(norms_d), p(st_d), p(ent_d), p(lu_d), 1.0, V, q, p(trial_d), p(curr), p(F),
                                         p(n_acc), p(slot), p(slot_F)), 'sbm_mh_accept')
        torch.cuda.synchronize()
        moved = np.array([1, 1, 0, 1, 0, 1], dtype=bool)
        assert np.array_equal(n_acc.cpu().numpy(), moved.astype(np.int32))
        assert np.array_equal(curr.cpu().numpy(), np.where(moved[:, None], trial, curr0))
        assert np.array_equal(slot.cpu().numpy(), curr.cpu().numpy())
        assert np.array_equal(F.cpu().numpy(), np.where(moved, 0.5 - ent, 5.0))
        assert np.array_equal(slot_F.cpu().numpy(), F.cpu().numpy())
        # no prior on group 1
        rc, _, _ = nopr.entropy(sims, 1.0)
        assert rc == -1 and b'log prior' in ctx.lib.sbm_last_error()
    finally:
        proj.close()
        nopr.close()


def test_propose_kernel(gpu_models):
    """trial = curr + samp z with one matrix for all chains and with one per chain."""
    import torch
    from sysbio_modeling_amd import _lib
    ctx = _lib.default_context()
    rng = np.random.default_rng(4)
    p = _lib.dev_ptr
    for C, q in ((3, 2), (65, 7)):
        curr, z = rng.standard_normal((C, q)), rng.standard_normal((C, q))
        for per_chain, samp in ((0, rng.standard_normal((q, q))), (1, rng.standard_normal((C, q, q)))):
            ref = curr + (np.einsum('cij,cj->ci', samp, z) if per_chain else z @ samp.T)
            d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (curr, samp, z)]
            trial = torch.empty((C, q), dtype=torch.float64, device='cuda')
            _lib.check(ctx.lib.sbm_mh_propose(ctx.handle, p(d[0]), p(d[1]), per_chain, p(d[2]), C, q, p(trial)), 'sbm_mh_propose')
            torch.cuda.synchronize()
            assert np.allclose(trial.cpu().numpy(), ref, rtol=0, atol=1e-14 * q * np.abs(samp).max() * np.abs(z).max())


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
def _gaussian_posterior_project(gpu_models, scale_factor):
    """The project of test_gpu_fitting.test_multi_chain_sampler_reproduces_the_gaussian_posterior; with
    ``scale_factor`` a scale factor on its measure, a log prior (0.1, 1.0) on it and 5 % error bars instead of 1 %:
    a B*^2 ~ 8e3 and a prior centre that stays within 3 prior sigmas of log B* along the chains, inside the ranges the
    entropy test measures its bound on.  (With 1 % error bars and a prior sigma of 0.5 the chains reach log I ~ -11,
    where scipy's quad, which stops at an ABSOLUTE error estimate, is 1.3e-7 off in the logarithm: a host replay
    could then not agree with the device to the bound of the entropy test, whatever the device does.)"""
    from sysbio_modeling_amd.experiment import Experiment
    from sysbio_modeling_amd.measurement import TimecourseMeasurement
    from sysbio_modeling_amd.project import Project
    m = gpu_models('simple')
    t = np.linspace(5.0, 100.0, 20)
    grid = np.linspace(0, 100.0, 1000)
    y = m.simulate(np.array([0.05, 0.3]), np.concatenate([[0.0], grid[np.searchsorted(grid, t)]]))[1:, 0]
    exp = Experiment('E', TimecourseMeasurement('Variable_1', y, t, (0.05 if scale_factor else 0.01) * y))
    kw = dict(sf_groups=[frozenset(['Variable_1'])]) if scale_factor else {}
    proj = Project(m, [exp], {'Global': ['k_deg', 'k_synt']}, {'Variable_1': ('direct', 0)}, reference_compat=False, **kw)
    if scale_factor:
        proj.set_scale_factor_log_prior('Variable_1', 0.1, 1.0)
    truth = np.zeros(2)
    truth[proj.get_param_index('k_deg', 'Global')] = np.log(0.05)
    truth[proj.get_param_index('k_synt', 'Global')] = np.log(0.3)
    return proj, truth


@pytest.fixture(scope='module')
def sf_project(gpu_models):
    """(project, truth, J^T J, the quadrature bound measured by the entropy test)"""
    proj, truth = _gaussian_posterior_project(gpu_models, True)
    J = proj.calc_project_jacobian(truth)
    return proj, truth, J.T @ J, _entropy_errors(gpu_models('simple'))['bound']


def _host_replay(proj, starts, samp, z, log_u, T, energy, every, **overrides):
    """The chain of ensembles.py:108-130 with given draws: project.evaluate_batch and the host scale_factor_entropy."""
    def F(th):
        res = proj.evaluate_batch(th, want=('sims', 'norms', 'status'), **overrides)
        out = 0.5 * res['norms']
        if energy == 'free_energy':
            out = out - np.array([proj.calc_scale_factors_entropy(T, sims=s) for s in res['sims']])
        return np.where(np.isfinite(out) & (res['status'] == 0), out, np.inf)
    curr, Fc = starts.copy(), F(starts)
    ens, ens_F, n_acc, margin = [curr.copy()], [Fc.copy()], np.zeros(len(starts)), np.inf
    for n in range(len(z)):
        trial = curr + z[n] @ samp.T
        Ft = F(trial)
        acc = np.isfinite(Ft) & (log_u[n] < -(Ft - Fc) / T)
        margin = min(margin, np.min(np.abs(log_u[n] + (Ft - Fc) / T)[np.isfinite(Ft)], initial=np.inf))
        curr, Fc = np.where(acc[:, None], trial, curr), np.where(acc, Ft, Fc)
        n_acc += acc
        if (n + 1) % every == 0:
            ens.append(curr.copy())
            ens_F.append(Fc.copy())
    return np.stack(ens), np.stack(ens_F), n_acc / len(z), margin


@pytest.mark.parametrize('energy', ['rss', 'free_energy'])
@pytest.mark.parametrize('skip_elems', [0, 4])
@pytest.mark.parametrize('C', [3, 65])
def test_device_sampler_walks_the_host_chain_with_the_same_draws(gpu_models, sf_project, C, skip_elems, energy):
    """sampler='device' with draws= against the host replay: the same accept decisions at every step (with
    skip_elems = 0 every step is recorded, so equal records mean equal decisions; the acceptance counts are compared
    exactly in both cases), positions to 1e-12, energies within the quadrature bound measured by the entropy test: an
    energy differs from the replay's by T (device error + host error) <= 2 T bound, plus the rounding of 0.5 |r|^2.
    The smallest |log u + dF / T| of the run must exceed 1e-6, far above that bound: no decision hangs on the
    quadrature."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch, sampling_matrix
    proj, truth, hess, bound = sf_project
    T, steps = 1.5, 30
    rng = np.random.default_rng(100 + C)
    starts = truth[None, :] + 0.01 * rng.standard_normal((C, 2))
    z, log_u = rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C)))
    samp = sampling_matrix(hess, 1e-4, T, 1.0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ens_h, F_h, ratio_h, margin = _host_replay(proj, starts, samp, z, log_u, T, energy, skip_elems + 1)
    ens_d, F_d, ratio_d = ensemble_log_params_batch(proj, starts, hess=hess, steps=steps, temperature=T, sing_val_cutoff=1e-4,
                                                    skip_elems=skip_elems, energy=energy, sampler='device', draws=(z, log_u))
    print("C=%d skip=%d %s: margin %.3e, max |dF| %.3e, max |dx| %.3e, acceptance %.2f"
          % (C, skip_elems, energy, margin, np.max(np.abs(F_d - F_h)), np.max(np.abs(ens_d - ens_h)), ratio_h.mean()))
    assert margin > 1e-6
    assert ens_d.shape == ens_h.shape == (1 + steps // (skip_elems + 1), C, 2) and F_d.shape == F_h.shape
    assert np.array_equal(ratio_d, ratio_h) and 0.05 < ratio_h.mean() < 0.95
    assert np.max(np.abs(ens_d - ens_h)) <= 1e-12
    tol = (2.0 * T * bound if energy == 'free_energy' else 0.0) + 1e-12 * np.maximum(1.0, np.abs(F_h))
    assert np.all(np.abs(F_d - F_h) <= tol)


def test_device_sampler_with_a_host_control_loop_integrator(gpu_models, sf_project):
    """method='auto' is a host control loop: the device sampler integrates through evaluate_batch and hands its tensors to
    the entropy and acceptance kernels.  Same draws, same chain as the replay with the same method."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch, sampling_matrix
    proj, truth, hess, bound = sf_project
    T, steps, C = 1.0, 5, 3
    rng = np.random.default_rng(31)
    starts = truth[None, :] + 0.01 * rng.standard_normal((C, 2))
    z, log_u = rng.standard_normal((steps, C, 2)), np.log(rng.random((steps, C)))
    samp = sampling_matrix(hess, 1e-4, T, 1.0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ens_h, F_h, ratio_h, margin = _host_replay(proj, starts, samp, z, log_u, T, 'free_energy', 1, method='auto')
        ens_d, F_d, ratio_d = ensemble_log_params_batch(proj, starts, hess=hess, steps=steps, temperature=T, sing_val_cutoff=1e-4,
                                                        energy='free_energy', sampler='device', draws=(z, log_u), method='auto')
    assert margin > 1e-6 and np.array_equal(ratio_d, ratio_h)
    assert np.max(np.abs(ens_d - ens_h)) <= 1e-12
    assert np.all(np.abs(F_d - F_h) <= 2.0 * T * bound + 1e-12 * np.maximum(1.0, np.abs(F_h)))


def test_device_sampler_reproduces_the_gaussian_posterior(gpu_models):
    """The statistics of test_gpu_fitting.test_multi_chain_sampler_reproduces_the_gaussian_posterior with
    sampler='device': 128 chains, 400 steps, random numbers drawn on the device."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    proj, truth = _gaussian_posterior_project(gpu_models, False)
    J = proj.calc_project_jacobian(truth)
    cov = np.linalg.inv(J.T @ J)
    ens, ens_F, ratio = ensemble_log_params_batch(proj, np.tile(truth, (128, 1)), steps=400, seeds=11, sampler='device')
    assert ens.shape == (401, 128, 2) and ens_F.shape == (401, 128) and ratio.shape == (128,)
    assert 0.3 < ratio.mean() < 0.75
    assert np.all(ens_F[0] < 1e-12) and np.all(ens_F >= 0)
    pooled = ens[100:].reshape(-1, 2)
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(pooled.mean(axis=0) - truth) < 0.1 * sd)
    assert np.allclose(pooled.std(axis=0), sd, rtol=0.15)
    assert np.corrcoef(pooled.T)[0, 1] == pytest.approx(cov[0, 1] / (sd[0] * sd[1]), abs=0.1)
    # the same seed gives the same chains, another seed others; skip_elems thins the record, not the walk
    runs = [ensemble_log_params_batch(proj, np.tile(truth, (4, 1)), steps=20, seeds=s, sampler='device')[0] for s in (5, 5, 6)]
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0], runs[2])
    ens2, _, _ = ensemble_log_params_batch(proj, truth, steps=50, seeds=3, skip_elems=4, sampler='device')
    assert ens2.shape == (11, 1, 2)


def test_device_free_energy_and_argument_checks(gpu_models, sf_project):
    """free_energy_batch(device=True) against the host path within the measured quadrature bound;
    scale_factors_entropy_batch against calc_scale_factors_entropy; what sampler='device' refuses."""
    from sysbio_modeling_amd.project.ensembles import ensemble_log_params_batch
    proj, truth, hess, bound = sf_project
    th = truth[None, :] + 0.02 * np.random.default_rng(1).standard_normal((5, 2))
    for T in (1.0, 2.5):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            host = proj.free_energy_batch(th, T)
        got = proj.free_energy_batch(th, T, device=True)
        assert np.all(np.abs(got - host) <= 2.0 * T * bound + 1e-12 * np.abs(host))
    sims = proj.evaluate_batch(th, want=('sims',))['sims']
    ent, grp = proj.scale_factors_entropy_batch(sims, 2.5, group_entropy=True)
    assert ent.shape == (5,) and grp.shape == (5, 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.all(np.abs(ent - [proj.calc_scale_factors_entropy(2.5, sims=s) for s in sims]) <= 2.0 * 2.5 * bound)
    with pytest.raises(ValueError):
        ensemble_log_params_batch(proj, truth, hess=hess, steps=2, sampler='device', recalc_hess_alg=True)
    with pytest.raises(ValueError):
        ensemble_log_params_batch(proj, truth, hess=hess, steps=2, sampler='gpu')
    with pytest.raises(ValueError):
        ensemble_log_params_batch(proj, truth, hess=hess, steps=2, sampler='device', draws=(np.zeros((3, 1, 2)), np.zeros((3, 1))))
