"""Oracle of the chain diagnostics (``sbm_chain_autocorr`` / ``sbm_chain_summary``, include/sbm.h) in ``np.longdouble``:
the direct lag sums, Geyer's window, split-R-hat and the effective sample size exactly as the header defines them, the
error bound the GPU tests hold the kernels to, and the test inputs (fixed seeds) that the CPU test vets first."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FLAG_CONSTANT, FLAG_TRUNCATED = 1, 2


def deviations(x):
    """(d, c0) of one series in extended precision: d = x - mean(x), c0 = sum d^2 / N"""
    x = np.asarray(x, dtype=LD)
    d = x - x.sum() / LD(x.size)
    return d, (d * d).sum() / LD(x.size)


def autocorrelation(x, K=None):
    """ac[k] = (sum_{i < N-k} d_i d_{i+k} / (N - k)) / c0, k < K (default N).  A constant series: NaN at every lag."""
    N = len(x)
    K = N if K is None else int(K)
    if np.min(x) == np.max(x):
        return np.full(K, np.nan, dtype=LD)
    d, c0 = deviations(x)
    return np.array([(d[:N - k] * d[k:]).sum() / LD(N - k) / c0 for k in range(K)], dtype=LD)


def autocorrelation_fft(x):
    """The reference's formula (project/Ensembles.py:14-29) with numpy.fft: 2N zero-padded de-meaned series, |f|^2
    transformed back, the first N lags times N / (N - k), divided by lag 0."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    f = np.fft.rfft(x - x.mean(), n=2 * N)
    ac = np.fft.irfft(np.abs(f) ** 2)[:N]
    ac = ac * (N / (N - 1.0 * np.arange(N)))
    return ac / ac[0]


def tolerance(x, K=None):
    """tol_k = 8 N u [ (sum_i |d_i d_{i+k}| / (N - k) + max|d|^2) / c0 + |ac_k| ]: first-order bound of a fixed-order sum
    of N - k products, the mean's error N u max|x - x_0| at every lag, the two divisions; 8 = margin for the order."""
    N = len(x)
    K = N if K is None else int(K)
    d, c0 = deviations(x)
    ac = autocorrelation(x, K)
    a = np.abs(d)
    s = np.array([(a[:N - k] * a[k:]).sum() / LD(N - k) for k in range(K)], dtype=LD)
    return np.asarray(8 * N * U * ((s + a.max() ** 2) / c0 + np.abs(ac)), dtype=np.float64)


def gammas(ac):
    ac = np.asarray(ac)
    pairs = ac.size // 2
    return ac[0:2 * pairs:2] + ac[1:2 * pairs:2]


def geyer(ac):
    """(tau, M, truncated) of the window rule on ``ac`` (any float type; sums in that type, in order)."""
    ac = np.asarray(ac)
    g = gammas(ac)
    stop = np.flatnonzero(g <= 0)
    M = int(stop[0]) if stop.size else g.size
    tau = -1 + 2 * g[:M].sum() if M else ac.dtype.type(-1)
    if np.isnan(ac[0]):
        return ac.dtype.type(np.nan), g.size, False
    return tau, M, not stop.size


def half_moments(x):
    """(mean, unbiased variance) of the first n = N // 2 steps and of the last n; n == 1: the variance is NaN"""
    x = np.asarray(x, dtype=LD)
    n = x.size // 2
    out = []
    for h in (x[:n], x[x.size - n:]):
        mu = h.sum() / LD(n)
        out += [mu, ((h - mu) ** 2).sum() / LD(n - 1) if n > 1 else LD(np.nan)]
    return np.array(out, dtype=LD)


def summary(ens, K):
    """(r_hat (q,), ess (q,), tau (C, q)) of an ensemble (N, C, q): split-R-hat over the 2C half-chains, ess = sum over
    the chains with a tau of N / tau, tau by the window rule on K lags"""
    ens = np.asarray(ens, dtype=np.float64)
    N, C, q = ens.shape
    n = N // 2
    rhat, ess, taus = np.full(q, np.nan, dtype=LD), np.full(q, np.nan, dtype=LD), np.full((C, q), np.nan, dtype=LD)
    for j in range(q):
        mom = np.array([half_moments(ens[:, c, j]) for c in range(C)])
        means, var = mom[:, [0, 2]].ravel(), mom[:, [1, 3]].ravel()
        W = var.sum() / LD(2 * C)
        Bn = ((means - means.sum() / LD(2 * C)) ** 2).sum() / LD(2 * C - 1)
        if W != 0:
            rhat[j] = np.sqrt((LD(n - 1) / LD(n) * W + Bn) / W)
        for c in range(C):
            taus[c, j] = geyer(autocorrelation(ens[:, c, j], K))[0]
        ok = ~np.isnan(taus[:, j])
        if ok.any():
            ess[j] = (LD(N) / taus[ok, j]).sum()
    return rhat, ess, taus


# ---------------------------------------------------------------------------------------------
# inputs of tests/test_gpu_chain_diagnostics.py; tests/test_chain_diagnostics_cpu.py checks the conditions on them
# ---------------------------------------------------------------------------------------------
def ar1(phi, N, seed, S=1):
    """(N, S) stationary AR(1) series x_i = phi x_{i-1} + e_i, unit innovations"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((N, S))
    x = np.empty((N, S))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for i in range(1, N):
        x[i] = phi * x[i - 1] + e[i]
    return x


AR1_N, AR1_K = 8192, 512
AR1_SEEDS = {0.0: 11, 0.5: 12, 0.9: 13}       # phi: seed


def ar1_case(phi):
    return ar1(phi, AR1_N, AR1_SEEDS[phi])[:, 0]


def random_record(N, S, seed, offset=3.0):
    """(N, S) independent AR(1) series with phi spread over [0, 0.8], offset from zero"""
    phis = np.linspace(0.0, 0.8, S)
    return np.stack([ar1(phis[s], N, seed + 101 * s)[:, 0] for s in range(S)], axis=1) + offset
