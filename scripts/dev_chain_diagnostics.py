"""Chain diagnostics at the workload shape (N = 16384 kept steps, C = 64 chains, q = 68 parameters: 4352 series), device
buffers in and out: (a) sbm_chain_autocorr with K = 1024 lags, (b) with K = N, the reference's semantics, (c) the same
normalised autocorrelation through torch.fft.rfft / irfft of the 2N-padded record on the device, with its peak extra memory,
and the reference's way: a numpy FFT per series on the host (timed on a sample of the series and scaled).
docs/history.md, "Chain diagnostics", has the figures.   usage: dev_chain_diagnostics.py [N C q]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sysbio_modeling_amd import _lib

N, C, q = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (16384, 64, 68)
S = C * q
ctx = _lib.default_context()
dev = torch.device('cuda:0')
p = _lib.dev_ptr
gen = torch.Generator(device=dev)
gen.manual_seed(1)
# AR(1) chains, phi = 0.9, built on the device: x_i = phi x_{i-1} + e_i
e = torch.randn((N, S), dtype=torch.float64, device=dev, generator=gen)
rec = torch.empty_like(e)
rec[0] = e[0] / np.sqrt(1.0 - 0.81)
for i in range(1, N):
    torch.add(e[i], rec[i - 1], alpha=0.9, out=rec[i])
del e
torch.cuda.synchronize()


def timed(fn, reps=4):
    best = 1e9
    for rep in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep:
            best = min(best, dt)
    return best


def device_call(K, with_rest):
    ac = torch.empty((S, K), dtype=torch.float64, device=dev)
    tau = torch.empty((S,), dtype=torch.float64, device=dev) if with_rest else None
    mom = torch.empty((S, 4), dtype=torch.float64, device=dev) if with_rest else None
    flags = torch.empty((S,), dtype=torch.int32, device=dev) if with_rest else None
    rhat = torch.empty((q,), dtype=torch.float64, device=dev)
    ess = torch.empty((q,), dtype=torch.float64, device=dev)

    def run():
        _lib.check(ctx.lib.sbm_chain_autocorr(ctx.handle, p(rec), N, S, S, K, p(ac), p(tau), p(mom), p(flags)), 'sbm_chain_autocorr')
        if with_rest:
            _lib.check(ctx.lib.sbm_chain_summary(ctx.handle, p(mom), p(tau), N, C, q, p(rhat), p(ess)), 'sbm_chain_summary')
    return run, ac


def fft_autocorr(K):
    """the reference's formula on the whole record at once; lag-first (K, S)"""
    d = rec - rec.mean(dim=0, keepdim=True)
    f = torch.fft.rfft(d, n=2 * N, dim=0)
    ac = torch.fft.irfft(f.real * f.real + f.imag * f.imag, n=2 * N, dim=0)[:K]
    ac = ac * (N / (N - torch.arange(K, dtype=torch.float64, device=dev)))[:, None]
    return ac / ac[0]


print('record %d x %d x %d: %d series, %.0f MB' % (N, C, q, S, rec.numel() * 8e-6), flush=True)
for label, K in (('(a) K = 1024', min(1024, N - 1)), ('(b) K = N', N)):
    run_ac, ac = device_call(K, False)
    run_all, _ = device_call(K, True)
    t_ac, t_all = timed(run_ac), timed(run_all)
    fma = S * sum(N - k for k in range(K))
    print('%s: autocorrelation alone %8.2f ms (%.2e FMA, %.2f TFMA/s)   with tau, moments, flags, r_hat, ess %8.2f ms'
          % (label, 1e3 * t_ac, fma, fma / t_ac * 1e-12, 1e3 * t_all), flush=True)
    if K < N:
        ref = fft_autocorr(K)
        print('    max |direct - FFT| over all series and lags: %.3g' % float((ac.t() - ref).abs().max()), flush=True)
        del ref
    del ac, run_ac, run_all
for label, K in (('K = 1024', min(1024, N - 1)), ('K = N', N)):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t_fft = timed(lambda: fft_autocorr(K))
    peak = torch.cuda.max_memory_allocated(dev) - base
    print('(c) torch.fft on the device, %s: %8.2f ms, peak extra memory %.0f MB' % (label, 1e3 * t_fft, peak * 1e-6), flush=True)
host = rec[:, :64].cpu().numpy()
t0 = time.perf_counter()
for s in range(host.shape[1]):
    x = host[:, s]
    f = np.fft.rfft(x - x.mean(), n=2 * N)
    a = np.fft.irfft(np.abs(f) ** 2)[:N] * (N / (N - 1.0 * np.arange(N)))
    a = a / a[0]
dt = time.perf_counter() - t0
print('(c) numpy FFT loop on the host: %.3f ms per series, %.2f s for %d series (scaled from 64), plus the read-back of %.0f MB'
      % (1e3 * dt / 64, dt / 64 * S, S, rec.numel() * 8e-6), flush=True)
