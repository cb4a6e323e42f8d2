"""Shared by the scale-factor entropy tests: the mpmath reference of the integral and the host compilation of the
quadrature rule (csrc/sbm_sf_quadrature.hpp)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mp_log_integral(a, b, mu, sigma, temperature, dps=25):
    """log integral du exp(-a / (2 T) (e^u B* - B*)^2 - (u + log B* - mu)^2 / (2 sigma^2)), B* = b / a, by ``mpmath.quad``
    at ``dps`` digits with break points at the edges (and centres) of both windows of the integrand: the likelihood
    factor's around u = 0 and the prior factor's around u = mu - log B*.  ``a`` and ``b`` may be mpmath numbers (exact
    row sums)."""
    import mpmath
    with mpmath.workdps(dps):
        a, b, mu, sg, T = (mpmath.mpf(x) for x in (a, b, mu, sigma, temperature))
        bs = b / a
        alpha, c = a * bs * bs / (2 * T), mu - mpmath.log(bs)

        def logf(u):
            return -alpha * mpmath.expm1(u) ** 2 - (u - c) ** 2 / (2 * sg ** 2)
        w1 = 1 / mpmath.sqrt(2 * alpha + 1 / sg ** 2)
        pts = sorted(set([c - 60 * sg, c - 12 * sg, c - 4 * sg, c, c + 4 * sg, c + 12 * sg, c + 60 * sg,
                          -60 * w1, -12 * w1, -4 * w1, mpmath.mpf(0), 4 * w1, 12 * w1, 60 * w1]))
        # quad's error control is absolute: the integrand is divided by (about) its maximum, which lies between 0 and c
        m = max(logf(c * k / 256) for k in range(257))
        return float(m + mpmath.log(mpmath.quad(lambda u: mpmath.exp(logf(u) - m), pts, maxdegree=10)))


def mp_row_sums(sims, data, sigma):
    """a = sum s^2 / sigma^2 and b = sum s d / sigma^2 of one group's rows, summed exactly (mpmath numbers)."""
    import mpmath
    with mpmath.workdps(40):
        a = mpmath.fsum(mpmath.mpf(float(s)) ** 2 / mpmath.mpf(float(g)) ** 2 for s, g in zip(sims, sigma))
        b = mpmath.fsum(mpmath.mpf(float(s)) * mpmath.mpf(float(d)) / mpmath.mpf(float(g)) ** 2
                        for s, d, g in zip(sims, data, sigma))
    return a, b


_WRAPPER = '''
#include "sbm_sf_quadrature.hpp"
extern "C" double sfq_log_integral(double alpha, double c, double sigma) { return sbm_sfq_log_integral(alpha, c, sigma); }
extern "C" int sfq_from_sums(double a, double b, double mu, double sigma, double T, double* out) {
  double alpha, c;
  if (!sbm_sfq_params(a, b, mu, T, &alpha, &c)) return 0;
  *out = sbm_sfq_log_integral(alpha, c, sigma);
  return 1;
}
extern "C" int sfq_panels(double alpha, double c, double sigma) {
  sbm_sfq_plan q;
  sbm_sfq_make_plan(alpha, c, sigma, &q);
  return q.n[0] + q.n[1];
}
'''


def host_rule(tmp_dir):
    """The quadrature header compiled for the host with the C++ compiler: a ctypes library with ``sfq_log_integral``,
    ``sfq_from_sums`` and ``sfq_panels``."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        raise RuntimeError("no C++ compiler")
    src = os.path.join(str(tmp_dir), 'sfq_host.cpp')
    out = os.path.join(str(tmp_dir), 'sfq_host.so')
    with open(src, 'w') as fh:
        fh.write(_WRAPPER)
    subprocess.run([cxx, '-O2', '-std=c++17', '-fPIC', '-shared', '-I', os.path.join(REPO, 'sysbio_modeling_amd', 'csrc'),
                    src, '-o', out], check=True)
    lib = ctypes.CDLL(out)
    lib.sfq_log_integral.restype = ctypes.c_double
    lib.sfq_log_integral.argtypes = [ctypes.c_double] * 3
    lib.sfq_from_sums.restype = ctypes.c_int
    lib.sfq_from_sums.argtypes = [ctypes.c_double] * 5 + [ctypes.POINTER(ctypes.c_double)]
    lib.sfq_panels.restype = ctypes.c_int
    lib.sfq_panels.argtypes = [ctypes.c_double] * 3
    return lib


def group_sims(rng, data, sigma, X, bstar):
    """Simulations of one scale-factor group with prescribed a B*^2 = X and B* = bstar: a multiple of the data plus a
    component orthogonal to it in the 1 / sigma^2 metric.  Needs X <= D = sum d^2 / sigma^2 (X = D for a single row)."""
    w = 1.0 / sigma ** 2
    D = np.sum(data ** 2 * w)
    e1 = data / np.sqrt(D)
    if len(data) == 1:
        return e1 * np.sqrt(D) / bstar
    cos2 = X / D
    assert cos2 <= 1.0
    n = rng.standard_normal(len(data))
    n -= np.sum(n * e1 * w) * e1
    n /= np.sqrt(np.sum(n * n * w))
    lam = np.sqrt(cos2 * D) / bstar
    return lam * (np.sqrt(cos2) * e1 + np.sqrt(1.0 - cos2) * n)
