"""The chain diagnostics without a device: the oracle of tests/support/chain_diagnostics_oracle.py against the reference's
FFT formula, the C ABI's declarations, the window rule of csrc/sbm_chain_diagnostics.hpp compiled for the host (plain and
under AddressSanitizer / UBSan, as a child process), and the conditions the inputs of the GPU tests have to meet."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.support import chain_diagnostics_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sysbio_modeling_amd', 'csrc')
MAIN = os.path.join(ROOT, 'tests', 'support', 'geyer_window_main.cpp')


def _series_cases():
    rng = np.random.default_rng(5)
    cases = [('N=%d' % N, rng.standard_normal(N) + 3.0) for N in (2, 3, 63, 64, 65, 1025)]
    cases += [('ar1 phi=%g' % phi, co.ar1_case(phi)[:2048]) for phi in co.AR1_SEEDS]
    return cases


def test_oracle_is_the_references_fft_formula():
    for name, x in _series_cases():
        direct = np.asarray(co.autocorrelation(x), dtype=np.float64)
        fft = co.autocorrelation_fft(x)
        assert direct[0] == 1.0
        err = np.max(np.abs(direct - fft))
        print(name, 'max |direct - fft| = %.3g' % err)
        assert err <= 1e-12, name


def test_header_and_bindings_declare_the_entries():
    from sysbio_modeling_amd import _lib
    with open(os.path.join(ROOT, 'include', 'sbm.h')) as fh:
        text = fh.read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+sbm_chain_autocorr\s*\(', code) and re.search(r'\bint\s+sbm_chain_summary\s*\(', code)
    assert re.search(r'#define\s+SBM_CHAIN_MAX_STEPS\s+16384\b', text) and _lib.CHAIN_MAX_STEPS == 16384
    assert re.search(r'#define\s+SBM_ABI_VERSION\s+4\b', text) and _lib.ABI_VERSION == 4
    assert len(_lib.SIGNATURES['sbm_chain_autocorr'][1]) == 10 and len(_lib.SIGNATURES['sbm_chain_summary'][1]) == 8
    lib = _lib.load_library()
    assert hasattr(lib, 'sbm_chain_autocorr') and hasattr(lib, 'sbm_chain_summary')
    from sysbio_modeling_amd import project
    assert callable(project.autocorrelation) and callable(project.ensemble_diagnostics)


# ---------------------------------------------------------------------------------------------
# the window rule on the host
# ---------------------------------------------------------------------------------------------
def _build(out, flags):
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-g', *flags, '-I', CSRC, MAIN, '-o', str(out)], check=True,
                   capture_output=True)
    return str(out)


@pytest.fixture(scope='module')
def binaries(tmp_path_factory):
    d = tmp_path_factory.mktemp('geyer')
    # the runtimes linked statically: the program stands alone, whatever else the environment loads into a process
    return (_build(d / 'plain', ['-O1']),
            _build(d / 'sanitized', ['-O1', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan',
                                     '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']))


WINDOW_CASES = [
    [1.0],                                              # K = 1: no complete pair
    [1.0, 0.5],                                         # K = 2: one pair, no stop
    [1.0, -1.0],                                        # K = 2: the first pair stops (m = 0)
    [1.0, 0.5, -9.0],                                   # K = 3: the odd trailing lag is ignored
    [1.0, -1.5, 0.3],                                   # K = 3, stop at m = 0
    [1.0, 0.6, 0.4, 0.2, 0.1, -0.2],                    # even K, stop at the last pair
    [1.0, 0.6, 0.4, 0.2, 0.1, -0.2, 7.0],               # odd K, stop at the last complete pair
    [1.0, 0.6, 0.4, 0.2, 0.1, 0.05],                    # even K, no stop
    [1.0, 0.6, 0.4, 0.2, 0.1, 0.05, -3.0],              # odd K, no stop: the trailing lag does not count
    [1.0, 0.6, -0.3, -0.4, 0.5, 0.5, 0.5, 0.5],         # stop in the middle: later positive pairs do not count
    [1.0, 0.5, -0.25, 0.25],                            # Gamma_1 == 0 stops
    [float('nan')] * 4,                                 # a constant series
]


def test_window_rule_compiles_for_the_host_and_reads_only_its_lags(binaries, tmp_path):
    path = tmp_path / 'cases.txt'
    path.write_text('\n'.join(' '.join(float(v).hex() for v in c) for c in WINDOW_CASES) + '\n')
    for binary in binaries:
        proc = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=120)
        assert proc.returncode == 0 and proc.stderr == '', (binary, proc.stderr)
        lines = proc.stdout.splitlines()
        assert len(lines) == len(WINDOW_CASES)
        for c, line in zip(WINDOW_CASES, lines):
            tau_s, trunc_s = line.split('\t')
            tau, M, truncated = co.geyer(np.array(c, dtype=np.float64))
            if np.isnan(tau):
                assert np.isnan(float.fromhex(tau_s)), c
            else:
                assert float.fromhex(tau_s) == float(tau), (c, tau_s, tau)
            assert int(trunc_s) == int(truncated), c


# ---------------------------------------------------------------------------------------------
# what tests/test_gpu_chain_diagnostics.py assumes of its inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('phi', sorted(co.AR1_SEEDS))
def test_ar1_cases_keep_their_windows_clear_of_zero(phi):
    """No Gamma_m up to and including the one that closes the window lies within tol_2m + tol_2m+1 of zero: a kernel
    within its bound closes the window at the oracle's M."""
    x = co.ar1_case(phi)
    ac, tol = co.autocorrelation(x, co.AR1_K), co.tolerance(x, co.AR1_K)
    g = co.gammas(ac)
    tau, M, truncated = co.geyer(ac)
    assert not truncated and M < g.size
    margin = np.abs(np.asarray(g[:M + 1], dtype=np.float64)) - (tol[0:2 * M + 2:2] + tol[1:2 * M + 2:2])
    print('phi = %g: M = %d, tau = %.4f, smallest margin %.3g' % (phi, M, float(tau), margin.min()))
    assert np.all(margin > 0)


def test_ar1_tau_is_near_its_expectation():
    tau = float(co.geyer(co.autocorrelation(co.ar1_case(0.5), co.AR1_K))[0])
    print('tau = %.4f' % tau)
    assert abs(tau - 3.0) <= 0.25 * 3.0


def test_truncated_case_is_truncated():
    """phi = 0.9 with K = 4: both pairs positive and clear of zero"""
    x = co.ar1_case(0.9)
    ac, tol = co.autocorrelation(x, 4), co.tolerance(x, 4)
    g = np.asarray(co.gammas(ac), dtype=np.float64)
    assert co.geyer(ac)[2] and np.all(g - (tol[0::2] + tol[1::2]) > 0)
