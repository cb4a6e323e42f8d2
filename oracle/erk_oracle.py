"""ORACLE (test infrastructure, not product code) -- the two adaptive explicit drivers, DOPRI45 and DOP853, restated.

csrc/sbm_rk_drivers.hpp::sbm_dopri45 / sbm_dop853 run one controller per WAVEFRONT: one trajectory's state together with
the sensitivity columns that wavefront holds (all of them, or one chunk of a column-chunked kernel).  This module restates
that driver in numpy, decision for decision: the solution arithmetic in plain float64, the controller arithmetic (error
ratios, their sums of squares, the norm, the step factor) in float32 as the driver has it.  Against it a kernel may differ
in rounding only -- in how it sums a row's products, contracts FMAs and approximates 1/x, log2 and exp2 in float32 -- so
that, on inputs whose decisions are not close calls (the margins returned below), step and rejection counts are equal
and the results agree at the rounding level of the problem instead of an integration tolerance.

THE RULES (one wavefront: state y, n rows; columns S[:, c] for c in ``columns``; ``sens=False``: the state alone)

  tableaus   DOPRI45: scipy.integrate._ivp.rk.RK45.{A, B, C, E}; DOP853: scipy.integrate._ivp.dop853_coefficients
             (A, B, C of the twelve stages, E3, E5).  Nothing is read from the header; tests/test_erk_oracle_cpu.py holds
             the header's entries to these, bit for bit.
  elements   "the elements" below are the n state entries and the n entries of each of the wavefront's columns, each once.
  start      t = t_out[0]; k1 = f(t, z).  h = h0 if h0 > 0, else Hairer's hinit with RAW sums (no division by the number of
             elements) over the elements:  sk = atol + rtol |z|, dnf = sum (k1 / sk)^2, dny = sum (z / sk)^2;
             h = 1e-6 if dnf <= 1e-10 or dny <= 1e-10 else 0.01 sqrt(dny / dnf);  h = min(h, span) with span = t_out[-1] -
             t_out[0] if that is > 0 else 1;  k2 = f(t + h, z + h k1);  der2 = sqrt(sum ((k2 - k1) / sk)^2) / h;
             der12 = max(|der2|, sqrt(dnf));  h1 = max(1e-6, 1e-3 |h|) if der12 <= 1e-15 else (0.01 / der12)^(1/q) with
             q = 5 (DOPRI45) or 8 (DOP853);  h = min(100 h, h1, span);  h = 1e-6 unless h > 0.
  outputs    for every output time, in order: step until t >= target, then record z.  t_out[0] records the initial values.
  budget     before an attempt: n_try >= budget -> status SBM_MAX_STEPS, failed.  budget = max_steps if > 0, |max_steps|
             if < 0, 10^6 if 0.
  early exit max_steps < 0 only, before an attempt with n_try >= 512 and n_try a multiple of 256:
             growing = float32(h) > 1.5 h_mark;  smooth = n_rej - rej_mark < 3;  then h_mark = float32(h), rej_mark = n_rej;
             not growing and not smooth and  t_out[-1] - t > 1.5 (budget - n_try) h  -> SBM_MAX_STEPS, failed.
  landing    hs = h; if t + 1.01 hs >= target: hs = target - t, the attempt is CLIPPED.
  stages     the tableau's, at hs; DOPRI45's seventh stage is f(t + hs, z_new) (FSAL), DOP853 forms z_new from B.
  error      per element  r = float32(e) * (1 / float32(atol + rtol max(|z|, |z_new|)))  in float32, e the embedded
             combination WITHOUT the factor hs;  per column and for the state the float32 sum of r^2 (NaN counts as inf);
             norm = sqrt(max(state sum, worst column sum) / n)   (``sens=False``: sqrt(state sum / n)).
             DOPRI45: err = |float32(hs)| norm(E).   DOP853: n5 = norm(E5), n3 = norm(E3), den = n5^2 + 0.01 n3^2,
             err = |float32(hs)| n5^2 / sqrt(den)  (0 if den is not > 0).
  controller finite = err is a number below 3e38 (DOP853: and so is n3).  accept = finite and err <= 1.
             fac = 0.9 max(err, 1e-30)^(-1/q) in float32, clipped to [0.2, 10] (DOPRI45) or [1/3, 6] (DOP853);
             not finite: fac = 0.2 / 1/3.
  accept     n_acc += 1;  t = target if clipped else t + hs;  z = z_new;  hn = hs fac;  h = max(hn, h) after a clipped step
             (a clipped step says nothing against the unclipped proposal), else hn.  DOPRI45: k1 = the seventh stage.
             DOP853: k1 = f(t, z) -- evaluated after acceptance only.
  reject     n_rej += 1;  h = hs min(fac, 1);  unless h > 1e-14 max(|t|, 1e-3): status SBM_STEP_UNDERFLOW (finite) or
             SBM_NON_FINITE, failed.  DOPRI45: k1 = f(t, z) again.
  failure    the output row of the interval that failed and every later one is NaN; counts as they stood.
  statuses   include/sbm.h: SBM_OK 0, SBM_MAX_STEPS 1, SBM_NON_FINITE 2, SBM_STEP_UNDERFLOW 3.

A column-chunked kernel (row-group splits, the matrix-core kernel) is one run per chunk (``integrate_chunks``): every chunk
sees the state once, in hinit and in the norm; Y is chunk 0's, status / n_acc / n_rej are the largest over the chunks.

MARGINS of a run, for choosing inputs whose decisions no rounding can flip: ``err_margin`` = min |err - 1| over the
attempts, ``land_margin`` = min over the attempts of |t + 1.01 hs - target| / (target - previous output time), and with
early exit ``exit_margins`` = for each of the three tests the smallest factor, over the checks made, by which its two
sides differ (max(a / b, b / a); the integer test n_rej - rej_mark < 3 is taken at 2.5).

``noise=(seed, a_rhs, a_err)`` multiplies every output of the right-hand side by 1 + a_rhs u and every err by 1 + a_err u,
u uniform in [-1, 1]: the model of a kernel's rounding from which the GPU tests' bound is derived.  ``mutate`` names ONE
deliberate error (MUTATIONS) -- the CPU tests show that the bound catches each.

PINNED: tests/test_erk_oracle_cpu.py (the header's tableaus against SciPy's, one step against SciPy's rk_step, parity with
odeint_oracle.tight_solution, order of convergence, margins of every input of tests/test_gpu_adaptive_scheme.py).

Only tests/ may import this.
"""
from __future__ import annotations

import re

import numpy as np

from .odeint_oracle import _wrap, _wrap_c

SBM_OK, SBM_MAX_STEPS, SBM_NON_FINITE, SBM_STEP_UNDERFLOW = 0, 1, 2, 3
F32 = np.float32
MUTATIONS = ('A65', 'E5', 'E3', 'landing', 'clip_max', 'fac_max', 'state_norm', 'hinit_all', 'budget')


def tableau(method):
    """dict(A (s, s) strictly lower, B (s,), C (s,), E or E5 / E3 (s + 1,), q) from SciPy; s = 6 / 12 stages before the
    new value's derivative, which the error weights' last entry multiplies."""
    if method == 'dopri45':
        from scipy.integrate._ivp.rk import RK45
        A = np.zeros((6, 6))
        A[:, :5] = RK45.A
        return dict(A=A, B=np.array(RK45.B, dtype=float), C=np.array(RK45.C, dtype=float), E=np.array(RK45.E, dtype=float), q=5)
    if method == 'dop853':
        from scipy.integrate._ivp import dop853_coefficients as d
        s = d.N_STAGES
        return dict(A=np.array(d.A[:s, :s]), B=np.array(d.B), C=np.array(d.C[:s]), E5=np.array(d.E5), E3=np.array(d.E3), q=8)
    raise ValueError("erk_oracle: method 'dopri45' or 'dop853', not %r" % (method,))


def _rhs(gm, p, columns, sens, use_c):
    """f(t, z) on the wavefront's elements z = [y (n), S[:, columns] row-major (n, c)]: the generated right-hand side of
    the full augmented system with the other columns held at zero (the columns are coupled through the state only)."""
    n, k = gm.n_vars, gm.n_sens
    if not sens:
        fw = _wrap_c(gm.c_library().sbm_rhs, n, p) if use_c else _wrap(gm.model, n, p)
        return lambda t, z: fw(z, t).copy()
    N = n + n * k
    fw = _wrap_c(gm.c_library().sbm_sens_rhs, N, p) if use_c else _wrap(gm.sens_model, N, p)
    cols = np.asarray(columns, dtype=int)
    pos = np.concatenate([np.arange(n), (n + np.arange(n)[:, None] * k + cols[None, :]).ravel()])
    full = np.zeros(N)

    def f(t, z):
        full[pos] = z
        return fw(full, t)[pos]
    return f


def _norm(r, n, c, with_state):
    """sqrt(max(state sum, worst column sum) / n) of the float32 ratios r (n + n c,), in float32"""
    sq = r * r
    sq = np.where(np.isnan(sq), F32(np.inf), sq)
    m = F32(0.0)
    if with_state:
        m = np.sum(sq[:n], dtype=F32)
    if c:
        m = max(m, np.max(np.sum(sq[n:].reshape(n, c), axis=0, dtype=F32)))
    return np.sqrt(F32(m) * (F32(1.0) / F32(n)))


def _side(a, b):
    a, b = abs(float(a)), abs(float(b))
    if a == b:
        return 1.0
    if a == 0.0 or b == 0.0:
        return float('inf')
    return max(a / b, b / a)


def integrate(gm, p, t_out, method='dopri45', rtol=1e-9, atol=1e-18, h0=0.0, max_steps=0, columns=None, sens=True,
              init_conditions=None, use_c=True, noise=None, mutate=None):
    """One wavefront.  ``columns``: the sensitivity columns it integrates (default: all).  ``init_conditions``: the full
    [y0; S0] (n + n k; n with ``sens=False``), zeros by default.  Returns dict(Z (len(t_out), n + n c): [y | S[:, columns]]
    row-major, status, n_acc, n_rej, n_try, err_margin, land_margin, exit_margins (growing, smooth, horizon) or None,
    errs: err of every attempt)."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError("erk_oracle: unknown mutation %r" % (mutate,))
    n, k = gm.n_vars, gm.n_sens
    tb = tableau(method)
    q = tb['q']
    dop = method == 'dop853'
    A, B, C = tb['A'].copy(), tb['B'].copy(), tb['C']
    s = len(C)
    if dop:
        E5, E3 = tb['E5'].copy(), tb['E3'].copy()
    else:
        E = tb['E'].copy()
    if mutate == 'A65':
        A[5, 4] *= 1.0 + 1e-9
    if mutate == 'E5' and not dop:
        E[4] *= 1.0 + 1e-3
    if mutate in ('E5', 'E3') and dop:
        (E5 if mutate == 'E5' else E3)[8] *= 1.0 + 1e-3
    land = 1.0 if mutate == 'landing' else 1.01
    fac_lo, fac_hi = (F32(1.0) / F32(3.0), F32(6.0)) if dop else (F32(0.2), F32(10.0))
    if mutate == 'fac_max':
        fac_hi = F32(5.0)
    fac_bad = fac_lo
    expo = F32(-1.0 / q)

    p = np.ascontiguousarray(p, dtype=np.float64)
    cols = list(range(k)) if columns is None else [int(c) for c in columns]
    if not sens:
        cols = []
    c = len(cols)
    f0 = _rhs(gm, p, cols, sens, use_c)
    rng = None
    a_rhs = a_err = 0.0
    if noise is not None:
        rng = np.random.default_rng(noise[0])
        a_rhs, a_err = float(noise[1]), float(noise[2])

    def f(t, z, fn=None):
        d = (fn or f0)(t, z)
        if rng is not None:
            d = d * (1.0 + a_rhs * rng.uniform(-1.0, 1.0, d.shape))
        return d

    t_out = np.asarray(t_out, dtype=float)
    if init_conditions is None:
        z = np.zeros(n + n * c)
        init_full = None
    else:
        init_full = np.array(init_conditions, dtype=float)
        if sens:
            S0 = init_full[n:].reshape(n, k)
            z = np.concatenate([init_full[:n], S0[:, cols].ravel()])
        else:
            z = init_full[:n].copy()
    with_state = mutate != 'state_norm'

    t = float(t_out[0])
    t_end = float(t_out[-1])
    span = t_end - t
    span = span if span > 0.0 else 1.0
    k1 = f(t, z)
    h = float(h0)
    if not h > 0.0:
        zi, ki, fi = z, k1, None
        if mutate == 'hinit_all' and sens:
            # the error: hinit sums over every column of S, not the chunk's
            fi = _rhs(gm, p, list(range(k)), True, use_c)
            zi = np.zeros(n + n * k) if init_full is None else init_full
            ki = f(t, zi, fi)
        sk = atol + rtol * np.abs(zi)
        dnf, dny = float(np.sum((ki / sk) ** 2)), float(np.sum((zi / sk) ** 2))
        h = 1e-6 if (dnf <= 1e-10 or dny <= 1e-10) else np.sqrt(dny / dnf) * 0.01
        h = min(h, span)
        k2 = f(t + h, zi + h * ki, fi)
        der2 = np.sqrt(float(np.sum(((k2 - ki) / sk) ** 2))) / h
        der12 = max(abs(der2), np.sqrt(dnf))
        h1 = max(1e-6, abs(h) * 1e-3) if der12 <= 1e-15 else (0.01 / der12) ** (1.0 / q)
        h = float(min(100.0 * h, h1, span))
        if not h > 0.0:
            h = 1e-6

    early = max_steps < 0
    budget = max_steps if max_steps > 0 else (-max_steps if max_steps < 0 else 1000000)
    n_try = n_acc = n_rej = 0
    status = SBM_OK
    failed = False
    h_mark, rej_mark = F32(0.0), 0
    err_margin = land_margin = float('inf')
    exit_m = [float('inf')] * 3 if early else None
    errs = []
    Z = np.full((len(t_out), n + n * c), np.nan)
    K = np.zeros((s + 1, n + n * c))
    t_prev_out = t
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for io, target in enumerate(t_out):
            target = float(target)
            while not failed and t < target:
                if (n_try > budget) if mutate == 'budget' else (n_try >= budget):
                    status, failed = SBM_MAX_STEPS, True
                    break
                if early and n_try >= 512 and n_try % 256 == 0:
                    hf = F32(h)
                    growing = hf > F32(1.5) * h_mark
                    smooth = n_rej - rej_mark < 3
                    lhs, rhs = t_end - t, 1.5 * float(budget - n_try) * h
                    exit_m[0] = min(exit_m[0], _side(hf, F32(1.5) * h_mark))
                    exit_m[1] = min(exit_m[1], _side(n_rej - rej_mark, 2.5))
                    exit_m[2] = min(exit_m[2], _side(lhs, rhs))
                    h_mark, rej_mark = hf, n_rej
                    if not growing and not smooth and lhs > rhs:
                        status, failed = SBM_MAX_STEPS, True
                        break
                n_try += 1
                hs, last = h, False
                edge = t + land * hs
                gap = target - t_prev_out
                land_margin = min(land_margin, abs(edge - target) / gap if gap > 0.0 else float('inf'))
                if edge >= target:
                    hs, last = target - t, True
                K[0] = k1
                for i in range(1, s):
                    K[i] = f(t + C[i] * hs, z + hs * (A[i, :i] @ K[:i]))
                zn = z + hs * (B @ K[:s])
                sc = atol + rtol * np.maximum(np.abs(z), np.abs(zn))
                rsc = F32(1.0) / sc.astype(F32)
                hsf = abs(F32(hs))
                if dop:
                    n5 = _norm((E5[:s] @ K[:s]).astype(F32) * rsc, n, c, with_state)
                    n3 = _norm((E3[:s] @ K[:s]).astype(F32) * rsc, n, c, with_state)
                    den = n5 * n5 + F32(0.01) * n3 * n3
                    err = hsf * (n5 * n5 / np.sqrt(den) if den > 0 else F32(0.0))
                    finite = bool(err == err and err < F32(3.0e38) and n3 == n3 and n3 < F32(3.0e38))
                else:
                    K[s] = f(t + hs, zn)
                    err = hsf * _norm((E @ K).astype(F32) * rsc, n, c, with_state)
                    finite = bool(err == err and err < F32(3.0e38))
                if rng is not None:
                    err = F32(err * F32(1.0 + a_err * rng.uniform(-1.0, 1.0)))
                errs.append(float(err))
                if finite:
                    err_margin = min(err_margin, abs(float(err) - 1.0))
                    fac = F32(0.9) * np.exp2(expo * np.log2(max(F32(err), F32(1e-30))), dtype=F32)
                    fac = min(fac_hi, max(fac_lo, F32(fac)))
                else:
                    fac = fac_bad
                if finite and err <= F32(1.0):
                    n_acc += 1
                    t = target if last else t + hs
                    z = zn
                    hn = hs * float(fac)
                    h = (hn if mutate == 'clip_max' else max(hn, h)) if last else hn
                    k1 = f(t, z) if dop else K[s].copy()
                else:
                    n_rej += 1
                    h = hs * float(min(fac, F32(1.0)))
                    if not h > 1e-14 * max(abs(t), 1e-3):
                        status, failed = (SBM_STEP_UNDERFLOW if finite else SBM_NON_FINITE), True
                    elif not dop:
                        k1 = f(t, z)
            if failed:
                break
            Z[io] = z
            t_prev_out = target
    return dict(Z=Z, status=status, n_acc=n_acc, n_rej=n_rej, n_try=n_try, err_margin=err_margin, land_margin=land_margin,
                exit_margins=None if exit_m is None else tuple(exit_m), errs=np.array(errs), columns=cols)


def integrate_chunks(gm, p, t_out, chunks, **kw):
    """A column-chunked kernel: one run per chunk of ``chunks`` (lists of columns that together are 0 .. k - 1).  Returns
    dict(Z (len(t_out), n + n k) = [Y of chunk 0 | S in the layout of calc_jacobian], status, n_acc, n_rej: the largest
    over the chunks; n_try: per chunk; err_margin, land_margin: the smallest; exit_margins; runs: the chunks' own results)."""
    n, k = gm.n_vars, gm.n_sens
    runs = [integrate(gm, p, t_out, columns=cols, **kw) for cols in chunks]
    assert sorted(c for cols in chunks for c in cols) == list(range(k)), "the chunks are a partition of the columns"
    Z = np.zeros((len(t_out), n + n * k))
    Z[:, :n] = runs[0]['Z'][:, :n]
    S = Z[:, n:].reshape(len(t_out), n, k)
    for cols, r in zip(chunks, runs):
        S[:, :, cols] = r['Z'][:, n:].reshape(len(t_out), n, len(cols))
    ex = None
    if runs[0]['exit_margins'] is not None:
        ex = tuple(min(r['exit_margins'][i] for r in runs) for i in range(3))
    return dict(Z=Z, status=max(r['status'] for r in runs), n_acc=max(r['n_acc'] for r in runs),
                n_rej=max(r['n_rej'] for r in runs), n_try=[r['n_try'] for r in runs],
                err_margin=min(r['err_margin'] for r in runs), land_margin=min(r['land_margin'] for r in runs),
                exit_margins=ex, runs=runs)


def header_sizes(gm):
    return tuple(int(re.search(r'static constexpr int %s = (\d+);' % key, gm.hip_source).group(1)) for key in ('NV', 'NK'))


def chunk_columns(gm, kernel):
    """The column sets of the wavefronts of one trajectory, per kernel: 'per_wave', 'row_lane', 'packed' hold every column in
    one wavefront; 'RG0' / 'RG1' / 'RG2' (the row-group splits: DOPRI45 and RK4 / small batches / DOP853) are RG_C * RG_CPL
    columns wide, read from the generated header as GeneratedModel.rowgroup_chunks reads RG_NCH; 'mfma' is 16 CT columns
    wide, CT = min(ceil(NK / 16), max(1, 12 / (4 ceil(NV / 16)))) (SbmMfmaPlan, csrc/sbm_sens_mfma.hpp)."""
    nv, nk = header_sizes(gm)
    if kernel in ('per_wave', 'row_lane', 'packed'):
        return [list(range(nk))]
    if kernel in ('RG0', 'RG1', 'RG2'):
        src = gm.hip_source
        m = re.search(r'struct %s \{.*?RG_C = (\d+), RG_CPL = (\d+).*?RG_NCH = (\d+)' % kernel, src, re.S)
        if m is None:
            alias = re.search(r'using %s = (RG\d);' % kernel, src)
            if alias is None:
                raise ValueError("%s has no row split %s" % (gm.name, kernel))
            return chunk_columns(gm, alias.group(1))
        width, nch = int(m.group(1)) * int(m.group(2)), int(m.group(3))
        if nch == 1:
            return [list(range(nk))]
    elif kernel == 'mfma':
        rt = (nv + 15) // 16
        ct = min((nk + 15) // 16, max(1, 12 // (4 * rt)))
        width = 16 * ct
        nch = (nk + width - 1) // width
    else:
        raise ValueError("erk_oracle.chunk_columns: unknown kernel %r" % (kernel,))
    out = [list(range(b, min(b + width, nk))) for b in range(0, nk, width)]
    assert len(out) == nch, (gm.name, kernel, width, nch)
    return out
