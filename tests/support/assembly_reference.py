"""TEST INFRASTRUCTURE -- the assembly kernel's arithmetic restated in extended precision.

What ``k_assemble`` (csrc/sbm_assemble.hpp) returns for one parameter vector -- simulations per row, model Jacobian, scale
factors and their gradient, residuals, Jacobian, sum of squares, gradient -- written from the formulas of include/sbm.h
(sbm_project_desc / sbm_loss_desc) and oracle/project_oracle.py, in numpy ``longdouble`` (64-bit mantissa) or, where the
platform's long double is no wider than a double, in mpmath at 40 digits.  Nothing here is taken from the kernel: no
row lanes, no partial sums, no caches -- plain sums over the rows of a group.

Every output comes as a triple

    value   the formula in wide arithmetic
    scale   the SAME formula with every term replaced by its absolute value and every subtraction by an addition
            (a sum: sum |terms|; a product: the product of the scales; a quotient by a positive quantity: scale / value;
            log x: |log x| + scale(x) / |x|; exp x: exp(x) (1 + scale(x)) -- the first-order propagation of an error
            that is ``count x u x scale`` in the argument).  Errors are judged as |gpu - ref| / scale, so a cancelling
            sum can neither inflate nor hide them.
    n       the length of the longest sum behind the entry: the rows of the group for a scale factor, its gradient and
            everything of a row that carries one (1 for a row without), all rows (R + priors) for ``norms`` and ``grad``.

The bound
---------
A sum of n floating-point terms, added in ANY order, is within (n - 1) u sum |terms| of the exact sum of those terms
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; u = 2^-53, first order in u).  Every other
operation of a formula -- a product, a quotient, the final division by sigma -- adds one rounding u relative to its own
result, which the scale bounds from above; log and exp of the device library count as two (1 ulp = 2 u, what the
OpenCL / HIP double-precision tables state for both).  An output's constant is therefore

    C(n) = n + K,      K = the number of roundings of the formula that are not additions of its longest sum,

counted along the formula, inputs first (a term of the sum counts once: all terms are built the same way).  Where a
formula holds several sums of the same length side by side (sde and sds of a scale factor, jde and jds of its
gradient) n is counted ONCE: the fully rigorous constant would multiply n by the number of such sums (up to 4 for the
square loss's dB); the tests use the tighter form C(n) = n + K on purpose.

  square loss                                                             K
    w = 1 / (sigma sigma)                                                  2
    sde term s d w, sds term s s w                                 2 + 2 (+ w: 2)
    B = sde / sds                                              6 + 1  ->   K_sf = 7
    r = (B s - d) / sigma                                         + 3  ->  K_R = 10
    sf-prior row (log B - m) / sigma_p                     + 2 + 1 + 1 ->  K_R (prior) = 11  (K_R = 11 is used for all rows)
    jde term Jm d w, jds term Jm s w                               2 + 2
    dB = jde / sds - 2 sde jds / (sds sds)           K_sf + 4 + 1 + 4  ->  K_dB = 16     (the factor 2 is exact)
    J = (B Jm + s dB) / sigma                              K_dB + 1 + 3 -> K_J = 20
    sf-prior row (dB / B) / sigma_p                        K_dB + K_sf + 2 <= K_J + 5: K_J = 25 is used for all rows
  log loss
    w = d d / (sigma sigma)                                                3
    sde term (log d - log s) w, sds term w                     2 + 2 + 1 + 1 (+ w: 3) = 9
    B = exp(sde / sds)                                        9 + 1 + 2 -> K_sf = 12
    r = (log(B s) - log d) / sigma                     + 1 + 2 + 2 + 1 + 1 -> K_R = 19
    sf-prior row                                              + 2 + 1 + 1 (less)
    jde term Jm d d / (sigma sigma s)                                      5
    dB = -B jde / sds                                        K_sf + 5 + 2 -> K_dB = 19
    J = (Jm / s + dB / B) / sigma                    K_dB + K_sf + 1 + 1 + 1 + 1 -> K_J = 35
  both
    norms = sum r^2          n = R + priors; a term r r carries twice r's roundings and its own: K = 2 (n_g + K_R) + 1,
                             n_g the longest group (the residuals' own sums are further roundings of THIS formula)
    grad_c = sum J_rc r_r    n = R + priors;  K = (n_g + K_J) + (n_g + K_R) + 1

The mapping half (``map_reference``) restates step 1 and pass A: sims from the sampled states for 'direct', 'sum' and
custom rows, and Jmodel[r][c] = exp(theta_c) sum_{m: pmap[e][m] = c, sens_col[m] >= 0} sum_k w_k S[var_k][sens_col[m]],
custom values and weights evaluated by mpmath from the sympy expression (never from the compiled program).
Only tests/ may import this."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
WIDE = np.finfo(np.longdouble).nmant >= 63      # the x87 format; elsewhere everything below runs on mpmath numbers
SQUARE, LOG = 0, 1
K_SF = {SQUARE: 7, LOG: 12}
K_R = {SQUARE: 11, LOG: 19}
K_DB = {SQUARE: 16, LOG: 19}
K_J = {SQUARE: 25, LOG: 35}


def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def to_mpf(x):
    """exact mpmath value of a float, a longdouble (head + tail, each a double) or an mpf"""
    m = _mp()
    if isinstance(x, np.longdouble):
        hi = float(x)
        if not np.isfinite(hi):
            return m.mpf(hi)
        return m.mpf(hi) + m.mpf(float(x - np.longdouble(hi)))
    return m.mpf(x)


class _Arith(object):
    """The two number systems: numpy longdouble, or object arrays of mpmath.mpf at 40 digits."""

    def __init__(self, use_mpmath):
        self.mp = bool(use_mpmath)
        if self.mp:
            m = _mp()
            self._log, self._exp = np.frompyfunc(m.log, 1, 1), np.frompyfunc(m.exp, 1, 1)
            self._conv = np.frompyfunc(lambda x: m.mpf(float(x)), 1, 1)

    def arr(self, a):
        a = np.asarray(a, dtype=np.float64)
        if not self.mp:
            return a.astype(np.longdouble)
        return self._conv(a) if a.size else a.astype(object)

    def zeros(self, shape):
        if not self.mp:
            return np.zeros(shape, dtype=np.longdouble)
        out = np.empty(shape, dtype=object)
        out[...] = _mp().mpf(0)
        return out

    def log(self, a):
        return self._log(a) if self.mp else np.log(a)

    def exp(self, a):
        return self._exp(a) if self.mp else np.exp(a)

    def sum(self, a, axis=None):
        a = np.asarray(a)
        if a.size == 0:
            return self.zeros(() if axis is None else tuple(s for i, s in enumerate(a.shape) if i != axis))
        return np.sum(a, axis=axis)


def arithmetic(use_mpmath=None):
    """longdouble where it is wide (asserted), mpmath otherwise or on request."""
    if use_mpmath is None:
        use_mpmath = not WIDE
    if not use_mpmath:
        assert np.finfo(np.longdouble).nmant >= 63, "numpy longdouble is not an extended format here: use mpmath"
    return _Arith(use_mpmath)


def assemble_reference(sims, Jm, data, sigma, group, n_groups, loss=SQUARE, compat=0, plain=None, theta=None,
                       prior=None, sf_prior=None, use_mpmath=None):
    """One vector.  sims [R], Jm [R][q] or None, the row tables data / sigma / group [R] (group -1: no scale factor),
    plain [R] or None (1: (s - d) / sigma even under the log loss), prior = (idx, mean, sigma) parameter-prior rows
    (needs theta [q]), sf_prior = (group, mean, sigma) scale-factor-prior rows.  Returns {name: (value, scale, n)} for
    'sf' [G], 'R_out' [RT], 'norms' [] and, with Jm, 'sf_grad' [G][q], 'J' [RT][q], 'grad' [q]; value and scale in the
    wide type, n integer arrays of the value's shape.  The caller decides what a non-finite simulation means: the
    formulas are evaluated as they stand."""
    ar = arithmetic(use_mpmath)
    s, d, sg = ar.arr(sims), ar.arr(data), ar.arr(sigma)
    grp = np.asarray(group, dtype=int)
    R, G = len(grp), int(n_groups)
    pl = np.zeros(R, dtype=bool) if plain is None else np.asarray(plain).astype(bool)
    p_idx, p_mean, p_sig = (np.zeros(0, int), np.zeros(0), np.zeros(0)) if prior is None else prior
    f_grp, f_mean, f_sig = (np.zeros(0, int), np.zeros(0), np.zeros(0)) if sf_prior is None else sf_prior
    p_idx, f_grp = np.asarray(p_idx, dtype=int), np.asarray(f_grp, dtype=int)
    NPR, NSP = len(p_idx), len(f_grp)
    RT = R + NPR + NSP
    q = None if Jm is None else np.asarray(Jm).shape[1]
    J_in = None if Jm is None else ar.arr(Jm)
    aJ = None if Jm is None else abs(J_in)
    logloss = loss == LOG
    one = ar.arr(1.0)

    B, scB, sde, a_sde, sds = ar.zeros(G), ar.zeros(G), ar.zeros(G), ar.zeros(G), ar.zeros(G)
    n_g = np.zeros(G, dtype=int)
    dB = sc_dB = None
    if q is not None:
        dB, sc_dB = ar.zeros((G, q)), ar.zeros((G, q))
    for g in range(G):
        sel = grp == g
        n_g[g] = int(sel.sum())
        sv, dv, sv_sg = s[sel], d[sel], sg[sel]
        if logloss:
            w = dv * dv / (sv_sg * sv_sg)
            sde[g] = ar.sum((ar.log(dv) - ar.log(sv)) * w)
            a_sde[g] = ar.sum((abs(ar.log(dv)) + abs(ar.log(sv))) * w)
            sds[g] = ar.sum(w)
            B[g] = ar.exp(sde[g] / sds[g])
            scB[g] = B[g] * (one + a_sde[g] / sds[g])
            if q is not None:
                wj = (w / sv)[:, None]
                jde, a_jde = ar.sum(J_in[sel] * wj, axis=0), ar.sum(aJ[sel] * abs(wj), axis=0)
                dB[g] = -B[g] * jde / sds[g]
                sc_dB[g] = scB[g] * a_jde / sds[g]
        else:
            w = one / (sv_sg * sv_sg)
            sde[g] = ar.sum(sv * dv * w)
            a_sde[g] = ar.sum(abs(sv * dv) * w)
            sds[g] = ar.sum(sv * sv * w)
            B[g] = sde[g] / sds[g]
            scB[g] = a_sde[g] / sds[g]
            if q is not None:
                jde, a_jde = ar.sum(J_in[sel] * (dv * w)[:, None], axis=0), ar.sum(aJ[sel] * abs(dv * w)[:, None], axis=0)
                jds, a_jds = ar.sum(J_in[sel] * (sv * w)[:, None], axis=0), ar.sum(aJ[sel] * abs(sv * w)[:, None], axis=0)
                dB[g] = jde / sds[g] - 2 * sde[g] * jds / (sds[g] * sds[g])
                sc_dB[g] = a_jde / sds[g] + 2 * a_sde[g] * a_jds / (sds[g] * sds[g])

    has = grp >= 0
    gi = np.where(has, grp, 0)
    Br = np.where(has, B[gi], one) if G else np.broadcast_to(one, (R,)).copy()
    scBr = np.where(has, scB[gi], one) if G else np.broadcast_to(one, (R,)).copy()
    n_row = np.where(has, n_g[gi], 1) if G else np.ones(R, dtype=int)
    logrow = np.full(R, logloss) & ~pl

    res, sc_res = ar.zeros(RT), ar.zeros(RT)
    n_res = np.ones(RT, dtype=int)
    n_res[:R] = n_row
    lin = ~logrow
    res[:R][lin] = ((Br * s - d) / sg)[lin]
    sc_res[:R][lin] = ((scBr * abs(s) + abs(d)) / abs(sg))[lin]
    if logrow.any():
        a = (Br * s)[logrow]
        sa = (scBr * abs(s))[logrow]
        res[:R][logrow] = (ar.log(a) - ar.log(d[logrow])) / sg[logrow]
        sc_res[:R][logrow] = (abs(ar.log(a)) + sa / abs(a) + abs(ar.log(d[logrow]))) / abs(sg[logrow])
    if NPR:
        th, pm, ps = ar.arr(theta)[p_idx], ar.arr(p_mean), ar.arr(p_sig)
        res[R:R + NPR] = (th - pm) / ps
        sc_res[R:R + NPR] = (abs(th) + abs(pm)) / abs(ps)
    if NSP:
        fm, fs = ar.arr(f_mean), ar.arr(f_sig)
        res[R + NPR:] = (ar.log(B[f_grp]) - fm) / fs
        sc_res[R + NPR:] = (abs(ar.log(B[f_grp])) + scB[f_grp] / abs(B[f_grp]) + abs(fm)) / abs(fs)
        n_res[R + NPR:] = n_g[f_grp]
    out = {'sf': (B, scB, n_g.copy()), 'R_out': (res, sc_res, n_res),
           'norms': (ar.sum(res * res), ar.sum(sc_res * sc_res), np.asarray(RT))}
    if q is None:
        return out

    J, sc_J = ar.zeros((RT, q)), ar.zeros((RT, q))
    if logloss:
        rel = (dB / B[:, None], sc_dB * scB[:, None] / (B * B)[:, None]) if G else (ar.zeros((0, q)),) * 2
        body = np.where(logrow[:, None], J_in / s[:, None], J_in)
        sc_body = np.where(logrow[:, None], aJ / abs(s)[:, None], aJ)
        if G:
            body = body + np.where((has & logrow)[:, None], rel[0][gi], 0 * one)
            sc_body = sc_body + np.where((has & logrow)[:, None], rel[1][gi], 0 * one)
    else:
        rel = (dB / B[:, None], sc_dB * scB[:, None] / (B * B)[:, None]) if G else (ar.zeros((0, q)),) * 2
        body, sc_body = J_in * Br[:, None], aJ * scBr[:, None]
        if G:
            body = body + np.where(has[:, None], s[:, None] * dB[gi], 0 * one)
            sc_body = sc_body + np.where(has[:, None], abs(s)[:, None] * sc_dB[gi], 0 * one)
    if not compat:
        body, sc_body = body / sg[:, None], sc_body / abs(sg)[:, None]
    J[:R], sc_J[:R] = body, sc_body
    for k in range(NPR):
        if not compat:
            J[R + k, p_idx[k]] = one / ar.arr(p_sig)[k]
            sc_J[R + k, p_idx[k]] = abs(J[R + k, p_idx[k]])
    for k in range(NSP):
        row, sc_row = rel[0][f_grp[k]], rel[1][f_grp[k]]
        if not compat:
            row, sc_row = row / ar.arr(f_sig)[k], sc_row / abs(ar.arr(f_sig)[k])
        J[R + NPR + k], sc_J[R + NPR + k] = row, sc_row
    n_J = np.broadcast_to(n_res[:, None], (RT, q)).copy()
    out['sf_grad'] = (dB, sc_dB, np.broadcast_to(n_g[:, None], (G, q)).copy())
    out['J'] = (J, sc_J, n_J)
    out['grad'] = (ar.sum(J * res[:, None], axis=0), ar.sum(sc_J * sc_res[:, None], axis=0), np.full(q, RT))
    return out


def bound_constants(loss, n_groups_rows):
    """{output: K}: the further roundings of every output's formula (module docstring).  ``n_groups_rows``: the rows of
    the largest scale-factor group (0 without groups), which norms and grad inherit through their terms."""
    ng = max(int(n_groups_rows), 1)
    return {'sf': K_SF[loss], 'R_out': K_R[loss], 'sf_grad': K_DB[loss], 'J': K_J[loss],
            'norms': 2 * (ng + K_R[loss]) + 1, 'grad': (ng + K_J[loss]) + (ng + K_R[loss]) + 1}


def normalised_error(got, value, scale, bound):
    """max |got - value| / (scale x bound) over the entries; ``bound`` = C(n) u, scalar or per entry.  An entry whose
    scale is zero must be matched exactly.  Any NaN or inf that is not at the same place (and, for inf, of the same sign)
    in both arrays gives inf: nothing that is not a finite number is ever within a bound."""
    got = np.asarray(got, dtype=np.float64)
    val = np.asarray(value)
    if got.shape != val.shape:
        raise ValueError("normalised_error: shapes %s and %s" % (got.shape, val.shape))
    if got.size == 0:
        return 0.0
    vf = val.astype(np.float64)
    bad_g, bad_v = ~np.isfinite(got), ~np.isfinite(vf)
    if (bad_g != bad_v).any():
        return float('inf')
    both = bad_g & bad_v
    if both.any():
        g, v = got[both], vf[both]
        if (np.isnan(g) != np.isnan(v)).any() or (g[~np.isnan(g)] != v[~np.isnan(v)]).any():
            return float('inf')
    ok = ~both
    if not ok.any():
        return 0.0
    if val.dtype == object:
        m = _mp()
        wide_got = np.frompyfunc(lambda x: m.mpf(float(x)), 1, 1)(got)
    else:
        wide_got = got.astype(val.dtype)
    with np.errstate(invalid='ignore'):
        err = np.asarray(abs(wide_got - val))[ok]
    den = (np.asarray(scale) * np.broadcast_to(np.asarray(bound, dtype=np.float64), val.shape))[ok]
    zero = np.asarray(den == 0)
    if (np.asarray(err != 0) & zero).any():
        return float('inf')
    if zero.all():
        return 0.0
    ratio = (err[~zero] / den[~zero]).astype(np.float64)
    worst = float(np.max(ratio))
    return worst if worst == worst else float('inf')


def check_outputs(got, ref, loss, what=''):
    """{output: fraction of its bound}: every output of ``got`` (name -> float64 array) against the reference dict of
    assemble_reference, bound C(n) u per entry."""
    ng = int(ref['sf'][2].max()) if ref['sf'][2].size else 0
    K = bound_constants(loss, ng)
    out = {}
    for name, arr in got.items():
        if arr is None or name not in ref:
            continue
        value, scale, n = ref[name]
        out[name] = normalised_error(np.asarray(arr).reshape(np.shape(value)), value, scale, (n + K[name]) * U)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the mapping half: step 1 and pass A
# ------------------------------------------------------------------------------------------------------------------
def custom_row_reference(expr, symbols, y_values, t):
    """(g, [dg/dy_k]) of a sympy expression in ``symbols`` (the row's variables, in the row's order) and the real symbol
    t, by mpmath at 40 digits; y_values[k] the value of symbols[k].  d|x| = sign(x) with sign(0) = 0."""
    import sympy
    m = _mp()
    syms = list(symbols)
    key = (expr, tuple(syms))
    if key not in _LAMBDIFIED:
        tsym = sympy.Symbol('t', real=True)
        mods = [{'sign': lambda x: m.sign(x), 'Abs': lambda x: abs(x)}, 'mpmath']
        _LAMBDIFIED[key] = [sympy.lambdify(syms + [tsym], e, modules=mods) for e in [expr] + [sympy.diff(expr, sy) for sy in syms]]
    args = [m.mpf(float(v)) for v in y_values] + [m.mpf(float(t))]
    fs = _LAMBDIFIED[key]
    return m.mpf(fs[0](*args)), [m.mpf(f(*args)) for f in fs[1:]]


_LAMBDIFIED = {}


def map_reference(desc, Y, S, theta, use_mpmath=None):
    """One vector.  desc: the descriptor arrays (tests/support/descriptor_builder.py) with, for custom rows,
    desc['row_expr'][r] = (sympy expression, variable names of the model) or None; Y [E][n_t][NV] and S [E][n_t][NV][NK]
    the sampled states and sensitivities per experiment (padded grids), theta [q].
    Returns {'sims': (value [R], scale [R], n [R]), 'Jmodel': (value [R][q], scale, n)}; n = the number of terms of the
    entry's sum (variables x model parameters reading the slot, at least 1)."""
    ar = arithmetic(use_mpmath)
    m = _mp()
    R, q = int(desc['n_rows']), int(desc['n_project_params'])
    NP = len(desc['sens_col'])
    pmap = np.asarray(desc['pmap']).reshape(-1, NP)
    sims, sc_s, n_s = ar.zeros(R), ar.zeros(R), np.ones(R, dtype=int)
    Jm, sc_J, n_J = ar.zeros((R, q)), ar.zeros((R, q)), np.ones((R, q), dtype=int)
    eth = ar.exp(ar.arr(theta))
    conv = (lambda x: x) if ar.mp else (lambda x: np.longdouble(m.nstr(x, 30)))
    exprs = desc.get('row_expr')
    for r in range(R):
        e, ti = int(desc['row_exp'][r]), int(desc['row_tidx'][r])
        vars_ = [int(v) for v in desc['row_vars'][desc['row_var_off'][r]:desc['row_var_off'][r + 1]]]
        y = Y[e, ti]
        if exprs is not None and exprs[r] is not None:
            expr, symbols = exprs[r]
            g, w = custom_row_reference(expr, symbols, [y[v] for v in vars_], desc['row_time'][r])
            sims[r], sc_s[r] = conv(g), abs(conv(g))
            w = [conv(x) for x in w]
        else:
            yv = ar.arr([y[v] for v in vars_])
            sims[r], sc_s[r], n_s[r] = ar.sum(yv), ar.sum(abs(yv)), max(len(vars_), 1)
            w = [ar.arr(1.0)] * len(vars_)
        if S is None:
            continue
        for c in range(q):
            ms = [k for k in np.flatnonzero(pmap[e] == c) if desc['sens_col'][k] >= 0]
            if not ms:
                continue
            acc, sacc = ar.arr(0.0), ar.arr(0.0)
            for k in ms:
                col = ar.arr(S[e, ti][vars_, int(desc['sens_col'][k])])
                for wk, sk in zip(w, col):
                    acc, sacc = acc + wk * sk, sacc + abs(wk * sk)
            Jm[r, c], sc_J[r, c], n_J[r, c] = eth[c] * acc, eth[c] * sacc, max(len(ms) * len(vars_), 1)
    return {'sims': (sims, sc_s, n_s), 'Jmodel': (Jm, sc_J, n_J)}
