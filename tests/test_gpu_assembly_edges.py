"""The assembly kernel (k_assemble, csrc/sbm_assemble.hpp) at every edge of its layout, against the wide reference of
tests/support/assembly_reference.py -- plain sums in numpy longdouble from the formulas of include/sbm.h and
oracle/project_oracle.py, errors normalised by each output's scale and bounded by C(n) u (derived there).

Direct mode (sbm_loss_eval_host, no integrator): tests/support/assembly_cases.py lists the shapes -- q at every change of
the row-lane count and of the number of column passes, R below / at / above the row lanes and the block, scale-factor
groups contiguous, interleaved, with gaps, on one row lane, split around another group, random; both losses, both
reference_compat values, scale-factor priors, plain rows; V = 3 with a NaN simulation in vector 1.
Integrated path (sbm_project_load on hand-built descriptors, tests/support/descriptor_builder.py, RK4 with a forced kernel
variant): 300 experiments with grids of unequal length, parameter maps with 0 / 1 / 2 / 4 readers per slot that change from
experiment to experiment, rows not sorted by experiment, 'direct' / 'sum' / custom rows mixed, every opcode of the
custom-observable interpreter.  sims and Jmodel are checked against the mapping of per-experiment integrations
(sbm_sens_batch_host) with the measured input uncertainty; everything downstream tightly, from the sims and Jmodel the
call itself returned.  docs/history.md records the measured figures."""
import ctypes

import numpy as np
import pytest

from tests.support import assembly_cases as ac
from tests.support import assembly_reference as ar
from tests.support import descriptor_builder as db

pytestmark = pytest.mark.gpu

U = ar.U
NON_FINITE = 2        # include/sbm.h: SBM_NON_FINITE
_worst = {}           # output -> (fraction of bound, case): the table of the last test
_ran = set()          # direct-mode cases that ran to their end


def _note(frac, what):
    for k, f in frac.items():
        if f > _worst.get(k, (-1.0, ''))[0]:
            _worst[k] = (f, what)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------
# direct mode
# ------------------------------------------------------------------------------------------------------------------
def loss_eval(c, sims, Jm, want=('J', 'sf', 'sf_grad', 'norms', 'status'), fill=7.0):
    """(rc, outputs) of sbm_loss_eval_host for the case's tables; outputs not wanted are passed as NULL, buffers are
    prefilled so that an unwritten entry shows"""
    from sysbio_modeling_amd import _lib
    lib, ctx = _lib.load_library(), _lib.default_context()
    sims = np.ascontiguousarray(sims, dtype=np.float64)
    V, R = sims.shape
    q = 0 if Jm is None else Jm.shape[2]
    NSP = len(c.sfp_group)
    nil_i, nil_d = ctypes.cast(None, _lib.c_int32_p), ctypes.cast(None, _lib.c_double_p)
    ip = lambda x: x.ctypes.data_as(_lib.c_int32_p) if x is not None and x.size else nil_i
    dp = lambda x: x.ctypes.data_as(_lib.c_double_p) if x is not None and x.size else nil_d
    keep = dict(data=np.ascontiguousarray(c.data[:R]), sigma=np.ascontiguousarray(c.sigma[:R]),
                group=np.ascontiguousarray(c.group[:R], dtype=np.int32),
                plain=None if c.plain is None else np.ascontiguousarray(c.plain[:R], dtype=np.int32),
                g=np.ascontiguousarray(c.sfp_group, dtype=np.int32), m=np.ascontiguousarray(c.sfp_mean), s=np.ascontiguousarray(c.sfp_sigma))
    desc = _lib.LossDesc(R, q, c.G, NSP, c.loss, c.compat, dp(keep['data']), dp(keep['sigma']), ip(keep['group']), ip(keep['plain']),
                         ip(keep['g']), dp(keep['m']), dp(keep['s']))
    Jm = None if Jm is None else np.ascontiguousarray(Jm, dtype=np.float64)
    out = {'R_out': np.full((V, R + NSP), fill)}
    if 'J' in want:
        out['J'] = np.full((V, R + NSP, max(q, 1)), fill)
    if 'sf' in want:
        out['sf'] = np.full((V, c.G), fill)
    if 'sf_grad' in want:
        out['sf_grad'] = np.full((V, c.G, max(q, 1)), fill)
    if 'norms' in want:
        out['norms'] = np.full((V,), fill)
    if 'status' in want:
        out['status'] = np.full((V,), -7, dtype=np.int32)
    p = lambda k: _lib.np_ptr(out[k]) if k in out and out[k].size else None
    rc = lib.sbm_loss_eval_host(ctx.handle, ctypes.byref(desc), V, _lib.np_ptr(sims), _lib.np_ptr(Jm) if Jm is not None else None,
                                p('R_out'), p('J'), p('sf'), p('sf_grad'), p('norms'), p('status'))
    msg = lib.sbm_last_error()
    return rc, out, (msg.decode() if msg else '')


def _expect_failed_vector(out, v, what):
    """What include/sbm.h states for a frame with a NaN (or, under the log loss, a non-positive) simulation."""
    assert np.all(np.isposinf(out['R_out'][v])), what
    assert np.all(np.isposinf(out['J'][v])), what
    assert np.all(np.isnan(out['sf'][v])) and np.all(np.isnan(out['sf_grad'][v])), what
    assert np.isposinf(out['norms'][v]) and out['status'][v] == NON_FINITE, what


def _check_vector(c, out, v, sims, what):
    ref = ar.assemble_reference(sims[v], c.Jm[v], c.data, c.sigma, c.group, c.G, c.loss, c.compat, plain=c.plain, sf_prior=c.sf_prior())
    got = {k: out[k][v] for k in ('R_out', 'J', 'sf', 'sf_grad')}
    got['norms'] = np.asarray(out['norms'][v])
    frac = ar.check_outputs(got, ref, c.loss)
    assert set(frac) == {'R_out', 'J', 'sf', 'sf_grad', 'norms'}
    print("%s vector %d: fraction of C(n) u  %s" % (what, v, '  '.join('%s %.3f' % kv for kv in sorted(frac.items()))))
    _note(frac, what)
    assert max(frac.values()) <= 1.0, (what, v, frac)
    assert out['status'][v] == 0


@pytest.mark.parametrize('shape', ac.SHAPES, ids=ac.IDS)
def test_direct_mode_edges(shape):
    """Vectors 0 and 2 within C(n) u of the wide reference; vector 1 (one NaN simulation) and, in the non-positive case,
    vector 2 as the header states for a failed frame; the failed vector's neighbours bit for bit what a call without
    the fault returns; the same call twice bitwise equal; a vector alone bitwise what it is inside the batch."""
    c = ac.Case(shape)
    assert (c.counts > 0).all() and len(c.counts) == c.G, "every group has rows"
    assert c.sims.shape == (3, c.R) and c.Jm.shape == (3, c.R, c.q)
    faulty = c.sims_with_faults()
    rc, clean, msg = loss_eval(c, c.sims, c.Jm)
    assert rc == 0, msg
    rc, out, msg = loss_eval(c, faulty, c.Jm)
    assert rc == 0, msg
    rc, again, msg = loss_eval(c, faulty, c.Jm)
    assert rc == 0, msg
    rc, alone, msg = loss_eval(c, c.sims[2:3], c.Jm[2:3])
    assert rc == 0, msg
    failed = [1, 2] if c.nonpositive else [1]
    for v in range(3):
        if v in failed:
            _expect_failed_vector(out, v, c.id)
        else:
            _check_vector(c, out, v, faulty, c.id)
            for k in clean:
                assert _same(out[k][v], clean[k][v]) if k != 'status' else out[k][v] == clean[k][v], (k, v, "changed by a neighbour's fault")
    _check_vector(c, clean, 1, c.sims, c.id + ' (clean call)')
    _check_vector(c, clean, 2, c.sims, c.id + ' (clean call)')
    for k in out:
        assert _same(out[k], again[k]) if k != 'status' else np.array_equal(out[k], again[k]), (k, "differs between two identical calls")
        assert _same(alone[k][0], clean[k][2]) if k != 'status' else alone[k][0] == clean[k][2], (k, "alone differs from inside the batch")
    _ran.add(c.id)


_NULLABLE = [s for s in ac.SHAPES if (s[0], s[1]) in ((3, 86), (64, 4), (257, 255), (1, 257))]


@pytest.mark.parametrize('shape', _NULLABLE, ids=[ac.case_id(s) for s in _NULLABLE])
def test_direct_mode_nullable_outputs(shape):
    """Jm NULL (residuals only, q = 0); J NULL with sf_grad wanted; sf, norms and status NULL: what is still returned is
    bit for bit what the full call returns, and nothing that was not asked for is touched."""
    c = ac.Case(shape)
    sims = c.sims_with_faults()
    rc, full, msg = loss_eval(c, sims, c.Jm)
    assert rc == 0, msg
    rc, res, msg = loss_eval(c, sims, None, want=('sf', 'norms', 'status'))
    assert rc == 0, msg
    for k in ('R_out', 'sf', 'norms'):
        assert _same(res[k], full[k]), k
    assert np.array_equal(res['status'], full['status'])
    rc, part, msg = loss_eval(c, sims, c.Jm, want=('sf_grad',))
    assert rc == 0, msg
    assert _same(part['sf_grad'], full['sf_grad']) and _same(part['R_out'], full['R_out'])
    rc, part, msg = loss_eval(c, sims, c.Jm, want=('J',))
    assert rc == 0, msg
    assert _same(part['J'], full['J']) and _same(part['R_out'], full['R_out'])
    # J or sf_grad without the model Jacobian is an argument error, not a launch
    rc, _, msg = loss_eval(c, sims, None, want=('sf', 'norms', 'status', 'sf_grad'))
    assert rc < 0 and 'model Jacobian' in msg, (rc, msg)


# -- dynamic LDS: q = 1, G = 0 needs 60 R + 4168 bytes (launch_assemble's formula: 2 R + 3 + 4 + 1 + 2 x 256 doubles,
# 2 R doubles and 7 R + 2 ints of row tables); the kernel's static LDS is 16 bytes (s_bad, padded to the dynamic block's
# alignment; scripts/isa_stats.sh on the built library); a workgroup of the MI355X has 160 KB.
LDS_LIMIT, LDS_STATIC = 160 * 1024, 16


def _lds_bytes(R):
    return 8 * (2 * R + 3 + 4 + 1 + 2 * 256) + 16 * R + 4 * (7 * R + 2)


LDS_LARGEST_R = (LDS_LIMIT - LDS_STATIC - _lds_bytes(0)) // 60


class _LdsCase(object):
    def __init__(self, R):
        rng = np.random.default_rng(R)
        self.R, self.q, self.G, self.loss, self.compat, self.plain = R, 1, 0, ac.SQUARE, 0, None
        self.group = np.full(R, -1, dtype=np.int32)
        self.data, self.sigma = rng.uniform(1.0, 2.0, R), rng.uniform(0.05, 0.2, R)
        self.sims, self.Jm = rng.uniform(0.5, 3.0, (3, R)), rng.standard_normal((3, R, 1))
        self.sfp_group, self.sfp_mean, self.sfp_sigma = np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0)
        self.id = 'lds-R%d' % R

    def sf_prior(self):
        return None


def test_lds_formula_and_limits_restated():
    assert _lds_bytes(1) - _lds_bytes(0) == 60 and _lds_bytes(0) == 4168
    # 64 KB, above which the launch has to raise the kernel's dynamic-LDS attribute, falls between R = 1022 and 1023
    assert _lds_bytes(1022) <= 64 * 1024 < _lds_bytes(1023) < _lds_bytes(1050) < _lds_bytes(1100)
    # the dynamic block ALONE fits 160 KB up to R = 2661; with the 16 static bytes only up to 2660
    assert _lds_bytes(2661) <= LDS_LIMIT < _lds_bytes(2662)
    assert _lds_bytes(2661) + LDS_STATIC > LDS_LIMIT >= _lds_bytes(2660) + LDS_STATIC
    assert LDS_LARGEST_R == 2660


@pytest.mark.parametrize('R', [1022, 1023, 1050, 1100, LDS_LARGEST_R])
def test_direct_mode_lds_sizes(R):
    """The last size in 64 KB (R = 1022), the first that needs the raised attribute (1023), two sizes beyond, and the
    largest whose dynamic AND static LDS fit the workgroup's 160 KB."""
    c = _LdsCase(R)
    sims = c.sims.copy()
    sims[1, R // 3] = np.nan
    rc, out, msg = loss_eval(c, sims, c.Jm)
    assert rc == 0, msg
    _expect_failed_vector(out, 1, c.id)
    for v in (0, 2):
        _check_vector(c, out, v, sims, c.id)


def test_direct_mode_too_large_is_refused_and_the_context_survives():
    """R = 2661 (dynamic block within 160 KB, dynamic + static not: accepted before this test existed, and then refused
    by the runtime at the launch) and R = 2662 come back with a negative code and the 'project too large' message;
    the same context then evaluates a small case correctly."""
    for R in (LDS_LARGEST_R + 1, LDS_LARGEST_R + 2):
        c = _LdsCase(R)
        rc, out, msg = loss_eval(c, c.sims, c.Jm)
        assert rc < 0 and 'project too large' in msg, (R, rc, msg)
        assert np.all(out['R_out'] == 7.0) and np.all(out['J'] == 7.0)
    c = ac.Case(ac.SHAPES[9])
    rc, out, msg = loss_eval(c, c.sims, c.Jm)
    assert rc == 0, msg
    for v in range(3):
        _check_vector(c, out, v, c.sims, c.id + ' (after a refusal)')


# ------------------------------------------------------------------------------------------------------------------
# integrated path
# ------------------------------------------------------------------------------------------------------------------
def _opts(h0):
    from sysbio_modeling_amd import _lib
    # one explicit variant in every call (the project's and the per-experiment ones): AUTO's batch-size rules cannot
    # pick different kernels for the V x E trajectories of the project and the V of an experiment
    return _lib.make_opts('rk4', h0=h0, variant='per_wave')


_spreads = {}     # case -> (largest normalised spread of sims, of Jmodel, measured error of sims, of Jmodel)


def _downstream(desc, out, theta, v, what):
    """R_out, J, sf, sf_grad, norms, grad from the sims and Jmodel the call returned: within C(n) u"""
    ref = ar.assemble_reference(out['sims'][v], out['Jmodel'][v], desc.row_data, desc.row_sigma, desc.row_sf, desc.G, desc.loss,
                                desc.compat, theta=theta[v], prior=desc.prior if len(desc.prior[0]) else None,
                                sf_prior=desc.sf_prior if len(desc.sf_prior[0]) else None)
    got = {k: out[k][v] for k in ('R_out', 'J', 'sf', 'sf_grad', 'grad')}
    got['norms'] = np.asarray(out['norms'][v])
    frac = ar.check_outputs(got, ref, desc.loss)
    assert set(frac) == set(got)
    print("%s vector %d downstream: fraction of C(n) u  %s" % (what, v, '  '.join('%s %.3f' % kv for kv in sorted(frac.items()))))
    _note(frac, what)
    assert max(frac.values()) <= 1.0, (what, v, frac)


def _normalised(got, value, scale):
    """|got - value| / scale entry by entry, computed in the reference's wide type; a non-zero error over a zero scale,
    or anything not finite: inf"""
    got = np.asarray(got)
    if not np.isfinite(got.astype(np.float64)).all():
        return np.full(got.shape, np.inf)
    err = np.asarray(abs(got.astype(value.dtype) - value))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0, 0.0, np.where(scale > 0, (err / np.where(scale > 0, scale, 1)).astype(np.float64), np.inf))


def _check_integrated(model, desc, theta, opts, what, extra_tol=None, vectors=None):
    """One evaluation of a hand-built project against the wide reference.  Returns the outputs.
    sims / Jmodel: the mapping of per-experiment integrations; tolerance (entries' own roundings + 4 x the largest spread
    between the runs with every mapped parameter at exp(theta), one ulp below and one ulp above) x scale.
    extra_tol(v) -> (absolute sims tolerance [R], absolute Jmodel tolerance [R][q]) adds the custom programs' own
    rounding bounds."""
    with db.LoadedProject(model, desc) as proj:
        out = proj.jacobian(theta, opts)
    V = theta.shape[0]
    vectors = range(V) if vectors is None else vectors
    runs = [db.sample_inputs(model, desc, theta, opts, shift) for shift in (0, -1, 1)]
    arrays = desc.reference_arrays()
    worst = [0.0, 0.0, 0.0, 0.0]
    for v in vectors:
        assert out['status'][v] == 0, (what, v, out['status'])
        maps = [ar.map_reference(arrays, Y[v], S[v], theta[v]) for Y, S in runs]
        for i, name in enumerate(('sims', 'Jmodel')):
            value, scale, n = maps[0][name]
            spread = max(float(np.max(_normalised(m[name][0], value, scale))) for m in maps[1:])
            spread2 = float(np.max(_normalised(maps[1][name][0], maps[2][name][0], scale)))
            spread = max(spread, spread2)
            assert np.isfinite(spread), (what, name, "the three runs disagree about an exact zero")
            err = _normalised(out[name][v], value, scale)
            tol = (n + 3) * U + 4.0 * spread
            if extra_tol is not None:
                with np.errstate(divide='ignore', invalid='ignore'):
                    tol = tol + np.where(np.asarray(scale, dtype=np.float64) > 0, extra_tol(v)[i] / np.asarray(scale, dtype=np.float64), 0.0)
            worst[i], worst[2 + i] = max(worst[i], spread), max(worst[2 + i], float(np.max(err)))
            assert np.all(err <= tol), (what, v, name, float(np.max(err / np.maximum(tol, 1e-300))), spread)
        _downstream(desc, out, theta, v, what)
    _spreads[what] = tuple(worst)
    print("%s: input spread sims %.2e Jmodel %.2e (x scale); measured error sims %.2e Jmodel %.2e" % ((what,) + tuple(worst)))
    return out


def _rows(rng, specs):
    """specs: (exp, tidx, vars or program name, sf) -> row dicts with seeded data / sigma"""
    rows = []
    for e, ti, what, sf in specs:
        r = dict(exp=e, tidx=ti, data=float(rng.uniform(1.0, 2.0)), sigma=float(rng.uniform(0.05, 0.2)), sf=sf)
        if isinstance(what, str):
            r['prog'] = what
        else:
            r['vars'] = list(what)
        rows.append(r)
    return rows


# -- 1. many experiments -------------------------------------------------------------------------------------------
_GRIDS = {0: [0.75], 1: [0.5, 1.0], 2: [0.0, 0.5, 1.0, 1.5, 2.0]}      # (binary fractions: dt / h0 is exact)
_E = 300
_E_FAIL = 290          # beyond the first 256 experiments of the status loop; carries no measurement rows


def _many_experiments(nan_fixed=False):
    """'simple' (one state, k_deg and k_synt): k_deg on slot 0, k_synt on slot 1 + e mod 3, except that the experiment
    _E_FAIL reads slot 4 alone (or, nan_fixed, has k_synt fixed at NaN through pfixed)."""
    rng = np.random.default_rng(300)
    pmap = np.zeros((_E, 2), dtype=np.int32)
    pmap[:, 1] = 1 + np.arange(_E) % 3
    pfixed = np.zeros((_E, 2))
    pmap[_E_FAIL, 1] = 4
    if nan_fixed:
        pmap[_E_FAIL, 1], pfixed[_E_FAIL, 1] = -1, np.nan
    grids = [_GRIDS[e % 3] for e in range(_E)]
    specs = []
    for e in range(_E):
        if e == _E_FAIL:
            continue
        n = len(grids[e])
        ti = [0, e % 2, (n - 1) if e % 2 else 1 + e % 3][e % 3]       # index 0 of a length-1 grid, the last of a length-5 one
        specs.append((e, ti, [0], e % 4 - 1))                        # groups 0..2 and rows without, interleaved
    specs.append((2, 0, [0], -1))                                    # index 0 of a grid that starts at t0: the state is exactly 0
    specs += [(5, 4, [0], 1), (5, 4, [0], 2)]                        # two rows on the same (experiment, index)
    return db.Descriptor(1, [0, 1], 5, pmap, pfixed, grids, _rows(rng, specs), n_groups=3,
                         sf_prior=([0, 2], [0.1, -0.2], [0.5, 0.8]), prior=([0, 3], [-0.5, 0.2], [1.0, 2.0]))


def _many_theta():
    rng = np.random.default_rng(301)
    return np.log([0.5, 1.0, 1.3, 0.8, 1.1])[None, :] + 0.2 * rng.standard_normal((3, 5))


def test_project_many_experiments_and_unequal_grids(gpu_models):
    """E = 300 (the status / step loop strides over E by 256), grid lengths 1, 2, 5 (n_t_max = 5: most blocks padded)."""
    model, desc, theta, opts = gpu_models('simple'), _many_experiments(), _many_theta(), _opts(0.125)
    assert desc.n_t_max == 5 and desc.E == 300 and (desc.row_exp != _E_FAIL).all()
    out = _check_integrated(model, desc, theta, opts, 'E300-grids-1-2-5')
    assert np.array_equal(out['n_steps'], out['traj_steps'].sum(axis=1))
    # RK4's partition (include/sbm.h): ceil(dt / h0) steps per output interval, from t0 = 0
    steps = out['traj_steps']
    assert (steps[:, 0::3] == 6).all() and (steps[:, 1::3] == 4 + 4).all() and (steps[:, 2::3] >= 4 * 4).all()
    assert (steps[:, 2::3] == steps[0, 2]).all()
    # the two rows on the same (experiment, index) sample the same value
    assert out['sims'][0, -1] == out['sims'][0, -2] and out['sims'][0, -3] == 0.0


def test_project_failed_experiment_beyond_256(gpu_models):
    """Experiment 290 has no measurement rows; where it fails, the vector's status is non-zero and its rows are +inf.
    Through pfixed = NaN the failure is every vector's (pfixed is per experiment); through a theta whose exp overflows on
    the slot only that experiment reads it is ONE vector's, and the others are bitwise what they are without it."""
    model, opts, theta = gpu_models('simple'), _opts(0.125), _many_theta()
    with db.LoadedProject(model, _many_experiments()) as proj:
        clean = proj.jacobian(theta, opts)
        bad_theta = theta.copy()
        bad_theta[1, 4] = 800.0
        out = proj.jacobian(bad_theta, opts)
    assert clean['status'].tolist() == [0, 0, 0]
    assert out['status'][1] != 0 and out['status'][0] == 0 and out['status'][2] == 0
    assert np.all(np.isposinf(out['R_out'][1])) and np.all(np.isposinf(out['J'][1])) and np.isposinf(out['norms'][1])
    assert np.all(np.isposinf(out['Jmodel'][1])) and np.all(np.isposinf(out['grad'][1]))
    assert np.all(np.isnan(out['sf'][1])) and np.all(np.isnan(out['sf_grad'][1]))
    for k in ('sims', 'R_out', 'J', 'Jmodel', 'sf', 'sf_grad', 'norms', 'grad'):
        for v in (0, 2):
            assert _same(out[k][v], clean[k][v]), (k, v)
    with db.LoadedProject(model, _many_experiments(nan_fixed=True)) as proj:
        out = proj.jacobian(theta, opts)
    assert (out['status'] != 0).all()
    assert np.all(np.isposinf(out['R_out'])) and np.all(np.isposinf(out['J'])) and np.all(np.isposinf(out['norms']))


# -- 2. parameter maps ---------------------------------------------------------------------------------------------
def _cascade_maps(sort_rows):
    """cascade20, E = 3, q = 5.  Model parameters k0..k6 and d0 are mapped, everything else fixed at its nominal value:
         experiment 0: slot 0 <- k0        1 <- k1 k2      2 <- k3 k4 k5 k6   3 <- nobody    4 <- d0
         experiment 1: slot 0 <- k1 k2     1 <- k3..k6     2 <- k0            3 <- d0        4 <- nobody
         experiment 2: slot 0 <- k3..k6    1, 2 <- nobody  3 <- k1 k2         4 <- k0        d0 FIXED here only
    -- every slot changes its readers from one experiment to the next."""
    from sysbio_modeling_amd import models_zoo
    nominal = models_zoo.cascade_nominal_params()
    layout = [{0: [0], 1: [1, 2], 2: [3, 4, 5, 6], 4: [20]}, {0: [1, 2], 1: [3, 4, 5, 6], 2: [0], 3: [20]},
              {0: [3, 4, 5, 6], 3: [1, 2], 4: [0]}]
    pmap = -np.ones((3, 40), dtype=np.int32)
    for e, slots in enumerate(layout):
        for c, ms in slots.items():
            pmap[e, ms] = c
    pfixed = np.tile(nominal, (3, 1))
    grids = [[2.0, 5.0], [1.0, 2.0, 3.0, 6.0], [4.0]]
    rng = np.random.default_rng(20)
    specs = []
    for e, g in enumerate(grids):
        for ti in range(len(g)):
            for var in range(12):
                specs.append((e, ti, [var], (var + ti) % 3 - 1))
    if not sort_rows:
        specs = [specs[i] for i in np.random.default_rng(21).permutation(len(specs))]
    # 84 rows on 256 // 5 = 51 row lanes: a lane that handles row r also handles row r + 51, of another experiment
    assert len(specs) == 84
    desc = db.Descriptor(20, np.arange(40), 5, pmap, pfixed, grids, _rows(rng, specs), n_groups=2)
    theta = np.log([1.1, 0.9, 1.2, 0.7, 0.4])[None, :] + 0.1 * rng.standard_normal((2, 5))
    return desc, theta, layout


@pytest.mark.parametrize('sort_rows', [True, False], ids=['rows-sorted', 'rows-not-sorted-by-experiment'])
def test_project_parameter_maps(gpu_models, sort_rows):
    """Slots read by no / one / two / four model parameters of an experiment, a parameter fixed in one experiment only, maps
    that change between consecutive experiments -- with rows sorted by experiment and not (include/sbm.h does not ask for
    sorted rows; the kernel caches a column's readers until the experiment changes)."""
    desc, theta, layout = _cascade_maps(sort_rows)
    crossing = desc.row_exp[:33] != desc.row_exp[51:]
    assert crossing.all() if sort_rows else crossing.sum() > 10, "row lanes with two rows see two experiments"
    if not sort_rows:
        assert (np.diff(desc.row_exp) != 0).sum() > 10
    out = _check_integrated(gpu_models('cascade20'), desc, theta, _opts(0.25), 'cascade20-maps-' + ('sorted' if sort_rows else 'unsorted'))
    for r in range(desc.R):
        unread = [c for c in range(5) if c not in layout[desc.row_exp[r]]]
        assert unread and np.all(out['Jmodel'][:, r, unread] == 0.0), "a slot nobody reads has an exactly zero column"


def test_project_parameter_without_sensitivity_column(gpu_models, zoo):
    """stiff50 has 50 parameters fixed at code generation (sens_col -1).  Slot 0 <- a0; slot 1 <- a1 AND b1 (one reader with
    a sensitivity column, one without); slot 2 <- b2 alone (its column of Jmodel is exactly zero, although the parameter
    moves the simulation); the rest fixed.  The time span is short enough for RK4 on the stiff system."""
    from sysbio_modeling_amd import models_zoo
    gm = zoo('stiff50')
    names = list(gm.param_order)
    sens_col = np.array([gm.sens_params.index(n) if n in gm.sens_params else -1 for n in names], dtype=np.int32)
    assert (sens_col < 0).sum() == 50
    nominal = models_zoo.stiff_nominal_params(50)
    a0, a1, b1, b2 = names.index('a0'), names.index('a1'), names.index('b1'), names.index('b2')
    pmap = -np.ones((2, 100), dtype=np.int32)
    pmap[0, [a0, a1, b1, b2]] = [0, 1, 1, 2]
    pmap[1, [a0, a1, b1, b2]] = [1, 0, 2, 2]
    pfixed = np.tile(nominal, (2, 1))
    grids = [[1.0e-7, 3.0e-7], [2.0e-7]]
    rng = np.random.default_rng(50)
    specs = [(e, ti, [var], -1) for e, g in enumerate(grids) for ti in range(len(g)) for var in (0, 1, 2)]
    desc = db.Descriptor(50, sens_col, 3, pmap, pfixed, grids, _rows(rng, specs))
    theta = np.log([nominal[a0], nominal[a1], nominal[b2]])[None, :] + 0.05 * rng.standard_normal((2, 3))
    out = _check_integrated(gpu_models('stiff50'), desc, theta, _opts(5.0e-8), 'stiff50-sens_col-1')
    assert np.all(out['Jmodel'][:, desc.row_exp == 0, 2] == 0.0) and np.all(out['Jmodel'][:, desc.row_exp == 1, 2] == 0.0)
    assert np.any(out['Jmodel'][:, :, 0] != 0.0)


# -- 3. row kinds mixed ----------------------------------------------------------------------------------------------
def _compiled(names):
    from sysbio_modeling_amd.project.observables import compile_observable
    return {nm: compile_observable(db.OPCODE_PROGRAMS[nm], db.OPCODE_VARIABLES) for nm in names}


@pytest.mark.parametrize('loss,compat', [(ac.SQUARE, 0), (ac.SQUARE, 1), (ac.LOG, 0), (ac.LOG, 1)],
                         ids=['square', 'square-compat', 'log', 'log-compat'])
def test_project_row_kinds_mixed(gpu_models, loss, compat):
    """'direct', 'sum' of 2 and of 5 variables and custom rows interleaved in one descriptor, some of each kind inside the
    same scale-factor group; parameter priors and scale-factor priors present; both losses, both reference_compat."""
    from sysbio_modeling_amd import models_zoo
    nominal = models_zoo.cascade_nominal_params()
    programs = _compiled(['ratio', 'trig_time'])
    pmap = -np.ones((2, 40), dtype=np.int32)
    pmap[0, :8], pmap[1, :8] = np.arange(8), [0, 1, 2, 3, 7, 6, 5, 4]
    pmap[:, 20:24] = [8, 9, 10, 11]
    pfixed = np.tile(nominal, (2, 1))
    grids = [[2.0, 5.0, 10.0], [3.0, 8.0]]
    kinds = [[2], 'ratio', [0, 1], [0, 2, 4, 6, 8], 'trig_time', [5]]
    specs = []
    for e, g in enumerate(grids):
        for ti in range(len(g)):
            for i, what in enumerate(kinds):
                specs.append((e, ti, what, (i + ti + e) % 3 - 1))          # every kind lands in group 0, group 1 and outside
    rng = np.random.default_rng(31 + 2 * loss + compat)
    desc = db.Descriptor(20, np.arange(40), 12, pmap, pfixed, grids, _rows(rng, specs), n_groups=2, programs=programs,
                         prior=([1, 9], [0.1, -1.0], [0.7, 1.5]), sf_prior=([1], [0.3], [0.6]), compat=compat, loss=loss)
    for g in range(2):
        kinds_in = set('custom' if r.get('prog') else len(r['vars']) for r in desc.rows if r['sf'] == g)
        assert kinds_in == {'custom', 1, 2, 5}
    theta = np.log(np.concatenate([nominal[:8], nominal[20:24]]))[None, :] + 0.1 * rng.standard_normal((2, 12))
    ulp = _device_libm_ulp(gpu_models('simple'))
    tol = _program_tolerances(gpu_models('cascade20'), desc, theta, _opts(0.25), ulp)
    out = _check_integrated(gpu_models('cascade20'), desc, theta, _opts(0.25), 'cascade20-mixed-%s-compat%d' % ('log' if loss else 'square', compat),
                            extra_tol=lambda v: tol[v])
    assert (out['sims'] > 0).all()


def test_project_row_kinds_on_the_two_state_model(gpu_models):
    """michaelis_menten (two states, five parameters): 'direct', 'sum' of both states and a custom ratio in one scale-factor
    group, log loss, three vectors, the two experiments sharing three slots and owning one each."""
    from sysbio_modeling_amd.project.observables import compile_observable
    programs = {'share': compile_observable('x0 / (x0 + x1)', ['x0', 'x1'])}
    pmap = np.array([[0, 1, 2, 3, 4], [0, 1, 5, 3, 4]], dtype=np.int32)
    grids = [[0.5, 1.0, 2.0], [1.5]]
    specs = [(e, ti, what, sf) for e, g in enumerate(grids) for ti in range(len(g))
             for what, sf in (([0], 0), ([0, 1], 0), ('share', 0), ([1], -1), ('share', -1))]
    rng = np.random.default_rng(2)
    desc = db.Descriptor(2, np.arange(5), 6, pmap, np.zeros((2, 5)), grids, _rows(rng, specs), n_groups=1, programs=programs,
                         prior=([5], [0.0], [1.0]), sf_prior=([0], [0.2], [0.9]), loss=ac.LOG)
    theta = np.log([1.0, 0.5, 1.0, 0.1, 0.2, 1.4])[None, :] + 0.1 * rng.standard_normal((3, 6))
    model, opts = gpu_models('michaelis_menten'), _opts(0.125)
    tol = _program_tolerances(model, desc, theta, opts, _device_libm_ulp(gpu_models('simple')))
    out = _check_integrated(model, desc, theta, opts, 'michaelis_menten-mixed-log', extra_tol=lambda v: tol[v])
    assert (out['sims'] > 0).all() and np.all(out['Jmodel'][:, desc.row_exp == 0, 5] == 0.0)


# -- 4. every opcode ---------------------------------------------------------------------------------------------------
_SWEEP = {'EXP': (-20.0, 20.0, False), 'LOG': (1.0e-3, 1.0e3, True), 'SQRT': (1.0e-3, 1.0e3, True), 'TANH': (-5.0, 5.0, False),
          'SIN': (-10.0, 10.0, False), 'COS': (-10.0, 10.0, False), 'POW2.5': (0.05, 20.0, True), 'POW-0.5': (0.05, 20.0, True)}
_ulp_cache = {}


def _device_libm_ulp(model):
    """Largest error of the device's exp, log, sqrt, tanh, sin, cos and pow against mpmath on 1000 arguments each, in ulps
    of the result (the ROCm tree here states no figure) -- measured through the interpreter itself: a program
    'TIME f END' without variables on rows whose row_time is the argument.  The bound used is TWICE the largest seen."""
    if _ulp_cache:
        return _ulp_cache
    import mpmath
    import sympy
    from sysbio_modeling_amd.project.observables import OP
    mpmath.mp.dps = 40
    rng = np.random.default_rng(1000)
    t = sympy.Symbol('t', real=True)
    programs, args = {}, {}
    for name, (lo, hi, logu) in _SWEEP.items():
        x = np.exp(rng.uniform(np.log(lo), np.log(hi), 1000)) if logu else rng.uniform(lo, hi, 1000)
        args[name] = x
        if name.startswith('POW'):
            ex = float(name[3:])
            code, consts, expr = [OP['TIME'], OP['CONST'], 0, OP['POW'], OP['END']], [ex], t ** sympy.Float(ex)
        else:
            code, consts, expr = [OP['TIME'], OP[name], OP['END']], [], getattr(sympy, name.lower())(t)
        programs[name] = dict(variables=[], subprograms=[code], constants=consts, expr=expr, symbols=[])
    rows = [dict(exp=0, tidx=0, prog=name, data=1.0, sigma=1.0, sf=-1, time=float(x)) for name in _SWEEP for x in args[name]]
    measured = {}
    for name in _SWEEP:       # one project per function: 1000 rows each
        sel = [r for r in rows if r['prog'] == name]
        desc = db.Descriptor(1, [0, 1], 2, [[0, 1]], [[0.0, 0.0]], [[0.0]], sel, programs={name: programs[name]})
        from sysbio_modeling_amd import _lib
        with db.LoadedProject(model, desc) as proj:
            out = proj.jacobian(np.zeros((1, 2)), _lib.make_opts('rk4', h0=1.0, variant='per_wave'))
        assert out['status'][0] == 0
        f = {'EXP': mpmath.exp, 'LOG': mpmath.log, 'SQRT': mpmath.sqrt, 'TANH': mpmath.tanh, 'SIN': mpmath.sin, 'COS': mpmath.cos}.get(name)
        worst = 0.0
        for x, got in zip(args[name], out['sims'][0]):
            want = f(mpmath.mpf(float(x))) if f else mpmath.power(mpmath.mpf(float(x)), mpmath.mpf(float(name[3:])))
            ulp_of = float(np.spacing(abs(float(want))))
            worst = max(worst, float(abs(mpmath.mpf(float(got)) - want)) / ulp_of)
        measured[name] = worst
    print("device math library, largest error over 1000 arguments (ulp): " + '  '.join('%s %.3f' % kv for kv in sorted(measured.items())))
    bound = {k: 2.0 * v for k, v in measured.items()}
    bound['POW'] = max(bound.pop('POW2.5'), bound.pop('POW-0.5'))
    _ulp_cache.update(bound, measured=measured)
    return _ulp_cache


def _program_tolerances(model, desc, theta, opts, ulp):
    """per vector (absolute sims tolerance [R], absolute Jmodel tolerance [R][q]) of the custom rows' own arithmetic: the
    running error bound of the value program, and for the Jacobian row sum_k bound(dg/dy_k) |S[var_k][col]| exp(theta_c)."""
    Y, S = db.sample_inputs(model, desc, theta, opts)
    out = []
    for v in range(theta.shape[0]):
        ts, tj = np.zeros(desc.R), np.zeros((desc.R, desc.q))
        for r, row in enumerate(desc.rows):
            if row.get('prog') is None:
                continue
            prog = desc.programs[row['prog']]
            e, ti = row['exp'], row['tidx']
            vals = [Y[v, e, ti, k] for k in prog['variables']]
            t = desc.row_time[r]
            ts[r] = db.program_error_bound(prog['subprograms'][0], prog['constants'], vals, t, ulp)
            wb = [db.program_error_bound(sub, prog['constants'], vals, t, ulp) for sub in prog['subprograms'][1:]]
            for c in range(desc.q):
                for m in np.flatnonzero(desc.pmap[e] == c):
                    if desc.sens_col[m] >= 0:
                        tj[r, c] += np.exp(theta[v, c]) * sum(b * abs(S[v, e, ti, k, desc.sens_col[m]]) for b, k in zip(wb, prog['variables']))
        out.append((ts, tj))
    return out


def test_device_math_library_errors(gpu_models):
    """The measured figures behind the custom rows' tolerances; a library function several ulps off would show here."""
    ulp = _device_libm_ulp(gpu_models('simple'))
    assert set(ulp['measured']) == set(_SWEEP) and all(np.isfinite(v) for v in ulp['measured'].values()), ulp['measured']


def test_project_every_opcode(gpu_models):
    """Every SBM_OP_* on the device: the compiled programs of descriptor_builder.OPCODE_PROGRAMS (ADD MUL NEG POW POWI EXP LOG
    SQRT TANH SIN COS ABS SIGN TIME VAR CONST; POWI -1, 2, -2, -3, -4, 63, 64), a hand-written one for SUB, DIV, POWI 0 and
    POWI 1, and a program 16 deep on the stack; ABS and SIGN at negative, zero and positive arguments (x0 is exactly 0 at
    index 0 of the grid, which starts at t0 = 0).  Value and Jacobian rows against mpmath on the sympy expression."""
    from sysbio_modeling_amd import models_zoo
    from sysbio_modeling_amd.project.observables import OP
    nominal = models_zoo.cascade_nominal_params()
    programs = _compiled(sorted(db.OPCODE_PROGRAMS))
    programs['sub_div_powi'] = db.hand_program('sub_div_powi')
    programs['deep16'] = db.hand_program('deep', 16)
    seen = set(op for p in programs.values() for sub in p['subprograms'] for op, _ in db.walk_program(sub))
    assert seen == set(OP.values())
    assert max(db.program_depth(sub) for sub in programs['deep16']['subprograms']) == 16
    pmap = -np.ones((1, 40), dtype=np.int32)
    pmap[0, :10] = np.arange(10)
    grid = [0.0, 2.0, 5.0, 10.0]
    specs = [(0, ti, nm, -1) for nm in sorted(programs) for ti in range(4) if ti > 0 or nm in db.ZERO_SAFE_PROGRAMS + ('deep16',)]
    rng = np.random.default_rng(4)
    desc = db.Descriptor(20, np.arange(40), 10, pmap, nominal[None, :], [grid], _rows(rng, specs), programs=programs)
    theta = np.log(nominal[:10])[None, :] + 0.05 * rng.standard_normal((2, 10))
    model = gpu_models('cascade20')
    ulp = _device_libm_ulp(gpu_models('simple'))
    tol = _program_tolerances(model, desc, theta, _opts(0.25), ulp)
    out = _check_integrated(model, desc, theta, _opts(0.25), 'cascade20-every-opcode', extra_tol=lambda v: tol[v])
    # the arguments ABS and SIGN saw: x0 - 2.5 negative, then positive; x0 itself exactly zero at t0
    zero_row = [r for r, row in enumerate(desc.rows) if row['prog'] == 'abs_sign' and row['tidx'] == 0][0]
    assert out['sims'][0, zero_row] == 1.0 + 2.5 and np.all(out['Jmodel'][:, zero_row] == 0.0)
    # one level deeper is refused when the project is loaded
    programs17 = {'deep17': db.hand_program('deep', 17)}
    bad = db.Descriptor(20, np.arange(40), 10, pmap, nominal[None, :], [grid], _rows(rng, [(0, 1, 'deep17', -1)]), programs=programs17)
    rc, h, msg = db.try_load(model, bad)
    assert rc < 0 and 'stack' in msg, (rc, msg)


def test_zz_error_table():
    """Prints what the tests above measured (docs/history.md holds the table of the run on an MI355X)."""
    if not _worst:
        return                                     # run on its own: nothing to report
    assert len(_ran) == len(ac.IDS) or len(_ran) < 5, "a direct-mode case was left out: %s" % sorted(set(ac.IDS) - _ran)
    for k, (f, what) in sorted(_worst.items()):
        print("largest normalised error of %-8s %.3f of its bound C(n) u   (%s)" % (k, f, what))
    for what, s in sorted(_spreads.items()):
        print("%-40s spread sims %.2e Jmodel %.2e   error sims %.2e Jmodel %.2e" % ((what,) + s))
    assert all(f <= 1.0 for f, _ in _worst.values())
