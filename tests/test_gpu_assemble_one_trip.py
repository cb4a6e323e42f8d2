"""k_assemble with a thread's rows of J kept in registers (csrc/sbm_assemble.hpp: AssembleForm::rows = 4 or 12, J stored
once) against the form through global memory (rows = 0: pass A stores the model Jacobian, pass B loads, scales and stores
it again), bit for bit.  Both forms are in the one library: SBM_ASSEMBLE_ROWS_IN_REGS=0, read at every launch, takes the
form through global memory for every shape, and under SBM_DEBUG_LAUNCH the launcher names the instantiation it took
(the first test reads that: the comparisons below would pass vacuously if the switch did nothing).

Every output array of the two launches is compared with numpy.array_equal where neither is NaN, and the NaN positions
separately.  Direct mode (sbm_loss_eval_host): the shapes of tests/support/assembly_cases.py and shapes built with its
Case at the edges of the tiles -- 3, 4, 5 and 11, 12, 13 rows a thread, with R a multiple of the row lanes and not (a
thread whose last row is missing), q = 1, 40, 64, 256 and 300, G = 0, 1 and 4 with groups interleaved, random, with
gaps and on one row lane (the flush of the per-lane partial sums), both losses with plain rows mixed in, both
reference_compat values, scale-factor priors, V = 3 with a NaN simulation in vector 1 (the fill path) and a non-positive
one.  Integrated path (sbm_jacobian_batch, RK4, 32 steps at most): cascade20 with 'direct' and 'sum' rows, two
experiments whose parameter maps differ, parameter and scale-factor priors, on 4 / 12 rows a thread (the second is the
headline's layout: 40 parameters on 6 row lanes); with one custom-observable row (the interpreter instantiation); one
vector of four failing.  Nullable outputs: J without Jmodel, Jmodel without J, J with grad and nothing else, no
sensitivities at all (sbm_residuals_batch), and in direct mode sf_grad alone, J alone and no model Jacobian.  (grad or
sf_grad without J and Jmodel is refused by sbm_jacobian_batch before any launch.)  The same launch twice gives the same
bits."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from tests.support import assembly_cases as ac
from tests.support import descriptor_builder as db

pytestmark = pytest.mark.gpu

SWITCH = 'SBM_ASSEMBLE_ROWS_IN_REGS'
SQUARE, LOG = ac.SQUARE, ac.LOG


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, val in kv.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val
        yield
    finally:
        for k, val in old.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val


def _both(call):
    """call() with the default instantiation, with the form through global memory, and with the default again"""
    with _env(**{SWITCH: None}):
        new = call()
    with _env(**{SWITCH: '0'}):
        ref = call()
    with _env(**{SWITCH: None}):
        again = call()
    return new, ref, again


def _assert_same(got, ref, what):
    assert set(got) == set(ref), what
    for k in sorted(got):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        if a.dtype.kind == 'f':
            na, nb = np.isnan(a), np.isnan(b)
            assert np.array_equal(na, nb), (what, k, 'NaN positions')
            assert np.array_equal(np.where(na, 0.0, a), np.where(nb, 0.0, b)), (what, k, int((a != b).sum() - na.sum()))
            # (array_equal takes -0.0 for +0.0: the signs too)
            assert np.array_equal(np.signbit(a), np.signbit(b)), (what, k, 'signs')
        else:
            assert np.array_equal(a, b), (what, k)


# ------------------------------------------------------------------------------------------------------------------
# direct mode
# ------------------------------------------------------------------------------------------------------------------
def _loss_eval(c, sims, Jm, want=('J', 'sf', 'sf_grad', 'norms', 'status'), fill=7.0):
    """outputs of sbm_loss_eval_host for the case's tables; outputs not wanted are passed as NULL, buffers are
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
    keep = dict(data=np.ascontiguousarray(c.data), sigma=np.ascontiguousarray(c.sigma),
                group=np.ascontiguousarray(c.group, dtype=np.int32),
                plain=None if c.plain is None else np.ascontiguousarray(c.plain, dtype=np.int32),
                g=np.ascontiguousarray(c.sfp_group, dtype=np.int32), m=np.ascontiguousarray(c.sfp_mean),
                s=np.ascontiguousarray(c.sfp_sigma))
    desc = _lib.LossDesc(R, q, c.G, NSP, c.loss, c.compat, dp(keep['data']), dp(keep['sigma']), ip(keep['group']),
                         ip(keep['plain']), ip(keep['g']), dp(keep['m']), dp(keep['s']))
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
    assert rc == 0, (rc, msg.decode() if msg else '')
    return out


# (q, R, G, pattern, loss, reference_compat, sf priors, plain rows, non-positive simulation in vector 2); the row lanes
# are 256 // q: 4 for q = 64, 6 for q = 40, 256 for q = 1, 1 for q = 256; q = 300 takes two passes over the columns
_TILE_EDGES = [
    (64, 12, 4, 'interleaved', SQUARE, 0, True, False, False),        # 3 rows a thread
    (64, 15, 4, 'random', LOG, 0, True, True, False),                 # 4, the last one missing on row lane 3
    (64, 16, 1, 'contiguous', SQUARE, 1, False, False, False),        # 4
    (64, 17, 4, 'interleaved_gaps', LOG, 1, False, False, False),     # 5: the larger tile, 7 of its rows missing
    (64, 44, 4, 'one_lane', SQUARE, 0, True, False, False),           # 11
    (64, 47, 4, 'random', LOG, 0, False, True, True),                 # 12, the last one missing on row lane 3
    (64, 48, 0, 'contiguous', SQUARE, 0, False, False, False),        # 12
    (64, 48, 4, 'single_row', LOG, 1, True, False, False),            # 12
    (64, 49, 4, 'interleaved', LOG, 0, True, False, False),           # 13: through global memory either way
    (40, 64, 4, 'interleaved', SQUARE, 0, True, False, False),        # the headline's shape: 11 rows on 6 row lanes
    (40, 64, 4, 'first_last', LOG, 0, False, True, False),
    (40, 72, 1, 'interleaved_gaps', SQUARE, 1, False, False, False),  # 12
    (40, 73, 4, 'random', SQUARE, 0, True, False, False),             # 13
    (40, 2, 1, 'contiguous', SQUARE, 0, False, False, False),         # fewer rows than row lanes: threads without a row
    (1, 3, 1, 'contiguous', SQUARE, 0, True, False, False),
    (1, 1024, 4, 'random', LOG, 0, True, False, False),               # 4 rows on 256 row lanes
    (1, 1025, 4, 'interleaved', SQUARE, 0, False, False, False),      # 5: the last on one lane only
    (256, 4, 4, 'interleaved', SQUARE, 0, True, False, False),        # one row lane
    (256, 5, 1, 'contiguous', LOG, 1, False, True, False),
    (256, 12, 4, 'interleaved_gaps', SQUARE, 0, False, False, False),
    (256, 13, 4, 'random', LOG, 0, True, False, False),
    (300, 5, 4, 'interleaved', SQUARE, 0, True, False, False),
]


def _rows_per_thread(q, R):
    return -(-R // ac.row_lanes(q))


def test_tile_edge_shapes_cover_the_list():
    per = {(s[0], _rows_per_thread(s[0], s[1])) for s in _TILE_EDGES}
    assert {(64, k) for k in (3, 4, 5, 11, 12, 13)} <= per and {(40, 11), (40, 12), (40, 13)} <= per
    assert {(256, 4), (256, 5), (256, 12), (256, 13), (1, 4), (1, 5)} <= per
    assert {s[2] for s in _TILE_EDGES} == {0, 1, 4} and {s[4] for s in _TILE_EDGES} == {SQUARE, LOG}
    assert any(s[1] % ac.row_lanes(s[0]) for s in _TILE_EDGES if s[0] == 64)
    assert any(s[7] for s in _TILE_EDGES) and any(s[6] for s in _TILE_EDGES) and {s[5] for s in _TILE_EDGES} == {0, 1}


def test_the_switch_picks_the_instantiation(capfd):
    """the launcher's own word for what the comparisons below compare"""
    c = ac.Case(_TILE_EDGES[9])
    capfd.readouterr()
    with _env(SBM_DEBUG_LAUNCH='1', **{SWITCH: None}):
        _loss_eval(c, c.sims, c.Jm)
    assert 'k_assemble<12, 0, 0>: R 64 q 40 G 4' in capfd.readouterr().err
    with _env(SBM_DEBUG_LAUNCH='1', **{SWITCH: '0'}):
        _loss_eval(c, c.sims, c.Jm)
    assert 'k_assemble<0, 0, 0>: R 64 q 40 G 4' in capfd.readouterr().err
    c = ac.Case(_TILE_EDGES[1])
    with _env(SBM_DEBUG_LAUNCH='1', **{SWITCH: None}):
        _loss_eval(c, c.sims, c.Jm)
    assert 'k_assemble<4, 0, 1>: R 15 q 64 G 4' in capfd.readouterr().err


_DIRECT = _TILE_EDGES + list(ac.SHAPES)


@pytest.mark.parametrize('shape', _DIRECT, ids=[ac.case_id(s) for s in _DIRECT])
def test_direct_mode_bits(shape):
    c = ac.Case(shape)
    sims = c.sims_with_faults()
    new, ref, again = _both(lambda: _loss_eval(c, sims, c.Jm))
    assert ref['status'][1] != 0 and ref['status'][0] == 0 and np.all(np.isposinf(ref['J'][1]))
    assert np.all(np.isfinite(ref['J'][0])) and not np.any(ref['J'][0] == 7.0)
    _assert_same(new, ref, c.id)
    _assert_same(again, new, c.id + ' (twice)')


_NULLABLE = [_TILE_EDGES[i] for i in (1, 5, 9, 15)]


@pytest.mark.parametrize('shape', _NULLABLE, ids=[ac.case_id(s) for s in _NULLABLE])
def test_direct_mode_nullable_outputs(shape):
    """sf_grad alone, J alone, no model Jacobian (residuals only): each bit for bit the other form's, and what is
    returned is what the full call returns"""
    c = ac.Case(shape)
    sims = c.sims_with_faults()
    full = _loss_eval(c, sims, c.Jm)
    for want, Jm in ((('sf_grad',), c.Jm), (('J',), c.Jm), (('sf', 'norms', 'status'), None)):
        new, ref, _ = _both(lambda: _loss_eval(c, sims, Jm, want=want))
        _assert_same(new, ref, (c.id, want))
        _assert_same({k: new[k] for k in new}, {k: full[k] for k in new}, (c.id, want, 'against the full call'))


# -- the scale-factor sums: every group's two sums are reduced side by side, and each must still be added up as block_sum
# adds: per thread over its rows r = tid, tid + 256, ... from +0.0, the butterfly over the 64 lanes of a wavefront
# (partner lane ^ 32, 16, ..., 1), the wavefront results in wavefront order from +0.0.  Both forms share that code, so the
# comparisons above cannot see its order; this one can: sigma = 1, simulations small integers and measurements +-2^k, so
# that every term (s d and s s) is exact whether or not the compiler fuses its multiply-add, and the sums, which are
# not, depend on the order alone.  The order is replayed in numpy.
class _ExactCase(object):
    def __init__(self, R, G, seed):
        rng = np.random.default_rng(seed)
        self.R, self.G, self.loss, self.compat, self.plain = R, G, SQUARE, 0, None
        self.group = (rng.integers(0, G, R)).astype(np.int32)
        self.group[:G] = np.arange(G)
        self.sigma = np.ones(R)
        self.data = rng.choice([-1.0, 1.0], R) * 2.0 ** rng.integers(0, 60, R)
        self.sims = rng.integers(1, 8, (3, R)).astype(np.float64)
        self.sfp_group, self.sfp_mean, self.sfp_sigma = np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0)


def _block_sum_replayed(terms):
    acc = np.zeros(256)
    for lo in range(0, len(terms), 256):
        chunk = terms[lo:lo + 256]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    v = acc.reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    total = 0.0
    for w in range(4):
        total = total + v[w, 0]
    return total


def test_block_sum_replay_sees_the_order():
    """the replay itself: 1 on wavefront 0, 2^53 on wavefront 1, -2^53 on wavefront 2 add up to 0 in wavefront order
    (and would to 1 from the last wavefront down)"""
    t = np.zeros(256)
    t[0], t[64], t[128] = 1.0, 2.0 ** 53, -2.0 ** 53
    assert _block_sum_replayed(t) == 0.0 and _block_sum_replayed(t[::-1].copy()) != 0.0


@pytest.mark.parametrize('R,G', [(256, 1), (200, 4), (700, 3)], ids=['R256-G1', 'R200-G4', 'R700-G3'])
def test_scale_factor_sums_keep_their_order(R, G):
    c = _ExactCase(R, G, [R, G])
    Jm = np.random.default_rng(R).standard_normal((3, R, 3))
    want = np.empty((3, G))
    for v in range(3):
        for g in range(G):
            sel = c.group == g
            sde = _block_sum_replayed(np.where(sel, c.sims[v] * c.data, 0.0))
            sds = _block_sum_replayed(np.where(sel, c.sims[v] * c.sims[v], 0.0))
            want[v, g] = sde / sds
    assert len(np.unique(want)) > G, "the sums are not all alike"
    new, ref, _ = _both(lambda: _loss_eval(c, c.sims, Jm))
    _assert_same(new, ref, 'exact terms')
    _assert_same({'sf': new['sf']}, {'sf': want}, 'scale factors against the replayed order')


# ------------------------------------------------------------------------------------------------------------------
# integrated path
# ------------------------------------------------------------------------------------------------------------------
def _opts():
    from sysbio_modeling_amd import _lib
    return _lib.make_opts('rk4', h0=0.25, variant='per_wave')


def _jacobian(proj, theta, opts, want, fill=7.0):
    """sbm_jacobian_batch with the outputs in `want` (the others NULL), or sbm_residuals_batch when want has neither J
    nor Jmodel"""
    import torch
    from sysbio_modeling_amd import _lib
    d = proj.desc
    theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1, d.q)
    V = theta.shape[0]
    RT = d.R + len(d.prior[0]) + len(d.sf_prior[0])
    dev = lambda *shape: torch.full(shape, fill, dtype=torch.float64, device='cuda')
    idev = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device='cuda')
    th = torch.from_numpy(theta).cuda()
    shapes = dict(sims=(V, d.R), R_out=(V, RT), J=(V, RT, d.q), Jmodel=(V, d.R, d.q), sf=(V, max(d.G, 1)),
                  sf_grad=(V, max(d.G, 1), d.q), norms=(V,), grad=(V, d.q))
    out = {k: dev(*shapes[k]) for k in want if k in shapes}
    out['status'], out['n_steps'] = idev(V), idev(V)
    p = lambda k: _lib.dev_ptr(out.get(k))
    if 'J' in want or 'Jmodel' in want:
        rc = proj.lib.sbm_jacobian_batch(proj.handle, _lib.dev_ptr(th), V, ctypes.byref(opts), p('sims'), p('R_out'), p('J'),
                                         p('Jmodel'), p('sf'), p('sf_grad'), p('norms'), p('grad'), p('status'), p('n_steps'))
    else:
        rc = proj.lib.sbm_residuals_batch(proj.handle, _lib.dev_ptr(th), V, ctypes.byref(opts), p('sims'), p('R_out'), p('sf'),
                                          p('norms'), p('status'), p('n_steps'))
    _lib.check(rc, 'sbm_jacobian_batch')
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_ALL = ('sims', 'R_out', 'J', 'Jmodel', 'sf', 'sf_grad', 'norms', 'grad')


def _rows(rng, specs):
    rows = []
    for e, ti, what, sf in specs:
        r = dict(exp=e, tidx=ti, data=float(rng.uniform(1.0, 2.0)), sigma=float(rng.uniform(0.05, 0.2)), sf=sf)
        if isinstance(what, str):
            r['prog'] = what
        else:
            r['vars'] = list(what)
        rows.append(r)
    return rows


def _cascade(q, n_vars_measured, loss, compat, custom):
    """cascade20, two experiments.  q = 40: every model parameter on its own slot, except that experiment 1 swaps the
    readers of slots 0..3 and puts k4 AND k5 on slot 4 (slot 5 has no reader there).  q = 12: k0..k7 and d0..d3 mapped
    (experiment 1 reverses slots 4..7), the rest fixed.  Rows: every (experiment, time point, measured variable), a
    'sum' of two and of five variables per time point (two time points an experiment for q = 40, three for q = 12: the
    states far down the cascade are not yet positive at t = 1), one custom ratio when asked for; groups (var + ti) % 5 - 1, so
    that consecutive rows change group and a thread's rows (every 6th or 21st) land in every group."""
    from sysbio_modeling_amd import models_zoo
    from sysbio_modeling_amd.project.observables import compile_observable
    nominal = models_zoo.cascade_nominal_params()
    pmap = -np.ones((2, 40), dtype=np.int32)
    if q == 40:
        pmap[0], pmap[1] = np.arange(40), np.arange(40)
        pmap[1, :4] = [3, 2, 1, 0]
        pmap[1, 5] = 4
        mapped = np.arange(40)
    else:
        pmap[0, :8], pmap[1, :8] = np.arange(8), [0, 1, 2, 3, 7, 6, 5, 4]
        pmap[:, 20:24] = [8, 9, 10, 11]
        mapped = np.concatenate([np.arange(8), np.arange(20, 24)])
    pfixed = np.tile(nominal, (2, 1))
    grids = [[2.0, 5.0], [1.0, 3.0]] if q == 40 else [[2.0, 5.0, 8.0], [1.0, 3.0, 6.0]]
    specs = []
    for e, g in enumerate(grids):
        for ti in range(len(g)):
            for var in range(n_vars_measured):
                specs.append((e, ti, [var], (var + ti) % 5 - 1))
            specs.append((e, ti, [0, 1], 0))
            specs.append((e, ti, [0, 2, 4, 6, 8], -1))
    programs = None
    if custom:
        programs = {'ratio': compile_observable(db.OPCODE_PROGRAMS['ratio'], db.OPCODE_VARIABLES)}
        specs.insert(7, (0, 1, 'ratio', 2))
    rng = np.random.default_rng([q, n_vars_measured, loss, compat, int(custom)])
    desc = db.Descriptor(20, np.arange(40), q, pmap, pfixed, grids, _rows(rng, specs), n_groups=4, programs=programs,
                         prior=([1, q - 1], [0.1, -1.0], [0.7, 1.5]), sf_prior=([1, 3], [0.3, -0.1], [0.6, 0.9]),
                         compat=compat, loss=loss)
    theta = np.log(nominal[mapped])[None, :] + 0.1 * rng.standard_normal((4, q))
    theta[2, 0] = 800.0          # exp overflows: vector 2 fails, its neighbours do not
    return desc, theta


# (q, measured variables, loss, compat, custom row) -> rows, rows a thread
_INTEGRATED = [
    (40, 14, SQUARE, 0, False),     # 64 rows on 6 row lanes: 11 a thread, the headline's layout
    (40, 15, LOG, 1, False),        # 68: 12 a thread, the last one missing on row lanes 2..5
    (40, 16, SQUARE, 0, True),      # 73 with the custom row: 13 a thread, through global memory either way
    (40, 14, LOG, 0, True),         # 65 with the custom row: the interpreter instantiation on the larger tile
    (12, 12, SQUARE, 1, False),     # three time points: 84 rows on 21 row lanes, 4 a thread
    (12, 12, LOG, 0, True),         # 85 with the custom row: 5 a thread
]


@pytest.mark.parametrize('q,nv,loss,compat,custom', _INTEGRATED,
                         ids=['q%d-vars%d-%s-compat%d%s' % (q, nv, 'log' if l else 'square', c, '-custom' if p else '')
                              for q, nv, l, c, p in _INTEGRATED])
def test_integrated_bits(gpu_models, q, nv, loss, compat, custom):
    desc, theta = _cascade(q, nv, loss, compat, custom)
    assert desc.R == (4 if q == 40 else 6) * (nv + 2) + int(custom)
    with db.LoadedProject(gpu_models('cascade20'), desc) as proj:
        new, ref, again = _both(lambda: _jacobian(proj, theta, _opts(), _ALL))
        assert ref['status'].tolist() == [0, 0, 2, 0] or (ref['status'][2] != 0 and not ref['status'][[0, 1, 3]].any())
        assert np.all(np.isposinf(ref['J'][2])) and np.all(np.isfinite(ref['J'][[0, 1, 3]]))
        assert not np.any(ref['J'] == 7.0) and not np.any(ref['Jmodel'] == 7.0) and not np.any(ref['grad'] == 7.0)
        assert np.any(ref['Jmodel'][0] != 0.0) and (ref['sims'][[0, 1, 3]] > 0).all()
        _assert_same(new, ref, 'all outputs')
        _assert_same(again, new, 'all outputs (twice)')
        if (q, nv) in ((40, 14), (12, 12)) and not custom:
            for want in (('R_out', 'J'), ('R_out', 'Jmodel'), ('R_out', 'J', 'grad'), ('R_out', 'sf', 'norms')):
                part, pref, _ = _both(lambda: _jacobian(proj, theta, _opts(), want))
                _assert_same(part, pref, want)
                if 'J' in want or 'Jmodel' in want:      # (the run without sensitivities is another integrator kernel)
                    _assert_same({k: part[k] for k in want}, {k: new[k] for k in want}, (want, 'against the full call'))
