"""The wide reference of the assembly kernel (tests/support/assembly_reference.py) against everything else that states
the same formulas: the float64 oracle (oracle/project_oracle.py through tests/loss_cases.RowsOnlyOracle), mpmath, and
-- for the custom observables -- oracle/program_oracle.py on the compiled programs against mpmath on the expression.
No GPU."""
import numpy as np
import pytest

from tests.loss_cases import RowsOnlyOracle
from tests.support import assembly_cases as ac
from tests.support import assembly_reference as ar
from tests.support import descriptor_builder as db


def test_longdouble_is_wide_or_mpmath_takes_over():
    a = ar.arithmetic()
    assert a.mp or np.finfo(np.longdouble).nmant >= 63
    x = a.arr([1.0]) + a.arr([2.0 ** -60])
    assert (x != a.arr([1.0])).all()          # a double could not hold it


@pytest.mark.parametrize('shape', ac.SHAPES, ids=ac.IDS)
def test_cases_are_what_they_claim(shape):
    """Every group non-empty, plain rows only without a group, the fault rows where the kernel has to notice them."""
    c = ac.Case(shape)
    assert (c.counts > 0).all() and len(c.counts) == c.G
    assert c.group.min() >= -1 and c.group.max() < max(c.G, 1)
    if c.plain is not None:
        assert (c.group[c.plain == 1] == -1).all()
        assert c.plain[c.nonpos_row] == 0
    assert c.sims.min() >= 0.5 and c.data.min() >= 1.0 and c.sigma.min() >= 0.05


def _oracle(c, v):
    rows = [(0, 'g%d' % g if g >= 0 else 'none', float(d), float(s), 0.0) for g, d, s in zip(c.group, c.data, c.sigma)]
    po = RowsOnlyOracle(rows, c.sims[v], c.Jm[v], ['g%d' % g for g in range(c.G)], c.q)
    po.loss = 'log' if c.loss == ac.LOG else 'square'
    po.compat = bool(c.compat)
    for g, m, s in zip(c.sfp_group, c.sfp_mean, c.sfp_sigma):
        po.sf_priors[int(g)] = (float(m), float(s))
    return po, rows


_ORACLE_SHAPES = [s for s in ac.SHAPES if not s[7] and not s[8] and s[0] * s[1] <= 70000]


@pytest.mark.parametrize('shape', _ORACLE_SHAPES, ids=[ac.case_id(s) for s in _ORACLE_SHAPES])
def test_wide_reference_against_float64_oracle(shape):
    """RowsOnlyOracle / ProjectOracle._sf / calc_project_jacobian in float64 on the direct-mode cases (those without
    plain rows, which the oracle does not know): within C(n) u of the wide reference, normalised by scale.  (A float64
    restatement with permuted rows was measured at most 3.8 u off the longdouble one on four shapes: a sanity figure;
    the assertion uses C(n).)"""
    c = ac.Case(shape)
    theta = np.zeros(c.q)
    for v in (0, 2):
        po, rows = _oracle(c, v)
        res, _, B = po.residuals(theta, return_parts=True)
        J = po.calc_project_jacobian(theta)
        dB = po._sf(rows, c.sims[v], c.Jm[v])[1]
        got = {'sf': np.asarray(B, dtype=float).reshape(c.G), 'R_out': res, 'J': J, 'sf_grad': dB.reshape(c.G, c.q),
               'norms': np.asarray(np.sum(res ** 2)), 'grad': (J.T * res).sum(axis=1)}
        ref = ar.assemble_reference(c.sims[v], c.Jm[v], c.data, c.sigma, c.group, c.G, c.loss, c.compat, sf_prior=c.sf_prior())
        frac = ar.check_outputs(got, ref, c.loss)
        assert set(frac) == set(got)
        assert max(frac.values()) <= 1.0, frac


_SMALL = [s for s in ac.SHAPES if s[0] * s[1] <= 400]


@pytest.mark.parametrize('shape', _SMALL, ids=[ac.case_id(s) for s in _SMALL])
def test_longdouble_against_mpmath(shape):
    """On the small shapes the longdouble evaluation against the 40-digit one: C(n) roundings of 2^-64 each, by the same
    count as for the double-precision kernel (the sums are numpy's, in some order)."""
    import mpmath
    c = ac.Case(shape)
    # (where longdouble is no extended format the default arithmetic IS mpmath and the comparison is an identity)
    ld = ar.assemble_reference(c.sims[0], c.Jm[0], c.data, c.sigma, c.group, c.G, c.loss, c.compat, plain=c.plain,
                               sf_prior=c.sf_prior(), use_mpmath=not ar.WIDE)
    mp = ar.assemble_reference(c.sims[0], c.Jm[0], c.data, c.sigma, c.group, c.G, c.loss, c.compat, plain=c.plain,
                               sf_prior=c.sf_prior(), use_mpmath=True)
    K = ar.bound_constants(c.loss, c.counts.max() if c.G else 0)
    assert set(ld) == set(mp) == {'sf', 'R_out', 'norms', 'sf_grad', 'J', 'grad'}
    for name in ld:
        v_ld, v_mp, sc, n = np.asarray(ld[name][0]), np.asarray(mp[name][0]), np.asarray(mp[name][1]), np.asarray(mp[name][2])
        assert v_ld.shape == v_mp.shape
        for a, b, s, nn in zip(v_ld.ravel(), v_mp.ravel(), sc.ravel(), n.ravel()):
            err = abs(ar.to_mpf(a) - b)
            assert err <= (int(nn) + K[name]) * mpmath.mpf(2) ** -64 * s, (name, a, b)


def test_comparison_catches_planted_nan_and_inf():
    c = ac.Case(ac.SHAPES[9])
    ref = ar.assemble_reference(c.sims[0], c.Jm[0], c.data, c.sigma, c.group, c.G, c.loss, c.compat)
    clean = {k: np.asarray(v[0], dtype=np.float64) for k, v in ref.items()}
    assert max(ar.check_outputs(clean, ref, c.loss).values()) <= 1.0
    for name, where in (('R_out', (5,)), ('J', (7, 2)), ('sf', (3,))):
        for poison in (np.nan, np.inf, -np.inf):
            got = {k: v.copy() for k, v in clean.items()}
            got[name][where] = poison
            frac = ar.check_outputs(got, ref, c.loss)
            assert frac[name] == float('inf') and all(np.isfinite(f) for k, f in frac.items() if k != name)
    # a NaN / inf at the SAME place in both is agreement; a different sign of inf is not
    val = np.array([1.0, np.inf, np.nan])
    assert ar.normalised_error(val, val.astype(np.longdouble), np.ones(3), ar.U) == 0.0
    assert ar.normalised_error(np.array([1.0, -np.inf, np.nan]), val.astype(np.longdouble), np.ones(3), ar.U) == float('inf')
    # zero scale: exact match or nothing
    assert ar.normalised_error(np.array([0.0]), np.zeros(1, np.longdouble), np.zeros(1), ar.U) == 0.0
    assert ar.normalised_error(np.array([1e-300]), np.zeros(1, np.longdouble), np.zeros(1), ar.U) == float('inf')


def test_reference_reproduces_a_hand_computed_case():
    """Two rows, one group, square loss: B = (s.d / sigma^2) / (s.s / sigma^2) by hand."""
    s, d, sg = np.array([1.0, 2.0]), np.array([2.0, 3.0]), np.array([1.0, 0.5])
    Jm = np.array([[1.0], [-1.0]])
    ref = ar.assemble_reference(s, Jm, d, sg, [0, 0], 1, ar.SQUARE, 0)
    sde, sds = 1 * 2 + 2 * 3 * 4, 1 + 4 * 4
    B = sde / sds
    assert float(ref['sf'][0][0]) == pytest.approx(B, rel=1e-15)
    jde, jds = 2 - 3 * 4, 1 - 2 * 4
    dB = jde / sds - 2 * sde * jds / sds ** 2
    assert float(ref['sf_grad'][0][0, 0]) == pytest.approx(dB, rel=1e-15)
    assert float(ref['sf_grad'][1][0, 0]) == pytest.approx((2 + 12) / sds + 2 * sde * (1 + 8) / sds ** 2, rel=1e-15)
    r = np.array([(B * 1 - 2) / 1, (B * 2 - 3) / 0.5])
    assert np.allclose(np.asarray(ref['R_out'][0], dtype=float), r, rtol=1e-15)
    J = np.array([(B * 1 + 1 * dB) / 1, (B * -1 + 2 * dB) / 0.5])
    assert np.allclose(np.asarray(ref['J'][0], dtype=float)[:, 0], J, rtol=1e-14)
    assert float(ref['grad'][0][0]) == pytest.approx(float(J @ r), rel=1e-13)
    assert ref['sf'][2].tolist() == [2] and int(ref['norms'][2]) == 2


@pytest.mark.parametrize('name', db.TEST_PROGRAM_NAMES)
def test_program_oracle_on_every_test_program_against_mpmath(name):
    """oracle/program_oracle.run on the programs the device test loads (compiled and hand-written), value and every
    derivative, against mpmath on the sympy expression -- within the running error bound of the program's own operations
    in float64."""
    from oracle import program_oracle
    c = db.all_test_programs()[name]
    rng = np.random.default_rng(len(name))
    for trial in range(4):
        y = rng.uniform(0.3, 1.7, len(db.OPCODE_VARIABLES))
        if trial == 3 and name in db.ZERO_SAFE_PROGRAMS + ('deep16',):
            y[:] = 0.0
        t = float(rng.uniform(0.5, 3.0))
        vals = [y[i] for i in c['variables']]
        g, w = ar.custom_row_reference(c['expr'], c['symbols'], vals, t)
        assert len(c['subprograms']) == 1 + len(c['variables'])
        for sub, want in zip(c['subprograms'], [g] + w):
            got = program_oracle.run(sub, c['constants'], vals, t)
            bound = db.program_error_bound(sub, c['constants'], vals, t, db.HOST_LIBM_ULP)
            assert abs(float(got) - float(want)) <= bound + abs(float(want)) * 2.0 ** -52, (name, trial, got, float(want), bound)


def test_every_opcode_is_used_by_the_test_programs():
    from sysbio_modeling_amd.project.observables import OP
    seen, powi = set(), set()
    for c in db.all_test_programs().values():
        for sub in c['subprograms']:
            for op, arg in db.walk_program(sub):
                seen.add(op)
                if op == OP['POWI']:
                    powi.add(arg)
    assert seen == set(OP.values())
    assert {0, 1, -1, 2, -3, 64} <= powi
    assert db.program_depth(db.deep_program(16)) == 16 and db.program_depth(db.deep_program(17)) == 17


def test_direct_mode_cases_cover_the_issue_shapes():
    qs, Rs, Gs = set(s[0] for s in ac.SHAPES), set(s[1] for s in ac.SHAPES), set(s[2] for s in ac.SHAPES)
    assert qs == {1, 2, 3, 63, 64, 65, 85, 86, 127, 128, 129, 255, 256, 257, 300, 513}
    assert {1, 2, 255, 256, 257, 700} <= Rs and Gs == {0, 1, 3, 7}
    for q, R, *_ in ac.SHAPES:
        assert ac.row_lanes(q) == 256 // min(q, 256)
    lanes = set((ac.row_lanes(s[0]), s[1]) for s in ac.SHAPES)
    assert any(R == rpp - 1 for rpp, R in lanes) and any(R == rpp for rpp, R in lanes) and any(R == rpp + 1 for rpp, R in lanes)
    assert set(s[3] for s in ac.SHAPES) == {'contiguous', 'interleaved', 'interleaved_gaps', 'single_row', 'one_lane', 'first_last', 'random'}
    assert set((s[4], s[5]) for s in ac.SHAPES) == {(0, 0), (0, 1), (1, 0), (1, 1)} and len(ac.SHAPES) >= 30
