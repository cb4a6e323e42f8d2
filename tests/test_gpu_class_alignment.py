"""The row kernels on aligned class slots (emit_rowlane.py::choose_alignment), on the GPU.

The alignment re-numbers the operand slots (SBM_RL_YS / PS) and the output slots (JYOUT, JYCOL, APOS, JPCOL, RG*_JYPOS,
rl_static, apply_lds, the MFMA tile image, IM_MFPOS / IM_DIAGSLOT) of every row kernel; tests/test_class_alignment.py
checks ``class_dispatch`` through the row-lane tables on the host, this file runs the kernels that read the other tables:
every case against the live oracle (LSODA at the reference's tolerances; a vector more than one unit off must pass the
arbitration of tests/conftest.py::check_parity against a tight solution -- no vector is left out), at the smallest
shapes at which a slot can go wrong.  The cascade20 variants are also compared with SBM_VARIANT_PER_WAVE, the kernel
that does not use ``class_dispatch``: two results that are each within one parity unit of the solution are within two
of each other."""
import numpy as np
import pytest

from tests.conftest import check_parity, parity_err

pytestmark = pytest.mark.gpu

GRID = np.linspace(0, 100.0, 1000)
IDX = np.array([0, 333, 999])            # t = 0 and two output times beyond it


def _oracle(gm, P, grid=GRID, idx=IDX):
    """per vector: (LSODA [Y | S] at the output times, tight solution on demand)"""
    from oracle import odeint_oracle as oo
    gm.c_library()
    out = []
    for p in P:
        S, Y = oo.calc_jacobian(gm, p, grid, use_c=True, return_states=True)
        tight = lambda p=p: oo.tight_solution(gm, p, grid[idx], use_c=True, atol=1e-30)[1:]     # noqa: E731
        out.append((np.concatenate([Y[idx[1:]], S[idx[1:]]], axis=1), tight))
    return out


def _check_all(S, Y, ref, what):
    for v, (lsoda, tight) in enumerate(ref):
        n_t = Y.shape[1]
        gpu = np.concatenate([Y[v, 1:].reshape(n_t - 1, -1), S[v, 1:].reshape(n_t - 1, -1)], axis=1)
        check_parity(gpu, lsoda, tight, what='%s, vector %d' % (what, v))


@pytest.fixture(scope='module')
def cascade20(gpu_models, zoo):
    from sysbio_modeling_amd import models_zoo
    _, P = models_zoo.cascade_ensemble(8)
    m = gpu_models('cascade20')
    ref = _oracle(zoo('cascade20'), P)
    S, Y = m.calc_jacobian_batch(P, GRID[IDX], return_states=True, variant='per_wave')
    assert not m.last_info['status'].any()
    return m, P, ref, (S, Y)


@pytest.mark.parametrize('variant,method', [('row_group', 'dopri45'), ('row_group', 'dop853'), ('row_lane', 'dopri45'),
                                            ('small_batch', 'dopri45')])
def test_cascade20_row_kernels(cascade20, variant, method):
    m, P, ref, (S_pw, Y_pw) = cascade20
    S, Y = m.calc_jacobian_batch(P, GRID[IDX], return_states=True, variant=variant, method=method)
    assert not m.last_info['status'].any()
    _check_all(S, Y, ref, 'cascade20 %s %s' % (variant, method))
    ey, es = parity_err(Y, Y_pw), parity_err(S, S_pw)
    print('%s %s vs per_wave: state %.3f sens %.3f parity units' % (variant, method, ey, es))
    assert ey <= 2.0 and es <= 2.0


def test_per_wave_kernel_itself(cascade20):
    m, P, ref, (S_pw, Y_pw) = cascade20
    _check_all(S_pw, Y_pw, ref, 'cascade20 per_wave')


def test_michaelis_menten_packed(gpu_models, zoo):
    from tests import reference_cases as rc
    rng = np.random.default_rng(11)
    P = rc.MM_PARAMS[None, :] * np.exp(0.3 * rng.standard_normal((8, len(rc.MM_PARAMS))))
    m = gpu_models('michaelis_menten')
    ref = _oracle(zoo('michaelis_menten'), P)
    S, Y = m.calc_jacobian_batch(P, GRID[IDX], return_states=True, variant='packed')
    assert not m.last_info['status'].any()
    _check_all(S, Y, ref, 'michaelis_menten packed')


@pytest.fixture(scope='module')
def rand30():
    from sysbio_modeling_amd.symbolic import GeneratedModel
    from sysbio_modeling_amd.model import OdeModel
    from tests.test_gpu_user_models import _random_network
    gm = GeneratedModel(_random_network(4, 30))
    m = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=gm.spec.name)
    rng = np.random.default_rng(104)
    P = np.exp(rng.uniform(np.log(0.2), np.log(2.0), (4, len(gm.param_order))))
    grid = np.linspace(0, 20.0, 1000)
    return m, P, grid, _oracle(gm, P, grid)


@pytest.mark.parametrize('variant', ['row_group', 'mfma'])
def test_random_network(rand30, variant):
    m, P, grid, ref = rand30
    S, Y = m.calc_jacobian_batch(P, grid[IDX], return_states=True, variant=variant)
    assert not m.last_info['status'].any()
    _check_all(S, Y, ref, 'rand30_4 %s' % variant)


def test_unequal_slot_counts_through_the_user_model_path():
    """tests/test_class_alignment.py::_unequal_spec: classes of three, two and one J_y entries, the two-entry rows out of
    column order, an operand slot left unused"""
    from sysbio_modeling_amd.symbolic import GeneratedModel
    from sysbio_modeling_amd.model import OdeModel
    from tests.test_class_alignment import _unequal_spec
    gm = GeneratedModel(_unequal_spec())
    assert gm.derived.align is not None
    m = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=gm.spec.name)
    rng = np.random.default_rng(7)
    P = np.exp(rng.uniform(np.log(0.3), np.log(1.5), (4, len(gm.param_order))))
    grid = np.linspace(0, 30.0, 1000)
    ref = _oracle(gm, P, grid)
    variants = ['auto', 'row_lane', 'per_wave'] + (['row_group'] if gm.rowgroup_chunks() else [])
    for variant in variants:
        S, Y = m.calc_jacobian_batch(P, grid[IDX], return_states=True, variant=variant)
        assert not m.last_info['status'].any(), variant
        _check_all(S, Y, ref, 'unequal7 %s' % variant)


def test_stiff50_fixed_step_implicit_kernel(gpu_models, zoo):
    """IM_MFPOS / IM_DIAGSLOT / IM_JPQ on aligned slots: 300 steps of the fixed-step kernel against the dense numpy
    restatement of the scheme (tolerances of tests/test_gpu_implicit.py::test_kernel_equals_scheme_oracle)"""
    from oracle import imid_oracle
    from sysbio_modeling_amd import models_zoo
    gm, m = zoo('stiff50'), gpu_models('stiff50')
    P = models_zoo.stiff_ensemble(2)[1]
    t_out = np.array([0.0, 2.2, 6.0])
    S, Y = m.calc_jacobian_batch(P, t_out, return_states=True, h0=0.02, method='implicit_midpoint', rtol=1e-10, atol=1e-12)
    assert m.last_info['status'].tolist() == [0, 0]
    for v in range(2):
        Yo, So, ns, nn = imid_oracle.integrate(gm, P[v], t_out[1:], 0.02)
        assert m.last_info['n_steps'][v] == ns
        assert np.allclose(Y[v, 1:], Yo, rtol=1e-9, atol=1e-12)
        assert np.allclose(S[v, 1:], So, rtol=1e-8, atol=1e-10 * np.abs(So).max())


def test_cascade70_two_state_rows_per_lane():
    from sysbio_modeling_amd import models_zoo
    from sysbio_modeling_amd.model import OdeModel
    from sysbio_modeling_amd.symbolic import GeneratedModel
    gm = GeneratedModel(models_zoo.cascade_spec(70, name='cascade70'))
    m = OdeModel(gm.model, gm.sens_model, gm.n_vars, gm.param_order, model_name=gm.spec.name)
    rng = np.random.default_rng(2026)
    P = models_zoo.cascade_nominal_params(70)[None, :] * np.exp(0.3 * rng.standard_normal((2, 140)))
    grid = np.linspace(0, 30.0, 1000)
    ref = _oracle(gm, P, grid)
    S, Y = m.calc_jacobian_batch(P, grid[IDX], return_states=True)
    assert not m.last_info['status'].any()
    _check_all(S, Y, ref, 'cascade70')


def test_a_nan_error_still_rejects_the_step(cascade20):
    """a pin of the controller: a NaN parameter makes every stage NaN, the error estimate is NaN, the step is rejected and
    the vector reports a failure -- its neighbours do not.  (It does not tell the one-instruction max(|z|, |zt|) of the
    error norm from fmax: the scale is never the deciding operand here.)"""
    import warnings
    m, P, ref, _ = cascade20
    bad = P.copy()
    bad[3, 5] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        S, Y = m.calc_jacobian_batch(bad, GRID[IDX], return_states=True, variant='row_group')
    status = m.last_info['status']
    assert status[3] != 0 and not np.delete(status, 3).any()
    good = [v for v in range(len(P)) if v != 3]
    _check_all(S[good], Y[good], [ref[v] for v in good], 'cascade20 next to a NaN vector')
