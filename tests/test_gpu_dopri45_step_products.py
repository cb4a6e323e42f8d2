"""sbm_dopri45 forms its stage arguments from the products hs * a_ij (hs = the step size AFTER it was clipped to land on
an output time), recomputed for every attempted step.  The shapes at which that can go wrong and the other tests are thin:

  * nearly every step clipped (a dense output grid): products formed from the unclipped h would land past the target;
  * first attempts rejected (h0 = the whole time span): the products of the retry must come from the new step size;
  * the other instantiations of the shared driver (per-wave, row-lane, packed kernels of the two small models);
  * row-group against per-wave on the headline model.

The oracle side of the first two cases was run on its own beforehand: for all 8 vectors the reference's LSODA result is
within 0.24 (dense grid) / 0.04 (three output times) tolerance units (1e-8 |ref| + 5e-9) of a tight DOP853 solution, so
the reference alone leaves the kernel at least three quarters of the tolerance and no vector is left out.
"""
import numpy as np
import pytest

from tests.conftest import check_parity, parity_err

pytestmark = pytest.mark.gpu

N_VEC = 8


@pytest.fixture(scope='module')
def cascade(zoo):
    from sysbio_modeling_amd import models_zoo
    gm = zoo('cascade20')
    _, P = models_zoo.cascade_ensemble(N_VEC)
    return gm, P


def _check_against_oracle(gm, P, t, Y, S, what):
    """Every vector on its own (none hides behind another's scale) against the reference's LSODA, with a tight solution
    to arbitrate where that fails (conftest.check_parity; the tight solution is only computed then)."""
    from oracle import odeint_oracle as oo
    n = gm.n_vars
    for v, p in enumerate(P):
        Sr, Yr = oo.calc_jacobian(gm, p, t, use_c=True, return_states=True)
        cache = []

        def tight(part, p=p, cache=cache):
            if not cache:
                cache.append(oo.tight_solution(gm, p, t, use_c=True))
            return cache[0][:, :n] if part == 'Y' else cache[0][:, n:]
        ey = check_parity(Y[v], Yr, lambda: tight('Y'), what='%s, vector %d, states' % (what, v))
        es = check_parity(S[v], Sr, lambda: tight('S'), what='%s, vector %d, sensitivities' % (what, v))
        print(what, 'vector', v, 'state err', ey, 'sens err', es)


def test_nearly_every_step_clipped_to_an_output_time(gpu_models, cascade):
    """201 output times on [0, 100]: the controller's proposal (several time units once the transient is over) is cut
    to target - t at almost every step, so the stage arguments are built from a step size other than h throughout."""
    gm, P = cascade
    m = gpu_models('cascade20')
    t = np.linspace(0.0, 100.0, 201)
    S, Y = m.calc_jacobian_batch(P, t, return_states=True, method='dopri45')
    assert m.last_info['status'].tolist() == [0] * N_VEC
    print('accepted', m.last_info['n_steps'].tolist(), 'rejected', m.last_info['n_rejected'].tolist())
    assert np.all(m.last_info['n_steps'] >= 200)          # at least one step per output interval
    _check_against_oracle(gm, P, t, Y, S, 'dense grid')


def test_products_follow_the_step_size_through_rejections(gpu_models, cascade):
    """h0 = the whole time span: the first attempts fail the error test and are retried with a smaller step, whose
    products must be the new ones."""
    gm, P = cascade
    m = gpu_models('cascade20')
    t = np.array([0.0, 50.0, 100.0])
    S, Y = m.calc_jacobian_batch(P, t, return_states=True, method='dopri45', h0=float(t[-1] - t[0]))
    print('accepted', m.last_info['n_steps'].tolist(), 'rejected', m.last_info['n_rejected'].tolist())
    assert m.last_info['status'].tolist() == [0] * N_VEC
    assert np.all(m.last_info['n_rejected'] > 0), m.last_info['n_rejected']
    _check_against_oracle(gm, P, t, Y, S, 'rejected first steps')


@pytest.mark.parametrize('variant', ['per_wave', 'row_lane', 'packed'])
@pytest.mark.parametrize('name,file', [('simple', 'simple_ref.npz'), ('michaelis_menten', 'mm_ref.npz')])
def test_other_instantiations_of_the_driver_on_the_goldens(gpu_models, golden, name, file, variant):
    """The per-wave, row-lane and packed kernels of the small models (sensitivity and state-only entry points), 4
    vectors (the golden's two, twice), against the trajectories of the real reference OdeModel at the tolerance the
    other tests of these goldens use."""
    m = gpu_models(name)
    g = golden(file)
    P = np.concatenate([g['P'], g['P']])
    S, Y2 = m.calc_jacobian_batch(P, g['t'], return_states=True, method='dopri45', variant=variant)
    assert m.last_info['status'].tolist() == [0] * 4
    Y = m.simulate_batch(P, g['t'], method='dopri45', variant=variant)
    assert m.last_info['status'].tolist() == [0] * 4
    for v in range(4):
        errs = (parity_err(Y[v], g['Y'][v % 2]), parity_err(Y2[v], g['Y'][v % 2]), parity_err(S[v], g['S'][v % 2]))
        print(name, variant, 'vector', v, 'state-only / state / sens err', errs)
        assert max(errs) <= 1.0, errs


def test_row_group_and_per_wave_still_agree(gpu_models, golden):
    """cascade20, the golden's 4 vectors: both kernels fold the step size, each in its own element layout; they differ
    by rounding only (the bounds of test_gpu_parity.test_kernel_variants_agree)."""
    m = gpu_models('cascade20')
    g = golden('cascade20_ref.npz')
    t_out = np.concatenate([[0.0], g['t'][g['idx']]])
    res = {}
    for variant in ('per_wave', 'row_group'):
        S, Y = m.calc_jacobian_batch(g['P'], t_out, return_states=True, method='dopri45', variant=variant)
        assert m.last_info['status'].tolist() == [0] * 4
        assert parity_err(Y[:, 1:], g['Y']) <= 1.0 and parity_err(S[:, 1:], g['S']) <= 1.0
        res[variant] = (Y, S, m.last_info['n_steps'].copy())
    (Ya, Sa, na), (Yb, Sb, nb) = res['per_wave'], res['row_group']
    print('max |dY|', np.max(np.abs(Ya - Yb)), 'max |dS|', np.max(np.abs(Sa - Sb)), 'steps', na.tolist(), nb.tolist())
    assert np.allclose(Ya, Yb, rtol=1e-9, atol=1e-11) and np.allclose(Sa, Sb, rtol=1e-9, atol=1e-10)
    assert np.all(np.abs(na - nb) <= 2)
