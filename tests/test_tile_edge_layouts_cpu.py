"""Which instantiation of sbm_sens_mfma_kernel and sbm_sens_packed_kernel each model of models_zoo.tile_edge_specs()
compiles, the structure of those models, and the fixed-step reference the GPU tests compare with.  No GPU needed.

Both kernels choose their lane layout from the model's size at compile time.  The plan is recomputed here in Python from
the formulas in the comments of csrc/sbm_sens_mfma.hpp (SbmMfmaShared, SbmMfmaPlan) and csrc/sbm_kernel_choice.hpp
(sbm_choose_kernel), on NV / NK / NNZ_JY read from the generated header, and held against the literal table EXPECTED: the
evidence of which instantiation each test of tests/test_gpu_tile_edges.py addresses.

  MFMA     RT = ceil(NV / 16) row tiles, CT = min(ceil(NK / 16), max(1, 12 / (4 RT))) column tiles per wavefront,
           NCH = ceil(NK / (16 CT)) wavefronts per trajectory, MP = 16 RT, LDJ = MP if MP % 32 == 16 else MP + 16,
           NC = 16 CT, LDA = NC if NC % 32 == 16 else NC + 16
  packed   NV <= 32, NK <= 32, NV (NK + 1) <= 256; SEG = 4 / 8 / 16 / 32 >= max(NV, NK), 64 / SEG trajectories per wavefront
  AUTO     (DOPRI45, RK4) MFMA where 16 <= NV <= 64 and NNZ_JY >= 35 % of NV^2, else packed where eligible, else the row
           kernels.  The tile-edge family has five non-zeros per row of df/dy (cheap to derive and to compile): AUTO takes
           MFMA for none of its models, the GPU tests force it.

The fixed-step reference is oracle/rk4_oracle.py, pinned here: fourth-order convergence to the tight solution, and the
compiled C right-hand side against the generated Python one -- two evaluations of the same expressions whose difference,
relative to each column's largest entry, is the rounding level rho of the problem at the GPU tests' step partition.
Measured (largest over five vectors of tile_edge_ensemble, T_OUT, H0 below; printed by test_rounding_level_of_every_model):

  tile7_16 1.64e-16   tile16_15 2.08e-16   tile7_32 1.99e-16   tile17_14 1.15e-16   tile16_17 2.18e-16
  tile15_33 2.02e-16  tile16_49 2.18e-16   tile33_17 1.61e-16  tile49_17 1.41e-16   tile64_16 1.88e-16

RHO_MAX below is the largest of them rounded up to two digits, 2.2e-16; the GPU tests' bound is 8 RHO_MAX = 1.76e-15."""
import re
from collections import OrderedDict

import numpy as np
import pytest
import sympy

from sysbio_modeling_amd import models_zoo

# ---- the GPU tests' fixed-step problem: 3 output times after t0, dyadic times and step (dt / h0 is an exact integer) ----
T_OUT = np.array([0.0, 1.0, 2.0, 3.0])
H0 = 1.0 / 128.0           # 128 steps per output interval
# the largest rounding level over the matrix (module docstring), rounded up
RHO_MAX = 2.2e-16
RK4_BOUND = 8 * RHO_MAX

# name: (NV, NK, packed (SEG, trajectories per wavefront) or None, RT, CT, NCH, LDJ, LDA, what AUTO runs)
EXPECTED = OrderedDict([
    ('tile7_16',  (7, 16, (16, 4), 1, 1, 1, 16, 16, 'packed')),     # NK == SEG, exactly one column tile
    ('tile16_15', (16, 15, (16, 4), 1, 1, 1, 16, 16, 'packed')),    # NV == SEG (256 entries: the limit), a phantom column
    ('tile7_32',  (7, 32, (32, 2), 1, 2, 1, 16, 48, 'packed')),     # NK == SEG, two full column tiles
    ('tile17_14', (17, 14, (32, 2), 2, 1, 1, 48, 16, 'packed')),    # NV > NK, one row in the second row tile
    ('tile16_17', (16, 17, None, 1, 2, 1, 16, 48, 'row')),          # second column tile one column wide
    ('tile15_33', (15, 33, None, 1, 3, 1, 16, 48, 'row')),          # three column tiles, three error sums
    ('tile16_49', (16, 49, None, 1, 3, 2, 16, 48, 'row')),          # second chunk: one column and two empty tiles
    ('tile33_17', (33, 17, None, 3, 1, 2, 48, 16, 'row')),          # RT 3
    ('tile49_17', (49, 17, None, 4, 1, 2, 80, 16, 'row')),          # RT 4: 16 elements per lane, one wavefront per SIMD
    ('tile64_16', (64, 16, None, 4, 1, 1, 80, 16, 'row')),          # every lane has a row
])
NAMES = list(EXPECTED)
PACKED = [n for n in NAMES if EXPECTED[n][2] is not None]


def matrix_specs():
    """the models of tests/test_gpu_tile_edges.py, by name (the same list build() compiles)"""
    return OrderedDict((s.name, s) for s in models_zoo.tile_edge_specs())


_GM = {}


def generated(name):
    if name not in _GM:
        from sysbio_modeling_amd.symbolic import GeneratedModel
        _GM[name] = GeneratedModel(matrix_specs()[name])
    return _GM[name]


def params_of(name, n_vec, seed=5):
    return models_zoo.tile_edge_ensemble(matrix_specs()[name], n_vec, seed=seed)


def header_sizes(text):
    return tuple(int(re.search(r'static constexpr int %s = (\d+);' % key, text).group(1)) for key in ('NV', 'NK', 'NNZ_JY'))


def mfma_plan(nv, nk, max_el=12):
    rt = (nv + 15) // 16
    ct_all = (nk + 15) // 16
    ct_fit = max(1, max_el // (4 * rt))
    ct = min(ct_all, ct_fit)
    nch = (nk + 16 * ct - 1) // (16 * ct)
    mp, nc = 16 * rt, 16 * ct
    return rt, ct, nch, (mp if mp % 32 == 16 else mp + 16), (nc if nc % 32 == 16 else nc + 16)


def packed_plan(nv, nk):
    if not (nv <= 32 and nk <= 32 and nv * (nk + 1) <= 256):
        return None
    need = max(nv, nk)
    seg = 4 if need <= 4 else (8 if need <= 8 else (16 if need <= 16 else 32))
    return seg, 64 // seg


def auto_choice(nv, nk, nnz_jy):
    if 16 <= nv <= 64 and nnz_jy * 100 >= 35 * nv * nv:
        return 'mfma'
    return 'packed' if packed_plan(nv, nk) is not None else 'row'


def test_matrix_is_the_list_build_compiles():
    assert list(matrix_specs()) == NAMES
    assert [(s.n_vars, s.n_sens) for s in models_zoo.tile_edge_specs()] == list(models_zoo.TILE_EDGE_SHAPES)


@pytest.mark.parametrize('name', NAMES)
def test_plan_of_each_model_from_its_header(name):
    nv, nk, nnz = header_sizes(generated(name).hip_source)
    spec = matrix_specs()[name]
    assert (nv, nk) == (spec.n_vars, spec.n_sens) and nnz == 5 * nv
    got = (nv, nk, packed_plan(nv, nk)) + mfma_plan(nv, nk) + (auto_choice(nv, nk, nnz),)
    assert got == EXPECTED[name], (name, got)
    # every model runs the MFMA kernel when forced (one state row per lane) and the row-lane kernel of the comparison
    assert nv <= 64 and nk <= 64


def test_random_networks_under_auto():
    """tests/test_gpu_user_models.py::test_random_networks_all_variants adds variant='auto' for its 6- and 11-state networks:
    rand6_1 (13 columns) is packed under AUTO, SEG 16, four per wavefront; rand11_2 (24 columns) would need SEG 32 but has
    11 x 25 = 275 entries, over the packed kernel's 256 -- AUTO runs it on the row kernels (below 16 states: never MFMA).
    Sizes as the generated header states them, the ones the launcher is compiled with."""
    from sysbio_modeling_amd.symbolic import GeneratedModel
    from tests.test_gpu_user_models import _random_network
    want = {(1, 6): (6, 13, (16, 4), 'packed'), (2, 11): (11, 24, None, 'row')}
    for (seed, n), (nv_w, nk_w, plan_w, auto_w) in want.items():
        spec = _random_network(seed, n)
        nv, nk, nnz = header_sizes(GeneratedModel(spec).hip_source)
        print("%s: header NV %d NK %d NNZ_JY %d" % (spec.name, nv, nk, nnz))
        assert (nv, nk) == (spec.n_vars, spec.n_sens) == (nv_w, nk_w) and nv <= nnz <= nv * nv
        assert packed_plan(nv, nk) == plan_w and auto_choice(nv, nk, nnz) == auto_w, spec.name
    assert 11 * (24 + 1) == 275 > 256


# ---- structure of the family ----
def _dependencies(spec):
    eqs = [sympy.sympify(spec.equations[v]) for v in spec.variables]
    return [set(str(s) for s in e.free_symbols) for e in eqs]


@pytest.mark.parametrize('name', NAMES)
def test_structure_of_the_free_columns(name):
    spec = matrix_specs()[name]
    n, k = spec.n_vars, spec.n_sens
    rt = (n + 15) // 16
    deps = _dependencies(spec)
    assert len(spec.params) == len(set(spec.params)) and len(spec.sens_params) == k
    assert max(len([p for p in spec.params if p in d]) for d in deps) <= 5        # parameters per row
    # every 16 x 16 block of df/dy has a non-zero, five per row
    jy = [[j for j in range(n) if 'x%d' % j in deps[i]] for i in range(n)]
    assert all(len(r) == 5 and i in r for i, r in enumerate(jy))
    assert {(i // 16, j // 16) for i in range(n) for j in jy[i]} == {(a, b) for a in range(rt) for b in range(rt)}
    # J_p: rows of every free column
    rows = [[i for i in range(n) if p in deps[i]] for p in spec.sens_params]
    # no sensitivity column is structurally zero: it has a J_p entry, and df/dy couples every state to every other
    assert all(rows)
    reach = np.eye(n, dtype=bool)
    adj = np.array([[j in jy[i] for j in range(n)] for i in range(n)])
    for _ in range(n):
        reach = reach | ((reach.astype(int) @ adj.astype(int)) > 0)
    assert reach.all()
    # every 16-column tile, a partial last one included, has J_p entries in more than one row tile
    for c0 in range(0, k, 16):
        tiles = {r // 16 for c in range(c0, min(c0 + 16, k)) for r in rows[c]}
        assert rt == 1 or len(tiles) > 1, (name, c0, tiles)


# ---- the fixed-step reference ----
@pytest.mark.parametrize('name', ['tile7_16', 'tile16_49', 'tile49_17'])
def test_rk4_oracle_converges_at_fourth_order(name):
    from oracle import odeint_oracle as oo, rk4_oracle
    gm = generated(name)
    n, k = gm.n_vars, gm.n_sens
    p = params_of(name, 1)[0]
    tight = oo.tight_solution(gm, p, T_OUT, use_c=True, atol=1e-30)
    err = [rk4_oracle.colmax_err(rk4_oracle.integrate(gm, p, T_OUT, H0 * 32, step_mult=m), tight, n, k) for m in (1, 2, 4)]
    print("%s: RK4 oracle vs tight solution at h, h/2, h/4: %.3g %.3g %.3g (ratios %.1f %.1f)"
          % (name, err[0], err[1], err[2], err[0] / err[1], err[1] / err[2]))
    # fourth order: 16 per halving (the next term of the expansion moves the ratio by a few units at these steps)
    assert 11.0 <= err[0] / err[1] <= 24.0 and 11.0 <= err[1] / err[2] <= 24.0
    assert err[2] > 1e-11          # truncation, not rounding, is what was measured
    # the partition is the contract's: step_mult * ceil(dt / h0) steps per interval
    assert rk4_oracle.steps_per_interval(T_OUT, H0) == [128, 128, 128]
    assert rk4_oracle.steps_per_interval([0.0, 0.5, 1.5, 3.0], 1.0 / 32.0) == [16, 32, 48]
    assert rk4_oracle.steps_per_interval([0.0, 0.5, 1.5, 3.0], 0.4, step_mult=2) == [4, 6, 8]
    assert rk4_oracle.steps_per_interval([0.0, 1.0], 0.3) == [4]


def test_the_comparison_lets_nothing_through():
    """colmax_err is what the GPU tests hold against RK4_BOUND: a NaN or inf the kernel stored anywhere -- in the state, in
    a sensitivity, in a column that is zero throughout -- is inf, never a small number; an error counts against its own
    column's largest entry, not the matrix's; a zero column must match exactly."""
    from oracle.rk4_oracle import colmax_err
    n, k, T = 3, 4, 2
    ref = np.ones((T, n + n * k))
    ref[:, n + 2::k] = 1e-6                 # sensitivity column 2 is small
    ref[:, n + 3::k] = 0.0                  # sensitivity column 3 is zero throughout
    assert colmax_err(ref.copy(), ref, n, k) == 0.0
    places = {'Y': (1, 1), 'S': (1, n + 1 * k + 1), 'S, last entry': (T - 1, n + n * k - 1), 'small column': (0, n + 2),
              'zero column': (1, n + 2 * k + 3)}
    for what, (t, j) in places.items():
        for bad in (np.nan, np.inf, -np.inf):
            a = ref.copy()
            a[t, j] = bad
            assert colmax_err(a, ref, n, k) == float('inf'), (what, bad)
    for t, j in places.values():            # and in the reference
        r = ref.copy()
        r[t, j] = np.nan
        assert colmax_err(ref.copy(), r, n, k) == float('inf')
    a = ref.copy()
    a[:] = np.nan
    assert colmax_err(a, ref, n, k) == float('inf')
    # relative to the entry's own column
    a = ref.copy()
    a[1, 0] += 1e-9
    assert colmax_err(a, ref, n, k) == pytest.approx(1e-9, rel=1e-6)
    a = ref.copy()
    a[0, n + 1 * k + 2] += 1e-9             # 1e-9 in the column whose largest entry is 1e-6
    assert colmax_err(a, ref, n, k) == pytest.approx(1e-3, rel=1e-6)
    a = ref.copy()
    a[1, n + 3] = 1e-300                    # anything in the zero column
    assert colmax_err(a, ref, n, k) == float('inf')
    a = ref.copy()
    a[0, n + 0 * k + 1], a[1, n + 2 * k + 1] = 1.0 + 1e-12, 1.0 - 3e-12      # the worst entry, not the first
    assert colmax_err(a, ref, n, k) == pytest.approx(3e-12, rel=1e-3)
    with pytest.raises(ValueError):
        colmax_err(ref[:, :-1], ref, n, k)


@pytest.mark.parametrize('name', NAMES)
def test_rounding_level_of_every_model(name):
    """C against Python right-hand side at the GPU tests' partition: rho, the figure RHO_MAX bounds (module docstring)."""
    from oracle import rk4_oracle
    gm = generated(name)
    n, k = gm.n_vars, gm.n_sens
    rho = 0.0
    for p in params_of(name, 5):          # the five vectors of the GPU tests
        a = rk4_oracle.integrate(gm, p, T_OUT, H0, use_c=True)
        b = rk4_oracle.integrate(gm, p, T_OUT, H0, use_c=False)
        rho = max(rho, rk4_oracle.colmax_err(b, a, n, k))
        assert np.all(np.abs(a[-1, n:]).reshape(n, k).max(axis=0) > 0.0)       # no zero column
    print("%s: rounding level rho = %.2e" % (name, rho))
    # RHO_MAX is a measurement (largest value 2.18e-16, 1 % below it), not a property of the project: rho depends on the
    # libm, on numpy and on how the C compiler contracts the oracle's right-hand side.  A failure here says nothing about
    # the kernels.
    assert 0.0 < rho <= RHO_MAX, (
        "%s: rho = %.3g exceeds RHO_MAX = %.3g.  No defect of the project: the rounding level was measured with another "
        "libm / numpy / C compiler.  Measure rho again for all ten models (pytest -s prints them), set RHO_MAX to the "
        "largest rounded up, and write the new values and 8 RHO_MAX into this module's docstring, that of "
        "tests/test_gpu_tile_edges.py and docs/history.md." % (name, rho, RHO_MAX))
