"""``sbm_choose_kernel`` and ``sbm_kernel_built`` (csrc/sbm_kernel_choice.hpp) on the host: which integrator kernel a call of a
model plugin runs, and which instantiations the plugin contains.  The header is plain C++ on a literal description of the
model (SbmModelTraits), compiled here with g++ and called through ctypes -- no GPU -- and checked against a table written
out by hand from the launcher, branch by branch.

The traits below are written by hand as well: the four committed models, cascade40 (tests/support/erk_cases.py), the ten
tile-edge models (tests/test_tile_edge_layouts_cpu.py), the stiff chains of tests/test_seq_kernel_layouts_cpu.py::EXPECTED
and one synthetic shape on each side of every size limit.  A compile-only probe ties those of michaelis_menten, cascade20
and stiff50 to what sbm_traits_of<SbmModel>() reads from the real headers.  The GPU side: tests/test_gpu_kernel_choice.py
(the launcher prints its choice under SBM_DEBUG_LAUNCH; it must be the one computed here)."""
import ctypes
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sysbio_modeling_amd', 'csrc')
STATE, SENS = 0, 1
METHODS = {'rk4': 0, 'dopri45': 1, 'imid': 2, 'imid_graded': 3, 'imad': 4, 'dop853': 5, 'iex': 6}
EXPLICIT = ('rk4', 'dopri45', 'dop853')
VARIANTS = {'auto': 0, 'per_wave': 1, 'row_lane': 2, 'row_group': 3, 'small_batch': 4, 'mfma': 5, 'packed': 6}
KERNELS = ['NONE', 'PER_WAVE', 'ROW_LANE', 'ROW_GROUP_RG0', 'ROW_GROUP_RG1', 'ROW_GROUP_RG2', 'MFMA', 'SENS_PACKED', 'STATE_LANE',
           'STATE_ROWS', 'STATE_PACKED', 'IMID', 'IMAD', 'IEX', 'IEX_SEQ', 'IEX_SEQ_ROT']
N_TRAJ = (1, 5, 2047, 2048, 20479, 20480, 65535, 65536)

HARNESS = r'''
#include "sbm_kernel_choice.hpp"
static SbmModelTraits traits(const int* v) {
  return SbmModelTraits{v[0], v[1], v[2], v[3] != 0, {v[4], v[5], v[6]}, v[7] != 0, v[8] != 0, v[9] != 0, v[10] != 0, v[11] != 0,
                        v[12] != 0, v[13] != 0, v[14], v[15] != 0, v[16]};
}
extern "C" void choose(const int* tr, int kind, int method, int variant, int step_mult, double rtol, int n_traj, int has_S,
                       int has_s0, int seq_enabled, int* out) {
  sbm_integrator_opts o = {};
  o.method = method; o.variant = variant; o.step_mult = step_mult; o.rtol = rtol;
  const SbmKernelChoice c = sbm_choose_kernel(traits(tr), kind, o, n_traj, has_S != 0, has_s0 != 0, seq_enabled != 0);
  out[0] = c.kernel; out[1] = c.method; out[2] = c.seg; out[3] = c.nch;
}
extern "C" int built(const int* tr, int kernel, int method) { return sbm_kernel_built(traits(tr), kernel, method); }
// one call at `count` batch sizes: kernel, method, seg, nch and whether the plugin contains that kernel for that method
extern "C" void choose_batches(const int* tr, int kind, int method, int variant, int step_mult, double rtol, const int* n_traj,
                               int count, int has_S, int has_s0, int seq_enabled, int* out) {
  for (int i = 0; i < count; ++i) {
    choose(tr, kind, method, variant, step_mult, rtol, n_traj[i], has_S, has_s0, seq_enabled, out + 5 * i);
    out[5 * i + 4] = sbm_kernel_built(traits(tr), out[5 * i], out[5 * i + 1]);
  }
}
extern "C" const char* name(int kernel) { return sbm_kernel_name(kernel); }
extern "C" int kernel_count() { return SBM_K_COUNT; }
// the function is constexpr: a choice is a compile-time constant of a model's traits
constexpr SbmModelTraits kCascade20{20, 40, 40, true, {1, 5, 2}, false, false, false, true, true, true, false, 8, false, 3};
constexpr sbm_integrator_opts kDop853{SBM_DOP853, 0, 0.0, 0.0, 0.0, 0.0, SBM_VARIANT_AUTO, 0};
static_assert(sbm_choose_kernel(kCascade20, SBM_KIND_SENS, kDop853, 4096, true, false, true).kernel == SBM_K_ROW_GROUP_RG2, "");
static_assert(sbm_kernel_built(kCascade20, SBM_K_ROW_GROUP_RG2, SBM_DOP853) && !sbm_kernel_built(kCascade20, SBM_K_ROW_GROUP_RG0, SBM_DOP853), "");
'''


def _traits(nv, nk, nnz_jy, rg_ok, rg_nch, rg_same, imid, imad, iex, iex_seq, kmax, rot_ok, mfma_nch):
    """the fields of SbmModelTraits in their order; rg_nch: RG0, RG1, RG2; rg_same: RG1 is RG0, RG2 is RG0, RG2 is RG1"""
    return (nv, nk, nnz_jy, int(rg_ok)) + tuple(rg_nch) + tuple(int(b) for b in rg_same) + \
        (int(imid), int(imad), int(iex), int(iex_seq), kmax, int(rot_ok), mfma_nch)


def _shape(nv, nk, nnz_jy, rg_ok, rg_nch=(1, 1, 1), rg_same=(True, True, True), implicit=True, mfma_nch=1):
    """a synthetic shape: no chain structure (never the seq kernel)"""
    return _traits(nv, nk, nnz_jy, rg_ok, rg_nch, rg_same, implicit, implicit, implicit, False, 8, False, mfma_nch)


def _chain(kmax):
    """a synthetic chain whose seq kernel is built up to order kmax: what makes the order chosen from rtol visible"""
    return _traits(24, 24, 47, True, (1, 3, 2), (False, False, False), True, True, True, True, kmax, True, 2)


SAME, APART = (True, True, True), (False, False, False)
RG2_IS_RG0 = (False, True, False)
TRAITS = {
    # the committed models
    'michaelis_menten': _traits(2, 5, 3, True, (1, 1, 1), SAME, True, True, True, True, 8, False, 1),
    'simple': _traits(1, 2, 1, False, (1, 1, 1), SAME, True, True, True, True, 8, False, 1),
    'cascade20': _traits(20, 40, 40, True, (1, 5, 2), APART, True, True, True, False, 8, False, 3),
    'stiff50': _traits(50, 50, 99, True, (5, 7, 7), APART, True, True, True, True, 8, True, 4),
    'cascade40': _traits(40, 80, 80, True, (5, 10, 8), APART, True, True, True, False, 8, False, 5),
    # the tile-edge models: five non-zeros per row of df/dy, MFMA_NCH as tests/test_tile_edge_layouts_cpu.py::EXPECTED
    'tile7_16': _traits(7, 16, 35, True, (1, 2, 1), RG2_IS_RG0, True, True, True, False, 8, False, 1),
    'tile16_15': _traits(16, 15, 80, True, (1, 2, 1), RG2_IS_RG0, True, True, True, False, 8, False, 1),
    'tile7_32': _traits(7, 32, 35, True, (1, 4, 1), RG2_IS_RG0, True, True, True, False, 8, False, 1),
    'tile17_14': _traits(17, 14, 85, True, (1, 2, 1), RG2_IS_RG0, True, True, True, False, 8, False, 1),
    'tile16_17': _traits(16, 17, 80, True, (1, 3, 1), RG2_IS_RG0, True, True, True, False, 8, False, 1),
    'tile15_33': _traits(15, 33, 75, True, (1, 5, 2), APART, True, True, True, False, 8, False, 1),
    'tile16_49': _traits(16, 49, 80, False, (1, 1, 1), SAME, True, True, True, False, 8, False, 2),      # no paying split
    'tile33_17': _traits(33, 17, 165, True, (1, 2, 2), APART, True, True, True, False, 8, False, 2),
    'tile49_17': _traits(49, 17, 245, True, (1, 2, 2), APART, True, True, True, False, 8, False, 2),
    'tile64_16': _traits(64, 16, 320, True, (2, 2, 2), SAME, True, True, True, False, 8, False, 1),
    # the stiff chains of tests/test_seq_kernel_layouts_cpu.py::EXPECTED
    'stiff16': _traits(16, 16, 31, True, (1, 2, 1), RG2_IS_RG0, True, True, True, True, 8, False, 1),
    'stiff17': _traits(17, 17, 33, True, (1, 2, 1), RG2_IS_RG0, True, True, True, True, 8, True, 2),
    'stiff24': _traits(24, 24, 47, True, (1, 3, 2), APART, True, True, True, True, 8, True, 2),
    'stiff31': _traits(31, 31, 61, True, (2, 4, 3), APART, True, True, True, True, 8, True, 2),
    'stiff32': _traits(32, 32, 63, True, (2, 4, 3), APART, True, True, True, True, 8, True, 2),
    'stiff33': _traits(33, 33, 65, True, (2, 4, 3), APART, True, True, True, True, 8, False, 3),
    'stiff48': _traits(48, 48, 95, True, (3, 6, 6), APART, True, True, True, True, 8, False, 3),
    'stiff49': _traits(49, 49, 97, True, (3, 6, 6), APART, True, True, True, True, 8, True, 4),
    'stiff64': _traits(64, 64, 127, True, (8, 8, 8), SAME, True, True, True, False, 8, False, 4),
    'stiff16_free': _traits(16, 32, 31, True, (1, 4, 2), APART, True, True, True, True, 8, False, 1),
    'stiff33_free': _traits(33, 66, 65, True, (3, 8, 6), APART, True, True, True, True, 8, False, 5),
    'stiff64_free': _traits(64, 128, 127, True, (11, 16, 11), RG2_IS_RG0, True, True, True, False, 8, False, 8),
    'stiff18_unused_trailing': _traits(18, 19, 35, True, (1, 2, 1), RG2_IS_RG0, True, True, True, True, 8, False, 2),
    'stiff18_unused_leading': _traits(18, 19, 35, True, (1, 2, 1), RG2_IS_RG0, True, True, True, True, 8, False, 2),
    # one synthetic shape on each side of every size limit (no row-group split unless named: the row-lane and per-wave
    # limits are visible only without one)
    'nv32': _shape(32, 7, 64, False),             # 32 x 8 = 256 sensitivity entries: the last packed model
    'nv33': _shape(33, 7, 66, False, mfma_nch=1),
    'nv64': _shape(64, 16, 128, False),
    'nv65': _shape(65, 16, 130, False),
    'nv256': _shape(256, 4, 512, False, implicit=False),
    'nv257': _shape(257, 4, 514, False, implicit=False),
    'entries4096': _shape(64, 63, 128, True, (4, 8, 8), APART, mfma_nch=4),       # 64 x 64
    'entries4097': _shape(17, 240, 34, True, (4, 8, 8), APART, mfma_nch=8),       # 17 x 241
    'density34': _shape(20, 40, 136, True, (1, 5, 2), APART, mfma_nch=3),         # 136 / 400
    'density35': _shape(20, 40, 140, True, (1, 5, 2), APART, mfma_nch=3),         # 140 / 400
    'chain_k4': _chain(4),
    'chain_k6': _chain(6),
}

# (model, kind, method, variant, n_traj[, extras]) -> (kernel, SEG, chunks).  extras: step_mult, rtol, has_S, has_s0,
# seq_enabled (defaults: 0, 0.0, has_S = a sensitivity call, no s0, enabled).
TABLE = [
    # ---- tests/support/erk_cases.py: SENS_CASES (four vectors a call) ----
    (('cascade20', SENS, 'dopri45', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('cascade20', SENS, 'dopri45', 'row_lane', 4), ('ROW_LANE', 0, 1)),
    (('cascade20', SENS, 'dopri45', 'row_group', 4), ('ROW_GROUP_RG0', 0, 1)),
    (('cascade20', SENS, 'dop853', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('cascade20', SENS, 'dop853', 'row_lane', 4), ('ROW_LANE', 0, 1)),
    (('cascade20', SENS, 'dop853', 'row_group', 4), ('ROW_GROUP_RG2', 0, 2)),
    (('cascade20', SENS, 'dopri45', 'small_batch', 4), ('ROW_GROUP_RG1', 0, 5)),
    (('cascade20', SENS, 'dop853', 'small_batch', 4), ('ROW_GROUP_RG1', 0, 5)),
    (('cascade20', SENS, 'dopri45', 'mfma', 4), ('MFMA', 0, 3)),
    (('cascade20', SENS, 'dop853', 'mfma', 4), ('MFMA', 0, 3)),
    (('michaelis_menten', SENS, 'dopri45', 'packed', 4), ('SENS_PACKED', 8, 1)),
    (('michaelis_menten', SENS, 'dopri45', 'row_lane', 4), ('ROW_LANE', 0, 1)),
    (('michaelis_menten', SENS, 'dopri45', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('michaelis_menten', SENS, 'dop853', 'packed', 4), ('SENS_PACKED', 8, 1)),
    (('michaelis_menten', SENS, 'dop853', 'row_lane', 4), ('ROW_LANE', 0, 1)),
    (('michaelis_menten', SENS, 'dop853', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('simple', SENS, 'dopri45', 'packed', 4), ('SENS_PACKED', 4, 1)),
    (('simple', SENS, 'dopri45', 'row_lane', 4), ('ROW_LANE', 0, 1)),
    (('simple', SENS, 'dopri45', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('simple', SENS, 'dop853', 'packed', 4), ('SENS_PACKED', 4, 1)),
    (('simple', SENS, 'dop853', 'row_lane', 4), ('ROW_LANE', 0, 1)),
    (('simple', SENS, 'dop853', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('tile49_17', SENS, 'dopri45', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('tile49_17', SENS, 'dop853', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    (('tile49_17', SENS, 'dopri45', 'mfma', 4), ('MFMA', 0, 2)),
    (('tile49_17', SENS, 'dop853', 'mfma', 4), ('MFMA', 0, 2)),
    (('cascade40', SENS, 'dopri45', 'per_wave', 4), ('PER_WAVE', 0, 1)),
    # ---- STATE_CASES ----
    (('cascade20', STATE, 'dopri45', 'auto', 4), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dop853', 'auto', 4), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'per_wave', 70), ('STATE_LANE', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'auto', 2049), ('STATE_PACKED', 32, 1)),
    (('cascade20', STATE, 'dop853', 'auto', 2049), ('STATE_PACKED', 32, 1)),
    (('michaelis_menten', STATE, 'dopri45', 'auto', 2049), ('STATE_PACKED', 16, 1)),
    (('michaelis_menten', STATE, 'dop853', 'auto', 2049), ('STATE_PACKED', 16, 1)),
    # ---- BUDGET_CASES (one vector a call) ----
    (('cascade20', SENS, 'dopri45', 'row_group', 1), ('ROW_GROUP_RG0', 0, 1)),
    (('cascade20', SENS, 'dop853', 'row_lane', 1), ('ROW_LANE', 0, 1)),
    (('michaelis_menten', SENS, 'dopri45', 'packed', 1), ('SENS_PACKED', 8, 1)),
    (('tile49_17', SENS, 'dopri45', 'per_wave', 1), ('PER_WAVE', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'auto', 1), ('STATE_ROWS', 0, 1)),
    # ---- tests/test_gpu_dop853.py::test_reference_fixture_models, tests/test_gpu_parity.py (packed against unpacked) ----
    (('simple', SENS, 'dop853', 'auto', 3), ('SENS_PACKED', 4, 1)),
    (('michaelis_menten', SENS, 'dop853', 'auto', 3), ('SENS_PACKED', 8, 1)),
    (('simple', STATE, 'dop853', 'auto', 3), ('STATE_ROWS', 0, 1)),
    (('michaelis_menten', STATE, 'dop853', 'auto', 3), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'auto', 4096), ('STATE_PACKED', 32, 1)),
    (('cascade20', STATE, 'dopri45', 'row_lane', 4096), ('STATE_ROWS', 0, 1)),
    (('michaelis_menten', STATE, 'dopri45', 'auto', 3003), ('STATE_PACKED', 16, 1)),
    (('michaelis_menten', STATE, 'rk4', 'row_lane', 3003), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'auto', 100), ('STATE_ROWS', 0, 1)),
    # ---- tests/test_gpu_tile_edges.py: CASES (RK4, five vectors), and what AUTO runs for the same models ----
    (('tile7_16', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 1)),
    (('tile16_15', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 1)),
    (('tile7_32', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 1)),
    (('tile17_14', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 1)),
    (('tile16_17', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 1)),
    (('tile15_33', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 1)),
    (('tile16_49', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 2)),
    (('tile33_17', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 2)),
    (('tile49_17', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 2)),
    (('tile64_16', SENS, 'rk4', 'mfma', 5), ('MFMA', 0, 1)),
    (('tile7_16', SENS, 'rk4', 'packed', 5), ('SENS_PACKED', 16, 1)),
    (('tile16_15', SENS, 'rk4', 'packed', 5), ('SENS_PACKED', 16, 1)),
    (('tile7_32', SENS, 'rk4', 'packed', 5), ('SENS_PACKED', 32, 1)),
    (('tile17_14', SENS, 'rk4', 'packed', 5), ('SENS_PACKED', 32, 1)),
    (('tile7_16', SENS, 'dopri45', 'auto', 5), ('SENS_PACKED', 16, 1)),
    (('tile17_14', SENS, 'dopri45', 'auto', 5), ('SENS_PACKED', 32, 1)),
    (('tile16_17', SENS, 'dopri45', 'auto', 5), ('ROW_GROUP_RG0', 0, 1)),       # 16 x 18 = 288 entries: not packed
    (('tile15_33', SENS, 'dopri45', 'auto', 5), ('ROW_GROUP_RG0', 0, 1)),
    (('tile16_49', SENS, 'dopri45', 'auto', 5), ('ROW_LANE', 0, 1)),            # no row-group split
    (('tile16_49', SENS, 'dopri45', 'row_group', 5), ('PER_WAVE', 0, 1)),       # ... a forced one: per-wave
    (('tile64_16', SENS, 'dopri45', 'auto', 5), ('ROW_GROUP_RG0', 0, 2)),
    (('tile64_16', SENS, 'dop853', 'auto', 5), ('ROW_GROUP_RG2', 0, 2)),
    # ---- tests/test_seq_kernel_layouts_cpu.py: EXPECTED (default order: 8 at the default tolerance) ----
    (('stiff16', SENS, 'iex', 'auto', 3), ('IEX_SEQ', 0, 1)),
    (('stiff17', SENS, 'iex', 'auto', 3), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff24', SENS, 'iex', 'auto', 3), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff31', SENS, 'iex', 'auto', 3), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff32', SENS, 'iex', 'auto', 3), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff33', SENS, 'iex', 'auto', 3), ('IEX_SEQ', 0, 1)),
    (('stiff48', SENS, 'iex', 'auto', 3), ('IEX_SEQ', 0, 1)),
    (('stiff49', SENS, 'iex', 'auto', 3), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff64', SENS, 'iex', 'auto', 3), ('IEX', 0, 1)),
    (('stiff16_free', SENS, 'iex', 'auto', 3), ('IEX_SEQ', 0, 1)),
    (('stiff33_free', SENS, 'iex', 'auto', 3), ('IEX_SEQ', 0, 2)),              # 66 columns: two chunks of 64
    (('stiff64_free', SENS, 'iex', 'auto', 3), ('IEX', 0, 2)),
    (('stiff18_unused_trailing', SENS, 'iex', 'auto', 3), ('IEX_SEQ', 0, 1)),
    (('stiff18_unused_leading', SENS, 'iex', 'auto', 3), ('IEX_SEQ', 0, 1)),
    # the other inputs of that decision: given initial sensitivities, an order above 8, the developer switch, no S
    (('stiff50', SENS, 'iex', 'auto', 3), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff50', SENS, 'iex', 'auto', 3, dict(has_s0=True)), ('IEX_SEQ', 0, 1)),
    (('stiff50', SENS, 'iex', 'auto', 3, dict(step_mult=8)), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff50', SENS, 'iex', 'auto', 3, dict(step_mult=9)), ('IEX', 0, 1)),
    (('stiff50', SENS, 'iex', 'auto', 3, dict(seq_enabled=False)), ('IEX', 0, 1)),
    (('stiff50', STATE, 'iex', 'auto', 3), ('IEX_SEQ_ROT', 0, 1)),
    (('stiff33_free', STATE, 'iex', 'auto', 3), ('IEX_SEQ', 0, 1)),             # state only: one chunk
    (('stiff50', SENS, 'imad', 'auto', 3), ('IMAD', 0, 1)),
    (('stiff50', SENS, 'imid', 'auto', 3), ('IMID', 0, 1)),
    (('stiff50', SENS, 'imid_graded', 'auto', 3), ('IMID', 0, 1)),
    (('cascade40', SENS, 'imid', 'auto', 3), ('IMID', 0, 2)),
    (('cascade40', SENS, 'imad', 'auto', 3), ('IMAD', 0, 2)),
    (('nv256', SENS, 'iex', 'auto', 3), ('NONE', 0, 1)),
    (('nv256', SENS, 'imad', 'auto', 3), ('NONE', 0, 1)),
    (('nv256', STATE, 'imid', 'auto', 3), ('NONE', 0, 1)),
    # the order chosen from rtol when step_mult <= 0: 4 from 1e-4, 6 from 1e-6, else 8 (rtol <= 0: 1e-8)
    (('chain_k4', SENS, 'iex', 'auto', 3, dict(rtol=1e-4)), ('IEX_SEQ_ROT', 0, 1)),
    (('chain_k4', SENS, 'iex', 'auto', 3, dict(rtol=0.99e-4)), ('IEX', 0, 1)),
    (('chain_k4', SENS, 'iex', 'auto', 3, dict(rtol=1e-4, step_mult=5)), ('IEX', 0, 1)),
    (('chain_k4', SENS, 'iex', 'auto', 3, dict(rtol=1e-9, step_mult=4)), ('IEX_SEQ_ROT', 0, 1)),
    (('chain_k6', SENS, 'iex', 'auto', 3, dict(rtol=0.99e-4)), ('IEX_SEQ_ROT', 0, 1)),
    (('chain_k6', SENS, 'iex', 'auto', 3, dict(rtol=1e-6)), ('IEX_SEQ_ROT', 0, 1)),
    (('chain_k6', SENS, 'iex', 'auto', 3, dict(rtol=0.99e-6)), ('IEX', 0, 1)),
    (('chain_k6', SENS, 'iex', 'auto', 3, dict(rtol=0.0)), ('IEX', 0, 1)),
    (('chain_k6', SENS, 'iex', 'auto', 3, dict(rtol=-1.0, step_mult=-1)), ('IEX', 0, 1)),
    # ---- the 35 % density rule: AUTO and SMALL_BATCH take the matrix cores from there, DOP853 never by itself ----
    (('density34', SENS, 'dopri45', 'auto', 5), ('ROW_GROUP_RG0', 0, 1)),
    (('density35', SENS, 'dopri45', 'auto', 5), ('MFMA', 0, 3)),
    (('density35', SENS, 'rk4', 'auto', 5), ('MFMA', 0, 3)),
    (('density34', SENS, 'dopri45', 'small_batch', 5), ('ROW_GROUP_RG1', 0, 5)),
    (('density35', SENS, 'dopri45', 'small_batch', 5), ('MFMA', 0, 3)),
    (('density35', SENS, 'dop853', 'auto', 5), ('ROW_GROUP_RG2', 0, 2)),
    (('density35', SENS, 'dop853', 'mfma', 5), ('MFMA', 0, 3)),
    (('density35', SENS, 'dopri45', 'row_group', 5), ('ROW_GROUP_RG0', 0, 1)),
    (('density35', STATE, 'dopri45', 'auto', 5), ('STATE_ROWS', 0, 1)),
    # ---- state kernels: 2048, and the lane kernel from 20480 (up to 32 state variables) or 65536 ----
    (('cascade20', STATE, 'dopri45', 'auto', 2047), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'auto', 2048), ('STATE_PACKED', 32, 1)),
    (('cascade20', STATE, 'rk4', 'auto', 2048), ('STATE_PACKED', 20, 1)),
    (('michaelis_menten', STATE, 'rk4', 'auto', 2048), ('STATE_PACKED', 4, 1)),
    (('cascade20', STATE, 'dopri45', 'row_lane', 2048), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'row_group', 65536), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'small_batch', 2048), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'per_wave', 5), ('STATE_LANE', 0, 1)),
    (('cascade20', STATE, 'dop853', 'per_wave', 5), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'auto', 20479), ('STATE_PACKED', 32, 1)),
    (('cascade20', STATE, 'dopri45', 'auto', 20480), ('STATE_LANE', 0, 1)),
    (('cascade20', STATE, 'dop853', 'auto', 20480), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'mfma', 20479), ('STATE_ROWS', 0, 1)),
    (('cascade20', STATE, 'dopri45', 'mfma', 20480), ('STATE_LANE', 0, 1)),
    (('simple', STATE, 'dopri45', 'auto', 2048), ('STATE_ROWS', 0, 1)),         # one state variable: nothing to pack
    (('simple', STATE, 'dopri45', 'auto', 20480), ('STATE_LANE', 0, 1)),
    (('stiff50', STATE, 'dopri45', 'auto', 2048), ('STATE_ROWS', 0, 1)),
    (('stiff50', STATE, 'dopri45', 'auto', 20480), ('STATE_ROWS', 0, 1)),
    (('stiff50', STATE, 'dopri45', 'auto', 65535), ('STATE_ROWS', 0, 1)),
    (('stiff50', STATE, 'dopri45', 'auto', 65536), ('STATE_LANE', 0, 1)),
    (('stiff50', STATE, 'dop853', 'auto', 65536), ('STATE_ROWS', 0, 1)),
    # ---- the small-batch split: RG1 while n_traj x its chunks <= 2048, only on request, only where it is another split ----
    (('cascade20', SENS, 'dopri45', 'small_batch', 409), ('ROW_GROUP_RG1', 0, 5)),      # 2045
    (('cascade20', SENS, 'dopri45', 'small_batch', 410), ('ROW_GROUP_RG0', 0, 1)),      # 2050
    (('cascade20', SENS, 'dop853', 'small_batch', 409), ('ROW_GROUP_RG1', 0, 5)),
    (('cascade20', SENS, 'dop853', 'small_batch', 410), ('ROW_GROUP_RG2', 0, 2)),
    (('tile7_16', SENS, 'dopri45', 'small_batch', 1024), ('ROW_GROUP_RG1', 0, 2)),      # 2048 exactly
    (('tile7_16', SENS, 'dopri45', 'small_batch', 1025), ('ROW_GROUP_RG0', 0, 1)),
    (('cascade20', SENS, 'dopri45', 'auto', 1), ('ROW_GROUP_RG0', 0, 1)),
    (('stiff50', SENS, 'dopri45', 'small_batch', 292), ('ROW_GROUP_RG1', 0, 7)),        # 2044
    (('stiff50', SENS, 'dopri45', 'small_batch', 293), ('ROW_GROUP_RG0', 0, 5)),        # 2051
    (('tile64_16', SENS, 'dopri45', 'small_batch', 1), ('ROW_GROUP_RG0', 0, 2)),        # RG1 is RG0
    (('michaelis_menten', SENS, 'dopri45', 'small_batch', 1), ('ROW_GROUP_RG0', 0, 1)),
    (('simple', SENS, 'dopri45', 'small_batch', 1), ('ROW_LANE', 0, 1)),
    # ---- a forced MFMA / PACKED that does not take the model falls to the row kernels ----
    (('cascade20', SENS, 'dopri45', 'packed', 5), ('ROW_GROUP_RG0', 0, 1)),             # 40 columns: not packed
    (('cascade20', SENS, 'dop853', 'packed', 5), ('ROW_GROUP_RG2', 0, 2)),
    (('tile16_49', SENS, 'dopri45', 'packed', 5), ('ROW_LANE', 0, 1)),
    (('nv65', SENS, 'dopri45', 'mfma', 5), ('PER_WAVE', 0, 1)),                         # 65 rows: neither MFMA nor row-lane
    (('nv65', SENS, 'dopri45', 'packed', 5), ('PER_WAVE', 0, 1)),
    (('entries4097', SENS, 'dopri45', 'packed', 5), ('ROW_GROUP_RG0', 0, 4)),
    (('michaelis_menten', SENS, 'dopri45', 'auto', 5), ('SENS_PACKED', 8, 1)),
    (('michaelis_menten', SENS, 'dopri45', 'mfma', 5), ('MFMA', 0, 1)),                 # forced: any model up to 64 rows
    (('michaelis_menten', SENS, 'dopri45', 'row_group', 5), ('ROW_GROUP_RG0', 0, 1)),
    # ---- size limits, both sides ----
    # 32 / 33 state variables: packed (sensitivity and state), DOP853 on the row-lane kernel
    (('nv32', SENS, 'dopri45', 'auto', 5), ('SENS_PACKED', 32, 1)),
    (('nv33', SENS, 'dopri45', 'auto', 5), ('ROW_LANE', 0, 1)),
    (('nv32', SENS, 'dop853', 'row_lane', 5), ('ROW_LANE', 0, 1)),
    (('nv33', SENS, 'dop853', 'row_lane', 5), ('PER_WAVE', 0, 1)),
    (('nv32', SENS, 'dop853', 'row_group', 5), ('ROW_LANE', 0, 1)),                     # DOP853: anything but PER_WAVE
    (('nv32', SENS, 'dop853', 'per_wave', 5), ('PER_WAVE', 0, 1)),
    (('nv32', STATE, 'dopri45', 'auto', 2048), ('STATE_PACKED', 32, 1)),
    (('nv33', STATE, 'dopri45', 'auto', 2048), ('STATE_ROWS', 0, 1)),
    (('nv32', STATE, 'dopri45', 'auto', 20480), ('STATE_LANE', 0, 1)),
    (('nv33', STATE, 'dopri45', 'auto', 20480), ('STATE_ROWS', 0, 1)),
    (('nv33', STATE, 'dopri45', 'auto', 65536), ('STATE_LANE', 0, 1)),
    # 64 / 65: MFMA, row-lane, the per-wave kernel with DOP853, the state lane kernel
    (('nv64', SENS, 'dopri45', 'mfma', 5), ('MFMA', 0, 1)),
    (('nv64', SENS, 'dopri45', 'auto', 5), ('ROW_LANE', 0, 1)),
    (('nv65', SENS, 'dopri45', 'auto', 5), ('PER_WAVE', 0, 1)),
    (('nv65', SENS, 'dopri45', 'row_lane', 5), ('PER_WAVE', 0, 1)),
    (('nv64', SENS, 'dop853', 'auto', 5), ('PER_WAVE', 0, 1)),                          # 64 elements per lane: the last
    (('nv65', SENS, 'dop853', 'auto', 5), ('NONE', 0, 1)),
    (('nv65', SENS, 'dop853', 'mfma', 5), ('NONE', 0, 1)),
    (('cascade40', SENS, 'dop853', 'per_wave', 5), ('NONE', 0, 1)),                     # 40 rows x 2 columns per lane
    (('cascade40', SENS, 'dop853', 'row_lane', 5), ('NONE', 0, 1)),
    (('cascade40', SENS, 'dop853', 'auto', 5), ('ROW_GROUP_RG2', 0, 8)),
    (('nv64', STATE, 'dopri45', 'per_wave', 5), ('STATE_LANE', 0, 1)),
    (('nv65', STATE, 'dopri45', 'per_wave', 5), ('STATE_ROWS', 0, 1)),
    (('nv64', STATE, 'dopri45', 'auto', 65536), ('STATE_LANE', 0, 1)),
    (('nv65', STATE, 'dopri45', 'auto', 65536), ('STATE_ROWS', 0, 1)),
    # 256 / 257: the state rows kernel; beyond it the lane kernel, which has no DOP853
    (('nv256', STATE, 'dopri45', 'auto', 5), ('STATE_ROWS', 0, 1)),
    (('nv256', STATE, 'dop853', 'per_wave', 5), ('STATE_ROWS', 0, 1)),
    (('nv257', STATE, 'dopri45', 'auto', 5), ('STATE_LANE', 0, 1)),
    (('nv257', STATE, 'dopri45', 'row_lane', 5), ('STATE_LANE', 0, 1)),
    (('nv257', STATE, 'dop853', 'auto', 5), ('NONE', 0, 1)),
    # 4096 / 4097 sensitivity entries with a row-group split: the per-wave kernel is not built beyond, variant is a no-op
    (('entries4096', SENS, 'dopri45', 'per_wave', 5), ('PER_WAVE', 0, 1)),
    (('entries4097', SENS, 'dopri45', 'per_wave', 5), ('ROW_GROUP_RG0', 0, 4)),
    (('entries4096', SENS, 'dopri45', 'row_lane', 5), ('ROW_LANE', 0, 1)),
    (('entries4097', SENS, 'dopri45', 'row_lane', 5), ('ROW_GROUP_RG0', 0, 4)),
    (('entries4097', SENS, 'dop853', 'per_wave', 5), ('ROW_GROUP_RG2', 0, 8)),
    (('entries4096', SENS, 'dop853', 'per_wave', 5), ('PER_WAVE', 0, 1)),
    (('entries4096', SENS, 'dop853', 'row_lane', 5), ('PER_WAVE', 0, 1)),               # 64 rows: no row-lane DOP853
    # a method the plugin does not know runs as RK4; a kind it does not know is a state call
    (('cascade20', SENS, 7, 'auto', 5), ('ROW_GROUP_RG0', 0, 1)),
    (('cascade20', 2, 'dopri45', 'auto', 5), ('STATE_ROWS', 0, 1)),
]

# kernel -> the explicit methods it is instantiated for, per model (spot checks of sbm_kernel_built; the sweep covers the rest)
BUILT = [
    ('cascade20', 'PER_WAVE', EXPLICIT), ('cascade20', 'ROW_LANE', EXPLICIT), ('cascade20', 'ROW_GROUP_RG0', ('rk4', 'dopri45')),
    ('cascade20', 'ROW_GROUP_RG1', EXPLICIT), ('cascade20', 'ROW_GROUP_RG2', EXPLICIT), ('cascade20', 'MFMA', EXPLICIT),
    ('cascade20', 'SENS_PACKED', ()), ('cascade20', 'STATE_LANE', ('rk4', 'dopri45')), ('cascade20', 'STATE_ROWS', EXPLICIT),
    ('cascade20', 'STATE_PACKED', EXPLICIT), ('cascade20', 'NONE', ()),
    ('michaelis_menten', 'ROW_GROUP_RG0', EXPLICIT), ('michaelis_menten', 'SENS_PACKED', EXPLICIT),
    ('tile16_17', 'ROW_GROUP_RG0', EXPLICIT),       # RG2 is RG0
    ('simple', 'ROW_GROUP_RG0', ()), ('simple', 'ROW_GROUP_RG2', ()), ('simple', 'STATE_PACKED', ()), ('simple', 'PER_WAVE', EXPLICIT),
    ('stiff50', 'ROW_LANE', ('rk4', 'dopri45')), ('stiff50', 'PER_WAVE', EXPLICIT), ('stiff50', 'STATE_PACKED', ()),
    ('cascade40', 'PER_WAVE', ('rk4', 'dopri45')), ('cascade40', 'ROW_LANE', ()),
    ('entries4097', 'PER_WAVE', ()), ('entries4096', 'PER_WAVE', EXPLICIT),
    ('nv65', 'MFMA', ()), ('nv65', 'STATE_LANE', ()), ('nv64', 'STATE_LANE', ('rk4', 'dopri45')), ('nv257', 'STATE_LANE', ('rk4', 'dopri45')),
    ('nv257', 'STATE_ROWS', ()), ('nv256', 'STATE_ROWS', EXPLICIT),
]
IMPLICIT_BUILT = {
    'cascade20': ('IMID', 'IMAD', 'IEX'), 'stiff50': ('IMID', 'IMAD', 'IEX', 'IEX_SEQ', 'IEX_SEQ_ROT'),
    'stiff16': ('IMID', 'IMAD', 'IEX', 'IEX_SEQ'), 'nv256': (),
}


def build_harness(directory):
    """compile the harness round the header into ``directory`` and return it as a ctypes library"""
    src, so = os.path.join(str(directory), 'harness.cpp'), os.path.join(str(directory), 'harness.so')
    with open(src, 'w') as fh:
        fh.write(HARNESS)
    subprocess.run(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wall', '-Wextra', '-Werror', '-I', CSRC, src, '-o', so],
                   check=True, capture_output=True)
    lib = ctypes.CDLL(so)
    ints = ctypes.POINTER(ctypes.c_int)
    lib.choose.argtypes = [ints] + [ctypes.c_int] * 4 + [ctypes.c_double] + [ctypes.c_int] * 4 + [ints]
    lib.choose_batches.argtypes = [ints] + [ctypes.c_int] * 4 + [ctypes.c_double, ints] + [ctypes.c_int] * 4 + [ints]
    lib.built.argtypes = [ints, ctypes.c_int, ctypes.c_int]
    lib.name.argtypes = [ctypes.c_int]
    lib.name.restype = ctypes.c_char_p
    return lib


def choose(lib, model, kind, method, variant, n_traj, step_mult=0, rtol=0.0, has_S=None, has_s0=False, seq_enabled=True):
    """(kernel name, method, SEG, chunks) of a call"""
    tr = (ctypes.c_int * 17)(*TRAITS[model])
    out = (ctypes.c_int * 4)()
    lib.choose(tr, kind, METHODS.get(method, method), VARIANTS.get(variant, variant), step_mult, rtol, n_traj,
               int(kind == SENS if has_S is None else has_S), int(has_s0), int(seq_enabled), out)
    return (lib.name(out[0]).decode(),) + tuple(out)[1:]


def is_built(lib, model, kernel, method):
    return bool(lib.built((ctypes.c_int * 17)(*TRAITS[model]), KERNELS.index(kernel), METHODS.get(method, method)))


def choose_batches(lib, model, kind, method, variant, sizes, step_mult=0, rtol=0.0, has_S=None, has_s0=False, seq_enabled=True):
    """[(kernel name, method, SEG, chunks, the plugin contains it)] of one call at every batch size of ``sizes``"""
    tr = (ctypes.c_int * 17)(*TRAITS[model])
    out = (ctypes.c_int * (5 * len(sizes)))()
    lib.choose_batches(tr, kind, METHODS.get(method, method), VARIANTS.get(variant, variant), step_mult, rtol,
                       (ctypes.c_int * len(sizes))(*sizes), len(sizes), int(kind == SENS if has_S is None else has_S), int(has_s0),
                       int(seq_enabled), out)
    return [(lib.name(out[5 * i]).decode(), out[5 * i + 1], out[5 * i + 2], out[5 * i + 3], bool(out[5 * i + 4]))
            for i in range(len(sizes))]


def launch_line(lib, model, kind, method, variant, n_traj):
    """what the launcher prints for the call under SBM_DEBUG_LAUNCH"""
    kernel, m, seg, nch = choose(lib, model, kind, method, variant, n_traj)
    return 'launch choice: %s method %d nch %d SEG %d, %d trajectories' % (kernel, m, nch, seg, n_traj)


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp('kernel_choice'))


def test_names_of_the_enum(lib):
    assert lib.kernel_count() == len(KERNELS)
    assert [lib.name(k).decode() for k in range(len(KERNELS))] == KERNELS
    assert lib.name(-1) == b'?' and lib.name(len(KERNELS)) == b'?'


def _id(call):
    return '-'.join(str(c) for c in call[:5]) + ('' if len(call) == 5 else '-' + '-'.join('%s=%s' % kv for kv in sorted(call[5].items())))


def test_table_has_no_call_twice_and_both_sides_of_every_threshold():
    calls = [_id(c) for c, _ in TABLE]
    assert len(set(calls)) == len(calls)
    have = {c[:5] for c, _ in TABLE}
    for a, b in ((2047, 2048), (20479, 20480)):
        assert ('cascade20', STATE, 'dopri45', 'auto', a) in have and ('cascade20', STATE, 'dopri45', 'auto', b) in have
    assert ('stiff50', STATE, 'dopri45', 'auto', 65535) in have and ('stiff50', STATE, 'dopri45', 'auto', 65536) in have
    # n_traj x RG1's chunks on both sides of 2048
    for model, (a, b) in (('cascade20', (409, 410)), ('stiff50', (292, 293))):
        nch1 = TRAITS[model][5]
        assert a * nch1 <= 2048 < b * nch1 and b == a + 1
        assert (model, SENS, 'dopri45', 'small_batch', a) in have and (model, SENS, 'dopri45', 'small_batch', b) in have
    assert TRAITS['tile7_16'][5] * 1024 == 2048 and ('tile7_16', SENS, 'dopri45', 'small_batch', 1024) in have and \
        ('tile7_16', SENS, 'dopri45', 'small_batch', 1025) in have
    # the synthetic shapes sit where their names say
    nv, nk = TRAITS['entries4096'][:2]
    assert nv * (nk + 1) == 4096
    nv, nk = TRAITS['entries4097'][:2]
    assert nv * (nk + 1) == 4097
    for name, pays in (('density34', False), ('density35', True)):
        nv, _, nnz = TRAITS[name][:3]
        assert (nnz * 100 >= 35 * nv * nv) == pays and nnz * 100 // (nv * nv) == int(name[-2:])
    assert TRAITS['nv32'][0] * (TRAITS['nv32'][1] + 1) == 256
    for n in (32, 33, 64, 65, 256, 257):
        assert TRAITS['nv%d' % n][0] == n
    # every model of the GPU matrices that name a kernel
    from tests.test_tile_edge_layouts_cpu import EXPECTED as TILE, PACKED
    from tests.test_seq_kernel_layouts_cpu import EXPECTED as SEQ
    for name, row in TILE.items():
        assert TRAITS[name][:3] == (row[0], row[1], 5 * row[0]) and TRAITS[name][16] == row[5]
        assert (name, SENS, 'rk4', 'mfma', 5) in have and ((name, SENS, 'rk4', 'packed', 5) in have) == (name in PACKED)
    for name in SEQ:
        assert (name, SENS, 'iex', 'auto', 3) in have


def test_table_names_the_kernels_the_gpu_matrices_name(lib):
    """tests/test_seq_kernel_layouts_cpu.py::EXPECTED and the plans of tests/test_tile_edge_layouts_cpu.py::EXPECTED"""
    from tests.test_tile_edge_layouts_cpu import EXPECTED as TILE
    from tests.test_seq_kernel_layouts_cpu import EXPECTED as SEQ
    want = {c[:5]: w for c, w in TABLE if len(c) == 5}
    for name, layout in SEQ.items():
        assert want[(name, SENS, 'iex', 'auto', 3)][0] == {'rot': 'IEX_SEQ_ROT', 'plain': 'IEX_SEQ', None: 'IEX'}[layout]
    for name, (nv, nk, packed, rt, ct, nch, ldj, lda, auto) in TILE.items():
        assert want[(name, SENS, 'rk4', 'mfma', 5)] == ('MFMA', 0, nch)
        if packed is not None:
            assert want[(name, SENS, 'rk4', 'packed', 5)] == ('SENS_PACKED', packed[0], 1)
        got = choose(lib, name, SENS, 'dopri45', 'auto', 5)[0]
        assert (got == 'SENS_PACKED') == (auto == 'packed') and got != 'MFMA'
        assert auto == 'packed' or got in ('ROW_GROUP_RG0', 'ROW_LANE')


@pytest.mark.parametrize('call,want', TABLE, ids=[_id(c) for c, _ in TABLE])
def test_choice(lib, call, want):
    model, kind, method, variant, n_traj = call[:5]
    extras = call[5] if len(call) > 5 else {}
    kernel, m, seg, nch = choose(lib, model, kind, method, variant, n_traj, **extras)
    assert (kernel, seg, nch) == want
    code = METHODS.get(method, method)
    assert m == (code if code in (1, 2, 3, 4, 5, 6) else 0)


@pytest.mark.parametrize('model,kernel,methods', BUILT, ids=['%s-%s' % b[:2] for b in BUILT])
def test_built(lib, model, kernel, methods):
    assert tuple(m for m in EXPLICIT if is_built(lib, model, kernel, m)) == tuple(methods)


@pytest.mark.parametrize('model', list(IMPLICIT_BUILT))
def test_built_implicit(lib, model):
    assert tuple(k for k in KERNELS[11:] if is_built(lib, model, k, 'iex')) == IMPLICIT_BUILT[model]


def _flag_sets(method):
    on_off = [dict(has_S=s, has_s0=z, seq_enabled=q) for s in (False, True) for z in (False, True) for q in (False, True)]
    if method in EXPLICIT:
        return on_off
    return [dict(f, step_mult=k, rtol=r) for f in on_off for k, r in ((0, 0.0), (0, 1e-4), (4, 0.0), (9, 0.0))]


@pytest.mark.parametrize('model', list(TRAITS))
def test_every_choice_is_a_kernel_the_plugin_contains_and_batch_size_moves_it_only_where_documented(lib, model):
    """All kinds x methods x variants x batch sizes x flags.  (1) The choice is NONE -- the launcher answers
    hipErrorInvalidConfiguration -- or a kernel sbm_kernel_built says the plugin contains, for the method the choice
    names: no call reaches a kernel that is not instantiated, and none leaves the launcher without a launch or an error.
    (2) The batch size moves the choice only where the launcher says it does: state calls (2048, 20480 / 65536) and the
    opt-in SMALL_BATCH.  A sensitivity call with any other variant runs one kernel whatever the batch ("a given model
    always runs the same kernel"), and so does every call of an implicit method."""
    nch_rg1 = TRAITS[model][5]
    for kind in (STATE, SENS):
        for method in METHODS:
            for variant in VARIANTS:
                first = None
                for flags in _flag_sets(method):
                    got = choose_batches(lib, model, kind, method, variant, N_TRAJ, **flags)
                    for kernel, m, seg, nch, built in got:
                        assert kernel == 'NONE' or built, (kind, method, variant, flags, kernel)
                        assert m == METHODS[method] and nch >= 1
                        assert (seg > 0) == (kernel in ('SENS_PACKED', 'STATE_PACKED'))
                    if method not in EXPLICIT or (kind == SENS and variant != 'small_batch'):
                        assert len(set(got)) == 1, (kind, method, variant, flags, got)
                    elif kind == SENS:
                        # SMALL_BATCH: the small-batch split while it pays, else one other kernel
                        assert got[-1][0] != 'ROW_GROUP_RG1'
                        assert set(got) <= {got[-1], ('ROW_GROUP_RG1', METHODS[method], 0, nch_rg1, True)}, got
                    else:
                        assert {c[0] for c in got} <= {'STATE_LANE', 'STATE_ROWS', 'STATE_PACKED', 'NONE'}
                        assert variant == 'auto' or not any(c[0] == 'STATE_PACKED' for c in got)
                    if method in EXPLICIT:
                        # the flags belong to the implicit methods
                        first = first or got
                        assert got == first


_TRAITS_PROBE = r'''
#include "sbm_integrators.hpp"
#include SBM_MODEL_HEADER
constexpr SbmModelTraits t = sbm_traits_of<SbmModel>();
constexpr int want[17] = {EXPECT};
static_assert(t.NV == want[0] && t.NK == want[1] && t.NNZ_JY == want[2], "sizes");
static_assert(t.RG_OK == (want[3] != 0) && t.RG_NCH[0] == want[4] && t.RG_NCH[1] == want[5] && t.RG_NCH[2] == want[6], "row-group splits");
static_assert(t.RG1_IS_RG0 == (want[7] != 0) && t.RG2_IS_RG0 == (want[8] != 0) && t.RG2_IS_RG1 == (want[9] != 0), "splits that are one type");
static_assert(t.IMID_FITS == (want[10] != 0) && t.IMAD_FITS == (want[11] != 0) && t.IEX_FITS == (want[12] != 0), "implicit kernels");
static_assert(t.IEX_SEQ_FITS == (want[13] != 0) && t.IEX_SEQ_KMAX == want[14] && t.IEX_SEQ_ROT_OK == (want[15] != 0), "seq kernel");
static_assert(t.MFMA_NCH == want[16], "matrix-core chunks");
'''


@pytest.mark.parametrize('name', ['michaelis_menten', 'cascade20', 'stiff50'])
def test_hand_written_traits_are_those_of_the_committed_headers(name, tmp_path):
    """sbm_traits_of<SbmModel>() on the real header against TRAITS, by the compiler alone (-fsyntax-only: no code generated)"""
    from sysbio_modeling_amd import build
    try:
        hipcc = build.hipcc_path()
    except build.BuildError:
        pytest.skip("needs hipcc")
    probe = tmp_path / 'probe.hip'
    probe.write_text(_TRAITS_PROBE)
    p = subprocess.run([hipcc, '--offload-arch=gfx950', '-std=c++17', '-fsyntax-only', '-I' + build.CSRC_DIR,
                        '-I' + os.path.join(build.REPO_DIR, 'include'),
                        '-DSBM_MODEL_HEADER="%s"' % os.path.join(build.MODELS_DIR, name + '.hpp'),
                        '-DEXPECT=%s' % ','.join(str(v) for v in TRAITS[name]), str(probe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
