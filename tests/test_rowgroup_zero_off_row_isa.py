"""The all-zero operands of lanes without a row (RL_F_ZERO_OFF_ROW, RowGroupSystem::kZeroOffRow) in the ISA of the
headline kernel, sbm_sens_rowgroup_kernel<cascade20, RG0, DOPRI45>: the default build of the plugin against its
-DSBM_RG_KEEP_F_SELECT=1 twin.  Both are compiled by build(); the code objects are read with the extraction of
tests/test_rowgroup_kernel_isa.py, no GPU.

Measured with this extraction, body of the step loop (six row evaluations, two v_cndmask_b32 of the select each):
    KEEP_F_SELECT (the code before)   833 VALU, 39 v_cndmask_b32
    default                           821 VALU, 27 v_cndmask_b32"""
import os
import shutil

import pytest

from tests.test_rowgroup_handover_isa import VMEM, _code, whole_loop
from tests.test_rowgroup_kernel_isa import KERNEL, LLVM, _count, step_loop

SELECT = ('-DSBM_RG_KEEP_F_SELECT=1',)


def test_no_select_for_lanes_without_a_row(tmp_path):
    if not (shutil.which('objcopy') and os.path.exists(os.path.join(LLVM, 'llvm-objdump'))):
        pytest.skip("needs objcopy and the LLVM binutils of ROCm")
    from sysbio_modeling_amd import build
    from sysbio_modeling_amd.symbolic import zoo_model
    assert 'SBM_PLUGIN_FLAGS' not in os.environ
    default = zoo_model('cascade20').plugin_path(build_if_missing=False)
    if not os.path.exists(default):
        pytest.skip("needs the built cascade20 plugin")
    twin = build.build_plugin('cascade20', os.path.join(build.MODELS_DIR, 'cascade20.hpp'), extra_flags=SELECT)
    bodies = {}
    for tag, plugin in (('default', default), ('select', twin)):
        text, meta = _code(plugin, str(tmp_path / tag))
        bodies[tag] = step_loop(text)
        print(tag, 'vgpr_count', meta[KERNEL]['vgpr_count'], 'vgpr_spill_count', meta[KERNEL]['vgpr_spill_count'],
              'scratch bytes', meta[KERNEL]['private_segment_fixed_size'], '; body VALU', _count(bodies[tag], r'v_'),
              'v_cndmask_b32', _count(bodies[tag], r'v_cndmask_b32'))
        assert _count(whole_loop(text, KERNEL), VMEM) == 0
    assert _count(bodies['default'], r'v_cndmask_b32') <= _count(bodies['select'], r'v_cndmask_b32') - 10
    assert _count(bodies['default'], r'v_') <= _count(bodies['select'], r'v_') - 10
