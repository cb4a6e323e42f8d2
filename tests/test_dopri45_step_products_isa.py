"""The step loop of the headline kernel after sbm_dopri45 folded the step size into the tableau (the products hs * a_ij are
formed per stage and every stage argument is one FMA chain seeded with z: no multiply opens a sum, no FMA scales it
afterwards), counted in the ISA of the built plugin with the extraction of tests/test_rowgroup_kernel_isa.py (no GPU needed).

Five VALU instructions per element and step go, 15 elements per lane; about 19 wave-uniform v_mul_f64 come.  Measured with
this extraction on sbm_sens_rowgroup_kernel<cascade20, RG0, DOPRI45>:

    each finished sum scaled by hs:   1175 instructions, 974 VALU, 127 v_mul_f64, 595 v_fma_f64, 6 v_rcp_f64, 148 ds_*, 0 vector-memory
    products per stage:               1114 instructions, 918 VALU,  71 v_mul_f64, 595 v_fma_f64, 6 v_rcp_f64, 148 ds_*, 0 vector-memory

The bound leaves 12 instructions for scheduling differences between compiler patch levels, not for a partial
implementation (one stage left unfolded costs 15).
"""
import os
import re
import shutil

import pytest

from tests.test_rowgroup_kernel_isa import LLVM, REPO, disassemble, loop_counts, step_loop

VALU_BOUND = 930


def test_step_loop_of_the_headline_kernel_without_the_scaling_fma(tmp_path):
    plugin = os.path.join(REPO, 'sysbio_modeling_amd', '_build', 'sbm_model_cascade20.so')
    if not (os.path.exists(plugin) and shutil.which('objcopy') and os.path.exists(os.path.join(LLVM, 'llvm-objdump'))):
        pytest.skip("needs the built cascade20 plugin and the LLVM binutils of ROCm")
    body = step_loop(disassemble(plugin, str(tmp_path)))
    c = loop_counts(body)
    c['mul64'] = sum(1 for ln in body if re.match(r'v_mul_f64', ln))
    c['fma64'] = sum(1 for ln in body if re.match(r'v_fmac?_f64', ln))
    print(c)
    assert c['vmem'] == 0, [ln for ln in body if re.match(r'(scratch_|global_|buffer_|flat_)', ln)]
    assert c['rcp64'] == 6, c
    assert c['valu'] <= VALU_BOUND, c
