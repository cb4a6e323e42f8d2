"""The per-stage operand hand-over of the row-group kernels (SBM_RG_EARLY_STAGES, csrc/sbm_kernels_rowgroup.hpp) in the ISA:
the default build of a plugin against its -DSBM_RG_EARLY_STAGES=0 twin (every stage fetches its operands in finish).
Both are compiled by build(); the code objects are read with the extraction of tests/test_rowgroup_kernel_isa.py, no GPU.

A stage that fetches early issues its 14 ds_read_b128 of A / JYL at the end of eval, so the stage argument is formed while
they are in flight: MORE VALU instructions lie between the last of those reads and the s_waitcnt that drains them than in
the mask-0 build of the same stage.  LDS instructions return in order, so the wait that drains a read is the first one
after it whose lgkmcnt is at most the number of LDS instructions issued since.

Measured with this extraction (cascade20, <RG0, DOPRI45>), VALU under the fetch in stages 2 ... 7:
    mask 0                    2,  5,  4, 11, 26,  4      loop body 837 VALU, vgpr_spill_count 24
    default, stages 2 3 4 7  13,  7, 19, 11, 22, 69      loop body 833 VALU, vgpr_spill_count 32
    all six stages (0xFC)    13,  7, 24,  4, 16,  9      (stages 5 and 6: the compiler forms the argument above the fetch)"""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_rowgroup_kernel_isa import KERNEL, LLVM, _count, disassemble, step_loop

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK0 = ('-DSBM_RG_EARLY_STAGES=0',)
VMEM = r'(scratch_|global_|buffer_|flat_)'
STAGES = (2, 3, 4, 5, 6, 7)              # the six stages inside the loop body, in program order
OPERAND_READS = 14                       # ds_read_b128 per stage of cascade20 / RG0: 7 of JYL, 7 of A


def _tools():
    return shutil.which('objcopy') and os.path.exists(os.path.join(LLVM, 'llvm-objdump'))


def _plugins(name):
    """(default build, mask-0 build) of a zoo model's plugin, as build() left them"""
    from sysbio_modeling_amd import build
    from sysbio_modeling_amd.symbolic import zoo_model
    header = os.path.join(build.MODELS_DIR, name + '.hpp')
    assert 'SBM_PLUGIN_FLAGS' not in os.environ
    return zoo_model(name).plugin_path(), build.build_plugin(name, header, extra_flags=MASK0)


def _code(plugin, tmp):
    """(disassembly, {kernel: metadata text}) of a plugin's gfx950 code object"""
    os.makedirs(tmp, exist_ok=True)
    text = disassemble(plugin, tmp)
    notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', os.path.join(tmp, 'dev.co')], check=True,
                           stdout=subprocess.PIPE, text=True).stdout
    meta = {}
    for blk in notes.split('- .agpr_count')[1:]:
        meta[re.search(r'\.name:\s+(\S+)', blk).group(1)] = {
            k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
            for k in ('vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size')}
    return text, meta


def whole_loop(text, kernel):
    """every instruction of the step loop (step_loop() returns its longest branch-free run): among the backward
    branches of the kernel, the span with the most fp64 arithmetic"""
    m = re.search(r'^([0-9a-f]+) <%s>:\n(.*?)(?=^[0-9a-f]+ <|\Z)' % re.escape(kernel), text, re.S | re.M)
    assert m, kernel
    base, insts = int(m.group(1), 16), []
    for ln in m.group(2).splitlines():
        mm = re.match(r'\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):', ln)
        if mm:
            tgt = re.search(r'<[^>+]+\+0x([0-9a-f]+)>\s*$', ln) if mm.group(1).startswith(('s_cbranch', 's_branch')) else None
            insts.append((int(mm.group(2), 16), mm.group(1), base + int(tgt.group(1), 16) if tgt else None))
    index_of = {a: i for i, (a, _, _) in enumerate(insts)}
    loop = []
    for i, (addr, _, tgt) in enumerate(insts):
        if tgt is not None and tgt <= addr and tgt in index_of:
            body = [t for _, t, _ in insts[index_of[tgt]:i + 1]]
            if _count(body, r'v_(fma|fmac|mul|add)_f64') > _count(loop, r'v_(fma|fmac|mul|add)_f64'):
                loop = body
    assert loop, kernel
    return loop


def valu_under_the_operand_fetch(body):
    """per stage: VALU instructions between the last of its 14 operand reads and the wait that drains it"""
    assert _count(body, r's_(load|buffer_load)') == 0          # (scalar loads would share lgkmcnt and return out of order)
    reads = [i for i, ln in enumerate(body) if ln.startswith('ds_read_b128')]
    assert len(reads) == OPERAND_READS * len(STAGES), len(reads)
    out = {}
    for k, stage in enumerate(STAGES):
        last = reads[OPERAND_READS * (k + 1) - 1]
        valu = lds_since = 0
        for ln in body[last + 1:]:
            if ln.startswith('ds_'):
                lds_since += 1
            elif ln.startswith('v_'):
                valu += 1
            elif ln.startswith('s_waitcnt'):
                m = re.search(r'lgkmcnt\((\d+)\)', ln)
                if m and int(m.group(1)) <= lds_since:
                    break
        else:
            raise AssertionError("stage %d: its operand reads are never waited for" % stage)
        out[stage] = valu
    return out


def default_mask():
    """the stages the default build of cascade20 / RG0 fetches early, from the source"""
    with open(os.path.join(REPO, 'sysbio_modeling_amd', 'csrc', 'sbm_kernels_rowgroup.hpp')) as fh:
        m = re.search(r'^#define SBM_RG_EARLY_DEFAULT\s+(0[xX][0-9a-fA-F]+|\d+)u?\s*$', fh.read(), re.M)
    assert m, "SBM_RG_EARLY_DEFAULT not found"
    return int(m.group(1), 0)


@pytest.fixture(scope='module')
def cascade20(tmp_path_factory):
    if not _tools():
        pytest.skip("needs objcopy and the LLVM binutils of ROCm")
    tmp = tmp_path_factory.mktemp('isa')
    new, old = _plugins('cascade20')
    return _code(new, str(tmp / 'new')), _code(old, str(tmp / 'old'))


def test_headline_step_loop(cascade20):
    (new, new_meta), (old, old_meta) = cascade20
    for text in (new, old):
        loop = whole_loop(text, KERNEL)
        assert _count(loop, VMEM) == 0, [ln for ln in loop if re.match(VMEM, ln)]
    v_new, v_old = _count(step_loop(new), r'v_'), _count(step_loop(old), r'v_')
    print('loop body VALU: default', v_new, 'mask 0', v_old, '; metadata', new_meta[KERNEL], old_meta[KERNEL])
    assert abs(v_new - v_old) <= 0.01 * v_old
    assert new_meta[KERNEL]['vgpr_count'] <= 256


def test_early_stages_form_their_argument_under_the_fetch(cascade20):
    (new, _), (old, _) = cascade20
    u_new, u_old = valu_under_the_operand_fetch(step_loop(new)), valu_under_the_operand_fetch(step_loop(old))
    mask = default_mask()
    print('VALU under the operand fetch, stage: default / mask 0:', {s: (u_new[s], u_old[s]) for s in STAGES}, 'mask', hex(mask))
    for s in STAGES:
        if (mask >> s) & 1:
            assert u_new[s] > u_old[s], (s, u_new, u_old)


def test_no_rowgroup_kernel_of_the_zoo_gains_memory_traffic_in_its_step_loop(tmp_path):
    if not _tools():
        pytest.skip("needs objcopy and the LLVM binutils of ROCm")
    from sysbio_modeling_amd.symbolic import ZOO_NAMES
    seen = 0
    for name in ZOO_NAMES:
        new, old = _plugins(name)
        (t_new, m_new), (t_old, m_old) = _code(new, str(tmp_path / name / 'new')), _code(old, str(tmp_path / name / 'old'))
        for kernel in sorted(k for k in m_new if 'sbm_sens_rowgroup_kernel' in k):
            n_new, n_old = _count(whole_loop(t_new, kernel), VMEM), _count(whole_loop(t_old, kernel), VMEM)
            print(name, kernel, 'vmem in the step loop', n_old, '->', n_new, '; spills', m_old[kernel]['vgpr_spill_count'],
                  '->', m_new[kernel]['vgpr_spill_count'], '; scratch bytes', m_old[kernel]['private_segment_fixed_size'],
                  '->', m_new[kernel]['private_segment_fixed_size'])
            assert n_new <= n_old, (name, kernel, n_old, n_new)
            seen += 1
    assert seen >= 6          # cascade20 and stiff50: RG0 / RG1 / RG2 under their methods
