"""The step loop of the headline kernel, sbm_sens_rowgroup_kernel<SbmModel, SbmModel::RG0, DOPRI45> of cascade20, counted in
the ISA of the built plugin (the code object is unbundled from the shared object and disassembled; no GPU needed).

The kernel is bound by the VALU issue slots it spends per step (docs/history.md, "class hoist"), so what the class hoist of
emit_rowlane.py buys is read off here: both classes of cascade20 open with SBM_RCP(ys[k] + 1.0), and the emitter now
evaluates that once per stage on a selected operand.

The step loop is the stretch from the target of a backward branch to that branch which holds the most fp64 arithmetic;
the loop BODY counted here is its longest branch-free run, up to and including the branch that ends it: the stages of one
attempted step, without the controller's accept and reject branches behind them (six row evaluations fall inside it).
Measured with this extraction:

    before the hoist (two reciprocal chains per stage):  1209 instructions, 1005 VALU, 12 v_rcp_f64, 87 v_cndmask_b32
    with the hoist:                                      1175 instructions,  974 VALU,  6 v_rcp_f64, 99 v_cndmask_b32
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
KERNEL = '_Z24sbm_sens_rowgroup_kernelI8SbmModelNS0_3RG0ELi1EEv15sbm_kernel_args'
VALU_BEFORE_THE_HOIST = 1005


def disassemble(plugin, tmp):
    fat = os.path.join(tmp, 'fat.bin')
    co = os.path.join(tmp, 'dev.co')
    subprocess.run(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', plugin, fat], check=True)
    subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--input=' + fat,
                    '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co, '--unbundle'], check=True)
    return subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', co], check=True, stdout=subprocess.PIPE,
                          text=True).stdout


def step_loop(text, kernel=KERNEL):
    """[mnemonic + operands] of the step loop of ``kernel``: among the backward branches of the kernel, the span (branch
    target .. branch) with the most fp64 arithmetic in it"""
    m = re.search(r'^([0-9a-f]+) <%s>:\n(.*?)(?=^[0-9a-f]+ <|\Z)' % re.escape(kernel), text, re.S | re.M)
    assert m, "%s not found in the code object" % kernel
    base = int(m.group(1), 16)
    insts = []                                  # (address, text, branch target or None)
    for ln in m.group(2).splitlines():
        mm = re.match(r'\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):', ln)
        if not mm:
            continue
        tgt = re.search(r'<[^>+]+\+0x([0-9a-f]+)>\s*$', ln) if mm.group(1).startswith(('s_cbranch', 's_branch')) else None
        insts.append((int(mm.group(2), 16), mm.group(1), base + int(tgt.group(1), 16) if tgt else None))
    index_of = {a: i for i, (a, _, _) in enumerate(insts)}
    fp64 = r'v_(fma|fmac|mul|add)_f64'
    loop = []
    for i, (addr, _, tgt) in enumerate(insts):
        if tgt is not None and tgt <= addr and tgt in index_of:
            body = [t for _, t, _ in insts[index_of[tgt]:i + 1]]
            if _count(body, fp64) > _count(loop, fp64):
                loop = body
    assert loop, "no loop found in %s" % kernel
    # the stages: the branch-free stretch of the loop with the most fp64 arithmetic, with the branch that ends it
    best, run = [], []
    for ln in loop:
        run.append(ln)
        if ln.startswith(('s_cbranch', 's_branch')):
            if _count(run, fp64) > _count(best, fp64):
                best = run
            run = []
    return best


def _count(body, pattern):
    return sum(1 for ln in body if re.match(pattern, ln))


def loop_counts(body):
    return dict(instructions=len(body), valu=_count(body, r'v_'), rcp64=_count(body, r'v_rcp_f64'),
                cndmask=_count(body, r'v_cndmask_b32'), lds=_count(body, r'ds_'),
                vmem=_count(body, r'(scratch_|global_|buffer_|flat_)'))


def test_step_loop_of_the_headline_kernel_has_one_reciprocal_per_stage(tmp_path):
    plugin = os.path.join(REPO, 'sysbio_modeling_amd', '_build', 'sbm_model_cascade20.so')
    if not (os.path.exists(plugin) and shutil.which('objcopy') and os.path.exists(os.path.join(LLVM, 'llvm-objdump'))):
        pytest.skip("needs the built cascade20 plugin and the LLVM binutils of ROCm")
    body = step_loop(disassemble(plugin, str(tmp_path)))
    c = loop_counts(body)
    print(c)
    assert c['rcp64'] == 6, c                   # six stages in the loop body, one reciprocal chain each (12 before)
    assert c['vmem'] == 0, [ln for ln in body if re.match(r'(scratch_|global_|buffer_|flat_)', ln)]
    assert c['valu'] < VALU_BEFORE_THE_HOIST, c
