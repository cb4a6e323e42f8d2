#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds, kernel by kernel.

    compare_code_objects.py DIR_A DIR_B                   every sbm_model_*.so (and libsbm_hip.so) found in both directories
    compare_code_objects.py TREE_A TREE_B MODEL [...]     compile MODEL from both source trees first, with the flags of
                                                          build.build_plugin (MODEL: a zoo name or the path of a generated
                                                          header; --flags "-DFOO=1" adds to both sides)

Per plugin and kernel: "identical" when the instruction streams are equal (disassembly without addresses and encodings;
the __hip_cuid_* symbol and source paths never reach it), otherwise the metadata keys that changed, old -> new, or
"code differs, metadata equal".  It diffs and prints; it looks for no particular instruction.  Exit status 1 when
anything differs."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get('SBM_LLVM_BIN', '/opt/rocm/lib/llvm/bin')
KEYS = ('vgpr_count', 'agpr_count', 'sgpr_spill_count', 'vgpr_spill_count', 'private_segment_fixed_size',
        'group_segment_fixed_size')


def code_object(shared_object, tmp):
    fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, 'dev.co')
    subprocess.run(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', shared_object, fat], check=True)
    subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--type=o', '--input=' + fat,
                    '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co, '--unbundle'], check=True)
    return co


def kernels_of(shared_object):
    """{kernel symbol: (instruction lines, {metadata key: value})}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(shared_object, tmp)
        dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True, stdout=subprocess.PIPE,
                               text=True).stdout
    code = {}
    for m in re.finditer(r'^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)', dis, re.S | re.M):
        # mnemonic + operands; the trailing "// address" comment goes, and so does the pc-relative offset of a constant
        # table (the literal of the s_add_u32 behind s_getpc_b64): it moves with the size of every kernel in between
        lines, pc = [], False
        for ln in m.group(2).splitlines():
            ln = re.sub(r'\s*//.*$', '', ln).strip()
            if pc and ln.startswith('s_add_u32'):
                ln = re.sub(r'0x[0-9a-f]+$', '<pcrel>', ln)
            pc = ln.startswith('s_getpc_b64')
            if ln:
                lines.append(ln)
        code[m.group(1)] = lines
    meta, cur = {}, {}
    for ln in notes.splitlines():
        m = re.match(r'\s*(?:- )?\.(\w+):\s*(\S.*?)\s*$', ln)
        if not m:
            continue
        if ln.lstrip().startswith('- ') and cur.get('symbol'):     # first key of the next kernel's map
            meta[cur['symbol'][:-len('.kd')]] = cur
            cur = {}
        if m.group(1) in KEYS + ('symbol',):
            cur[m.group(1)] = m.group(2).strip("'\"")
    if cur.get('symbol'):
        meta[cur['symbol'][:-len('.kd')]] = cur
    return {k: (code[k], {key: meta[k].get(key) for key in KEYS}) for k in code if k in meta}


def compare(a, b):
    """lines of the report for shared objects a and b; [] when every kernel is identical"""
    ka, kb = kernels_of(a), kernels_of(b)
    out = []
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            out.append('%s: only in %s' % (k, 'B' if k not in ka else 'A'))
        elif ka[k][0] != kb[k][0]:
            changed = ['%s %s -> %s' % (key, ka[k][1][key], kb[k][1][key]) for key in KEYS if ka[k][1][key] != kb[k][1][key]]
            out.append('%s: %s (%d -> %d instructions)' % (k, ', '.join(changed) or 'code differs, metadata equal',
                                                           len(ka[k][0]), len(kb[k][0])))
    return out, len(ka)


def build_from_tree(tree, model, flags, out_dir):
    header = model if os.path.isfile(model) else os.path.join(tree, 'sysbio_modeling_amd', 'csrc', 'models', model + '.hpp')
    name = os.path.splitext(os.path.basename(header))[0]
    out = os.path.join(out_dir, 'sbm_model_%s.so' % name)
    # the flags of sysbio_modeling_amd/build.py::build_plugin
    subprocess.run(['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared',
                    '-DSBM_MODEL_HEADER="%s"' % os.path.abspath(header), *flags,
                    os.path.join(tree, 'sysbio_modeling_amd', 'csrc', 'sbm_plugin_main.hip'), '-o', out], check=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('models', nargs='*')
    ap.add_argument('--flags', default='')
    ap.add_argument('--jobs', type=int, default=4)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=args.jobs) as pool:
        if args.models:
            dirs = []
            for side, tree in (('a', args.a), ('b', args.b)):
                d = os.path.join(tmp, side)
                os.makedirs(d)
                dirs.append(d)
                list(pool.map(lambda m: build_from_tree(tree, m, args.flags.split(), d), args.models))
        else:
            dirs = [args.a, args.b]
        names = sorted(f for f in os.listdir(dirs[0]) if f.endswith('.so') and f.startswith(('sbm_model_', 'libsbm_hip')))
        missing = [f for f in names if not os.path.exists(os.path.join(dirs[1], f))]
        names = [f for f in names if f not in missing]
        results = pool.map(lambda f: compare(os.path.join(dirs[0], f), os.path.join(dirs[1], f)), names)
        differs = bool(missing)
        for f, (lines, n) in zip(names, results):
            print('%s: %s' % (f, 'identical (%d kernels)' % n if not lines else '%d of %d kernels differ' % (len(lines), n)))
            for ln in lines:
                print('    ' + ln)
            differs = differs or bool(lines)
        for f in missing:
            print('%s: only in A' % f)
    return 1 if differs else 0


if __name__ == '__main__':
    sys.exit(main())
