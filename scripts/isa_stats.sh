#!/bin/bash
# usage: scripts/isa_stats.sh <model> : compile plugin with -save-temps in /tmp/sbm and print per-kernel stats
#        scripts/isa_stats.sh <built plugin .so> : the registers, spills, scratch and LDS of every kernel from the code
#        object's metadata alone (no compile: for models whose header is generated, not committed, e.g.
#        sysbio_modeling_amd/_build/sbm_model_tile49_17_<digest>.so after build())
set -e
M=${1:-cascade20}
if [ -f "$M" ] && [[ "$M" == *.so ]]; then
  SO=$(readlink -f "$M")
  LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
  T=$(mktemp -d) && trap 'rm -rf "$T"' EXIT
  "$LLVM"/llvm-objcopy --dump-section .hip_fatbin="$T"/fat.bin "$SO"
  "$LLVM"/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$T"/fat.bin --output="$T"/gfx950.co
  # one line per kernel (an entry of amdhsa.kernels begins at "  - ."; its keys are in alphabetical order, .name in the middle)
  "$LLVM"/llvm-readelf --notes "$T"/gfx950.co | awk '
    function flush() { if (v[".name"] != "") printf "%s: vgpr %s (of which agpr %s) vgpr_spill %s sgpr_spill %s scratch %s B lds %s B\n", v[".name"],
        v[".vgpr_count"], v[".agpr_count"], v[".vgpr_spill_count"], v[".sgpr_spill_count"], v[".private_segment_fixed_size"], v[".group_segment_fixed_size"]; delete v }
    /^  - \./ { flush(); sub(/- /, "  ") }
    /^    \.(name|agpr_count|vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):/ { k = $1; sub(/:$/, "", k); v[k] = $2 }
    /^amdhsa\.target/ { flush() }
    END { flush() }'
  exit 0
fi
mkdir -p /tmp/sbm && cd /tmp/sbm && rm -f *.s
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -DSBM_MODEL_HEADER="\"/root/repo/sysbio_modeling_amd/csrc/models/$M.hpp\"" /root/repo/sysbio_modeling_amd/csrc/sbm_plugin_main.hip -o /tmp/sbm/$M.so -save-temps 2>&1 | grep -E "error|warning" | head
grep -E "^\s+\.(vgpr_count|sgpr_spill_count|vgpr_spill_count|name|private_segment_fixed_size):" *gfx950*.s
for k in $(grep -E "^\s+\.name:" *gfx950*.s | awk '{print $2}'); do
  awk "/^$k:/,/s_endpgm/" *gfx950*.s > k.s
  echo "== $k: $(grep -cE '^\s+[a-z_0-9]+ ' k.s) instrs; fp64: $(grep -cE 'v_(fma|fmac|mul|add|rcp|max|min)_f64' k.s) accvgpr: $(grep -c accvgpr k.s) cndmask: $(grep -c v_cndmask k.s) scratch: $(grep -c scratch_ k.s) saveexec: $(grep -c saveexec k.s)"
done
