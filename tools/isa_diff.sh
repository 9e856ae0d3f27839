#!/bin/bash
# Device-code identity of two source trees: tools/isa_diff.sh <tree_a> <tree_b>
# Compiles the nine device units of each tree for gfx950 with the Makefile's flags (the same build id on
# both sides), and compares the disassembly and the code-object notes (kernel list, VGPR/SGPR, LDS, scratch,
# max workgroup size).  Needs no GPU.  Exit 0 = every unit identical.  KEEP=1 keeps the work directory.
set -u
[ $# -eq 2 ] || { echo "usage: $0 <tree_a> <tree_b>" >&2; exit 2; }
ROCM=${ROCM_PATH:-/opt/rocm}; LLVM=$ROCM/lib/llvm/bin; ARCH=${ARCH:-gfx950}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=$ARCH -Wall -Wno-unused-function -Wno-unused-variable"
W=$(mktemp -d); [ "${KEEP:-0}" = 1 ] || trap 'rm -rf "$W"' EXIT
UNITS="engine group polzn sampler decay spectra_12 spectra_3 spectra_4 spectra_5"
one() {  # <tree> <out dir> <unit>
  local src=$3.hip def=
  case $3 in spectra_*) src=spectra_tu.hip; def=-DIS3D_TU=${3#spectra_};; engine) def='-DIS3D_BUILD_ID="isa_diff"';; esac
  "$ROCM/bin/hipcc" $FLAGS $def --cuda-device-only -c -o "$2/$3.bundle" "$1/is3d2_amd/csrc/$src" 2> "$2/$3.log" &&
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--$ARCH --input="$2/$3.bundle" --output="$2/$3.co" &&
  "$LLVM/llvm-objdump" -d "$2/$3.co" | grep -v 'file format' > "$2/$3.s" &&
  "$LLVM/llvm-readelf" --notes "$2/$3.co" > "$2/$3.notes"
}
for side in a b; do
  tree=$1; [ $side = b ] && tree=$2
  mkdir -p "$W/$side"
  for u in $UNITS; do one "$tree" "$W/$side" $u & done
  wait
done
rc=0
for u in $UNITS; do
  for k in s notes; do [ -s "$W/a/$u.$k" ] && [ -s "$W/b/$u.$k" ] || { echo "$u: BUILD FAILED (see $W/*/$u.log; KEEP=1)"; rc=1; continue 2; }; done
  n=$(grep -c '^ *\.name: ' "$W/b/$u.notes"); l=$(wc -l < "$W/b/$u.s")
  if cmp -s "$W/a/$u.s" "$W/b/$u.s" && cmp -s "$W/a/$u.notes" "$W/b/$u.notes"; then
    echo "$u: identical ($l disassembly lines, $n note names)"
  else
    echo "$u: DIFFERENT (disassembly $(diff "$W/a/$u.s" "$W/b/$u.s" | grep -c '^[<>]') lines, notes $(diff "$W/a/$u.notes" "$W/b/$u.notes" | grep -c '^[<>]') lines)"; rc=1
  fi
done
exit $rc
