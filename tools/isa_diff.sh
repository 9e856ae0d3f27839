#!/bin/bash
# Device-code identity of two source trees: tools/isa_diff.sh <tree_a> <tree_b>
# Compiles the device units of each tree for gfx950 with the Makefile's flags (the same build id on both sides): the
# units of its csrc/Makefile's UNITS line (a tree from before that line: the six units it had) and the four spectra
# units.  Needs no GPU.  KEEP=1 keeps the work directory.
#  - A unit both trees have is compared whole: the disassembly and the code-object notes (kernel list, VGPR/SGPR, LDS,
#    scratch, max workgroup size).
#  - Where that differs (kernels moved to another unit, or an argument struct renamed), every kernel of tree_a's unit
#    is compared with the kernel of the same unqualified name and template arguments in whichever unit of tree_b holds
#    it: the disassembly without addresses (branch targets print as symbol + offset; the kernel's own symbol is
#    masked) and its notes entry (registers, LDS, scratch, kernarg and workgroup size).
# Exit 0 = every unit, or every kernel of it, identical.
set -u
[ $# -eq 2 ] || { echo "usage: $0 <tree_a> <tree_b>" >&2; exit 2; }
ROCM=${ROCM_PATH:-/opt/rocm}; LLVM=$ROCM/lib/llvm/bin; ARCH=${ARCH:-gfx950}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=$ARCH -Wall -Wno-unused-function -Wno-unused-variable"
W=$(mktemp -d); [ "${KEEP:-0}" = 1 ] || trap 'rm -rf "$W"' EXIT
SPECTRA="spectra_12 spectra_3 spectra_4 spectra_5"
units_of() {  # <tree>: its Makefile's unit list
  local u; u=$(sed -n 's/^UNITS := *//p' "$1/is3d2_amd/csrc/Makefile")
  echo "${u:-engine group polzn sampler decay decay_list} $SPECTRA"
}
one() {  # <tree> <out dir> <unit>
  local src=$3.hip def=
  case $3 in spectra_*) src=spectra_tu.hip; def=-DIS3D_TU=${3#spectra_};; engine) def='-DIS3D_BUILD_ID="isa_diff"';; esac
  "$ROCM/bin/hipcc" $FLAGS $def --cuda-device-only -c -o "$2/$3.bundle" "$1/is3d2_amd/csrc/$src" 2> "$2/$3.log" &&
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--$ARCH --input="$2/$3.bundle" --output="$2/$3.co" &&
  "$LLVM/llvm-objdump" -d "$2/$3.co" | { grep -v 'file format' || true; } > "$2/$3.s" &&   # a host-only unit: empty
  "$LLVM/llvm-readelf" --notes "$2/$3.co" > "$2/$3.notes"
}
UA=$(units_of "$1"); UB=$(units_of "$2")
for side in a b; do
  tree=$1; units=$UA; [ $side = b ] && { tree=$2; units=$UB; }
  mkdir -p "$W/$side"
  for u in $units; do one "$tree" "$W/$side" $u & done
  wait
done

# ---- per-kernel mode --------------------------------------------------------------------------------------------------
per_kernel() {  # <unit of tree_a>; the units of tree_b that built follow
python3 - "$LLVM" "$W" "$@" <<'PY'
import re, subprocess, sys
llvm, W, ua, ubs = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
FIELDS = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
          "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size", "vgpr_spill_count", "sgpr_spill_count")
def run(*a): return subprocess.run(a, capture_output=True, text=True).stdout
def key(dem):                      # unqualified kernel name + template arguments
    k = re.sub(r"^void ", "", dem).replace("(anonymous namespace)::", "")
    d = 0
    for i in range(len(k) - 1, -1, -1):          # drop the parameter list: the last balanced (...) group
        d += k[i] == ")"
        if k[i] == "(":
            d -= 1
            if d == 0: k = k[:i]; break
    head, lt, rest = k.partition("<")
    return (head.rsplit("::", 1)[-1] + lt + rest).replace(" ", "")
def unit(side, u):
    co = "%s/%s/%s.co" % (W, side, u)
    row = re.compile(r"^([0-9a-f]+) .*\t([0-9a-f]+) (?:\.[a-z]+ )?(.*)$")
    tab = [row.match(l) for l in run(llvm + "/llvm-objdump", "-t", co).splitlines()]
    dem = [row.match(l) for l in run(llvm + "/llvm-objdump", "-t", "-C", co).splitlines()]
    names = {m.group(3): d.group(3) for m, d in zip(tab, dem) if m and d}
    objs = sorted((int(m.group(1), 16), int(m.group(2), 16), m.group(3)) for m in tab if m and int(m.group(2), 16))
    def sym_at(addr):              # symbol + offset of an address (the __constant__ tables a kernel points at)
        for a, n, s in objs:
            if a <= addr < a + n: return "%s+0x%x" % (names.get(s, s), addr - a)
        return "0x%x" % addr
    notes = {}
    for ent in re.split(r"\n(?=\s+- \.a)", run(llvm + "/llvm-readelf", "--notes", co)):
        m = re.search(r"\.symbol:\s*'?([^'\s]+)\.kd", ent)
        if m: notes[m.group(1)] = sorted(l.strip() for l in ent.splitlines() if l.strip().lstrip("- ").split(":")[0].lstrip(".") in FIELDS)
    # llvm-objdump -d --no-show-raw-insn --no-leading-addr; the amdgpu printer's "// address: words" comment gives the
    # address of an s_getpc_b64, whose pc-relative literal is printed as the symbol + offset it reaches
    body, cur, pc = {}, None, None
    for l in run(llvm + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(.*)>:$", l)
        if m: cur = m.group(1); body[cur] = []; pc = None; continue
        if cur is None or not l.strip() or l.strip() == "...": continue      # "...": padding up to the next function
        c = re.search(r"// ([0-9A-F]+):(?: [0-9A-F]{8})+", l)
        t = re.sub(r"// [0-9A-F]+:(?: [0-9A-F]{8})+", "", l).replace(cur, "KERNEL").rstrip()
        t = re.sub(r"\s+", " ", t)
        if pc is not None:
            m = re.match(r"^ ?s_add_u32 (s\d+), \1, (0x[0-9a-f]+|-?\d+)$", t)
            if m:
                imm = int(m.group(2), 0) & 0xffffffff
                t = " s_add_u32 %s, %s, <%s>" % (m.group(1), m.group(1), sym_at((pc + imm - (1 << 32 if imm >> 31 else 0))))
        pc = int(c.group(1), 16) + 4 if c and "s_getpc_b64" in t else None
        body[cur].append(t)
    return {key(names[s]): (s, body.get(s), notes[s]) for s in notes if s in names}
A = unit("a", ua)
B = {}
for ub in ubs:
    for k, v in unit("b", ub).items(): B.setdefault(k, (ub,) + v)
bad, moved = not A, []
if not A: print("  no kernels found in tree_a's " + ua)
for k, (s, body, note) in A.items():
    if k not in B: print("  %s: MISSING in tree_b" % k); bad = True; continue
    ub, sb, bodyb, noteb = B[k]
    if body and note and body == bodyb and note == noteb:
        if ub != ua: moved.append("%s->%s" % (k, ub))
        continue
    import difflib
    nd = sum(1 for l in difflib.unified_diff(body or [], bodyb or [], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
    nn = sum(1 for l in difflib.unified_diff(note or [], noteb or [], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
    print("  %s (%s -> %s): DIFFERENT (disassembly %d lines, notes %d lines)" % (k, ua, ub, nd, nn)); bad = True
if not bad: print("%s: identical per kernel (%d kernels%s)" % (ua, len(A), "; moved: " + " ".join(moved) if moved else ""))
sys.exit(1 if bad else 0)
PY
}
BUILT_B=$(for u in $UB; do [ -s "$W/b/$u.notes" ] && grep -q '\.symbol:' "$W/b/$u.notes" && echo $u; done)

rc=0
for u in $UA; do
  [ -s "$W/a/$u.co" ] && [ -e "$W/a/$u.notes" ] || { echo "$u: BUILD FAILED (see $W/a/$u.log; KEEP=1)"; rc=1; continue; }
  if cmp -s "$W/a/$u.s" "$W/b/$u.s" && cmp -s "$W/a/$u.notes" "$W/b/$u.notes"; then
    echo "$u: identical ($(wc -l < "$W/b/$u.s") disassembly lines, $(grep -c '^ *\.name: ' "$W/b/$u.notes") note names)"
  else
    per_kernel $u $BUILT_B || { echo "$u: DIFFERENT"; rc=1; }
  fi
done
# a unit only tree_b has must have built too (its kernels are checked when they came from tree_a)
for u in $UB; do [ -s "$W/b/$u.co" ] && [ -e "$W/b/$u.notes" ] || { echo "$u: BUILD FAILED in tree_b (see $W/b/$u.log; KEEP=1)"; rc=1; }; done
exit $rc
