#!/bin/bash
# Compares the gfx950 device code of two builds of the package, unit by unit: the code object is taken out
# of each host object's .hip_fatbin section, compared byte for byte, and its disassembly compared too.
# usage: tools/device_code_diff.sh <build dir A> <build dir B> [unit ...]
set -u
B=${ROCM_LLVM:-/opt/rocm/llvm/bin}
A_DIR=$1; B_DIR=$2; shift 2
UNITS=${*:-gar_kernels gar_bg_f32a gar_bg_f32b gar_bg_f64 gar_hx gar_hx_i1 gar_hx_i2 gar_hx_i3 gar_hx_i4 gar_hx_i5 gar_hxs gar_hxs_i1 gar_hxs_i2 gar_hxs_i3 gar_hxs_i4 gar_hxt_i1 gar_hxt_i2 gar_hxt_i3}
T=$(mktemp -d)
rc=0
code() {  # $1 object, $2 output prefix: 0 extracted, 1 no device code
    [ "$("$B/llvm-readelf" -S "$1" | grep -c hip_fatbin)" = 0 ] && return 1
    "$B/llvm-objcopy" -O binary --only-section=.hip_fatbin "$1" "$2.fatbin" &&
        "$B/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$2.fatbin" --output="$2.co" &&
        "$B/llvm-objdump" -d --no-show-raw-insn "$2.co" | grep -v "file format" > "$2.s"
}
for u in $UNITS; do
    code "$A_DIR/$u.o" "$T/a"; ra=$?
    code "$B_DIR/$u.o" "$T/b"; rb=$?
    if [ $ra = 1 ] && [ $rb = 1 ]; then echo "$u: no device code in either build"
    elif [ $ra != 0 ] || [ $rb != 0 ]; then echo "$u: device code in one build only, or extraction failed"; rc=1
    elif cmp -s "$T/a.co" "$T/b.co" && cmp -s "$T/a.s" "$T/b.s"; then echo "$u: code objects byte-identical ($(wc -l < "$T/b.s") lines of disassembly)"
    elif cmp -s "$T/a.s" "$T/b.s"; then echo "$u: disassembly identical, code objects differ outside the code"
    else echo "$u: DIFFERS"; rc=1
    fi
done
rm -rf "$T"
exit $rc
