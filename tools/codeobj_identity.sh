#!/bin/bash
# Are the device code objects of two builds of fdoct_amd/csrc the same?  For refactors that must not change the shipped kernels.
#   usage: tools/codeobj_identity.sh <parent csrc dir> <head csrc dir> ["<object names>"] > profiles/<record>.txt
# Both directories hold the objects of the default build (`make -C fdoct_amd/csrc`), built from the same relative path with the
# same flags.  A third argument (or OBJS in the environment) names other objects, without ".o", in place of the default build's
# 24: the instrument builds of tests/test_dev_builds.py compiled to objects in both directories, for one.
# Per object the gfx950 code object is unbundled and three texts are hashed (SHA-256): the disassembly of .text,
# the contents of .rodata (kernel descriptors) and the ELF notes (registers, scratch, LDS, argument layout).  The raw objects are
# NOT compared: they carry a source-derived identifier in .dynstr that a comment-only edit changes.  Exit status 1 on a difference.
set -euo pipefail
PARENT=$1
HEAD=$2
LLVM=${LLVM:-$(hipconfig -l)}   # the directory of ROCm's clang and llvm-* tools
OBJS=${3:-${OBJS:-"fdoct_kernels $(for i in 0 1 2 3 4 5 6 7 8; do echo fdoct_kernels_p$i; done) $(for i in 0 1 2 3 4 5 6 7 8; do echo fdoct_kernels_q$i; done) fdoct_generic fdoct_wave fdoct_wave_x1 fdoct_wave_x2 fdoct_big"}}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT

echo "# per object: SHA-256 of three texts of the gfx950 code object, parent | head"
echo "#   llvm-objcopy -O binary --only-section=.hip_fatbin X.o X.fatbin"
echo "#   clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=X.fatbin --output=X.co"
echo "#   text:   llvm-objdump -d X.co          (the 'file format' line, which names the file, dropped)"
echo "#   rodata: llvm-objdump -s -j .rodata X.co"
echo "#   notes:  llvm-readelf --notes X.co"
sums() {  # <object file> <prefix>: the three hashes into $TMP/<prefix>.{text,rodata,notes}; any failing step ends the script
  "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$1" "$TMP/x.fatbin"
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$TMP/x.fatbin" --output="$TMP/x.co"
  [ -s "$TMP/x.co" ]
  "$LLVM/llvm-objdump" -d "$TMP/x.co" | grep -v 'file format' | sha256sum | cut -d" " -f1 > "$TMP/$2.text"
  "$LLVM/llvm-objdump" -s -j .rodata "$TMP/x.co" | grep -v 'file format' | sha256sum | cut -d" " -f1 > "$TMP/$2.rodata"
  "$LLVM/llvm-readelf" --notes "$TMP/x.co" | sha256sum | cut -d" " -f1 > "$TMP/$2.notes"
  rm -f "$TMP/x.fatbin" "$TMP/x.co"
}
bad=0
printf '%-18s %-7s %-64s   %-64s  %s\n' object what parent head same
for o in $OBJS; do
  sums "$PARENT/$o.o" p
  sums "$HEAD/$o.o" h
  for k in text rodata notes; do
    a=$(cat "$TMP/p.$k"); b=$(cat "$TMP/h.$k")
    same=yes
    [ "$a" = "$b" ] || { same=NO; bad=1; }
    printf '%-18s %-7s %-64s | %-64s  %s\n' "$o" "$k" "$a" "$b" "$same"
  done
done
[ $bad = 0 ] && echo "# all identical" || echo "# DIFFERENT"
exit $bad
