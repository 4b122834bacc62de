#!/usr/bin/env bash
# Compare the gfx950 device code of two builds of wcmc_amd/csrc, kernel by kernel -- the check behind a refactor that must not
# change any kernel's machine code (moving kernels between translation units, reordering helpers, renaming files).  No GPU needed.
#
#   scripts/compare_device_code.sh OLD_CSRC NEW_CSRC [> profiles/<name>.txt]
#
# OLD_CSRC / NEW_CSRC: two csrc directories after `make all debug` (the objects *.o and *.dbg.o are read; file names need not match).
# Per build (release = *.o, debug = *.dbg.o) it reports
#   * the kernel symbols (FUNC symbols of the code objects) only one side has,
#   * the kernels that occur in more than one code object of a side (expected for the `static` kernels of conv_common.h only),
#   * the kernels whose disassembly differs (the `// address: encoding` comments, which carry load addresses, are stripped).
# Exit status 0 iff the symbol sets are equal and no kernel differs, in both builds.
set -euo pipefail
[ $# -eq 2 ] || { sed -n '2,12p' "$0"; exit 2; }
OLD=$(cd "$1" && pwd); NEW=$(cd "$2" && pwd)
LLVM=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
ARCH=${ARCH:-gfx950}
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT

# dump <side dir> <object> : writes "<md5 of the kernel's instructions> <symbol> <object>" lines
dump() {
  local obj=$2 base; base=$(basename "$2")
  "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$TMP/fb" "$obj" /dev/null 2>/dev/null || return 0      # (no device code: api.o)
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--$ARCH --input="$TMP/fb" --output="$TMP/co"
  "$LLVM/llvm-readelf" -sW "$TMP/co" | awk '$4 == "FUNC" { print $8 }' | sort -u > "$TMP/syms"
  [ -s "$TMP/syms" ] || return 0
  # one disassembly per code object, cut at the `<symbol>:` labels, hashed per kernel
  "$LLVM/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "$TMP/co" | sed -E 's#//.*$##; s/[[:space:]]+$//' |
    awk -v base="$base" -v symfile="$TMP/syms" -v out="$TMP/k" '
      BEGIN { while ((getline s < symfile) > 0) want[s] = 1; n = 0 }
      /^[0-9a-f]* *<[^>]+>:$/ { name = $0; sub(/^[^<]*</, "", name); sub(/>:$/, "", name);
                                if (name in want) { cur = out "." (++n); print name > (out ".names") } else cur = ""; next }
      cur != "" { print > cur }'
  local i=0 name
  while read -r name; do
    i=$((i + 1))
    # (alignment padding behind a kernel -- s_nop / s_code_end / zeros up to the next kernel or the end of .text -- depends on what follows it)
    echo "$(tac "$TMP/k.$i" | awk 'body || !/^[[:space:]]*(s_nop 0|s_code_end|\.\.\.)?[[:space:]]*$/ { body = 1; print }' | md5sum | cut -d' ' -f1) $name $base"
  done < "$TMP/k.names"
  rm -f "$TMP"/k.*
}

status=0
for build in release debug; do
  for side in OLD NEW; do
    dir=${!side}
    : > "$TMP/$side.$build"
    for obj in "$dir"/*.o; do
      case "$obj" in *.dbg.o) [ $build = debug ] || continue ;; *) [ $build = release ] || continue ;; esac
      dump "$dir" "$obj" >> "$TMP/$side.$build"
    done
    # symbol -> sorted set of hashes (a kernel that several objects carry must be the same set on both sides)
    sort -k2,2 -k1,1 -u "$TMP/$side.$build" | awk '{ print $2, $1 }' | sort -u > "$TMP/$side.$build.pairs"
    cut -d' ' -f1 "$TMP/$side.$build.pairs" | sort -u > "$TMP/$side.$build.syms"
  done
  nold=$(wc -l < "$TMP/OLD.$build.syms"); nnew=$(wc -l < "$TMP/NEW.$build.syms")
  comm -23 "$TMP/OLD.$build.syms" "$TMP/NEW.$build.syms" > "$TMP/only_old"
  comm -13 "$TMP/OLD.$build.syms" "$TMP/NEW.$build.syms" > "$TMP/only_new"
  comm -12 "$TMP/OLD.$build.syms" "$TMP/NEW.$build.syms" > "$TMP/both"
  ndiff=0; : > "$TMP/differ"
  while read -r s; do
    a=$(awk -v s="$s" '$1 == s { print $2 }' "$TMP/OLD.$build.pairs" | tr '\n' ' ')
    b=$(awk -v s="$s" '$1 == s { print $2 }' "$TMP/NEW.$build.pairs" | tr '\n' ' ')
    [ "$a" = "$b" ] || { ndiff=$((ndiff + 1)); echo "$s" >> "$TMP/differ"; }
  done < "$TMP/both"
  nboth=$(wc -l < "$TMP/both")
  echo "== $build build"
  echo "kernel symbols: old $nold, new $nnew; only in old $(wc -l < "$TMP/only_old"), only in new $(wc -l < "$TMP/only_new")"
  echo "kernels compared: $nboth; identical $((nboth - ndiff)); differing $ndiff"
  for side in OLD NEW; do
    echo "kernels in more than one code object ($side):"
    awk '{ n[$2]++; o[$2] = o[$2] " " $3 } END { for (s in n) if (n[s] > 1) print "  " s ":" o[s] }' "$TMP/$side.$build" | sort
  done
  echo "kernels per code object (NEW):"
  awk '{ n[$3]++ } END { for (o in n) print "  " o ": " n[o] }' "$TMP/NEW.$build" | sort
  sed 's/^/only in old: /' "$TMP/only_old"; sed 's/^/only in new: /' "$TMP/only_new"; sed 's/^/DIFFERS: /' "$TMP/differ"
  if [ -s "$TMP/only_old" ] || [ -s "$TMP/only_new" ] || [ $ndiff -ne 0 ]; then status=1; fi
done
exit $status
