#!/usr/bin/env bash
# Compares the gfx950 device assembly of every srsran-5g_amd/csrc/*.hip of two source trees, compiled with build.sh's
# flags: the proof that a refactor of force-inlined device helpers moved code and changed none. Lines with the
# __hip_cuid_ symbol (a hash of the source text) are left out; any other difference, register numbers and instruction
# order included, counts. An optional third argument is a sed script applied to both sides first, for a refactor that
# renames a type in a kernel's signature and with it the kernel's mangled name (e.g. 's/8prach_cf/3cpx/g').
#   tools/isa_diff.sh <old-tree> <new-tree> [sed-script]      (a `git worktree` of the parent commit is an old tree)
# Prints the files that differ and "<n> files, <m> differ"; the exit status is 0 when none does. The assembly and the
# diffs stay in $ISA_DIFF_OUT (default: a fresh temporary directory) for reading.
set -euo pipefail
[ $# -ge 2 ] || { echo "usage: $0 <old-tree> <new-tree> [sed-script]" >&2; exit 2; }
OLD=$(cd "$1" && pwd) NEW=$(cd "$2" && pwd) RENAME=${3:-}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${ISA_DIFF_OUT:-$(mktemp -d)}
mkdir -p "$OUT/old" "$OUT/new"

assemble() {  # <tree> <file name> <output>
  local extra=""
  [[ "$2" == pusch_demodulator.hip || "$2" == ofdm.hip ]] && extra="-fno-slp-vectorize"
  $HIPCC -std=c++17 -O3 -fPIC --offload-arch=gfx950 -I"$1/include" -I"$1/srsran-5g_amd/csrc" $extra -x hip \
    -Wno-unused-command-line-argument --offload-device-only -S "$1/srsran-5g_amd/csrc/$2" -o - | grep -v __hip_cuid_ | sed -e "$RENAME" > "$3"
}

names=()
for src in "$NEW"/srsran-5g_amd/csrc/*.hip; do
  name=$(basename "$src")
  names+=("$name")
  assemble "$OLD" "$name" "$OUT/old/$name.s" &
  assemble "$NEW" "$name" "$OUT/new/$name.s" &
done
wait  # (a failed compilation leaves an empty or missing file, which differs below)
differ=0
for name in "${names[@]}"; do
  if ! [ -s "$OUT/new/$name.s" ] || ! diff "$OUT/old/$name.s" "$OUT/new/$name.s" > "$OUT/$name.diff"; then
    echo "DIFFERS: $name ($OUT/$name.diff)"
    differ=$((differ + 1))
  fi
done
echo "${#names[@]} files, $differ differ"
[ "$differ" -eq 0 ]
