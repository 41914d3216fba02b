#!/bin/bash
# Routes and bits of two builds of the library over the routing grid (tools/lib_equal.py per configuration):
#   [JOBS=3] tools/route_equal.sh libA libB [scale]
# f x solver x gram mode at the default pre-split; pre-split off / on / verify at f = 64, 100, 144, 200; the packed
# in-kernel split and the Gram-free CG of short rows switched off at f = 64, 100.  One line per configuration.
A=$1; B=$2; S=${3:-0.1}
R=$(cd "$(dirname "$0")/.." && pwd)
J=${JOBS:-3}
run() {  # label, lib_equal arguments after the two libraries; JOBS configurations side by side, output in order
  local label=$1; shift
  while [ "$(jobs -rp | wc -l)" -ge "$J" ]; do wait -n; done
  local out; out=$(mktemp); OUTS+=("$out")
  { echo "== $label f=$1 $2 gram=$4 presplit=$5"; python "$R/tools/lib_equal.py" "$A" "$B" "$@"; } > "$out" 2>&1 &
}
OUTS=()
for f in 10 20 32 64 96 100 112 128 144 160 200 250; do
  for s in lu cg; do for g in auto exact fast; do run default $f $s $S $g auto; done; done
done
for f in 64 100 144 200; do
  for s in lu cg; do for p in off on verify; do run presplit $f $s $S auto $p; done; done
done
for f in 64 100; do
  for s in lu cg; do
    CUMF_ALS_SPLITPK=0 run splitpk=0 $f $s $S auto auto
    CUMF_ALS_SHORT_CG=0 run short_cg=0 $f $s $S auto auto
  done
done
wait
cat "${OUTS[@]}"; rm -f "${OUTS[@]}"
