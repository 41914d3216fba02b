#!/bin/bash
# Routes and bits of two builds of the library over the routing grid, one tools/lib_equal.py after another:
#   tools/route_equal.sh libA libB [scale] [f ...]      (the whole grid, or the given f only)
# f x solver x gram mode at the default pre-split; pre-split off / on / verify at f = 64, 100, 144, 200; the packed in-kernel
# split and the Gram-free CG of short rows switched off at f = 64, 100.  One line per configuration: DIFFERENT is reported
# and the grid goes on; a configuration that fails or takes longer than 700 s stops it.
A=$1; B=$2; S=${3:-0.1}; shift 3 2>/dev/null || shift $#
R=$(cd "$(dirname "$0")/.." && pwd); FS=" $* "  # FS: the f values to run, "  " for all
run() {  # label, lib_equal arguments after the two libraries
  local label="$1 f=$2 $3 gram=$5 presplit=$6"; shift
  [ "$FS" = "  " ] || [[ "$FS" == *" $1 "* ]] || return 0
  echo "== $label"
  timeout -k 10 700 python "$R/tools/lib_equal.py" "$A" "$B" "$@" || [ $? -le 1 ] ||
    { echo "route_equal: $label failed or ran out of time; stopping" >&2; exit 2; }
}
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
