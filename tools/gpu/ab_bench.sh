#!/bin/bash
# same-box A/B of the bench: ab_old/ holds an older checkout (git archive <rev> | tar -x -C ab_old, plus the built .so),
# the working tree is B.  usage: bash tools/gpu/ab_bench.sh <tag> [rounds]
# Stops at the first run that fails (nothing more is started on a GPU that a run may have left in a bad state).
tag=${1:-ab}
rounds=${2:-2}
out=$(pwd)/gpurun_out/$tag
mkdir -p $out
export TMPDIR=/tmp
root=$(pwd)
args="--steps 20 --warmup 5 --no-cpu-baseline --no-roofline --min-seconds 3"
for r in $(seq 1 $rounds); do
  (cd $root/ab_old && timeout -k 10 200 python bench.py $args > $out/a$r.json 2> $out/a$r.err) || { echo "A$r failed (rc $?): $out/a$r.err"; exit 1; }
  echo "A$r $(grep -o 'median [0-9.]*s ([0-9.]* frames/s)' $out/a$r.err)"
  (cd $root && timeout -k 10 200 python bench.py $args > $out/b$r.json 2> $out/b$r.err) || { echo "B$r failed (rc $?): $out/b$r.err"; exit 1; }
  echo "B$r $(grep -o 'median [0-9.]*s ([0-9.]* frames/s)' $out/b$r.err)"
done
