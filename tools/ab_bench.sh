#!/bin/bash
# Interleaved A/B of whole bench.py runs on one GPU box: one process per run, the arms in turn, round after round.
#
#   tools/ab_bench.sh <out.txt> <arm> [<arm> ...]        arm = name:dir[:VAR=value[,VAR=value ...]]
#
# `dir` is a built tree (its own bench.py and library): "." for this one, a checkout of the parent commit for the parent.
# Environment: AB_ROUNDS (3), AB_BENCH_ARGS ("--gpus 1 --steps 20 --warmup 5"), AB_STEP_TIMEOUT (seconds per run, 240).
# Every run is its own GPU step under its own time limit; the first run that fails, faults or times out ends the script.
# Writes one summary line per run and, below them, the raw JSON line of every run.
#
# Example (parent against the change against the change with a knob off):
#   tools/ab_bench.sh profiles/x_ab.txt parent:../parent change:. "off:.:MFSR_MARGIN_SITES=0"
set -u
out=${1:?usage: ab_bench.sh out.txt name:dir[:VAR=value,...] ...}
shift
rounds=${AB_ROUNDS:-3}
args=${AB_BENCH_ARGS:---gpus 1 --steps 20 --warmup 5}
limit=${AB_STEP_TIMEOUT:-240}
top=$PWD
case $out in /*) ;; *) out=$top/$out ;; esac
raw=$(mktemp)
: > "$out"
for round in $(seq 1 "$rounds"); do
  for arm in "$@"; do
    name=${arm%%:*}
    rest=${arm#*:}
    dir=${rest%%:*}
    envs=""
    [ "$rest" != "$dir" ] && envs=$(echo "${rest#*:}" | tr ',' ' ')
    line=$(set -o pipefail; cd "$top/$dir" && env $envs timeout -k 10 "$limit" python3 bench.py $args 2>/dev/null | tail -1)
    rc=$?
    if [ $rc -ne 0 ] || [ -z "$line" ]; then
      echo "round $round $name: bench.py failed (exit $rc)" | tee -a "$out"
      exit 1
    fi
    echo "$line" | python3 -c "
import json, sys
d = json.loads(sys.stdin.read())
print('$name | value %s %s | ms_per_step %s | avg_launch_ms %s | sha %s' % (d['value'], d['unit'], d['ms_per_step'], d.get('roofline', {}).get('avg_launch_ms'), d.get('out16_sha256_16')))
" | tee -a "$out"
    printf '## round %s %s\n%s\n' "$round" "$name" "$line" >> "$raw"
  done
done
cat "$raw" >> "$out"
rm -f "$raw"
