#!/bin/bash
# GPU box: the benchmark's headline (the scoring phase of a step at C5, exploded layout) of a BUILT checkout of the parent commit against
# this tree, interleaved in one job -- boxes differ by a few per cent, only same-job pairs compare.  The parent runs from its own
# tree (its own graal_amd package and library: the bindings of this tree expect graal_set_scan_path).
# usage: tools/scan_rows_ab.sh PARENT_TREE [PAIRS] [bench.py arguments ...]     (default: 7 pairs of --steps 20 --warmup 5)
# With GRAAL_SCAN_PATH=1 in the environment this tree streams every step: the pair then prices everything BUT the producer.
# Every run is printed; stops at the first run that fails.
here=$(cd "$(dirname "$0")/.." && pwd)
parent=$(cd "$1" && pwd) || exit 2
pairs=${2:-7}
shift; shift
args=("$@")
[ ${#args[@]} -eq 0 ] && args=(--steps 20 --warmup 5)
line='
import sys, json
for l in sys.stdin:
    if l.startswith("{"):
        j = json.loads(l)
        c = j.get("engine_counters", {})
        print("%-9s %.3f M evals/s  %.2f us/step  1000 steps: %s  indexed %s of %s evaluations, fallbacks %s" % (sys.argv[1], j["value"] / 1e6, 1e3 * j["ms_per_step"],
              ("%.3f M" % (j["value_1000"] / 1e6)) if "value_1000" in j else "-", c.get("indexed_passes", "-"), c.get("evaluations", "-"), c.get("fallbacks", "-")))
        break
else:
    sys.exit(3)
'
for ((p = 1; p <= pairs; p++)); do
  for who in parent candidate; do
    if [ $who = parent ]; then dir=$parent; else dir=$here; fi
    (cd "$dir" && env -u GRAAL_HIP_LIB timeout -k 10 560 python bench.py --gpus 1 "${args[@]}" 2>/dev/null) | python -c "$line" $who || { echo "$who: run failed"; exit 1; }
  done
done
