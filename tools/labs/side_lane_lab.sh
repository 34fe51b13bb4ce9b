#!/bin/bash
# tools/labs/side_lane_lab.cpp on the GPU box's host (no GPU is touched): the single pwrite thread, the warm-then-write
# pair, and the pair with 1, 2 and 3 side threads that populate and fill pages through a shared mapping -- side blocks of
# 256 KiB, 512 KiB and 2 MiB, the mapping one window per piece (0) or long-lived windows of 256 MiB and 1 GiB --
# interleaved, five repetitions, every process under its own time limit; the first failure ends the run.  Then mean and
# range per variant and the stop rule: a variant counts only when its slowest repetition beats the pair's fastest.
#
#   g++ -O2 -std=c++17 tools/labs/side_lane_lab.cpp -o tools/labs/build/side_lane_lab -lpthread
#   tools/labs/side_lane_lab.sh [dir=/dev/shm] [out=side_lane_lab.log] [reps=5]
set -euo pipefail
DIR=${1:-/dev/shm}
OUT=${2:-side_lane_lab.log}
REPS=${3:-5}
LAB=$(dirname "$0")/build/side_lane_lab
mkdir -p "$(dirname "$OUT")"
{ echo "# $(uname -r), $(nproc) CPUs, $(df --output=fstype "$DIR" | tail -1) at $DIR"; } > "$OUT"
for rep in $(seq "$REPS"); do
  timeout -k 10 120 "$LAB" "$DIR" 1 0 0 0 | tee -a "$OUT"
  timeout -k 10 120 "$LAB" "$DIR" 2 0 0 0 | tee -a "$OUT"
  for window in 0 256 1024; do
    for block in 256 512 2048; do
      for side in 1 2 3; do
        timeout -k 10 120 "$LAB" "$DIR" 2 $side $block $window | tee -a "$OUT"
      done
    done
  done
done
python3 - "$OUT" <<'EOF' | tee -a "$OUT"
import json, sys
runs = {}
for line in open(sys.argv[1]):
    if line.startswith("{"):
        d = json.loads(line)
        runs.setdefault((d["lane"], d["side"], d["block_KiB"], d["window_MiB"]), []).append(d)
pair = [d["GBps"] for d in runs[(2, 0, 0, 0)]]
print("# variant: lane side block_KiB window_MiB | GB/s mean (min - max) | pwrite / populate / copy us per 16 MiB | side share")
winners = []
for key in sorted(runs):
    v = [d["GBps"] for d in runs[key]]
    m = lambda f: sum(d[f] for d in runs[key]) / len(runs[key])
    print("# %d %d %4d %4d | %.2f (%.2f - %.2f) | %.0f / %.0f / %.0f | %.2f" % (key + (sum(v) / len(v), min(v), max(v),
          m("pwrite_us_per_16MiB"), m("populate_us_per_16MiB"), m("copy_us_per_16MiB"), m("side_share"))))
    if key[1] != 0 and min(v) > max(pair):
        winners.append(key)
print("# pair %.2f - %.2f GB/s; variants whose slowest repetition beats its fastest: %s" % (min(pair), max(pair), winners or "none"))
EOF
