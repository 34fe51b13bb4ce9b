#!/bin/bash
# tools/labs/warm_write_lab.hip on the GPU box: the pipeline's writer as it is (a), the warm-then-write pair (b) and trio (c)
# at five sub-piece sizes, one thread that warms its own sub-pieces (w), and every one of them again with the piece
# page-congruent in its slab (d) -- interleaved, three repetitions, every process under its own time limit; the first
# failure ends the run.  Then mean and range per variant and the stop rule: a variant counts only when its lowest
# repetition lies above the baseline's highest.
#
#   hipcc -O2 --offload-arch=gfx950 tools/labs/warm_write_lab.hip -o tools/labs/build/warm_write_lab -lpthread
#   tools/labs/warm_write_lab.sh [dir=/dev/shm] [out=warm_write_lab.log]
set -euo pipefail
DIR=${1:-/dev/shm}
OUT=${2:-warm_write_lab.log}
LAB=$(dirname "$0")/build/warm_write_lab
mkdir -p "$(dirname "$OUT")"
: > "$OUT"
for rep in 1 2 3; do
  for congruent in 0 1; do
    timeout -k 10 120 "$LAB" "$DIR" 1 16384 0 $congruent | tee -a "$OUT"
    timeout -k 10 120 "$LAB" "$DIR" 1 1024 1 $congruent | tee -a "$OUT"
    for sub in 256 512 1024 2048 4096; do
      for threads in 2 3; do
        timeout -k 10 120 "$LAB" "$DIR" $threads $sub 1 $congruent | tee -a "$OUT"
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
        runs.setdefault((d["threads"], d["warm"], d["sub_KiB"], d["congruent"]), []).append(d)
base = [d["GBps"] for d in runs[(1, 0, 16384, 0)]]
print("# variant: threads warm sub_KiB congruent | GB/s mean (min - max) | pwrite / warm / ticket wait us per 16 MiB")
winners = []
for key in sorted(runs):
    v = [d["GBps"] for d in runs[key]]
    m = lambda f: sum(d[f] for d in runs[key]) / len(runs[key])
    print("# %d %d %5d %d | %.2f (%.2f - %.2f) | %.0f / %.0f / %.0f" % (key + (sum(v) / len(v), min(v), max(v),
          m("pwrite_us_per_16MiB"), m("warm_us_per_16MiB"), m("ticket_wait_us_per_16MiB"))))
    if key != (1, 0, 16384, 0) and min(v) > max(base):
        winners.append(key)
print("# baseline %.2f - %.2f GB/s; variants whose lowest repetition lies above its highest: %s" % (min(base), max(base), winners or "none"))
EOF
