#!/bin/bash
# Headline benchmark, a built checkout of the parent commit and this tree alternated in one
# job on one GPU: ab.sh PARENT_DIR OUT.jsonl [ROUNDS].  One line per run:
# {"build": "parent" | "change", "result": <bench.py's JSON line>}; summary.py reads it.
set -o pipefail
parent=${1:?a built checkout of the parent commit}
out=$(realpath "${2:?output .jsonl}")
rounds=${3:-4}
here=$(cd "$(dirname "$0")/../.." && pwd)
: > "$out"
run() {   # run NAME DIR
  (cd "$2" && timeout -k 10 150 python bench.py --gpus 1 --steps 50 --warmup 10 | tail -1 |
     sed "s/^/{\"build\": \"$1\", \"result\": /; s/\$/}/") >> "$out"
}
for i in $(seq "$rounds"); do
  run parent "$parent" || { echo "parent run $i failed"; exit 1; }
  run change "$here" || { echo "change run $i failed"; exit 1; }
done
python "$here/bench/e2e_route/summary.py" "$out"
