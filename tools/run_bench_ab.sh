#!/bin/bash
# developer A/B on the GPU box, UNTRACED: bench.py headline (no CPU baseline, no other configs) alternating between the
# in-tree library and the parent's:  tools/run_bench_ab.sh _variants/libyololite_hip_parent.so [rounds] [extra bench args]
# (the parent's library: build the parent commit in a `git worktree` -- python yololite-official-repo_amd/csrc/build.py there --
# and copy its libyololite_hip.so to _variants/, which git ignores).  AB_ORDER="new old" runs the in-tree library first.
# Stops at the first run that does not end with status 0: after a fault or a time limit nothing more is started on the GPU.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd) || exit 1   # the repository: this script lies in its tools/
export TMPDIR=/tmp
cd $ROOT || exit 1
OLD=$1; R=${2:-3}; shift 2
for r in $(seq $R); do
  for w in ${AB_ORDER:-old new}; do
    if [ $w == old ]; then export YOLOLITE_HIP_LIB=$ROOT/$OLD; else unset YOLOLITE_HIP_LIB; fi
    echo -n "$w "; timeout -k 5 200 python bench.py --full --no-cpu-baseline --other-configs 0 "$@" 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['blocks']['images_per_sec_min'], d['blocks']['images_per_sec_max'])" || { s=$?; echo "run_bench_ab: $w run $r ended with status $s, stopping"; exit $s; }
  done
done
