#!/bin/bash
# run bench.py once per variant library: tools/ab.sh TAG NAME1 NAME2 ...   (results: $AB_OUT/ab_TAG_NAME.{json,err}, default ab_out/)
TAG=$1; shift
O=${AB_OUT:-ab_out}; mkdir -p $O
for n in "$@"; do
  if [ "$n" == "base" ]; then L=""; else L="$PWD/_variants/libyololite_hip_$n.so"; fi
  YOLOLITE_HIP_LIB=$L python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --layers > $O/ab_${TAG}_$n.json 2> $O/ab_${TAG}_$n.err
  python - <<PY
import json; d=json.load(open("$O/ab_${TAG}_$n.json")); print("$n", d["value"], d["network"]["forward_ms_sum_of_layers"])
PY
done
