#!/bin/bash
# interleaved A/B of library builds on one box: ab_libs.sh <rounds> "<bench args>" <name> <name> ...   (tools/exp/ablibs/lib_<name>.so; scratch copies)
# a run that fails or does not end within 5 minutes ends the whole comparison: nothing more is started on that device
set -e -o pipefail
rounds=$1; args=$2; shift 2
for r in $(seq 1 $rounds); do
  for v in "$@"; do
    cp tools/exp/ablibs/lib_$v.so uw-slam_amd/libuwt_hip.so
    timeout -k 10 300 python bench.py --cpu-pairs 0 --no-profile --steps 20 --warmup 5 $args 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$v#$r [$args]', d['value'], d['ms_per_step'])"
  done
done
