#!/bin/bash
# Same-box A/B of pytorch-openpose_amd/lib/ab_base.so (the previous build) against the default
# library: raw outputs bit-identity (scripts/ab_outputs.py), then bench.py --full --steps 20
# alternated (frames/s, C2 latency, Hand latency, serial 3x3 / 7x7 class ms).  Results go to
# $AB_OUT (default: ab_out/ in the repository root).
cd "$(dirname "$0")/.." && OUT=${AB_OUT:-ab_out} && mkdir -p $OUT && export TMPDIR=/tmp
OPOSE_LIB=pytorch-openpose_amd/lib/ab_base.so timeout -k 10 200 python scripts/ab_outputs.py save $OUT/ab_a.npz > /dev/null 2>&1 || exit 1
timeout -k 10 200 python scripts/ab_outputs.py save $OUT/ab_b.npz > /dev/null 2>&1 || exit 1
python scripts/ab_outputs.py compare $OUT/ab_a.npz $OUT/ab_b.npz | grep -c "bit-identical" || exit 1
for round in 1 2; do
for L in pytorch-openpose_amd/lib/ab_base.so ""; do
  if [ -n "$L" ]; then export OPOSE_LIB=$L; else unset OPOSE_LIB; fi
  timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu > $OUT/ab_bench.json 2>/dev/null || exit 1
  python -c "
import json; d = json.loads(open('$OUT/ab_bench.json').read().strip().splitlines()[-1])
s = d['stage_ms_per_step']
print('lib %s: %.1f frames/s  C2 %.3f ms  hand %.3f ms  serial 3x3 %.4f 7x7 %.4f 1x1 %.4f assemble %.4f gauss %.4f | pipelined assemble %.4f gauss %.4f' % ('base' if '$L' else 'new', d['value'], d['latency_ms_single_frame'], d['c3_hand']['latency_ms'], s['conv3x3'], s['conv7x7'], s['conv1x1'], s['assemble'], s['gauss_nms_resize'], d['stage_ms_per_step_pipelined']['assemble'], d['stage_ms_per_step_pipelined']['gauss_nms_resize']))"
done
done
