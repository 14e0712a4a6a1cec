#!/bin/bash
# A/B session: parity of one variant library (the whole -m gpu suite against it), then a bench sweep.
#   LIB=variants/lib_x.so SWEEP=tools/sweepNN.txt bash tools/ab.sh
set -u
export O=${O:-bench_out}
mkdir -p $O
if [ -n "${LIB:-}" ]; then
  HALOGEN_LIB=$LIB timeout -k 10 300 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $O/pt_ab.log 2>&1
  rc=$?; tail -4 $O/pt_ab.log; [ $rc -le 1 ] || exit $rc
fi
SWEEP_TIMEOUT=${SWEEP_TIMEOUT:-200} bash tools/sweep.sh "$SWEEP" || exit $?
python3 - <<'PY'
import json, os
for l in open(os.environ["O"] + "/sweep.jsonl"):
    r = json.loads(l)
    print(f"{r['value']:8.1f} {r.get('simd_utilisation')} {r['args']}")
PY
