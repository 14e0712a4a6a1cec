#!/bin/bash
# Configuration sweep of bench.py --full, one process per line.  A line is "[VAR=value ...] bench-args"; VAR=value
# words (e.g. HALOGEN_LIB=variants/lib_w8.so) become the environment of that run.  Stops on a fault/timeout.
# The lines' own --no-... options prune the legs; the results go to $O/sweep.jsonl (O defaults to bench_out).
set -u
O=${O:-bench_out}
mkdir -p $O
OUT=$O/sweep.jsonl
: > $OUT
while read -r line; do
  [ -z "$line" ] && continue
  envs=(); args=()
  for w in $line; do
    if [[ "$w" == *=* && "$w" != --* ]]; then envs+=("$w"); else args+=("$w"); fi
  done
  env "${envs[@]}" timeout -k 10 ${SWEEP_TIMEOUT:-300} python bench.py --full --no-cpu-baseline "${args[@]}" > $O/sweep_one.json 2> $O/sweep_one.err
  rc=$?
  if [ $rc -ne 0 ]; then echo "FAILED rc=$rc: $line"; tail -5 $O/sweep_one.err; exit $rc; fi
  python3 -c "
import json,sys; r=json.loads(open('$O/sweep_one.json').read().strip().splitlines()[-1])
r['args']='$line'; print(json.dumps(r))
k=r.get('kernel_ms',{})
tr=(k.get('trace_total',0)/max(k.get('trace_launches',1),1))
print(f\"{r['value']:9.1f} Mpaths/s {r['ms_per_step']:9.3f} ms/step trace_total={k.get('trace_total',0):8.1f}ms  $line\", file=sys.stderr)" >> $OUT
done < "${1:-/dev/stdin}"
