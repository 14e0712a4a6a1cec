set -u
# shading sub-phase clock split of the streaming kernel (analysis builds with HG_PHASE_DETAIL=1 / 2)
O=${O:-bench_out}
mkdir -p $O
for v in ${PHASES:-phase phase2 phase3}; do
  timeout -k 10 300 env HALOGEN_LIB=variants/lib_$v.so python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/${v}_C3.json 2> $O/${v}_C3.err || exit $?
  python3 -c "import json; r=json.load(open('$O/${v}_C3.json')); print('$v', round(r['value']), r['phase_split'], r['shading_detail'])"
done
