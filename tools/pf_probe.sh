set -u
O=${O:-bench_out}
mkdir -p $O
timeout -k 10 200 python3 bench.py --per-frame-only --steps 2 --coalesce 32 > $O/pf_a.log 2>&1 || exit $?
timeout -k 10 300 python3 bench.py --full --steps 8 --no-cpu-baseline --no-framed > $O/pf_b.log 2>&1 || exit $?
timeout -k 10 300 python3 bench.py --full --steps 8 --no-cpu-baseline > $O/pf_c.log 2>&1 || exit $?
