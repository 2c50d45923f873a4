cd "$(dirname "$0")/.."; export TMPDIR=/tmp; D=${PROF_OUT:-prof_out}; C=${1:-c4}; T=${2:-r05c}_$C; mkdir -p $D/$T
rocprofv3 --kernel-trace --stats --output-format csv -d $D/$T/trace -- python3 bench.py --full --config $C --steps 8 --warmup 3 --no-cpu-baseline --no-gemm-alone > $D/$T/bench_profiled.json 2> $D/$T/bench_profiled.err
python scripts/timeline.py $(find $D/$T/trace -name "*kernel_trace.csv" | head -1) 5 > $D/$T/timeline.txt 2>&1
cp $(find $D/$T/trace -name "*kernel_stats.csv" | head -1) $D/$T/kernel_stats.csv
rm -rf $D/$T/trace
timeout 900 python bench.py --full --config $C > $D/$T/bench.json 2> $D/$T/bench.err; echo "rc $?"
python - <<PY
import json
d=json.load(open('$D/$T/bench.json'))
print(d['value'], d['ms_per_step'], json.dumps(d['ms_per_step_by_entry_point']))
for k,v in d['roofline']['families_in_step'].items(): print(k[:40], v['ms_per_step'], v['frac'], v['executed_frac'])
PY
head -25 $D/$T/kernel_stats.csv | cut -c1-150
