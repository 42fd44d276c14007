# default bench repeated (no CPU baseline / extras; --full for the calibration step behind `pipeline`)
o=$(mktemp)
for i in 1 2 3 4; do
timeout 200 python bench.py --full --no-cpu-baseline --no-extras > $o 2>/dev/null
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['value'], d['ms_per_step'], d['roofline']['achieved'], d['pipeline']['sustained_tflops'], d['host_cpu_cores_busy_per_gpu'])" $o
done
rm -f $o
