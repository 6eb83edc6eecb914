# Clock-probe check: the probe's GPU test, then three bench runs' clock fields.
set -o pipefail
export OUT=${OUT:-logs}  # where the logs go
mkdir -p $OUT
timeout -k 10 200 python -u -m pytest -x -v --timeout 120 --timeout-method thread tests/test_gpu_probe.py -m gpu > $OUT/probe.log 2>&1 || { tail -30 $OUT/probe.log; exit 1; }
tail -2 $OUT/probe.log
for i in 1 2 3; do
  timeout -k 10 120 python bench.py --full --cpu-budget-s 0 > $OUT/bench$i.log 2>&1 || exit 1
  grep "^{" $OUT/bench$i.log | python -c "import sys,json; d=json.loads(sys.stdin.readline()); print(d['value'], d['sclk_mhz_timed'], d['clock']['per_xcd_mhz'])"
done
