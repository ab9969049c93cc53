#!/bin/bash
# last closing run at HEAD: the whole GPU suite, smoke(), the default bench line
set -o pipefail
O=${OUT:-bench_out/r4f}
mkdir -p "$O"
export PYTHONUNBUFFERED=1
T="timeout -k 10"
$T 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
  -p no:cacheprovider > $O/gpu_suite_last.log 2>&1 || { tail -60 $O/gpu_suite_last.log; exit 1; }
tail -1 $O/gpu_suite_last.log
$T 120 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke_last.log 2>&1 \
  || { tail -20 $O/smoke_last.log; exit 1; }
tail -1 $O/smoke_last.log
$T 600 python -u bench.py --full > $O/bench_last.json 2> $O/bench_last.err \
  || { tail -20 $O/bench_last.err; exit 1; }
wc -l < $O/bench_last.json
python scripts/bench_brief.py $O/bench_last.json > $O/bench_last_brief.txt
grep -E "head|train_step|literal|bip1m|syn2m|bf16 " $O/bench_last_brief.txt
