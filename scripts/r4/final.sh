#!/bin/bash
# Round-4 closing run: the whole GPU suite (one process), the default bench line (the
# driver's command), smoke(), and the C4 bf16 row-score A/B (MSHA_ROW_SCORES=1 vs default).
set -o pipefail
O=${OUT:-bench_out/r4f}
mkdir -p "$O"
export PYTHONUNBUFFERED=1
T="timeout -k 10"
$T 900 python -u -m pytest tests -m gpu -x -q -rs --timeout 300 --timeout-method thread \
  -p no:cacheprovider > $O/gpu_suite.log 2>&1 || { tail -60 $O/gpu_suite.log; exit 1; }
tail -3 $O/gpu_suite.log
$T 120 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1 \
  || { tail -20 $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
$T 600 python -u bench.py --full > $O/bench_line.json 2> $O/bench.err \
  || { tail -20 $O/bench.err; exit 1; }
python scripts/bench_brief.py $O/bench_line.json | head -40
for RS in 1 0; do
  MSHA_ROW_SCORES=$RS $T 300 python -u bench.py --full --workload syn100k --steps 20 --warmup 5 --no-cpu-baseline \
    --no-r15 --no-syn2m --no-bip1m --no-link-score --no-dropout-leg > $O/rs$RS.json 2> $O/rs$RS.err \
    || { tail -20 $O/rs$RS.err; exit 1; }
  echo "== MSHA_ROW_SCORES=$RS"; python scripts/bench_brief.py $O/rs$RS.json | grep -i "bf16\|head" | head -6
done
