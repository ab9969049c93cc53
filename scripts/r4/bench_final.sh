#!/bin/bash
# the default bench line (the driver's command) and smoke() at HEAD
set -o pipefail
O=${OUT:-bench_out/r4f}
mkdir -p "$O"
export PYTHONUNBUFFERED=1
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke2.log 2>&1 \
  || { tail -20 $O/smoke2.log; exit 1; }
tail -1 $O/smoke2.log
timeout -k 10 600 python -u bench.py --full > $O/bench_final.json 2> $O/bench_final.err \
  || { tail -20 $O/bench_final.err; exit 1; }
wc -l $O/bench_final.json
python scripts/bench_brief.py $O/bench_final.json
