#!/bin/bash
# round-end check on an MI355X: the whole GPU suite, then the full bench line (bench.py --full); logs under $OUT (default check_out/)
set -o pipefail
export OUT=${OUT:-check_out}
mkdir -p "$OUT"
( time python3 -m pytest tests -x -q -m gpu --durations=6 ) > "$OUT"/pytest_final.log 2>&1; rc=$?; echo "pytest gpu rc=$rc"; tail -14 "$OUT"/pytest_final.log
[ $rc -eq 0 ] || exit 1
( time python3 bench.py --full ) > "$OUT"/bench_final.log 2>&1; echo "bench rc=$?"; grep "^{" "$OUT"/bench_final.log > "$OUT"/bench_line_final.json; python3 - <<'PY'
import json, os
d=json.load(open(os.path.join(os.environ['OUT'], 'bench_line_final.json')))
e=d['extra']
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['traffic'], d['roofline']['traffic_source'])
for k,v in e.items():
    if k.startswith('mg_'): print(k, v.get('setup_secs_all'), v.get('solve_secs'), v.get('iters'), v.get('true_res'), (v.get('plain_gcr') or {}).get('iters'))
    else: print(k, json.dumps(v)[:500])
PY
tail -4 "$OUT"/bench_final.log | grep real
