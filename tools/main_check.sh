#!/bin/bash
# GPU box: the forward kernel after a loader change -- fold forms (bit-identity), goldens, full-size cases, stamps; then the default bench line twice.
export NCX_OUT=${NCX_OUT:-out}          # output folder of this script (relative to the repository root)
mkdir -p "$NCX_OUT"
timeout -k 10 500 python -m pytest tests -x -q -m gpu -k "fold_forms or configs1 or golden or ragged or distance_inside or phased_forward or clock_stamps or x6_forward" > $NCX_OUT/main_tests.log 2>&1; echo "pytest rc $?"; tail -3 $NCX_OUT/main_tests.log
timeout -k 10 200 python tools/main_stamps.py > $NCX_OUT/main_stamps.log 2>&1; tail -6 $NCX_OUT/main_stamps.log
for i in 1 2; do timeout -k 10 200 python bench.py --full --no-cpu-baseline > $NCX_OUT/main_bench$i.json 2> $NCX_OUT/main_bench$i.err; done
python - <<'PY'
import os; OUT = os.environ["NCX_OUT"]
import json
for f in (OUT + "/main_bench1.json", OUT + "/main_bench2.json"):
    j = json.loads([l for l in open(f) if l.startswith("{")][-1])
    print(f, j["ms_per_step"], "ms", j["value"], "triplets/s", {k: v["launch_ms"] for k, v in j["roofline"]["other"].items()}, "frac", j["roofline"]["frac"])
PY
