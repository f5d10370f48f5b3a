#!/bin/bash
# split engine: parity suite, bench at the default geometry and with 8-lane groups
cd "$GRAFT_REPO_ROOT" || exit 1
export O=${OUT_DIR:-build/ab_geometries}; mkdir -p $O
timeout 900 python -m pytest tests -m gpu -x -q 2>&1 | tail -4 > $O/split_tests.log
cat $O/split_tests.log
timeout 600 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/bench_split.json 2> $O/bench_split.err
python - <<'PY'
import json, os
for f in ("bench_split",):
    d=json.loads(open(os.path.join(os.environ["O"], "%s.json"%f)).read().strip().splitlines()[-1])
    print(f, d["value"], d["decrypt"]["value"], d["config"]["geometry"])
PY
PHE_HIP_GROUP=8 timeout 600 python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $O/bench_g8.json 2> $O/bench_g8.err
PHE_HIP_GROUP=4 timeout 600 python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $O/bench_g4.json 2> $O/bench_g4.err
python - <<'PY'
import json, os
for f in ("bench_g8","bench_g4"):
    try:
        d=json.loads(open(os.path.join(os.environ["O"], "%s.json"%f)).read().strip().splitlines()[-1])
        print(f, d["value"], d["decrypt"]["value"], d["config"]["geometry"])
    except Exception as e: print(f, "failed", e)
PY
