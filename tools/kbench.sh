set -e
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for k in 74 102; do python bench.py --full --no-workloads --no-cpu-baseline --steps 30 --warmup 5 --P 500000 --K $k > $OUT/k$k.json; done
python - "$OUT" <<'PY'
import json, sys
for k in (74,102):
    d=json.load(open(sys.argv[1] + "/k%d.json"%k)); print(k, round(d["value"],1), {a:round(b,3) for a,b in d["stages_ms"].items()})
PY
