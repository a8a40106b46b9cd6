# forward-stage time of the wide kernel under ablation flags (HSR_FWD_DEBUG): usage bash tools/ablate_wide.sh 102
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
K=${1:-102}
for f in 0 1 2 3 4 6; do
  HSR_FWD_DEBUG=$f python bench.py --full --no-workloads --no-cpu-baseline --steps 20 --warmup 3 --P 500000 --K $K > $OUT/abl_$f.json
  python -c "import json;d=json.load(open('$OUT/abl_$f.json'));print('flags $f fwd_render %.3f ms' % d['stages_ms']['fwd_render'])"
done
