# the --full line's per-layer and per-kernel launch times: tools/bench_layers.sh [FILE]  (FILE keeps the line)
f=${1:-$(mktemp)}
python bench.py --full --steps 100 --warmup 20 --no-cpu-baseline --no-secure --sustain-s 0 2>/dev/null | tail -1 > "$f"
python - "$f" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print(d['value'], d['ms_per_step'], d['roofline']['kernel'], d['roofline']['frac'])
L=d['roofline']['layers_us']
for k,v in L.items(): print(f"{k:32s} {v:8.1f}")
for k,v in d['roofline']['kernels'].items(): print(k[:60], v)
PY
