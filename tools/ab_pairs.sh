out=${BENCH_OUT:-bench_out}; mkdir -p "$out"          # where the JSON lines are kept
for P in 32 16; do for mode in classic st; do
  if [ $mode = classic ]; then export LINETR_SIG_PATH=classic; else unset LINETR_SIG_PATH; fi
  python bench.py --full --pairs $P --steps 20 --warmup 3 --no-cpu-baseline --no-sub-workloads 2>/dev/null | tail -1 > "$out/ab_p${P}_$mode.json"
  python - $P $mode "$out/ab_p${P}_$mode.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[3]))
print(f"== pairs {sys.argv[1]} {sys.argv[2]}: {d['value']/1e6:.3f} M desc/s, {d['ms_per_step']:.3f} ms/step")
for k, v in sorted(d["kernels"].items(), key=lambda kv: -kv[1]["ms"])[:4]:
    print(f"   {k:28s} {v['calls']:3d} x  {v['ms']:.4f} ms  {v['tflops']}")
PY
done; done
