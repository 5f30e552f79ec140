# parity tests + GEMM microbench + bench (no cpu baseline); logs go to $OUT (default bench_out/)
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1
rc=$?
echo "pytest rc=$rc"; tail -3 "$OUT/pytest_gpu.log"
if [ $rc -ne 0 ]; then grep -E "Error|assert|FAILED" "$OUT/pytest_gpu.log" | head -20; exit $rc; fi
timeout -k 10 120 python scripts/gemm_micro.py 20 > "$OUT/micro.log" 2>&1 || exit $?
grep TFLOP "$OUT/micro.log"
timeout -k 10 300 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline ${BENCH_ARGS} > "$OUT/bench.log" 2>&1 || exit $?
python - <<'PY'
import json,os
r=json.loads(open(os.path.join(os.environ["OUT"], "bench.log")).read().strip().splitlines()[-1])
print(r["value"], r["ms_per_step"], r["config"]["image_chunk"], {k:(v.get("tflops") or v.get("gbs")) for k,v in r["kernels"].items()})
PY
