# GPU check: parity tests, smoke, short bench (--full: every secondary leg and check).  Each GPU
# step has its own time limit; a crash/timeout (not a plain test failure) stops the script.
# logs go to $OUT (default bench_out/)
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1
rc=$?
echo "pytest rc=$rc"
tail -5 "$OUT/pytest_gpu.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.build(); g.smoke()" > "$OUT/smoke.log" 2>&1 || exit $?
tail -2 "$OUT/smoke.log"
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---steps 3 --warmup 1} > "$OUT/bench.log" 2>&1
rc=$?
tail -c 3000 "$OUT/bench.log"
exit $rc
