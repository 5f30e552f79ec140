# Secondary BASELINE configs on one GPU (parity-test cases, not the bench line):
# configs[2] ViT-L/14 bf16 (x256 queries) and configs[4]'s model ViT-L/14@336px (x1000 queries).
# logs go to $OUT (default bench_out/)
OUT=${OUT:-bench_out}
mkdir -p "$OUT/cfg"
timeout -k 10 400 python bench.py --full --model ViT-L/14 --frames ${L14_FRAMES:-20000} --queries 256 --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/cfg/l14.log" 2>&1 || exit $?
tail -1 "$OUT/cfg/l14.log"
timeout -k 10 400 python bench.py --full --model ViT-L/14@336px --frames ${L336_FRAMES:-5000} --queries 1000 --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/cfg/l336.log" 2>&1 || exit $?
tail -1 "$OUT/cfg/l336.log"
