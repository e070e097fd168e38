# One-GPU rehearsal of the driver's multi-GPU bench (2 ranks on cuda:0 over gloo: the strategies
# block, the timed bucket planner, replica digests) and the bucket-plan profile at 32 images
set -o pipefail
OUT=${OUT:-bench_logs}
mkdir -p $OUT
timeout -k 10 400 python bench.py --gpus 2 --dist-backend gloo --full --steps 5 --warmup 3 > $OUT/rehearsal2.log 2>&1 || { tail -30 $OUT/rehearsal2.log; exit 1; }
tail -1 $OUT/rehearsal2.log | cut -c1-600
timeout -k 10 200 python scripts/bucket_plan.py 32 > $OUT/bucket_plan_b32.md 2> $OUT/bucket_plan.err || { tail -20 $OUT/bucket_plan.err; exit 1; }
timeout -k 10 200 python scripts/bucket_plan.py 256 > $OUT/bucket_plan_b256.md 2>> $OUT/bucket_plan.err || { tail -20 $OUT/bucket_plan.err; exit 1; }
tail -5 $OUT/bucket_plan_b32.md
