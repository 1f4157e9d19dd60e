#!/bin/bash
# What the driver does at round end, on one MI355X:  pytest -m gpu, smoke(), the full bench line, the torchrun launch.
#   bash tools/gpu_scripts/round_check.sh <out dir>
# Every GPU step has a time limit of its own; the first one that fails ends the script.
set -x
O=${1:?usage: round_check.sh <out dir>}
mkdir -p "$O"
export TMPDIR=/tmp
FK_PARITY_LOG=$O/parity_errors.jsonl timeout -k 10 1500 python -m pytest tests -m gpu -q -x -p no:cacheprovider > "$O/pytest_gpu.log" 2>&1; rc=$?
echo "pytest rc=$rc"; tail -4 "$O/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1; rc=$?
echo "smoke rc=$rc"; tail -2 "$O/smoke.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$O/bench_default.json" 2> "$O/bench_default.err"; rc=$?
echo "bench rc=$rc"; cat "$O/bench_default.json"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 \
    bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu > "$O/bench_torchrun.json" 2> "$O/bench_torchrun.err"; rc=$?
echo "torchrun rc=$rc"; exit $rc
