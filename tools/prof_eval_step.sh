#!/bin/bash
# per-kernel times and launches per step of the evaluation step:
#   bash tools/prof_eval_step.sh TAG B L R [--shipped] [--mbr] [--no-metrics]
#   -> build/prof/TAG_eval_step_kernel_stats.csv, build/prof/TAG_eval_step.log (launch count, metric-launch time)
set -o pipefail
tag=${1:?tag}; shift
mkdir -p build/prof
out=build/prof/prof_${tag}_es
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$out" -- python tools/time_eval_step.py --one "$@" > build/prof/${tag}_eval_step.log 2>&1 || { tail -20 build/prof/${tag}_eval_step.log; exit 1; }
f=$(find "$out" -name "*kernel_stats.csv" | head -1); cp "$f" build/prof/${tag}_eval_step_kernel_stats.csv
python tools/time_eval_step.py --count "$out" | tee -a build/prof/${tag}_eval_step.log
