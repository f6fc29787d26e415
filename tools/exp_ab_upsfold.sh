#!/bin/bash
# Step-level evidence for the folded upsampler convolutions (ME_UPS_FOLD=0 | 1) on ONE box:  tools/exp_ab_upsfold.sh [pairs] [steps] [warmup] [parent tree]
#   1. `pairs` alternating runs of bench.py with the switch off / on -- the change counts as a gain only if EVERY fold-on run is faster than EVERY fold-off run;
#   2. with a built checkout of the parent commit as 4th argument: one run of it, and --dump-outputs of parent / off / on compared (off must be bitwise the parent);
#   3. one --full run each way (executed_tflop_per_step falls by ~3.6, the reference-semantics figure stays);
#   4. bench.py --vae-decode each way (secondary).
# A failing run prints bench.py's last stderr lines and ends the script.  The kernel traces are tools/collect_profiles.sh's business (runs of their own).
set -o pipefail
cd "$(dirname "$0")/.."
pairs=${1:-3}; n=${2:-20}; w=${3:-5}; parent=$4
T=$(mktemp -d)
run() {   # run <label> <dir> <env assignment> <bench.py arguments...>: prints "<label> <ms/step or value>"
  local label=$1 dir=$2 envv=$3; shift 3
  ( cd "$dir" && env $envv timeout -k 10 400 python bench.py "$@" 2> $T/err | grep '^{' | tail -1 > $T/line ) || { echo "$label: bench.py failed"; tail -5 $T/err; exit 1; }
  python - "$label" $T/line <<'PY' || exit 1
import json, sys
d = json.load(open(sys.argv[2]))
extra = f" executed {d['executed_tflop_per_step']} TFLOP, reference semantics {d['step_tflop_reference_semantics']}, gemm family {d['kernel_families']['gemm']['ms_per_step']} ms" if 'executed_tflop_per_step' in d else ''
print(sys.argv[1], d.get('ms_per_step', d['value']), 'ms/step' if 'ms_per_step' in d else d['unit'], extra)
PY
}
for i in $(seq 1 $pairs); do
  for val in 0 1; do run "ME_UPS_FOLD=$val pair $i" . ME_UPS_FOLD=$val --gpus 1 --steps $n --warmup $w; done
done
if [ -n "$parent" ]; then
  run "parent commit" "$parent" ME_UPS_FOLD=1 --gpus 1 --steps $n --warmup $w --dump-outputs $T/parent
  run "ME_UPS_FOLD=0 (dump run)" . ME_UPS_FOLD=0 --gpus 1 --steps $n --warmup $w --dump-outputs $T/off
  run "ME_UPS_FOLD=1 (dump run)" . ME_UPS_FOLD=1 --gpus 1 --steps $n --warmup $w --dump-outputs $T/on
  python - $T <<'PY'
import glob, os, sys
import numpy as np
t = sys.argv[1]
for a in sorted(glob.glob(t + '/parent/*.npy')):
    n = os.path.basename(a)
    p, off, on = np.load(a), np.load(f'{t}/off/{n}'), np.load(f'{t}/on/{n}')
    print(f"dump {n}: ME_UPS_FOLD=0 vs parent bitwise {'EQUAL' if p.tobytes() == off.tobytes() else 'DIFFERENT'}; fold on vs off rel-L2 {np.linalg.norm(on.astype(np.float64) - off) / np.linalg.norm(off):.3e}")
PY
fi
for val in 0 1; do run "ME_UPS_FOLD=$val --full" . ME_UPS_FOLD=$val --gpus 1 --full --steps $n --warmup $w --no-cpu-baseline; done
for val in 0 1; do run "ME_UPS_FOLD=$val --vae-decode" . ME_UPS_FOLD=$val --vae-decode --steps 5 --warmup 2; done
rm -rf $T
