#!/bin/bash
# GPU-box A/B of the GroupNorm statistics pass (loads in flight per thread), then the suite pieces that depend on it.
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
mkdir -p "${OUT_DIR:?set OUT_DIR to the directory the results go to}"; O=$(cd "$OUT_DIR" && pwd)
export TMPDIR=/tmp
out=$O/gn_ab.txt
: > $out
for v in old u4 "" u16 u8a8 old ""; do
  lib=$R/motioneditor_amd/libmotioned.so
  [ -n "$v" ] && lib=$R/tools/_bin/libmotioned_gn_$v.so
  echo "== ${v:-u8 (tree)}" >> $out
  ME_LIB=$lib timeout 200 python tools/kbench.py gn 2>&1 | grep -i "groupnorm" >> $out
done
timeout 900 python -m pytest tests/test_kernels_gpu.py tests/test_model_gpu.py -m gpu -q -x -p no:cacheprovider -k "groupnorm or norm or planned or full_size_properties or unet_single or config0" > $O/gn_pytest.log 2>&1
echo "pytest exit $?" >> $out
tail -3 $O/gn_pytest.log >> $out
timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $O/gn_smoke.log 2>&1
echo "smoke exit $?" >> $out
tail -2 $O/gn_smoke.log >> $out
timeout 400 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline 2>&1 | tail -1 > $O/gn_bench.json
python - "$O/gn_bench.json" <<'PY' >> $out
import json, sys
d = json.load(open(sys.argv[1]))
print("bench ms/step", d["ms_per_step"], "host", d["host_enqueue_ms_per_step"], "plan", d["config"].get("launch_plan_replay"), {k: v for k, v in d.get("kernel_families", {}).items()} if isinstance(d.get("kernel_families"), dict) else "")
PY
cat $out
