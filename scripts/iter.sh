#!/bin/bash
# One development iteration on an MI355X: selected GPU tests, the phase-stamped driver
# (scripts/dbg/ph, if built) and a short emb bench line.  Every GPU step has its own limit.
# Logs go to $OUT_DIR (default iter_out/).
set -u
O="${OUT_DIR:-iter_out}"
cd "$(dirname "$0")/.."; mkdir -p "$O"
T="${TESTS:-tests/test_gpu_fused.py tests/test_gpu_parity.py tests/test_gpu_vc.py}"
if [ "$T" != "none" ]; then
  timeout -k 10 600 python -u -m pytest $T -m gpu -x -q --tb=short --timeout 300 --timeout-method thread > "$O/pytest_it.log" 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -3 "$O/pytest_it.log" | cut -c1-300; [ $rc -eq 0 ] || { grep -E "Error|assert" "$O/pytest_it.log" | head -20; exit $rc; }
fi
if [ -x scripts/dbg/ph/avc_bench ] && [ "${PH:-1}" = 1 ]; then
  timeout -k 10 120 scripts/dbg/ph/avc_bench 256 128 20 1 1 1 ${PH_ATTACK:-0} > "$O/ph.log" 2>&1
  rc=$?; echo "phases rc=$rc"; [ $rc -eq 0 ] || exit $rc
fi
for A in ${ATTACKS-emb}; do
  # --full for the roofline figures printed below
  timeout -k 10 300 python bench.py --attack $A --steps 1 --warmup 1 --full --no-cpu-baseline --no-fp32-compare > "$O/bench_q_$A.log" 2>&1
  rc=$?; echo "bench $A rc=$rc"; [ $rc -eq 0 ] || { tail -3 "$O/bench_q_$A.log"; exit $rc; }
  python - "$O/bench_q_$A.log" "$A" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[2], d["value"], "utts/s", "frac", d["roofline"]["frac"], {k: v["avg_ms"] for k, v in d["roofline"]["per_kernel"].items()})
PY
done
echo ALL_OK
