set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-run_out/r5r}
mkdir -p $OUT
timeout -k 10 800 python -u -m pytest tests/test_gpu_dist.py -x -v -m gpu --timeout 780 --timeout-method thread > $OUT/pytest.log 2>&1 || { tail -40 $OUT/pytest.log; exit 1; }
tail -3 $OUT/pytest.log
timeout -k 10 600 python bench.py --full --no-cpu --no-cstr --no-ntt > $OUT/bench.log 2>&1 || { tail -30 $OUT/bench.log; exit 1; }
OUT=$OUT python - <<'PY'
import json, os
d = json.loads([l for l in open(os.environ["OUT"] + "/bench.log") if l.startswith('{"metric"')][-1])
h = d["config5"]["hempc_gemv"]
print("headline", round(d["value"]), "c5", round(d["config5"]["value"]), "c5 hempc gemv", round(h["value"]), "gemv/s", round(h["us_per_gemv_per_gpu"], 1), "us")
for k, v in h["kernels"].items():
    print("  ", k, round(v["avg_us"], 1), round(v["us_per_gemv"], 2))
PY
