# Round evidence on the GPU box (repo root): parity sweep, per-config bench lines, the full bench line, rocprofv3 kernel statistics +
# PMC counters (tools/profile_round.py), the near-tie census and a randomised differential run.  Everything but tools/profile_round.py's
# own output lands under $OUT (default evidence/) and is copied into profiles/ by hand afterwards.  usage: bash tools/round_evidence.sh r04
TAG=${1:-r06}
# second argument: the commit the evidence is taken at (the GPU box has no .git): bash tools/round_evidence.sh r06 $(git rev-parse --short HEAD)
export GACQ_EVIDENCE_HEAD=${2:-unknown}
OUT=${OUT:-evidence}
mkdir -p "$OUT"
echo "$GACQ_EVIDENCE_HEAD" > "$OUT/evidence_head.txt"
timeout 900 python tools/parity_sweep.py > "$OUT/parity_sweep.log" 2>&1
for c in 2 3 4 5; do timeout 600 python bench.py --config $c --steps 20 --warmup 5 --full --no-others 2>/dev/null | grep '^{' ; done > "$OUT/bench_lines.json"
timeout 900 python bench.py --full > "$OUT/bench_full_line.json" 2>/dev/null
timeout 1500 python tools/profile_round.py $TAG > "$OUT/profile_round.log" 2>&1
timeout 400 python tools/tie_census.py 20 4242 > "$OUT/tie_census.log" 2>&1
timeout 400 python tools/fuzz_engines.py 300 5501 > "$OUT/fuzz_engines.log" 2>&1
timeout 200 python tools/exp_epl_latency.py > "$OUT/epl_latency.log" 2>&1
tail -12 "$OUT/parity_sweep.log"
python - "$OUT/bench_lines.json" <<'PY'
import json, sys
for l in open(sys.argv[1]):
    j=json.loads(l); r=j["roofline"]
    print(j["config"]["baseline_config"], "%.4g"%j["value"], "%.3f ms"%j["ms_per_step"], r["bound"], r["kernel"], "%.3f"%r["frac"], r.get("traffic"), (r.get("traffic_source") or {}).get("measured_in_this_run"), "sustained %.4g"%j["sustained"]["value"], "cpu %.3g"%j["cpu_baseline"]["value"], j.get("tie_safe"))
PY
tail -3 "$OUT/tie_census.log" | cut -c1-300
tail -1 "$OUT/fuzz_engines.log" | cut -c1-600
