# Round-5 verification and measurement on one lease: every GPU test, smoke(),
# the bench lines (C2 long and the driver's short form x3, C4, C5 steady /
# default, SuperGridRL, C2 + dijkstra) and the rocprofv3 profiles of the timed
# steps (kernel trace, FETCH_SIZE / WRITE_SIZE, SQ counters) of C2, C4, C5.
#   TAG=r5/final [SKIP_TESTS=1] [SKIP_PROF=1] bash tools/gpu_r5_final.sh
set -u
R="$GRAFT_REPO_ROOT"; OUT="$R/gpurun_out/${TAG:-r5/final}"; mkdir -p "$OUT"; cd "$R"
if [ -z "${SKIP_TESTS:-}" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1 || { tail -40 "$OUT/gpu_tests.log"; exit 1; }
  tail -1 "$OUT/gpu_tests.log"
  timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { tail -5 "$OUT/smoke.log"; exit 1; }
  tail -1 "$OUT/smoke.log"
fi
b() {  # name, args...
  local n=$1; shift
  timeout -k 10 400 python3 bench.py "$@" > "$OUT/bench_$n.json" 2> "$OUT/bench_$n.err" || { tail -5 "$OUT/bench_$n.err"; exit 1; }
  python3 -c "import json; d=json.load(open('$OUT/bench_$n.json')); r=d['roofline']; print('$n', round(d['value']/1e6,2), 'M', d['ms_per_step']*1e3, 'us/step', r['kernel_us'], 'kernel_us frac', r['frac'])"
}
b c2 --full
for i in 1 2 3; do b c2_short_$i --gpus 1 --steps 20 --warmup 5 --no-cpu; done
b c4 --config c4 --steps 50 --warmup 5 --no-cpu
b c5_steady --config c5 --steps 30 --warmup 600 --no-cpu
b c5 --config c5 --no-cpu
b sg_c2 --config sg_c2 --no-cpu
b c2_dijkstra --config c2_dijkstra --no-cpu
[ -n "${SKIP_PROF:-}" ] && exit 0
timeout -k 10 900 python3 tools/prof_config.py --config c2 --steps 200 --warmup 20 --sq --out "$OUT/prof/c2" > "$OUT/prof_c2.log" 2>&1 || { tail -5 "$OUT/prof_c2.log"; exit 1; }
timeout -k 10 900 python3 tools/prof_config.py --config c4 --steps 30 --warmup 5 --sq --out "$OUT/prof/c4" > "$OUT/prof_c4.log" 2>&1 || { tail -5 "$OUT/prof_c4.log"; exit 1; }
timeout -k 10 900 python3 tools/prof_config.py --config c5 --steps 30 --warmup 600 --sq --out "$OUT/prof/c5_steady" > "$OUT/prof_c5.log" 2>&1 || { tail -5 "$OUT/prof_c5.log"; exit 1; }
echo prof done
exit 0
