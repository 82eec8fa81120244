set -u
OUT=${1:?usage: bash tools/profile_all.sh OUT_DIR}
bash tools/profile_round.sh "$OUT" C > "$OUT.log" 2>&1
for i in 1 2 3; do timeout 600 python3 bench.py --full --steps 20 --warmup 5 > "$OUT/driver_form_run$i.json" 2> "$OUT/driver_form_run$i.err"; done
timeout 900 python3 bench.py --full --workload D > "$OUT/bench_d_line.json" 2> "$OUT/bench_d.err"
timeout 900 python3 bench.py --full --workload B > "$OUT/bench_b_line.json" 2> "$OUT/bench_b.err"
timeout 900 python3 bench.py --full --workload C_avenue --no-stress > "$OUT/bench_c_avenue_line.json" 2> "$OUT/bench_c_avenue.err"
ls -la "$OUT"
timeout 900 python3 tests/replay_vs_cpu.py --seconds 20 --style boulevard --mount 16,90 --cam-hz 15 --points 440 --out "$OUT/replay_vs_cpu_c_boulevard.json" > "$OUT/replay_vs_cpu.log" 2>&1
