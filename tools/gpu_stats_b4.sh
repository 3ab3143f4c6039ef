repo=$(cd "$(dirname "$0")/.." && pwd); cd /tmp && export TMPDIR=/tmp; cd "$repo" || exit 1
out=${LAGO_OUT_DIR:-out}
rm -rf $out/stats_b4
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats_b4 -- python3 bench.py --full --batch 4 --steps 4 --warmup 2 --no-cpu-baseline --no-micro --no-atlas > $out/stats_b4.out 2> $out/stats_b4.err
python3 tools/rocprof_summary.py $out/stats_b4/*/*_kernel_stats.csv | head -12
rm -f $out/stats_b4/*/*_kernel_trace.csv
