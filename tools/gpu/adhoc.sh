set -o pipefail
O=${OUT_DIR:-out}
mkdir -p $O
export TMPDIR=/tmp
rm -rf $O/rk8
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --config 2 --steps 1 --warmup 0 > $O/c2_phases.json 2> $O/c2_phases.err || { tail -20 $O/c2_phases.err; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace -d $O/rk8 -o rk --output-format csv -- python3 tools/rank_frames.py --config 2 --world 8 --rank 0 --frames 2 > $O/rk8.log 2>&1 || { tail -20 $O/rk8.log; exit 1; }
grep frame $O/rk8.log
python3 tools/iter_gaps.py "$O/rk8/**/*kernel_trace.csv" > $O/rk8_gaps.json && cat $O/rk8_gaps.json
