# step timeline of the timed leg of config 3 (see profiles/*_step_timeline_config3.md).  Usage: bash tools/experiments/run_timeline.sh <output directory>
OUT=$(realpath -m "${1:?usage: run_timeline.sh <output directory>}"); mkdir -p "$OUT"
R=$PWD; cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_tl
timeout 600 rocprofv3 --kernel-trace -d $OUT/prof_tl -o kt -- python $R/bench.py --steps 50 --warmup 20 --no-cpu-baseline --no-readback-leg --full > $OUT/tl_bench.log 2>&1
db=$(find $OUT/prof_tl -name "*.db" | head -1)
python $R/tools/step_timeline.py $db --steps 40 --skip-last 60 > $OUT/step_timeline.md
rm -rf $OUT/prof_tl
cat $OUT/step_timeline.md
