#!/bin/bash
# rocprofv3 kernel trace (+stats) of the bench command, then two PMC passes.
cd "$(dirname "$0")/.."
RESULTS=$(realpath -m "${RESULTS:-results}"); mkdir -p "$RESULTS"
export TMPDIR=/tmp
ROOT=$(pwd)
CMD="python $ROOT/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline"
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $RESULTS/prof_trace -o bench -- $CMD > $RESULTS/prof_trace.log 2>&1
tail -2 $RESULTS/prof_trace.log
timeout 600 rocprofv3 --pmc FETCH_SIZE -d $RESULTS/prof_fetch -o bench -- $CMD > $RESULTS/prof_fetch.log 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE -d $RESULTS/prof_write -o bench -- $CMD > $RESULTS/prof_write.log 2>&1
cd $ROOT
find $RESULTS/prof_trace $RESULTS/prof_fetch $RESULTS/prof_write -type f | head -30
# keep only the small summaries + a compressed kernel trace (scratch dir is capped at 64 MiB)
for d in prof_trace prof_fetch prof_write; do
  find $RESULTS/$d -name "*.db" -delete 2>/dev/null
  find $RESULTS/$d -name "*_kernel_trace.csv" -size +20M -exec sh -c 'head -200000 "$1" > "$1.head"; rm "$1"' _ {} \;
done
python tools/prof_summary.py $RESULTS > $RESULTS/prof_summary.txt 2>&1
cat $RESULTS/prof_summary.txt | head -60
