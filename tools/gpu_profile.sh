#!/bin/bash
# Official measurement set of a round: default bench with every side figure (--full: cpu_baseline, rooflines, ...),
# rocprofv3 kernel stats and the PMC passes of the same command (eager launches so that every kernel is a dispatch),
# traffic summary.  Run from the repository root on an MI355X:
#   bash tools/gpu_profile.sh <tag> [output folder, default profile_out]
TAG=${1:-r01}
O=${2:-profile_out}
export TMPDIR=/tmp
mkdir -p "$O"
A=$(cd "$O" && pwd)
CMD="python $(pwd)/bench.py --steps 50 --warmup 10 --no-graph --no-cpu-baseline --no-also --full"
echo "== bench default"; timeout 300 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err; echo "rc=$?"; cat $O/bench_$TAG.json
echo "== rocprof stats"; (cd "$TMPDIR" && timeout 150 rocprofv3 --kernel-trace --stats --output-format csv -d $A/prof_${TAG}_stats -o bench -- $CMD > $A/rocprof_stats.log 2>&1); echo "rc=$?"
echo "== rocprof pmc SQ"; (cd "$TMPDIR" && timeout 150 rocprofv3 --kernel-trace --output-format csv --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES -d $A/prof_${TAG}_sq -o bench -- $CMD > $A/rocprof_sq.log 2>&1); echo "rc=$?"
echo "== rocprof pmc FETCH"; (cd "$TMPDIR" && timeout 150 rocprofv3 --kernel-trace --output-format csv --pmc FETCH_SIZE -d $A/prof_${TAG}_fetch -o bench -- $CMD > $A/rocprof_fetch.log 2>&1); echo "rc=$?"
echo "== rocprof pmc WRITE"; (cd "$TMPDIR" && timeout 150 rocprofv3 --kernel-trace --output-format csv --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum -d $A/prof_${TAG}_write -o bench -- $CMD > $A/rocprof_write.log 2>&1); echo "rc=$?"
S=$O/summary_$TAG.txt
{
echo "# rocprofv3 summaries of: $CMD   (tag $TAG)"
echo "# tree: $(cat BUILD_STAMP 2>/dev/null || echo unknown: run through tools/grun.sh)"
echo "## kernel stats (--kernel-trace --stats)"; f=$(find $O/prof_${TAG}_stats -name "*kernel_stats.csv" | head -1); cat "$f"
echo "## SQ counters, average per dispatch (quad-cycles)"; f=$(find $O/prof_${TAG}_sq -name "*counter_collection.csv" | head -1); python tools/rocprof_summary.py "$f" --pmc | sed -n '/^$/,$p'
echo "## FETCH_SIZE [KiB, x2 for wide reads on gfx950]"; f1=$(find $O/prof_${TAG}_fetch -name "*counter_collection.csv" | head -1); python tools/rocprof_summary.py "$f1" --pmc | sed -n '/^$/,$p'
echo "## WRITE_SIZE [KiB], TCC hit/miss"; f2=$(find $O/prof_${TAG}_write -name "*counter_collection.csv" | head -1); python tools/rocprof_summary.py "$f2" --pmc | sed -n '/^$/,$p'
} > $S 2>&1
python tools/pmc_traffic.py "$f1" "$f2" uniform-f16-c64-n100000 | tee $O/traffic_fragment_$TAG.json   # ONE key's entry; the keyed file is profiles/traffic.json
cp profiles/traffic.json $O/traffic.json
tail -5 $O/bench_$TAG.err
