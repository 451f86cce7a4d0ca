#!/bin/bash
# The measurements of this directory, one visit to the GPU box, parent and new alternating.
#   usage, from the root of a built checkout of this commit:
#     profiles/r14/run.sh <built checkout of the parent commit> [<checkout of this commit built with the fill workgroups first>] [out dir]
# A "checkout" here needs bench.py, bendy_tracer_amd/ (library, CLI, csrc), tools/, scenes/, tests/sphere_scenes.py, profiles/pmc_live.json.
# The fill-first tree was this commit with the prologue's three ranges swapped (fill workgroups w < n_fill, traced ones behind
# them), built with `make variant NAME=fillfirst KFLAGS=-DBT_FILL_FIRST`; the flag left the source once it had been measured.
# Every step has a time limit of its own; the first step that fails ends the script.
PARENT=${1:?path of the parent checkout}; VARIANT=$2; O=${3:-build_r14}
export TMPDIR=/tmp
mkdir -p $O; O=$(cd $O && pwd); H=$(cd "$(dirname "$0")" && pwd)
run() { local t=$1 f=$2; shift 2; timeout -k 10 $t "$@" >> $f 2>> $O/stderr.txt; local rc=$?; tail -n 1 $f | cut -c1-260; if [ $rc -ne 0 ]; then echo "FAILED rc=$rc: $*" | tee -a $O/failed.txt; exit $rc; fi; }
tree() { case $1 in parent) echo $PARENT;; fillfirst) echo $VARIANT;; *) echo .;; esac; }
TREES="parent new"; [ -n "$VARIANT" ] && TREES="parent new fillfirst"
# 1. the premise: a 1920x1080x64 frame in which every block is empty
for r in 1 2; do for v in parent new; do run 150 $O/premise_$v.txt python $H/time_empty_frame.py $(tree $v); done; done
# 2. the headline, five alternating runs, and C5, three
for r in 1 2 3 4 5; do for v in $TREES; do run 150 $O/c3_$v.txt python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3; done; done
for r in 1 2 3; do for v in $TREES; do run 200 $O/c5_$v.txt python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --workload C5; done; done
# 4. identity of the frames
for v in parent new; do
  run 150 /dev/null python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs $O/dump_c3_$v
  run 200 /dev/null python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --workload C5 --dump-outputs $O/dump_c5_$v
done
run 60 $O/dump_compare.txt python $H/dump_compare.py $O
rm -rf $O/dump_c3_* $O/dump_c5_*
# the Depth build (its loop has more spill reloads than the parent's): scene.json and a frame without an empty block
for r in 1 2 3; do for v in parent new; do run 200 $O/depth_$v.txt python $H/time_depth.py $(tree $v); done; done
# 3. where it went: kernel traces (runs of their own), then bench.py --full (its counter passes are runs of their own too)
for v in parent new; do
  d=$(tree $v)
  run 200 $O/trace_$v.log rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$v -o kt -- $d/bendy_tracer_amd/bendy-tracer-hip --output full --width 1920 --height 1080 --subsample 1 --samples 1472 --samples-per-call 64 --scene $d/scenes/scene.json.gz --no-screenshot --quiet
  find $O/trace_$v -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_$v.csv \; ; rm -rf $O/trace_$v
done
run 200 $O/trace_new_c5.log rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_c5 -o kt -- ./bendy_tracer_amd/bendy-tracer-hip --output full --width 3840 --height 2160 --subsample 1 --samples 512 --samples-per-call 256 --scene scenes/scene.json.gz --no-screenshot --quiet
find $O/trace_c5 -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_new_c5.csv \; ; rm -rf $O/trace_c5
for v in parent new; do run 560 $O/full_$v.txt python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --full --no-cpu-baseline; done
