#!/bin/bash
# The measurements of this directory that compare the parent commit with this one, parent and new alternating.
#   usage, from the root of a built checkout of this commit:
#     profiles/r15/run.sh <built checkout of the parent commit> [out dir] [stages, default "census ab dump occ trace full"]
# A "checkout" here needs bench.py, bendy_tracer_amd/ (library, CLI, csrc), tools/, scenes/, profiles/pmc_live.json.
# tools/residency_census must have been built (the command is at the top of tools/residency_census.hip).
# Every step has a time limit of its own; the first step that fails ends the script.
# (The A/B runs of the forms that were tried on the way -- c3_probe_*.txt here -- were variant libraries of this commit's
# source with flags that left the source once they had been measured; README.md lists what each one was.)
PARENT=${1:?path of the parent checkout}; O=${2:-build_r15}; STAGES=${3:-census ab dump occ trace full}
export TMPDIR=/tmp
mkdir -p $O; O=$(cd $O && pwd); H=$(cd "$(dirname "$0")" && pwd)
run() { local t=$1 f=$2; shift 2; timeout -k 10 $t "$@" >> $f 2>> $O/stderr.txt; local rc=$?; tail -n 1 $f | cut -c1-200; if [ $rc -ne 0 ]; then echo "FAILED rc=$rc: $*" | tee -a $O/failed.txt; exit $rc; fi; }
tree() { case $1 in parent) echo $PARENT;; *) echo .;; esac; }
has() { case " $STAGES " in *" $1 "*) return 0;; *) return 1;; esac; }
CLI_ARGS="--output full --width 1920 --height 1080 --subsample 1 --samples 256 --samples-per-call 64 --no-screenshot --quiet"
# A. residency: the two census kernels, then (occ) the render kernel's own wave-level occupancy, counters only
if has census; then run 60 $O/census_tool.txt tools/residency_census 4096 16; cat $O/census_tool.txt; fi
# the headline, five alternating runs, and C5, three
if has ab; then
  for r in 1 2 3 4 5; do for v in parent new; do run 150 $O/c3_$v.txt python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3; done; done
  for r in 1 2 3; do for v in parent new; do run 200 $O/c5_$v.txt python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --workload C5; done; done
fi
# identity of the frames
if has dump; then
  for v in parent new; do
    run 150 /dev/null python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs $O/dump_c3_$v
    run 200 /dev/null python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --workload C5 --dump-outputs $O/dump_c5_$v
  done
  run 60 $O/dump_compare.txt python $H/../r14/dump_compare.py $O
  cat $O/dump_compare.txt
  rm -rf $O/dump_c3_* $O/dump_c5_*
  if grep -q DIFFERENT $O/dump_compare.txt; then echo "FAILED: frames differ" | tee -a $O/failed.txt; exit 1; fi
fi
if has occ; then
  for v in parent new; do d=$(tree $v)
    run 200 $O/occ_$v.log rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/occ_$v -o pmc -- $d/bendy_tracer_amd/bendy-tracer-hip $CLI_ARGS --scene $d/scenes/scene.json.gz
    python $H/pmc_occupancy.py $v $O/occ_$v | tee -a $O/census_render_kernel.txt
    rm -rf $O/occ_$v
  done
fi
# where it went: kernel traces (runs of their own), then bench.py --full (its counter passes are runs of their own too)
if has trace; then
  for v in parent new; do d=$(tree $v)
    run 200 $O/trace_$v.log rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$v -o kt -- $d/bendy_tracer_amd/bendy-tracer-hip --output full --width 1920 --height 1080 --subsample 1 --samples 1472 --samples-per-call 64 --scene $d/scenes/scene.json.gz --no-screenshot --quiet
    find $O/trace_$v -name "*kernel_stats.csv" -exec cp {} $O/kernel_stats_$v.csv \; ; rm -rf $O/trace_$v
  done
fi
if has full; then
  for v in new parent; do run 560 $O/full_$v.txt python $(tree $v)/bench.py --gpus 1 --steps 20 --warmup 3 --full --no-cpu-baseline; done
fi
