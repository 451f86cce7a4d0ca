"""Mean wave-level occupancy of the render kernel from a counters-only rocprofv3 pass: pmc_occupancy.py <label> <output dir>.
SQ_WAVE_CYCLES / SQ_BUSY_CU_CYCLES is the mean number of waves resident per SIMD of a busy CU; seven workgroups of four
waves per CU are 7 per SIMD, eight are 8 (less what the ends of a launch take off)."""
import collections
import csv
import glob
import sys

label, out = sys.argv[1], sys.argv[2]
agg = collections.defaultdict(list)
for f in glob.glob(out + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "bt_render" in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
m = {k: sum(v) / len(v) for k, v in agg.items()}
print(label, " ".join("%s %.5g" % kv for kv in sorted(m.items())), "launches", len(agg.get("SQ_WAVES", [])))
print(label, "SQ_WAVE_CYCLES / SQ_BUSY_CU_CYCLES = %.3f" % (m["SQ_WAVE_CYCLES"] / m["SQ_BUSY_CU_CYCLES"]))
