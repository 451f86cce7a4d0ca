#!/usr/bin/env python3
"""Compare the device assembly of bt_kernels.hip before and after a change, kernel by kernel.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S bt_kernels.hip -o before.s      (on the parent commit)
    hipcc <the Makefile's FLAGS> --cuda-device-only -S bt_kernels.hip -o after.s       (on the change)
    tools/compare_kernel_asm.py before.s after.s [--json out.json]

For every kernel of `before.s` whose name contains one of --match (default: bt_render_kernel, bt_block_mask_kernel) the
instruction stream (label to the end of its code, comments stripped, the function number in local labels dropped) must be identical
in `after.s` once the literal offsets of the hidden kernel arguments are masked: BtLaunch is passed by value, so growing it
moves everything behind it in the kernarg segment.  Such an offset is a literal of an s_load_* / s_add_u32 instruction at or
behind the struct's size (read from each file's metadata); it is rewritten as HIDDEN+<distance>, which still has to agree.
Also printed: the resource usage (VGPRs, SGPRs, spills, scratch, occupancy) of every matched kernel of both files; kernels
that exist only in `after.s` are listed as new.  Exit status 1 if any instruction stream or resource figure differs."""
import argparse
import json
import re
import sys


def parse(path, match):
    text = open(path).read()
    lines = text.split("\n")
    kernels = {}
    # metadata: name -> (by-value size of the first argument, spill counts)
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, flags=re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        first = re.search(r"\.args:\s*\n\s*- \.offset:\s+0\s*\n\s*\.size:\s+(\d+)", blk)
        meta[name] = {"struct": int(first.group(1)) if first else 0,
                      "sgpr_spills": int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                      "vgpr_spills": int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                      "kernarg_size": int(re.search(r"\.kernarg_segment_size:\s+(\d+)", blk).group(1))}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):\s", lines[i] + " ")
        if m and any(k in m.group(1) for k in match) and m.group(1) in meta:
            name, body, body_done = m.group(1), [], False
            i += 1
            while not lines[i].startswith(".Lfunc_end"):
                if not lines[i].startswith("\t.section") and not body_done:
                    body.append(lines[i])
                else:
                    body_done = True          # (a comdat kernel's descriptor sits between its code and .Lfunc_end)
                i += 1
            tail = "\n".join(lines[i:i + 160])
            res = {k: int(re.search(r"; " + k + r":\s+(\d+)", tail).group(1))
                   for k in ("TotalNumSgprs", "NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")}
            res.update(sgpr_spills=meta[name]["sgpr_spills"], vgpr_spills=meta[name]["vgpr_spills"])
            kernels[name] = {"body": body, "res": res, "struct": meta[name]["struct"], "kernarg_size": meta[name]["kernarg_size"]}
        i += 1
    return kernels


def normalise(body, struct):
    out, masked = [], 0
    for ln in body:
        ln = ln.split(";")[0].rstrip()
        if not ln.strip():
            continue
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        if re.match(r"\s+(s_load_\w+|s_add_u32)\s", ln):
            def fix(m):
                nonlocal masked
                v = int(m.group(0), 16)
                if struct <= v < struct + 0x200:
                    masked += 1
                    return "HIDDEN+0x%x" % (v - struct)
                return m.group(0)
            ln = re.sub(r"\b0x[0-9a-f]+\b", fix, ln)
        out.append(ln)
    return out, masked


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--match", nargs="*", default=["bt_render_kernel", "bt_block_mask_kernel"])
    ap.add_argument("--json")
    a = ap.parse_args()
    before, after = parse(a.before, a.match), parse(a.after, a.match)
    rows, bad = [], 0
    for name, kb in before.items():
        ka = after.get(name)
        if ka is None:
            rows.append({"kernel": name, "verdict": "missing after the change"})
            bad += 1
            continue
        nb, mb = normalise(kb["body"], kb["struct"])
        na, ma = normalise(ka["body"], ka["struct"])
        same_isa = nb == na
        same_res = kb["res"] == ka["res"]
        first = None
        if not same_isa:
            for j, (x, y) in enumerate(zip(nb, na)):
                if x != y:
                    first = {"line": j, "before": x.strip(), "after": y.strip()}
                    break
            if first is None:
                first = {"line": min(len(nb), len(na)), "before": "%d instructions" % len(nb), "after": "%d instructions" % len(na)}
        bad += (not same_isa) or (not same_res)
        rows.append({"kernel": name, "instructions": len(nb), "hidden_arg_literals_masked": [mb, ma],
                     "struct_bytes": [kb["struct"], ka["struct"]], "kernarg_size": [kb["kernarg_size"], ka["kernarg_size"]],
                     "identical_instruction_stream": same_isa, "identical_resources": same_res, "resources": ka["res"],
                     **({"resources_before": kb["res"]} if not same_res else {}), **({"first_difference": first} if first else {})})
    new = [{"kernel": n, "resources": k["res"]} for n, k in after.items() if n not in before]
    for r in rows:
        print("%-70s %s" % (r["kernel"], "identical (%d instructions, %d offsets masked)" % (r["instructions"], r["hidden_arg_literals_masked"][1])
                            if r.get("identical_instruction_stream") and r.get("identical_resources") else "DIFFERS: " + json.dumps(r)))
    for r in new:
        print("%-70s new: %s" % (r["kernel"], json.dumps(r["resources"])))
    print("%d kernels compared, %d differ, %d new" % (len(rows), bad, len(new)))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"compared": rows, "new": new, "differ": bad}, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
