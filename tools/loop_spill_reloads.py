#!/usr/bin/env python3
"""Static count of SGPR-spill traffic inside a render kernel's loop.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S bt_kernels.hip -o kernels.s
    tools/loop_spill_reloads.py KERNEL_SYMBOL kernels.s [other.s ...]

The loop is taken to be the longest backward branch of the kernel (label ... branch back to it): for bt_render_kernel
that is the `for (;;)` of the work queue, together with whatever blocks the compiler has laid out inside its span.
Printed per listing: instructions and VALU instructions in the span, v_readlane (reloads of spilled SGPRs, plus the few
explicit readlanes of the loop) and v_writelane in it, v_readlane in the whole kernel, and the metadata's resource figures."""
import re
import sys


def kernel_text(lines, name):
    i = next(k for k, l in enumerate(lines) if l.startswith(name + ":"))
    j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
    return lines[i:j + 1]


def metadata(lines, name):
    i = next((k for k, l in enumerate(lines) if re.match(r"\s*\.name:\s*%s\s*$" % re.escape(name), l)), None)
    if i is None:
        return {}
    out = {}
    for l in lines[max(0, i - 40):i + 40]:
        m = re.match(r"\s*\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|sgpr_count|private_segment_fixed_size):\s*(\d+)", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def analyse(path, name):
    lines = open(path).read().split("\n")
    t = kernel_text(lines, name)
    labels = {m.group(1): k for k, l in enumerate(t) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    span, first, last = 0, 0, 0
    for k, l in enumerate(t):
        m = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), k) < k and k - labels[m.group(1)] > span:
            span, first, last = k - labels[m.group(1)], labels[m.group(1)], k
    body = [l.strip() for l in t[first:last + 1] if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    count = lambda ls, p: sum(1 for l in ls if l.startswith(p))
    print("%s: loop %d instructions, VALU %d, v_readlane %d, v_writelane %d; whole kernel v_readlane %d; %s" % (
        path, len(body), count(body, "v_"), count(body, "v_readlane"), count(body, "v_writelane"),
        count([l.strip() for l in t], "v_readlane"), metadata(lines, name)))


if __name__ == "__main__":
    for p in sys.argv[2:]:
        analyse(p, sys.argv[1])
