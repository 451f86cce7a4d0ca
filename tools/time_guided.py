#!/usr/bin/env python3
"""What the guided render (bt_render_guided_device) costs and saves, on the GPU.

Per workload three variants are timed with HIP events around back-to-back calls, alternating between the variants
(ROUNDS rounds of CALLS calls each, after a warm-up of every variant):
  full      one plain Full render                         (Tracer.render, Output.Full)
  guided    one guided render with all three guides       (Tracer.render_guided)
  separate  the four plain renders the guided one replaces (Output.Full, Albedo, Normal, Depth)
Every call starts at sample_base 0, so that each call of a variant does the same work.  A row records the mean time per call
of each variant, min and max over the rounds, the ratios guided / full and guided / separate, and last_stats().launches and
.packed of the full and the guided call.  `scratch_cap` rows repeat a workload with bt_tuning.scratch_cap_bytes raised.

    python tools/time_guided.py [--json profiles/<round>/guided_timing.json] [--rounds 5] [--calls 4] [--only NAME ...]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [
    # name, scene, width, height, samples, subsample, scratch cap (0 = the default 2 GiB), calls per round x this (short calls)
    ("C3 scene 1920x1080x64", "scene", 1920, 1080, 64, 0, 0, 1),
    ("C3 scene 1920x1080x64, cap 8 GiB", "scene", 1920, 1080, 64, 0, 8 << 30, 1),
    ("cornell 1920x1080x64", "cornell", 1920, 1080, 64, 0, 0, 1),
    ("volume 1920x1080x64", "volume", 1920, 1080, 64, 0, 0, 1),
    ("C2 cornell2 512x512x16", "cornell2", 512, 512, 16, 0, 0, 10),
    ("interactive scene 768x512, 1 x Subpixel(2)", "scene", 768, 512, 1, 2, 0, 50),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    import torch
    import bendy_tracer_amd as b
    if not torch.cuda.is_available():
        sys.exit("time_guided.py needs a GPU: there is nothing to time without one")
    rows = []
    for name, scene, w, h, spp, n, cap, mult in WORKLOADS:
        if a.only and not any(o in name for o in a.only):
            continue
        sc = b.Scene.load(os.path.join(ROOT, "scenes", scene + ".json.gz"))
        cam = sc.find_by_tag("camera")
        sc.set_camera_aspect(cam, w / h)
        if cap:
            sc.set_tuning(scratch_cap_bytes=cap)
        rc = b.RenderConfig(samples=spp, subsample=b.Subsample(n))
        bufs = [b.Buffer.new(w, h) for _ in range(4)]
        tracers = [b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4, output=o))
                   for o in (b.Output.Full, b.Output.Albedo, b.Output.Normal, b.Output.Depth)]
        stats = {}

        def full():
            tracers[0].render(sc, cam, rc, bufs[0], sample_base=0)

        def guided():
            tracers[0].render_guided(sc, cam, rc, *bufs, sample_base=0)

        def separate():
            for t, buf in zip(tracers, bufs):
                t.render(sc, cam, rc, buf, sample_base=0)

        variants = {"full": full, "guided": guided, "separate": separate}
        for key, fn in variants.items():                       # warm-up: code objects, scratch, block masks
            fn()
            fn()
            torch.cuda.synchronize()
            st = sc.last_stats()
            stats[key] = {"launches": st.launches, "packed": st.packed, "slices": st.slices,
                          "parked_bytes": st.parked_bytes, "scratch_bytes": st.scratch_bytes}
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for key, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls * mult):
                    fn()
                e1.record()
                e1.synchronize()
                times[key].append(e0.elapsed_time(e1) / (a.calls * mult))
        row = {"workload": name, "scene": scene, "width": w, "height": h, "samples": spp, "subsample": n,
               "scratch_cap_bytes": cap or (2 << 30), "calls_per_variant": a.rounds * a.calls * mult}
        for key in variants:
            t = times[key]
            row[key] = {"ms_mean": sum(t) / len(t), "ms_min": min(t), "ms_max": max(t), **stats[key]}
        row["guided_over_full"] = row["guided"]["ms_mean"] / row["full"]["ms_mean"]
        row["guided_over_separate"] = row["guided"]["ms_mean"] / row["separate"]["ms_mean"]
        rows.append(row)
        print("%-46s full %8.3f ms | guided %8.3f ms (%d launches, packed %d) | four separate %8.3f ms | guided/full %.2f  guided/separate %.2f"
              % (name, row["full"]["ms_mean"], row["guided"]["ms_mean"], row["guided"]["launches"], row["guided"]["packed"],
                 row["separate"]["ms_mean"], row["guided_over_full"], row["guided_over_separate"]), flush=True)
        del bufs
        sc.trim()
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_round": a.calls, "rows": rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
