#!/usr/bin/env python3
"""What adaptive sampling (bt_render_adaptive_device) costs and saves, on the GPU.

overhead     One adaptive pass with every tile active (threshold 0, no cap in reach) against the plain Full render of the same
             samples, HIP events around back-to-back asynchronous calls, alternating between the variants (ROUNDS rounds of
             CALLS calls after a warm-up).  `plain` lets the library shape the launch, `plain_unpacked` pins bt_tuning.packed = 0,
             which is what an adaptive pass always is.
convergence  scene / cornell2 / volume at 768 x 512 (--size W H): passes of 16 samples (--pass N) at bt_adaptive_params_default until BT_DONE against a
             uniform render at the cap; total pixel-samples, wall time (host clock around the whole loop, polls included) and
             relMSE = mean((x - y)^2 / (y^2 + 0.01)) of both means against a truth of TRUTH samples from another seed.
             --maps DIR writes each scene's per-tile counts as a grey PNG (one pixel per tile, 255 = the cap).
             --thresholds repeats the adaptive run for other thresholds (how the default was chosen).

    python tools/time_adaptive.py [--json profiles/<round>/adaptive_timing.json] [--maps DIR] [--thresholds 0.01 0.02 0.05]
                                  [--size 1920 1080] [--pass 64] [--skip overhead]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OVERHEAD = [
    # name, scene, width, height, samples, subsample, calls per round x this (short calls)
    ("C3 scene 1920x1080x64", "scene", 1920, 1080, 64, 0, 1),
    ("cornell2 1920x1080x16", "cornell2", 1920, 1080, 16, 0, 1),
    ("volume 1920x1080x16", "volume", 1920, 1080, 16, 0, 1),
    ("interactive scene 768x512, 1 x Subpixel(2)", "scene", 768, 512, 1, 2, 50),
]
CONVERGENCE = ["scene", "cornell2", "volume"]
TRUTH = 8192


def load(b, scene, w, h):
    sc = b.Scene.load(os.path.join(ROOT, "scenes", scene + ".json.gz"))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    return sc, cam


def overhead(b, torch, rounds, calls):
    from bendy_tracer_amd import api
    rows = []
    for name, scene, w, h, spp, n, mult in OVERHEAD:
        sc, cam = load(b, scene, w, h)
        sc0, cam0 = load(b, scene, w, h)
        sc0.set_tuning(packed=0)
        tr = b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4))
        rc = b.RenderConfig(samples=spp, subsample=b.Subsample(n))
        buf, buf0, abuf = b.Buffer.new(w, h), b.Buffer.new(w, h), b.Buffer.new(w, h)
        ad = b.Adaptive(w, h, threshold=0.0, min_samples=1 << 30, max_samples=1 << 30)
        cc, cr = api._c_configs(tr.config, rc, 0)
        cp = ad.params._c()
        stream = torch.cuda.current_stream().cuda_stream

        def plain():
            tr.render(sc, cam, rc, buf, sample_base=0)

        def plain_unpacked():
            tr.render(sc0, cam0, rc, buf0, sample_base=0)

        def adaptive():                                          # asynchronous: no poll inside the timed region
            api._check(api.lib.bt_render_adaptive_device(sc0._h, cam0, C.byref(cc), C.byref(cr), ad._h, C.byref(cp),
                                                         abuf.data.data_ptr(), w, h, tr.DEFAULT_SEED, stream))

        variants = {"plain": plain, "plain_unpacked": plain_unpacked, "adaptive": adaptive}
        info = {}
        for key, fn in variants.items():
            fn()
            fn()
            torch.cuda.synchronize()
            st = (sc if key == "plain" else sc0).last_stats()
            info[key] = {"launches": st.launches, "packed": st.packed, "slices": st.slices}
        times = {k: [] for k in variants}
        for _ in range(rounds):
            for key, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls * mult):
                    fn()
                e1.record()
                e1.synchronize()
                times[key].append(e0.elapsed_time(e1) / (calls * mult))
        assert ad.poll().active_tiles == ad.poll().tiles
        row = {"workload": name, "calls_per_variant": rounds * calls * mult}
        for key in variants:
            t = times[key]
            row[key] = {"ms_mean": sum(t) / len(t), "ms_min": min(t), "ms_max": max(t), **info[key]}
        row["adaptive_over_plain"] = row["adaptive"]["ms_mean"] / row["plain"]["ms_mean"]
        row["adaptive_over_plain_unpacked"] = row["adaptive"]["ms_mean"] / row["plain_unpacked"]["ms_mean"]
        rows.append(row)
        print("%-44s plain %8.3f ms (packed %d) | unpacked %8.3f ms | adaptive pass %8.3f ms | adaptive/plain %.3f  adaptive/unpacked %.3f"
              % (name, row["plain"]["ms_mean"], row["plain"]["packed"], row["plain_unpacked"]["ms_mean"], row["adaptive"]["ms_mean"],
                 row["adaptive_over_plain"], row["adaptive_over_plain_unpacked"]), flush=True)
    return rows


def rel_mse(x, y):
    import numpy as np
    x, y = x.astype(np.float64), y.astype(np.float64)
    return float(np.mean((x - y) ** 2 / (y ** 2 + 0.01)))


def convergence(b, torch, maps, thresholds, W, H, PASS):
    import numpy as np
    d = b.AdaptiveParams()
    cap = d.max_samples
    tr = b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4))
    rows = []
    for scene in CONVERGENCE:
        sc, cam = load(b, scene, W, H)
        truth = b.Buffer.new(W, H)
        tr.render(sc, cam, b.RenderConfig(samples=TRUTH), truth, seed=0xACE)
        y = truth.mean()
        # uniform render at the cap, in the same passes (twice: the first call also pays for scratch and code objects)
        for _ in range(2):
            uni = b.Buffer.new(W, H)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(cap // PASS):
                tr.render(sc, cam, b.RenderConfig(samples=PASS), uni)
            torch.cuda.synchronize()
            t_uni = time.perf_counter() - t0
        row = {"scene": scene, "width": W, "height": H, "pass": PASS, "cap": cap, "min_samples": d.min_samples,
               "uniform": {"pixel_samples": W * H * cap, "seconds": t_uni, "relMSE": rel_mse(uni.mean(), y)}, "adaptive": []}
        for thr in thresholds:
            for _ in range(2):
                buf, ad = b.Buffer.new(W, H), b.Adaptive(W, H, threshold=thr)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                while tr.render_adaptive(sc, cam, b.RenderConfig(samples=PASS), buf, ad) != b.Status.Done:
                    pass
                t_ad = time.perf_counter() - t0
            st, counts = ad.poll(), ad.counts()
            x = ad.resolve(buf).numpy()[..., :3]
            row["adaptive"].append({"threshold": thr, "pixel_samples": st.pixel_samples, "seconds": t_ad, "passes": st.passes,
                                    "min_count": st.min_count, "max_count": st.max_count, "mean_count": float(counts.mean()),
                                    "tiles_at_cap": int((counts >= cap).sum()), "tiles": st.tiles, "relMSE": rel_mse(x, y)})
            print("%-9s threshold %.3f: %5.1f%% of the uniform render's samples, %.3f s against %.3f s, relMSE %.3e against %.3e, "
                  "counts %d .. %d (mean %.0f), %d of %d tiles at the cap"
                  % (scene, thr, 100.0 * st.pixel_samples / (W * H * cap), t_ad, t_uni, row["adaptive"][-1]["relMSE"],
                     row["uniform"]["relMSE"], st.min_count, st.max_count, counts.mean(), (counts >= cap).sum(), st.tiles), flush=True)
            if maps and abs(thr - d.threshold) < 1e-9:
                grey = np.zeros(counts.shape + (4,), dtype=np.uint8)
                grey[..., :3] = (counts.astype(np.int64) * 255 // cap).astype(np.uint8)[..., None]
                grey[..., 3] = 255
                os.makedirs(maps, exist_ok=True)
                b.write_png(os.path.join(maps, "adaptive_counts_%s.png" % scene), grey)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json")
    ap.add_argument("--maps")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--thresholds", type=float, nargs="*")
    ap.add_argument("--size", type=int, nargs=2, default=[768, 512])
    ap.add_argument("--pass", dest="pass_", type=int, default=16)
    ap.add_argument("--skip", nargs="*", default=[], choices=["overhead", "convergence"])
    a = ap.parse_args()
    import torch
    import bendy_tracer_amd as b
    if not torch.cuda.is_available():
        sys.exit("time_adaptive.py needs a GPU: there is nothing to time without one")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_round": a.calls}
    if "overhead" not in a.skip:
        out["overhead"] = overhead(b, torch, a.rounds, a.calls)
    if "convergence" not in a.skip:
        out["convergence"] = convergence(b, torch, a.maps, a.thresholds or [b.AdaptiveParams().threshold], a.size[0], a.size[1], a.pass_)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
