"""kernel_ms of a 1920x1080x64 frame in which every block is empty; usage: premise.py <tree root> [renders]"""
import json, os, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np, torch
import bendy_tracer_amd as b
from sphere_scenes import sphere_scene
doc = json.loads(sphere_scene(4242, n_spheres=1, focus=False))
for o in doc["objects"]["collection"].values():
    t = o["transform"]
    for name in ("transform_world", "transform_local"):
        if o["tag"] == "camera":
            t[name][:9] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]; t[name][9:12] = [0.0, 0.0, 0.0]
        else:
            t[name][9:12] = [0.0, 0.0, 6.0]
    if o["tag"] != "camera":
        o["inner"]["Sphere"]["radius"] = 0.5
w, h, spp = 1920, 1080, 64
sc = b.Scene.from_json(json.dumps(doc)); cam = sc.find_by_tag("camera"); sc.set_camera_aspect(cam, w / h)
tr = b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4)); rc = b.RenderConfig.with_samples(spp)
buf = b.Buffer.new(w, h); ms = []
for i in range(int(sys.argv[2]) if len(sys.argv) > 2 else 12):
    tr.render(sc, cam, rc, buf, seed=0x5EED, sample_base=i * spp); torch.cuda.synchronize()
    st = sc.last_stats(); ms.append(round(st.kernel_ms, 4))
m = tr.primary_masks(sc, cam, rc, w, h, st.slices)
print(json.dumps({"tree": sys.argv[1], "frame": [w, h, spp], "slices": st.slices, "packed": st.packed, "blocks": int(m.size), "all_masks_zero": bool((m == 0).all()),
                  "segments": st.segments, "kernel_ms": ms, "kernel_ms_median_after_first": float(np.median(ms[1:]))}))
