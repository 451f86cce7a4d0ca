"""kernel_ms of Depth / Full renders at 1920x1080x64; usage: depth_time.py <tree root>"""
import json, os, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np, torch
import bendy_tracer_amd as b
from sphere_scenes import sphere_scene
def full_doc():
    doc = json.loads(sphere_scene(4242, n_spheres=1, focus=False))
    for o in doc["objects"]["collection"].values():
        t = o["transform"]
        for name in ("transform_world", "transform_local"):
            if o["tag"] == "camera":
                t[name][:9] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]; t[name][9:12] = [0.0, 0.0, 0.0]
            else:
                t[name][9:12] = [0.0, 0.0, -30.0]
        if o["tag"] != "camera":
            o["inner"]["Sphere"]["radius"] = 29.0
    return json.dumps(doc)
w, h, spp = 1920, 1080, 64
out = {"tree": sys.argv[1]}
for name, sc in (("scene.json", b.Scene.load(os.path.join(root, "scenes", "scene.json.gz"))), ("no_empty_block", b.Scene.from_json(full_doc()))):
    cam = sc.find_by_tag("camera"); sc.set_camera_aspect(cam, w / h)
    for output in (3, 0):
        tr = b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4, output=b.Output(output))); rc = b.RenderConfig.with_samples(spp)
        buf = b.Buffer.new(w, h); ms = []
        for i in range(16):
            tr.render(sc, cam, rc, buf, seed=0x5EED, sample_base=i * spp); torch.cuda.synchronize()
            ms.append(sc.last_stats().kernel_ms)
        out[f"{name}:output{output}"] = {"kernel_ms_median": round(float(np.median(ms[2:])), 4), "min": round(min(ms[2:]), 4), "max": round(max(ms[2:]), 4)}
print(json.dumps(out))
