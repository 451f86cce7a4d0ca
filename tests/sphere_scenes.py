"""Random sphere-only scenes without volumes (the build that skips empty pixel blocks) and a float32
restatement of the kernel's camera rays and sphere test, for brute-force checks of the per-block sphere masks
(test infrastructure)."""
import json
import math

import numpy as np

f32 = np.float32


def _rot(rng, spread):
    a, b, c = rng.uniform(-spread, spread, 3)
    ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    return ry @ rx @ rz


ROOT_KEYS = {"Emissive": 1, "Flat": 7, "Diffuse": 8, "Metallic": 9, "Glass": 10}


def sphere_scene(seed, n_spheres=None, focus=None, cam_post=None, focal_length=None, fstop=None, focus_dist=None,
                 root=None):
    """A camera with a random orientation and spheres placed so that many pixel blocks see nothing and many see a
    sphere's silhouette: in front, off to the sides, behind the camera, and now and then around the camera.

    The optional arguments reach the inputs the ordinary camera never has (tests/test_cull_edges.py); left at None they
    change nothing, and none of them changes the number or order of the random draws, so the spheres of a seed stay
    where they are:
    cam_post: 3x3, multiplied onto the random rotation (scale, mirror, shear); the spheres are placed along the
    rotation's own axes.  focal_length, fstop, focus_dist: replace the drawn values (focus_dist only with focus).
    root: the root material's kind, "Flat" / "Diffuse" / "Metallic" / "Glass" / "Emissive" (rows 7 - 10 are added for
    the first four, with colours from a generator of their own)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 9)) if n_spheres is None else n_spheres
    if focus is None:
        focus = bool(rng.uniform() < 0.5)
    rot = _rot(rng, 0.6)
    cam_m = rot.astype(np.float32)
    if cam_post is not None:
        cam_m = (rot @ np.asarray(cam_post, np.float64).reshape(3, 3)).astype(np.float32)
        rot = rot.astype(np.float32)
    cam_t = rng.uniform(-3, 3, 3).astype(np.float32)
    col = lambda: dict(zip("rgb", [float(v) for v in rng.uniform(0.1, 0.9, 3)]))
    data = {"0": {"inner": {"Material": {"Flat": {"albedo": {"r": 0.0, "g": 0.0, "b": 0.0}}}}},
            "1": {"inner": {"Material": {"Emissive": {"albedo": col(), "intensity": float(rng.uniform(0.2, 1.0))}}}},
            "2": {"inner": {"Material": {"Diffuse": {"albedo": col(), "roughness": 0.5}}}},
            "3": {"inner": {"Material": {"Metallic": {"albedo": col(), "roughness": 0.2}}}},
            "4": {"inner": {"Material": {"Glass": {"albedo": col(), "roughness": 0.02, "ior": 1.4}}}},
            "5": {"inner": {"Material": {"Flat": {"albedo": col()}}}},
            "6": {"inner": {"Material": {"Emissive": {"albedo": col(), "intensity": 8.0}}}}}
    objects = {}

    def add(inner, m, t, tag=None, flags=0):
        k = len(objects)
        a = [float(v) for v in np.concatenate([np.asarray(m, np.float32).T.reshape(-1), np.asarray(t, np.float32)])]
        objects[str(k)] = {"object_ref": k, "tag": tag, "flags": {"bits": flags},
                           "transform": {"transform_world": a, "transform_local": a, "transform_parent": None},
                           "inner": inner, "children": None}

    root_material = 1
    if root is not None:
        rng_root = np.random.default_rng([seed, 0x7007])
        rcol = lambda: dict(zip("rgb", [float(v) for v in rng_root.uniform(0.1, 0.9, 3)]))
        data["7"] = {"inner": {"Material": {"Flat": {"albedo": rcol()}}}}
        data["8"] = {"inner": {"Material": {"Diffuse": {"albedo": rcol(), "roughness": 0.5}}}}
        data["9"] = {"inner": {"Material": {"Metallic": {"albedo": rcol(), "roughness": 0.2}}}}
        data["10"] = {"inner": {"Material": {"Glass": {"albedo": rcol(), "roughness": 0.02, "ior": 1.4}}}}
        root_material = ROOT_KEYS[root]

    cam = {"sensor_size": 0.024, "focal_length": float(rng.uniform(0.02, 0.06)), "aspect_ratio": 1.5,
           "fstop": float(rng.uniform(0.5, 4.0)), "focus": float(rng.uniform(3, 12)) if focus else None}
    if focal_length is not None:
        cam["focal_length"] = float(focal_length)
    if fstop is not None:
        cam["fstop"] = float(fstop)
    if focus_dist is not None and focus:
        cam["focus"] = float(focus_dist)
    add({"Camera": cam}, cam_m, cam_t, tag="camera")
    axes = cam_m if cam_post is None else rot
    fwd, right, up = -axes[:, 2], axes[:, 0], axes[:, 1]
    for i in range(n):
        kind = rng.uniform()
        r = float(rng.uniform(0.2, 1.5))
        if kind < 0.55:      # in front, anywhere across (and beyond) the view
            dist = rng.uniform(2, 15)
            c = cam_t + fwd * dist + right * dist * rng.uniform(-0.7, 0.7) + up * dist * rng.uniform(-0.5, 0.5)
        elif kind < 0.8:     # behind the camera
            c = cam_t - fwd * rng.uniform(r + 0.3, 8) + right * rng.uniform(-2, 2)
        elif kind < 0.9:     # around the camera (the aperture disc inside)
            r = float(rng.uniform(0.3, 4.0))
            c = cam_t + rng.uniform(-0.2, 0.2, 3) * r
        else:                # a huge ground sphere below the view
            r = float(rng.uniform(50, 200))
            c = cam_t - up * (r + rng.uniform(0.5, 3)) + fwd * rng.uniform(0, 10)
        mat = 6 if i == 0 else int(rng.integers(2, 6))
        add({"Sphere": {"material": mat, "volume": None, "radius": r}}, np.eye(3), c, flags=1 if i == 0 else 0)
    return json.dumps({"roots": [], "root_material": root_material, "objects": {"collection": objects, "next_key": len(objects)},
                       "data": {"collection": data, "next_key": len(data)}})


def camera_of(doc, aspect):
    """The launch's camera block as bt_api.cpp fill_launch computes it (float32)."""
    cam = next(o for o in doc["objects"]["collection"].values() if o["tag"] == "camera")
    a = np.asarray(cam["transform"]["transform_world"], np.float32)
    c = cam["inner"]["Camera"]
    yfov = f32(2.0) * f32(math.atan2(f32(c["sensor_size"]), f32(2.0) * f32(c["focal_length"])))
    return {"m": a[:9].reshape(3, 3).T.copy(), "t": a[9:12].copy(), "yfov": f32(yfov), "xfov": f32(yfov * f32(aspect)),
            "focus": None if c["focus"] is None else f32(c["focus"]),
            "aperture": f32(f32(0.5) * f32(c["focal_length"]) / f32(c["fstop"]))}


def spheres_of(doc):
    rows = []
    for k in sorted(doc["objects"]["collection"], key=int):
        o = doc["objects"]["collection"][k]
        if "Sphere" in o["inner"]:
            t = np.asarray(o["transform"]["transform_world"], np.float32)[9:12]
            r = f32(o["inner"]["Sphere"]["radius"])
            rows.append((t[0], t[1], t[2], f32(r * r)))
    return np.asarray(rows, np.float32).reshape(-1, 4)


def primary_rays(cam, w, h, px, py, n, jit, disk):
    """Camera rays (bt_kernels.hip camera event) in float32 for pixels (px, py), sub-pixel cells of Subsample(n),
    jitter fractions jit (k x 2, in [0, 1)) and aperture points disk (m x 2: angle, radius fraction).

    `cam["m"]` may be any matrix, as in the kernel: the direction M d_cam is normalised BEFORE the focus distance
    multiplies it, the lens offset M (defocus * aperture) is not (under a matrix of scale s the lens is s times as
    wide, the focus plane stays where it is).  Nothing here assumes |yrot| <= pi/2: beyond it d_cam.z changes sign, the
    ray points behind the camera and focus / |d_cam.z| passes its pole, as in the kernel."""
    pw, ph = f32(2.0) * (f32(1.0) / f32(w)), f32(2.0) * (f32(1.0) / f32(h))
    sub = f32(1.0) / f32(n) if n > 1 else f32(1.0)
    umin, vmin = f32(-0.5) * pw * sub, f32(-0.5) * ph * sub
    uscale, vscale = f32(-2.0) * umin, f32(-2.0) * vmin
    nn = max(n, 1)
    cells = [(f32(i % nn) * (f32(1.0) / f32(nn)), f32(i // nn) * (f32(1.0) / f32(nn))) for i in range(nn * nn)] if n > 1 else [(f32(0), f32(0))]
    O, D = [], []
    for us, vs in cells:
        for ju, jv in jit:
            uu = (px.astype(np.float32) * pw - f32(1.0)) + (us * pw + (f32(ju) * uscale + umin))
            vv = (py.astype(np.float32) * ph - f32(1.0)) + (vs * ph + (f32(jv) * vscale + vmin))
            yrot = cam["xfov"] * f32(0.5) * -uu
            xrot = cam["yfov"] * f32(0.5) * -vv
            sy, cy, sx, cx = np.sin(yrot), np.cos(yrot), np.sin(xrot), np.cos(xrot)
            d_cam = np.stack([-(cx * sy), sx, -(cx * cy)], -1).astype(np.float32)
            m = cam["m"]
            dw = (d_cam @ m.T).astype(np.float32)
            dw = dw / np.linalg.norm(dw, axis=-1, keepdims=True).astype(np.float32)
            if cam["focus"] is None:
                O.append(np.broadcast_to(cam["t"], dw.shape))
                D.append(dw)
            else:
                for ang, rad in disk:
                    defocus = (np.array([1, 0, 0], np.float32) * f32(math.cos(ang)) + np.array([0, -1, 0], np.float32) * f32(math.sin(ang))) * f32(rad)
                    off = (m @ (defocus * cam["aperture"])).astype(np.float32)
                    f = (cam["focus"] / np.abs(d_cam[:, 2])).astype(np.float32)
                    O.append(np.broadcast_to(cam["t"] + off, dw.shape))
                    D.append(dw * f[:, None] - off)
    O, D = np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32)
    D = D / np.linalg.norm(D, axis=-1, keepdims=True).astype(np.float32)
    return O, D


def sphere_hits(O, D, rows, tmin=f32(0.01), tmax=f32(1000.0)):
    """[rays, rows] bool: intersect_spheres_plain's `ok` for each row on its own, float32 in the kernel's order."""
    out = np.zeros((O.shape[0], rows.shape[0]), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (cx, cy, cz, r2) in enumerate(rows):
            ocx, ocy, ocz = O[:, 0] - cx, O[:, 1] - cy, O[:, 2] - cz
            hb = (ocx * D[:, 0] + ocy * D[:, 1]) + ocz * D[:, 2]
            cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - r2
            disc = hb * hb - cc
            sq = np.sqrt(np.maximum(disc, f32(0)))
            t1, t2 = -hb - sq, -hb + sq
            ok = ((t1 >= tmin) & (t1 <= tmax)) | ((t2 >= tmin) & (t2 <= tmax))
            out[:, i] = (disc >= 0) & ok
    return out


def block_rects(w, h, slices, rank=0, world=1):
    """Pixel rectangles of the blocks of a launch, in launch order (bt_kernels.hip block_ref / block_extent)."""
    tiles_x, tiles_y = (w + 15) // 16, (h + 15) // 16
    grid = (tiles_x * tiles_y + world - 1) // world
    pxb = 256 // slices
    bw = 16 if pxb >= 128 else (8 if pxb >= 32 else 4)
    bh = pxb // bw
    per_row = 16 // bw
    out = []
    for b in range(grid * slices):
        slot, sub = b // slices, b % slices
        tile = slot * world + rank if world > 1 else slot
        tx, ty = tile % tiles_x, tile // tiles_x
        x0, y0 = tx * 16 + (sub % per_row) * bw, ty * 16 + (sub // per_row) * bh
        nx = max(0, min(bw, w - x0)) if ty < tiles_y else 0
        ny = max(0, min(bh, h - y0)) if ty < tiles_y else 0
        out.append((x0, y0, nx, ny))
    return out
