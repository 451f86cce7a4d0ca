"""The ray query's yardstick (test infrastructure): `try_hit` (tracer/mod.rs:389-402) with the oracle, and the
ray recipe the query tests share.

try_hit: for each ray loop `oracle.object_hit(scene, j, o, d, (tmin, clip_max))` over the non-camera, non-empty objects in
ascending index, shrink clip_max to each hit's t and keep the last hit.  A batch's reference is computed once per process and
handed out read-only."""
import json

import numpy as np

FACES = {"Front": 0, "Back": 1, "Volume": 2, "VolumeFront": 3, "VolumeBack": 4}
NO_REF = 0xFFFFFFFFFFFFFFFF
REF_DTYPE = np.dtype([("position", "<f4", 3), ("t", "<f4"), ("normal", "<f4", 3), ("face", "<i4"), ("object_ref", "<u8"),
                      ("tie", "?")])
N_RAYS = 2000


def aim_points(doc):
    """The translations of the document's objects other than cameras and empties."""
    pts = [o["transform"]["transform_world"][9:12] for _, o in sorted(doc["objects"]["collection"].items(), key=lambda kv: int(kv[0]))
           if o["inner"] != "Empty" and "Camera" not in o["inner"]]
    return np.asarray(pts, np.float64).reshape(-1, 3)


def recipe_rays(seed, aims, n=N_RAYS):
    """[n, 8] float32 `bt_ray` rows: origins uniform in [-6, 6] x [-1.9, 6] x [-8, 10]; the first half aim at a random aim point
    plus N(0, 0.3), the next tenth are signed unit axis directions (parallel to walls, |q| <= 1e-5), the rest isotropic;
    directions normalised in float32; the last fifth get tmin ~ U(0, 6), tmax = tmin + U(0, 6), everything else [0.01, 1000]."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-6.0, -1.9, -8.0], [6.0, 6.0, 10.0], (n, 3)).astype(np.float32)
    n_aim, n_axis = n // 2, n // 10
    d = np.empty((n, 3), np.float32)
    target = aims[rng.integers(len(aims), size=n_aim)] + rng.normal(0.0, 0.3, (n_aim, 3))
    d[:n_aim] = (target - o[:n_aim]).astype(np.float32)
    axis, sign = rng.integers(3, size=n_axis), rng.choice([-1.0, 1.0], n_axis)
    d[n_aim:n_aim + n_axis] = 0.0
    d[np.arange(n_aim, n_aim + n_axis), axis] = sign
    d[n_aim + n_axis:] = rng.normal(0.0, 1.0, (n - n_aim - n_axis, 3)).astype(np.float32)
    l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    d = (d / np.sqrt(l2)[:, None]).astype(np.float32)
    rays = np.empty((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3], rays[:, 7] = 0.01, 1000.0
    k = n - n // 5
    rays[k:, 3] = rng.uniform(0.0, 6.0, n - k).astype(np.float32)
    rays[k:, 7] = rays[k:, 3] + rng.uniform(0.0, 6.0, n - k).astype(np.float32)
    return rays


def try_hit(o, sc, rays, ties=False):
    """REF_DTYPE records: the oracle's try_hit per ray; a miss has t = inf, face = -1, object_ref = NO_REF and zeros.  With
    `ties`, `tie` marks the rays that meet two objects at the winning t, bit for bit, each object tested alone against the ray's
    own clip (a second pass over the objects)."""
    objs = [j for j in range(sc.c.n_objects) if sc._objects[j].kind not in (o.EMPTY, o.CAMERA)]
    out = np.zeros(len(rays), REF_DTYPE)
    out["t"], out["face"], out["object_ref"] = np.inf, -1, NO_REF
    for i, r in enumerate(rays):
        org, d, tmin, clip_max = r[0:3], r[4:7], float(r[3]), float(r[7])
        best = None
        for j in objs:
            h = o.object_hit(sc, j, org, d, (tmin, clip_max))
            if h is not None:
                clip_max, best = h["t"], (j, h)
        if best is not None:
            j, h = best
            tie = False
            if ties:
                alone = [o.object_hit(sc, k, org, d, (tmin, float(r[7]))) for k in objs]
                tie = sum(1 for a in alone if a is not None and np.float32(a["t"]) == np.float32(h["t"])) >= 2
            out[i] = (h["position"], h["t"], h["normal"], FACES[h["face"]], sc.object_keys[j], tie)
    out.flags.writeable = False
    return out


def materials_of(doc):
    """object_ref -> the set of material refs a hit on the object may report (a cuboid: its faces')."""
    mats = {}
    for k, obj in doc["objects"]["collection"].items():
        inner = obj["inner"]
        if inner == "Empty" or "Camera" in inner:
            continue
        (name, body), = inner.items()
        mats[int(k)] = {int(r["material"]) for _, r in body["faces"]} if name == "Cuboid" else {int(body["material"])}
    return mats


def volumes_of(doc):
    return {int(k): obj["inner"]["Sphere"]["volume"] for k, obj in doc["objects"]["collection"].items()
            if obj["inner"] != "Empty" and "Sphere" in obj["inner"]}


_CACHE = {}


def reference(o, key, text, seed, aims=None, ties=False):
    """(rays [N_RAYS, 8] float32, REF_DTYPE records, doc) of one batch, computed once per (key, seed)."""
    if (key, seed) not in _CACHE:
        doc = json.loads(text)
        rays = recipe_rays(seed, aim_points(doc) if aims is None else aims)
        rays.flags.writeable = False
        _CACHE[(key, seed)] = (rays, try_hit(o, o.Scene(doc), rays, ties), doc)
    return _CACHE[(key, seed)]
