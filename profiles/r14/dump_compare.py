import hashlib, os, sys
O = sys.argv[1]
for wl in ("c3", "c5"):
    for f in ("frame.npy", "frame_index.npy"):
        p = [os.path.join(O, f"dump_{wl}_{v}", f) for v in ("parent", "new")]
        if not all(os.path.exists(q) for q in p):
            continue
        h = [hashlib.sha256(open(q, "rb").read()).hexdigest() for q in p]
        print(wl, f, os.path.getsize(p[0]), "bytes", "sha256", h[0][:16], h[1][:16], "IDENTICAL" if h[0] == h[1] else "DIFFERENT")
