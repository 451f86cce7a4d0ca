"""Adaptive sampling (EXTENSION): Tracer.render_adaptive / bt_render_adaptive_device add a pass's samples to the
tiles whose error estimate is still above the threshold.  Yardsticks: the plain render (a tile with count c holds what
`Tracer.render` gives its pixels for c samples), the CPU oracle (its frames, and its per-sample colours through
`bt_oracle_py.trace_one` for the moments) and tests/adaptive_ref.py, the float32 restatement of the estimate.  Everything is
bit for bit unless said otherwise.

Counts are in samples per pixel, n^2 per subsampled sample, as `Buffer.samples` is: a pass of `samples` x Subpixel(n) adds
T = samples * n^2 to every active tile's count, and min_samples / max_samples are compared with that count."""
import functools

import numpy as np
import pytest

import adaptive_ref as R
from helpers import gpu_scene, oracle_scene

pytestmark = pytest.mark.gpu

SEED = 0x5EED
INVALID_ARG, UNSUPPORTED = -1, -9
BUNDLED = [("scene", 61, 37), ("cornell", 96, 54), ("cornell2", 45, 77), ("volume", 61, 37), ("cloud", 50, 30)]
# Thresholds of the runs to BT_DONE (45 x 35: nine tiles, the right column 13 and the bottom row 3 pixels wide; passes of 4
# samples, min 8, max 32).  Chosen on the CPU from the oracle's per-sample colours with adaptive_ref, so that tiles stop at
# different counts and no decision of the restatement lies within threshold * (1 +- 1e-4) -- which
# test_estimates_and_decisions asserts again, on the same colours.
RUNS = {"scene": 0.06, "cornell2": 0.2, "volume": 0.04}
W, H, PASS, MIN, MAX = 45, 35, 4, 8, 32


def _tracer(b):
    return b.Tracer.with_config(b.Config(chunks_x=8, chunks_y=4))


def _rc(b, spp, n=0):
    return b.RenderConfig(samples=spp, subsample=b.Subsample(n))


def _plain(b, sc, cam, w, h, spp, n=0):
    import torch
    buf = b.Buffer.new(w, h)
    _tracer(b).render(sc, cam, _rc(b, spp, n), buf, seed=SEED)
    torch.cuda.synchronize()
    return buf.numpy(), sc.last_stats()


@functools.lru_cache(maxsize=None)
def _oracle_samples(name, w, h, T, n=0):
    """The oracle's colour of every sample index 0 .. T-1 of every pixel (iterative form), float32 [T, h, w, 3]."""
    import bt_oracle_py as o
    sc, cam = oracle_scene(o, name, w, h)
    cfg = o.default_config(samples=1, subsample_n=n, recursive=0)
    out = np.zeros((T, h, w, 3), dtype=np.float32)
    for k in range(T):
        for y in range(h):
            for x in range(w):
                out[k, y, x] = o.trace_one(sc, cam, cfg, w, h, x, y, k, SEED)["color"]
    return out


def _oracle_frames(o, name, w, h, step, upto, n=0):
    """{count: the oracle's frame of running sums after `count` samples per pixel}, count = step, 2 step, ... upto."""
    sc, cam = oracle_scene(o, name, w, h)
    nn = max(1, n * n)
    frames, img = {}, None
    for base in range(0, upto, step):
        cfg = o.default_config(samples=step // nn, subsample_n=n, recursive=0, sample_base=base // nn)
        img, _, _ = o.render(sc, cam, cfg, w, h, SEED, nthreads=16, rgba=img)
        frames[base + step] = img.copy()
    return frames


def _composite(per_count, counts, w, h):
    """The frame whose tiles come from per_count[the tile's count]."""
    cpp = R.per_pixel(counts, w, h)
    out = np.zeros_like(next(iter(per_count.values())))
    for c, img in per_count.items():
        out[cpp == c] = img[cpp == c]
    assert set(np.unique(counts)) <= set(per_count)
    return out


_runs = {}


def _run(b, name, w=W, h=H, spp=PASS, n=0, limit=64, **params):
    """Passes until Status.Done on a fresh handle; after every pass the GPU's counts, sums, moments and errors."""
    key = (name, w, h, spp, n, tuple(sorted(params.items())))
    if key not in _runs:
        sc, cam = gpu_scene(b, name, w, h)
        buf, ad, tr = b.Buffer.new(w, h), b.Adaptive(w, h, **params), _tracer(b)
        hist = []
        for _ in range(limit):
            st = tr.render_adaptive(sc, cam, _rc(b, spp, n), buf, ad, seed=SEED)
            hist.append(dict(status=st, counts=ad.counts(), sums=buf.numpy().copy(), moments=ad.moments(), errors=ad.errors(),
                             stats=ad.poll(), segments=sc.last_stats().segments))
            if st == b.Status.Done:
                break
        _runs[key] = dict(sc=sc, cam=cam, buf=buf, ad=ad, hist=hist)
    return _runs[key]


# ---- 1. threshold 0, min = max = N: the plain render of N samples ------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("name,w,h", BUNDLED)
def test_one_pass_of_everything_is_the_plain_render(bendy, name, w, h, n):
    spp = 2 if n else 5
    N = spp * max(1, n * n)
    sc, cam = gpu_scene(bendy, name, w, h)
    want, wstats = _plain(bendy, sc, cam, w, h, spp, n)
    buf, ad = bendy.Buffer.new(w, h), bendy.Adaptive(w, h, threshold=0.0, min_samples=N, max_samples=N)
    st = _tracer(bendy).render_adaptive(sc, cam, _rc(bendy, spp, n), buf, ad, seed=SEED)
    stats = sc.last_stats()
    assert st == bendy.Status.Done and buf.samples == 0                      # every tile reached the cap; the buffer's counter is not used
    assert np.array_equal(buf.numpy(), want)
    assert (ad.counts() == N).all()
    assert stats.segments == wstats.segments and stats.packed == 0
    p = ad.poll()
    assert (p.active_tiles, p.min_count, p.max_count, p.pixel_samples, p.passes) == (0, N, N, w * h * N, 1)
    # a further pass is refused nothing and changes nothing
    assert _tracer(bendy).render_adaptive(sc, cam, _rc(bendy, spp, n), buf, ad, seed=SEED) == bendy.Status.Done
    assert np.array_equal(buf.numpy(), want) and ad.poll().passes == 1


@pytest.mark.parametrize("slices", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("name", ["scene", "cornell2", "volume"])
def test_every_pinned_slices(bendy, name, slices):
    """Both shapes of the summing wave (blocks of >= 64 pixels, and the shuffled one below): frame, moments and segments do not
    depend on the shape.  bt_tuning.packed = 2 is pinned too: an adaptive pass is never packed."""
    w, h, spp = 61, 37, 6
    sc0, cam0 = gpu_scene(bendy, name, w, h)
    want, wstats = _plain(bendy, sc0, cam0, w, h, spp)
    sc, cam = gpu_scene(bendy, name, w, h, tuning={"slices": slices, "packed": 2})
    buf, ad = bendy.Buffer.new(w, h), bendy.Adaptive(w, h, threshold=0.0, min_samples=spp, max_samples=spp)
    assert _tracer(bendy).render_adaptive(sc, cam, _rc(bendy, spp), buf, ad, seed=SEED) == bendy.Status.Done
    stats = sc.last_stats()
    assert stats.slices == slices and stats.packed == 0 and stats.segments == wstats.segments
    assert np.array_equal(buf.numpy(), want) and (ad.counts() == spp).all()
    assert np.array_equal(ad.moments(), R.moment_of(_oracle_samples(name, w, h, spp)))


def test_small_scratch_cap_splits_the_pass(bendy):
    """The cap that makes 40 plain samples four launches (12 + 12 + 12 + 4, as tests/test_gpu_parity.py pins it) does the same
    to an adaptive pass; the tiles are judged once, behind the last part."""
    w, h, spp = 64, 48, 40
    sc, cam = gpu_scene(bendy, "volume", w, h, tuning={"scratch_cap_bytes": 64 * 48 * 12 * 12})
    want, wstats = _plain(bendy, sc, cam, w, h, spp)
    assert wstats.launches == 4
    buf, ad = bendy.Buffer.new(w, h), bendy.Adaptive(w, h, threshold=0.0, min_samples=spp, max_samples=spp)
    assert _tracer(bendy).render_adaptive(sc, cam, _rc(bendy, spp), buf, ad, seed=SEED) == bendy.Status.Done
    stats = sc.last_stats()
    assert stats.launches == 4 and stats.segments == wstats.segments
    assert np.array_equal(buf.numpy(), want) and (ad.counts() == spp).all() and ad.poll().passes == 1
    assert np.array_equal(ad.moments(), R.moment_of(_oracle_samples("volume", w, h, spp)))


# ---- 2. a real threshold, until BT_DONE ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(RUNS))
def test_run_to_done_matches_the_oracle_tile_by_tile(bendy, oracle, name):
    run = _run(bendy, name, threshold=RUNS[name], min_samples=MIN, max_samples=MAX)
    hist = run["hist"]
    assert hist[-1]["status"] == bendy.Status.Done and all(p["status"] == bendy.Status.InProgress for p in hist[:-1])
    assert hist[-1]["stats"].active_tiles == 0 and hist[-1]["stats"].passes == len(hist) <= MAX // PASS
    prev = np.zeros_like(hist[0]["counts"])
    stopped = np.zeros(prev.shape, dtype=bool)
    for p in hist:
        c = p["counts"]
        assert ((c - prev == PASS) | (c == prev)).all()                       # never less, never another step
        assert (c[stopped] == prev[stopped]).all()                           # stopped once, stopped for good
        stopped |= c == prev
        assert p["stats"].active_tiles <= (~stopped).sum()
        assert (p["stats"].min_count, p["stats"].max_count) == (c.min(), c.max())
        assert p["stats"].pixel_samples == int(R.per_pixel(c, W, H).astype(np.int64).sum())
        prev = c
    final = hist[-1]["counts"]
    assert (final % PASS == 0).all() and final.min() >= MIN and final.max() <= MAX
    assert len(np.unique(final)) >= 2, "the threshold was chosen so that tiles stop at different counts"
    frames = _oracle_frames(oracle, name, W, H, PASS, int(final.max()))
    assert np.array_equal(hist[-1]["sums"], _composite(frames, final, W, H))
    for p in hist[:-1]:                                                       # ... and after every pass before the last
        assert np.array_equal(p["sums"], _composite(frames, p["counts"], W, H))


# ---- 3. moments ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,spp", [(0, 4), (2, 1)])
@pytest.mark.parametrize("name", list(RUNS))
def test_moments_equal_the_restatement_over_the_oracles_samples(bendy, name, n, spp):
    """32 x 32, at most 16 samples per pixel.  With Subpixel(2) too: trace_one's sample index is the flat one (sample * n^2 +
    sub-pixel), so it reaches every sub-sample."""
    w = h = 32
    T = spp * max(1, n * n)
    run = _run(bendy, name, w, h, spp, n, threshold=RUNS[name], min_samples=T, max_samples=16)
    samples = _oracle_samples(name, w, h, 16, n)
    final = run["hist"][-1]["counts"]
    assert final.max() <= 16 and (final % T == 0).all()
    want_m, want_s = np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
    cpp = R.per_pixel(final, w, h)
    for c in np.unique(final):
        sums = np.zeros((h, w, 3), np.float32)
        for k in range(c):
            sums = sums + samples[k]
        want_m[cpp == c] = R.moment_of(samples[:c])[cpp == c]
        want_s[cpp == c] = sums[cpp == c]
    assert np.array_equal(run["hist"][-1]["moments"], want_m)
    assert np.array_equal(run["hist"][-1]["sums"][..., :3], want_s)


# ---- 4. estimates and decisions ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(RUNS))
def test_estimates_and_decisions(bendy, name):
    """errors() against adaptive_ref on the GPU's own sums, moments and counts: relative 1e-4 -- a sum of at most 256
    non-negative floats in any order is within 255 * 2^-24 = 1.5e-5 of exact, the division adds one rounding.  Every (tile, pass)
    decision whose reference e_t lies outside threshold * (1 +- 1e-4) must be the restatement's; at most 1 % may lie inside."""
    thr = RUNS[name]
    hist = _run(bendy, name, threshold=thr, min_samples=MIN, max_samples=MAX)["hist"]
    lo, hi = float(np.float32(thr)) * (1 - 1e-4), float(np.float32(thr)) * (1 + 1e-4)
    prev_c = np.zeros_like(hist[0]["counts"])
    prev_e = np.zeros_like(hist[0]["errors"])
    decisions = unchecked = 0
    for i, p in enumerate(hist):
        c, e = p["counts"], p["errors"]
        ran = c > prev_c                                                     # the tiles this pass sampled and judged
        ref = R.tile_error(p["sums"], p["moments"], c)
        print(name, "pass", i, "max rel err", float(np.max(np.abs(e[ran] - ref[ran]) / np.maximum(ref[ran], 1e-30))) if ran.any() else 0.0)
        assert (np.abs(e[ran].astype(np.float64) - ref[ran]) <= 1e-4 * ref[ran]).all()
        assert np.array_equal(e[~ran], prev_e[~ran])                         # a stopped tile keeps its last estimate
        went_on = hist[i + 1]["counts"] > c if i + 1 < len(hist) else np.zeros(c.shape, dtype=bool)
        want = R.goes_on(c, ref, thr, MIN, MAX)
        inside = (ref >= lo) & (ref <= hi) & (c >= MIN) & (c < MAX)
        decisions += int(ran.sum())
        unchecked += int((ran & inside).sum())
        assert np.array_equal(went_on[ran & ~inside], want[ran & ~inside])
        prev_c, prev_e = c, e
    assert unchecked * 100 <= decisions
    # the same passes by the restatement alone, on the oracle's per-sample colours: no decision inside the band, and the
    # counts the GPU ended with
    samples = _oracle_samples(name, W, H, MAX)
    ty, tx = R.tile_shape(W, H)
    counts, active = np.zeros((ty, tx), dtype=np.int64), np.ones((ty, tx), dtype=bool)
    sums, mom = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    for i in range(len(hist)):
        on = R.per_pixel(active, W, H)
        for k in range(i * PASS, (i + 1) * PASS):
            sums[on] = (sums + samples[k])[on]
        mom[on] = R.moment_add(mom, samples[i * PASS:(i + 1) * PASS])[on]
        counts[active] += PASS
        ref = R.tile_error(sums, mom, counts)
        assert not (active & (ref >= lo) & (ref <= hi) & (counts >= MIN) & (counts < MAX)).any()
        active &= R.goes_on(counts, ref, thr, MIN, MAX)
        assert np.array_equal(counts, hist[i]["counts"])
    assert not active.any()


# ---- 5. tiles that see nothing stop at min_samples -----------------------------------------------------------------------------

def test_empty_tiles_stop_at_min_samples(bendy):
    """Every sample of a tile whose primary rays hit nothing is the background's value v, so its variance is 0 up to rounding:
    S and M are sums of c equal terms, each partial sum rounded once (relative error <= (c - 1) u, u = 2^-24), so M / c and
    mu * mu each lie within about (c + 2) u of Y^2 relatively, var <= 2 (c + 2) u Y^2 and
    e_p = sqrt(var / c) / (mu + eps) <= sqrt(2 (1 + 2 / c) u) = 3.9e-4 at c = 8 -- a fiftieth of the threshold of 0.02."""
    w, h, spp, mn, mx = 160, 96, 4, 8, 24
    sc, cam = gpu_scene(bendy, "scene", w, h)
    masks = _tracer(bendy).primary_masks(sc, cam, _rc(bendy, spp), w, h, slices=1).reshape(R.tile_shape(w, h))
    empty = masks == 0
    assert empty.sum() >= 4 and (~empty).sum() >= 4
    run = _run(bendy, "scene", w, h, spp, 0, threshold=0.02, min_samples=mn, max_samples=mx)
    final, err = run["hist"][-1]["counts"], run["hist"][-1]["errors"]
    assert (final[empty] == mn).all()
    assert (err[empty] <= 3.9e-4).all()
    assert final.max() > mn                                                  # ... while other tiles went on


# ---- 6. the resolved mean ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(RUNS))
def test_resolve_preview_and_denoise(bendy, oracle, name):
    import torch
    run = _run(bendy, name, threshold=RUNS[name], min_samples=MIN, max_samples=MAX)
    final = run["hist"][-1]["counts"]
    mean = run["ad"].resolve(run["buf"])
    assert mean.samples == 1 and mean.color_space == run["buf"].color_space and mean.data.data_ptr() != run["buf"].data.data_ptr()
    frames = _oracle_frames(oracle, name, W, H, PASS, int(final.max()))
    shown = {c: oracle.preview(img, c).reshape(H, W, 4) for c, img in frames.items()}
    assert np.array_equal(mean.preview(), _composite(shown, final, W, H))
    assert np.array_equal(mean.numpy()[..., 3], run["buf"].numpy()[..., 3])
    out = bendy.Buffer.new(W, H)
    assert run["ad"].resolve(run["buf"], out=out) is out and np.array_equal(out.numpy(), mean.numpy())
    with pytest.raises(bendy.BendyError):
        run["ad"].resolve(run["buf"], out=run["buf"])
    plain = bendy.Buffer.new(W, H)
    plain.data.copy_(mean.data)
    plain.samples = 1
    a, b_ = bendy.denoise(mean), bendy.denoise(plain)
    torch.cuda.synchronize()
    assert np.array_equal(a.numpy(), b_.numpy()) and np.isfinite(a.numpy()).all()
    # a handle that has sampled nothing resolves to black
    zero = bendy.Adaptive(W, H).resolve(run["buf"]).numpy()
    assert not zero[..., :3].any() and np.array_equal(zero[..., 3], run["buf"].numpy()[..., 3])


# ---- 7. the scene handle's scratch is shared with the other renders -----------------------------------------------------------------

def _guided_frames(b, sc, cam, w, h, spp):
    import torch
    bufs = [b.Buffer.new(w, h) for _ in range(4)]
    _tracer(b).render_guided(sc, cam, _rc(b, spp), *bufs, seed=SEED)
    torch.cuda.synchronize()
    return [x.numpy() for x in bufs]


@pytest.mark.parametrize("name", ["scene", "cornell2", "volume"])
def test_other_renders_on_the_same_handle_are_unchanged(bendy, name):
    w, h = 61, 37
    params = dict(threshold=RUNS[name], min_samples=8, max_samples=24)
    sc, cam = gpu_scene(bendy, name, w, h)
    plain0, _ = _plain(bendy, sc, cam, w, h, 3)
    guided0 = _guided_frames(bendy, sc, cam, w, h, 3)
    buf, ad, tr = bendy.Buffer.new(w, h), bendy.Adaptive(w, h, **params), _tracer(bendy)

    def passes(spp=4):
        out = []
        while tr.render_adaptive(sc, cam, _rc(bendy, spp), buf, ad, seed=SEED) != bendy.Status.Done:
            out.append(ad.counts())
            assert len(out) < 16
        return out + [ad.counts()]

    first = passes()
    frame1, mom1 = buf.numpy().copy(), ad.moments()
    assert sc.last_stats().scratch_bytes >= w * h * 4 * 12                   # the handle's scratch, grown for the passes
    assert np.array_equal(_plain(bendy, sc, cam, w, h, 3)[0], plain0)
    assert all(np.array_equal(a, b_) for a, b_ in zip(_guided_frames(bendy, sc, cam, w, h, 3), guided0))
    # the same passes again after a reset, with the scratch trimmed, then shrunk by shallow renders in between
    for prepare in (lambda: sc.trim(), lambda: [_plain(bendy, sc, cam, 16, 16, 1) for _ in range(9)]):
        big, _ = _plain(bendy, sc, cam, w, h, 40)                            # grow ...
        prepare()                                                            # ... and give back
        sc.set_camera_aspect(cam, w / h)
        ad.reset()
        buf.clear()
        assert ad.poll().passes == 0 and not ad.counts().any() and not ad.moments().any()
        again = passes()
        assert len(again) == len(first) and all(np.array_equal(a, b_) for a, b_ in zip(again, first))
        assert np.array_equal(buf.numpy(), frame1) and np.array_equal(ad.moments(), mom1)
        assert np.array_equal(_plain(bendy, sc, cam, w, h, 40)[0], big)
    assert np.array_equal(_plain(bendy, sc, cam, w, h, 3)[0], plain0)
    assert all(np.array_equal(a, b_) for a, b_ in zip(_guided_frames(bendy, sc, cam, w, h, 3), guided0))


def test_a_changed_pass_size_is_refused_until_reset(bendy):
    """The refusal that needs an earlier pass (the others are in test_adaptive_abi.py): behind min > max, ahead of the lens."""
    w, h = 32, 32
    sc, cam = gpu_scene(bendy, "scene", w, h)
    buf, ad, tr = bendy.Buffer.new(w, h), bendy.Adaptive(w, h, threshold=0.0, min_samples=64, max_samples=64), _tracer(bendy)
    assert tr.render_adaptive(sc, cam, _rc(bendy, 4), buf, ad, seed=SEED) == bendy.Status.InProgress
    before = buf.numpy().copy()
    for rc in (_rc(bendy, 2), _rc(bendy, 4, 2), _rc(bendy, 1, 2)):
        with pytest.raises(bendy.BendyError) as e:
            tr.render_adaptive(sc, cam, rc, buf, ad, seed=SEED)
        assert e.value.code == INVALID_ARG and "earlier passes" in str(e.value)
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    with pytest.raises(bendy.BendyError) as e:
        tr.render_adaptive(sc, cam, _rc(bendy, 2), buf, ad, seed=SEED)
    assert e.value.code == INVALID_ARG                                       # ahead of the lens
    ad.params.min_samples = 65
    with pytest.raises(bendy.BendyError) as e:
        tr.render_adaptive(sc, cam, _rc(bendy, 2), buf, ad, seed=SEED)
    assert e.value.code == INVALID_ARG and "min_samples" in str(e.value)     # behind min > max
    ad.params.min_samples = 64
    with pytest.raises(bendy.BendyError) as e:
        tr.render_adaptive(sc, cam, _rc(bendy, 4), buf, ad, seed=SEED)
    assert e.value.code == UNSUPPORTED
    sc.clear_lens()
    assert np.array_equal(buf.numpy(), before) and ad.poll().passes == 1 and (ad.counts() == 4).all()
    with pytest.raises(bendy.BendyError) as e:                               # ... and ahead of samples == 0
        tr.render_adaptive(sc, cam, _rc(bendy, 0), buf, ad, seed=SEED)
    assert e.value.code == INVALID_ARG and "earlier passes" in str(e.value)
    assert tr.render_adaptive(sc, cam, _rc(bendy, 4), buf, ad, seed=SEED) == bendy.Status.InProgress
    assert (ad.counts() == 8).all()
    assert np.array_equal(buf.numpy(), _plain(bendy, sc, cam, w, h, 8)[0])   # two passes of 4 = the samples 0 .. 7
    ad.reset()
    buf.clear()
    assert tr.render_adaptive(sc, cam, _rc(bendy, 2, 2), buf, ad, seed=SEED) == bendy.Status.InProgress
    assert (ad.counts() == 8).all() and np.array_equal(buf.numpy(), _plain(bendy, sc, cam, w, h, 2, 2)[0])
