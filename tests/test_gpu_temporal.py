"""Temporal accumulation with reprojection on the GPU (EXTENSION): resets, a camera that does not move, a
known-answer shift, disocclusion, real frames against the float32 numpy restatement (tests/temporal_ref.py), renders left
untouched, and the error against a converged render under a moving camera."""
import numpy as np
import pytest

import temporal_ref as tr
from conftest import scene_path
from test_view_projection import BASE_L, BASE_T, make_view, rot

pytestmark = pytest.mark.gpu

EXPLICIT = dict(alpha_min=0.05, max_history=256.0, depth_tolerance=0.05, normal_min=0.9)
# per-frame camera motion of the sequences on real frames: a translation along the camera's own x axis, in scene units, that
# moves the image by about one pixel of a 128-pixel-wide frame (the pixel's angle times the distance to what the camera looks at)
STEP_128 = {"scene": 0.026, "cornell2": 0.037, "volume": 0.026}


def _buffer(bendy, arr, samples):
    import torch
    b = bendy.Buffer.new(arr.shape[1], arr.shape[0])
    b.data.copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)))
    b.samples = samples
    return b


def _scene(bendy, name, w, h):
    sc = bendy.Scene.load(scene_path(name))
    cam = sc.find_by_tag("camera")
    sc.set_camera_aspect(cam, w / h)
    return sc, cam


def _frame(bendy, sc, cam, w, h, spp, n, base, seed=0x5EED, albedo=False):
    """One displayed frame: cleared buffers, `spp` x Subpixel(n) samples from index `base` through the guided pass."""
    bufs = [bendy.Buffer.new(w, h) for _ in range(4 if albedo else 3)]
    color, normal, depth = bufs[0], bufs[-2], bufs[-1]
    bendy.Tracer.new().render_guided(sc, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n)), color,
                                     bufs[1] if albedo else None, normal, depth, seed=seed, sample_base=base)
    return bufs


def moved_pose(m0, f, step, yaw=0.0, lift=0.0, pitch=0.0):
    """The base pose `m0` (12 floats) after f frames: translated by f * step along its own x axis and f * lift along its own y,
    yawed by f * yaw about its own y and pitched by f * pitch about its own x."""
    m = np.asarray(m0, dtype=np.float64).copy()
    L = m[:9].reshape(3, 3).T
    m[9:] += f * step * L[:, 0] + f * lift * L[:, 1]
    m[:9] = (L @ rot([0, 1, 0], f * yaw) @ rot([1, 0, 0], f * pitch)).T.reshape(-1)
    return m.astype(np.float32)


def _tolerance(hist_prev, c, expected, xf, yf):
    """4 eps_px max|taps, c| + 1e-5 |expected|, per pixel and channel of (rgb, length): the taps are the history texels within
    one pixel of the reprojected position, whichever side of it rounding puts the float32 position on."""
    H, W = c.shape[:2]
    big = np.zeros((H, W, 4), dtype=np.float64)
    x0, y0 = np.floor(np.nan_to_num(xf)).astype(int), np.floor(np.nan_to_num(yf)).astype(int)
    for j in (-1, 0, 1, 2):
        for i in (-1, 0, 1, 2):
            qx, qy = np.clip(x0 + i, 0, W - 1), np.clip(y0 + j, 0, H - 1)
            near = (np.abs(x0 + i - xf) <= 1.01) & (np.abs(y0 + j - yf) <= 1.01)
            big = np.maximum(big, np.where(near[..., None], np.abs(hist_prev[qy, qx]), 0.0))
    big[..., :3] = np.maximum(big[..., :3], np.abs(c[..., :3]))
    return 4 * tr.EPS_PX * big + 1e-5 * np.abs(expected)


# ---- 1. reset ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 1), (16, 17), (45, 35)])
def test_first_call_and_reset_write_the_frames_own_mean(bendy, w, h):
    rng = np.random.default_rng(w * 100 + h)
    t = bendy.Temporal(w, h, **EXPLICIT)
    view = make_view(bendy, BASE_L, BASE_T, w, h, 2)
    moved = make_view(bendy, BASE_L @ rot([0, 1, 0], 0.01), BASE_T, w, h, 2)

    def inputs(nc):
        C_ = rng.random((h, w, 4), dtype=np.float32) * nc
        C_[..., 3] = rng.random((h, w), dtype=np.float32)
        N_ = rng.standard_normal((h, w, 4)).astype(np.float32)
        D_ = rng.random((h, w, 4), dtype=np.float32) * 5
        return C_, N_, D_

    for round_, nc in enumerate((3, 7, 5)):
        C_, N_, D_ = inputs(nc)
        out = t.accumulate(view if round_ != 1 else moved, _buffer(bendy, C_, nc), _buffer(bendy, N_, 2), _buffer(bendy, D_, 5))
        got, hist = out.numpy(), t.history()
        if round_ == 1:                                   # a second call blends (or resets pixel by pixel): not what is checked here
            assert out.samples == 1 and (hist[..., 3] >= nc).all()
            t.reset()
            assert not t.history().any()
            continue
        assert np.array_equal(got[..., :3], C_[..., :3] / np.float32(nc))          # bit for bit
        assert np.array_equal(got[..., 3], C_[..., 3])
        assert np.array_equal(hist[..., :3], got[..., :3]) and (hist[..., 3] == nc).all()
    t.close()


# ---- 2. a camera that does not move ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_static_camera_accumulates_the_running_mean(bendy, name):
    import torch
    w, h, spp, n, frames = 45, 35, 4, 2, 4
    sc, cam = _scene(bendy, name, w, h)
    view = sc.camera_view(cam, bendy.Config(), bendy.RenderConfig(subsample=bendy.Subsample(n)), w, h)
    t = bendy.Temporal(w, h)
    params = dict(alpha_min=0.0, max_history=1e9, depth_tolerance=0.05, normal_min=0.9)
    total, state = bendy.Buffer.new(w, h), None
    for f in range(frames):
        color, normal, depth = _frame(bendy, sc, cam, w, h, spp, n, f * spp)
        out = t.accumulate(view, color, normal, depth, **params)
        ref, state, _ = tr.accumulate(state, view, color.numpy(), color.samples, normal.numpy(), normal.samples, depth.numpy(),
                                      depth.samples, **params)
        bendy.Tracer.new().render(sc, cam, bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n)), total)   # the plain running sums
        torch.cuda.synchronize()
        got, hist = out.numpy(), t.history()
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
        np.testing.assert_allclose(got[..., :3], total.mean(), rtol=1e-5, atol=0)
        assert total.samples == (f + 1) * spp * n * n and (hist[..., 3] == total.samples).all()
    t.close()


# ---- 3. / 4. shift known-answer test and disocclusion -------------------------------------------------------------------------

NC_A, NC_B, NN, ND = 3, 2, 4, 4


def _shift_inputs(w, h, k, seed):
    """Frame A (random colour, unit normals, depths in (0.05, 0.75) with columns 5 and 6 at z = 1) and frame B: A's guides moved by k
    columns (B[x] = A[x + k]; the columns without a source random) under fresh colours."""
    rng = np.random.default_rng(seed)

    def frame():
        C_ = rng.random((h, w, 4), dtype=np.float32)
        C_[..., :3] *= 4.0
        N_ = rng.standard_normal((h, w, 4)).astype(np.float32)
        N_[..., :3] /= np.linalg.norm(N_[..., :3], axis=-1, keepdims=True)
        D_ = np.repeat((0.05 + 0.7 * rng.random((h, w), dtype=np.float32))[..., None], 4, axis=-1)
        D_[:, 5:7] = 1.0
        return C_, N_, D_

    A, B = frame(), frame()
    for a, b in zip(A[1:], B[1:]):
        b[:, :w - k] = a[:, k:]
    return A, B


def _shift_views(bendy, w, h, k):
    """prev, cur: the previous camera is the current one yawed by k pixels, so pixel (x, y) of cur lies at (x + k, y) of prev."""
    cur = make_view(bendy, BASE_L, BASE_T, w, h, 2)
    theta = k * (float(cur.xfov) / 2) * (2.0 / w)
    return make_view(bendy, BASE_L @ rot([0, 1, 0], theta), BASE_T, w, h, 2), cur


def _run_shift(bendy, w, h, k, A, B, with_normal=True):
    prev, cur = _shift_views(bendy, w, h, k)
    t = bendy.Temporal(w, h, **EXPLICIT)
    Ca, Na, Da = A[0].copy(), A[1] * np.float32(NN), A[2] * np.float32(ND)          # means -> running sums
    Cb, Nb, Db = B[0].copy(), B[1] * np.float32(NN), B[2] * np.float32(ND)
    Ca[..., :3] *= NC_A
    Cb[..., :3] *= NC_B
    nbuf = lambda N_: _buffer(bendy, N_, NN) if with_normal else None
    t.accumulate(prev, _buffer(bendy, Ca, NC_A), nbuf(Na), _buffer(bendy, Da, ND))
    hist_a = t.history()
    out = t.accumulate(cur, _buffer(bendy, Cb, NC_B), nbuf(Nb), _buffer(bendy, Db, ND)).numpy()
    hist_b = t.history()
    t.close()
    _, st, _ = tr.accumulate(None, prev, Ca, NC_A, Na if with_normal else None, NN, Da, ND, **EXPLICIT)
    assert np.array_equal(st["hist"], hist_a)
    ref, _, info = tr.accumulate(st, cur, Cb, NC_B, Nb if with_normal else None, NN, Db, ND, **EXPLICIT)
    return out, hist_a, hist_b, Cb, ref, info


@pytest.mark.parametrize("w,h", [(45, 35), (64, 36)])
@pytest.mark.parametrize("k", [1, 3])
def test_shift_by_k_columns(bendy, w, h, k):
    A, B = _shift_inputs(w, h, k, seed=w + k)
    out, hist_a, hist_b, Cb, _, info = _run_shift(bendy, w, h, k, A, B)
    c = Cb[..., :3] / np.float32(NC_B)
    # columns with a source: m = the history moved by k columns, N = NC_A + NC_B, alpha = NC_B / N
    m = hist_a[:, k:, :3]
    N = np.float32(NC_A + NC_B)
    alpha = max(np.float32(NC_B) / N, np.float32(EXPLICIT["alpha_min"]))
    expected = m + (c[:, :w - k] - m) * alpha
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64) + k, np.arange(h, dtype=np.float64))
    tol = _tolerance(hist_a, c, np.concatenate([np.pad(expected, ((0, 0), (0, k), (0, 0))), np.full((h, w, 1), N)], axis=-1), xs, ys)
    err = np.abs(out[:, :w - k, :3].astype(np.float64) - expected)
    print(f"shift {k} at {w}x{h}: largest error {err.max():.3e}, tolerance there {tol[:, :w - k, :3][err == err.max()].max():.3e}")
    assert (err <= tol[:, :w - k, :3]).all()
    assert np.abs(hist_b[:, :w - k, 3] - N).max() <= 4 * tr.EPS_PX * NC_A + 1e-5 * N
    assert np.array_equal(hist_b[:, :w - k, :3], out[:, :w - k, :3])
    # revealed columns: a reset, exact
    assert np.array_equal(out[:, w - k:, :3], c[:, w - k:]) and (hist_b[:, w - k:, 3] == NC_B).all()
    assert np.array_equal(out[..., 3], Cb[..., 3])
    assert np.abs(info["xf"] - xs).max() <= tr.EPS_PX and np.abs(info["yf"] - ys).max() <= tr.EPS_PX


@pytest.mark.parametrize("w,h,k", [(45, 35, 1), (64, 36, 3)])
def test_disocclusion_resets_exactly_the_changed_pixels(bendy, w, h, k):
    A, B = _shift_inputs(w, h, k, seed=7 * w + k)
    depth_rect = (slice(4, 15), slice(10, 22))                 # rows, columns of the PREVIOUS frame, clear of the z = 1 columns
    normal_rect = (slice(18, 30), slice(25, 40))

    def expected_reset(rects):
        e = np.zeros((h, w), dtype=bool)
        e[:, w - k:] = True                                     # no source
        for rows, cols in rects:
            e[rows, cols.start - k:cols.stop - k] = True        # pixel (x, y) looks at (x + k, y)
        return e

    Ad = (A[0], A[1], A[2].copy())
    Ad[2][depth_rect] *= np.float32(1.0 + 4 * EXPLICIT["depth_tolerance"])      # pushed beyond depth_tolerance
    Ad[2][depth_rect] = np.minimum(Ad[2][depth_rect], np.float32(0.99))
    assert (np.abs(Ad[2][depth_rect] - A[2][depth_rect]) > 2 * EXPLICIT["depth_tolerance"] * A[2][depth_rect]).all()
    An = (A[0], A[1].copy(), A[2])
    An[1][normal_rect] *= np.float32(-1.0)
    Adn = (A[0], An[1], Ad[2])
    for prev_frame, with_normal, rects in ((Ad, True, [depth_rect]), (An, True, [normal_rect]),
                                           (Adn, True, [depth_rect, normal_rect]), (Adn, False, [depth_rect])):
        out, _, hist_b, Cb, _, info = _run_shift(bendy, w, h, k, prev_frame, B, with_normal)
        reset = hist_b[..., 3] == NC_B
        # (fragile here: the first and last rows and the last column with a source, where a shift by whole pixels puts a
        # zero-weight tap on the frame's edge; every pixel inside is checked)
        want, keep = expected_reset(rects), ~info["fragile"]
        assert keep[1:-1, :w - k - 1].mean() > 0.98
        assert np.array_equal(reset[keep], want[keep])
        assert np.array_equal(info["reset"][keep], want[keep])                   # the restatement agrees
        c = Cb[..., :3] / np.float32(NC_B)
        assert np.array_equal(out[..., :3][reset], c[reset])


# ---- 5. real frames against the restatement ---------------------------------------------------------------------------------

SEQ_YAW = 0.002                                             # radians per frame, about the camera's own y axis


def real_sequence_views(bendy, sc, cam, name, w, h, n, frames=3):
    base = sc.camera_view(cam, bendy.Config(), bendy.RenderConfig(subsample=bendy.Subsample(n)), w, h)
    # (the lift and the pitch keep the frame's first and last rows, near and far pixels alike, from landing on a row of the
    # previous frame to within eps_px, where the restatement would call every pixel of them fragile: which taps are inside the
    # frame would hang on the last ulp)
    step = STEP_128[name] * 128.0 / w * 0.6
    poses = [moved_pose(base.matrix(), f, step, SEQ_YAW, 0.37 * step, 0.4 * SEQ_YAW) for f in range(frames)]
    return base, poses


@pytest.mark.parametrize("w,h", [(64, 36), (45, 35)])
@pytest.mark.parametrize("name", ["scene", "cornell2", "volume"])
def test_real_frames_match_the_restatement(bendy, name, w, h):
    spp, n = 2, 2
    sc, cam = _scene(bendy, name, w, h)
    base, poses = real_sequence_views(bendy, sc, cam, name, w, h, n)
    t = bendy.Temporal(w, h, **EXPLICIT)
    state, worst = None, 0.0
    for f, pose in enumerate(poses):
        sc.set_camera_pose(cam, pose)
        view = sc.camera_view(cam, bendy.Config(), bendy.RenderConfig(subsample=bendy.Subsample(n)), w, h)
        color, normal, depth = _frame(bendy, sc, cam, w, h, spp, n, f * spp)
        out = t.accumulate(view, color, normal, depth).numpy()
        hist = t.history()
        C_, N_, D_ = color.numpy(), normal.numpy(), depth.numpy()
        ref, new_state, info = tr.accumulate(state, view, C_, color.samples, N_, normal.samples, D_, depth.samples, **EXPLICIT)
        fragile = info["fragile"]
        assert fragile.mean() <= 0.02, f"frame {f}: {fragile.mean():.3%} of the pixels are fragile"
        if state is None:
            assert np.array_equal(out, ref) and np.array_equal(hist, new_state["hist"])
        else:
            assert not info["reset"].all() and info["reset"].mean() < 0.5       # the sequence does reproject
            c = C_[..., :3] / np.float32(color.samples)
            want = new_state["hist"]
            tol = _tolerance(state["hist"], c, want, info["xf"], info["yf"])
            err = np.abs(hist.astype(np.float64) - want)
            ok = (err <= tol).all(axis=-1) | fragile
            worst = max(worst, float((err / np.maximum(tol, 1e-30))[~fragile].max()))
            assert ok.all(), f"frame {f}: {int((~ok).sum())} pixels off, worst error / tolerance {worst:.3f}"
            assert np.array_equal(out[..., :3], hist[..., :3]) and np.array_equal(out[..., 3], C_[..., 3])
        # the next frame's restatement starts from the GPU's own history (and the guides both derive bit for bit from the inputs)
        state = dict(hist=hist, guide=new_state["guide"], view=view)
    print(f"{name} {w}x{h}: worst error / tolerance on non-fragile pixels {worst:.3f}")
    t.close()


# ---- 6. renders are untouched -------------------------------------------------------------------------------------------------

def test_renders_are_untouched_by_accumulate_and_a_pose_round_trip(bendy):
    import torch
    w, h, spp, n = 45, 35, 2, 2
    sc, cam = _scene(bendy, "scene", w, h)
    rc = bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))

    def renders():
        plain = bendy.Buffer.new(w, h)
        bendy.Tracer.new().render(sc, cam, rc, plain)
        guided = _frame(bendy, sc, cam, w, h, spp, n, 0, albedo=True)
        torch.cuda.synchronize()
        return [plain.numpy().copy()] + [g.numpy().copy() for g in guided]

    before = renders()
    assert np.array_equal(before[0], before[1])
    base = sc.camera_view(cam, bendy.Config(), rc, w, h)
    t = bendy.Temporal(w, h, **EXPLICIT)
    for f in range(3):
        sc.set_camera_pose(cam, moved_pose(base.matrix(), f, 0.05, 0.004))
        view = sc.camera_view(cam, bendy.Config(), rc, w, h)
        color, normal, depth = _frame(bendy, sc, cam, w, h, spp, n, f * spp)
        t.accumulate(view, color, normal, depth)
    sc.set_camera_pose(cam, base.matrix())
    after = renders()
    for a, b_ in zip(before, after):
        assert np.array_equal(a, b_)
    t.close()


# ---- 7. it helps ------------------------------------------------------------------------------------------------------------

def rel_mse(x, y):
    """mean((x - y)^2 / (y^2 + 0.01)), DESIGN.md 11."""
    x, y = x[..., :3].astype(np.float64), y[..., :3].astype(np.float64)
    return float(np.mean((x - y) ** 2 / (y ** 2 + 0.01)))


def moving_camera_ratios(bendy, name, params=None, w=128, h=128, frames=8, spp=1, n=2):
    """The sequence of DESIGN.md 14: `frames` displayed frames of spp x Subpixel(n) samples, the camera translating by about a
    pixel per frame.  Returns relMSE ratios against a render of 1024 samples per pixel (256 x Subpixel(2)) at the last pose from another seed: temporal / last
    frame alone, denoise(temporal) / denoise(last frame), and a buffer that kept adding samples while the camera moved / last
    frame alone; and the mean history length."""
    import torch
    sc, cam = _scene(bendy, name, w, h)
    rc = bendy.RenderConfig(samples=spp, subsample=bendy.Subsample(n))
    base = sc.camera_view(cam, bendy.Config(), rc, w, h)
    t = bendy.Temporal(w, h, **(params or {}))
    naive = bendy.Buffer.new(w, h)
    for f in range(frames):
        sc.set_camera_pose(cam, moved_pose(base.matrix(), f, STEP_128[name] * 128.0 / w))
        view = sc.camera_view(cam, bendy.Config(), rc, w, h)
        color, albedo, normal, depth = _frame(bendy, sc, cam, w, h, spp, n, f * spp, albedo=True)
        out = t.accumulate(view, color, normal, depth)
        bendy.Tracer.new().render(sc, cam, rc, naive)
    truth = bendy.Buffer.new(w, h)
    bendy.Tracer.new().render(sc, cam, bendy.RenderConfig(samples=256, subsample=bendy.Subsample(n)), truth, seed=0xBEEF)
    den_last = bendy.denoise(color, albedo, normal, depth)
    den_temporal = bendy.denoise(out, albedo, normal, depth)
    torch.cuda.synchronize()
    y = truth.mean()
    last = rel_mse(color.mean(), y)
    res = dict(temporal=rel_mse(out.numpy(), y) / last, denoised=rel_mse(den_temporal.numpy(), y) / rel_mse(den_last.numpy(), y),
               naive=rel_mse(naive.mean(), y) / last, last=last, mean_history=float(t.history()[..., 3].mean()))
    t.close()
    return res


# relMSE(temporal) / relMSE(last frame alone) and the same for the denoised pair, as measured on an MI355X with the default
# parameters, plus the 25 % DESIGN.md 11 gives its ratios for seed-to-seed spread
HELPS_BOUNDS = {"scene": (0.116, 0.972), "cornell2": (0.080, 0.111)}       # measured 0.0928 / 0.777 and 0.0642 / 0.0887


@pytest.mark.parametrize("name", ["scene", "cornell2"])
def test_it_helps_under_a_moving_camera(bendy, name):
    r = moving_camera_ratios(bendy, name)
    print(f"{name}: relMSE ratio temporal / last frame {r['temporal']:.4f}, denoised pair {r['denoised']:.4f}, naive buffer "
          f"{r['naive']:.4f} (last frame's relMSE {r['last']:.4f}, mean history {r['mean_history']:.1f})")
    b_temporal, b_denoised = HELPS_BOUNDS[name]
    assert r["temporal"] <= b_temporal and r["temporal"] < 1
    assert r["denoised"] <= b_denoised and r["denoised"] < 1
