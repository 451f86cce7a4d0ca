"""AOV-guided a-trous denoiser (include/bendy_hip.h `bt_denoiser`).  EXTENSION, NOT IN THE REFERENCE:
bendy-tracer v1 has no denoiser, so there is no parity claim.  The spec is tests/denoise_ref.py (float32 numpy, same tap
and operation order as bt_denoise.hip); the GPU must match it to the ulps of expf / powf, must improve real noisy frames,
must be deterministic and must leave every render untouched."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as ref
from conftest import ROOT, scene_path
from helpers import gpu_render, gpu_scene

CLI = os.path.join(ROOT, "bendy_tracer_amd", "bendy-tracer-hip")
PARAMS_B = dict(sigma_color=0.35, sigma_normal=8.0, sigma_depth=0.5, eps_albedo=0.05)
f32 = np.float32


def _inputs(w, h, seed):
    """Random running sums with the features the filter reacts to: albedo below eps, zero normals (misses), depth jumps."""
    rng = np.random.default_rng(seed)
    n = dict(n_c=7, n_a=3, n_n=5, n_d=2)
    color = np.empty((h, w, 4), f32)
    color[..., :3] = rng.uniform(0.0, 1.5, (h, w, 3)) * n["n_c"]
    color[..., 3] = rng.uniform(0.5, 1.0, (h, w))
    albedo = np.zeros((h, w, 4), f32)
    albedo[..., :3] = rng.uniform(0.0, 1.0, (h, w, 3)) * n["n_a"]
    albedo[..., :3][rng.uniform(size=(h, w, 3)) < 0.1] = 0.0
    v = rng.normal(size=(h, w, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v[..., 2] = np.abs(v[..., 2]) + 1.0                   # mostly facing one way, so that w_n is not ~0 everywhere
    v[rng.uniform(size=(h, w)) < 0.1] = 0.0
    normal = np.zeros((h, w, 4), f32)
    normal[..., :3] = v * n["n_n"]
    depth = np.zeros((h, w, 4), f32)
    depth[..., 0] = np.where(rng.uniform(size=(h, w)) < 0.5, 0.2, 0.6) * n["n_d"] + rng.uniform(0, 0.01, (h, w))
    return color, albedo, normal, depth, n


def _host_call(d, color, nc, albedo=None, na=0, normal=None, nn=0, depth=None, nd=0, out=None, w=None, h=None, params=None):
    from bendy_tracer_amd import api
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    p = api.DenoiseParams(**(params or {}))._c()
    return api.lib.bt_denoise(d, fp(color), nc, fp(albedo), na, fp(normal), nn, fp(depth), nd, fp(out),
                              color.shape[1] if w is None else w, color.shape[0] if h is None else h, C.byref(p))


# ---------------------------------------------------------------- the reference itself (CPU)

def test_reference_keeps_a_constant_frame():
    h, w = 23, 31
    color = np.full((h, w, 4), 0.3 * 4, f32)
    albedo = np.full((h, w, 4), 0.7 * 2, f32)
    normal = np.zeros((h, w, 4), f32)
    normal[..., 2] = 3.0
    depth = np.full((h, w, 4), 0.25, f32)
    got = ref.denoise(color, 4, albedo, 2, normal, 3, depth, 1)
    mean = color[..., :3] / f32(4)
    np.testing.assert_allclose(got[..., :3], mean, rtol=1e-6, atol=0)
    assert np.array_equal(got[..., 3], color[..., 3])


def test_reference_levels_0_is_the_mean():
    color, albedo, normal, depth, n = _inputs(19, 11, 1)
    got = ref.denoise(color, n["n_c"], albedo, n["n_a"], normal, n["n_n"], depth, n["n_d"], levels=0)
    assert np.array_equal(got[..., :3], color[..., :3] / f32(n["n_c"]))
    assert np.array_equal(got[..., 3], color[..., 3])


def test_reference_hard_normal_edge_does_not_bleed():
    """Left half faces +x with a constant colour, right half faces +z with noise: max(0, n_p . n_q)^64 = 0 across the
    edge, so the left half keeps its value for every level."""
    h, w = 32, 40
    rng = np.random.default_rng(3)
    color = np.zeros((h, w, 4), f32)
    color[:, :20, :3] = 0.8
    color[:, 20:, :3] = rng.uniform(0, 5, (h, 20, 3))
    normal = np.zeros((h, w, 4), f32)
    normal[:, :20, 0] = 1.0
    normal[:, 20:, 2] = 1.0
    got = ref.denoise(color, 1, None, 1, normal, 1, levels=5)
    assert np.abs(got[:, :20, :3] - f32(0.8)).max() <= 1e-6
    assert np.abs(got[:, 20:, :3] - color[:, 20:, :3]).max() > 0.1       # the noisy side was filtered


# ---------------------------------------------------------------- ABI and Python surface without a GPU

def test_abi_validation_comes_before_the_device(bendy):
    lib = bendy.api.lib
    d = lib.bt_denoiser_new()
    try:
        color, albedo, normal, depth, n = _inputs(8, 4, 2)
        out = np.zeros_like(color)
        ok = dict(albedo=albedo, na=3, normal=normal, nn=5, depth=depth, nd=2, out=out)
        bad = [
            dict(w=0), dict(h=0),
            dict(nc=0), dict(na=0), dict(nn=0), dict(nd=0),
            dict(params=dict(levels=11)),
            dict(params=dict(sigma_color=0.0)), dict(params=dict(sigma_color=-1.0)), dict(params=dict(sigma_color=math.inf)),
            dict(params=dict(sigma_color=math.nan)), dict(params=dict(sigma_depth=0.0)), dict(params=dict(sigma_depth=math.inf)),
            dict(params=dict(sigma_normal=-1.0)), dict(params=dict(sigma_normal=math.nan)),
            dict(out=color), dict(out=albedo), dict(out=normal), dict(out=depth), dict(out=None),
        ]
        for b in bad:
            args = {**ok, "nc": 7, **b}
            rc = _host_call(d, color, **args)
            assert rc == -1, (b, rc)
            assert lib.bt_last_error() and lib.bt_last_error_code() == -1
        # a guide whose pointer is NULL may carry a sample count of 0; sigma_normal = 0 is allowed
        for b in (dict(albedo=None, na=0), dict(normal=None, nn=0, depth=None, nd=0), dict(params=dict(sigma_normal=0.0)),
                  dict(params=dict(levels=10))):
            assert _host_call(d, color, **{**ok, "nc": 7, **b}) != -1, b
        assert lib.bt_denoise_device(d, None, 1, None, 0, None, 0, None, 0, None, 4, 4, None, None) == -1
        assert lib.bt_denoise_device(None, None, 1, None, 0, None, 0, None, 0, None, 4, 4, None, None) == -1
    finally:
        lib.bt_denoiser_free(d)


def test_valid_call_without_a_gpu_is_a_device_error(bendy):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bendy.api.lib
    d = lib.bt_denoiser_new()
    color, albedo, normal, depth, n = _inputs(8, 4, 2)
    out = np.zeros_like(color)
    assert _host_call(d, color, 7, albedo, 3, normal, 5, depth, 2, out) == -8
    assert _host_call(d, color, 7, out=out, params=dict(levels=0)) == -8
    lib.bt_denoiser_free(d)
    with pytest.raises(bendy.BendyError) as e:
        bendy.denoise(_cpu_buffer(bendy, color, 7))
    assert e.value.code == -8


def _cpu_buffer(bendy, data, samples, cs=None):
    b = bendy.Buffer.new(data.shape[1], data.shape[0], cs or bendy.ColorSpace.SRgb, device="cpu")
    b.data[...] = data
    b.samples = samples
    return b


def test_python_surface_and_mismatches(bendy):
    assert bendy.DenoiseParams() == bendy.DenoiseParams(**ref.DEFAULTS)
    c = bendy.api._CDenoiseParams()
    bendy.api.lib.bt_denoise_params_default(C.byref(c))
    assert (c.levels, c.sigma_color, c.sigma_normal, c.sigma_depth, c.eps_albedo) == (2, 16.0, 16.0, 1.0, f32(1e-3))
    color = _cpu_buffer(bendy, np.ones((4, 6, 4), f32), 1)
    small = _cpu_buffer(bendy, np.ones((4, 5, 4), f32), 1)
    dn = bendy.Denoiser()
    for kw in (dict(albedo=small), dict(normal=small), dict(depth=small), dict(out=small)):
        with pytest.raises(bendy.BendyError) as e:
            dn.denoise(color, **kw)
        assert e.value.code == -1
    with pytest.raises(bendy.BendyError):
        bendy.denoise(color, out=color)
    with pytest.raises(TypeError):
        bendy.denoise(color, sigma=2.0)
    dn.close()


# ---------------------------------------------------------------- GPU

def _gpu_denoise(bendy, dn, color, albedo, normal, depth, n, params, device="cuda"):
    import torch

    def buf(a, s):
        if a is None:
            return None
        b = bendy.Buffer.new(a.shape[1], a.shape[0], device=device)
        if device == "cpu":
            b.data[...] = a
        else:
            b.data.copy_(torch.from_numpy(a))
        b.samples = s
        return b
    out = dn.denoise(buf(color, n["n_c"]), buf(albedo, n["n_a"]), buf(normal, n["n_n"]), buf(depth, n["n_d"]), **params)
    if device != "cpu":
        torch.cuda.synchronize()
    return out.numpy().copy()


def _check_case(bendy, dn, size, levels, mask, params, seed):
    w, h = size
    color, albedo, normal, depth, n = _inputs(w, h, seed)
    g = [albedo if mask & 1 else None, normal if mask & 2 else None, depth if mask & 4 else None]
    got = _gpu_denoise(bendy, dn, color, *g, n, dict(levels=levels, **params))
    want = ref.denoise(color, n["n_c"], g[0], n["n_a"], g[1], n["n_n"], g[2], n["n_d"], levels=levels, **params)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=f"{size} levels={levels} guides={mask} {params}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (17, 9), (61, 37)])
def test_gpu_matches_reference_small(bendy, size):
    dn = bendy.Denoiser()
    for params in ({}, PARAMS_B):
        for levels in range(6):
            for mask in range(8):
                _check_case(bendy, dn, size, levels, mask, params, seed=levels * 8 + mask)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(256, 256), (768, 512)])
def test_gpu_matches_reference_large(bendy, size):
    dn = bendy.Denoiser()
    for params in ({}, PARAMS_B):
        _check_case(bendy, dn, size, 5, 7, params, seed=11)
    if size == (256, 256):
        for mask in range(7):
            _check_case(bendy, dn, size, 3, mask, {}, seed=mask)


def _rel_mse(x, y):
    return float(np.mean((x - y) ** 2 / (y * y + 0.01)))


# relMSE(denoised) / relMSE(noisy) with the default parameters, measured 0.047 / 0.143 / 0.137, plus ~25 %
QUALITY_BOUND = {"cornell": 0.06, "scene": 0.18, "volume": 0.17}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "scene", "volume"])
def test_denoised_frame_is_closer_to_the_converged_one(bendy, name):
    """128x128: colour and the three guides at 4 spp from the library's own AOV outputs; ground truth 1024 spp."""
    w = h = 128
    color, _, _ = gpu_render(bendy, name, w, h, 4)
    guides = [gpu_render(bendy, name, w, h, 4, output=o)[0] for o in (1, 2, 3)]
    truth, _, _ = gpu_render(bendy, name, w, h, 1024)
    den = bendy.denoise(color, *guides)
    y = truth.mean()
    noisy, filtered = _rel_mse(color.mean(), y), _rel_mse(den.numpy()[..., :3], y)
    ratio = filtered / noisy
    print(f"[denoise quality] {name}: relMSE noisy {noisy:.5f} denoised {filtered:.5f} ratio {ratio:.4f}")
    assert den.samples == 1 and den.color_space == color.color_space
    assert ratio <= QUALITY_BOUND[name], (noisy, filtered, ratio)


@pytest.mark.gpu
def test_denoise_is_deterministic_and_leaves_renders_alone(bendy):
    import torch
    w, h = 96, 64
    sc, cam = gpu_scene(bendy, "scene", w, h)
    tr = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4))
    rcfg = bendy.RenderConfig.with_samples(2)

    def render(output=bendy.Output.Full, device="cuda"):
        b = bendy.Buffer.new(w, h, device=device)
        t = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4, output=output))
        t.render(sc, cam, rcfg, b, seed=5)
        torch.cuda.synchronize()
        return b
    before = render().numpy().copy()
    color = render()
    guides = [render(o) for o in (bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth)]
    a = bendy.denoise(color, *guides).numpy().copy()
    dn = bendy.Denoiser()
    b = dn.denoise(color, *guides)
    torch.cuda.synchronize()
    assert np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32))
    # host path == device path
    cpu = [_cpu_buffer(bendy, x.numpy(), x.samples) for x in [color] + guides]
    c = dn.denoise(*cpu)
    assert c.device == "cpu" and c.samples == 1
    assert np.array_equal(a.view(np.uint32), c.numpy().view(np.uint32))
    # the inputs are untouched and renders on the scene handle are bit-identical afterwards
    assert np.array_equal(color.numpy(), before)
    after = render().numpy()
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    # a denoise into a caller's buffer on another device is refused
    with pytest.raises(bendy.BendyError):
        dn.denoise(color, cpu[1])
    dn.close()


@pytest.mark.gpu
def test_cli_denoise_equals_library(bendy, tmp_path):
    """--denoise: the screenshot is denoise(progressive colour, 4-sample guides) previewed with samples = 1."""
    import torch
    from test_cli_io import read_png
    w, h, samples, sub, seed = 96, 64, 8, 2, 31
    shot = tmp_path / "dn.png"
    r = subprocess.run([CLI, "--output", "full", "--width", str(w), "--height", str(h), "--samples", str(samples),
                        "--subsample", str(sub), "--screenshot", str(shot), "--scene", scene_path("scene"), "--seed",
                        str(seed), "--denoise", "--quiet"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "denoised with guides of 16 samples" in r.stderr
    sc, cam = gpu_scene(bendy, "scene", w, h)
    color = bendy.Buffer.new(w, h, bendy.ColorSpace.SRgb)
    tr = bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4))
    while color.samples < samples:
        tr.render(sc, cam, bendy.RenderConfig.with_samples_subsample(1, bendy.Subsample(sub)), color, seed=seed)
    guides = []
    for o in (bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth):
        g = bendy.Buffer.new(w, h)
        bendy.Tracer.with_config(bendy.Config(chunks_x=8, chunks_y=4, output=o)).render(
            sc, cam, bendy.RenderConfig.with_samples_subsample(4, bendy.Subsample(sub)), g, seed=seed)
        guides.append(g)
    den = bendy.denoise(color, *guides)
    torch.cuda.synchronize()
    assert np.array_equal(read_png(shot), den.preview())
    r = subprocess.run([CLI, "--output", "albedo", "--denoise"], capture_output=True, text=True)
    assert r.returncode != 0 and "--denoise needs --output full" in r.stderr
