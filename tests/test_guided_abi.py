"""bt_render_guided_device / Tracer.render_guided / --denoise-inline (EXTENSION): what is decided before the
device is touched.  Runs without a GPU; the pointers handed to the library here are dummies that a refused call never
dereferences."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT, scene_path

CLI = os.path.join(ROOT, "bendy_tracer_amd", "bendy-tracer-hip")
INVALID_ARG, DEVICE, UNSUPPORTED, DONE = -1, -8, -9, 0
# four distinct non-NULL "device" addresses: colour, albedo, normal, depth
FRAMES = [0x1000, 0x2000, 0x3000, 0x4000]


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _setup(bendy, samples=2, output=0, render_output=None):
    from bendy_tracer_amd import api
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    rcfg = bendy.RenderConfig(samples=samples, output=None if render_output is None else bendy.Output(render_output))
    c, r = api._c_configs(bendy.Config(output=bendy.Output(output)), rcfg, 0)
    return api, sc, cam, c, r


def _call(api, sc, cam, c, r, frames=FRAMES, scene=True, w=32, h=16):
    fr = [C.c_void_p(f) if f else None for f in frames]
    return api.lib.bt_render_guided_device(sc._h if scene else None, cam, C.byref(c) if c is not None else None,
                                           C.byref(r) if r is not None else None, *fr, w, h, 1, None)


def test_symbol_is_declared_and_exported(bendy):
    from bendy_tracer_amd import api
    assert "bt_render_guided_device" in api.EXPORTS
    assert hasattr(api.lib, "bt_render_guided_device")
    hdr = open(os.path.join(ROOT, "include", "bendy_hip.h")).read()
    assert "int bt_render_guided_device(" in hdr and "EXTENSION -- NOT IN THE REFERENCE" in hdr


def test_null_arguments_are_refused_first(bendy):
    api, sc, cam, c, r = _setup(bendy)
    assert _call(api, sc, cam, c, r, scene=False) == INVALID_ARG
    assert _call(api, sc, cam, None, r) == INVALID_ARG
    assert _call(api, sc, cam, c, None) == INVALID_ARG
    assert _call(api, sc, cam, c, r, frames=[0] + FRAMES[1:]) == INVALID_ARG
    # ... ahead of everything else: a lens, a wrong output and samples == 0 do not change the verdict
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    r.samples = 0
    c.output = 1
    assert _call(api, sc, cam, c, r, frames=[0] + FRAMES[1:]) == INVALID_ARG


@pytest.mark.parametrize("output", [1, 2, 3])
def test_effective_output_must_be_full(bendy, output):
    api, sc, cam, c, r = _setup(bendy, output=output)                        # Config.output
    assert _call(api, sc, cam, c, r) == INVALID_ARG
    assert b"output" in api.lib.bt_last_error()
    api, sc, cam, c, r = _setup(bendy, output=0, render_output=output)       # RenderConfig.output overrides it (mod.rs:220)
    assert _call(api, sc, cam, c, r) == INVALID_ARG
    api, sc, cam, c, r = _setup(bendy, output=output, render_output=0)       # ... in both directions
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    assert _call(api, sc, cam, c, r) == UNSUPPORTED                          # (valid output: the next test in the list decides)
    # ahead of the lens and of samples == 0
    api, sc, cam, c, r = _setup(bendy, samples=0, output=output)
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    assert _call(api, sc, cam, c, r) == INVALID_ARG


@pytest.mark.parametrize("i,j", [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)])
def test_two_frames_must_not_be_the_same(bendy, i, j):
    api, sc, cam, c, r = _setup(bendy, samples=0)
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)                              # (neither the lens nor samples == 0 comes first)
    frames = list(FRAMES)
    frames[j] = frames[i]
    assert _call(api, sc, cam, c, r, frames=frames) == INVALID_ARG
    assert b"same" in api.lib.bt_last_error()


def test_lens_is_unsupported_then_zero_samples_is_done(bendy):
    api, sc, cam, c, r = _setup(bendy, samples=0)
    sc.set_lens((0.0, 0.0, 0.0), 0.1, 0.1, 2.0)
    assert _call(api, sc, cam, c, r) == UNSUPPORTED                          # ahead of samples == 0
    assert _call(api, sc, cam, c, r, frames=[FRAMES[0], 0, 0, 0]) == UNSUPPORTED   # ... also without any guide
    sc.clear_lens()
    assert _call(api, sc, cam, c, r) == DONE                                 # mod.rs:186-188; the device is not needed for it
    assert _call(api, sc, cam, c, r, frames=[FRAMES[0], 0, FRAMES[2], 0]) == DONE


def test_valid_call_without_a_device_is_a_device_error(bendy):
    if _have_gpu():
        pytest.skip("a GPU is present")            # (the dummy frames would be written to)
    api, sc, cam, c, r = _setup(bendy)
    assert _call(api, sc, cam, c, r) == DEVICE
    assert _call(api, sc, cam, c, r, frames=[FRAMES[0], 0, 0, 0]) == DEVICE


class _FakeDeviceData:
    """Stands in for a torch tensor in HBM where none can exist: render_guided's own checks come before any use of it."""
    def data_ptr(self):
        raise AssertionError("a refused call must not reach the library")


def _fake_gpu_buffer(bendy, w, h):
    b = bendy.Buffer.new(w, h, device="cpu")
    b.device = "cuda"
    b.data = _FakeDeviceData()
    return b


def test_python_method_refuses_cpu_buffers_sizes_and_outputs(bendy):
    sc = bendy.Scene.load(scene_path("scene"))
    cam = sc.find_by_tag("camera")
    tr = bendy.Tracer.new()
    rcfg = bendy.RenderConfig.with_samples(1)
    cpu = [bendy.Buffer.new(16, 8, device="cpu") for _ in range(4)]
    with pytest.raises(bendy.BendyError) as e:
        tr.render_guided(sc, cam, rcfg, *cpu)
    assert e.value.code == INVALID_ARG
    gpu = [_fake_gpu_buffer(bendy, 16, 8) for _ in range(4)]
    with pytest.raises(bendy.BendyError) as e:                               # one guide on the host
        tr.render_guided(sc, cam, rcfg, gpu[0], gpu[1], cpu[2], gpu[3])
    assert e.value.code == INVALID_ARG
    with pytest.raises(bendy.BendyError) as e:                               # a guide of another size
        tr.render_guided(sc, cam, rcfg, gpu[0], depth=_fake_gpu_buffer(bendy, 16, 9))
    assert e.value.code == INVALID_ARG
    for out in (bendy.Output.Albedo, bendy.Output.Normal, bendy.Output.Depth):
        with pytest.raises(bendy.BendyError) as e:                           # Config.output
            bendy.Tracer.with_config(bendy.Config(output=out)).render_guided(sc, cam, rcfg, *gpu)
        assert e.value.code == INVALID_ARG
        with pytest.raises(bendy.BendyError) as e:                           # RenderConfig.output
            tr.render_guided(sc, cam, bendy.RenderConfig(samples=1, output=out), *gpu)
        assert e.value.code == INVALID_ARG
    assert all(b.samples == 0 for b in cpu + gpu)


def _cli(*extra):
    return subprocess.run([CLI, "--width", "16", "--height", "16", "--samples", "1", "--denoise-inline", *extra],
                          capture_output=True, text=True, timeout=60)


def test_cli_refuses_denoise_inline_combinations():
    r = _cli("--output", "albedo")
    assert r.returncode != 0 and "--denoise-inline needs --output full" in r.stderr
    r = _cli("--output", "full", "--denoise")
    assert r.returncode != 0 and "--denoise-inline and --denoise" in r.stderr
    r = _cli("--output", "full", "--lens", "0,0,0,0.1,0.1,2")
    assert r.returncode != 0 and "--denoise-inline" in r.stderr and "--lens" in r.stderr
    r = _cli("--output", "full", "--shard", "0,2")
    assert r.returncode != 0 and "--denoise-inline" in r.stderr and "--shard" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--denoise-inline" in r.stderr
