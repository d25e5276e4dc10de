"""rt_denoise: the edge-avoiding à-trous filter guided by the first-hit AOVs.  The device output is compared bit for bit with the
C restatement of the header's arithmetic (tests/denoise_reference.py), on rendered frames of every kind and on shapes and settings
at the edges of the contract; the reference itself is checked for what the filter promises on synthetic images; and the filter is
held to a fixed quality bar against a 1024-spp ground truth (renders are bit-exact, so the numbers are deterministic)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as dr
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = 1 << 32          # a device address that is never dereferenced: every check comes before any HIP call


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} values differ (first at {np.argwhere(bad)[0]})"


# ---- no GPU needed -----------------------------------------------------------------------------------------------------

def test_params_mirror_and_init():
    assert C.sizeof(rb.DenoiseParams) == 20
    assert [rb.DenoiseParams.__dict__[f].offset for f in ("iterations", "sigma_depth", "sigma_luminance", "normal_squarings")] == [4, 8, 12, 16]
    p = rb.DenoiseParams()
    p.struct_bytes, p.iterations, p.normal_squarings = 3, 99, -4
    rb.amd_lib().rt_denoise_params_init(C.byref(p))
    assert (p.struct_bytes, p.iterations, p.sigma_depth, p.sigma_luminance, p.normal_squarings) == (20, 5, 1.0, 4.0, 7)
    q = rb.denoise_params(iterations=2, sigma_luminance=2.5)
    assert (q.iterations, q.sigma_depth, q.sigma_luminance, q.normal_squarings) == (2, 1.0, 2.5, 7)
    with pytest.raises(TypeError):
        rb.denoise_params(sigma=1.0)
    lib = rb.amd_lib()
    assert all(hasattr(lib, s) for s in ("rt_denoise", "rt_denoise_params_init", "rt_denoise_workspace_bytes"))


def test_workspace_bytes_grow_with_the_image():
    lib = rb.amd_lib()
    assert lib.rt_denoise_workspace_bytes(0, 5) == 0 and lib.rt_denoise_workspace_bytes(5, -1) == 0
    sizes = [(1, 1), (1, 2), (3, 1), (2, 2), (77, 45), (45, 78), (320, 180), (1920, 1080), (3840, 2160), (4096, 4096), (1 << 24, 1)]
    got = [lib.rt_denoise_workspace_bytes(w, h) for w, h in sizes]
    assert all(b >= 64 * w * h for b, (w, h) in zip(got, sizes))
    px = [w * h for w, h in sizes]
    assert all((a < b) if pa < pb else (a == b) for a, b, pa, pb in zip(got, got[1:], px, px[1:]))
    assert got[-1] == got[-2] == lib.rt_denoise_workspace_bytes(1, 1 << 24)


def _call(fb=FAKE, aov="full", width=8, height=4, spp=4, params=None, ws=None, ws_bytes=None, out=None):
    lib = rb.amd_lib()
    b = None
    if aov == "full":
        b = rb.AovBuffers()
        b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count = 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE
    elif aov is not None:
        b = aov
    ws = 6 * FAKE if ws is None else ws
    ws_bytes = lib.rt_denoise_workspace_bytes(width, height) if ws_bytes is None else ws_bytes
    out = 7 * FAKE if out is None else out
    st = lib.rt_denoise(C.c_void_p(fb), C.byref(b) if b is not None else None, width, height, spp, C.byref(params) if params else None,
                        C.c_void_p(ws), ws_bytes, C.c_void_p(out), None)
    return st, lib.rt_get_last_error_string().decode()


def test_invalid_arguments_and_limits_without_a_device():
    lib = rb.amd_lib()
    invalid, unsupported = 1, 4
    cases = [dict(fb=0), dict(aov=None), dict(ws=0), dict(out=0), dict(width=0), dict(height=-3), dict(spp=0), dict(spp=65537),
             dict(ws_bytes=lib.rt_denoise_workspace_bytes(8, 4) - 1), dict(out=2 * FAKE + 12), dict(out=6 * FAKE + 100),
             dict(out=FAKE - 8 * 4 * 12 + 4), dict(out=5 * FAKE + 124), dict(ws=FAKE + 64)]
    for field in ("albedo_sum", "normal_sum", "depth_sum", "hit_count"):
        b = rb.AovBuffers()
        b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count = 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE
        setattr(b, field, None)
        cases.append(dict(aov=b))
    short = rb.AovBuffers()
    short.albedo_sum, short.normal_sum, short.depth_sum, short.hit_count = 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE
    short.struct_bytes = 32                                           # hit_count lies past struct_bytes: it counts as NULL
    cases.append(dict(aov=short))
    for field, bad in (("iterations", -1), ("iterations", 9), ("sigma_depth", 0.0), ("sigma_depth", -1.0), ("sigma_depth", float("inf")),
                       ("sigma_depth", float("nan")), ("sigma_luminance", 0.0), ("sigma_luminance", float("inf")),
                       ("normal_squarings", -1), ("normal_squarings", 11), ("struct_bytes", 4)):
        p = rb.denoise_params()
        setattr(p, field, bad)
        cases.append(dict(params=p))
    for kw in cases:
        lib.rt_get_last_error_string()
        st, msg = _call(**kw)
        assert st == invalid and msg.startswith("rt_denoise:"), (kw, st, msg)
    for w, h in ((4097, 4096), (1 << 24, 2), (1, (1 << 24) + 1)):
        st, msg = _call(width=w, height=h)
        assert st == unsupported and "2^24" in msg, (w, h, st, msg)
    # the edges that are allowed pass their check and fail a later one (nothing here may reach a launch: the addresses are fake)
    older = rb.DenoiseParams()
    older.struct_bytes, older.iterations = 8, 0                      # a shorter struct: the other fields keep their defaults
    short_ws = lib.rt_denoise_workspace_bytes(8, 4) - 1
    for kw in (dict(spp=65536), dict(spp=1), dict(params=older), dict(params=rb.denoise_params(iterations=8, normal_squarings=10, sigma_depth=1e-30)),
               dict(params=rb.denoise_params(iterations=0, normal_squarings=0)), dict(width=4096, height=4096, ws_bytes=64 << 24)):
        st, msg = _call(ws_bytes=kw.pop("ws_bytes", short_ws), **kw)
        assert st == invalid and "workspace_bytes" in msg, (kw, st, msg)
    for out in (2 * FAKE + 8 * 4 * 12, FAKE - 8 * 4 * 12):            # d_out right after / right before an input
        st, msg = _call(out=out, ws=5 * FAKE + 64)
        assert st == invalid and "the workspace overlaps an input" in msg, (out, st, msg)


def test_cli_denoise_refuses_the_multi_gpu_drivers(test_config_text):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    for extra in (["--devices", "1"], ["--shard", "1"]):
        out = subprocess.run([exe, "--gpu", "--denoise"] + extra, input=test_config_text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--denoise" in out.stderr, (extra, out.returncode, out.stderr)
    out = subprocess.run([exe, "--gpu", "--denoise"], input=test_config_text, capture_output=True, text=True, timeout=120,
                         env={**os.environ, "RTP_DEVICES": "2"})
    assert out.returncode == 2 and "--denoise" in out.stderr, (out.returncode, out.stderr)


def _flat_scene(w, h, spp, albedo, illumination, normal=(0.0, 0.0, 1.0), depth=5.0):
    """Synthetic sums of a frame whose every sample hits: fb = albedo * illumination per sample."""
    s = np.float32(spp)
    a = np.broadcast_to(np.asarray(albedo, np.float32), (h, w, 3)).astype(np.float32)
    aov = {"albedo": a * s, "normal": np.broadcast_to(np.asarray(normal, np.float32) * s, (h, w, 3)).copy(),
           "depth": np.full((h, w), depth * spp, np.float32), "hits": np.full((h, w), spp, np.uint32)}
    return (a * np.asarray(illumination, np.float32) * s).astype(np.float32), aov


def test_reference_keeps_texture_under_constant_light():
    h, w, spp = 24, 40, 16
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.where(((xx // 3) + (yy // 3)) % 2 == 0, 0.8, 0.05).astype(np.float32)[..., None] * np.array([1.0, 0.7, 0.4], np.float32)
    fb, aov = _flat_scene(w, h, spp, checker, 0.6)
    for it in (1, 5, 8):
        out = dr.reference(fb, aov, spp, iterations=it)
        assert np.abs(out / fb - 1).max() < 1e-6, it


def test_reference_does_not_leak_across_opposite_normals():
    h, w, spp = 32, 48, 8
    rng = np.random.default_rng(5)
    light = np.full((h, w, 1), 0.5, np.float32)
    light[:, : w // 2, 0] = rng.exponential(5.0, (h, w // 2)).astype(np.float32)          # heavy noise on the left half only
    normal = np.zeros((h, w, 3), np.float32)
    normal[:, : w // 2, 0], normal[:, w // 2:, 0] = 1.0, -1.0
    fb, aov = _flat_scene(w, h, spp, 0.5, light)
    aov["normal"] = normal * np.float32(spp)
    out = dr.reference(fb, aov, spp)
    right, left = out[:, w // 2:] / fb[:, w // 2:], out[:, : w // 2] / np.float32(0.5 * spp)
    assert np.abs(right - 1).max() < 1e-5
    assert left.std() < 0.5 * (fb[:, : w // 2] / np.float32(0.5 * spp)).std()          # the noisy half was filtered
    # sky pixels pass through bit for bit, whatever they hold, and take no part in their neighbours' filter
    sky = aov["hits"].copy()
    sky[::5, ::3] = 0
    fb2 = fb.copy()
    fb2[sky == 0] = rng.uniform(-1e6, 1e6, ((sky == 0).sum(), 3)).astype(np.float32)
    out2 = dr.reference(fb2, {**aov, "hits": sky}, spp)
    assert_same(out2[sky == 0], fb2[sky == 0], "sky pixels")
    fb3 = fb.copy()
    fb3[sky == 0] = 0
    assert_same(dr.reference(fb3, {**aov, "hits": sky}, spp)[sky > 0], out2[sky > 0], "sky values do not reach hit pixels")


# ---- on the GPU --------------------------------------------------------------------------------------------------------

def _frame(host, cam):
    dev = rb.DeviceScene(host, device=0)
    fb, _ = dev.render_to_host(cam)
    aov, _ = dev.render_aov_to_host(cam)
    dev.close()
    return fb, aov


def _check(fb, aov, spp, what, **params):
    got = rb.denoise_to_host(fb, aov, spp, **params)
    assert_same(got, dr.reference(fb, aov, spp, **params), f"{what} {params}")
    return got


@pytest.mark.gpu
def test_rtiow_odd_size_every_iteration_count_and_setting():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(77, 45, 8, 50)
    fb, aov = _frame(host, cam)
    assert (aov["hits"] == 0).any() and (aov["hits"] > 0).any()
    for it in range(9):
        got = _check(fb, aov, 8, "rtiow 77x45", iterations=it)
        assert_same(got[aov["hits"] == 0], fb[aov["hits"] == 0], "sky pixels")
    for params in (dict(sigma_depth=0.25), dict(sigma_luminance=0.5, normal_squarings=0), dict(sigma_depth=7.5, normal_squarings=10),
                   dict(iterations=3, sigma_luminance=40.0, normal_squarings=2)):
        _check(fb, aov, 8, "rtiow 77x45", **params)
    # one-pixel-wide images: a column and a row of the frame, each an image of its own
    col = {k: np.ascontiguousarray(v[:, 30:31]) for k, v in aov.items()}
    row = {k: np.ascontiguousarray(v[22:23, :]) for k, v in aov.items()}
    _check(np.ascontiguousarray(fb[:, 30:31]), col, 8, "45x1 column")
    _check(np.ascontiguousarray(fb[22:23, :]), row, 8, "1x77 row", iterations=8)
    _check(fb[22:23, 40:41].copy(), {k: np.ascontiguousarray(v[22:23, 40:41]) for k, v in aov.items()}, 8, "1x1")


@pytest.mark.gpu
def test_config_scene_with_its_jpeg_floor(test_config_text):
    rb.amd_lib().rt_set_device(0)
    text = test_config_text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    assert host.desc.num_textures == 1
    cam = host.frame_camera(0)
    fb, aov = _frame(host, cam)
    _check(fb, aov, cam.samples_per_pixel, "config scene")


@pytest.mark.gpu
def test_array_scene_with_every_material_and_plane_type():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow(half_extent=2, textured_quad=True, texture_size=64)
    desc = host.desc
    mats = desc.materials
    diffuse = [k for k in range(desc.num_materials) if mats[k].type == 0]
    mats[diffuse[1]].type = 3
    mats[diffuse[1]].emit.e[:] = (4.0, 3.0, 2.0)
    for k in diffuse[2:30]:
        mats[k].texture_id = 1
    assert {mats[k].type for k in range(desc.num_materials)} == {0, 1, 2, 3}
    cam = rb.make_camera(160, 100, 45.0, (3.5, 1.6, 1.8), (0, 0, 0.2), (0.6, 0.7, 0.9), 5, 12)
    for ptype in (0, 1, 2):
        desc.planes[0].type = ptype
        fb, aov = _frame(host, cam)
        _check(fb, aov, 5, f"plane type {ptype}")


@pytest.mark.gpu
def test_all_sky_frame_and_the_headline_frame():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    sky = rb.make_camera(120, 80, 20.0, (13, 3, 2), (26, 6, 40), (0.3, 0.5, 0.9), 3, 50)
    fb, aov = _frame(host, sky)
    assert not aov["hits"].any()
    assert_same(_check(fb, aov, 3, "all sky"), fb, "all sky passes through")
    cam = rb.rtiow_camera(1920, 1080, 4, 50)
    fb, aov = _frame(host, cam)
    _check(fb, aov, 4, "1920x1080 headline camera")


@pytest.mark.gpu
def test_enqueued_on_a_side_stream():
    import torch
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(200, 120, 8, 50)
    fb, aov = _frame(host, cam)
    want = dr.reference(fb, aov, 8, iterations=4)
    t = {"fb": torch.from_numpy(fb).to("cuda:0")}
    for key in ("albedo", "normal", "depth"):
        t[key] = torch.from_numpy(aov[key]).to("cuda:0")
    t["hits"] = torch.from_numpy(aov["hits"].view(np.int32)).to("cuda:0")
    out = torch.full_like(t["fb"], float("nan"))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rb.denoise(t["fb"].data_ptr(), {k: t[k].data_ptr() for k in ("albedo", "normal", "depth", "hits")}, 200, 120, 8, out.data_ptr(),
                   stream=stream.cuda_stream, iterations=4)
    stream.synchronize()
    assert_same(out.cpu().numpy(), want, "side stream")


def _mse(fb, spp, truth):
    return float(np.mean((np.clip(fb / np.float32(spp), 0, 1) - truth) ** 2))


@pytest.mark.gpu
def test_quality_against_a_1024_spp_ground_truth():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    fb8, aov8 = _frame(host, rb.rtiow_camera(320, 180, 8, 50))
    fbgt, aovgt = _frame(host, rb.rtiow_camera(320, 180, 1024, 50))
    truth = np.clip(fbgt / np.float32(1024), 0, 1)
    noisy = _mse(fb8, 8, truth)
    denoised = _mse(rb.denoise_to_host(fb8, aov8, 8), 8, truth)
    moved = _mse(rb.denoise_to_host(fbgt, aovgt, 1024), 1024, truth)
    print(f"quality: noisy MSE {noisy:.6g}, denoised {denoised:.6g} (ratio {denoised / noisy:.4f}), 1024 spp moved by {moved:.6g} "
          f"({moved / noisy:.4f} of the noisy MSE)")
    assert denoised <= 0.4 * noisy          # measured 0.314
    assert moved < 0.1 * noisy


@pytest.mark.gpu
def test_cli_writes_the_reference_denoised_file(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines)
    out = subprocess.run([exe, "--gpu", "--denoise", "--aov"], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.from_config(text)
    cam = host.frame_camera(0)
    fb, aov = _frame(host, cam)
    want = dr.reference(fb, aov, cam.samples_per_pixel)
    data = open(tmp_path / "f_0.png.denoised", "rb").read()
    assert data == rb.binary_image_bytes(want, cam.image_width, cam.image_height, host.info.sqrt_spp)
    assert os.path.exists(tmp_path / "f_0.png.aov")
