"""First-hit AOVs (rt_render_aov / rt_render_aov_tile): albedo, normal, depth, hit count and primitive id per pixel, bit for bit
against the CPU reference of tests/aov_reference.py (the oracle's get_ray, hit_bvh and tex2D_cpu), on every path a handle
resolves camera rays by — the per-pixel candidate lists with the primary pass, their undecided samples re-walked, and the
reference-order walk alone — and without changing a single decision of the handle's beauty frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_reference as ar
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = ("albedo", "normal", "depth", "hits", "prim")


def assert_same_aovs(got, want, what):
    for k in KEYS:
        g = np.ascontiguousarray(got[k]).view(np.uint32)
        w = np.ascontiguousarray(want[k]).view(np.uint32)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = g != w
        assert not bad.any(), f"{what}: {k} differs in {bad.sum()} of {bad.size} values (first at {np.argwhere(bad)[0]})"


# ---- no GPU needed -----------------------------------------------------------------------------------------------------

def test_aov_buffers_mirror_and_init():
    lib = rb.amd_lib()
    assert C.sizeof(rb.AovBuffers) == 48
    assert [rb.AovBuffers.__dict__[f].offset for f in ("albedo_sum", "normal_sum", "depth_sum", "hit_count", "first_prim")] == [8, 16, 24, 32, 40]
    b = rb.AovBuffers()
    b.struct_bytes, b.albedo_sum, b.first_prim = 7, 1234, 5678
    lib.rt_aov_buffers_init(C.byref(b))
    assert b.struct_bytes == 48 and not any((b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count, b.first_prim))
    assert b"rtp_amd 0.5 gfx950" in lib.rt_version_string()


def test_aov_invalid_arguments():
    lib = rb.amd_lib()
    cam = rb.rtiow_camera(8, 8, 1)
    b = rb.AovBuffers()
    assert lib.rt_render_aov(None, C.byref(cam), None, C.byref(b), None, 1, None) == 1            # every buffer NULL
    assert b"every AOV buffer is NULL" in lib.rt_get_last_error_string()
    assert lib.rt_render_aov_tile(None, C.byref(cam), 0, 0, 4, 4, C.byref(b), None, 1, None) == 1
    assert b"every AOV buffer is NULL" in lib.rt_get_last_error_string()
    assert lib.rt_render_aov(None, C.byref(cam), None, None, None, 1, None) == 1                    # no buffer struct
    b.depth_sum = 4096
    b.struct_bytes = 8                                                                              # shorter than any pointer
    assert lib.rt_render_aov(None, C.byref(cam), None, C.byref(b), None, 1, None) == 1
    b.struct_bytes = C.sizeof(rb.AovBuffers)
    assert lib.rt_render_aov(None, C.byref(cam), None, C.byref(b), None, 1, None) == 1            # null scene
    assert b"null scene" in lib.rt_get_last_error_string()
    assert lib.rt_render_aov_tile(None, C.byref(cam), 0, 0, 4, 4, C.byref(b), None, 1, None) == 1
    assert b"null scene" in lib.rt_get_last_error_string()


def aov_file_bytes(aov, width, height, spp):
    """What rtp_main --gpu --aov writes for a frame: int32 width, height, spp, then 8 float32 per pixel (float32 divisions)."""
    n = np.float32(spp)
    hits = aov["hits"].reshape(-1).astype(np.float32)
    rec = np.zeros((width * height, 8), np.float32)
    rec[:, 0:3] = aov["albedo"].reshape(-1, 3) / n
    rec[:, 3:6] = aov["normal"].reshape(-1, 3) / n
    depth = aov["depth"].reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rec[:, 6] = np.where(hits > 0, depth / np.where(hits > 0, hits, np.float32(1)), np.float32(0))
    rec[:, 7] = hits / n
    return np.array([width, height, spp], np.int32).tobytes() + rec.tobytes()


def test_aov_file_layout(tmp_path):
    """The .aov file of rtp_main --gpu --aov (host/camera.cpp, write_aov_file) written from a synthetic buffer."""
    rng = np.random.default_rng(3)
    w, h, spp = 7, 5, 13
    aov = {"albedo": rng.uniform(0, 13, (h, w, 3)).astype(np.float32), "normal": rng.uniform(-13, 13, (h, w, 3)).astype(np.float32),
           "depth": rng.uniform(0, 300, (h, w)).astype(np.float32), "hits": rng.integers(0, spp + 1, (h, w)).astype(np.uint32)}
    aov["hits"][0, :3] = 0
    path = str(tmp_path / "f.aov")
    hl = rb.host_lib()
    hl.rtp_host_write_aov.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert hl.rtp_host_write_aov(path.encode(), w, h, spp, aov["albedo"].ctypes.data, aov["normal"].ctypes.data, aov["depth"].ctypes.data,
                                 aov["hits"].ctypes.data) == 0
    data = open(path, "rb").read()
    assert len(data) == 12 + 32 * w * h
    assert data == aov_file_bytes(aov, w, h, spp)
    rec = np.frombuffer(data[12:], np.float32).reshape(h, w, 8)
    assert (rec[0, :3, 6] == 0).all()


def test_cli_aov_refuses_the_multi_gpu_drivers(test_config_text):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    for extra in (["--devices", "1"], ["--shard", "1"]):
        out = subprocess.run([exe, "--gpu", "--aov"] + extra, input=test_config_text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "--aov" in out.stderr, (extra, out.returncode, out.stderr)


# ---- on the GPU --------------------------------------------------------------------------------------------------------

def _material(mtype, albedo=(0, 0, 0), fuzz=0.0, ir=1.0, emit=(0, 0, 0)):
    m = rb.Material()
    m.type, m.fuzz, m.ir = mtype, fuzz, ir
    m.albedo.e[:] = albedo
    m.emit.e[:] = emit
    return m


@pytest.mark.gpu
def test_small_rtiow_frame_on_every_resolve_path():
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(160, 90, 6, 50)
    want = ar.reference(host, cam)
    dev = rb.DeviceScene(host, device=0)
    got, t = dev.render_aov_to_host(cam)
    assert t.primary_visibility == 1 and t.kernel_ms > 0 and t.primary_ms > 0 and 0 < t.traced_samples <= 160 * 90 * 6
    assert t.guarded == 0 and t.trace_launches == 0 and t.trace_ms == 0
    assert_same_aovs(got, want, "candidate lists")
    assert (want["hits"] > 0).any() and len(np.unique(want["prim"])) > 20
    dev.configure(primary_visibility=-1)
    got, t = dev.render_aov_to_host(cam)
    assert t.primary_visibility == 0 and t.flagged_samples == 160 * 90 * 6 and t.rework_ms > 0
    assert_same_aovs(got, want, "primary_visibility = -1")
    dev.configure(primary_visibility=0, traversal=rb.TRAVERSAL_EXACT)
    got, t = dev.render_aov_to_host(cam)
    assert t.primary_visibility == 0
    assert_same_aovs(got, want, "exact walk")


@pytest.mark.gpu
def test_config_scene_with_its_jpeg_floor(test_config_text):
    text = test_config_text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    assert host.desc.num_textures == 1 and host.desc.materials[0].texture_id == 1
    cam = host.frame_camera(0)
    dev = rb.DeviceScene(host, device=0)
    got, _ = dev.render_aov_to_host(cam)
    want = ar.reference(host, cam)
    assert_same_aovs(got, want, "config scene")
    assert len(np.unique(want["albedo"].reshape(-1, 3), axis=0)) > 100          # the texture shows


@pytest.mark.gpu
def test_array_scene_with_every_material_texture_and_plane_type():
    """All four material types, a textured sphere and a textured quad, then the same plane as an ellipse and a triangle."""
    host = rb.HostScene.rtiow(half_extent=2, textured_quad=True, texture_size=64)
    desc = host.desc
    mats = desc.materials
    diffuse = [k for k in range(desc.num_materials) if mats[k].type == 0]
    mats[diffuse[1]].type = 3
    mats[diffuse[1]].emit.e[:] = (4.0, 3.0, 2.0)
    for k in diffuse[2:30]:
        mats[k].texture_id = 1
    present = {mats[k].type for k in range(desc.num_materials)}
    assert present == {0, 1, 2, 3}
    cam = rb.make_camera(160, 100, 45.0, (3.5, 1.6, 1.8), (0, 0, 0.2), (0.6, 0.7, 0.9), 5, 12)
    for ptype in (0, 1, 2):            # QUAD, ELLIPSE, TRIANGLE
        desc.planes[0].type = ptype
        dev = rb.DeviceScene(host, device=0)
        got, t = dev.render_aov_to_host(cam)
        assert_same_aovs(got, ar.reference(host, cam), f"plane type {ptype}")
        dev.close()


@pytest.mark.gpu
def test_flagged_and_small_scenes():
    import test_gpu_parity as tgp
    host, cam, n = tgp._stress_scene(9, 4, 8, 320, 180)
    assert n == 325
    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
    _, tb = dev.render_to_host(cam)          # (the beauty frame re-packs the guarded tree for this camera; the AOV call uses it)
    assert tb.primary_visibility == 1
    got, t = dev.render_aov_to_host(cam)
    assert t.primary_visibility == 1 and t.flagged_samples > 0, (t.primary_visibility, t.flagged_samples)
    assert_same_aovs(got, ar.reference(host, cam), "heavily flagged scene")
    # under 64 primitives: the exact walk only
    rng = np.random.default_rng(11)
    sph = np.zeros((30, 5), np.float32)
    sph[:, :3] = rng.uniform(-3, 3, (30, 3))
    sph[:, 3] = rng.uniform(0.2, 0.9, 30)
    sph[:, 4] = rng.integers(0, 4, 30)
    small = rb.HostScene.from_arrays(sph, np.zeros((0, 11), np.float32),
                                     [_material(0, (0.7, 0.2, 0.1)), _material(1, (0.5, 0.6, 0.7), 0.2), _material(2, ir=1.5),
                                      _material(3, emit=(2, 2, 2))])
    scam = rb.make_camera(96, 64, 50.0, (9, 4, 3), (0, 0, 0), (0.2, 0.3, 0.4), 7, 10)
    d = rb.DeviceScene(small, device=0)
    got, t = d.render_aov_to_host(scam)
    assert t.primary_visibility == 0 and t.flagged_samples == 96 * 64 * 7
    assert_same_aovs(got, ar.reference(small, scam), "30 spheres")


@pytest.mark.gpu
def test_shards_tiles_passes_and_sky():
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(150, 97, 5, 50)
    want = ar.reference(host, cam)
    dev = rb.DeviceScene(host, device=0)
    whole, _ = dev.render_aov_to_host(cam)
    assert_same_aovs(whole, want, "whole frame")
    for p in range(3):
        shard = rb.Shard(8, 3, p)
        got, _ = dev.render_aov_to_host(cam, shard=shard)
        rows = ar.image_rows(cam, shard)
        assert_same_aovs(got, {k: v[rows] for k, v in want.items()}, f"shard {{8, 3, {p}}}")
    for x0, y0, w, h in ((0, 0, 61, 33), (61, 0, 89, 33), (0, 33, 150, 64), (149, 96, 1, 1), (17, 40, 77, 3)):
        got, _ = dev.render_aov_to_host(cam, tile=(x0, y0, w, h))
        assert_same_aovs(got, {k: v[y0:y0 + h, x0:x0 + w] for k, v in want.items()}, f"tile {x0},{y0} {w}x{h}")
    dev.configure(pass_spp=2)              # three passes: the sums go on across them
    got, _ = dev.render_aov_to_host(cam)
    assert_same_aovs(got, want, "pass_spp = 2")
    dev.configure(pass_spp=2, primary_visibility=-1)
    got, _ = dev.render_aov_to_host(cam)
    assert_same_aovs(got, want, "pass_spp = 2 without lists")
    # views with a non-zero background: more than half of the samples miss, and nothing but sky
    dev.configure(pass_spp=0, primary_visibility=0)
    for what, target in (("mostly misses", (0, 0, 2)), ("all sky", (26, 6, 40))):
        sky = rb.make_camera(200, 120, 20.0, (13, 3, 2), target, (0.3, 0.5, 0.9), 9, 50)
        got, t = dev.render_aov_to_host(sky)
        w2 = ar.reference(host, sky)
        assert t.primary_visibility == 1 and (w2["hits"] == 0).mean() > 0.5, what
        if what == "all sky":
            assert not w2["hits"].any() and (w2["prim"] == -1).all()
        else:
            assert w2["hits"].any()
        assert_same_aovs(got, w2, what)


@pytest.mark.gpu
def test_headline_and_stress_frames_at_size():
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(1920, 1080, 500, 50)
    got, t = dev.render_aov_to_host(cam)
    assert t.primary_visibility == 1
    rows = [3, 140, 300, 539, 540, 777, 1001, 1079]
    assert_same_aovs({k: v[rows] for k, v in got.items()}, ar.reference(host, cam, rows=rows), "configs[2], 8 rows")
    dev.close()
    host = rb.HostScene.rtiow(half_extent=158, textured_quad=True, texture_size=256)
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(3840, 2160, 2, 50)
    got, t = dev.render_aov_to_host(cam)
    assert t.primary_visibility == 1
    assert_same_aovs(got, ar.reference(host, cam), "configs[4] geometry, whole 4K frame at 2 spp")


@pytest.mark.gpu
def test_aov_calls_leave_the_handles_decisions_alone():
    """Under AUTO, beauty / AOV / beauty (other camera) / AOV / beauty: the beauty frames and the handle's choices are those of the
    same beauty calls alone.  The setup decides by flag share, not by timing: S-rtiow with a 2-entry stack and no front
    primitives gives up its first guarded pass and the handle steps aside."""
    host = rb.HostScene.rtiow()
    cams = [rb.rtiow_camera(240, 135, 8, 50), rb.make_camera(240, 135, 30.0, (10, 4, -6), (0, 0.5, 0), (0.7, 0.8, 1.0), 8, 50)]

    def run(with_aov):
        dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_AUTO, guard_keep=0, guard_front_primitives=-1, stack_levels=2)
        frames, fields, aovs = [], [], []
        for k, cam in enumerate((cams[0], cams[1], cams[0])):
            fb, t = dev.render_to_host(cam)
            frames.append(fb)
            fields.append((t.kernel, t.guarded, t.guard_paused, t.primary_visibility))
            if with_aov and k < 2:
                aovs.append(dev.render_aov_to_host(cam)[0])
        dev.close()
        return frames, fields, aovs

    frames0, fields0, _ = run(False)
    frames1, fields1, aovs = run(True)
    assert fields0[0][1:3] == (1, 1), fields0        # the first frame is guarded and the handle steps aside
    assert fields1 == fields0
    for a, b in zip(frames0, frames1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for cam, got in zip(cams, aovs):
        assert_same_aovs(got, ar.reference(host, cam), "AOVs between beauty frames")


@pytest.mark.gpu
def test_cli_writes_the_reference_aov_file(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines)
    out = subprocess.run([exe, "--gpu", "--aov"], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    host = rb.HostScene.from_config(text)
    cam = host.frame_camera(0)
    want = aov_file_bytes(ar.reference(host, cam), cam.image_width, cam.image_height, cam.samples_per_pixel)
    assert open(tmp_path / "f_0.png.aov", "rb").read() == want
    assert os.path.exists(tmp_path / "f_0.png")
