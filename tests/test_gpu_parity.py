"""Parity tests proper: the HIP path, called through the C ABI, against the CPU oracle.

Tolerance: NONE for this float path — per-sample radiance, ray counts, RNG states and per-pixel
sums are compared bit for bit.  (The kernel evaluates the reference's float expressions unfused
and in the same order; the libm-dependent pieces — expf, powf(x, 5) of the Schlick term, acosf and
atan2f of a textured sphere's uv — are restatements of the host libm's own algorithms, compared with it
for every float of their domains on the CPU: tests/test_device_math.py, tools/libm_exhaustive.cpp.)
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import oracle_bindings as ob
import rtp_bindings as rb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_frame(got, want, what):
    same = (bits(got) == bits(want)).all(axis=-1)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} pixels differ, max abs diff {np.abs(got - want).max()}"


# Handles in this module render many frames each: unless a test says otherwise they ask for the guarded walk outright (where the
# scene is eligible) and keep it, so that which walk a frame took does not depend on what the handle has measured or flagged on
# its earlier frames.  The policy has its own tests, on handles made with traversal=rb.TRAVERSAL_AUTO — what rt_config_init gives.
@pytest.fixture(scope="module", autouse=True)
def guarded_walk_by_default():
    rb.DEFAULTS.update(traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
    yield
    rb.DEFAULTS.clear()


@pytest.fixture(scope="module")
def rtiow(guarded_walk_by_default):
    host = rb.HostScene.rtiow()
    return host, rb.DeviceScene(host, device=0)


@pytest.fixture(scope="module")
def config_scene(test_config_text, guarded_walk_by_default):
    host = rb.HostScene.from_config(test_config_text)
    return host, rb.DeviceScene(host, device=0)


def test_native_library_is_loaded():
    lib = rb.amd_lib()
    assert b"gfx950" in lib.rt_version_string()
    with open("/proc/self/maps") as f:
        assert "librtp_amd.so" in f.read()


def test_config_scene_probe_matches_golden(config_scene):
    host, dev = config_scene
    g = np.load(os.path.join(HERE, "golden", "config_probe.npz"))
    cam = host.frame_camera(0)
    rad, rays, seeds = dev.trace_samples(cam, g["ijs"])
    assert np.array_equal(bits(rad), g["rad_bits"])
    assert np.array_equal(rays, g["rays"]) and np.array_equal(seeds, g["seeds"])


def test_config_scene_frame_reproduces_reference_file(config_scene, golden):
    """GPU render → BinarySaver bytes → the sha256 of the file the REFERENCE's CPU path wrote."""
    host, dev = config_scene
    cam = host.frame_camera(0)
    fb, _ = dev.render_to_host(cam)
    g = np.load(os.path.join(HERE, "golden", "config_probe.npz"))
    assert np.array_equal(bits(fb), g["fb_bits"])
    data = rb.binary_image_bytes(fb, cam.image_width, cam.image_height, host.info.sqrt_spp)
    assert hashlib.sha256(data).hexdigest() == golden["test_config_binary_saver_sha256"]


def test_config_scene_c1(config_scene):
    """BASELINE configs[0]: config scene, 400x225, depth 10, 3^2 and 4^2 spp."""
    host, dev = config_scene
    for sqrt_spp in (3, 4):
        base = host.frame_camera(0)
        eye = list(base.origin.e)
        cam = rb.make_camera(400, 225, 50.0, eye, (0.0, 0.0, 4.5), (0, 0, 0), sqrt_spp * sqrt_spp, 10)
        fb, _ = dev.render_to_host(cam)
        assert_same_frame(fb, ob.render(host, cam, threads=8), f"C1 {sqrt_spp}^2 spp")


def test_rtiow_probe_at_headline_config(rtiow):
    host, dev = rtiow
    g = np.load(os.path.join(HERE, "golden", "rtiow_probe.npz"))
    cam = rb.rtiow_camera(1920, 1080, 500, 50)
    rad, rays, seeds = dev.trace_samples(cam, g["ijs"])
    assert np.array_equal(bits(rad), g["rad_bits"])
    assert np.array_equal(rays, g["rays"]) and np.array_equal(seeds, g["seeds"])
    assert rays.max() > 20        # deep paths are exercised


def test_rtiow_small_frame_matches_golden(rtiow):
    host, dev = rtiow
    g = np.load(os.path.join(HERE, "golden", "rtiow_probe.npz"))
    fb, t = dev.render_to_host(rb.rtiow_camera(96, 64, 4, 50))
    assert np.array_equal(bits(fb), g["fb_bits"])
    assert t.scene_in_lds == 1 and t.kernel_ms > 0


def test_rtiow_c2_rows_at_full_width(rtiow):
    """BASELINE configs[1] geometry (1200x800, depth 50) at 6 spp: every pixel of the GPU frame
    equals the oracle's, checked on three row bands the oracle finishes in seconds."""
    host, dev = rtiow
    cam = rb.rtiow_camera(1200, 800, 6, 50)
    fb, _ = dev.render_to_host(cam)
    for row0 in (0, 396, 780):
        want = ob.render(host, cam, row0=row0, row1=row0 + 20, threads=8)
        assert_same_frame(fb[row0:row0 + 20], want, f"rows {row0}..")


def test_production_kernel_at_the_headline_config():
    """BASELINE configs[2] — 1920x1080, 500 spp, 50 bounces — through the DEFAULT path of a fresh handle: ONE launch of the
    sphere-only trace kernel fed by the primary-visibility pass (render_kernel, src/camera.cu:17-34), three rows of the frame
    compared bit for bit with the oracle."""
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0, honour_env=False, traversal=rb.TRAVERSAL_AUTO, guard_keep=0)      # what rt_config_init gives
    cam = rb.rtiow_camera(1920, 1080, 500, 50)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.sphere_only == 1 and t.primary_visibility == 1 and t.trace_launches == 1 and t.scene_in_lds == 1
    assert t.workgroup_size == 1024 and t.num_workgroups == 512
    assert 0 < t.flagged_samples < 1e-3 * 1920 * 1080 * 500
    for row in (3, 540, 1073):        # sky, the big spheres, the foreground
        want = ob.render(host, cam, row0=row, row1=row + 1, threads=1)
        assert_same_frame(fb[row:row + 1], want, f"headline frame, row {row}")
    dev.close()


def test_rtiow_c2_at_full_spp():
    """BASELINE configs[1] at its full 1200x800 x 100 spp x 50 bounces through the default path; two rows against the oracle."""
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0, honour_env=False, traversal=rb.TRAVERSAL_AUTO, guard_keep=0)      # what rt_config_init gives
    cam = rb.rtiow_camera(1200, 800, 100, 50)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.sphere_only == 1 and t.primary_visibility == 1 and t.trace_launches == 1
    for row in (420, 777):
        want = ob.render(host, cam, row0=row, row1=row + 1, threads=1)
        assert_same_frame(fb[row:row + 1], want, f"C2 frame, row {row}")
    dev.close()


def test_primary_visibility_pass_changes_nothing_but_the_time(config_scene):
    """rt_config.primary_visibility: camera rays resolved from per-pixel candidate lists (rt_primary.hip.inc) or walked like every
    other ray — the same frame bit for bit, on the sphere-only kernel, on the general kernel (planes: the config scene), with
    passes shorter and longer than a wave (the pass per batch and the pass per pixel), with several passes per frame, on a
    row shard, and where most pixels have no list at all (fat pixels: more candidates than a list holds)."""
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0, honour_env=False, traversal=rb.TRAVERSAL_GUARDED)
    cases = [(rb.rtiow_camera(160, 90, 9, 50), {}, None), (rb.rtiow_camera(96, 54, 200, 50), {}, None),
             (rb.rtiow_camera(64, 36, 300, 50), {"pass_spp": 150}, None), (rb.rtiow_camera(64, 36, 200, 50), {"pass_spp": 64}, None),
             (rb.rtiow_camera(128, 72, 130, 50), {}, rb.Shard(8, 3, 1)), (rb.make_camera(16, 9, 90.0, (13, 3, 2), (0, 0, 0), (0.7, 0.8, 1.0), 130, 50), {}, None),
             (rb.make_camera(200, 120, 60.0, (0.3, 0.2, 0.12), (4, 0, 0.2), (0.7, 0.8, 1.0), 16, 50), {}, None)]
    for cam, cfg, shard in cases:
        dev.configure(primary_visibility=0, pass_spp=cfg.get("pass_spp", 0))
        a, ta = dev.render_to_host(cam, shard)
        dev.configure(primary_visibility=-1)
        b, tb = dev.render_to_host(cam, shard)
        assert ta.primary_visibility == 1 and tb.primary_visibility == 0 and ta.guarded == 1 and tb.guarded == 1
        assert_same_frame(a, b, f"{cam.image_width}x{cam.image_height}x{cam.samples_per_pixel} {cfg}")
    dev.configure(primary_visibility=0, pass_spp=0)
    cam = rb.rtiow_camera(96, 54, 130, 50)
    fb, t = dev.render_to_host(cam)
    assert t.primary_visibility == 1
    assert_same_frame(fb, ob.render(host, cam, threads=8), "pixel pass against the oracle")
    dev.close()
    # planes, triangles, quads, emitters: the general kernel
    hostc, devc = config_scene
    eye = list(hostc.frame_camera(0).origin.e)
    for spp in (9, 144):
        cam = rb.make_camera(200, 112, 50.0, eye, (0.0, 0.0, 4.5), (0, 0, 0), spp, 10)
        devc.configure(primary_visibility=0, traversal=rb.TRAVERSAL_GUARDED)
        a, ta = devc.render_to_host(cam)
        devc.configure(primary_visibility=-1)
        b, tb = devc.render_to_host(cam)
        devc.configure(primary_visibility=0, traversal=rb.TRAVERSAL_GUARDED)
        assert ta.primary_visibility == 1 and ta.sphere_only == 0 and tb.primary_visibility == 0
        assert_same_frame(a, b, f"config scene {spp} spp")
        if spp == 9:
            assert_same_frame(a, ob.render(hostc, cam, threads=8), "config scene against the oracle")


def test_sky_pixels_and_the_fetch_order(config_scene):
    """The primary pass finishes sky pixels itself and the trace kernel takes the other pixels through a table, expensive ones
    first (rt_primary.hip.inc, order_* kernels); at the end of a pass the waves of a workgroup take what the others still
    hold.  Frames against the oracle where those paths have their corners: nothing but sky (no pixel for the trace kernel),
    no sky at all, sky with a background of negative zeros (0 + 1 * -0 is +0), fewer pixels than one block of the sort, more
    samples than pixels, both primary kernels (passes under and over 96 samples), several passes, a row shard, a tile."""
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0, honour_env=False)
    sky = (0.7, 0.8, 1.0)
    cases = [("all sky", rb.make_camera(64, 36, 20.0, (13, 3, 2), (26, 6, 40), sky, 9, 50), None),
             ("all sky, pixel pass", rb.make_camera(8, 8, 20.0, (13, 3, 2), (26, 6, 40), sky, 130, 50), None),
             ("no sky", rb.make_camera(96, 54, 30.0, (13, 3, 6), (0, 0, -2), sky, 12, 50), None),
             ("negative zero background", rb.make_camera(48, 27, 40.0, (13, 3, 2), (0, 0, 3), (-0.0, 0.25, -0.0), 140, 50), None),
             ("three pixels", rb.rtiow_camera(3, 1, 700, 50), None),
             ("one pixel of sky", rb.make_camera(1, 1, 1.0, (13, 3, 2), (26, 6, 40), sky, 5, 50), None),
             ("shard", rb.rtiow_camera(160, 90, 24, 50), rb.Shard(8, 3, 2)),
             ("horizon", rb.make_camera(320, 20, 20.0, (13, 3, 0.5), (0, 0, 0.5), sky, 200, 50), None)]
    for what, cam, shard in cases:
        fb, t = dev.render_to_host(cam, shard)
        assert t.primary_visibility == 1 and t.guarded == 1, what
        rows = None if shard is None else [r for r in range(cam.image_height) if (r // shard.band_rows) % shard.num_parts == shard.part]
        want = ob.render(host, cam, threads=8)
        assert_same_frame(fb, want if rows is None else want[rows], what)
        if what.startswith("all sky"):
            assert t.flagged_samples == 0 and np.unique(bits(fb).reshape(-1, 3), axis=0).shape[0] == 1
    # several passes, and a tile cut out of the frame
    cam = rb.rtiow_camera(96, 54, 300, 50)
    dev.configure(pass_spp=70)
    fb, t = dev.render_to_host(cam)
    dev.configure(pass_spp=0)
    assert t.trace_launches == 5
    want = ob.render(host, cam, threads=8)
    assert_same_frame(fb, want, "five passes")
    tile, _ = dev.render_tile_to_host(cam, 17, 0, 40, 23)
    assert_same_frame(tile, want[0:23, 17:57], "tile over sky and ground")
    dev.close()
    # the general kernel (planes, emitters) over a frame that is mostly background
    hostc, devc = config_scene
    eye = list(hostc.frame_camera(0).origin.e)
    cam = rb.make_camera(120, 68, 100.0, eye, (0.0, 0.0, 4.5), (0.1, 0.2, 0.3), 130, 10)
    devc.configure(primary_visibility=0, traversal=rb.TRAVERSAL_GUARDED)
    fb, t = devc.render_to_host(cam)
    devc.configure(primary_visibility=0, traversal=rb.TRAVERSAL_GUARDED)
    assert t.primary_visibility == 1 and t.sphere_only == 0
    assert_same_frame(fb, ob.render(hostc, cam, threads=8), "config scene, wide view")


def test_samples_accumulate_in_order(rtiow):
    """Linearity-style property usable at any size: the 64-spp pixel sum is the in-order float sum
    of the 64 per-sample radiances (src/camera.cu:27-31)."""
    host, dev = rtiow
    cam = rb.rtiow_camera(64, 40, 64, 50)
    fb, _ = dev.render_to_host(cam)
    pix = [(5, 7), (33, 20), (63, 39), (0, 0)]
    for (i, j) in pix:
        ijs = np.array([[i, j, s] for s in range(64)], dtype=np.int32)
        rad, _, _ = dev.trace_samples(cam, ijs)
        acc = np.zeros(3, dtype=np.float32)
        for s in range(64):
            acc = acc + rad[s]
        assert np.array_equal(bits(acc), bits(fb[j, i]))


def test_pass_size_does_not_change_the_frame(rtiow):
    """rt_render cuts the samples of a pixel into passes sized by the slab budget; whatever the
    cut (one pass of 150, 64+64+22, 100+50, 7-sample passes), the in-order sum is the same bits,
    and equals the oracle's on a row band."""
    host, dev = rtiow
    cam = rb.rtiow_camera(96, 50, 150, 50)
    want, t = dev.render_to_host(cam)
    assert t.trace_launches == 1
    assert_same_frame(want[20:26], ob.render(host, cam, row0=20, row1=26, threads=8), "one pass of 150 spp")
    try:
        for forced, launches in ((64, 3), (100, 2), (7, 22)):
            dev.configure(pass_spp=forced)
            got, t = dev.render_to_host(cam)
            assert t.trace_launches == launches
            assert_same_frame(got, want, f"passes of {forced} spp")
    finally:
        dev.configure(pass_spp=0)


def test_sharded_render_equals_full_frame(rtiow):
    host, dev = rtiow
    cam = rb.rtiow_camera(200, 117, 3, 50)       # width and height not multiples of 8
    full, _ = dev.render_to_host(cam)
    assert_same_frame(full, ob.render(host, cam, threads=8), "full frame")
    import frame_parallel as fp
    for world, band in ((2, 8), (3, 5), (8, 16)):
        frame = np.zeros_like(full)
        for r in range(world):
            part, _ = dev.render_to_host(cam, rb.Shard(band, world, r))
            rows = fp.shard_row_indices(cam.image_height, band, world, r)
            assert part.shape[0] == len(rows)
            frame[rows] = part
        assert np.array_equal(bits(frame), bits(full))


def test_tiles_of_any_shape_assemble_the_frame(rtiow, config_scene):
    """rt_render_tile (tile_x0, tile_y0, w, h): rectangles rendered one by one — ragged sizes, a single pixel, a
    single column — put together are the bits of the whole frame, with and without the primary-visibility pass, on the
    sphere-only kernel, the general kernel (planes) and the exact walk; a rectangle that leaves the image is refused."""
    for (host, dev), cam, cfg in ((rtiow, rb.rtiow_camera(97, 61, 130, 50), {}), (rtiow, rb.rtiow_camera(97, 61, 7, 50), {"primary_visibility": -1}),
                                  (rtiow, rb.rtiow_camera(64, 40, 5, 50), {"traversal": rb.TRAVERSAL_EXACT}),
                                  (config_scene, rb.make_camera(90, 50, 50.0, list(config_scene[0].frame_camera(0).origin.e), (0.0, 0.0, 4.5), (0, 0, 0), 9, 10),
                                   {"traversal": rb.TRAVERSAL_GUARDED})):
        dev.configure(**cfg)
        W, H = cam.image_width, cam.image_height
        whole, _ = dev.render_to_host(cam)
        got = np.full_like(whole, np.nan)
        xs = [0, 1, 34, W - 1, W]                  # columns [0,1) [1,34) [34,W-1) [W-1,W)
        ys = [0, 17, 18, H]
        for y0, y1 in zip(ys[:-1], ys[1:]):
            for x0, x1 in zip(xs[:-1], xs[1:]):
                tile, t = dev.render_tile_to_host(cam, x0, y0, x1 - x0, y1 - y0)
                assert tile.shape == (y1 - y0, x1 - x0, 3)
                got[y0:y1, x0:x1] = tile
        assert_same_frame(got, whole, f"tiles of a {W}x{H} frame {cfg}")
        dev.configure(**{k: 0 for k in cfg})
    host, dev = rtiow
    cam = rb.rtiow_camera(32, 20, 2, 8)
    for bad in ((-1, 0, 4, 4), (30, 0, 4, 4), (0, 18, 4, 4), (0, 0, 0, 4)):
        with pytest.raises(RuntimeError, match="tile"):
            dev.render_tile_to_host(cam, *bad)


def test_render_into_torch_buffer_on_a_stream(rtiow):
    import torch
    host, dev = rtiow
    cam = rb.rtiow_camera(160, 96, 2, 50)
    stream = torch.cuda.Stream()
    fb = torch.zeros((96, 160, 3), dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(stream):
        dev.render(cam, fb.data_ptr(), stream=stream.cuda_stream, sync=False)
    stream.synchronize()
    assert dev.last_kernel_ms() > 0
    assert_same_frame(fb.cpu().numpy(), ob.render(host, cam, threads=8), "torch stream render")


def test_device_tonemap_matches_saver_bytes(rtiow):
    import torch
    host, dev = rtiow
    cam = rb.rtiow_camera(128, 72, 9, 50)
    fb = torch.zeros((72, 128, 3), dtype=torch.float32, device="cuda:0")
    dev.render(cam, fb.data_ptr())
    out = torch.zeros(fb.numel(), dtype=torch.uint8, device="cuda:0")
    assert rb.amd_lib().rt_tonemap(C.c_void_p(fb.data_ptr()), C.c_void_p(out.data_ptr()), fb.numel(), 3, None) == 0
    torch.cuda.synchronize()
    want = ob.write_color_bytes(fb.cpu().numpy(), 3).reshape(-1)
    assert np.array_equal(out.cpu().numpy(), want)


# ---- edge cases -------------------------------------------------------------------------------------

def _scene_from_arrays(spheres, planes, materials, textures=()):
    """Build a HostScene-like object from python lists using the host BVH builder through a
    config-free path: write the arrays into ctypes structs and run the oracle/host on them."""
    class Obj:
        pass
    o = Obj()
    o.spheres = (rb.Sphere * max(len(spheres), 1))(*spheres)
    o.planes = (rb.Plane * max(len(planes), 1))(*planes)
    o.materials = (rb.Material * max(len(materials), 1))(*materials)
    o.textures = (rb.Texture * max(len(textures), 1))(*textures)
    return o


def _material(mtype, albedo=(0, 0, 0), fuzz=0.0, ir=1.0, absorption=(0, 0, 0), emit=(0, 0, 0), tex=0):
    m = rb.Material()
    m.type, m.fuzz, m.ir = mtype, fuzz, ir
    m.albedo.e[:] = albedo
    m.absorption.e[:] = absorption
    m.emit.e[:] = emit
    m.texture_id = tex
    return m


def test_empty_scene_and_degenerate_cameras(rtiow):
    host, dev = rtiow
    empty = rb.HostScene.rtiow()      # reuse the handle type, then blank the description
    empty.desc.num_spheres = empty.desc.num_planes = empty.desc.num_nodes = 0
    d = rb.DeviceScene(empty, device=0)
    cam = rb.make_camera(33, 17, 40.0, (3, 2, 1), (0, 0, 0), (0.25, 0.5, 0.75), 5, 7)
    fb, _ = d.render_to_host(cam)
    assert_same_frame(fb, ob.render(empty, cam), "empty scene")
    assert np.array_equal(fb[0, 0], np.array([1.25, 2.5, 3.75], dtype=np.float32))
    # zero samples / zero depth: the reference's loops add nothing
    for spp, depth in ((0, 5), (4, 0)):
        cam0 = rb.rtiow_camera(40, 24, spp, depth)
        fb, _ = dev.render_to_host(cam0)
        assert not fb.any()
        assert_same_frame(fb, ob.render(host, cam0), "degenerate camera")
    # 1x1 image, depth 1
    cam1 = rb.rtiow_camera(1, 1, 7, 1)
    fb, _ = dev.render_to_host(cam1)
    assert_same_frame(fb, ob.render(host, cam1), "1x1")


def test_all_plane_types_materials_and_textures():
    """A hand-made scene with QUAD / ELLIPSE / TRIANGLE planes, all four materials, absorbing
    glass (expf path) and a textured quad (software bilinear fetch)."""
    host = rb.HostScene.rtiow(half_extent=2, textured_quad=True, texture_size=64)
    # turn one small sphere into absorbing glass and one into a light, switch two planes' types
    desc = host.desc
    assert desc.num_planes == 1 and desc.num_textures == 1
    mats = desc.materials
    glass = [k for k in range(desc.num_materials) if mats[k].type == 2]
    mats[glass[0]].absorption.e[:] = (0.9, 0.2, 0.05)
    diffuse = [k for k in range(desc.num_materials) if mats[k].type == 0]
    mats[diffuse[1]].type = 3
    mats[diffuse[1]].emit.e[:] = (4.0, 3.0, 2.0)
    mats[diffuse[2]].texture_id = 1            # a textured SPHERE: acosf/atan2f uv path
    dev = rb.DeviceScene(host, device=0)
    cam = rb.make_camera(160, 100, 35.0, (6, 2, 2.5), (0, 0, 0.3), (0.6, 0.7, 0.9), 6, 12)
    fb, _ = dev.render_to_host(cam)
    want = ob.render(host, cam, threads=8)
    # the textured sphere's uv go through the host libm's acosf / atan2f ALGORITHMS on the device too (rt_device_math.h
    # acos_libm / atan2_libm, pinned on the CPU against this libm for every float): no tolerance here either
    assert_same_frame(fb, want, "QUAD + textured sphere + absorbing glass + light")
    desc.planes[0].type = 1                       # ELLIPSE
    dev2 = rb.DeviceScene(host, device=0)
    fb2, _ = dev2.render_to_host(cam)
    assert_same_frame(fb2, ob.render(host, cam, threads=8), "ELLIPSE")
    assert not np.array_equal(fb, fb2)
    # many textured spheres, seen from close by: every branch of acosf (|y| < 0.5, y < -0.5, y > 0.5) and every quadrant of atan2f
    for k in diffuse[3:40]:
        mats[k].texture_id = 1
    dev3 = rb.DeviceScene(host, device=0)
    cam3 = rb.make_camera(200, 120, 60.0, (1.5, 1.2, 1.1), (0, 0, 0.2), (0.6, 0.7, 0.9), 8, 12)
    fb3, _ = dev3.render_to_host(cam3)
    assert_same_frame(fb3, ob.render(host, cam3, threads=8), "textured spheres close up")


def test_config_scene_with_texture_and_triangles(test_config_text, tmp_path):
    """The polyhedra scene (triangles + quads + absorbing dielectrics) with a real floor texture
    loaded by the host texture loader (binary PPM)."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    ppm = tmp_path / "floor.ppm"
    with open(ppm, "wb") as f:
        f.write(b"P6\n53 37\n255\n" + img.tobytes())
    text = test_config_text.replace("../floor2.jpg", str(ppm))
    host = rb.HostScene.from_config(text)
    assert host.desc.num_textures == 1 and host.desc.materials[0].texture_id == 1
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera(0)
    fb, _ = dev.render_to_host(cam)
    assert_same_frame(fb, ob.render(host, cam, threads=4), "textured config scene")


def test_scene_validation_errors(rtiow):
    host, _ = rtiow
    lib = rb.amd_lib()
    bad = rb.HostScene.rtiow(half_extent=1)
    bad.desc.spheres[0].material_idx = 10_000
    h = C.c_void_p()
    assert lib.rt_scene_create(C.byref(bad.desc), C.byref(h)) == 1
    assert b"material index" in lib.rt_get_last_error_string()
    bad2 = rb.HostScene.rtiow(half_extent=1)
    bad2.desc.nodes[0].left = 0          # child index not after its parent
    assert lib.rt_scene_create(C.byref(bad2.desc), C.byref(h)) == 1
    assert lib.rt_set_device(99) == 2


def test_stress_scene_bvh_from_global_memory():
    """~100k spheres: the traversal tables exceed LDS and are read through L1/L2 instead."""
    host = rb.HostScene.rtiow(half_extent=158)
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(240, 136, 2, 50)
    fb, t = dev.render_to_host(cam)
    assert t.scene_in_lds == 0
    assert_same_frame(fb, ob.render(host, cam, threads=8), "100k spheres")


def test_cli_frame_drivers_write_reference_bytes(test_config_text, golden, tmp_path):
    """rtp_main (the reference's CLI shape): frame-after-frame driver and the pipelined driver
    (device-side saver arithmetic + overlapped file output) write the same bytes; frame 0 of the
    unmodified test config is the file the reference's CPU path wrote (sha256 pin)."""
    import subprocess
    root = os.path.dirname(HERE)
    exe = os.path.join(root, "ray-tracing-practice_amd", "rtp_main")
    lines = test_config_text.split("\n")
    assert lines[0] == "1" and lines[1] == "test_output_%d.png"
    # (a) the unmodified scene, one frame
    lines[1] = str(tmp_path / "a_%d.png")
    out = subprocess.run([exe, "--gpu"], input="\n".join(lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    n, ms, rays = out.stdout.strip().split("\t")
    assert (n, rays) == ("0", str(200 * 100 * 4)) and float(ms) > 0
    data = open(tmp_path / "a_0.png", "rb").read()
    assert hashlib.sha256(data).hexdigest() == golden["test_config_binary_saver_sha256"]
    # (b) a 3-frame orbit, both drivers
    lines[0] = "3"
    lines[5] = "0.0 0.0 1.0"          # wrc wzc wc: the eye circles the scene
    for tag, extra in (("seq", []), ("pipe", ["--devices", "1"]), ("shard", ["--shard", "1"])):
        lines[1] = str(tmp_path / (tag + "_%d.png"))
        out = subprocess.run([exe, "--gpu"] + extra, input="\n".join(lines), capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert len(out.stdout.strip().split("\n")) == 3
    host = rb.HostScene.from_config("\n".join(lines))
    for f in range(3):
        a = open(tmp_path / f"seq_{f}.png", "rb").read()
        b = open(tmp_path / f"pipe_{f}.png", "rb").read()
        c = open(tmp_path / f"shard_{f}.png", "rb").read()        # rt_context / rt_render_sharded / RCCL self gather
        assert a == b and a == c and len(a) == 60008
        cam = host.frame_camera(f)
        want = rb.binary_image_bytes(ob.render(host, cam, threads=4), 200, 100, host.info.sqrt_spp)
        assert a == want
    assert open(tmp_path / "seq_0.png", "rb").read() != open(tmp_path / "seq_1.png", "rb").read()


def test_alternative_kernels_agree_with_default(rtiow):
    """The exact walk alone (rt_config.traversal = RT_TRAVERSAL_EXACT) must give the bits of the default
    (guarded walk + exact re-walk).  Set through the configuration API, not the environment."""
    host, dev = rtiow
    cam = rb.rtiow_camera(320, 200, 8, 50)
    want, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.guard_unproven == 0
    assert_same_frame(want, ob.render(host, cam, threads=8), "default kernel")
    try:
        dev.configure(traversal=rb.TRAVERSAL_EXACT)
        assert dev.config().traversal == rb.TRAVERSAL_EXACT
        got, t = dev.render_to_host(cam)
        assert t.guarded == 0 and t.flagged_samples == 0
        assert_same_frame(got, want, "exact walk only")
    finally:
        dev.configure(traversal=rb.TRAVERSAL_GUARDED)


def test_context_renders_sharded_frames_through_the_c_abi():
    """rt_context / rt_render_sharded / rt_gather: (a) a one-device context — the gather runs through RCCL
    (ncclSend/ncclRecv to itself: the code path of an 8-GPU node, transport "rccl") and the frame is the oracle's;
    (b) the same device listed 2 and 3 times ("copy" transport: RCCL does not admit one GPU twice): interleaved bands of
    4 and 8 rows with ragged ends, rendered as separate shards on separate streams and reassembled — bit-identical."""
    import torch
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(200, 117, 5, 50)             # 117 rows: the last band is partial
    want = ob.render(host, cam, threads=8)
    fb = torch.empty((117, 200, 3), dtype=torch.float32, device="cuda:0")
    ctx = rb.Context(1)
    assert ctx.num_devices == 1 and ctx.transport == "rccl"
    ctx.scene(host)
    ts = ctx.render(cam, fb.data_ptr())
    assert len(ts) == 1 and ts[0].kernel_ms > 0
    assert_same_frame(fb.cpu().numpy(), want, "one-device context, RCCL self gather")
    ctx.close()
    for parts, band in ((2, 8), (3, 4)):
        ctx = rb.Context(parts, ordinals=[0] * parts)
        assert ctx.num_devices == parts and ctx.transport == "copy"
        ctx.scene(host)
        fb.zero_()
        ts = ctx.render(cam, fb.data_ptr(), band_rows=band)
        assert len(ts) == parts
        assert_same_frame(fb.cpu().numpy(), want, f"{parts}-way shard of one GPU, bands of {band}")
        ctx.close()


def test_two_rank_bench_rehearsal_on_one_gpu():
    """The N > 1 path of bench.py with the REAL HIP render: `bench.py --gpus 2` as its own launcher, two ranks sharing this
    box's one GPU, each rendering its interleaved row bands of the headline frame, the bands gathered over gloo (RCCL does not
    admit one GPU twice) and the assembled frame compared with the oracle on two rows.  What it cannot show is the RCCL
    transport itself — that needs two GPUs."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(RTP_BENCH_BACKEND="gloo", RTP_BENCH_CHECK="1")
    from conftest import run_child
    res = run_child([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], 200, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["world_size_seen_by_collective"] == 2 and out["config"]["collective_backend"] == "gloo"
    assert out["checked_rows"]["assembled_frame_bit_identical"] is True
    assert out["roofline"]["per_rank"]["trace_ms"] > 0 and out["roofline"]["per_rank"]["gather_ms"] > 0
    assert out["value"] > 0 and out["scaling"] == "strong"


def test_distance_aware_margins():
    """rt_config.guard_dynamic_margins: (a) forced on S-rtiow (such scenes take their records through L1 / L2 whatever their
    size: step_pair_par), near and very far cameras — no far-origin flags, no re-pack needed; (b) tiny spheres scattered over a wide volume, a
    scene whose static margins would exceed 64 radii: eligible for the guarded walk only with distance-aware margins,
    which the automatic rule grants to scenes whose small spheres are of one size class (this one is not: forced here);
    frames are the oracle's."""
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0, honour_env=False, guard_dynamic_margins=2)
    for cam in (rb.rtiow_camera(240, 135, 8, 50), rb.make_camera(160, 90, 3.0, (400.0, 90.0, 60.0), (0, 0, 0), (0.7, 0.8, 1.0), 4, 50)):
        fb, t = dev.render_to_host(cam)
        assert t.guarded == 1 and t.guard_dynamic == 1 and t.scene_in_lds == 0
        assert_same_frame(fb, ob.render(host, cam, threads=8), "S-rtiow, distance-aware margins")
    rng = np.random.default_rng(4242)
    mats = [_material(0, albedo=(0.8, 0.7, 0.6)), _material(1, albedo=(0.9, 0.9, 0.8), fuzz=0.05), _material(2, ir=1.5)]
    n = 3000
    spheres = np.zeros((n, 5), dtype=np.float32)
    spheres[:, :3] = rng.uniform(-400, 400, (n, 3))
    spheres[:, 3] = rng.uniform(0.02, 0.6, n)
    spheres[:, 4] = rng.integers(0, 3, n)
    spheres[0] = [0, 0, -2000, 1600, 0]
    host = rb.HostScene.from_arrays(spheres, np.zeros((0, 11), np.float32), mats)
    static = rb.DeviceScene(host, device=0, honour_env=False, guard_dynamic_margins=1)
    assert "margins exceed" in static.guard_reason()
    auto = rb.DeviceScene(host, device=0, honour_env=False)
    assert "margins exceed" in auto.guard_reason()     # radii over a factor 30: the automatic rule keeps such scenes on the exact walk
    dev = rb.DeviceScene(host, device=0, honour_env=False, guard_dynamic_margins=2)
    assert dev.guard_reason() == ""
    cam = rb.make_camera(320, 180, 50.0, (300, -250, 120), (0, 0, 0), (0.6, 0.7, 0.9), 4, 30)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.guard_dynamic == 1
    assert_same_frame(fb, ob.render(host, cam, threads=8), "scattered tiny spheres, distance-aware margins")


def test_wide_nodes_with_distance_aware_margins_and_a_short_stack():
    """The walk with distance-aware margins on 4-wide nodes (step_wide_par: S-rtiow with the margins forced and the general build),
    with its own stack and with a 3-entry one that overflows (more flagged samples): the oracle's frames."""
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(240, 135, 8, 50)
    want = ob.render(host, cam, threads=8)
    dev = rb.DeviceScene(host, device=0, honour_env=False, guard_dynamic_margins=2, sphere_only_kernel=-1, traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.wide_nodes == 1 and t.guard_dynamic == 1 and t.scene_in_lds == 0
    assert_same_frame(fb, want, "S-rtiow, wide nodes + distance-aware margins")
    dev.configure(stack_levels=3, guard_keep=1)
    fb, t3 = dev.render_to_host(cam)
    assert t3.wide_nodes == 1 and t3.flagged_samples > t.flagged_samples
    assert_same_frame(fb, want, "S-rtiow, wide nodes + distance-aware margins, 3-entry stack")


def test_distance_aware_margins_with_the_by_pixel_primary_pass():
    """the combination a big scene rendered in few big passes takes by default — distance-aware margins (kDyn
    kernels) x the primary-visibility pass in its by-pixel form (primary_pixel_kernel: passes of 96 samples per pixel or more),
    with and without planes — against the oracle on whole small frames: S-rtiow with the margins forced, 3 000 tiny spheres
    spread wide (alone, and with quads, ellipses and triangles among them), and a 130-spp row band of S-100k."""
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0, honour_env=False, guard_dynamic_margins=2)
    cam = rb.rtiow_camera(96, 54, 130, 50)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.guard_dynamic == 1 and t.primary_visibility == 1 and t.trace_launches == 1 and t.abandoned_passes == 0
    assert_same_frame(fb, ob.render(host, cam, threads=8), "S-rtiow, distance-aware margins, 130 spp in one pass")
    rng = np.random.default_rng(777)
    mats = [_material(0, albedo=(0.8, 0.7, 0.6)), _material(1, albedo=(0.9, 0.9, 0.8), fuzz=0.05), _material(2, ir=1.5),
            _material(3, emit=(2.0, 1.5, 1.0))]
    n = 3000
    spheres = np.zeros((n, 5), dtype=np.float32)
    spheres[:, :3] = rng.uniform(-400, 400, (n, 3))
    spheres[:, 3] = rng.uniform(0.02, 0.6, n)
    spheres[:, 4] = rng.integers(0, 4, n)
    spheres[0] = [0, 0, -2000, 1600, 0]
    planes = np.zeros((24, 11), dtype=np.float32)
    planes[:, :3] = rng.uniform(-300, 300, (24, 3))
    planes[:, 3:6] = rng.uniform(-60, 60, (24, 3))
    planes[:, 6:9] = rng.uniform(-60, 60, (24, 3))
    planes[:, 9] = rng.integers(0, 4, 24)
    planes[:, 10] = rng.integers(0, 3, 24)
    cam = rb.make_camera(80, 48, 50.0, (300, -250, 120), (0, 0, 0), (0.6, 0.7, 0.9), 136, 30)
    for pl, what in ((np.zeros((0, 11), np.float32), "spheres only"), (planes, "with planes")):
        host = rb.HostScene.from_arrays(spheres, pl, mats)
        dev = rb.DeviceScene(host, device=0, honour_env=False, guard_dynamic_margins=2, traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
        assert dev.guard_reason() == "", dev.guard_reason()
        fb, t = dev.render_to_host(cam)
        assert t.guarded == 1 and t.guard_dynamic == 1 and t.primary_visibility == 1 and t.trace_launches == 1, what
        assert_same_frame(fb, ob.render(host, cam, threads=8), f"scattered tiny spheres {what}, 136 spp in one pass")
    host = rb.HostScene.rtiow(half_extent=158, textured_quad=True, texture_size=256)
    dev = rb.DeviceScene(host, device=0, honour_env=False)
    cam = rb.rtiow_camera(3840, 2160, 130, 50)
    fb, t = dev.render_tile_to_host(cam, 0, 1300, 3840, 2)
    assert t.scene_in_lds == 0 and t.guarded == 1 and t.guard_dynamic == 1 and t.primary_visibility == 1 and t.trace_launches == 1
    assert_same_frame(fb, ob.render(host, cam, row0=1300, row1=1302, threads=16), "S-100k, rows 1300-1301 at 130 spp")


def test_config_api_without_environment():
    """A handle created with honour_env=False takes everything from rt_config: forced pass size, a capped stack,
    an opt-in unproven margin (reported in rt_timing.guard_unproven) — frames are the oracle's in every case."""
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(160, 90, 70, 50)
    want = ob.render(host, cam, threads=8)
    dev = rb.DeviceScene(host, device=0, honour_env=False, pass_spp=64, stack_levels=3)
    fb, t = dev.render_to_host(cam)
    assert t.trace_launches == 2 and t.guarded == 1 and t.guard_unproven == 0
    assert_same_frame(fb, want, "pass_spp=64, stack_levels=3")
    dev2 = rb.DeviceScene(host, device=0, honour_env=False, guard_gamma_ulps=8.0)
    fb, t = dev2.render_to_host(cam)
    assert t.guarded == 1 and t.guard_unproven == 1
    assert_same_frame(fb, want, "guard_gamma_ulps=8 (opt-in, unproven)")
    dev3 = rb.DeviceScene(host, device=0, honour_env=False, workspace_bytes=160 * 90 * 12 * 64)
    fb, t = dev3.render_to_host(cam)
    assert t.trace_launches == 2
    assert_same_frame(fb, want, "workspace for 64 spp per pass: two passes of 35")


def test_sphere_only_kernel_and_general_kernel_give_the_same_frame():
    """rt_config.sphere_only_kernel: a scene without planes and textures is rendered by the sphere-only build of the octant
    kernel (1024-thread workgroups, 8 waves per SIMD, reported in rt_timing.sphere_only); -1 forces the general build.  Same
    frame, which is the oracle's; a scene WITH a plane never gets the sphere-only build."""
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(320, 180, 24, 50)
    want = ob.render(host, cam, threads=8)
    fast = rb.DeviceScene(host, device=0, honour_env=False)
    fb, t = fast.render_to_host(cam)
    assert t.guarded == 1 and t.sphere_only == 1 and t.workgroup_size == 1024, (t.guarded, t.sphere_only, t.workgroup_size)
    assert_same_frame(fb, want, "sphere-only build")
    general = rb.DeviceScene(host, device=0, honour_env=False, sphere_only_kernel=-1)
    fb2, t2 = general.render_to_host(cam)
    assert t2.guarded == 1 and t2.sphere_only == 0 and t2.workgroup_size == 768
    assert_same_frame(fb2, want, "general build")
    quad = rb.DeviceScene(rb.HostScene.rtiow(half_extent=3, textured_quad=True, texture_size=64), device=0, honour_env=False)
    _, t3 = quad.render_to_host(rb.rtiow_camera(64, 36, 4, 8))
    assert t3.sphere_only == 0


def test_first_frame_after_a_repack_that_changes_the_margins():
    """A camera outside the reach the guarded walk's margins were sized for makes the handle re-pack its tree on the FIRST frame —
    and the re-packed tree may have static margins where the first one had distance-aware ones (or the other way round): the walk,
    its node form (pair / 4-wide) and the kernel are chosen from the tables as they are AFTER the re-pack.  (Round 4: a handle that
    had picked 4-wide nodes for margins the re-pack then dropped launched nothing — found by tools/guard_stress.py, seed 1 scene 19.)"""
    for seed, trial, n_want in ((1, 19, 118), (2, 39, 109), (7, 7, 2685)):
        host, cam, n = _stress_scene(seed, trial, 12, 640, 360)
        assert n == n_want
        want, _ = rb.DeviceScene(host, device=0, honour_env=False, traversal=rb.TRAVERSAL_EXACT).render_to_host(cam)
        assert_same_frame(want[180:182], ob.render(host, cam, row0=180, row1=182, threads=8), "exact walk against the oracle")
        for kw in (dict(traversal=rb.TRAVERSAL_AUTO, guard_keep=0), dict(traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)):
            dev = rb.DeviceScene(host, device=0, honour_env=False, **kw)
            for frame in range(3):
                fb, t = dev.render_to_host(cam)
                assert_same_frame(fb, want, f"seed {seed} scene {trial}, frame {frame}, {kw}")
                assert t.trace_ms > 0.05, "a trace launch that did nothing"


def test_scene_sizes_around_what_lds_holds():
    """The S-rtiow family across the size at which its tables stop fitting LDS at full occupancy: up to there the sphere-only
    octant walk, beyond it distance-aware margins (small where static ones would have done) and the walk through L1 / L2 — its
    sphere-only build on pair nodes, or with sphere_only_kernel = -1 the general one on 4-wide nodes — chosen at pack time
    (PackOptions::lds_pair_budget), reported in rt_timing; frames are the oracle's on both sides, and with the rule switched off
    (guard_dynamic_margins = 1: one margin per sphere, LDS-resident whatever the occupancy)."""
    seen = set()
    for half in (11, 12, 13, 16):
        host = rb.HostScene.rtiow(half_extent=half)
        cam = rb.rtiow_camera(160, 90, 10, 50)
        want = ob.render(host, cam, threads=8)
        dev = rb.DeviceScene(host, device=0, honour_env=False)
        fb, t = dev.render_to_host(cam)
        assert t.guarded == 1 and t.front_primitives == 1 and t.primary_visibility == 1
        assert (t.scene_in_lds, t.guard_dynamic, t.wide_nodes, t.sphere_only) in ((1, 0, 0, 1), (0, 1, 0, 1)), (half, t.scene_in_lds, t.guard_dynamic, t.wide_nodes)
        seen.add(t.scene_in_lds)
        assert_same_frame(fb, want, f"half_extent {half}: {host.desc.num_spheres} spheres")
        general = rb.DeviceScene(host, device=0, honour_env=False, sphere_only_kernel=-1)
        fb, t = general.render_to_host(cam)
        assert (t.guard_dynamic, t.wide_nodes, t.sphere_only) in ((0, 0, 0), (1, 1, 0)), (half, t.guard_dynamic, t.wide_nodes, t.sphere_only)
        assert_same_frame(fb, want, f"half_extent {half}, general build")
        static = rb.DeviceScene(host, device=0, honour_env=False, guard_dynamic_margins=1)
        fb, t = static.render_to_host(cam)
        assert t.guarded == 1 and t.guard_dynamic == 0 and t.scene_in_lds == 1
        assert_same_frame(fb, want, f"half_extent {half}, static margins")
    assert seen == {0, 1}, "both sides of the limit"


def test_flagged_samples_resume_from_the_flagged_ray(rtiow):
    """rt_config.resume_flagged: the exact re-walk of a flagged sample goes on from the ray that was flagged (its path's state is left
    in a table of the handle) instead of redoing the sample from the camera — the same frame, which is the oracle's: with the few
    flags of the default walk, with a stack so short that a sixth of the samples is flagged at every depth of their paths (far
    more than the table has slots: the others restart), over several passes, and with the primary-visibility pass off."""
    host, _ = rtiow
    cam = rb.rtiow_camera(320, 180, 48, 50)
    want = ob.render(host, cam, threads=8)
    for kw in (dict(), dict(stack_levels=3), dict(stack_levels=3, pass_spp=16), dict(stack_levels=4, primary_visibility=-1), dict(sphere_only_kernel=-1, stack_levels=3)):
        times = {}
        for resume in (0, -1):
            dev = rb.DeviceScene(host, device=0, honour_env=False, resume_flagged=resume, **kw)
            dev.render_to_host(cam)
            fb, t = dev.render_to_host(cam)
            assert t.guarded == 1 and t.flagged_samples > 0
            assert_same_frame(fb, want, f"resume_flagged={resume}, {kw}")
            times[resume] = (t.rework_ms, t.flagged_samples)
        # (which samples a short stack flags depends on which lanes share a wave's leaf steps — a few in 200 000 differ from run to run)
        assert abs(times[0][1] - times[-1][1]) <= 0.01 * times[0][1]


def test_candidate_lists_are_reused_for_the_same_view(rtiow):
    """The per-pixel candidate lists and the fetch order are kept with the handle: a call with the same camera, image, shard and
    tree on the same stream (the next batch of a progressive render) does not make them again, any other call does — frames are the
    oracle's in every order of views."""
    host, _ = rtiow
    dev = rb.DeviceScene(host, device=0, honour_env=False)
    a, b = rb.rtiow_camera(160, 90, 8, 50), rb.make_camera(160, 90, 35.0, (-9, 4, 6), (0, 0.5, 0), (0.7, 0.8, 1.0), 8, 50)
    more = rb.rtiow_camera(160, 90, 20, 50)        # the view of `a`, more samples: the lists do not depend on the sample count
    want = {id(c): ob.render(host, c, threads=8) for c in (a, b, more)}
    times = []
    for cam in (a, a, b, a, more, more):
        fb, t = dev.render_to_host(cam)
        assert t.guarded == 1 and t.primary_visibility == 1
        assert_same_frame(fb, want[id(cam)], "view sequence")
        times.append(t.primary_ms)
    shard = rb.Shard(8, 2, 1)
    for _ in range(2):
        fb, t = dev.render_to_host(a, shard)
        rows = np.concatenate([want[id(a)][r:r + 8] for r in range(8, 90, 16)])
        assert_same_frame(fb, rows, "row shard of the same view")
    # (a repeated view — the second call, and `more` after `a` — costs the per-sample pass alone)
    assert times[1] < 0.5 * times[0] and times[4] < 0.5 * times[3] and times[5] < 0.5 * times[3], times
    # … unless the caller wants every call to do all of a frame's work (what bench.py asks for)
    every = rb.DeviceScene(host, device=0, honour_env=False, reuse_view_lists=-1)
    again = [every.render_to_host(a) for _ in range(2)]
    assert_same_frame(again[1][0], want[id(a)], "lists made again")
    assert again[1][1].primary_ms > 0.5 * again[0][1].primary_ms


def test_front_primitives_change_nothing_but_the_time(test_config_text):
    """rt_config.guard_front_primitives: primitives that span the scene (S-rtiow's ground sphere; the ground sphere and the
    floor quad of the textured scene; the floor of the reference's config scene) are not leaves of the guarded walk's tree —
    every ray tests them as it is armed, the per-pixel candidate lists take them from the handle — and -1 keeps every primitive
    in the tree.  Same frame either way, which is the oracle's: sphere-only kernel, general kernel (planes, textures), the
    distance-aware kernels, with and without the primary-visibility pass, by-batch and by-pixel."""
    cases = [
        ("S-rtiow", rb.HostScene.rtiow(), rb.rtiow_camera(200, 112, 20, 50), dict(), 1),
        ("S-rtiow, camera rays walk", rb.HostScene.rtiow(), rb.rtiow_camera(200, 112, 12, 50), dict(primary_visibility=-1), 1),
        ("S-rtiow + textured quad", rb.HostScene.rtiow(half_extent=6, textured_quad=True, texture_size=64), rb.rtiow_camera(160, 90, 130, 50), dict(), 2),
        ("S-rtiow + textured quad, distance-aware margins", rb.HostScene.rtiow(half_extent=6, textured_quad=True, texture_size=64),
         rb.rtiow_camera(160, 90, 16, 50), dict(guard_dynamic_margins=2), 2),
        ("S-rtiow + textured quad from global memory", rb.HostScene.rtiow(half_extent=6, textured_quad=True, texture_size=64),
         rb.rtiow_camera(160, 90, 16, 50), dict(guard_dynamic_margins=2, scene_in_lds=0), 2),
    ]
    host = rb.HostScene.from_config(test_config_text)
    cases.append(("config scene", host, host.frame_camera(0), dict(), None))
    for what, host, cam, kw, want_front in cases:
        want = ob.render(host, cam, threads=8)
        front = rb.DeviceScene(host, device=0, honour_env=False, **kw)
        fb, t = front.render_to_host(cam)
        assert t.guarded == 1 and (want_front is None or t.front_primitives == want_front), (what, t.guarded, t.front_primitives)
        assert_same_frame(fb, want, what)
        leaves = rb.DeviceScene(host, device=0, honour_env=False, guard_front_primitives=-1, **kw)
        fb0, t0 = leaves.render_to_host(cam)
        assert t0.guarded == 1 and t0.front_primitives == 0, what
        assert_same_frame(fb0, want, what + ", every primitive a leaf")


def test_frame_sizes_from_one_pixel_to_the_limit():
    """rt_render's limits and corner sizes through the sphere-only kernel: the largest frame it accepts (2^24 pixels), 4K, one
    pixel, one sample per pixel (the index arithmetic's d == 1 case) — first, middle and last image row against the oracle."""
    host = rb.HostScene.rtiow()
    for (w, h, spp) in ((4096, 4096, 2), (3840, 2160, 4), (64, 64, 1), (1, 1, 3), (7, 3, 65)):
        cam = rb.rtiow_camera(w, h, spp, 50)
        dev = rb.DeviceScene(host, device=0, honour_env=False)
        fb, t = dev.render_to_host(cam)
        assert t.guarded == 1 and t.sphere_only == 1
        for r in sorted({0, h // 2, h - 1}):
            want = ob.render(host, cam, row0=r, row1=r + 1, threads=8)
            assert np.array_equal(want.view(np.uint32), fb[r:r + 1].view(np.uint32)), (w, h, spp, r)


def test_overlapped_rewalk_gives_the_same_frame():
    """rt_config.overlap_rework: by default the exact re-walk and the accumulation of the pixels it touches run on the handle's
    second stream beside the accumulation of all other pixels; -1 runs them one after the other.  Same frame (the oracle's),
    also over several passes and with a stack so short that a sixth of the samples is flagged."""
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(256, 144, 200, 50)
    want = ob.render(host, cam, threads=8)
    for kw, what in ((dict(), "default"), (dict(pass_spp=64), "four passes"), (dict(pass_spp=64, stack_levels=3), "four passes, short stack")):
        on = rb.DeviceScene(host, device=0, honour_env=False, **kw)
        fb, t = on.render_to_host(cam)
        assert t.guarded == 1 and t.flagged_samples > 0
        assert_same_frame(fb, want, "overlapped, " + what)
        off = rb.DeviceScene(host, device=0, honour_env=False, overlap_rework=-1, **kw)
        fb2, t2 = off.render_to_host(cam)
        assert t2.flagged_samples > 0          # (not necessarily the same count: which samples a parked test flags depends on when the wave ran its leaf steps)
        assert_same_frame(fb2, want, "sequential, " + what)
    # the same handle again (marks and lists of the previous frame must not leak into the next)
    fb3, _ = on.render_to_host(cam)
    assert_same_frame(fb3, want, "second frame on the same handle")


def test_guarded_walk_flags_and_rewalks(rtiow, force_guarded):
    """The guarded near-first walk hands a small share of the samples (far origins, hits in front of
    their own leaf box, a full stack) to the exact walk; with a 2-entry stack it hands over many
    more — the frame is the oracle's either way."""
    host, dev = rtiow
    cam = rb.rtiow_camera(480, 270, 16, 50)
    n = 480 * 270 * 16
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.scene_in_lds == 1
    assert 0 < t.flagged_samples < 0.02 * n, t.flagged_samples
    rows = ob.render(host, cam, row0=100, row1=140, threads=8)
    assert_same_frame(fb[100:140], rows, "guarded walk")
    try:
        dev.configure(stack_levels=2)
        fb2, t2 = dev.render_to_host(cam)
        assert t2.guarded == 1 and t2.flagged_samples > 4 * t.flagged_samples
        assert_same_frame(fb2, fb, "2-entry stack")
        # a flagged-sample list that overflows its capacity makes the exact walk redo every sample
        dev.configure(flag_capacity=1000)
        fb3, t3 = dev.render_to_host(cam)
        assert t3.guarded == 1 and t3.flagged_samples > 1000
        assert_same_frame(fb3, fb, "overflowed flag list")
    finally:
        dev.configure(stack_levels=0, flag_capacity=0)


def test_guarded_scene_handles_are_independent_and_reusable():
    """Two scene handles alive at once, renders of growing and shrinking sizes on each (slab and flag
    list regrow), an asynchronous render whose timing is read later: all frames are the oracle's."""
    import torch
    a = rb.HostScene.rtiow()
    b = rb.HostScene.rtiow(seed=777, half_extent=9)
    da, dbv = rb.DeviceScene(a, device=0), rb.DeviceScene(b, device=0)
    for (w, h, spp) in ((64, 40, 2), (300, 170, 3), (48, 30, 70)):
        for host, dev in ((a, da), (b, dbv)):
            cam = rb.rtiow_camera(w, h, spp, 50)
            fb, t = dev.render_to_host(cam)
            assert t.guarded == 1
            assert_same_frame(fb, ob.render(host, cam, threads=8), f"{w}x{h}x{spp}")
    cam = rb.rtiow_camera(200, 100, 5, 50)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f1 = torch.zeros((100, 200, 3), dtype=torch.float32, device="cuda:0")
    f2 = torch.zeros((100, 200, 3), dtype=torch.float32, device="cuda:0")
    da.render(cam, f1.data_ptr(), stream=s1.cuda_stream, sync=False)         # two scenes, two streams, in flight together
    dbv.render(cam, f2.data_ptr(), stream=s2.cuda_stream, sync=False)
    s1.synchronize(); s2.synchronize()
    ta, tb = da.last_timing(), dbv.last_timing()
    assert ta.guarded == 1 and tb.guarded == 1 and ta.trace_ms > 0 and tb.rework_ms > 0
    assert_same_frame(f1.cpu().numpy(), ob.render(a, cam, threads=8), "async scene a")
    assert_same_frame(f2.cpu().numpy(), ob.render(b, cam, threads=8), "async scene b")


def test_guarded_walk_steps_aside_or_is_timed_when_it_flags(rtiow):
    """What RT_TRAVERSAL_AUTO does with a guarded walk that keeps handing samples back; the frames are the same bits whichever
    walk made them.  (a) A 2-entry stack on S-rtiow flags a third of the samples: the pass gives up in the launch, the exact
    walk renders it, the handle steps aside.  (b) A scene that flags about 4 % (332 overlapping spheres): above 0.4 % the
    handle MEASURES — the next frame is the exact walk's, and whichever cost less per sample stays.  A caller who forces a
    walk gets that walk, no measuring."""
    host = rb.HostScene.rtiow()
    # (with the ground sphere in the tree: as a front primitive it never costs a stack entry, and two entries flag a quarter only)
    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_AUTO, guard_keep=0, guard_front_primitives=-1)
    cam = rb.rtiow_camera(240, 135, 8, 50)
    want = ob.render(host, cam, threads=8)
    dev.configure(stack_levels=2)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.abandoned_passes == 1 and t.guard_paused == 1, (t.flagged_samples, t.abandoned_passes)
    assert_same_frame(fb, want, "frame whose guarded pass gave up")
    dev.configure(stack_levels=0)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 0 and t.flagged_samples == 0
    assert_same_frame(fb, want, "next frame, exact walk")

    host, cam, n = _stress_scene(2, 14, 16, 640, 360)
    assert n == 332
    exact = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_EXACT)
    want, _ = exact.render_to_host(cam)
    assert_same_frame(want[100:104], ob.render(host, cam, row0=100, row1=104, threads=8), "exact walk against the oracle")
    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_AUTO, guard_keep=0)
    fb, t = dev.render_to_host(cam)
    share = t.flagged_samples / (640 * 360 * 16)
    assert t.guarded == 1 and t.abandoned_passes == 0 and t.guard_paused == 0 and 0.004 < share < 0.09, share
    assert_same_frame(fb, want, "flagged frame")
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 0 and t.flagged_samples == 0, "the frame after it is the exact walk's (timed against the guarded one)"
    assert_same_frame(fb, want, "measuring frame")
    fb, t3 = dev.render_to_host(cam)
    assert t3.guarded == (0 if t3.guard_paused else 1), "… and the faster walk stays"
    assert_same_frame(fb, want, "third frame")
    fb, t4 = dev.render_to_host(cam)
    assert t4.guarded == t3.guarded, "no further measuring"
    forced = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_GUARDED, guard_keep=0)
    for k in range(3):
        fb, t = forced.render_to_host(cam)
        assert t.guarded == 1, "a forced walk is not second-guessed by timing"
    assert_same_frame(fb, want, "forced guarded")


def _stress_scene(seed, trial, spp, width, height):
    """Scene `trial` of tools/guard_stress.py's sequence for `seed`."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    import guard_stress
    for k, sph, pl, mats, cam, spread in guard_stress.scenes(seed, trial + 1, spp, width, height):
        if k == trial:
            return rb.HostScene.from_arrays(sph, pl, mats), cam, sph.shape[0]


def test_heavily_flagged_scene_costs_little_more_than_the_exact_walk():
    """VERDICT r03 W3.  325 overlapping spheres, 56 % of the samples flagged by the guarded walk (scenes like it cost round 3 fifteen
    times the exact walk: one atomic per flagged sample on one counter).  Now a wave appends its flagged samples together (in
    chunks of 64 slots once it keeps flagging), and the pass gives up in the launch once the flagged share of what has been handed out passes rt_config.guard_bail_share: the
    exact walk renders the whole pass, the frame is the exact walk's bit for bit, and the handle steps aside for its next
    frames WITHOUT anybody calling rt_last_timing."""
    import torch
    host, cam, n = _stress_scene(9, 4, 48, 1280, 720)
    assert n == 325
    exact = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_EXACT)
    exact.render_to_host(cam)
    want, te = exact.render_to_host(cam)
    exact_ms = min(te.kernel_ms, exact.render_to_host(cam)[1].kernel_ms)
    rows = ob.render(host, cam, row0=300, row1=302, threads=8)
    assert_same_frame(want[300:302], rows, "exact walk against the oracle")

    kept = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)       # no bail-out: the walk's real flagged share
    fb, tk = kept.render_to_host(cam)
    assert tk.guarded == 1 and tk.abandoned_passes == 0 and tk.flagged_samples > 0.3 * 1280 * 720 * 48, tk.flagged_samples
    assert_same_frame(fb, want, "guarded walk kept, every flagged sample re-walked from the list")
    assert tk.kernel_ms < 4.0 * exact_ms, (tk.kernel_ms, exact_ms)          # (was 15 x)

    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_AUTO, guard_keep=0)                                                 # the defaults
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.abandoned_passes == 1 and t.guard_paused == 1
    assert_same_frame(fb, want, "abandoned pass")
    assert t.kernel_ms <= 1.5 * exact_ms, (t.kernel_ms, exact_ms)
    fb, t2 = dev.render_to_host(cam)
    assert t2.guarded == 0
    assert_same_frame(fb, want, "frame after the abandoned one")

    # an asynchronous caller that never asks for timings: the second frame already runs on the exact walk
    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_AUTO, guard_keep=0)
    f = torch.zeros((720, 1280, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream()
    t = dev.render(cam, f.data_ptr(), stream=stream.cuda_stream, sync=False)
    assert t.guarded == 1
    stream.synchronize()
    t = dev.render(cam, f.data_ptr(), stream=stream.cuda_stream, sync=False)
    assert t.guarded == 0, "the handle read what the first frame left in host memory"
    stream.synchronize()
    assert_same_frame(f.cpu().numpy(), want, "asynchronous caller")
    # … and one that queues frames without ever waiting: the judgement arrives a few frames late, never wrong
    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_AUTO, guard_keep=0)
    walks = []
    for k in range(8):
        walks.append(dev.render(cam, f.data_ptr(), stream=stream.cuda_stream, sync=False).guarded)
    stream.synchronize()
    assert walks[0] == 1 and walks[-1] == 0, walks
    assert_same_frame(f.cpu().numpy(), want, "eight frames queued back to back")


def test_a_pass_that_flags_a_third_of_its_samples_appends_them_in_chunks():
    """690 overlapping spheres with the camera among them: 35 % of the samples flagged, and tables that leave LDS no room for
    anything else.  One atomic per wave and shade step on the list's counter made the guarded launch of this frame 78 ms against
    the exact walk's 14 (the counter takes one atomic per ~11 ns, whoever sends it); now a wave that keeps flagging reserves 64
    slots at a time and fills the ones it does not use with holes the re-walk passes over (rt_kernel.hip.inc, flag_collect): the
    launch takes 11.5 ms.  The frame is the exact walk's bit for bit, the reported count is the samples flagged (slots less holes),
    and by default the pass is given up early: the frame takes 1.33 x the exact walk's time (was 2.34 x)."""
    host, cam, n = _stress_scene(22, 32, 48, 1280, 720)
    assert n == 690
    total = 1280 * 720 * 48
    exact = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_EXACT)
    exact.render_to_host(cam)
    want, te = exact.render_to_host(cam)
    exact_ms = min(te.kernel_ms, exact.render_to_host(cam)[1].kernel_ms)
    rows = ob.render(host, cam, row0=400, row1=402, threads=8)
    assert_same_frame(want[400:402], rows, "exact walk against the oracle")

    kept = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
    fb, tk = kept.render_to_host(cam)
    assert tk.guarded == 1 and tk.abandoned_passes == 0
    assert 0.34 * total < tk.flagged_samples < 0.37 * total, tk.flagged_samples / total        # (35.34 %: holes are not counted)
    assert_same_frame(fb, want, "guarded walk kept: a third of the frame re-walked from a list with holes")
    assert tk.trace_ms < 1.5 * exact_ms, (tk.trace_ms, exact_ms)            # (was 5.4 x)
    fb, tk2 = kept.render_to_host(cam)
    assert abs(int(tk2.flagged_samples) - int(tk.flagged_samples)) < 0.001 * total
    assert_same_frame(fb, want, "guarded walk kept, second frame")

    # … the same in three passes (each launch starts its waves' chunks afresh, each pass has its own counters), on a row shard, on a tile
    _, cam3, _ = _stress_scene(22, 32, 192, 640, 360)                  # (the same view at a quarter of the pixels, four times the samples)
    want3, _ = exact.render_to_host(cam3)
    many = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_GUARDED, guard_keep=1, workspace_bytes=640 * 360 * 12 * 64)
    fb, tm = many.render_to_host(cam3)
    assert tm.trace_launches == 3 and tm.abandoned_passes == 0
    assert 0.3 * total < tm.flagged_samples < 0.4 * total, tm.flagged_samples / total
    assert_same_frame(fb, want3, "three passes")
    shard = rb.Shard(8, 3, 1)
    part, ts = kept.render_to_host(cam, shard)
    rows_of_shard = np.concatenate([np.arange(b, min(b + 8, 720)) for b in range(8, 720, 24)])
    assert ts.flagged_samples > 0.2 * len(rows_of_shard) * 1280 * 48
    assert_same_frame(part, want[rows_of_shard], "row shard 1 of 3")
    tile, tt = kept.render_tile_to_host(cam, 333, 201, 517, 263)
    assert tt.flagged_samples > 0
    assert_same_frame(tile, want[201:201 + 263, 333:333 + 517], "tile")

    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_AUTO, guard_keep=0)                    # the defaults
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.abandoned_passes == 1 and t.guard_paused == 1
    assert t.flagged_samples < 0.12 * total, t.flagged_samples / total      # given up early: 6 % of the pass on the list, plus what was in flight
    assert_same_frame(fb, want, "pass given up")
    assert t.kernel_ms <= 1.6 * exact_ms, (t.kernel_ms, exact_ms)            # (measured 1.33; was 2.34)


def test_guarded_walk_far_camera_and_ties(force_guarded):
    """Cases the guards exist for.  (a) A camera far outside the distance the box inflation was
    sized for: every primary ray takes the far-origin test.  (b) Coincident and overlapping
    spheres: exact ties of the hit distance, which the reference resolves by visit order."""
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    cam = rb.make_camera(160, 90, 3.0, (400.0, 90.0, 60.0), (0, 0, 0), (0.7, 0.8, 1.0), 4, 50)
    want = ob.render(host, cam, threads=8)
    dev.configure(guard_repack=0)                   # margins as packed: the far-origin test has to catch the primary rays
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.flagged_samples > 1000
    assert_same_frame(fb, want, "far camera, far-origin test")
    dev.configure(guard_repack=1)
    fb, t2 = dev.render_to_host(cam)                # default: the tree is re-packed with margins for this camera
    assert t2.guarded == 1 and t2.flagged_samples < t.flagged_samples // 4
    assert_same_frame(fb, want, "far camera, re-packed tree")
    near = rb.rtiow_camera(160, 90, 4, 50)           # and the re-packed tree serves the usual camera as well
    fb, t3 = dev.render_to_host(near)
    assert t3.guarded == 1
    assert_same_frame(fb, ob.render(host, near, threads=8), "near camera after a re-pack")

    mats = [_material(0, albedo=(0.8, 0.3, 0.3)), _material(0, albedo=(0.2, 0.9, 0.3)), _material(1, albedo=(0.9, 0.9, 0.9), fuzz=0.1),
            _material(2, ir=1.5)]
    spheres = np.array([[0, 0, 0, 1, 0], [0, 0, 0, 1, 1],                      # the same sphere twice, two materials
                        [2, 0, 0, 1, 2], [2, 0, 0, 1, 3],                      # again, metal and glass
                        [0, 2.5, 0, 1, 1], [0, 2.5, 0.75, 1, 0],               # overlapping
                        [0, 0, -101, 100, 0]], dtype=np.float32)
    host = rb.HostScene.from_arrays(spheres, np.zeros((0, 11), np.float32), mats)
    dev = rb.DeviceScene(host, device=0)
    cam = rb.make_camera(200, 120, 40.0, (6, 5, 2.5), (0.7, 0.8, 0), (0.6, 0.7, 0.9), 6, 20)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.flagged_samples > 0          # the ties
    assert_same_frame(fb, ob.render(host, cam, threads=8), "coincident spheres")


@pytest.fixture
def force_guarded():
    """rt_config for every handle the test makes or re-configures: guarded walk whatever the scene's size, and kept even
    after a frame that flags more than 2 % of its samples (such a handle would otherwise switch to the exact walk)."""
    before = dict(rb.DEFAULTS)
    rb.DEFAULTS.update(traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
    yield
    rb.DEFAULTS.clear()
    rb.DEFAULTS.update(before)


def test_guarded_walk_on_plane_scenes(config_scene, force_guarded):
    """Scenes with quads, ellipses and triangles through the guarded walk (asked for explicitly:
    these trees are small): the config scene at C1, and random mixed scenes with axis-aligned
    (thin-box) and tilted planes."""
    host, dev = config_scene
    base = host.frame_camera(0)
    cam = rb.make_camera(400, 225, 50.0, list(base.origin.e), (0.0, 0.0, 4.5), (0, 0, 0), 16, 10)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1, dev.guard_reason()
    assert_same_frame(fb, ob.render(host, cam, threads=8), "config scene, guarded")
    rng = np.random.default_rng(4242)
    for trial in range(8):
        host = _random_scene(rng, int(rng.integers(1, 80)), int(rng.integers(1, 40)), axis_aligned=trial % 2 == 0)
        dev = rb.DeviceScene(host, device=0)
        eye = rng.uniform(-9, 9, 3)
        cam = rb.make_camera(int(rng.integers(33, 160)), int(rng.integers(17, 90)), float(rng.uniform(20, 100)), eye, rng.uniform(-2, 2, 3),
                             rng.uniform(0, 1, 3), int(rng.integers(1, 7)), int(rng.integers(1, 30)))
        fb, t = dev.render_to_host(cam)
        assert dev.guard_reason() == "" and t.guarded == 1
        assert_same_frame(fb, ob.render(host, cam, threads=8), f"mixed scene {trial}, guarded")


def test_device_built_tree_gives_the_same_frames(force_guarded):
    """rt_config.tree_build = RT_BUILD_DEVICE_LBVH: the guarded walk's tree is an LBVH built on the GPU (rt_build.hip).  Any tree
    over the inflated leaf boxes must give the oracle's frame: S-rtiow (one huge + 485 small
    spheres), mixed sphere/plane scenes, scenes of one and two primitives, equal Morton keys
    (coincident spheres)."""
    rb.DEFAULTS.update(tree_build=rb.BUILD_DEVICE_LBVH)
    try:
        host = rb.HostScene.rtiow()
        dev = rb.DeviceScene(host, device=0)
        cam = rb.rtiow_camera(320, 180, 8, 50)
        fb, t = dev.render_to_host(cam)
        assert t.guarded == 1
        assert_same_frame(fb, ob.render(host, cam, threads=8), "S-rtiow on a device-built tree")
        rng = np.random.default_rng(31337)
        mats = [_material(0, albedo=(0.7, 0.6, 0.5)), _material(1, albedo=(0.8, 0.8, 0.9), fuzz=0.2), _material(2, ir=1.4)]
        cases = [np.array([[0, 0, 0, 1, 0]], np.float32),                                   # one primitive: no tree at all
                 np.array([[0, 0, 0, 1, 0], [1.5, 0.2, 0.1, 0.7, 1]], np.float32),           # two
                 np.array([[0, 0, 0, 1, 0]] * 5 + [[2, 0, 0, 0.5, 2]] * 3, np.float32)]      # identical centres: equal keys
        for k, spheres in enumerate(cases):
            host = rb.HostScene.from_arrays(spheres, np.zeros((0, 11), np.float32), mats)
            dev = rb.DeviceScene(host, device=0)
            cam = rb.make_camera(120, 80, 45.0, (5, 4, 2), (0.5, 0, 0), (0.5, 0.6, 0.8), 4, 12)
            fb, t = dev.render_to_host(cam)
            assert_same_frame(fb, ob.render(host, cam, threads=8), f"tiny scene {k} on a device-built tree")
        for trial in range(5):
            host = _random_scene(rng, int(rng.integers(2, 120)), int(rng.integers(0, 40)), axis_aligned=trial % 2 == 0)
            dev = rb.DeviceScene(host, device=0)
            cam = rb.make_camera(int(rng.integers(33, 160)), int(rng.integers(17, 90)), float(rng.uniform(20, 100)), rng.uniform(-9, 9, 3),
                                 rng.uniform(-2, 2, 3), rng.uniform(0, 1, 3), int(rng.integers(1, 7)), int(rng.integers(1, 30)))
            fb, t = dev.render_to_host(cam)
            assert t.guarded == 1
            assert_same_frame(fb, ob.render(host, cam, threads=8), f"mixed scene {trial} on a device-built tree")
    finally:
        rb.DEFAULTS.pop("tree_build", None)


def test_guarded_walk_random_sphere_scenes(force_guarded):
    """Sphere-only random scenes through the guarded walk: radii over 2.5 decades,
    overlaps, a huge ground sphere in half of them, cameras inside and far outside the cluster."""
    rng = np.random.default_rng(77)
    eligible = walked_guarded = 0
    for trial in range(12):
        n = int(rng.integers(2, 300))
        mats = [_material(int(rng.integers(0, 4)), albedo=rng.uniform(0.1, 1.0, 3), fuzz=float(rng.uniform(0, 0.7)),
                          ir=float(rng.uniform(1.1, 2.0)), absorption=rng.uniform(0, 0.6, 3) if rng.random() < 0.5 else (0, 0, 0),
                          emit=rng.uniform(0.5, 3.0, 3)) for _ in range(6)]
        spheres = np.zeros((n, 5), dtype=np.float32)
        spread = float(rng.choice([3.0, 10.0, 40.0]))
        spheres[:, :3] = rng.uniform(-spread, spread, (n, 3))
        spheres[:, 3] = 10.0 ** rng.uniform(-2.0, 0.5, n)
        spheres[:, 4] = rng.integers(0, len(mats), n)
        if trial % 2 == 0:
            spheres[0] = (0, 0, -1000 - spread, 1000, 0)
        host = rb.HostScene.from_arrays(spheres, np.zeros((0, 11), np.float32), mats)
        dev = rb.DeviceScene(host, device=0)
        eye = rng.uniform(-spread, spread, 3) * (20.0 if trial % 5 == 4 else 1.0)
        cam = rb.make_camera(int(rng.integers(40, 200)), int(rng.integers(30, 120)), float(rng.uniform(15, 90)), eye,
                             rng.uniform(-1, 1, 3), rng.uniform(0, 1, 3), int(rng.integers(1, 6)), int(rng.integers(1, 40)))
        fb, t = dev.render_to_host(cam)
        # tiny spheres scattered over a wide volume are not eligible (their margins would swallow the tree)
        assert dev.guard_reason() in ("", "margins exceed 64 radii for the smallest spheres")
        eligible += dev.guard_reason() == ""
        walked_guarded += int(t.guarded)      # (a camera too far out for the margins gets the exact walk for that call)
        assert_same_frame(fb, ob.render(host, cam, threads=8), f"sphere scene {trial}")
    assert eligible >= 6 and walked_guarded >= 4, (eligible, walked_guarded)


def test_stress_scene_whole_4k_frame():
    """BASELINE configs[4] geometry: ~100k spheres + a textured quad at 3840x2160, 2 spp: the WHOLE frame (8.3 M
    pixels, 16.6 M samples, index arithmetic at full size) against the oracle, through the default path (guarded walk
    with the proven margin, tables read through L1/L2) and through the exact walk alone."""
    host = rb.HostScene.rtiow(half_extent=158, textured_quad=True, texture_size=256)
    dev = rb.DeviceScene(host, device=0, honour_env=False)
    cam = rb.rtiow_camera(3840, 2160, 2, 50)
    want = ob.render(host, cam, threads=16)
    fb, t = dev.render_to_host(cam)
    assert t.scene_in_lds == 0 and t.guarded == 1 and t.guard_unproven == 0 and t.guard_dynamic == 1 and t.primary_visibility == 1
    assert_same_frame(fb, want, "4K frame, guarded walk with distance-aware margins")
    dev.configure(traversal=rb.TRAVERSAL_EXACT)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 0
    assert_same_frame(fb, want, "4K frame, exact walk")


def _random_scene(rng, n_spheres, n_planes, axis_aligned=False):
    mats = []
    for _ in range(6):
        t = int(rng.integers(0, 4))
        mats.append(_material(t, albedo=rng.uniform(0.1, 1.0, 3), fuzz=float(rng.uniform(0, 0.7)), ir=float(rng.uniform(1.1, 2.0)),
                              absorption=rng.uniform(0, 0.6, 3) if rng.random() < 0.5 else (0, 0, 0),
                              emit=rng.uniform(0.5, 3.0, 3) if t == 3 else (0, 0, 0)))
    spheres = np.zeros((n_spheres, 5), dtype=np.float32)
    spheres[:, :3] = rng.uniform(-6, 6, (n_spheres, 3))
    spheres[:, 3] = rng.uniform(0.05, 1.5, n_spheres)
    spheres[:, 4] = rng.integers(0, len(mats), n_spheres)
    planes = np.zeros((n_planes, 11), dtype=np.float32)
    planes[:, :3] = rng.uniform(-6, 6, (n_planes, 3))
    if axis_aligned:     # boxes thin in one axis, normals along axes: exercises the 1e-4 padding and 1/0 slabs
        for k in range(n_planes):
            a = int(rng.integers(0, 3))
            u = np.zeros(3); v = np.zeros(3)
            u[(a + 1) % 3] = rng.uniform(1, 4); v[(a + 2) % 3] = rng.uniform(1, 4)
            planes[k, 3:6] = u; planes[k, 6:9] = v
    else:
        planes[:, 3:6] = rng.uniform(-3, 3, (n_planes, 3))
        planes[:, 6:9] = rng.uniform(-3, 3, (n_planes, 3))
    planes[:, 9] = rng.integers(0, len(mats), n_planes)
    planes[:, 10] = rng.integers(0, 3, n_planes)
    return rb.HostScene.from_arrays(spheres, planes, mats)


def test_random_scenes_bit_identical():
    """Randomised scenes (all materials, all plane types, absorbing glass, lights, random and
    axis-aligned geometry, cameras inside the scene, rays with zero direction components):
    per-pixel sums bit-identical to the oracle."""
    rng = np.random.default_rng(2024)
    for trial in range(10):
        host = _random_scene(rng, int(rng.integers(1, 60)), int(rng.integers(0, 25)), axis_aligned=trial % 3 == 0)
        dev = rb.DeviceScene(host, device=0)
        eye = rng.uniform(-9, 9, 3)
        if trial % 4 == 1:
            eye = np.array([0.0, 8.0, 0.5])       # looks along -y: pixel columns with d.x == 0 exactly
            target = np.array([0.0, 0.0, 0.5])
        else:
            target = rng.uniform(-2, 2, 3)
        cam = rb.make_camera(int(rng.integers(33, 160)), int(rng.integers(17, 90)), float(rng.uniform(20, 100)), eye, target,
                             rng.uniform(0, 1, 3), int(rng.integers(1, 7)), int(rng.integers(1, 30)))
        fb, _ = dev.render_to_host(cam)
        want = ob.render(host, cam, threads=8)
        assert_same_frame(fb, want, f"random scene {trial}")


def _oracle_hits(host, origins, directions):
    lib = ob.lib()
    n = origins.shape[0]
    hit = np.zeros(n, dtype=np.int32)
    t = np.zeros(n, dtype=np.float32)
    prim = np.zeros(n, dtype=np.int32)
    tt, ty, ix = C.c_float(), C.c_int(), C.c_int()
    for k in range(n):
        o = np.ascontiguousarray(origins[k], dtype=np.float32)
        d = np.ascontiguousarray(directions[k], dtype=np.float32)
        if lib.orc_closest_hit(C.byref(host.desc), o.ctypes.data, d.ctypes.data, C.byref(tt), C.byref(ty), C.byref(ix)):
            hit[k], t[k], prim[k] = 1, tt.value, 2 * ix.value + ty.value
    return hit, t, prim


def test_hit_scene_on_crafted_rays():
    """hit_bvh / AABB::hit / hit_sphere / hit_plane at the ray level (rt_closest_hits against the
    oracle's hit_scene), on the inputs where float semantics bite: direction components that are
    exactly zero (1/0 = inf slabs), origins exactly on box planes (0 * inf = NaN), origins inside
    and on spheres, tangent rays, rays along plane surfaces, huge and tiny directions, rays that
    start behind everything."""
    rng = np.random.default_rng(99)
    mats = [_material(0, albedo=(0.5, 0.5, 0.5))]
    spheres = np.array([[0, 0, 0, 1, 0], [3, 0, 0, 0.5, 0], [0, 4, 0, 2, 0], [0, 0, -1000, 999, 0], [2, 2, 2, 0.05, 0],
                        [-3, -3, 0.5, 0.5, 0], [5, 5, 5, 1e-3, 0]], dtype=np.float32)
    planes = np.array([[-2, -2, 3, 4, 0, 0, 0, 4, 0, 0, 0],          # axis-aligned quad z = 3
                       [-2, -2, -3, 4, 0, 0, 0, 4, 0, 0, 2],         # triangle z = -3
                       [4, -1, -1, 0, 2, 0, 0, 0, 2, 0, 1],          # ellipse x = 4
                       [-6, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0]], dtype=np.float32)     # tilted quad
    host = rb.HostScene.from_arrays(spheres, planes, mats)
    dev = rb.DeviceScene(host, device=0)
    O, D = [], []
    axes = np.eye(3, dtype=np.float32)
    for c in spheres[:, :3]:
        for a in axes:
            for sgn in (1.0, -1.0):
                O.append(c + sgn * 7 * a); D.append(-sgn * a)                      # through the centre along an axis: two zero components
                O.append(c + sgn * 7 * a + np.roll(a, 1)); D.append(-sgn * a)      # offset by exactly the unit sphere's radius: tangent
        O.append(c.copy()); D.append(np.array([1, 0, 0], np.float32))              # origin at the centre
        O.append(c + np.array([0.25, 0, 0], np.float32)); D.append(np.array([0, 1, 1], np.float32))   # inside
    for s in spheres:                                                               # origins exactly on the leaf box faces
        lo, hi = s[:3] - s[3], s[:3] + s[3]
        for a in range(3):
            p = s[:3].copy(); p[a] = lo[a]
            d = np.ones(3, np.float32); d[a] = 0.0
            O.append(p.copy()); D.append(d.copy())                                  # on the face, moving inside the face plane
            p[a] = hi[a]; O.append(p.copy()); D.append(-d)
    for z in (3.0, -3.0):                                                           # along and across the flat quads' padded boxes
        O.append(np.array([-5, 0, z], np.float32)); D.append(np.array([1, 0, 0], np.float32))
        O.append(np.array([0, 0, z + 5], np.float32)); D.append(np.array([0, 0, -1], np.float32))
        O.append(np.array([0, 0, z], np.float32)); D.append(np.array([0.3, 0.1, 0], np.float32))
        O.append(np.array([-2, -2, z + 1], np.float32)); D.append(np.array([0, 0, -1], np.float32))     # exactly through a corner
        O.append(np.array([2, -2, z + 1], np.float32)); D.append(np.array([0, 0, -2.5], np.float32))     # exactly through an edge end
    for scale in (1e-20, 1e-6, 1e6, 1e18):                                          # tiny / huge direction lengths
        O.append(np.array([-9, 0.1, 0.2], np.float32)); D.append(np.array([scale, 0, 0], np.float32))
        O.append(np.array([0.3, 0.2, 40], np.float32)); D.append(np.array([0, scale * 0.01, -scale], np.float32))
    O.append(np.array([0, 0, 0], np.float32)); D.append(np.array([0, 0, 0], np.float32))       # null direction
    O.append(np.array([50, 50, 50], np.float32)); D.append(np.array([1, 1, 1], np.float32))    # everything behind
    for _ in range(3000):                                                           # plus random rays, some axis-parallel
        o = rng.uniform(-8, 8, 3).astype(np.float32)
        d = rng.normal(size=3).astype(np.float32)
        if rng.random() < 0.3:
            d[int(rng.integers(0, 3))] = 0.0
        if rng.random() < 0.1:
            d[int(rng.integers(0, 3))] = -0.0
        O.append(o); D.append(d)
    O = np.array(O, dtype=np.float32); D = np.array(D, dtype=np.float32)
    hit, t, prim = dev.closest_hits(O, D)
    ohit, ot, oprim = _oracle_hits(host, O, D)
    assert np.array_equal(hit, ohit), np.where(hit != ohit)[0][:10]
    h = hit == 1
    assert np.array_equal(t[h].view(np.uint32), ot[h].view(np.uint32)), np.where(t[h] != ot[h])[0][:10]
    assert np.array_equal(prim[h], oprim[h])
    assert h.sum() > 1000 and (~h).sum() > 500
    # the same on the benchmark scene (ground sphere of radius 1000 under tangent small spheres)
    host2 = rb.HostScene.rtiow()
    dev2 = rb.DeviceScene(host2, device=0)
    O2 = rng.uniform(-12, 12, (6000, 3)).astype(np.float32); O2[:, 2] = np.abs(O2[:, 2]) * 0.2 + 1e-3
    D2 = rng.normal(size=(6000, 3)).astype(np.float32)
    D2[::5, 2] = -np.abs(D2[::5, 2])
    hit, t, prim = dev2.closest_hits(O2, D2)
    ohit, ot, oprim = _oracle_hits(host2, O2, D2)
    assert np.array_equal(hit, ohit)
    h = hit == 1
    assert np.array_equal(t[h].view(np.uint32), ot[h].view(np.uint32)) and np.array_equal(prim[h], oprim[h])


def test_developer_build_checks_and_retired_experiments():
    """The developer build (make dev → librtp_amd_dev.so: the shipped library plus the rt_debug_* entry points and the tripwire)
    through tests/dev_build_checks.py, in ONE child process that loads that library instead of the shipped one: recip() /
    sqrt_cr() against the compiler's correctly rounded forms on all 2^32 floats ON THIS DEVICE, the shared-reciprocal sphere roots
    on 2^32 sampled operand sets, the tripwire.  The shipped library must not carry any of it, and refuses the retired experiments
    (RT_KERNEL_WAVEFRONT, rt_config.wide_nodes = 1)."""
    import subprocess
    import sys
    lib = rb.amd_lib()
    assert b"dev=0" in lib.rt_version_string() and b"parity=1" in lib.rt_version_string()
    assert not hasattr(lib, "rt_debug_check_fast_math") and not hasattr(lib, "rt_debug_check_sphere_roots")
    assert not hasattr(lib, "rt_debug_build_lbvh") and not hasattr(lib, "rt_debug_guard_leaves")
    assert not hasattr(lib, "rt_debug_math_eval") and not hasattr(lib, "rt_debug_fog_rays")
    host = rb.HostScene.rtiow()
    with pytest.raises(RuntimeError, match="retired"):
        rb.DeviceScene(host, device=0, honour_env=False, kernel=rb.KERNEL_WAVEFRONT).render_to_host(rb.rtiow_camera(32, 20, 2, 8))
    with pytest.raises(RuntimeError, match="retired"):
        rb.DeviceScene(host, device=0, honour_env=False, wide_nodes=1).render_to_host(rb.rtiow_camera(32, 20, 2, 8))
    dev_lib = os.path.join(os.path.dirname(HERE), "ray-tracing-practice_amd", "librtp_amd_dev.so")
    assert os.path.exists(dev_lib), "run __graft_entry__.build() (make -C ray-tracing-practice_amd dev)"
    env = dict(os.environ, RTP_AMD_LIB=dev_lib)
    from conftest import run_child
    res = run_child([sys.executable, "-m", "pytest", os.path.join(HERE, "dev_build_checks.py"), "-x", "-q", "-p", "no:cacheprovider"], 200, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "failed" not in res.stdout
