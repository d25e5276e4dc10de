"""The fetch-order table of the primary-visibility path (csrc/rt_primary.hip.inc, order_scatter_kernel): one 16-byte row per position
of the fetch order — the centre of the pixel on the image plane as camera_ray builds it, and the local pixel — read by every guarded
trace kernel where it starts a sample (map_fetch, csrc/rt_kernel.hip.inc).  A wrong row is a wrong camera ray or a sample stored under
a wrong name, so every frame here is compared bit for bit against the oracle, at the smallest shapes that reach each way the table
can be wrong: widths that are a multiple neither of 64 nor of 4, every kernel family that reads it, row shards with a partial last
band, several passes, an offset first sample, changing views on one handle, frames with no traced pixel and with nothing but traced
pixels, and a tile away from the image's corner.  Which kernels a frame took is read from rt_timing (as
tests/test_render_kernel_families.py does), so that a change of the dispatch cannot pass these by default.  No tolerance."""
import numpy as np
import pytest

import oracle_bindings as ob
import rtp_bindings as rb

pytestmark = pytest.mark.gpu

GUARDED = dict(traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
W, H = 67, 35          # the width is a multiple neither of 64 nor of 4; 35 rows in bands of 8: the last band has 3
SKY = (0.7, 0.8, 1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (bits(got) == bits(want)).all(axis=-1)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} pixels differ, max abs diff {np.abs(got - want).max()}"


def headline_kernels(dev, t):
    """The sphere-only octant kernel fed by the primary-visibility pass."""
    assert t.guarded == 1 and t.sphere_only == 1 and t.scene_in_lds == 1 and t.primary_visibility == 1, \
        (t.guarded, t.sphere_only, t.scene_in_lds, t.primary_visibility, dev.guard_reason())
    assert dev.trace_kernel_name() == "void rtk::render_kernel<true, false, false, false, true, true>(rtk::KParams)"


def view(eye, target, spp, vfov=20.0, w=W, h=H):
    return rb.make_camera(w, h, vfov, eye, target, SKY, spp, 50)


@pytest.fixture(scope="module")
def rtiow():
    return rb.HostScene.rtiow()


@pytest.fixture(scope="module")
def mixed():
    """The `mixed` scene of tests/test_render_kernel_families.py: a textured METAL quad, metal and diffuse spheres, absorbing glass."""
    host = rb.HostScene.rtiow(half_extent=4, textured_quad=True, texture_size=64)
    desc = host.desc
    assert desc.num_planes == 1 and desc.num_textures == 1
    mats = desc.materials
    types = [mats[k].type for k in range(desc.num_materials)]
    assert 1 in types and 2 in types, "the scene has METAL and DIELECTRIC materials"
    for k in range(desc.num_materials):
        if mats[k].type == 2:
            mats[k].absorption.e[:] = (0.9, 0.2, 0.05)
    return host


@pytest.fixture(scope="module")
def big():
    host = rb.HostScene.rtiow(half_extent=16)
    assert host.desc.num_spheres >= 785 and host.desc.num_planes == 0
    return host


@pytest.fixture(scope="module")
def wanted(rtiow):
    """The oracle's S-rtiow frames that more than one test needs, rendered once and shared read-only."""
    cams = {"100": rb.rtiow_camera(W, H, 100, 50), "8": rb.rtiow_camera(W, H, 8, 50), "5": rb.rtiow_camera(W, H, 5, 50)}
    frames = {k: ob.render(rtiow, c, threads=8) for k, c in cams.items()}
    for f in frames.values():
        f.setflags(write=False)
    return cams, frames


def test_rtiow_one_100_spp_pass(rtiow, wanted):
    """S-rtiow 67x35, 100 samples in one pass: the primary pass by pixel (from 96 samples per pixel and pass) and the sphere-only
    trace kernel: the two kernels of the headline frame."""
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cams["100"])
    headline_kernels(dev, t)
    assert t.trace_launches == 1, t.trace_launches
    assert t.traced_samples > 0, t.traced_samples
    assert_same_frame(fb, frames["100"], "S-rtiow 67x35x100")


def test_rtiow_5_spp_primary_pass_by_batch(rtiow, wanted):
    """5 samples per pixel: the primary pass works by batch of samples; the pass count (5) is no power of two."""
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cams["5"])
    headline_kernels(dev, t)
    assert_same_frame(fb, frames["5"], "S-rtiow 67x35x5")


def test_general_octant_kernel(mixed):
    """Plane, texture, glass and metal at 45x23x8: the general build of the octant kernel."""
    cam = rb.rtiow_camera(45, 23, 8, 50)
    dev = rb.DeviceScene(mixed, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.sphere_only == 0 and t.scene_in_lds == 1 and t.workgroup_size == 768 and t.primary_visibility == 1, \
        (t.guarded, t.sphere_only, t.scene_in_lds, t.workgroup_size, t.primary_visibility, dev.guard_reason())
    assert_same_frame(fb, ob.render(mixed, cam, threads=8), "mixed scene 45x23x8")


def test_kernels_through_l1_l2(big):
    """A scene beyond what LDS holds, 45x23x8: the pair walk's sphere-only build, and with sphere_only_kernel = -1 the general build on
    4-wide nodes (the kernel of BASELINE configs[4])."""
    cam = rb.rtiow_camera(45, 23, 8, 50)
    want = ob.render(big, cam, threads=8)
    for more, sphere_only in ((dict(), 1), (dict(sphere_only_kernel=-1), 0)):
        dev = rb.DeviceScene(big, device=0, honour_env=False, **more, **GUARDED)
        fb, t = dev.render_to_host(cam)
        assert t.guarded == 1 and t.scene_in_lds == 0 and t.guard_dynamic == 1 and t.sphere_only == sphere_only and t.primary_visibility == 1, \
            (t.guarded, t.scene_in_lds, t.guard_dynamic, t.sphere_only, t.primary_visibility, dev.guard_reason())
        assert_same_frame(fb, want, f"{big.desc.num_spheres} spheres through L1 / L2, sphere_only = {sphere_only}")


@pytest.mark.parametrize("parts", [2, 3])
def test_row_shards_with_a_partial_last_band(rtiow, wanted, parts):
    """The 67x35x8 frame in interleaved bands of 8 rows (five bands, the last of 3 rows), one render per part: each part's rows are
    the oracle's rows — the band interleave in the table's pixel rows."""
    import frame_parallel as fp
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    seen = np.zeros(H, dtype=bool)
    for part in range(parts):
        rows = fp.shard_row_indices(H, 8, parts, part)
        fb, t = dev.render_to_host(cams["8"], shard=fp.shard_for_rank(part, parts, 8))
        headline_kernels(dev, t)
        assert_same_frame(fb, frames["8"][rows], f"part {part} of {parts}")
        seen[rows] = True
    assert seen.all()


def test_three_passes(rtiow, wanted):
    """67x35x100 in passes: the table is read again by every pass's trace launch, with another slab pitch and another pass count.
    (A workspace budget never makes a pass shorter than 64 samples — rt_accel.cpp, plan_passes — so 100 samples split in three
    only through pass_spp: 34 + 33 + 33, passes of two lengths.  The smallest workspace_bytes gives two passes of 50: rendered too.)"""
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, pass_spp=34, **GUARDED)
    fb, t = dev.render_to_host(cams["100"])
    headline_kernels(dev, t)
    assert t.trace_launches >= 3, t.trace_launches
    assert_same_frame(fb, frames["100"], "S-rtiow 67x35x100, pass_spp = 34")
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, workspace_bytes=1, **GUARDED)
    fb, t = dev.render_to_host(cams["100"])
    headline_kernels(dev, t)
    assert t.trace_launches == 2, t.trace_launches
    assert_same_frame(fb, frames["100"], "S-rtiow 67x35x100, workspace_bytes = 1")


def test_four_passes_by_workspace_bytes(rtiow):
    """workspace_bytes small enough for several passes: at 67x35x200 the smallest budget gives four passes of 50 samples."""
    cam = rb.rtiow_camera(W, H, 200, 50)
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, workspace_bytes=1, **GUARDED)
    fb, t = dev.render_to_host(cam)
    headline_kernels(dev, t)
    assert t.trace_launches >= 3, t.trace_launches
    assert_same_frame(fb, ob.render(rtiow, cam, threads=8), "S-rtiow 67x35x200, workspace_bytes = 1")


def test_offset_first_sample(rtiow):
    """rt_render_samples with sample_first = 3: samples 3 … 6 of every pixel.  The oracle's frames start at sample 0, so the wanted
    sums are its per-sample radiances (oracle_bindings.trace_samples) added in sample order from 0, as its frame loop adds them."""
    first, spp = 3, 4
    cam = rb.rtiow_camera(W, H, spp, 50)
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cam, sample_first=first)
    headline_kernels(dev, t)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    want = np.zeros((H, W, 3), dtype=np.float32)
    for s in range(first, first + spp):
        ijs = np.stack([ii.ravel(), jj.ravel(), np.full(W * H, s)], axis=1).astype(np.int32)
        rad = ob.trace_samples(rtiow, cam, ijs)[0]
        want = (want + np.asarray(rad, dtype=np.float32).reshape(H, W, 3)).astype(np.float32)
    assert_same_frame(fb, want, "S-rtiow 67x35, samples 3 … 6")


def test_view_list_cache_follows_the_view(rtiow, wanted):
    """reuse_view_lists at its default: view A, view A again (the handle's table is used again), view B from another lookfrom (made
    anew), then view A (made anew again).  Each frame is its view's."""
    cams, frames = wanted
    cam_a = cams["8"]
    cam_b = view((-6.0, 2.5, 9.0), (0, 0, 0), 8)
    want = {"A": frames["8"], "B": ob.render(rtiow, cam_b, threads=8)}
    assert not np.array_equal(want["A"], want["B"])
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    assert dev.config().reuse_view_lists == 0
    for which, cam in (("A", cam_a), ("A", cam_a), ("B", cam_b), ("A", cam_a)):
        fb, t = dev.render_to_host(cam)
        headline_kernels(dev, t)
        assert_same_frame(fb, want[which], f"view {which}")


def test_only_sky(rtiow):
    """A camera that sees only sky and whose pixels have no candidate: the table's front part is empty, the trace kernel has no
    sample, and the frame is the background added spp times.  (A pixel's candidates come from a cone test whose margin grows with
    the pixel's angle and with the distance to a box's farthest corner — rt_beam.h, beam_hits_box — and the ground sphere's box is
    2500 across: at 67x35 and 20 degrees of view a camera 3 above that box is inside the grown box whichever way it looks, and
    every pixel has the ground on its list — still so with 2 degrees.  With 1 degree of view the margin stays below the camera's
    height; the camera looks up and away from the scene.)"""
    cam = view((13, 3, 2), (26, 9, 4), 8, vfov=1.0)
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.primary_visibility == 1 and t.traced_samples == 0, (t.guarded, t.primary_visibility, t.traced_samples)
    want = ob.render(rtiow, cam, threads=8)
    one = np.zeros(3, dtype=np.float32)
    for _ in range(8):
        one = (one + np.asarray(SKY, dtype=np.float32)).astype(np.float32)
    assert (bits(want) == bits(one)).all(), "the oracle's frame is nothing but sky"
    assert_same_frame(fb, want, "only sky")


def test_no_sky(rtiow):
    """A camera that looks down at the ground: every pixel is in the table's front part."""
    cam = view((4, 6, 3), (0, 0, 0), 8)
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cam)
    headline_kernels(dev, t)
    assert t.traced_samples == W * H * 8, t.traced_samples
    assert_same_frame(fb, ob.render(rtiow, cam, threads=8), "no sky")


def test_tile_away_from_the_corner(rtiow, wanted):
    """rt_render_tile with tile_x0 = 21, tile_y0 = 9, 33 x 17 pixels: the same window of the whole oracle frame — the tile's offsets in
    the table's pixel columns and rows."""
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    x0, y0, w, h = 21, 9, 33, 17
    fb, t = dev.render_tile_to_host(cams["8"], x0, y0, w, h)
    headline_kernels(dev, t)
    assert_same_frame(fb, frames["8"][y0:y0 + h, x0:x0 + w], "tile (21, 9) 33x17 of 67x35x8")
