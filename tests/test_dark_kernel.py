"""The sphere-only octant kernel behind the primary-visibility pass in its build for scenes in which nothing emits (csrc/rt_kernel.hip.inc,
kDark / RTP_BODY_CARRY: no radiance accumulator in the lane, each ray's |d|^2 and fp64 reciprocal made once where the ray is armed), and
render_emit_kernel, the build that carries radiance, for the same scenes with an emitter or with rt_config.dark_kernel = -1.

Every frame here is compared bit for bit against the oracle (oracle_bindings.render), no tolerance, at the shapes that reach each
thing the build changes: three passes of two lengths (the retired samples of every pass), a frame in which the guarded walk flags
samples (resume_save leaves a dark lane's state to the exact re-walk), an emitting twin of the scene and one whose only "emission"
is a -0.0 (both must take the kernel that carries radiance), a sharded and a tiled render.  Which build ran is read from rt_timing."""
import numpy as np
import pytest

import oracle_bindings as ob
import rtp_bindings as rb

pytestmark = pytest.mark.gpu

W, H, SPP = 67, 35, 100        # the width is a multiple neither of 64 nor of 4
PASSES = dict(pass_spp=34)     # 34 + 33 + 33: three passes of two lengths
GUARDED = dict(traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
HEADLINE = "void rtk::render_kernel<true, false, false, false, true, true>(rtk::KParams)"
EMIT = "rtk::render_emit_kernel(rtk::KParams)"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_frame(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (bits(got) == bits(want)).all(axis=-1)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} pixels differ, max abs diff {np.abs(got - want).max()}"


def sphere_only_behind_primary(t, dev):
    assert t.guarded == 1 and t.sphere_only == 1 and t.scene_in_lds == 1 and t.primary_visibility == 1, \
        (t.guarded, t.sphere_only, t.scene_in_lds, t.primary_visibility, dev.guard_reason())


def ran_dark(t, dev):
    sphere_only_behind_primary(t, dev)
    assert t.dark_kernel == 1, t.dark_kernel
    assert dev.trace_kernel_name() == HEADLINE
    assert t.trace_vgprs <= 64 and t.trace_scratch_bytes == 0, (t.trace_vgprs, t.trace_scratch_bytes)


def ran_emitting(t, dev):
    sphere_only_behind_primary(t, dev)
    assert t.dark_kernel == 0, t.dark_kernel
    assert dev.trace_kernel_name() == EMIT


@pytest.fixture(scope="module")
def rtiow():
    host = rb.HostScene.rtiow()
    mats = host.desc.materials
    for k in range(host.desc.num_materials):
        assert all(bits(np.float32(mats[k].emit.e[j])) == 0 for j in range(3)), "S-rtiow emits nothing"
    return host


@pytest.fixture(scope="module")
def wanted(rtiow):
    """The oracle's 67x35x100 frame of S-rtiow, rendered once and shared read-only."""
    cam = rb.rtiow_camera(W, H, SPP, 50)
    frame = ob.render(rtiow, cam, threads=8)
    frame.setflags(write=False)
    return cam, frame


def test_three_passes_default_and_knob_off(rtiow, wanted):
    """S-rtiow 67x35x100 in passes of 34, 33 and 33 samples.  Default configuration: the dark build ran.  dark_kernel = -1: the build
    that carries radiance ran.  The two frames are equal, and both are the oracle's."""
    cam, frame = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **PASSES)
    assert dev.config().dark_kernel == 0
    fb_dark, t = dev.render_to_host(cam)
    ran_dark(t, dev)
    assert t.trace_launches == 3, t.trace_launches
    assert_same_frame(fb_dark, frame, "S-rtiow 67x35x100, default configuration")
    off = rb.DeviceScene(rtiow, device=0, honour_env=False, dark_kernel=-1, **PASSES)
    fb_emit, t = off.render_to_host(cam)
    ran_emitting(t, off)
    assert t.trace_launches == 3, t.trace_launches
    assert np.array_equal(bits(fb_dark), bits(fb_emit))
    assert_same_frame(fb_emit, frame, "S-rtiow 67x35x100, dark_kernel = -1")


def test_flagged_samples_resume_from_a_dark_lane(rtiow):
    """400x225x16 from the benchmark camera: the guarded walk flags a few hundred of the 1.44 M samples (the headline frame flags
    1.7e-4 of its samples from this view), so resume_save writes a dark lane's state — zeros where the radiance was — and the exact
    re-walk takes the samples over from there."""
    cam = rb.rtiow_camera(400, 225, 16, 50)
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False)
    assert dev.config().resume_flagged == 0
    fb, t = dev.render_to_host(cam)
    ran_dark(t, dev)
    print(f"flagged samples: {t.flagged_samples} of {400 * 225 * 16}")
    assert t.flagged_samples > 0, t.flagged_samples
    assert_same_frame(fb, ob.render(rtiow, cam, threads=8), "S-rtiow 400x225x16")


def emitting_twin(colour):
    """S-rtiow with the material of its last sphere — one of the three big ones — made a DIFFUSE_LIGHT of that colour."""
    host = rb.HostScene.rtiow()
    desc = host.desc
    k = desc.num_materials - 1
    assert desc.spheres[desc.num_spheres - 1].material_idx == k and desc.spheres[desc.num_spheres - 1].radius == 1.0
    desc.materials[k].type = 3
    desc.materials[k].emit.e[:] = colour
    return host


def test_a_light_takes_the_kernel_that_carries_radiance(wanted):
    cam, frame = wanted
    host = emitting_twin((4.0, 3.0, 2.0))
    dev = rb.DeviceScene(host, device=0, honour_env=False, **PASSES)
    fb, t = dev.render_to_host(cam)
    ran_emitting(t, dev)
    want = ob.render(host, cam, threads=8)
    assert not np.array_equal(bits(want), bits(frame)), "the light is in view"
    assert_same_frame(fb, want, "S-rtiow with a DIFFUSE_LIGHT sphere 67x35x100")


def test_a_negative_zero_counts_as_emission(rtiow, wanted):
    """One material's emit = (-0.0, 0, 0): (+0) + beta * (-0) is still +0, but only +0.0f bit for bit counts as dark."""
    cam, frame = wanted
    host = rb.HostScene.rtiow()
    host.desc.materials[7].emit.e[:] = (-0.0, 0.0, 0.0)
    assert bits(np.float32(host.desc.materials[7].emit.e[0])) == 0x80000000
    dev = rb.DeviceScene(host, device=0, honour_env=False, **PASSES)
    fb, t = dev.render_to_host(cam)
    ran_emitting(t, dev)
    assert_same_frame(fb, ob.render(host, cam, threads=8), "S-rtiow with emit = (-0, 0, 0) 67x35x100")
    assert_same_frame(fb, frame, "… which is S-rtiow's own frame")


def test_two_row_shards(rtiow, wanted):
    """The frame in interleaved bands of 8 rows (the last band has 3), one render per part, through the dark build."""
    import frame_parallel as fp
    cam, frame = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED, **PASSES)      # (two frames on one handle: no measuring frame between them)
    seen = np.zeros(H, dtype=bool)
    for part in range(2):
        rows = fp.shard_row_indices(H, 8, 2, part)
        fb, t = dev.render_to_host(cam, shard=rb.Shard(8, 2, part))
        ran_dark(t, dev)
        assert_same_frame(fb, frame[rows], f"part {part} of 2")
        seen[rows] = True
    assert seen.all()


def test_tile_away_from_the_corner(rtiow, wanted):
    cam, frame = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **PASSES)
    x0, y0, w, h = 21, 9, 33, 17
    fb, t = dev.render_tile_to_host(cam, x0, y0, w, h)
    ran_dark(t, dev)
    assert_same_frame(fb, frame[y0:y0 + h, x0:x0 + w], "tile (21, 9) 33x17 of 67x35x100")
