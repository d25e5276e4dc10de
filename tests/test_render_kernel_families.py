"""Every kernel family of the render kernels' translation unit (csrc/rt_capi.hip, built with its own flag set: see the Makefile's
RENDERFLAGS), once each at the smallest shapes that reach it, bit for bit against the oracle.  Which family a frame took is read
from rt_timing, so that a change of the dispatch cannot quietly leave one of them untested.  No tolerance: tests/test_gpu_parity.py
says why."""
import numpy as np
import pytest

import oracle_bindings as ob
import rtp_bindings as rb

pytestmark = pytest.mark.gpu

GUARDED = dict(traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
EXACT = dict(traversal=rb.TRAVERSAL_EXACT)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_frame(got, want, what):
    same = (bits(got) == bits(want)).all(axis=-1)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} pixels differ, max abs diff {np.abs(got - want).max()}"


@pytest.fixture(scope="module")
def rtiow():
    return rb.HostScene.rtiow()


@pytest.fixture(scope="module")
def mixed():
    """A textured METAL quad, metal and diffuse spheres, and glass that absorbs (the expf path): the general kernel's material code."""
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
def wanted(rtiow, mixed):
    """The oracle's frames, rendered once and shared (read-only) by the tests below."""
    cams = {"rtiow_128": rb.rtiow_camera(32, 18, 128, 50), "rtiow_8": rb.rtiow_camera(48, 27, 8, 50), "mixed_8": rb.rtiow_camera(48, 27, 8, 50)}
    frames = {"rtiow_128": ob.render(rtiow, cams["rtiow_128"], threads=8), "rtiow_8": ob.render(rtiow, cams["rtiow_8"], threads=8),
              "mixed_8": ob.render(mixed, cams["mixed_8"], threads=8)}
    for f in frames.values():
        f.setflags(write=False)
    return cams, frames


def test_headline_kernels_one_128_spp_pass(rtiow, wanted):
    """S-rtiow 32x18, one pass of 128 samples: the primary-visibility pass by pixel (from 96 samples per pixel and pass) and the
    sphere-only trace kernel fed by it — the two kernels of the headline frame."""
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cams["rtiow_128"])
    assert t.trace_launches == 1 and t.guarded == 1 and t.sphere_only == 1 and t.scene_in_lds == 1 and t.primary_visibility == 1, \
        (t.trace_launches, t.guarded, t.sphere_only, t.scene_in_lds, t.primary_visibility, dev.guard_reason())
    assert dev.trace_kernel_name() == "void rtk::render_kernel<true, false, false, false, true, true>(rtk::KParams)"
    assert_same_frame(fb, frames["rtiow_128"], "S-rtiow 32x18x128")


def test_per_batch_primary_pass(rtiow, wanted):
    """The same scene at 48x27x8: below 96 samples per pixel and pass the primary-visibility pass works by batch of samples."""
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cams["rtiow_8"])
    assert t.guarded == 1 and t.sphere_only == 1 and t.primary_visibility == 1, (t.guarded, t.sphere_only, t.primary_visibility)
    assert_same_frame(fb, frames["rtiow_8"], "S-rtiow 48x27x8")


def test_general_kernel_with_plane_texture_glass_and_metal(mixed, wanted):
    """A scene with a textured plane: the general build of the octant kernel (768-thread workgroups), its plane, texture, metal and
    absorbing-glass code."""
    cams, frames = wanted
    dev = rb.DeviceScene(mixed, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cams["mixed_8"])
    assert t.guarded == 1 and t.sphere_only == 0 and t.workgroup_size == 768, (t.guarded, t.sphere_only, t.workgroup_size, dev.guard_reason())
    assert_same_frame(fb, frames["mixed_8"], "textured quad + absorbing glass + metal 48x27x8")


@pytest.mark.parametrize("which", ["rtiow_8", "mixed_8"])
def test_exact_walks(rtiow, mixed, wanted, which):
    """traversal = exact: the reference-order walk, sphere-only build and general build."""
    cams, frames = wanted
    dev = rb.DeviceScene(rtiow if which == "rtiow_8" else mixed, device=0, honour_env=False, **EXACT)
    fb, t = dev.render_to_host(cams[which])
    assert t.guarded == 0, t.guarded
    assert_same_frame(fb, frames[which], f"exact walk, {which}")


def test_parametric_walk_through_l1_l2():
    """A sphere-only scene beyond what LDS holds at full occupancy (1 000 spheres and more): distance-aware margins in parametric
    form, node and sphere records through L1 / L2."""
    host = rb.HostScene.rtiow(half_extent=16)
    assert host.desc.num_spheres >= 785 and host.desc.num_planes == 0
    cam = rb.rtiow_camera(48, 27, 8, 50)
    dev = rb.DeviceScene(host, device=0, honour_env=False, **GUARDED)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1 and t.scene_in_lds == 0 and t.guard_dynamic == 1 and t.sphere_only == 1, \
        (t.guarded, t.scene_in_lds, t.guard_dynamic, t.sphere_only, dev.guard_reason())
    want = ob.render(host, cam, threads=8)
    assert_same_frame(fb, want, f"{host.desc.num_spheres} spheres through L1 / L2, 48x27x8")
    # the general build of the same walk, on 4-wide nodes: the kernel of the stress scene (BASELINE configs[4])
    general = rb.DeviceScene(host, device=0, honour_env=False, sphere_only_kernel=-1, **GUARDED)
    fb, t = general.render_to_host(cam)
    assert t.guarded == 1 and t.scene_in_lds == 0 and t.guard_dynamic == 1 and t.sphere_only == 0, (t.guarded, t.scene_in_lds, t.guard_dynamic, t.sphere_only)
    assert_same_frame(fb, want, f"{host.desc.num_spheres} spheres through L1 / L2, general build")
