"""rt_render_lens / rt_render_aov_lens / rt_lens_camera_rays: thin-lens depth of field and shutter motion blur (include/rtp_amd.h,
DESIGN.md §12).

The header fixes the camera ray in float32 order; tests/cpu_native/lens_ref.c restates it on the oracle (lens_reference.py) and every
frame, AOV sum and probed ray must equal it bit for bit, on every walk.  With no lens and no motion the calls are rt_render_samples /
rt_render_aov_samples.  On the CPU: the ABI, every argument check (they come before anything else, so no scene and no device are
needed for them), the reference's geometry and the CLI refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_reference as lr
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, INVALID = 0, 1
F = np.float32


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} bytes differ (first at {np.argwhere(bad)[0]})"


def rtiow_pair(w, h, spp):
    """The benchmark camera and a second pose of the same orbit-like swing (the shutter's close end)."""
    return rb.rtiow_camera(w, h, spp), rb.make_camera(w, h, 20.0, (12.6, 3.6, 2.1), (0, 0, 0), (0.7, 0.8, 1.0), spp, 50)


FOCUS_RTIOW = float(np.sqrt(13.0 ** 2 + 3.0 ** 2 + 2.0 ** 2))      # the scene centre


def config_host(text):
    return rb.HostScene.from_config(text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg")))


def v(x):
    return np.array(x.e[:3], dtype=np.float64)


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_mirrors_symbols_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_lens_params_init", "rt_render_lens", "rt_render_aov_lens", "rt_lens_camera_rays"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.LensParams) == 12
    assert len(lib.rt_render_lens.argtypes) == 10 and len(lib.rt_render_aov_lens.argtypes) == 10
    assert len(lib.rt_lens_camera_rays.argtypes) == 8
    p = rb.lens_params()
    assert (p.struct_bytes, p.lens_radius, p.focus_distance) == (12, 0.0, 10.0)
    for name in ("render_lens", "render_lens_to_host", "render_aov_lens", "render_aov_lens_to_host", "lens_camera_rays"):
        assert hasattr(rb.DeviceScene, name)
    assert hasattr(rb.HostScene, "frame_camera_at")
    assert hasattr(rb.host_lib(), "rtp_host_frame_camera_at")


def _calls(cam_open, cam_close, lens):
    """(status, message) of each lens entry point with these arguments and no scene (device pointers never looked at)."""
    lib = rb.amd_lib()
    o = C.byref(cam_open) if cam_open is not None else None
    c = C.byref(cam_close) if cam_close is not None else None
    l = C.byref(lens) if lens is not None else None
    out = []
    st = lib.rt_render_lens(None, o, c, l, None, 0, C.c_void_p(1 << 32), None, 1, None)
    out.append((st, lib.rt_get_last_error_string().decode()))
    b = rb.AovBuffers()
    b.albedo_sum = 1 << 32
    st = lib.rt_render_aov_lens(None, o, c, l, None, 0, C.byref(b), None, 1, None)
    out.append((st, lib.rt_get_last_error_string().decode()))
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    sd = (C.c_uint32 * 1)()
    st = lib.rt_lens_camera_rays(o, c, l, 1, ijs, f, f, sd)
    out.append((st, lib.rt_get_last_error_string().decode()))
    return out


def test_argument_checks_come_first():
    """Each bad argument is refused by all three calls before anything else (no scene is needed to see it)."""
    cam, close = rtiow_pair(8, 4, 2)
    nan, inf = float("nan"), float("inf")
    bad = []
    for field, value in (("image_width", 9), ("image_height", 5), ("samples_per_pixel", 3), ("max_depth", 7)):
        c = rb.CameraData.from_buffer_copy(close)
        setattr(c, field, value)
        bad.append((c, rb.lens_params(), "cam_close"))
    c = rb.CameraData.from_buffer_copy(close)
    c.background.e[1] = 0.5
    bad.append((c, rb.lens_params(), "cam_close"))
    for r in (-0.1, nan, inf, -inf):
        bad.append((None, rb.lens_params(lens_radius=r), "lens_radius"))
    for fd in (0.0, -1.0, nan, inf):
        bad.append((close, rb.lens_params(lens_radius=0.1, focus_distance=fd), "focus_distance"))
    short = rb.lens_params(lens_radius=0.1)
    short.struct_bytes = 4
    bad.append((None, short, "struct_bytes"))
    for close_cam, lens, word in bad:
        for st, msg in _calls(cam, close_cam, lens):
            assert st == INVALID and word in msg, (word, st, msg)
    # a camera whose origin lies in its image plane: refused with the lens on, at either end
    flat = rb.CameraData.from_buffer_copy(cam)
    flat.pixel00_loc.e[0], flat.pixel00_loc.e[1], flat.pixel00_loc.e[2] = flat.origin.e[0], flat.origin.e[1], flat.origin.e[2]
    for o, c in ((flat, None), (cam, flat), (flat, cam)):
        for st, msg in _calls(o, c, rb.lens_params(lens_radius=0.1)):
            assert st == INVALID and "image plane" in msg, (st, msg)
    # … but not with the lens off (the focus distance is not read then either)
    for st, msg in _calls(flat, None, rb.lens_params(focus_distance=-1.0))[:2]:
        assert st == INVALID and "null scene" in msg, (st, msg)
    # good arguments: then the scene (null here); a short struct of an older caller keeps the defaults for the rest
    p = rb.lens_params(lens_radius=0.1, focus_distance=-1.0)
    p.struct_bytes = 8
    for st, msg in _calls(cam, close, p)[:2]:
        assert st == INVALID and "null scene" in msg, (st, msg)
    for st, msg in _calls(None, close, None):
        assert st == INVALID, (st, msg)
    lib = rb.amd_lib()
    assert lib.rt_lens_camera_rays(C.byref(cam), None, None, -1, None, None, None, None) == INVALID
    assert lib.rt_lens_camera_rays(C.byref(cam), None, None, 0, None, None, None, None) == OK


def _random_cameras(rng, k):
    for _ in range(k):
        eye = rng.uniform(-20, 20, 3)
        target = eye + rng.normal(0, 1, 3) * rng.uniform(1, 30)
        w, h = int(rng.integers(8, 200)), int(rng.integers(8, 200))
        yield rb.make_camera(w, h, float(rng.uniform(10, 90)), tuple(eye), tuple(target), spp=4)


def _orbit_cameras(text):
    host = config_host(text)
    return host, [host.frame_camera_at(t) for t in (0.0, 0.5, 7.25, 33.0, 99.5)]


def test_reference_geometry_focus_lens_disc_and_time(test_config_text):
    """Every lens ray of one (pixel, ox, oy) passes through the pinhole ray's point on the plane in focus; lens points lie in the
    (du, dv) plane within R of the origin; tau lies in [0, 1)."""
    rng = np.random.default_rng(11)
    _, orbit = _orbit_cameras(test_config_text)
    cams = list(_random_cameras(rng, 12)) + orbit
    for cam in cams:
        n = 2000
        ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1)
        R, fd = float(rng.uniform(0.01, 2.0)), float(rng.uniform(0.5, 40.0))
        po, pd, pseed, _, _ = lr.rays(cam, None, 0.0, fd, ijs)
        lo, ld, lseed, _, lxy = lr.rays(cam, None, R, fd, ijs)
        o, du, dv, p00 = v(cam.origin), v(cam.pixel_delta_u), v(cam.pixel_delta_v), v(cam.pixel00_loc)
        nrm = np.cross(du, dv)
        nrm /= np.linalg.norm(nrm)
        dimg = abs(np.dot(p00 - o, nrm))
        focus = po.astype(np.float64) + (fd / dimg) * pd.astype(np.float64)
        scale = np.abs(focus).max(axis=1) + np.abs(o).max() + fd
        # the lens ray reaches the focus point at parameter 1 (F - L): within a few ulps of the scale
        reach = lo.astype(np.float64) + ld.astype(np.float64)
        assert (np.abs(reach - focus).max(axis=1) <= 64 * np.finfo(F).eps * scale).all()
        # the focus point is on the plane at focus_distance along the image plane's normal
        assert np.allclose(np.abs((focus - o) @ nrm), fd, rtol=1e-4)
        # lens points: in the (du, dv) plane, within R
        off = lo.astype(np.float64) - o
        assert (np.abs(off @ nrm) <= 1e-5 * (np.abs(o).max() + R)).all()
        assert (np.linalg.norm(off, axis=1) <= R * (1 + 1e-5) + 1e-5 * np.abs(o).max()).all()
        assert (lxy[:, 0] ** 2 + lxy[:, 1] ** 2 < 1).all()
        # the pinhole ray's draws stop after oy; the lens adds at least two
        assert (pseed != lseed).all()
    # tau ∈ [0, 1), and the pose at tau lies between the ends
    cam, close = rtiow_pair(64, 32, 4)
    ijs = np.stack([rng.integers(0, 64, 5000), rng.integers(0, 32, 5000), rng.integers(0, 1 << 20, 5000)], 1)
    mo, _, _, tau, _ = lr.rays(cam, close, 0.0, 10.0, ijs)
    assert (tau >= 0).all() and (tau < 1).all() and tau.std() > 0.2
    a, b = v(cam.origin), v(close.origin)
    t = (mo.astype(np.float64) - a) @ (b - a) / np.dot(b - a, b - a)
    assert np.allclose(t, tau, atol=1e-5)


def test_reference_pinhole_frame_is_the_oracles(test_config_text):
    """With R = 0 and no motion, the reference's frame is orc_render's, bit for bit."""
    import oracle_bindings as ob
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(48, 27, 3)
    assert_same(lr.frame(host, cam, threads=8), ob.render(host, cam, threads=8), "rtiow")
    chost, orbit = _orbit_cameras(test_config_text)
    c = rb.CameraData.from_buffer_copy(chost.frame_camera(3))
    c.image_width, c.image_height, c.samples_per_pixel = 32, 24, 2
    assert_same(lr.frame(chost, c, threads=8), ob.render(chost, c, threads=8), "config scene")


def test_frame_camera_at_whole_frames_are_frame_camera(test_config_text):
    host = config_host(test_config_text)
    for f in (0, 1, 17, 99):
        assert bytes(host.frame_camera_at(float(f))) == bytes(host.frame_camera(f))


def test_cli_refusals(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    for args, env in ((["--lens", "0.1:10", "--denoise-temporal"], {}), (["--motion-blur", "0.5", "--adaptive", "0.1"], {}),
                      (["--lens", "0.1:10", "--devices", "2"], {}), (["--motion-blur", "0.5", "--shard", "2"], {}),
                      (["--lens", "0.1:10", "--aov", "--devices", "1"], {}), (["--lens", "0.1:10"], {"RTP_DEVICES": "2"}),
                      (["--motion-blur", "0"], {}), (["--motion-blur", "1.5"], {}), (["--motion-blur", "x"], {}), (["--lens", "-1:10"], {}),
                      (["--lens", "0.1:0"], {}), (["--lens", "0.1"], {}), (["--lens", "nan:10"], {})):
        r = subprocess.run([exe, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                           env={**os.environ, **env})
        assert r.returncode == 99 and ("--lens" in r.stderr or "--motion-blur" in r.stderr), (args, env, r.returncode, r.stderr)
        assert not os.listdir(tmp_path), (args, os.listdir(tmp_path))


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

WALKS = (dict(), dict(traversal=rb.TRAVERSAL_GUARDED), dict(traversal=rb.TRAVERSAL_GUARDED, primary_visibility=-1),
         dict(traversal=rb.TRAVERSAL_EXACT))
MODES = (("lens", False, 0.1), ("motion", True, 0.0), ("both", True, 0.1))


@pytest.mark.gpu
def test_identity_without_lens_or_motion():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(160, 90, 8)
    shard = rb.Shard(4, 3, 1)
    for config in WALKS:
        dev = rb.DeviceScene(host, device=0, **config)
        for sh in (None, shard):
            for first in (0, 5):
                want, _ = dev.render_to_host(cam, shard=sh, sample_first=first)
                got, t = dev.render_lens_to_host(cam, shard=sh, sample_first=first)
                assert_same(got, want, f"identity {config} shard={sh is not None} first={first}")
                got, _ = dev.render_lens_to_host(cam, lens={"lens_radius": 0.0, "focus_distance": 3.0}, shard=sh, sample_first=first)
                assert_same(got, want, f"identity, explicit R = 0 {config}")
        dev.close()


@pytest.mark.gpu
def test_parity_rtiow_every_walk_and_rework_form():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam, close = rtiow_pair(160, 90, 8)
    walks = WALKS + (dict(traversal=rb.TRAVERSAL_GUARDED, resume_flagged=-1), dict(traversal=rb.TRAVERSAL_GUARDED, overlap_rework=-1))
    flagged = {}
    for name, motion, R in MODES:
        c = close if motion else None
        want = lr.frame(host, cam, c, R, FOCUS_RTIOW)
        for config in walks:
            dev = rb.DeviceScene(host, device=0, **config)
            got, t = dev.render_lens_to_host(cam, cam_close=c, lens={"lens_radius": R, "focus_distance": FOCUS_RTIOW})
            assert_same(got, want, f"rtiow {name} {config}")
            if config.get("traversal") == rb.TRAVERSAL_GUARDED:
                assert t.guarded == 1, (name, config)
                key = "resume" if "resume_flagged" in config else ("serial" if "overlap_rework" in config else "default")
                flagged[key] = flagged.get(key, 0) + int(t.flagged_samples)
            if config.get("traversal") == rb.TRAVERSAL_EXACT:
                assert t.guarded == 0 and t.flagged_samples == 0
            dev.close()
    # the exact re-walk of flagged samples ran on lens frames in each form (resumed, restarted from the lens camera, not overlapped)
    assert all(flagged.get(k, 0) > 0 for k in ("default", "resume", "serial")), flagged


@pytest.mark.gpu
def test_parity_config_scene_orbit_shard_and_sample_first(test_config_text):
    rb.amd_lib().rt_set_device(0)
    host = config_host(test_config_text)
    f = 7

    def small(cam):
        c = rb.CameraData.from_buffer_copy(cam)
        c.image_width, c.image_height, c.samples_per_pixel = 96, 64, 4
        return c
    cam, close = small(host.frame_camera_at(float(f))), small(host.frame_camera_at(f + 0.5))
    fd = float(np.linalg.norm(v(cam.origin)))
    shard = rb.Shard(4, 2, 1)
    for config in WALKS:
        dev = rb.DeviceScene(host, device=0, **config)
        for name, motion, R in MODES:
            c = close if motion else None
            for sh, first in ((None, 0), (shard, 0), (None, 3)):
                want = lr.frame(host, cam, c, R, fd, shard=sh, sample_first=first)
                got, _ = dev.render_lens_to_host(cam, cam_close=c, lens={"lens_radius": R, "focus_distance": fd}, shard=sh, sample_first=first)
                assert_same(got, want, f"config scene {name} {config} shard={sh is not None} first={first}")
        dev.close()


@pytest.mark.gpu
def test_probe_rays_equal_the_reference():
    rb.amd_lib().rt_set_device(0)
    rng = np.random.default_rng(5)
    cam, close = rtiow_pair(1920, 1080, 64)
    n = 100000
    ijs = np.stack([rng.integers(0, 1920, n), rng.integers(0, 1080, n), rng.integers(0, 1 << 24, n)], 1).astype(np.int32)
    for name, motion, R in MODES + (("pinhole", False, 0.0),):
        c = close if motion else None
        go, gd, gs = rb.lens_camera_rays(cam, c, rb.lens_params(lens_radius=R, focus_distance=FOCUS_RTIOW), ijs)
        wo, wd, ws, _, _ = lr.rays(cam, c, R, FOCUS_RTIOW, ijs)
        assert_same(go, wo, f"{name} origins")
        assert_same(gd, wd, f"{name} directions")
        assert_same(gs, ws, f"{name} seeds")


@pytest.mark.gpu
def test_aov_lens_against_the_reference_and_the_denoiser():
    import torch
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam, close = rtiow_pair(96, 54, 4)
    dev = rb.DeviceScene(host, device=0)
    for name, motion, R in MODES:
        c = close if motion else None
        got, _ = dev.render_aov_lens_to_host(cam, cam_close=c, lens={"lens_radius": R, "focus_distance": FOCUS_RTIOW})
        want = lr.aov(host, cam, c, R, FOCUS_RTIOW)
        for k in want:
            assert_same(got[k], want[k], f"aov {name} {k}")
    # no lens, no motion: rt_render_aov_samples
    for first in (0, 2):
        got, _ = dev.render_aov_lens_to_host(cam, sample_first=first)
        want, _ = dev.render_aov_to_host(cam, sample_first=first)
        for k in want:
            assert_same(got[k], want[k], f"aov identity {k} first={first}")
    # rt_denoise on a lens frame with its AOVs
    fb = torch.zeros((54, 96, 3), device="cuda:0")
    dev.render_lens(cam, fb.data_ptr(), cam_close=close, lens={"lens_radius": 0.1, "focus_distance": FOCUS_RTIOW})
    aov = {k: torch.zeros((54, 96, per) if per > 1 else (54, 96), dtype={np.float32: torch.float32, np.uint32: torch.int32,
                                                                        np.int32: torch.int32}[dt], device="cuda:0")
           for k, _, dt, per in rb.AOV_CHANNELS}
    dev.render_aov_lens(cam, {k: t.data_ptr() for k, t in aov.items()}, cam_close=close, lens={"lens_radius": 0.1, "focus_distance": FOCUS_RTIOW})
    out = torch.zeros_like(fb)
    rb.denoise(fb.data_ptr(), {k: t.data_ptr() for k, t in aov.items()}, 96, 54, 4, out.data_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isfinite(o).all() and o.max() > 0
    dev.close()


@pytest.mark.gpu
def test_reach_a_huge_lens_takes_the_exact_walk():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(96, 54, 4)
    lens = {"lens_radius": 200.0, "focus_distance": FOCUS_RTIOW}
    guarded = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_GUARDED)
    exact = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_EXACT)
    got, t = guarded.render_lens_to_host(cam, lens=lens)
    want, _ = exact.render_lens_to_host(cam, lens=lens)
    assert t.guarded == 0
    assert_same(got, want, "huge lens")
    assert_same(got, lr.frame(host, cam, None, 200.0, FOCUS_RTIOW), "huge lens against the reference")
    # a small lens on the same handle stays guarded
    _, t = guarded.render_lens_to_host(cam, lens={"lens_radius": 0.05, "focus_distance": FOCUS_RTIOW})
    assert t.guarded == 1
    # near the reach: the largest radius the guarded walk still takes (bisection), then a camera whose du and dv are far from
    # orthogonal — its lens points reach up to sqrt(2) R from the origin — at just below that radius: the reference's bits
    tiny = rb.rtiow_camera(16, 9, 1)
    lo, hi = 0.0, 64.0
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        _, t = guarded.render_lens_to_host(tiny, lens={"lens_radius": mid, "focus_distance": FOCUS_RTIOW})
        lo, hi = (mid, hi) if t.guarded else (lo, mid)
    assert lo > 0.05
    skew = rb.CameraData.from_buffer_copy(cam)
    du, dv = v(cam.pixel_delta_u), v(cam.pixel_delta_v)
    sdv = dv + 0.95 * np.linalg.norm(dv) / np.linalg.norm(du) * du
    for k in range(3):
        skew.pixel_delta_v.e[k] = float(sdv[k])
    R = lo * 0.999
    got, t = guarded.render_lens_to_host(skew, lens={"lens_radius": R, "focus_distance": FOCUS_RTIOW})
    assert t.guarded == 1
    assert_same(got, lr.frame(host, skew, None, R, FOCUS_RTIOW), "skewed camera near the reach")
    _, t = guarded.render_lens_to_host(skew, lens={"lens_radius": hi * 1.001, "focus_distance": FOCUS_RTIOW})
    assert t.guarded == 0
    guarded.close()
    exact.close()


@pytest.mark.gpu
def test_handle_state_is_left_alone():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam, close = rtiow_pair(128, 72, 8)
    dev = rb.DeviceScene(host, device=0)
    first, _ = dev.render_to_host(cam)
    before = dev.last_timing()
    dev.render_lens_to_host(cam, cam_close=close, lens={"lens_radius": 0.1, "focus_distance": FOCUS_RTIOW})
    dev.render_aov_lens_to_host(cam, cam_close=close, lens={"lens_radius": 0.1, "focus_distance": FOCUS_RTIOW})
    after = dev.last_timing()
    assert bytes(before) == bytes(after), "rt_last_timing still reports the last rt_render"
    again, t = dev.render_to_host(cam)
    fresh = rb.DeviceScene(host, device=0)
    want, _ = fresh.render_to_host(cam)
    assert_same(again, want, "rt_render after lens calls")
    assert_same(first, want, "the first frame")
    fresh.close()
    dev.close()
    # the cached view lists survive lens calls: at 1920 x 1080 x 1 spp making the lists is most of a frame's primary time, so a
    # repeated frame that reuses them spends a fraction of the first one's (one that made them anew would spend as much)
    # (GUARDED: AUTO may make a later frame an exploring exact one, which has no lists — a decision of its own frames)
    big, big_close = rtiow_pair(1920, 1080, 1)
    dev = rb.DeviceScene(host, device=0, traversal=rb.TRAVERSAL_GUARDED)
    dev.render_to_host(big)
    t_first = dev.last_timing()
    dev.render_to_host(big)
    t_reuse = dev.last_timing()
    dev.render_lens_to_host(big, cam_close=big_close, lens={"lens_radius": 0.1, "focus_distance": FOCUS_RTIOW})
    dev.render_aov_lens_to_host(big, cam_close=big_close, lens={"lens_radius": 0.1, "focus_distance": FOCUS_RTIOW})
    dev.render_to_host(big)
    t_after = dev.last_timing()
    assert t_first.primary_visibility == 1 and t_reuse.primary_visibility == 1 and t_after.primary_visibility == 1
    assert t_reuse.primary_ms < 0.6 * t_first.primary_ms, (t_first.primary_ms, t_reuse.primary_ms)
    assert t_after.primary_ms < 0.6 * t_first.primary_ms, (t_first.primary_ms, t_after.primary_ms)
    dev.close()


@pytest.mark.gpu
def test_retired_kernel_settings_are_refused_as_by_render_samples():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(32, 18, 1)
    for config in (dict(kernel=rb.KERNEL_WAVEFRONT), dict(wide_nodes=1)):
        dev = rb.DeviceScene(host, device=0, **config)
        with pytest.raises(rb.RtError):
            dev.render_to_host(cam, sample_first=1)
        with pytest.raises(rb.RtError, match="retired"):
            dev.render_lens_to_host(cam)
        dev.close()


@pytest.mark.gpu
def test_sync_zero_on_a_torch_stream():
    import torch
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam, close = rtiow_pair(96, 54, 4)
    dev = rb.DeviceScene(host, device=0)
    lens = {"lens_radius": 0.1, "focus_distance": FOCUS_RTIOW}
    want, _ = dev.render_lens_to_host(cam, cam_close=close, lens=lens)
    s = torch.cuda.Stream()
    fb = torch.full((54, 96, 3), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dev.render_lens(cam, fb.data_ptr(), cam_close=close, lens=lens, stream=s.cuda_stream, sync=False)
    s.synchronize()
    assert_same(fb.cpu().numpy(), want, "sync = 0 on a side stream")
    dev.close()


@pytest.mark.gpu
def test_cli_lens_motion_frames_are_the_python_paths(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    out = subprocess.run([exe, "--gpu", "--lens", "0.2:12", "--motion-blur", "0.5", "--aov", "--denoise"], input=text, capture_output=True,
                         text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    cam, close = host.frame_camera_at(0.0), host.frame_camera_at(0.5)
    lens = {"lens_radius": 0.2, "focus_distance": 12.0}
    fb, _ = dev.render_lens_to_host(cam, cam_close=close, lens=lens)
    want = rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp)
    assert open(tmp_path / "f_0.png", "rb").read() == want
    # … which are also rt_tonemap's bytes of the device sums
    import torch
    d = torch.from_numpy(fb).to("cuda:0").contiguous()
    rgb = torch.zeros(d.numel(), dtype=torch.uint8, device="cuda:0")
    assert rb.amd_lib().rt_tonemap(C.c_void_p(d.data_ptr()), C.c_void_p(rgb.data_ptr()), d.numel(), info.sqrt_spp, None) == OK
    torch.cuda.synchronize()
    assert open(tmp_path / "f_0.png", "rb").read()[8:] == rgb.cpu().numpy().tobytes()
    assert os.path.getsize(tmp_path / "f_0.png.aov") > 12 and os.path.getsize(tmp_path / "f_0.png.denoised") > 8
    dev.close()
