"""rt_render_adaptive and rt_tonemap_spp: per-pixel adaptive sampling to a noise target (include/rtp_amd.h).

The central promise is checked per pixel: every pixel that got n samples equals, bit for bit, the same pixel of rt_render at
n samples per pixel — on a guarded and an exact handle, with and without primary visibility, on a shard of rows, and against the
oracle for a few rows.  The moments and the stopping rule are restated on the CPU (numpy float32, one operation at a time) from
rt_trace_samples radiances and must give the same counts and moments exactly.  On the CPU: the ABI and every argument check
(they come before anything else, so no scene and no device are needed for them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = 1 << 32          # a device address that is never dereferenced
OK, INVALID, UNSUPPORTED = 0, 1, 4
F = np.float32


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} bytes differ (first at {np.argwhere(bad)[0]})"


# ---- the header's rule, restated: float32, one operation at a time ---------------------------------------------------------

def lum(rad):
    """rad (..., 3) float32 → y = (0.2126f*r + 0.7152f*g) + 0.0722f*b."""
    r, g, b = rad[..., 0], rad[..., 1], rad[..., 2]
    return ((F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b).astype(F)


def goes_on(s1, s2, n, batch, max_spp, t):
    if n + batch > max_spp:
        return np.zeros(s1.shape, bool)
    t = F(t)
    if t == 0:
        return np.ones(s1.shape, bool)
    with np.errstate(all="ignore"):
        mean = (s1 / F(n)).astype(F)
        var = np.fmax(F(0), ((s2 - s1 * mean).astype(F) / F(n - 1)).astype(F))
        return (var / F(n)).astype(F) > (t * t) * ((mean * mean).astype(F) + F(1e-4))


def reference(rad, min_spp, batch, max_spp, t):
    """rad (pixels, samples >= max_spp, 3): per-sample radiances → (counts, S1, S2) by the header's C loop."""
    y = lum(rad)
    pixels = rad.shape[0]
    s1, s2 = np.zeros(pixels, F), np.zeros(pixels, F)
    for s in range(min_spp):
        s1 = (s1 + y[:, s]).astype(F)
        s2 = (s2 + (y[:, s] * y[:, s]).astype(F)).astype(F)
    n = np.full(pixels, min_spp, np.int32)
    on = np.ones(pixels, bool)
    for r in range(1, (max_spp - min_spp) // batch + 1):
        k = min_spp + (r - 1) * batch
        on &= goes_on(s1, s2, k, batch, max_spp, t)
        if not on.any():
            break
        for s in range(k, k + batch):
            s1 = np.where(on, (s1 + y[:, s]).astype(F), s1)
            s2 = np.where(on, (s2 + (y[:, s] * y[:, s]).astype(F)).astype(F), s2)
        n[on] += batch
    return n, s1, s2


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_mirrors_symbols_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_adaptive_params_init", "rt_render_adaptive", "rt_tonemap_spp"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.AdaptiveParams) == 20
    assert len(lib.rt_render_adaptive.argtypes) == 10 and len(lib.rt_tonemap_spp.argtypes) == 5
    p = rb.adaptive_params()
    assert (p.struct_bytes, p.min_spp, p.batch_spp, p.max_spp) == (20, 16, 16, 256) and p.threshold == F(0.02)
    for name in ("render_adaptive", "render_adaptive_to_host"):
        assert hasattr(rb.DeviceScene, name)


def _call(params="default", scene=None, cam="default", fb=FAKE, spp=2 * FAKE, mom=None, timing=None):
    lib = rb.amd_lib()
    if params == "default":
        params = rb.adaptive_params(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1)
    if cam == "default":
        cam = rb.make_camera(8, 4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    st = lib.rt_render_adaptive(scene, C.byref(cam) if cam is not None else None, None, C.byref(params) if params is not None else None,
                                C.c_void_p(fb), C.c_void_p(spp), C.c_void_p(mom), None, 1, C.byref(timing) if timing is not None else None)
    return st, lib.rt_get_last_error_string().decode()


def test_argument_checks_come_first():
    """Each bad argument is refused with its code; the parameter checks need no scene (nothing is looked at after them)."""
    def params(**kw):
        return rb.adaptive_params(**{**dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1), **kw})
    assert _call(params=None)[0] == INVALID
    short = params()
    short.struct_bytes = 4
    assert _call(params=short)[0] == INVALID
    for kw, code, word in ((dict(min_spp=1), INVALID, "min_spp"), (dict(min_spp=-5), INVALID, "min_spp"), (dict(batch_spp=0), INVALID, "batch_spp"),
                           (dict(max_spp=3), INVALID, "max_spp"), (dict(threshold=-0.01), INVALID, "threshold"),
                           (dict(threshold=float("nan")), INVALID, "threshold"), (dict(threshold=float("inf")), INVALID, "threshold"),
                           (dict(max_spp=65537), UNSUPPORTED, "65536"), (dict(min_spp=70000, max_spp=70000), UNSUPPORTED, "65536")):
        st, msg = _call(params=params(**kw))
        assert st == code and word in msg, (kw, st, msg)
    # good parameters: then the scene and camera are checked (null here)
    assert _call()[0] == INVALID
    assert _call(cam=None)[0] == INVALID
    # a short struct of an older caller: its fields, defaults for the rest (batch_spp 0 is past its end: 16)
    p = params(batch_spp=0)
    p.struct_bytes = 8
    st, msg = _call(params=p)
    assert st == INVALID and "null scene" in msg


def test_tonemap_spp_arguments():
    lib = rb.amd_lib()
    assert lib.rt_tonemap_spp(None, None, None, 0, None) == OK
    assert lib.rt_tonemap_spp(None, C.c_void_p(FAKE), C.c_void_p(FAKE), 5, None) == INVALID
    assert lib.rt_tonemap_spp(C.c_void_p(FAKE), None, C.c_void_p(FAKE), 5, None) == INVALID
    assert lib.rt_tonemap_spp(C.c_void_p(FAKE), C.c_void_p(FAKE), None, 5, None) == INVALID


def test_reference_rule_on_synthetic_samples():
    rng = np.random.default_rng(7)
    pixels = 64
    rad = np.zeros((pixels, 64, 3), F)
    rad[16:32] = F(0.5)                                                     # constant: stops at min_spp
    rad[32:] = rng.uniform(0, 4, (pixels - 32, 64, 3)).astype(F)            # noisy: goes on
    n, s1, _ = reference(rad, 4, 4, 64, 0.01)
    assert (n[:32] == 4).all() and (n[32:] > 4).all()
    assert ((n - 4) % 4 == 0).all() and n.max() <= 64
    n0, _, _ = reference(rad, 4, 4, 64, 0.0)
    assert (n0 == 64).all()
    nh, _, _ = reference(rad, 4, 4, 64, 1e30)
    assert (nh == 4).all()
    n7, _, _ = reference(rad, 4, 7, 64, 0.0)                                # 4 + 8 * 7 = 60: the cap is not reached
    assert (n7 == 60).all()
    assert s1[16] == F(2.0)


def test_cli_refuses_adaptive_with_other_drivers(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    for extra in (["--denoise"], ["--aov"], ["--shard", "2"], ["--devices", "2"], ["--adaptive-spp", "4x4x8"]):
        r = subprocess.run([exe, "--gpu", "--adaptive", "0.1", *extra], input=test_config_text, capture_output=True, text=True, cwd=tmp_path,
                           timeout=60)
        assert r.returncode == 2 and "adaptive" in r.stderr, (extra, r.returncode, r.stderr)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _uniform(dev, cam, n, shard=None):
    c = rb.CameraData.from_buffer_copy(cam)
    c.samples_per_pixel = int(n)
    fb, _ = dev.render_to_host(c, shard=shard)
    return fb


def _check_parity(dev, cam, what, shard=None, **params):
    fb, spp, mom, _ = dev.render_adaptive_to_host(cam, shard=shard, **params)
    levels = np.unique(spp)
    mn, b, mx = params["min_spp"], params["batch_spp"], params["max_spp"]
    assert ((levels - mn) % b == 0).all() and levels.min() >= mn and levels.max() <= mx, (what, levels)
    covered = np.zeros(spp.shape, bool)
    for n in levels:
        want = _uniform(dev, cam, n, shard)
        sel = spp == n
        assert_same(fb[sel], want[sel], f"{what}: pixels with {n} samples")
        covered |= sel
    assert covered.all()
    return fb, spp, mom


def _levels_threshold(dev, cam, **params):
    """A threshold under which at least three stop levels occur (the first of a few candidates that gives them)."""
    for t in (0.1, 0.05, 0.2, 0.03, 0.3, 0.02, 0.5):
        _, spp, _, _ = dev.render_adaptive_to_host(cam, threshold=t, **params)
        if len(np.unique(spp)) >= 3:
            return t
    raise AssertionError("no candidate threshold gives three stop levels")


SPP = dict(min_spp=4, batch_spp=4, max_spp=64)


@pytest.mark.gpu
def test_per_pixel_parity_rtiow_on_every_walk():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(160, 90, 1, 50)
    t = _levels_threshold(rb.DeviceScene(host, device=0), cam, **SPP)
    shard = rb.Shard(4, 3, 1)
    for config in (dict(), dict(traversal=rb.TRAVERSAL_GUARDED), dict(traversal=rb.TRAVERSAL_GUARDED, primary_visibility=-1),
                   dict(traversal=rb.TRAVERSAL_GUARDED, overlap_rework=-1), dict(traversal=rb.TRAVERSAL_EXACT)):
        dev = rb.DeviceScene(host, device=0, **config)
        _, spp, _ = _check_parity(dev, cam, f"rtiow {config}", threshold=t, **SPP)
        assert len(np.unique(spp)) >= 3
        _check_parity(dev, cam, f"rtiow {config} shard", shard=shard, threshold=t, **SPP)
        dev.close()


@pytest.mark.gpu
def test_per_pixel_parity_config_scene_and_oracle_rows(test_config_text):
    import oracle_bindings as ob
    rb.amd_lib().rt_set_device(0)
    text = test_config_text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    cam = host.frame_camera(0)
    dev = rb.DeviceScene(host, device=0)
    t = _levels_threshold(dev, cam, **SPP)
    fb, spp, _ = _check_parity(dev, cam, "config scene", threshold=t, **SPP)
    # a few rows against the oracle, at each of their pixels' own counts
    for row in (cam.image_height // 3, cam.image_height // 2):
        for n in np.unique(spp[row]):
            c = rb.CameraData.from_buffer_copy(cam)
            c.samples_per_pixel = int(n)
            want = ob.render(host, c, row, row + 1, threads=8)[0]
            sel = spp[row] == n
            assert_same(fb[row][sel], want[sel], f"oracle row {row} n={n}")
    dev.close()


@pytest.mark.gpu
def test_rule_and_moments_against_the_cpu_restatement():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(48, 27, 1, 50)
    w, h = cam.image_width, cam.image_height
    for config in (dict(), dict(traversal=rb.TRAVERSAL_EXACT)):
        dev = rb.DeviceScene(host, device=0, **config)
        jj, ii, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(64), indexing="ij")
        ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], axis=1).astype(np.int32)
        rad, _, _ = dev.trace_samples(cam, ijs)
        rad = rad.reshape(h * w, 64, 3)
        for t, params in ((0.1, SPP), (0.05, SPP), (0.2, dict(min_spp=2, batch_spp=3, max_spp=64)), (0.0, SPP), (1e30, SPP)):
            n, s1, s2 = reference(rad, params["min_spp"], params["batch_spp"], params["max_spp"], t)
            fb, spp, mom, _ = dev.render_adaptive_to_host(cam, threshold=t, **params)
            assert_same(spp.ravel(), n, f"{config} t={t} counts")
            assert_same(mom.reshape(-1, 2)[:, 0], s1, f"{config} t={t} S1")
            assert_same(mom.reshape(-1, 2)[:, 1], s2, f"{config} t={t} S2")
        dev.close()


@pytest.mark.gpu
def test_edge_cases_threshold_zero_huge_and_min_equals_max():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(64, 36, 1, 50)
    dev = rb.DeviceScene(host, device=0)
    fb, spp, _, _ = dev.render_adaptive_to_host(cam, min_spp=4, batch_spp=4, max_spp=32, threshold=0.0)
    assert (spp == 32).all()
    assert_same(fb, _uniform(dev, cam, 32), "threshold 0 = rt_render at max_spp")
    fb, spp, _, _ = dev.render_adaptive_to_host(cam, min_spp=4, batch_spp=5, max_spp=32, threshold=0.0)
    assert (spp == 29).all()                      # 4 + 5 * 5: the next batch would pass the cap
    assert_same(fb, _uniform(dev, cam, 29), "threshold 0, cap not reached")
    huge, spp_h, mom_h, _ = dev.render_adaptive_to_host(cam, min_spp=6, batch_spp=4, max_spp=64, threshold=1e30)
    assert (spp_h == 6).all()
    assert_same(huge, _uniform(dev, cam, 6), "huge threshold = rt_render at min_spp")
    same, spp_s, mom_s, _ = dev.render_adaptive_to_host(cam, min_spp=6, batch_spp=4, max_spp=6, threshold=0.05)
    assert_same(same, huge, "min == max")
    assert_same(spp_s, spp_h, "min == max counts")
    assert_same(mom_s, mom_h, "min == max moments")
    dev.close()


@pytest.mark.gpu
def test_sync_zero_on_a_torch_stream_and_null_moments():
    import torch
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(96, 54, 1, 50)
    dev = rb.DeviceScene(host, device=0)
    want_fb, want_spp, _, _ = dev.render_adaptive_to_host(cam, threshold=0.1, **SPP)
    s = torch.cuda.Stream()
    fb = torch.full((54, 96, 3), float("nan"), device="cuda:0")
    spp = torch.full((54, 96), -1, dtype=torch.int32, device="cuda:0")
    rgb = torch.zeros((54, 96, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dev.render_adaptive(cam, fb.data_ptr(), spp.data_ptr(), None, stream=s.cuda_stream, sync=False, threshold=0.1, **SPP)
        assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(fb.data_ptr()), C.c_void_p(spp.data_ptr()), C.c_void_p(rgb.data_ptr()), 96 * 54,
                                           C.c_void_p(s.cuda_stream)) == OK
    s.synchronize()
    assert_same(fb.cpu().numpy(), want_fb, "sync = 0 on a side stream")
    assert_same(spp.cpu().numpy(), want_spp, "counts")
    # rt_tonemap_spp: rt_tonemap's bytes at each pixel's own divisor (the oracle's write_color)
    import oracle_bindings as ob
    got = rgb.cpu().numpy().reshape(-1, 3)
    flat, counts = want_fb.reshape(-1, 3), want_spp.ravel()
    for n in np.unique(counts):
        sel = counts == n
        assert_same(got[sel], ob.write_color_bytes(flat[sel], int(n)), f"rt_tonemap_spp n={n}")
    dev.close()


@pytest.mark.gpu
def test_refusals_enqueue_nothing_and_the_handle_stays_fresh():
    import torch
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(64, 36, 16, 50)
    dev = rb.DeviceScene(host, device=0)
    fb = torch.full((36 * 64 * 3,), float("nan"), device="cuda:0")
    spp = torch.full((36 * 64,), -1, dtype=torch.int32, device="cuda:0")
    mom = torch.full((36 * 64 * 2,), float("nan"), device="cuda:0")
    for kw, code in ((dict(min_spp=1), INVALID), (dict(batch_spp=0), INVALID), (dict(max_spp=2), INVALID), (dict(threshold=-1.0), INVALID),
                     (dict(threshold=float("nan")), INVALID), (dict(max_spp=70000), UNSUPPORTED)):
        p = rb.adaptive_params(**{**dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1), **kw})
        st = lib.rt_render_adaptive(dev._h, C.byref(cam), None, C.byref(p), C.c_void_p(fb.data_ptr()), C.c_void_p(spp.data_ptr()),
                                    C.c_void_p(mom.data_ptr()), None, 1, None)
        assert st == code, (kw, st)
    p = rb.adaptive_params(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1)
    assert lib.rt_render_adaptive(dev._h, C.byref(cam), None, C.byref(p), None, C.c_void_p(spp.data_ptr()), None, None, 1, None) == INVALID
    assert lib.rt_render_adaptive(dev._h, C.byref(cam), None, C.byref(p), C.c_void_p(fb.data_ptr()), None, None, None, 1, None) == INVALID
    bad = rb.Shard(4, 3, 7)
    assert lib.rt_render_adaptive(dev._h, C.byref(cam), C.byref(bad), C.byref(p), C.c_void_p(fb.data_ptr()), C.c_void_p(spp.data_ptr()),
                                  None, None, 1, None) == INVALID
    torch.cuda.synchronize()
    assert torch.isnan(fb).all() and (spp == -1).all() and torch.isnan(mom).all()
    # an adaptive call, then rt_render: the same bits as a fresh handle's
    t = rb.Timing()
    assert lib.rt_render_adaptive(dev._h, C.byref(cam), None, C.byref(p), C.c_void_p(fb.data_ptr()), C.c_void_p(spp.data_ptr()),
                                  C.c_void_p(mom.data_ptr()), None, 1, C.byref(t)) == OK
    assert t.kernel_ms > 0 and t.trace_launches >= 16
    after, _ = dev.render_to_host(cam)
    fresh = rb.DeviceScene(host, device=0)
    want, _ = fresh.render_to_host(cam)
    assert_same(after, want, "rt_render after an adaptive call")
    fresh.close()
    dev.close()


def _mse(fb, spp, truth):
    return float(np.mean((np.clip(fb / spp.astype(np.float32)[..., None], 0, 1) - truth) ** 2))


@pytest.mark.gpu
def test_quality_against_uniform_at_the_same_sample_count():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(320, 180, 1, 50)
    dev = rb.DeviceScene(host, device=0)
    gt_cam = rb.CameraData.from_buffer_copy(cam)
    gt_cam.samples_per_pixel = 1024
    gt, _ = dev.render_to_host(gt_cam, sample_first=1 << 20)
    truth = np.clip(gt / np.float32(1024), 0, 1)
    fb, spp, _, _ = dev.render_adaptive_to_host(cam, min_spp=8, batch_spp=8, max_spp=128, threshold=0.05)
    mean_spp = float(spp.mean())
    uniform_n = max(1, int(round(mean_spp)))
    ufb = _uniform(dev, cam, uniform_n)
    adaptive = _mse(fb, spp, truth)
    uniform = _mse(ufb, np.full(spp.shape, uniform_n, np.int32), truth)
    print(f"quality: adaptive MSE {adaptive:.6g} at {mean_spp:.2f} spp mean ({np.unique(spp).size} levels), uniform {uniform:.6g} at {uniform_n} spp, "
          f"ratio {adaptive / uniform:.4f}")
    # measured 1.695: under this metric — absolute error of the clamped mean — the relative-error rule does NOT beat
    # uniform sampling at the same sample count; the bar pins the measurement with a 10 % margin so that a regression shows
    assert adaptive <= 1.86 * uniform
    dev.close()
