"""rt_denoise_temporal and the sample ranges it needs from the renderer (rt_render_samples, rt_render_aov_samples).

The device filter is compared bit for bit, output and history buffer, with the C restatement of the header's arithmetic
(tests/denoise_temporal_reference.py) over sequences of rendered frames; with an empty history it must be rt_denoise itself.  The
sample ranges are compared with the in-order sums of rt_trace_samples radiances and with a CPU restatement of the AOV rules.  On
the CPU: the ABI, the argument checks (fake device addresses: every check comes before any HIP call) and the reference's
properties on synthetic frames.  Quality: against 1024-spp ground truths, still and moving camera."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpu_ref
import denoise_reference as dr
import denoise_temporal_reference as dtr
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = 1 << 32          # a device address that is never dereferenced
INVALID, UNSUPPORTED = 1, 4


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} bytes differ (first at {np.argwhere(bad)[0]})"


# ---- no GPU needed -----------------------------------------------------------------------------------------------------

def test_abi_mirrors_and_symbols():
    lib = rb.amd_lib()
    for s in ("rt_render_samples", "rt_render_aov_samples", "rt_denoise_history_bytes", "rt_denoise_temporal"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.CameraData) == 76
    assert len(lib.rt_denoise_temporal.argtypes) == 11 and lib.rt_denoise_history_bytes.restype is C.c_uint64
    assert lib.rt_render_samples.argtypes[3] is C.c_int32 and lib.rt_render_aov_samples.argtypes[3] is C.c_int32
    for name in ("denoise_temporal", "TemporalDenoiser"):
        assert hasattr(rb, name)


def test_history_bytes_grow_with_the_image():
    lib = rb.amd_lib()
    assert lib.rt_denoise_history_bytes(0, 5) == 0 and lib.rt_denoise_history_bytes(5, -1) == 0
    sizes = [(1, 1), (1, 2), (3, 1), (77, 45), (320, 180), (1920, 1080), (3840, 2160), (1 << 24, 1)]
    got = [lib.rt_denoise_history_bytes(w, h) for w, h in sizes]
    assert got == [dtr.history_bytes(w, h) for w, h in sizes]
    assert all(a < b for a, b in zip(got, got[1:]))


W8, H4 = 8, 4
PIX = W8 * H4


def _aov(**drop):
    b = rb.AovBuffers()
    b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count, b.first_prim = 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE, 6 * FAKE
    for field in drop:
        setattr(b, field, None)
    return b


def _call(fb=FAKE, aov="full", cam="default", params=None, prev=9 * FAKE, nxt=10 * FAKE, hist_bytes=None, ws=7 * FAKE, ws_bytes=None, out=8 * FAKE):
    lib = rb.amd_lib()
    if aov == "full":
        aov = _aov()
    if cam == "default":
        cam = rb.make_camera(W8, H4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    w, h = (cam.image_width, cam.image_height) if cam is not None else (W8, H4)
    hist_bytes = lib.rt_denoise_history_bytes(w, h) if hist_bytes is None else hist_bytes
    ws_bytes = lib.rt_denoise_workspace_bytes(w, h) if ws_bytes is None else ws_bytes
    st = lib.rt_denoise_temporal(C.c_void_p(fb), C.byref(aov) if aov is not None else None, C.byref(cam) if cam is not None else None,
                                 C.byref(params) if params else None, C.c_void_p(prev), C.c_void_p(nxt), hist_bytes, C.c_void_p(ws), ws_bytes,
                                 C.c_void_p(out), None)
    return st, lib.rt_get_last_error_string().decode()


def _cam(**fields):
    cam = rb.make_camera(W8, H4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    for k, v in fields.items():
        setattr(cam, k, v)
    return cam


def test_invalid_arguments_overlaps_and_limits_without_a_device():
    lib = rb.amd_lib()
    hist = lib.rt_denoise_history_bytes(W8, H4)
    need = lib.rt_denoise_workspace_bytes(W8, H4)
    cases = [dict(fb=0), dict(aov=None), dict(cam=None), dict(nxt=0), dict(ws=0), dict(out=0),
             dict(cam=_cam(image_width=0)), dict(cam=_cam(image_height=-3)), dict(cam=_cam(samples_per_pixel=0)),
             dict(cam=_cam(samples_per_pixel=65537)), dict(ws_bytes=need - 1), dict(hist_bytes=hist - 1),
             dict(prev=9 * FAKE + 4), dict(nxt=10 * FAKE + 8),
             # history_next overlapping history_prev, an input, the workspace, d_out
             dict(nxt=9 * FAKE + hist - 16), dict(nxt=9 * FAKE - hist + 16), dict(nxt=6 * FAKE + 4 * PIX - 16), dict(nxt=FAKE + 368),
             dict(nxt=7 * FAKE + need - 16), dict(nxt=8 * FAKE + 12 * PIX - 16),
             # d_out overlapping an input, the workspace, history_prev; the workspace overlapping an input, history_prev
             dict(out=6 * FAKE + 4), dict(out=2 * FAKE + 12), dict(out=7 * FAKE + 100), dict(out=9 * FAKE + hist - 4),
             dict(ws=5 * FAKE + 124), dict(ws=9 * FAKE + 64)]
    for field in ("albedo_sum", "normal_sum", "depth_sum", "hit_count", "first_prim"):
        cases.append(dict(aov=_aov(**{field: 1})))
    short = _aov()
    short.struct_bytes = 40                                           # first_prim lies past struct_bytes: it counts as NULL
    cases.append(dict(aov=short))
    for field, bad in (("iterations", -1), ("iterations", 9), ("sigma_depth", 0.0), ("sigma_depth", float("nan")),
                       ("sigma_luminance", float("inf")), ("normal_squarings", 11), ("struct_bytes", 4)):
        p = rb.denoise_params()
        setattr(p, field, bad)
        cases.append(dict(params=p))
    for kw in cases:
        st, msg = _call(**kw)
        assert st == INVALID and msg.startswith("rt_denoise_temporal:"), (kw, st, msg)
    for w, h in ((4097, 4096), (1 << 24, 2)):
        st, msg = _call(cam=_cam(image_width=w, image_height=h))
        assert st == UNSUPPORTED and "2^24" in msg, (w, h, st, msg)
    # edges that are allowed pass their check and fail a later one (nothing here may reach a launch: the addresses are fake)
    for kw in (dict(prev=0), dict(cam=_cam(samples_per_pixel=65536)), dict(params=rb.denoise_params(iterations=0)),
               dict(params=rb.denoise_params(iterations=8, normal_squarings=10)),
               dict(cam=_cam(image_width=4096, image_height=4096), ws_bytes=1 << 40)):
        st, msg = _call(hist_bytes=hist - 1, **kw)
        assert st == INVALID and "history_bytes" in msg, (kw, st, msg)


def test_cli_refuses_denoise_temporal_with_denoise_and_on_the_multi_gpu_drivers(test_config_text):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    runs = [(["--denoise", "--denoise-temporal"], {}), (["--denoise-temporal", "--devices", "1"], {}),
            (["--denoise-temporal", "--shard", "1"], {}), (["--denoise-temporal"], {"RTP_DEVICES": "2"})]
    for extra, env in runs:
        out = subprocess.run([exe, "--gpu"] + extra, input=test_config_text, capture_output=True, text=True, timeout=120,
                             env={**os.environ, **env})
        assert out.returncode == 2 and "--denoise-temporal" in out.stderr, (extra, out.returncode, out.stderr)


# ---- the C reference's properties (synthetic frames) ---------------------------------------------------------------------

def _synthetic(cam, rng, prim=0, fb=None, depth=8.0):
    """A frame of cam whose every sample hits a surface facing the camera at ray parameter `depth`."""
    w, h, s = cam.image_width, cam.image_height, np.float32(cam.samples_per_pixel)
    if fb is None:
        fb = (rng.exponential(0.4, (h, w, 3)) * s).astype(np.float32)
    aov = {"albedo": np.full((h, w, 3), 0.5 * s, np.float32), "normal": np.broadcast_to(np.float32([0, 0, s]), (h, w, 3)).copy(),
           "depth": np.full((h, w), depth * s, np.float32), "hits": np.full((h, w), cam.samples_per_pixel, np.uint32),
           "prim": np.broadcast_to(np.asarray(prim, np.int32), (h, w)).copy()}
    return np.ascontiguousarray(fb, np.float32), aov


def _still_cam(w=40, h=24, spp=4):
    return rb.make_camera(w, h, 40.0, (0, 0, 0), (-1, 0, 0), (0.2, 0.3, 0.4), spp, 8)


def test_reference_empty_history_is_rt_denoise():
    rng = np.random.default_rng(1)
    cam = _still_cam()
    fb, aov = _synthetic(cam, rng)
    aov["hits"][3:7, 5:11] = 0                      # some sky
    fb2, aov2 = _synthetic(cam, rng)
    _, hist = dtr.reference(fb2, aov2, cam)         # a real history of this size, then made unusable three ways
    zero = np.zeros_like(hist)
    other_cam = _still_cam(41, 24)
    _, other = dtr.reference(*_synthetic(other_cam, rng), other_cam)
    for it in (0, 1, 5):
        want = dr.reference(fb, aov, 4, iterations=it)
        got, nxt = dtr.reference(fb, aov, cam, None, iterations=it)
        assert_same(got, want, f"empty history, {it} iterations")
        for prev, what in ((zero, "all-zero history"), (other, "history of another size")):
            g, n = dtr.reference(fb, aov, cam, prev, iterations=it)
            assert_same(g, want, what)
            assert_same(n, nxt, what + " (next history)")
        moments = dtr.planes(nxt, cam.image_width, cam.image_height)["moments"]
        assert (moments[..., 2][aov["hits"] > 0] == 1).all() and (moments[aov["hits"] == 0] == 0).all()


def test_reference_still_camera_reprojects_onto_itself():
    rng = np.random.default_rng(2)
    cam = _still_cam()
    w, h = cam.image_width, cam.image_height
    _, hist = dtr.reference(*_synthetic(cam, rng), cam, iterations=0)
    # colour history := the pixel's own coordinates; a black frame then gives L = (1 - 1/2) * (bilinear mean of the coordinates)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    body = np.frombuffer(hist, np.float32, offset=dtr.HEADER_BYTES).reshape(4, h, w, 4).copy()
    body[0, ..., 0], body[0, ..., 1], body[0, ..., 2] = xx, yy, 0
    hist2 = np.concatenate([hist[:dtr.HEADER_BYTES], body.view(np.uint8).ravel()])
    fb, aov = _synthetic(cam, rng, fb=np.zeros((h, w, 3), np.float32))
    _, nxt = dtr.reference(fb, aov, cam, hist2, iterations=0)
    p = dtr.planes(nxt, w, h)
    assert (p["moments"][..., 2] == 2).all()
    uv = 2 * p["colour"][..., :2]
    err = max(np.abs(uv[..., 0] - xx).max(), np.abs(uv[..., 1] - yy).max())
    assert err < 1e-3, err


def test_reference_camera_jump_behind_disoccludes_everything():
    rng = np.random.default_rng(3)
    cam = _still_cam()
    # the old camera stands beyond every point of the new frame and looks away from it
    old = rb.make_camera(cam.image_width, cam.image_height, 40.0, (-50, 0, 0), (-100, 0, 0), (0.2, 0.3, 0.4), 4, 8)
    _, hist = dtr.reference(*_synthetic(old, rng), old)
    fb, aov = _synthetic(cam, rng)
    want, want_next = dtr.reference(fb, aov, cam, None)
    got, nxt = dtr.reference(fb, aov, cam, hist)
    assert_same(got, want, "camera jump")
    assert_same(nxt, want_next, "camera jump (next history)")
    # … while the same history under a still camera is taken everywhere
    _, hist = dtr.reference(*_synthetic(cam, rng), cam)
    _, nxt = dtr.reference(fb, aov, cam, hist)
    assert (dtr.planes(nxt, cam.image_width, cam.image_height)["moments"][..., 2] == 2).all()


def test_reference_first_prim_mismatch_rejects_a_tap():
    rng = np.random.default_rng(4)
    cam = _still_cam()
    w = cam.image_width
    _, hist = dtr.reference(*_synthetic(cam, rng, prim=6), cam)
    prim = np.full((cam.image_height, w), 6, np.int32)
    prim[:, : w // 2] = 7
    fb, aov = _synthetic(cam, rng, prim=prim)
    _, nxt = dtr.reference(fb, aov, cam, hist)
    length = dtr.planes(nxt, w, cam.image_height)["moments"][..., 2]
    assert (length[:, : w // 2 - 1] == 1).all() and (length[:, w // 2 + 1:] == 2).all()
    # the moments after four frames come from the history, not the 3x3 window
    for _ in range(3):
        _, hist = dtr.reference(*_synthetic(cam, rng, prim=6), cam, hist)
    assert np.abs(dtr.planes(hist, w, cam.image_height)["moments"][..., 2] - 4).max() < 1e-5      # (a bilinear mean of 3s, +1)


# ---- on the GPU --------------------------------------------------------------------------------------------------------

def _torch_buf(n_floats, fill=float("nan")):
    import torch
    return torch.full((n_floats,), fill, dtype=torch.float32, device="cuda:0")


@pytest.mark.gpu
def test_sample_range_refused_before_anything_is_enqueued():
    import torch
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(32, 16, 4, 50)
    fb = _torch_buf(32 * 16 * 3)
    aov = {k: _torch_buf(32 * 16 * per) for k, _, _, per in rb.AOV_CHANNELS}
    b = rb.AovBuffers()
    for key, field, _, _ in rb.AOV_CHANNELS:
        setattr(b, field, aov[key].data_ptr())
    for first, code in ((-1, INVALID), (-(1 << 31), INVALID), ((1 << 30) - 3, UNSUPPORTED), ((1 << 31) - 1, UNSUPPORTED)):
        t = rb.Timing()
        st = lib.rt_render_samples(dev._h, C.byref(cam), None, first, C.c_void_p(fb.data_ptr()), None, 1, C.byref(t))
        assert st == code and "sample_first" in lib.rt_get_last_error_string().decode(), (first, st)
        st = lib.rt_render_aov_samples(dev._h, C.byref(cam), None, first, C.byref(b), None, 1, C.byref(t))
        assert st == code and "sample_first" in lib.rt_get_last_error_string().decode(), (first, st)
    torch.cuda.synchronize()
    assert torch.isnan(fb).all() and all(torch.isnan(a).all() for a in aov.values())
    # the last range that fits is rendered
    dev.render(cam, fb.data_ptr(), sample_first=(1 << 30) - 4)
    assert not torch.isnan(fb).any()
    dev.close()


@pytest.mark.gpu
def test_first_zero_is_rt_render_on_every_path():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(96, 54, 9, 50)
    shard = rb.Shard(4, 3, 1)
    for config in (dict(traversal=rb.TRAVERSAL_EXACT), dict(traversal=rb.TRAVERSAL_GUARDED), dict(traversal=rb.TRAVERSAL_GUARDED, primary_visibility=-1),
                   dict(traversal=rb.TRAVERSAL_GUARDED, pass_spp=2), dict(traversal=rb.TRAVERSAL_EXACT, pass_spp=4)):
        dev = rb.DeviceScene(host, device=0, **config)
        for sh in (None, shard):
            want, _ = dev.render_to_host(cam, shard=sh)
            import torch
            rows = rb.amd_lib().rt_shard_rows(cam.image_height, C.byref(sh) if sh else None)
            d = torch.empty((rows, cam.image_width, 3), dtype=torch.float32, device="cuda:0")
            t = rb.Timing()
            st = rb.amd_lib().rt_render_samples(dev._h, C.byref(cam), C.byref(sh) if sh else None, 0, C.c_void_p(d.data_ptr()), None, 1, C.byref(t))
            assert st == 0
            assert_same(d.cpu().numpy(), want, f"{config} shard={sh is not None}")
            aov_want, _ = dev.render_aov_to_host(cam, shard=sh)
            bufs = {k: torch.empty(rows * cam.image_width * per, dtype=torch.float32, device="cuda:0") for k, _, _, per in rb.AOV_CHANNELS}
            b = rb.AovBuffers()
            for key, field, _, _ in rb.AOV_CHANNELS:
                setattr(b, field, bufs[key].data_ptr())
            assert rb.amd_lib().rt_render_aov_samples(dev._h, C.byref(cam), C.byref(sh) if sh else None, 0, C.byref(b), None, 1, C.byref(t)) == 0
            for key, _, dtype, _ in rb.AOV_CHANNELS:
                assert_same(bufs[key].cpu().numpy().view(dtype).reshape(aov_want[key].shape), aov_want[key], f"AOV {key} {config}")
        dev.close()


@pytest.mark.gpu
def test_sample_offsets_are_the_samples_they_name():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    spp = 4
    cam = rb.rtiow_camera(20, 12, spp, 50)
    w, h = cam.image_width, cam.image_height
    lib = _aov_samples_lib()
    for config in (dict(traversal=rb.TRAVERSAL_EXACT), dict(traversal=rb.TRAVERSAL_GUARDED)):
        dev = rb.DeviceScene(host, device=0, **config)
        for first in (7, 1000, (1 << 30) - spp):
            fb, _ = dev.render_to_host(cam, sample_first=first)
            jj, ii, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(first, first + spp), indexing="ij")
            ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], axis=1).astype(np.int32)
            rad, _, _ = dev.trace_samples(cam, ijs)
            rad = rad.reshape(h, w, spp, 3)
            acc = np.zeros((h, w, 3), np.float32)
            for s in range(spp):
                acc = (acc + rad[:, :, s]).astype(np.float32)
            assert_same(fb, acc, f"{config} first={first}")
            got, _ = dev.render_aov_to_host(cam, sample_first=first)
            want = _aov_samples(lib, host, cam, first)
            for key in want:
                assert_same(got[key], want[key], f"AOV {key} first={first}")
        dev.close()


def _aov_samples_lib():
    l = cpu_ref.build("aov_samples_ref.c", "oracle/rt_oracle.c")
    l.aov_samples_reference.argtypes = [C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.c_int32] + [C.c_void_p] * 5
    l.aov_samples_reference.restype = None
    return l


def _aov_samples(lib, host, cam, first):
    w, h = cam.image_width, cam.image_height
    out = {"albedo": np.zeros((h, w, 3), np.float32), "normal": np.zeros((h, w, 3), np.float32), "depth": np.zeros((h, w), np.float32),
           "hits": np.zeros((h, w), np.uint32), "prim": np.zeros((h, w), np.int32)}
    lib.aov_samples_reference(C.byref(host.desc), C.byref(cam), first, *[out[k].ctypes.data for k in ("albedo", "normal", "depth", "hits", "prim")])
    return out


def _frame(dev, cam, first=0):
    fb, _ = dev.render_to_host(cam, sample_first=first)
    aov, _ = dev.render_aov_to_host(cam, sample_first=first)
    return fb, aov


def _sequence(host, frames, what, resets=(), **params):
    """frames: [(cam, sample_first)].  The device TemporalDenoiser against the C reference, output and history, frame by frame."""
    dev = rb.DeviceScene(host, device=0)
    cam0 = frames[0][0]
    td = rb.TemporalDenoiser(cam0.image_width, cam0.image_height, **params)
    prev = None
    outs = []
    for n, (cam, first) in enumerate(frames):
        if n in resets:
            td.reset()
            prev = None
        fb, aov = _frame(dev, cam, first)
        got = td.step_to_host(fb, aov, cam)
        want, prev = dtr.reference(fb, aov, cam, prev, **params)
        assert_same(got, want, f"{what}: frame {n} {params}")
        assert_same(td.history_to_host(), prev, f"{what}: history after frame {n}")
        outs.append((got, fb, aov))
    td.close()
    dev.close()
    return outs


@pytest.mark.gpu
def test_config_scene_along_its_orbit(test_config_text):
    rb.amd_lib().rt_set_device(0)
    text = test_config_text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    _sequence(host, [(host.frame_camera(n), 0) for n in (0, 1, 2, 3)], "config orbit")


@pytest.mark.gpu
def test_rtiow_still_camera_with_sample_offsets_and_a_reset():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(77, 45, 4, 50)
    _sequence(host, [(cam, 4 * k) for k in range(6)], "rtiow still", resets=(3,))
    _sequence(host, [(cam, 4 * k) for k in range(5)], "rtiow still", iterations=0)
    _sequence(host, [(cam, 4 * k) for k in range(5)], "rtiow still", iterations=1, sigma_luminance=2.0, normal_squarings=3)
    _sequence(host, [(cam, 4 * k) for k in range(3)], "rtiow still", iterations=8, sigma_depth=0.5)


@pytest.mark.gpu
def test_odd_thin_tiny_and_all_sky_frames():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    for w, h in ((45, 1), (1, 77), (1, 1), (33, 17)):
        cam = rb.rtiow_camera(w, h, 4, 50)
        _sequence(host, [(cam, 4 * k) for k in range(3)], f"{w}x{h}")
    orbit = [rb.make_camera(64, 36, 20.0, (13 * np.cos(a), 3, 13 * np.sin(a)), (0, 0, 0), (0.7, 0.8, 1.0), 4, 50) for a in (0.15, 0.17, 0.19)]
    _sequence(host, [(c, 0) for c in orbit], "small orbit")
    sky = rb.make_camera(120, 80, 20.0, (13, 3, 2), (26, 6, 40), (0.3, 0.5, 0.9), 3, 50)
    outs = _sequence(host, [(sky, 0), (sky, 3)], "all sky")
    for got, fb, aov in outs:
        assert not aov["hits"].any()
        assert_same(got, fb, "all sky passes through")


@pytest.mark.gpu
def test_empty_history_on_the_device_is_rt_denoise():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(160, 90, 8, 50)
    fb, aov = _frame(dev, cam)
    for it in (0, 1, 5):
        td = rb.TemporalDenoiser(160, 90, iterations=it)
        assert_same(td.step_to_host(fb, aov, cam), rb.denoise_to_host(fb, aov, 8, iterations=it), f"empty history, {it} iterations")
        td.close()
    dev.close()


@pytest.mark.gpu
def test_side_stream_and_a_headline_frame_pair():
    import torch
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(200, 120, 4, 50)
    lib = rb.amd_lib()
    hist_bytes = lib.rt_denoise_history_bytes(200, 120)
    hist = [torch.zeros(hist_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    ws = torch.empty(lib.rt_denoise_workspace_bytes(200, 120), dtype=torch.uint8, device="cuda:0")
    prev = None
    stream = torch.cuda.Stream()
    for n in range(3):
        fb, aov = _frame(dev, cam, 4 * n)
        t = {"fb": torch.from_numpy(fb).to("cuda:0")}
        for key, _, dtype, _ in rb.AOV_CHANNELS:
            t[key] = torch.from_numpy(aov[key].view(np.float32) if dtype != np.float32 else aov[key]).to("cuda:0")
        out = torch.full_like(t["fb"], float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            # frame 0 reads the zero-filled buffer: an empty history
            rb.denoise_temporal(t["fb"].data_ptr(), {k: t[k].data_ptr() for k, _, _, _ in rb.AOV_CHANNELS}, cam, hist[(n + 1) & 1].data_ptr(),
                                hist[n & 1].data_ptr(), hist_bytes, out.data_ptr(), (ws.data_ptr(), ws.numel()), stream=stream.cuda_stream)
        stream.synchronize()
        want, prev = dtr.reference(fb, aov, cam, prev)
        assert_same(out.cpu().numpy(), want, f"side stream frame {n}")
        assert_same(hist[n & 1].cpu().numpy(), prev, f"side stream history {n}")
    cam = rb.rtiow_camera(1920, 1080, 2, 50)
    _sequence(host, [(cam, 0), (cam, 2)], "1920x1080")
    dev.close()


@pytest.mark.gpu
def test_cli_writes_the_temporal_sequence(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    lines = test_config_text.split("\n")
    lines[0] = "3"
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines)
    out = subprocess.run([exe, "--gpu", "--denoise-temporal"], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.from_config(text)
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera(0)
    td = rb.TemporalDenoiser(cam.image_width, cam.image_height)
    for n in range(3):
        cam = host.frame_camera(n)
        fb, aov = _frame(dev, cam)
        want = td.step_to_host(fb, aov, cam)
        data = open(tmp_path / f"f_{n}.png.denoised", "rb").read()
        assert data == rb.binary_image_bytes(want, cam.image_width, cam.image_height, host.info.sqrt_spp), n
    td.close()
    dev.close()


def _mse(fb, spp, truth):
    return float(np.mean((np.clip(fb / np.float32(spp), 0, 1) - truth) ** 2))


def _temporal_against_spatial(host, cams, spp):
    """MSE against 1024 spp at the last camera: (temporal output of the last frame, spatial rt_denoise of the last frame alone,
    the noisy last frame)."""
    dev = rb.DeviceScene(host, device=0)
    td = rb.TemporalDenoiser(cams[0].image_width, cams[0].image_height)
    for k, cam in enumerate(cams):
        fb, aov = _frame(dev, cam, spp * k)
        out = td.step_to_host(fb, aov, cam)
    gt_cam = rb.CameraData.from_buffer_copy(cams[-1])
    gt_cam.samples_per_pixel = 1024
    gt, _ = dev.render_to_host(gt_cam, sample_first=1 << 20)
    truth = np.clip(gt / np.float32(1024), 0, 1)
    spatial = rb.denoise_to_host(fb, aov, spp)
    td.close()
    dev.close()
    return _mse(out, spp, truth), _mse(spatial, spp, truth), _mse(fb, spp, truth)


@pytest.mark.gpu
def test_quality_still_camera_against_1024_spp():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(320, 180, 4, 50)
    temporal, spatial, noisy = _temporal_against_spatial(host, [cam] * 8, 4)
    print(f"quality still: temporal MSE {temporal:.6g}, spatial {spatial:.6g}, noisy {noisy:.6g}, temporal / spatial {temporal / spatial:.4f}")
    assert temporal <= 0.75 * spatial          # measured 0.618


@pytest.mark.gpu
def test_quality_moving_orbit_against_1024_spp():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    r, a0 = float(np.hypot(13, 2)), float(np.arctan2(2, 13))
    cams = [rb.make_camera(320, 180, 20.0, (r * np.cos(a0 + 0.004 * k), 3, r * np.sin(a0 + 0.004 * k)), (0, 0, 0), (0.7, 0.8, 1.0), 4, 50)
            for k in range(8)]
    temporal, spatial, noisy = _temporal_against_spatial(host, cams, 4)
    print(f"quality orbit: temporal MSE {temporal:.6g}, spatial {spatial:.6g}, noisy {noisy:.6g}, temporal / spatial {temporal / spatial:.4f}")
    assert temporal <= 0.85 * spatial          # measured 0.709
