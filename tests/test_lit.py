"""rt_render_lit / rt_trace_samples_lit: emitters, environment and lens in one frame (include/rtp_amd.h).

The header composes rt_render_lens's camera, rt_render_nee's light sample and rt_render_env's light sample and fixes their order;
tests/cpu_native/lit_ref.c restates that on the oracle (lit_reference.py), and probed samples and frames must equal it bit for bit.  On
the CPU: the ABI, every argument check, the restatement's three identities against the three existing restatements, its expectation
(by z-scores) and the CLI refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import env_reference as er
import lens_reference as lensr
import lit_reference as lr
import nee_reference as nr
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
OK, INVALID = 0, 1
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_LIGHT = 0, 1, 2, 3
LUM = np.array([0.2126, 0.7152, 0.0722])
LENS = (0.2, 12.0)


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} bytes differ (first at {np.argwhere(bad)[0]})"


# ---- scenes and cameras (test_env.py's) ---------------------------------------------------------------------------------------------

def config_host(text):
    return rb.HostScene.from_config(text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg")))


def config_camera(host, frame, w=96, h=64, spp=4, depth=50):
    cam = rb.CameraData.from_buffer_copy(host.frame_camera(frame))
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, spp, depth
    return cam


def material(kind, albedo=(0.5, 0.5, 0.5), emit=(0, 0, 0), fuzz=0.0, ir=1.5):
    m = rb.Material()
    m.type = kind
    m.fuzz = fuzz
    m.ir = ir
    for k in range(3):
        m.albedo.e[k] = albedo[k]
        m.emit.e[k] = emit[k]
    return m


def night_rtiow():
    """rtiow with every eighth small sphere made DIFFUSE_LIGHT."""
    base = rb.HostScene.rtiow()          # (kept alive: desc points into it)
    d = base.desc
    spheres, mats = [], []
    for i in range(d.num_spheres):
        s = d.spheres[i]
        m = d.materials[s.material_idx]
        if 0 < i < d.num_spheres - 3 and i % 8 == 5:
            m = material(MAT_LIGHT, emit=(6.0, 4.5, 3.0) if i % 16 == 5 else (1.5, 2.0, 3.0))
        spheres.append([s.center.e[0], s.center.e[1], s.center.e[2], s.radius, len(mats)])
        mats.append(rb.Material.from_buffer_copy(m))
    night = rb.HostScene.from_arrays(np.array(spheres, np.float32), np.zeros((0, 11), np.float32), mats)
    base.close()
    return night


def night_camera(w, h, spp, max_depth=50, background=(0, 0, 0), eye=(13, 3, 2)):
    return rb.make_camera(w, h, 20.0, eye, (0, 0, 0), background, spp, max_depth)


def three_ball_scene(spp=8192, depth=6, lamp=False, w=8, h=8):
    """LAMBERTIAN floor sphere, a METAL and a LAMBERTIAN ball (test_env.py's); lamp: plus one DIFFUSE_LIGHT sphere above them."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_METAL, (0.8, 0.7, 0.5), fuzz=0.4), material(MAT_LAMBERTIAN, (0.3, 0.5, 0.8))]
    sph = [[0, -100, 0, 100, 0], [-1.1, 1, 0, 1, 1], [1.1, 1, 0, 1, 2]]
    if lamp:
        mats.append(material(MAT_LIGHT, emit=(8.0, 6.0, 4.0)))
        sph.append([0, 2.6, 0.5, 0.3, 3])
    cam = rb.make_camera(w, h, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), spp, depth)
    return rb.HostScene.from_arrays(np.array(sph, np.float32), np.zeros((0, 11), np.float32), mats), cam


def scaled(cam, w, h, spp, depth):
    c = rb.CameraData.from_buffer_copy(cam)
    c.image_width, c.image_height, c.samples_per_pixel, c.max_depth = w, h, spp, depth
    return c


def write_pfm(path, img, little=True):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n{'-1.0' if little else '1.0'}\n".encode())
        f.write(img[::-1].astype("<f4" if little else ">f4").tobytes())


# A setting of the call: what both lit_reference and the bindings take, under their own names
def setting(close=None, lens=None, emitters=True, mis=1, m=None, ep=None):
    return dict(close=close, lens=lens, emitters=emitters, mis=mis, m=m, ep=ep)


def ref_args(s):
    return dict(cam_close=s["close"], lens=s["lens"], emitters=s["emitters"], nee_mis=s["mis"], rgb=s["m"], env_params=s["ep"])


def dev_args(s, env):
    return dict(cam_close=s["close"], lens=None if s["lens"] is None else dict(lens_radius=s["lens"][0], focus_distance=s["lens"][1]),
                emitters=s["emitters"], nee=dict(mis=s["mis"]), env=env if s["m"] is not None else None, env_params=s["ep"])


def four_settings(m, close, rot):
    ep = lambda mode: dict(mode=mode, scale=0.75, **({"rot": rot} if rot is not None else {}))
    return [("both MIS, lens, motion", setting(close, LENS, True, 1, m, ep(1))),
            ("both light-only, pinhole", setting(None, None, True, 0, m, ep(2))),
            ("emitters off, env MIS, lens", setting(None, LENS, False, 1, m, ep(1))),
            ("emitters, no env, motion", setting(close, None, True, 1, None, None))]


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_symbols_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_lit_params_init", "rt_render_lit", "rt_trace_samples_lit"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.LitParams) == 8 + 5 * C.sizeof(C.c_void_p)
    assert len(lib.rt_render_lit.argtypes) == 9 and len(lib.rt_trace_samples_lit.argtypes) == 10
    p = rb.LitParams()
    p.sample_emitters = 7
    p.env = 5
    lib.rt_lit_params_init(C.byref(p))
    assert (p.struct_bytes, p.sample_emitters) == (C.sizeof(rb.LitParams), 1)
    assert not p.cam_close and not p.lens and not p.nee and not p.env and not p.env_params
    lib.rt_lit_params_init(None)
    q = rb.lit_params(emitters=False, lens=dict(lens_radius=0.5), nee=dict(mis=0), env_params=dict(mode=2))
    assert q.sample_emitters == 0 and q.lens.contents.lens_radius == 0.5 and q.nee.contents.mis == 0 and q.env_params.contents.mode == 2
    for name in ("render_lit", "render_lit_to_host", "trace_samples_lit"):
        assert hasattr(rb.DeviceScene, name)


def _calls(cam, lit):
    """(status, message) of rt_render_lit and of rt_trace_samples_lit with a null scene."""
    lib = rb.amd_lib()
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    pc = C.byref(cam) if cam is not None else None
    pl = C.byref(lit) if lit is not None else None
    out = [lib.rt_render_lit(None, pc, pl, None, 0, C.c_void_p(1 << 32), None, 1, None), lib.rt_get_last_error_string().decode()]
    out += [lib.rt_trace_samples_lit(None, pc, pl, 1, ijs, f, r, s, s, s), lib.rt_get_last_error_string().decode()]
    return out


def test_argument_checks_come_first():
    """Every refusal of rt_render_lens, rt_render_nee and rt_render_env is rt_render_lit's, before the scene is looked at (it is null
    here, and no device is needed); parameters that pass reach the null-scene check."""
    cam = rb.rtiow_camera(8, 4, 2)
    fake_env = 1 << 32        # (never dereferenced: the scene is null)

    def refused(word, cam=cam, **kw):
        lit = kw.pop("lit", None) or rb.lit_params(**kw)
        st1, m1, st2, m2 = _calls(cam, lit)
        assert st1 == INVALID and word in m1 and "rt_render_lit" in m1, (word, kw, m1)
        assert st2 == INVALID and word in m2 and "rt_trace_samples_lit" in m2, (word, kw, m2)

    def with_env(**kw):
        lit = rb.lit_params(**kw)
        lit.env = fake_env
        return lit
    # rt_lit_params itself
    short = rb.lit_params()
    short.struct_bytes = 4
    refused("struct_bytes", lit=short)
    for bad in (2, -1):
        two = rb.lit_params()
        two.sample_emitters = bad
        refused("sample_emitters", lit=two)
    # rt_render_lens's
    assert _calls(None, rb.lit_params())[0] == INVALID and "null camera" in _calls(None, rb.lit_params())[1]
    for field, value in (("image_width", 9), ("image_height", 5), ("samples_per_pixel", 3), ("max_depth", 7)):
        close = rb.CameraData.from_buffer_copy(cam)
        setattr(close, field, value)
        refused("cam_close", cam_close=close)
    close = rb.CameraData.from_buffer_copy(cam)
    close.background.e[1] += 0.5
    refused("cam_close", cam_close=close)
    for r in (-0.1, float("nan"), float("inf")):
        refused("lens_radius", lens=dict(lens_radius=r))
    for fd in (0.0, -1.0, float("nan"), float("inf")):
        refused("focus_distance", lens=dict(lens_radius=0.1, focus_distance=fd))
    flat = rb.CameraData.from_buffer_copy(cam)
    for k in range(3):
        flat.pixel00_loc.e[k] = flat.origin.e[k]
    refused("image plane", cam=flat, lens=dict(lens_radius=0.1))
    lens_short = rb.lens_params()
    lens_short.struct_bytes = 4
    refused("struct_bytes", lens=lens_short)
    # rt_render_nee's (read only when sample_emitters != 0)
    refused("mis", nee=dict(mis=2))
    refused("mis", nee=dict(mis=-1))
    nee_short = rb.nee_params()
    nee_short.struct_bytes = 7
    refused("struct_bytes", nee=nee_short)
    assert "null scene" in _calls(cam, rb.lit_params(emitters=False, nee=dict(mis=2)))[1]
    # rt_render_env's (read only when env != NULL)
    tilted = [1, 0, 0, 0, 1, 0, 0, 1e-3, 1]
    for word, kw in (("mode", dict(mode=-1)), ("mode", dict(mode=3)), ("scale", dict(scale=-0.5)), ("scale", dict(scale=float("nan"))),
                     ("scale", dict(scale=float("inf"))), ("camera_visible", dict(camera_visible=2)), ("rot", dict(rot=[0] * 9)),
                     ("rot", dict(rot=tilted))):
        refused(word, lit=with_env(env_params=kw))
        assert "null scene" in _calls(cam, rb.lit_params(env_params=kw))[1], kw
    env_short = rb.env_params()
    env_short.struct_bytes = 4
    refused("struct_bytes", lit=with_env(env_params=env_short))
    # the order: lens before emitters before environment
    both = with_env(lens=dict(lens_radius=-1.0), nee=dict(mis=2), env_params=dict(mode=3))
    assert "lens_radius" in _calls(cam, both)[1]
    both = with_env(nee=dict(mis=2), env_params=dict(mode=3))
    assert "mis" in _calls(cam, both)[1]
    # good parameters reach the scene; lit == NULL is the defaults
    good = [None, rb.lit_params(), rb.lit_params(emitters=False), with_env(env_params=dict(mode=2, rot=er.Z_UP, camera_visible=0)),
            with_env(cam_close=rb.CameraData.from_buffer_copy(cam), lens=dict(lens_radius=0.2, focus_distance=12.0), nee=dict(mis=0))]
    for lit in good:
        st1, m1, st2, m2 = _calls(cam, lit)
        assert st1 == INVALID and "null scene" in m1, m1
        assert st2 == INVALID, m2
    # an older caller's 8-byte struct: sample_emitters is read, the pointers keep their defaults
    old = with_env(env_params=dict(mode=3))
    old.struct_bytes = 8
    assert "null scene" in _calls(cam, old)[1]
    old.sample_emitters = 2
    assert "sample_emitters" in _calls(cam, old)[1]
    assert rb.amd_lib().rt_trace_samples_lit(None, C.byref(cam), None, -1, None, None, None, None, None, None) == INVALID


def _identity_cases(test_config_text):
    host = config_host(test_config_text)
    yield "config", host, lambda d, spp=4: config_camera(host, 11, 32, 24, spp, d), er.Z_UP
    night = night_rtiow()
    yield "night rtiow", night, lambda d, spp=4: night_camera(32, 24, spp, d, background=(0.05, 0.1, 0.2)), None


def test_restatement_reduces_to_the_three_restatements(test_config_text):
    """The identities of the header on the restatements: no environment, pinhole = nee_reference; no emitter samples, pinhole =
    env_reference; neither light = lens_reference (with and without lens and motion)."""
    m = er.sun_and_sky(256)
    shard = rb.Shard(4, 3, 2)
    for name, host, camera, rot in _identity_cases(test_config_text):
        for depth in (2, 50):
            cam = camera(depth)
            close = rb.CameraData.from_buffer_copy(cam)
            close.origin.e[0] += 0.3
            close.pixel00_loc.e[0] += 0.3
            for sh, first in ((None, 0), (shard, 0), (None, 37)):
                what = f"{name} depth={depth} shard={sh is not None} first={first}"
                kw = dict(shard=sh, sample_first=first, threads=8)
                for mis in (1, 0):
                    assert_same(lr.frame(host, cam, emitters=True, nee_mis=mis, **kw), nr.frame(host, cam, mis=mis, **kw), f"nee mis={mis} {what}")
                for mode in (0, 1, 2):
                    p = dict(mode=mode, scale=0.75, camera_visible=mode != 2)
                    if rot is not None:
                        p["rot"] = rot
                    assert_same(lr.frame(host, cam, emitters=False, rgb=m, env_params=p, **kw), er.frame(host, cam, m, p, **kw), f"env mode={mode} {what}")
                for c, lens in ((None, None), (close, None), (None, LENS), (close, LENS)):
                    want = lensr.frame(host, cam, c, *(lens or (0.0, 10.0)), **kw)
                    assert_same(lr.frame(host, cam, cam_close=c, lens=lens, emitters=False, **kw), want, f"lens {lens} motion={c is not None} {what}")
    # an empty emitter table is sample_emitters = 0
    host, cam = three_ball_scene(spp=4, w=32, h=24)
    p = dict(mode=1)
    assert_same(lr.frame(host, cam, emitters=True, rgb=m, env_params=p), er.frame(host, cam, m, p), "no emitter in the scene")


def _zscores(m_a, m_b, spp):
    """Luminance z-scores of two estimators from their channel sums and sums of squares (test_env.py's)."""
    def stats(m):
        mean = m[..., :3] / spp
        ex2 = m[..., 3:] / spp
        var = np.maximum(ex2 - mean * mean, 0) * spp / (spp - 1)
        return mean @ LUM, var @ (LUM * LUM)
    ma, va = stats(m_a)
    mb, vb = stats(m_b)
    return (ma - mb) / np.sqrt((va + vb) / spp + 1e-30)


def test_restatement_is_unbiased():
    """The three-ball scene with a lamp under the sun-and-sky map, 8 x 8 pixels x 8192 samples from disjoint sample ranges: both
    lights with MIS against the path alone (no emitter samples, env mode 0) per 4 x 4 block within 5 sigma and over the image within
    4; both lights sampled alone (nee.mis = 0, env mode 2) against MIS per 2 x 2 block within 5 sigma."""
    host, cam = three_ball_scene(lamp=True)
    spp = cam.samples_per_pixel
    m = er.sun_and_sky(256)
    _, mis = lr.frame(host, cam, emitters=True, nee_mis=1, rgb=m, env_params=dict(mode=1), sample_first=0, moments=True)
    _, path = lr.frame(host, cam, emitters=False, rgb=m, env_params=dict(mode=0), sample_first=spp, moments=True)
    _, light = lr.frame(host, cam, emitters=True, nee_mis=0, rgb=m, env_params=dict(mode=2), sample_first=2 * spp, moments=True)

    def blocks(x, b):
        return x.reshape(8 // b, b, 8 // b, b, 6).sum((1, 3))
    z = _zscores(blocks(mis, 4), blocks(path, 4), spp * 16)
    print("MIS against the path alone, 4 x 4 blocks:", np.abs(z).max())
    assert np.abs(z).max() < 5.0, np.abs(z).max()
    za = _zscores(mis.sum((0, 1)), path.sum((0, 1)), spp * 64)
    print("MIS against the path alone, image:", za)
    assert abs(za) < 4.0, za
    z = _zscores(blocks(light, 2), blocks(mis, 2), spp * 4)
    print("light-only against MIS, 2 x 2 blocks:", np.abs(z).max())
    assert np.abs(z).max() < 5.0, np.abs(z).max()


def test_cli_refusals(test_config_text, tmp_path):
    good = str(tmp_path / "sky.pfm")
    write_pfm(good, np.ones((4, 8, 3), np.float32))
    before = sorted(os.listdir(tmp_path))

    def run(args, env=None):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                              env={**os.environ, **(env or {})})
    cases = [(["--lit", "--adaptive", "0.1"], {}), (["--lit", "--denoise-temporal"], {}), (["--lit", "--devices", "2"], {}),
             (["--lit", "--shard", "2"], {}), (["--lit"], {"RTP_DEVICES": "2"}), (["--lit", "--env", good, "--nee", "--shard", "2"], {}),
             (["--lens", "0.2:12", "--lit", "--adaptive", "0.1"], {})]
    for args, env in cases:
        r = run(args, env)
        assert r.returncode == 99 and "--lit" in r.stderr, (args, env, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    # bad values of the combined flags are still refused under --lit, by their own messages
    for args, word in ((["--lit", "--nee", "both"], "--nee"), (["--lit", "--lens", "x"], "--lens"), (["--lit", "--motion-blur", "2"], "--motion-blur"),
                       (["--lit", "--env", good, "--env-mode", "both"], "--env"), (["--lit", "--env-mode", "mis"], "--env")):
        r = run(args)
        assert r.returncode == 99 and word in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    # without --lit the combinations stay refused
    for args, word in ((["--env", good, "--nee"], "--env"), (["--env", good, "--lens", "0.1:10"], "--env"), (["--nee", "--lens", "0.1:10"], "--nee")):
        r = run(args)
        assert r.returncode == 99 and word in r.stderr and "--lit" not in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _gpu_scenes(test_config_text, w, h, spp, depth=50, config_frame=5):
    host = config_host(test_config_text)
    cam = scaled(host.frame_camera(config_frame), w, h, spp, depth) if w else host.frame_camera(config_frame)
    close = rb.CameraData.from_buffer_copy(host.frame_camera_at(config_frame + 0.5))
    close.image_width, close.image_height, close.samples_per_pixel, close.max_depth = cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth
    yield "config", host, cam, close, er.Z_UP
    night = night_rtiow()
    nw, nh = (w, h) if w else (320, 180)
    yield "night rtiow", night, night_camera(nw, nh, spp, depth), night_camera(nw, nh, spp, depth, eye=(12.6, 3.2, 2.5)), None


@pytest.mark.gpu
def test_probe_samples_equal_the_restatement(test_config_text):
    rb.amd_lib().rt_set_device(0)
    rng = np.random.default_rng(15)
    n = 4000
    m = er.sun_and_sky(256)
    with rb.Env(m) as env:
        for name, host, cam, close, rot in _gpu_scenes(test_config_text, 0, 0, 1):
            dev = rb.DeviceScene(host, device=0)
            ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)
            settings = four_settings(m, close, rot)
            for what, s in settings:
                got = dev.trace_samples_lit(cam, ijs, **dev_args(s, env))
                want = lr.trace(host, cam, ijs, **ref_args(s))
                for g, w_, col in zip(got, want, ("radiance", "rays", "seed", "nee seed", "env seed")):
                    assert_same(g, w_, f"{name}, {what}: {col}")
                start = lr.trace(host, scaled(cam, cam.image_width, cam.image_height, 1, 0), ijs, **ref_args(s))
                if not s["emitters"]:
                    assert_same(got[3], start[3], f"{name}, {what}: the emitter stream never advances")
                if s["m"] is None:
                    assert_same(got[4], start[4], f"{name}, {what}: the environment stream never advances")
            if name == "night rtiow":
                # both lights cost more shadow rays than either alone (the same camera and path: the streams do not touch the path's)
                s = settings[0][1]
                for trace in (lambda **kw: dev.trace_samples_lit(cam, ijs, **dev_args(setting(**kw), env)),
                              lambda **kw: lr.trace(host, cam, ijs, **ref_args(setting(**kw)))):
                    both = trace(**s)[1]
                    emitters_only = trace(**{**s, "m": None, "ep": None})[1]
                    env_only = trace(**{**s, "emitters": False})[1]
                    more = ((both > emitters_only) & (both > env_only)).mean()
                    print(f"{name}: samples with more rays than either single light: {more:.4f}")
                    assert more > 0.02, more
            dev.close()


@pytest.mark.gpu
def test_frames_equal_the_restatement(test_config_text):
    rb.amd_lib().rt_set_device(0)
    m = er.sun_and_sky(256)
    shard = rb.Shard(4, 3, 2)
    with rb.Env(m) as env:
        for depth in (2, 50):
            for name, host, cam, close, rot in _gpu_scenes(test_config_text, 64, 48, 4, depth, config_frame=11):
                dev = rb.DeviceScene(host, device=0)
                for what, s in four_settings(m, close, rot)[:2]:
                    for sh, first in ((None, 0), (shard, 0), (None, 37)):
                        got, t = dev.render_lit_to_host(cam, shard=sh, sample_first=first, **dev_args(s, env))
                        want = lr.frame(host, cam, shard=sh, sample_first=first, **ref_args(s))
                        assert_same(got, want, f"{name} depth={depth}, {what}, shard={sh is not None} first={first}")
                        assert t.guarded == 0 and t.trace_scratch_bytes == 0 and t.trace_launches >= 1, (t.guarded, t.trace_scratch_bytes)
                    # camera_visible = 0 with a background that is not black
                    bg, bg_close = rb.CameraData.from_buffer_copy(cam), rb.CameraData.from_buffer_copy(close)
                    for c in (bg, bg_close):
                        c.background.e[0], c.background.e[1], c.background.e[2] = 0.3, 0.1, 0.2
                    hidden = dict(s, ep=dict(s["ep"], camera_visible=0), close=bg_close if s["close"] is not None else None)
                    got, _ = dev.render_lit_to_host(bg, **dev_args(hidden, env))
                    assert_same(got, lr.frame(host, bg, **ref_args(hidden)), f"{name} depth={depth}, {what}, camera_visible=0")
                dev.close()


@pytest.mark.gpu
def test_identities_against_the_existing_calls(test_config_text):
    rb.amd_lib().rt_set_device(0)
    m = er.sun_and_sky(256)
    with rb.Env(m) as env:
        for name, host, cam, close, rot in _gpu_scenes(test_config_text, 64, 48, 4, config_frame=11):
            p = dict(mode=1, scale=0.75)
            if rot is not None:
                p["rot"] = rot
            lens = dict(lens_radius=LENS[0], focus_distance=LENS[1])
            for config in (dict(), dict(traversal=rb.TRAVERSAL_EXACT)):
                dev = rb.DeviceScene(host, device=0, **config)
                for first in (0, 5):
                    what = f"{name} {config} first={first}"
                    for mis in (1, 0):
                        got, _ = dev.render_lit_to_host(cam, nee=dict(mis=mis), sample_first=first)
                        assert_same(got, dev.render_nee_to_host(cam, params=dict(mis=mis), sample_first=first)[0], f"rt_render_nee mis={mis} {what}")
                    got, _ = dev.render_lit_to_host(cam, emitters=False, env=env, env_params=p, sample_first=first)
                    assert_same(got, dev.render_env_to_host(cam, env, params=p, sample_first=first)[0], f"rt_render_env {what}")
                    for c, l in ((None, None), (close, lens)):
                        got, _ = dev.render_lit_to_host(cam, cam_close=c, lens=l, emitters=False, sample_first=first)
                        assert_same(got, dev.render_lens_to_host(cam, cam_close=c, lens=l, sample_first=first)[0], f"rt_render_lens {l} {what}")
                    got, _ = dev.render_lit_to_host(cam, emitters=False, sample_first=first)
                    assert_same(got, dev.render_to_host(cam, sample_first=first)[0], f"rt_render_samples {what}")
                dev.close()
    # an empty emitter table with an environment is rt_render_env
    host, cam = three_ball_scene(spp=4, w=64, h=48)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(m) as env:
        assert_same(dev.render_lit_to_host(cam, env=env)[0], dev.render_env_to_host(cam, env)[0], "no emitter in the scene")
    dev.close()


@pytest.mark.gpu
def test_handle_state_streams_and_sharing():
    import torch
    rb.amd_lib().rt_set_device(0)
    m = er.sun_and_sky(256)
    env = rb.Env(m)
    host = night_rtiow()
    cam, close = night_camera(128, 72, 8), night_camera(128, 72, 8, eye=(12.6, 3.2, 2.5))
    kw = dict(cam_close=close, lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), env=env)
    dev = rb.DeviceScene(host, device=0)
    first, _ = dev.render_to_host(cam)
    before = dev.last_timing()
    lit, t = dev.render_lit_to_host(cam, **kw)
    assert t.guarded == 0 and t.trace_launches >= 1 and t.kernel_ms > 0
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    assert_same(dev.render_to_host(cam)[0], first, "rt_render after rt_render_lit")
    # the emitter table is the handle's one table, whichever call builds it
    table = dev.nee_light_table()
    fresh = rb.DeviceScene(host, device=0)
    nee_first, _ = fresh.render_nee_to_host(cam)
    for g, w in zip(table, fresh.nee_light_table()):
        assert_same(g, w, "the emitter table built by rt_render_lit")
    assert len(table[0]) > 0
    assert_same(dev.render_nee_to_host(cam)[0], nee_first, "rt_render_nee after rt_render_lit")
    assert_same(fresh.render_lit_to_host(cam, **kw)[0], lit, "rt_render_lit after rt_render_nee")
    # sync = 0 on a side stream, then a copy; one environment serves two scenes
    host2, _ = three_ball_scene(lamp=True)
    cam2 = rb.make_camera(128, 72, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), 8, 6)
    dev2 = rb.DeviceScene(host2, device=0)
    lit2, _ = dev2.render_lit_to_host(cam2, env=env)
    assert_same(lit2, lr.frame(host2, cam2, rgb=m), "scene 2 against the restatement")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fb1 = torch.full((72, 128, 3), float("nan"), device="cuda:0")
    fb2 = torch.full((72, 128, 3), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        dev.render_lit(cam, fb1.data_ptr(), stream=s1.cuda_stream, sync=False, **kw)
    with torch.cuda.stream(s2):
        dev2.render_lit(cam2, fb2.data_ptr(), stream=s2.cuda_stream, sync=False, env=env)
    s1.synchronize()
    s2.synchronize()
    assert_same(fb1.cpu().numpy(), lit, "scene 1 on its stream")
    assert_same(fb2.cpu().numpy(), lit2, "scene 2 on its stream")
    dev.close()
    fresh.close()
    dev2.close()
    env.close()


# the restatement's ratios at this size (48 x 32, 16 spp against 8192, the seeds are fixed)
LIT_OVER_ENV_ONLY_MSE = 0.998288717
LIT_OVER_EMITTERS_ONLY_MSE = 0.406293145


@pytest.mark.gpu
def test_quality_at_equal_samples():
    """The lamp scene under the sun-and-sky map at equal samples: luminance MSE at 16 spp of both lights with MIS over the environment
    sampled alone (rt_render_env mode 1: the lamp is found by the path) and over the emitters sampled alone (rt_render_nee: the sky is
    a constant-background miss there, so this one renders another image — see DESIGN.md §16), against a lit frame at 8192 spp from a
    disjoint sample range.  Every frame is the restatement's bit for bit, so the ratios are the restatement's."""
    rb.amd_lib().rt_set_device(0)
    host, _ = three_ball_scene(lamp=True)
    cam = rb.make_camera(48, 32, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), 8192, 6)
    m = er.sun_and_sky(256)
    dev = rb.DeviceScene(host, device=0)
    first = 1 << 24
    with rb.Env(m) as env:
        truth_fb, _ = dev.render_lit_to_host(cam, env=env)
        assert_same(truth_fb, lr.frame(host, cam, rgb=m), "the 8192 spp frame")
        truth = truth_fb.astype(np.float64) / cam.samples_per_pixel @ LUM
        c = scaled(cam, 48, 32, 16, 6)
        frames = {"lit": (dev.render_lit_to_host(c, env=env, sample_first=first)[0], lr.frame(host, c, rgb=m, sample_first=first)),
                  "env": (dev.render_env_to_host(c, env, sample_first=first)[0], er.frame(host, c, m, sample_first=first)),
                  "nee": (dev.render_nee_to_host(c, sample_first=first)[0], nr.frame(host, c, sample_first=first))}
    mse = {}
    for k, (got, want) in frames.items():
        assert_same(got, want, f"{k} at 16 spp")
        mse[k] = float(((got.astype(np.float64) / 16 @ LUM - truth) ** 2).mean())
    over_env, over_nee = mse["lit"] / mse["env"], mse["lit"] / mse["nee"]
    print(f"luminance MSE at 16 spp: {mse}; lit / env-only {over_env:.6g}, lit / emitters-only {over_nee:.6g}")
    assert abs(over_env / LIT_OVER_ENV_ONLY_MSE - 1) < 1e-4, over_env
    assert abs(over_nee / LIT_OVER_EMITTERS_ONLY_MSE - 1) < 1e-4, over_nee
    dev.close()


@pytest.mark.gpu
def test_cli_lit_frames_are_the_python_paths(test_config_text, tmp_path):
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    v, u = np.meshgrid((np.arange(32) + 0.5) / 32, (np.arange(64) + 0.5) / 64, indexing="ij")
    img = np.stack([0.4 + 0.3 * u, 0.5 + 0.4 * (1 - v), 0.9 - 0.5 * v], -1).astype(np.float32)
    img[6:9, 20:24] += 400.0
    write_pfm(str(tmp_path / "sky.pfm"), img)
    out = subprocess.run([EXE, "--gpu", "--lit", "--nee", "mis", "--env", str(tmp_path / "sky.pfm") + ":64", "--env-up", "z", "--lens", "0.2:12",
                          "--motion-blur", "0.5", "--aov", "--denoise"], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    with rb.Env.from_equirect(rb.load_hdr_image(str(tmp_path / "sky.pfm")), 64) as env:
        for f in range(info.num_frames):
            cam, close = host.frame_camera_at(float(f)), host.frame_camera_at(f + 0.5)
            fb, _ = dev.render_lit_to_host(cam, cam_close=close, lens=dict(lens_radius=0.2, focus_distance=12.0), nee=dict(mis=1), env=env,
                                           env_params=dict(rot=er.Z_UP))
            want = rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp)
            assert open(tmp_path / f"f_{f}.png", "rb").read() == want, f
            assert os.path.getsize(tmp_path / f"f_{f}.png.aov") > 12 and os.path.getsize(tmp_path / f"f_{f}.png.denoised") > 8
    dev.close()
