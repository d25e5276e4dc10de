"""rt_render_medium / rt_trace_samples_medium (include/rtp_amd.h, "participating medium"): a homogeneous medium on the lit
path.  The contract's restatement is tests/cpu_native/medium_ref.c (tests/medium_reference.py); the CPU tests check the restatement and
the ABI, the GPU tests the kernels against the restatement, bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gloss_reference as glr
import lit_fuzz as lf
import lit_reference as lr
import medium_reference as mr
import rtp_bindings as rb
from test_lit import LENS, assert_same, night_camera, night_rtiow, three_ball_scene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
INVALID = 1
FAR_BALL = dict(sigma_t=0.7, albedo=(0.9, 0.8, 0.7), g=0.7, ball=(0.0, 0.0, 1.0e4, 1.0))      # 10^4 units behind every camera used here


def sun_map():
    """16 x 16, dim, with a small sun."""
    m = np.full((16, 16, 3), 0.05, np.float32)
    m[5, 9] = (60, 50, 40)
    return m


ENV_MIS, ENV_LIGHT = dict(mode=1, scale=0.8), dict(mode=2, scale=0.8)
# the settings of a call: name → (the restatement's keywords, the device call's keywords; "env" marks the calls that need an rb.Env)
SETTINGS = {
    "mis": (dict(nee_mis=1), dict(nee=dict(mis=1))),
    "light-only": (dict(nee_mis=0), dict(nee=dict(mis=0))),
    "sample_planes": (dict(planes=1), dict(nee=dict(sample_planes=1))),
    "select": (dict(select=1, planes=1), dict(nee=dict(select=1, sample_planes=1))),
    "glossy": (dict(glossy=1, glossy_env=1, rgb=sun_map(), env_params=ENV_MIS),
               dict(nee=dict(glossy=1), env="sun", env_params=dict(glossy=1, **ENV_MIS))),
    "glossy emitters": (dict(glossy=1), dict(nee=dict(glossy=1))),
    "env sun mis": (dict(rgb=sun_map(), env_params=ENV_MIS), dict(env="sun", env_params=ENV_MIS)),
    "env sun light": (dict(rgb=sun_map(), env_params=ENV_LIGHT, emitters=False), dict(env="sun", env_params=ENV_LIGHT, emitters=False)),
    "lens + motion": (dict(lens=LENS, cam_close="close"), dict(lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), cam_close="close")),
}


@functools.lru_cache(maxsize=None)
def scenes():
    """name → (host, camera(w, h, spp, depth), the closing camera's eye): the three scenes of the issue."""
    three, cam3 = three_ball_scene(lamp=True)
    fz = lf.case(1)
    assert fz.has_planes(1)
    return {
        "three balls": (three, lambda w, h, spp, d: rb.make_camera(w, h, 40.0, (0, 2, 7), (0, 1, 0), (0.1, 0.2, 0.3), spp, d),
                        lambda w, h, spp, d: rb.make_camera(w, h, 40.0, (0.3, 2.1, 7), (0, 1, 0), (0.1, 0.2, 0.3), spp, d)),
        "night rtiow": (night_rtiow(), lambda w, h, spp, d: night_camera(w, h, spp, d, (0.02, 0.03, 0.05)),
                        lambda w, h, spp, d: night_camera(w, h, spp, d, (0.02, 0.03, 0.05), eye=(13.2, 3.1, 2))),
        "fuzz planes": (fz.host, lambda w, h, spp, d: fz.camera(w, h, spp, d),
                        lambda w, h, spp, d: rb.make_camera(w, h, fz.vfov, fz.eye_close, (0, 0, 0), fz.background, spp, d)),
    }


def ref_kw(scene, setting, w, h, spp, depth):
    kw = dict(SETTINGS[setting][0])
    if kw.get("cam_close") == "close":
        kw["cam_close"] = scenes()[scene][2](w, h, spp, depth)
    return kw


def dev_kw(scene, setting, env, w, h, spp, depth):
    kw = dict(SETTINGS[setting][1])
    if kw.get("cam_close") == "close":
        kw["cam_close"] = scenes()[scene][2](w, h, spp, depth)
    if kw.get("env") == "sun":
        kw["env"] = env
    return kw


# the media of the probe cases: regions 0 / 1 / 2 and g in {0, 0.7, -0.5}
def media(scene):
    box = dict(box=(-4.0, -0.5, -4.0, 4.0, 3.5, 4.0))
    ball = dict(ball=(0.0, 1.0, 0.0, 3.0))
    return {"all space g=0": dict(sigma_t=0.08, albedo=(0.9, 0.85, 0.8), g=0.0),
            "ball g=0.7": dict(sigma_t=0.35, albedo=(0.95, 0.9, 0.8), g=0.7, **ball),
            "box g=-0.5": dict(sigma_t=0.25, albedo=0.9, g=-0.5, **box)}


def all_ijs(w, h, spp):
    i, j, s = np.meshgrid(np.arange(w), np.arange(h), np.arange(spp), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), s.ravel()], 1).astype(np.int32)


# ---- no GPU needed ---------------------------------------------------------------------------------------------------------------------

def test_abi_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_medium_params_init", "rt_render_medium", "rt_trace_samples_medium"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.MediumParams) == 4 * 13
    assert len(lib.rt_render_medium.argtypes) == 10 and len(lib.rt_trace_samples_medium.argtypes) == 13
    p = rb.MediumParams()
    p.region, p.sigma_t, p.g = 2, 3.0, 0.5
    p.a[1] = p.b[2] = 4.0
    lib.rt_medium_params_init(C.byref(p))
    assert (p.struct_bytes, p.region, p.sigma_t, p.g) == (C.sizeof(rb.MediumParams), 0, 0.0, 0.0)
    assert list(p.albedo) == [1.0, 1.0, 1.0] and list(p.a) == [0.0] * 3 and list(p.b) == [0.0] * 3
    lib.rt_medium_params_init(None)
    q = rb.medium_params(sigma_t=0.5, albedo=(0.1, 0.2, 0.3), g=-0.4, box=(0, 1, 2, 3, 4, 5))
    assert q.region == 2 and list(q.a) == [0.0, 1.0, 2.0] and list(q.b) == [3.0, 4.0, 5.0] and abs(q.albedo[1] - 0.2) < 1e-7
    q = rb.medium_params(sigma_t=0.5, ball=(1, 2, 3, 4))
    assert q.region == 1 and list(q.a) == [1.0, 2.0, 3.0] and q.b[0] == 4.0
    assert lib.rt_version_string().startswith(b"rtp_amd 0.5 ")
    for name in ("render_medium", "render_medium_to_host", "trace_samples_medium"):
        assert hasattr(rb.DeviceScene, name)


def _calls(cam, lit, medium):
    """(status, message) of rt_render_medium and of rt_trace_samples_medium with a null scene."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    pl = C.byref(lit) if lit is not None else None
    pm = C.byref(medium) if medium is not None else None
    out = [lib.rt_render_medium(None, C.byref(cam), pl, pm, None, 0, C.c_void_p(1 << 32), None, 1, None), lib.rt_get_last_error_string().decode()]
    out += [lib.rt_trace_samples_medium(None, C.byref(cam), pl, pm, 1, ijs, f, r, r, s, s, s, s), lib.rt_get_last_error_string().decode()]
    return out


def test_refusals_before_the_scene_is_looked_at():
    """rt_render_lit's parameter refusals first, then every refusal of rt_medium_params, all with a null scene: nothing can have been
    enqueued.  Parameters that pass reach the null-scene check; medium == NULL is the defaults."""
    cam = rb.rtiow_camera(8, 4, 2)
    nan, inf = float("nan"), float("inf")

    def refused(word, medium, lit=None):
        st1, m1, st2, m2 = _calls(cam, lit, medium)
        assert st1 == INVALID and word in m1 and "rt_render_medium" in m1, (word, m1)
        assert st2 == INVALID and word in m2 and "rt_trace_samples_medium" in m2, (word, m2)

    short = rb.medium_params(sigma_t=1.0)
    short.struct_bytes = 4
    refused("struct_bytes", short)
    for region in (-1, 3):
        m = rb.medium_params(sigma_t=1.0)
        m.region = region
        refused("region", m)
    for s in (-0.5, nan, inf, -inf):
        refused("sigma_t", rb.medium_params(sigma_t=s))
    for alb in ((-0.1, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, nan)):
        refused("albedo", rb.medium_params(sigma_t=1.0, albedo=alb))
    for g in (0.96, -0.96, nan, inf):
        refused("|g|", rb.medium_params(sigma_t=1.0, g=g))
    for r in (0.0, -1.0):
        refused("radius", rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, r)))
    refused("finite", rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, nan)))
    for box in ((0, 0, 0, 0, 1, 1), (0, 0, 0, 1, -1, 1), (0, 0, 2, 1, 1, 2)):
        refused("lo < hi", rb.medium_params(sigma_t=1.0, box=box))
    refused("finite", rb.medium_params(sigma_t=1.0, ball=(inf, 0, 0, 1)))
    refused("finite", rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, inf, 1)))
    # rt_render_lit's come first
    refused("mis", rb.medium_params(sigma_t=-1.0), lit=rb.lit_params(nee=dict(mis=2)))
    refused("lens_radius", rb.medium_params(sigma_t=-1.0), lit=rb.lit_params(lens=dict(lens_radius=-1.0)))
    # what passes reaches the scene
    old = rb.medium_params(sigma_t=1.0, g=5.0)
    old.struct_bytes = 8           # an older caller's struct: region is read, everything behind it keeps its default
    for m in (None, rb.medium_params(), rb.medium_params(sigma_t=2.0, albedo=0.0, g=-0.95, ball=(0, 0, 0, 1e-3)),
              rb.medium_params(sigma_t=0.0, box=(0, 0, 0, 1, 1, 1)), old):
        st1, m1, st2, m2 = _calls(cam, None, m)
        assert st1 == INVALID and "null scene" in m1, m1
        assert st2 == INVALID and "sigma_t" not in m2, m2


def test_cli_refusals(test_config_text, tmp_path):
    cases = [(["--fog", "0.5"], "needs --lit"), (["--lit", "--fog", "0.5", "--noise-target", "0.1"], "--noise-target"),
             (["--lit", "--fog"], "SIGMA"), (["--lit", "--fog", "-1"], "SIGMA"), (["--lit", "--fog", "0.5:2"], "SIGMA"),
             (["--lit", "--fog", "0.5:0.9:0.99"], "SIGMA"), (["--lit", "--fog", "0.5:0.9x"], "SIGMA"), (["--lit", "--fog", "0.5:0.9:0.1:3"], "SIGMA"),
             (["--lit", "--fog", "nan"], "SIGMA"), (["--lit", "--fog-ball", "0,0,0,1"], "need --fog"),
             (["--lit", "--fog", "0.5", "--fog-ball", "0,0,0"], "cx,cy,cz,r"), (["--lit", "--fog", "0.5", "--fog-ball", "0,0,0,-1"], "cx,cy,cz,r"),
             (["--lit", "--fog", "0.5", "--fog-box", "0,0,0,1,1"], "x0,y0,z0"), (["--lit", "--fog", "0.5", "--fog-box", "0,0,0,1,0,1"], "x0,y0,z0"),
             (["--lit", "--fog", "0.5", "--fog-ball", "0,0,0,1", "--fog-box", "0,0,0,1,1,1"], "exclude")]
    for extra, word in cases:
        res = subprocess.run([EXE, "--gpu"] + extra, input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert res.returncode == 99 and word in res.stderr, (extra, res.returncode, res.stderr[-300:])


IDENTITY_VIEW = (12, 8, 2)


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_restatement_identities(scene):
    """No medium (None, sigma_t = 0) and a region no ray touches give rt_render_lit's restatement — gloss_reference's, which is
    lit_reference's with sample_planes, select and glossy; lit_reference itself where it can express the setting — in every column."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    ijs = all_ijs(w, h, spp)
    for setting in SETTINGS:
        for depth in (12,):
            cam = camera(w, h, spp, depth)
            kw = ref_kw(scene, setting, w, h, spp, depth)
            want = glr.trace(host, cam, ijs, **{**dict(glossy=0, glossy_env=0), **kw})
            if setting in ("mis", "light-only", "env sun mis", "env sun light", "lens + motion"):
                plain = lr.trace(host, cam, ijs, **kw)
                for a, b in zip(plain, want[:5]):
                    assert_same(a, b, f"{scene} / {setting}: gloss_reference against lit_reference")
            for name, medium in (("none", None), ("sigma_t = 0", dict(sigma_t=0.0, ball=(0, 1, 0, 3))), ("far ball", FAR_BALL)):
                rad, rays, events, ends, seeds = mr.trace(host, cam, ijs, medium=medium, **kw)
                what = f"{scene} / {setting} / {name}"
                assert_same(rad, want[0], what + ": radiance")
                assert_same(rays, want[1], what + ": rays")
                for k in range(3):
                    assert_same(seeds[:, k], want[2 + k], what + f": seed {k}")
                assert not events.any()
                base = [rb_wang(rb_wang(rb_wang(int(i) * w + int(j)) + int(s)) ^ 0x4D454431) for i, j, s in ijs]
                assert_same(seeds[:, 3], np.array(base, np.uint32), what + ": the med stream as initialised")


def rb_wang(s):
    s &= 0xFFFFFFFF
    s = ((s ^ 61) ^ (s >> 16)) & 0xFFFFFFFF
    s = (s * 9) & 0xFFFFFFFF
    s ^= s >> 4
    s = (s * 0x27D4EB2D) & 0xFFFFFFFF
    s ^= s >> 15
    return s


def _fog_ball_scene():
    """One far-away tiny sphere (a scene needs a primitive) and a camera looking down -z at a fog ball of radius 1 at the origin."""
    from test_lit import MAT_LAMBERTIAN, material
    host = rb.HostScene.from_arrays(np.array([[0, 1000, 0, 0.5, 0]], np.float32), np.zeros((0, 11), np.float32), [material(MAT_LAMBERTIAN)])
    return host


ABSORB_N = 4096           # samples per pixel of the absorption test, chosen on the restatement (the RNG is deterministic)
BACKGROUND = (0.8, 0.6, 0.4)


@pytest.mark.parametrize("tau", [0.1, 1.0, 3.0])
def test_pure_absorption_is_beer_lambert(tau):
    """albedo = 0, a fog ball of radius 1 in front of a constant background, no emitters, pinhole: every sample is 0 or the background, and
    the mean over ABSORB_N samples lies within |z| <= 4.5 of background * exp(-sigma_t * chord), the chord in float64 from the pixel-centre
    ray.  Pixels: those whose chord varies by < 1 % over the pixel's corners.  tau = sigma_t * diameter."""
    host = _fog_ball_scene()
    w = h = 9
    cam = rb.make_camera(w, h, 20.0, (0, 1, 8), (0, 0, 0), BACKGROUND, ABSORB_N, 8)
    sigma = tau / 2.0
    medium = dict(sigma_t=sigma, albedo=0.0, ball=(0, 0, 0, 1.0))
    o = np.array([cam.origin.e[k] for k in range(3)], np.float64)
    p00 = np.array([cam.pixel00_loc.e[k] for k in range(3)], np.float64)
    du = np.array([cam.pixel_delta_u.e[k] for k in range(3)], np.float64)
    dv = np.array([cam.pixel_delta_v.e[k] for k in range(3)], np.float64)

    def chord(i, j):
        d = p00 + i * du + j * dv - o
        d /= np.linalg.norm(d)
        b = np.dot(o, d)
        disc = b * b - (np.dot(o, o) - 1.0)
        return 2.0 * np.sqrt(disc) if disc > 0 else 0.0
    checked = 0
    fb, mom = mr.frame(host, cam, medium=medium, emitters=False, moments=True)
    bg = np.array(BACKGROUND, np.float32)
    for j in range(h):
        for i in range(w):
            c = chord(i, j)
            corners = [chord(i + a, j + b) for a in (-0.5, 0.5) for b in (-0.5, 0.5)]
            if c == 0.0 or min(corners) <= 0.0 or (max(corners) - min(corners)) > 0.01 * c:
                continue
            checked += 1
            p = np.exp(-sigma * c)
            mean = mom[j, i, 0] / ABSORB_N / BACKGROUND[0]          # the share of samples that came through
            z = (mean - p) / np.sqrt(p * (1 - p) / ABSORB_N)
            print(f"tau {tau} pixel ({i}, {j}) chord {c:.4f} share {mean:.5f} want {p:.5f} z {z:+.2f}")
            assert abs(z) <= 4.5, (i, j, z)
    assert checked >= 1
    # every sample is 0 or the background, exactly
    ijs = all_ijs(w, h, 16)
    rad, rays, events, ends, seeds = mr.trace(host, cam, ijs, medium=medium, emitters=False)
    zero = (rad == 0).all(1)
    full = (rad == bg[None, :]).all(1)
    assert (zero | full).all() and zero.any() and full.any()
    assert ((events == 1) == zero).all() and (ends[zero] == mr.END_BLACK).all()


@pytest.mark.parametrize("g", [0.0, 0.7])
def test_white_furnace(g):
    """albedo = 1 in a fog ball of optical diameter 2 under background 1, max_depth = 200: every path that ends by a miss returns exactly
    1.0f in every channel, and at most 0.1 % of the samples are cut by depth (a condition on the scene: it holds with room to spare)."""
    host = _fog_ball_scene()
    cam = rb.make_camera(16, 16, 20.0, (0, 1, 8), (0, 0, 0), (1.0, 1.0, 1.0), 8, 200)
    ijs = all_ijs(16, 16, 8)
    rad, rays, events, ends, seeds = mr.trace(host, cam, ijs, medium=dict(sigma_t=1.0, albedo=1.0, g=g, ball=(0, 0, 0, 1.0)), emitters=False)
    missed = ends == mr.END_MISS
    assert (rad[missed] == np.float32(1.0)).all()
    assert (~missed).mean() <= 0.001, (~missed).mean()
    assert events.max() >= 3 and (events > 0).mean() > 0.1


@pytest.mark.parametrize("g", [0.0, 0.3, -0.3, 0.95, -0.95])
def test_phase_function_integrates_to_one(g):
    """2 pi * integral of ph(c) dc over [-1, 1], by float64 Gauss-Legendre quadrature of the float32 restatement: 1 within 1e-5 (float32
    rounding of ph is 6e-8 relative; g = +-0.95 peaks at 62, resolved by 4000 nodes)."""
    x, wq = np.polynomial.legendre.leggauss(4000)
    total = 2.0 * np.pi * np.sum(wq * mr.ph(g, x.astype(np.float32)).astype(np.float64))
    # the nodes are rounded to float32 before ph sees them: ph'/ph <= 2g/(1-g)^2 * 6e-8 adds < 1e-4 at |g| = 0.95
    assert abs(total - 1.0) < (2e-4 if abs(g) > 0.9 else 1e-5), total


COS_N = 1 << 18


@pytest.mark.parametrize("g", [0.0, 0.7, -0.5])
def test_sampled_cosine_has_mean_g(g):
    """The mean of COS_N draws of cos_t is g (Henyey-Greenstein's mean cosine) within 4.5 standard errors, the standard error from the
    draws' own variance."""
    c = mr.cos_draws(g, COS_N, 12345).astype(np.float64)
    assert (np.abs(c) <= 1.0).all()
    z = (c.mean() - g) / (c.std(ddof=1) / np.sqrt(COS_N))
    print(f"g {g}: mean {c.mean():+.6f} z {z:+.2f}")
    assert abs(z) <= 4.5


EQUAL_SPP = 4096          # chosen on the restatement
FOG_BOX = dict(sigma_t=0.125, albedo=(0.9, 0.9, 0.9), g=0.3, box=(-4.0, -0.5, -4.0, 4.0, 3.5, 4.0))     # optical depth 1 across its 8 units


def _channel_z(a, b, spp):
    """z per pixel and channel of the difference of two frames' means, from their double moments (per channel: sum, sum of squares): the
    sample variance of each channel of each frame, exactly."""
    ma, mb = a[..., :3] / spp, b[..., :3] / spp
    va = np.maximum(a[..., 3:] / spp - ma * ma, 0) * (spp / (spp - 1.0)) / spp
    vb = np.maximum(b[..., 3:] / spp - mb * mb, 0) * (spp / (spp - 1.0)) / spp
    return (ma - mb) / np.sqrt(va + vb + 1e-300)


def test_equal_expectation_under_fog():
    """The fogged lamp scene (a fog box of optical depth 1 around the three balls): mis against light-only, light samples off (the
    rt_render_lit mode that expresses it: sample_emitters = 0), and select = 1 against select = 0 agree per pixel and per channel:
    |z| <= 4.5 with each channel's own sample variance.  EQUAL_SPP was chosen here on the restatement (the RNG is deterministic)."""
    host, _, _ = scenes()["three balls"]
    cam = rb.make_camera(4, 4, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), EQUAL_SPP, 6)
    frames = {}
    for name, kw in (("mis", dict(nee_mis=1)), ("light", dict(nee_mis=0)), ("off", dict(emitters=False)), ("select", dict(nee_mis=1, select=1))):
        frames[name] = mr.frame(host, cam, medium=FOG_BOX, moments=True, **kw)[1]
    for a, b in (("mis", "light"), ("mis", "off"), ("mis", "select")):
        z = _channel_z(frames[a], frames[b], EQUAL_SPP)
        print(a, b, "max |z|", float(np.abs(z).max()), np.round(z, 2).tolist())
        assert np.abs(z).max() <= 4.5, (a, b, z)
    assert frames["mis"][..., :3].sum() > 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------

PROBE_VIEW = (16, 9, 3)


@functools.lru_cache(maxsize=None)
def probe_reference(scene, setting, medium_name, depth):
    host, camera, _ = scenes()[scene]
    w, h, spp = PROBE_VIEW
    return mr.trace(host, camera(w, h, spp, depth), all_ijs(w, h, spp), medium=media(scene)[medium_name], **ref_kw(scene, setting, w, h, spp, depth))


def _probe_cases():
    """Every setting and every medium at least once on every scene, the depths spread over them."""
    out = []
    names = list(SETTINGS)
    for si, scene in enumerate(("three balls", "night rtiow", "fuzz planes")):
        for k, setting in enumerate(names):
            medium_name = list(media(scene))[(k + si) % 3]
            out.append((scene, setting, medium_name, (12, 2, 1)[(k + si) % 3] if k % 2 else 12))
    return out


def _compare_probe(got, want, what):
    rad, rays, events, seeds, ns, es, ms = got
    wrad, wrays, wevents, wends, wseeds = want
    assert_same(rad, wrad, what + ": radiance")
    assert_same(rays, wrays, what + ": rays")
    assert_same(events, wevents, what + ": medium events")
    for k, col in enumerate((seeds, ns, es, ms)):
        assert_same(col, wseeds[:, k], what + f": final seed {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow", "fuzz planes"])
def test_probe_samples_equal_the_restatement(scene):
    host, camera, _ = scenes()[scene]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    seen_events = 0
    with rb.Env(sun_map()) as env:
        for sc, setting, medium_name, depth in _probe_cases():
            if sc != scene:
                continue
            want = probe_reference(scene, setting, medium_name, depth)
            got = dev.trace_samples_medium(camera(w, h, spp, depth), ijs, medium=media(scene)[medium_name], **dev_kw(scene, setting, env, w, h, spp, depth))
            _compare_probe(got, want, f"{scene} / {setting} / {medium_name} / depth {depth}")
            seen_events += int(want[2].sum())
    assert seen_events > 100
    dev.close()


@pytest.mark.gpu
def test_frames_equal_the_restatement():
    """40 x 27 x 3 spp (3 240 work items: no multiple of 64 or of the chunk), 7 x 5 x 1 (less than a wave), a 3-row shard of the first,
    sample_first = 5, sync = 0 on a torch stream, and one small fogged frame through each of the other instantiations."""
    import torch
    scene, setting = "three balls", "glossy"
    host, camera, _ = scenes()[scene]
    medium = media(scene)["ball g=0.7"]
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env:
        for (w, h, spp), more in (((40, 27, 3), {}), ((7, 5, 1), {}), ((40, 27, 3), dict(shard=rb.Shard(3, 1, 4))), ((40, 27, 3), dict(sample_first=5))):
            cam = camera(w, h, spp, 12)
            want = mr.frame(host, cam, medium=medium, **more, **ref_kw(scene, setting, w, h, spp, 12))
            got, _ = dev.render_medium_to_host(cam, medium=medium, **more, **dev_kw(scene, setting, env, w, h, spp, 12))
            assert_same(got, want, f"frame {w}x{h}x{spp} {more}")
        # lens + motion with the light tree over the two-kind table, on a stream, without waiting inside the call
        scene2 = "fuzz planes"
        host2, camera2, _ = scenes()[scene2]
        dev2 = rb.DeviceScene(host2, device=0)
        w, h, spp = 40, 27, 3
        cam = camera2(w, h, spp, 12)
        medium2 = media(scene2)["box g=-0.5"]
        kw_r = {**ref_kw(scene2, "lens + motion", w, h, spp, 12), "select": 1, "planes": 1}
        kw_d = dev_kw(scene2, "lens + motion", env, w, h, spp, 12)
        kw_d["nee"] = dict(select=1, sample_planes=1)
        want = mr.frame(host2, cam, medium=medium2, **kw_r)
        stream = torch.cuda.Stream()
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        with torch.cuda.stream(stream):
            dev2.render_medium(cam, fb.data_ptr(), medium=medium2, stream=stream.cuda_stream, sync=False, **kw_d)
        stream.synchronize()
        assert_same(fb.cpu().numpy(), want, "sync = 0 on a torch stream")
        # the other six instantiations of medium_render_kernel under real fog — pinhole and lens over the sphere-only table, the two-kind
        # table and the trees — each on a small frame, the three regions (all space included) in turn
        w, h, spp = 24, 13, 2
        names = list(media(scene2))
        k = 0
        for lens in (False, True):
            for select, planes in ((0, 0), (0, 1), (1, 0), (1, 1)):
                if (lens, select, planes) == (True, 1, 1):
                    continue            # (above)
                setting = "lens + motion" if lens else "mis"
                cam = camera2(w, h, spp, 12)
                medium3 = media(scene2)[names[k % 3]]
                kw_r = {**ref_kw(scene2, setting, w, h, spp, 12), "select": select, "planes": planes}
                kw_d = dev_kw(scene2, setting, env, w, h, spp, 12)
                kw_d["nee"] = dict(select=select, sample_planes=planes)
                want = mr.frame(host2, cam, medium=medium3, **kw_r)
                got, _ = dev2.render_medium_to_host(cam, medium=medium3, **kw_d)
                assert_same(got, want, f"frame lens={lens} select={select} planes={planes} {names[k % 3]}")
                k += 1
        dev2.close()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_device_identities(scene):
    """medium None / sigma_t = 0 is rt_render_lit; a ball no ray touches is rt_render_lit THROUGH THE MEDIUM KERNELS: the same radiance,
    rays and three streams as rt_trace_samples_lit, no event, the med stream untouched, and the same frame."""
    host, camera, _ = scenes()[scene]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env:
        for setting in SETTINGS:
            # (the far ball subtends 3e-8 sr: no path ray and no shadow ray of these frames — the environment's included — crosses it, as
            # test_restatement_identities shows on the restatement for the same settings)
            kw = dev_kw(scene, setting, env, w, h, spp, 12)
            cam = camera(w, h, spp, 12)
            lit = dev.trace_samples_lit(cam, ijs, **kw)
            for name, medium in (("none", None), ("sigma_t = 0", dict(sigma_t=0.0)), ("far ball", FAR_BALL)):
                rad, rays, events, seeds, ns, es, ms = dev.trace_samples_medium(cam, ijs, medium=medium, **kw)
                what = f"{scene} / {setting} / {name}"
                for a, b, col in zip((rad, rays, seeds, ns, es), lit, ("radiance", "rays", "seed", "nee seed", "env seed")):
                    assert_same(a, b, f"{what}: {col}")
                assert not events.any()
                init = np.array([rb_wang(rb_wang(rb_wang(int(i) * w + int(j)) + int(s)) ^ 0x4D454431) for i, j, s in ijs], np.uint32)
                assert_same(ms, init, what + ": the med stream as initialised")
            want, _ = dev.render_lit_to_host(cam, **kw)
            for medium in (None, FAR_BALL):
                got, t = dev.render_medium_to_host(cam, medium=medium, **kw)
                assert_same(got, want, f"{scene} / {setting}: frame, medium {medium is not None}")
    dev.close()


@pytest.mark.gpu
def test_handle_state_is_left_alone():
    """rt_render and rt_render_lit of a handle after a medium call equal a fresh handle's."""
    host, camera, _ = scenes()["three balls"]
    cam = camera(24, 16, 2, 12)
    fresh = rb.DeviceScene(host, device=0)
    want_render, _ = fresh.render_to_host(cam)
    want_lit, _ = fresh.render_lit_to_host(cam)
    fresh.close()
    dev = rb.DeviceScene(host, device=0)
    dev.render_medium_to_host(cam, medium=media("three balls")["box g=-0.5"])
    got_render, _ = dev.render_to_host(cam)
    got_lit, _ = dev.render_lit_to_host(cam)
    assert_same(got_render, want_render, "rt_render after rt_render_medium")
    assert_same(got_lit, want_lit, "rt_render_lit after rt_render_medium")
    dev.close()


@pytest.mark.gpu
def test_device_log_libm_is_the_stated_algorithm_for_every_float():
    """tests/dev_log_checks.py in a child process that loads the developer library: log_libm compiled for gfx950 against
    tests/cpu_native/log_sweep_ref.cpp's restatement on all 2^32 floats, 0 differences."""
    from conftest import run_child
    dev_lib = os.path.join(ROOT, "ray-tracing-practice_amd", "librtp_amd_dev.so")
    assert os.path.exists(dev_lib), "run __graft_entry__.build() (make -C ray-tracing-practice_amd dev)"
    env = dict(os.environ, RTP_AMD_LIB=dev_lib)
    res = run_child([sys.executable, "-m", "pytest", os.path.join(HERE, "dev_log_checks.py"), "-x", "-q", "-s", "-p", "no:cacheprovider"], 200, env=env)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "2 passed" in res.stdout and "failed" not in res.stdout and "skipped" not in res.stdout


def test_log_reference_against_the_host_libm():
    """rt_device_math.h's log_libm compiled for the host equals the restatement (log_ref.h) on all 2^32 floats; the restatement against this host's logf: every float of (0, 1] (what the kernel needs) — a count, printed; the
    contract is the algorithm.  On glibc 2.35 it is 0.  The specials are the header's."""
    so = os.path.join(__import__("tempfile").mkdtemp(prefix="lsr_"), "liblsr.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so, os.path.join(HERE, "cpu_native", "log_sweep_ref.cpp")],
                   check=True)
    l = C.CDLL(so)
    l.lsr_vs_libm.restype = C.c_uint64
    l.lsr_vs_libm.argtypes = [C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    l.lsr_log_bits.restype = C.c_uint32
    l.lsr_log_bits.argtypes = [C.c_uint32]
    l.lsr_sanity.restype = C.c_uint64
    l.lsr_sanity.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_double, C.POINTER(C.c_uint64)]
    worst = (C.c_uint32 * 8)()
    differ = l.lsr_vs_libm(1, 0x3F800000, min(16, len(os.sched_getaffinity(0))), worst)
    print(f"log_ref against logf on (0, 1]: {differ} of {0x3F800000} inputs differ")
    # rt_device_math.h's log_libm itself, compiled for this host, is the restatement on every float
    l.lsr_vs_host_build.restype = C.c_uint64
    l.lsr_vs_host_build.argtypes = [C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    bad = l.lsr_vs_host_build(0, 1 << 32, min(16, len(os.sched_getaffinity(0))), worst)
    assert bad == 0, (bad, [hex(x) for x in worst])
    for bits, want in ((0x3F800000, 0x00000000), (0x00000000, 0xFF800000), (0x80000000, 0xFF800000), (0x7F800000, 0x7F800000), (0xBF800000, 0x7FC00000),
                       (0xFF800000, 0x7FC00000), (0x7F800001, 0x7FC00001), (0xFFC12345, 0xFFC12345)):
        assert l.lsr_log_bits(bits) == want, (hex(bits), hex(l.lsr_log_bits(bits)))
    sampled = C.c_uint64()
    assert l.lsr_sanity(0, 0x7F800000, 977, 1.0, C.byref(sampled)) == 0 and sampled.value > 2_000_000
