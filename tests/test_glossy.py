"""The glossy switch: light samples at METAL's reflect branch in rt_render_nee, rt_render_env, rt_render_lit and rt_render_lit_adaptive
(rt_nee_params.glossy, rt_env_params.glossy; include/rtp_amd.h "glossy = 1").

The header fixes pg — the density of unit(r + fuzz * in_sphere) — in float32 order, the glossy event, its light sample and the weight the
ray that leaves it carries; tests/cpu_native/gloss_ref.c restates that on the oracle (gloss_reference.py), and probed samples and frames
of the device must equal it bit for bit.  On the CPU: pg against the histogram of the restatement's own draws and its integral, the
restatement's identities against the older restatements, its expectation (against the oracle's ray_color, by z-scores) and what it gains
at equal samples."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import env_reference as er
import gloss_reference as gr
import nee_reference as nr
import rtp_bindings as rb
import tree_reference as tr
from test_nee_planes import (LUM, MAT_DIELECTRIC, MAT_LAMBERTIAN, MAT_LIGHT, MAT_METAL, QUAD, _zscores, assert_same, config_host, material,
                             night_camera)

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ray-tracing-practice_amd", "rtp_main")
OK, INVALID = 0, 1
LENS = (0.05, 7.0)
MIN_FUZZ = 2.0 ** -10


# ---- the scene: ten primitives, every kind of vertex the switch touches -----------------------------------------------------------------
def scene():
    """A METAL floor (fuzz 0.3) under a small emissive sphere and an emissive quad; METAL spheres of fuzz 0, 2^-11 (both mirrors for the
    switch), 0.05 and 1.5 (the vertex inside the lobe's ball), a LAMBERTIAN and a glass sphere."""
    mats = [material(MAT_METAL, (0.8, 0.8, 0.8), fuzz=0.3), material(MAT_METAL, (0.9, 0.6, 0.5), fuzz=0.0),
            material(MAT_METAL, (0.6, 0.9, 0.5), fuzz=2.0 ** -11), material(MAT_METAL, (0.5, 0.6, 0.9), fuzz=0.05),
            material(MAT_METAL, (0.9, 0.9, 0.6), fuzz=1.5), material(MAT_LAMBERTIAN, (0.7, 0.4, 0.3)), material(MAT_DIELECTRIC, ir=1.5),
            material(MAT_LIGHT, emit=(20, 18, 14)), material(MAT_LIGHT, emit=(3, 4, 6))]
    planes = np.array([[-6, 0, 6, 12, 0, 0, 0, 0, -12, 0, QUAD],
                       [-3.5, 2.5, -2.5, 1.5, 0, 0, 0, 1.0, 0.3, 8, QUAD]], np.float32)
    spheres = np.array([[-2.4, 0.5, 0.5, 0.5, 1], [-1.2, 0.5, -0.6, 0.5, 2], [0.0, 0.5, 0.8, 0.5, 3], [1.3, 0.5, -0.4, 0.5, 4],
                        [2.5, 0.5, 0.9, 0.5, 5], [-0.9, 0.4, 2.0, 0.4, 6], [0.6, 2.0, -0.8, 0.3, 7]], np.float32)
    return rb.HostScene.from_arrays(spheres, planes, mats)


def camera(w, h, spp, depth=50):
    """Low above the floor: its hits graze."""
    return rb.make_camera(w, h, 40.0, (0, 0.7, 7), (0, 0.6, 0), (0, 0, 0), spp, depth)


def hot_map():
    """16 x 16, dim, with one hot texel."""
    m = np.full((16, 16, 3), 0.05, np.float32)
    m[5, 9] = (60, 50, 40)
    return m


def mirror_night_rtiow():
    """test_nee.py's night rtiow (every eighth small sphere a light) with the fuzz of every METAL forced to 0: no glossy event anywhere."""
    base = rb.HostScene.rtiow()
    d = base.desc
    spheres, mats = [], []
    for i in range(d.num_spheres):
        s = d.spheres[i]
        m = rb.Material.from_buffer_copy(d.materials[s.material_idx])
        if 0 < i < d.num_spheres - 3 and i % 8 == 5:
            m = material(MAT_LIGHT, emit=(6.0, 4.5, 3.0) if i % 16 == 5 else (1.5, 2.0, 3.0))
        if m.type == MAT_METAL:
            m.fuzz = 0.0
        spheres.append([s.center.e[0], s.center.e[1], s.center.e[2], s.radius, len(mats)])
        mats.append(rb.Material.from_buffer_copy(m))
    night = rb.HostScene.from_arrays(np.array(spheres, np.float32), np.zeros((0, 11), np.float32), mats)
    base.close()
    return night


# The estimators the tests walk through: name → (the restatement's keywords, the device call and its keywords)
ENV_MIS, ENV_LIGHT = dict(mode=1, scale=0.8), dict(mode=2, scale=0.8)


def _nee_case(planes, select, mis):
    return (dict(glossy=1, planes=planes, select=select, nee_mis=mis), "nee", dict(params=dict(mis=mis, sample_planes=planes, select=select, glossy=1)))


def _env_case(ep):
    return (dict(glossy=0, glossy_env=1, emitters=False, rgb=hot_map(), env_params=ep), "env", dict(params=dict(glossy=1, **ep)))


def _lit_case(gn, ge):
    return (dict(glossy=gn, glossy_env=ge, planes=1, select=1, rgb=hot_map(), env_params=ENV_MIS, lens=LENS), "lit",
            dict(lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), nee=dict(sample_planes=1, select=1, glossy=gn),
                 env_params=dict(glossy=ge, **ENV_MIS)))


def probe_cases():
    cases = {}
    for planes in (0, 1):
        for select in (0, 1):
            for mis in (1, 0):
                cases[f"nee planes={planes} select={select} mis={mis}"] = _nee_case(planes, select, mis)
    cases["env mis"] = _env_case(ENV_MIS)
    cases["env light"] = _env_case(ENV_LIGHT)
    for gn, ge in ((1, 0), (0, 1), (1, 1)):
        cases[f"lit glossy={gn}{ge}"] = _lit_case(gn, ge)
    return cases


# which of gloss_reference.COUNTERS a case can move at all: a call without an environment weights no miss, one without emitters no hit
def possible_counters(name):
    if name.startswith("nee") or name == "lit glossy=10":
        return ("samples", "absorbed", "pg_zero", "fuzz_gt1", "hit_carried")
    if name.startswith("env") or name == "lit glossy=01":
        return ("samples", "absorbed", "pg_zero", "fuzz_gt1", "miss_carried")
    return gr.COUNTERS


@functools.lru_cache(maxsize=None)
def probe_set():
    """10^4 (i, j, s) of the 96 x 64 view."""
    rng = np.random.default_rng(23)
    n = 10000
    return np.stack([rng.integers(0, 96, n), rng.integers(0, 64, n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def probe_reference(name, depth):
    """The restatement's answer for one case (computed once, shared by the CPU and the GPU tests; nobody writes into it)."""
    rkw = probe_cases()[name][0]
    out = gr.trace(scene(), camera(96, 64, 1, depth), probe_set(), **rkw)
    for a in out:
        a.setflags(write=False)
    return out


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi():
    """The switch in both structs: rt_nee_params grew to 20 bytes (the 16-byte struct is still what nee_params() returns without the
    field), rt_env_params kept its size — glossy is the first of the former reserved words."""
    assert C.sizeof(rb.NeeParams) == 16 and C.sizeof(rb.NeeParamsGlossy) == 20
    p = rb.nee_params(glossy=1, select=1)
    assert isinstance(p, rb.NeeParamsGlossy) and (p.struct_bytes, p.mis, p.sample_planes, p.select, p.glossy) == (20, 1, 0, 1, 1)
    assert bytes(p)[16:20] == (1).to_bytes(4, "little")
    assert rb.nee_params(glossy=0).glossy == 0 and rb.nee_params().struct_bytes == 16
    e = rb.env_params(glossy=1)
    assert C.sizeof(rb.EnvParams) == 64 and (e.glossy, e.reserved[0], e.reserved[1], e.reserved[2]) == (1, 1, 0, 0)
    assert rb.env_params().glossy == 0 and rb.EnvParams.glossy.offset == 52
    with pytest.raises(rb.RtError):
        rb.env_params(reserved=1)


PG_DRAWS = 400000
PG_BINS = 40
PG_SIGMAS = 5.0


def _directions(c):
    """Unit directions whose cosine to r = (0, 0, 1) is c (float32: dot(w, r) is w[2] exactly)."""
    c = c.astype(np.float32)
    return np.stack([np.sqrt(np.maximum(0.0, 1.0 - c.astype(np.float64) ** 2)).astype(np.float32), np.zeros_like(c), c], 1)


def _pg_quadrature(fuzz, lo, hi, nodes=20001):
    """The integral of pg over the directions with lo <= cos <= hi (2 pi pg dc), the restatement's float32 pg at float32 cosines.  Below
    fuzz 1 pg starts like a square root at the lobe's rim, so the nodes are uniform in s = sqrt(c^2 - rim^2), where pg is smooth; the
    trapezoid rule runs over the cosines as float32 holds them."""
    rim = np.sqrt(max(0.0, 1.0 - fuzz * fuzz))
    if fuzz < 1.0:
        s = np.linspace(np.sqrt(max(lo * lo - rim * rim, 0.0)), np.sqrt(hi * hi - rim * rim), nodes)
        c = np.sqrt(s * s + rim * rim)
    else:
        c = np.linspace(lo, hi, nodes)
    c32 = np.clip(c, -1.0, 1.0).astype(np.float32)
    y = gr.pg(_directions(c32), (0, 0, 1), fuzz).astype(np.float64)
    x = c32.astype(np.float64)
    return float(2.0 * np.pi * np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x)))


@pytest.mark.parametrize("fuzz", [0.05, 0.3, 1.0, 1.5])
def test_pg_is_the_density_of_the_lobe(fuzz):
    """pg against the histogram of the restatement's own unit(r + fuzz * random_in_unit_sphere), binned in c = cos to r: every bin's
    count within PG_SIGMAS binomial sigmas of N x (the integral of pg over the bin) — 40 bins, so a 5 sigma bound fails a true density
    about once in 10^5 runs, and the draws are fixed by their seed; and pg integrates to 1 over the sphere within 1e-6."""
    lo = float(np.sqrt(1.0 - fuzz * fuzz)) if fuzz < 1.0 else (0.0 if fuzz == 1.0 else -1.0)
    edges = np.linspace(lo, 1.0, PG_BINS + 1)
    draws = gr.lobe_draws((0, 0, 1), fuzz, PG_DRAWS, 0x9E3779B9)
    assert draws.min() >= lo - 1e-6 and draws.max() <= 1.0 + 1e-6, (draws.min(), draws.max())
    counts, _ = np.histogram(np.clip(draws, lo, 1.0), edges)
    p = np.array([_pg_quadrature(fuzz, edges[k], edges[k + 1], 2001) for k in range(PG_BINS)])
    sigma = np.sqrt(PG_DRAWS * p * (1.0 - p))
    z = (counts - PG_DRAWS * p) / np.maximum(sigma, 1.0)
    total = _pg_quadrature(fuzz, lo, 1.0)
    print(f"fuzz {fuzz}: max |z| over {PG_BINS} bins {np.abs(z).max():.3f}, integral - 1 = {total - 1.0:.3e}")
    assert np.abs(z).max() < PG_SIGMAS, (fuzz, z)
    assert abs(total - 1.0) <= 1e-6, (fuzz, total)
    # outside the lobe, and behind the vertex when it is outside the ball: 0
    if fuzz < 1.0:
        assert not gr.pg(_directions(np.linspace(-1.0, lo - 1e-4, 101)), (0, 0, 1), fuzz).any()
    # both forms agree where both apply (t1 > 0): the factored form against t2^3 - t1^3 in double, to float32 accuracy of the inputs
    c = np.linspace(max(lo, 0.0) + 1e-3, 1.0, 1001)[:-1].astype(np.float32).astype(np.float64)
    f = float(np.float32(fuzz))
    s = np.sqrt(np.maximum(c * c - 1.0 + f * f, 0.0))
    t1, t2 = np.maximum(c - s, 0.0), c + s
    want = (t2 ** 3 - t1 ** 3) / (4.0 * np.pi * f ** 3)
    got = gr.pg(_directions(c), (0, 0, 1), fuzz).astype(np.float64)
    # disc = (c^2 - 1) + fuzz^2 loses up to 2^-24 absolutely before the square root: a relative 2^-24 / disc in disc
    disc = np.maximum(c * c - 1.0 + f * f, 1e-30)
    assert (np.abs(got - want) <= (4 * 2.0 ** -24 / disc + 8 * 2.0 ** -24) * want + 1e-30).all()


@pytest.mark.parametrize("depth", [2, 50])
def test_restatement_identities(depth):
    """gloss_ref.c with both switches on is tree_ref.c bit for bit where no METAL is rough (night rtiow with every fuzz 0), and with both
    off it is tree_ref.c on the test scene — every table, the environment, the lens."""
    m = hot_map()
    shard = rb.Shard(4, 3, 2)
    settings = [dict(planes=p, select=s, nee_mis=mis) for p in (0, 1) for s in (0, 1) for mis in (1, 0)]
    settings += [dict(emitters=False, rgb=m, env_params=ep) for ep in (ENV_MIS, ENV_LIGHT)]
    settings += [dict(planes=1, select=1, rgb=m, env_params=ENV_MIS, lens=LENS)]
    for name, host, cam, gl in (("mirror night rtiow", mirror_night_rtiow(), night_camera(32, 24, 4, depth), 1),
                                ("test scene", scene(), camera(32, 24, 4, depth), 0)):
        for kw in settings:
            for sh, first in ((None, 0), (shard, 0), (None, 37)):
                want = tr.frame(host, cam, shard=sh, sample_first=first, **kw)
                got = gr.frame(host, cam, glossy=gl, glossy_env=gl, shard=sh, sample_first=first, **kw)
                assert_same(got, want, f"{name} depth={depth} glossy={gl} {kw.keys()} shard={sh is not None} first={first}")
    # … and on the test scene the switch does change the estimator
    cam = camera(32, 24, 4, depth)
    assert not np.array_equal(gr.frame(scene(), cam, glossy=1), gr.frame(scene(), cam, glossy=0))


def test_probe_sets_reach_every_counter():
    """The max_depth 50 probe sets of the GPU test, on the restatement alone: every counter a case can move is > 0 in that case — a call
    without an environment weights no miss and one without emitters no hit (possible_counters) — and the lit case with both switches on
    moves all six."""
    for name in probe_cases():
        cnt = probe_reference(name, 50)[5].sum(0)
        got = dict(zip(gr.COUNTERS, (int(x) for x in cnt)))
        print(name, got)
        for k in possible_counters(name):
            assert got[k] > 0, (name, k, got)
    assert possible_counters("lit glossy=11") == gr.COUNTERS


UNBIASED_CAMERA = dict(w=8, h=8, spp=8192, depth=6)


def test_unbiased_against_the_oracle():
    """Test scene, 8 x 8 pixels x 8192 samples of each estimator from disjoint sample ranges (test_nee_planes.py's protocol and bounds):
    the luminance means of every 2 x 2 block agree with the oracle's ray_color (under the map: the path alone, mode 0) within 5 sigma and
    the whole image's within 4 — nee with MIS, nee alone, env with MIS, and lit with both lights, every switch on."""
    host = scene()
    c = UNBIASED_CAMERA
    cam = camera(c["w"], c["h"], c["spp"], c["depth"])
    spp = cam.samples_per_pixel
    m = hot_map()
    _, plain = nr.frame(host, cam, nr.PLAIN, sample_first=0, moments=True)
    _, plain_map = er.frame(host, cam, m, dict(mode=0, scale=0.8), sample_first=0, moments=True)

    def blocks(x):
        return x.reshape(4, 2, 4, 2, 6).sum((1, 3))
    for k, (name, want, kw) in enumerate((("nee mis", plain, dict(glossy=1, nee_mis=1)), ("nee light", plain, dict(glossy=1, nee_mis=0)),
                                          ("env mis", plain_map, dict(glossy=0, glossy_env=1, emitters=False, rgb=m, env_params=ENV_MIS)),
                                          ("lit", plain_map, dict(glossy=1, glossy_env=1, planes=1, rgb=m, env_params=ENV_MIS)))):
        _, got = gr.frame(host, cam, sample_first=(k + 1) * spp, moments=True, **kw)
        z = _zscores(blocks(got), blocks(want), spp * 4)
        za = _zscores(got.sum((0, 1)), want.sum((0, 1)), spp * 64)
        print(f"{name}: 2 x 2 blocks max |z| {np.abs(z).max():.3f}, image z {float(za):.3f}")
        assert np.abs(z).max() < 5.0, (name, np.abs(z).max())
        assert abs(za) < 4.0, (name, za)


# measured on the restatement, whose bits are the device's: luminance MSE of rt_render_nee with glossy = 1 over glossy = 0 at
# 16 spp, 48 x 32, against glossy = 1 at 8192 spp from a disjoint sample range
TEST_SCENE_MSE_RATIO = 0.512558
CONFIG_MSE_RATIO = 0.988109


def _mse_ratio(host, cam_of):
    truth = gr.frame(host, cam_of(8192), glossy=1, sample_first=1 << 20).astype(np.float64) / 8192 @ LUM
    on = gr.frame(host, cam_of(16), glossy=1).astype(np.float64) / 16 @ LUM
    off = gr.frame(host, cam_of(16), glossy=0).astype(np.float64) / 16 @ LUM
    return float(((on - truth) ** 2).mean() / ((off - truth) ** 2).mean())


def test_cli_refusals(test_config_text, tmp_path):
    """--glossy needs a call that takes light samples: exit 99, worded like --light-tree's refusal, and nothing written."""
    before = sorted(os.listdir(tmp_path))
    for args in (["--glossy"], ["--glossy", "--aov"], ["--glossy", "--lens", "0.2:12"], ["--glossy", "--env", "sky.pfm", "--env-mode", "path"]):
        r = subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert r.returncode == 99 and "--glossy" in r.stderr and "it needs --nee" in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before


def test_quality_at_equal_samples(test_config_text):
    """Luminance MSE of glossy = 1 over glossy = 0 at 16 spp (rt_render_nee, mis): below 1 on the test scene, whose rough METAL sees a
    small emitter directly; pinned, not bounded, on the config scene (frame 11 of the test configuration: 0.988 — its lights are large
    and far, and its floor's lobe is wide)."""
    ratio = _mse_ratio(scene(), lambda spp: camera(48, 32, spp))
    print(f"test scene MSE ratio glossy 1 / 0 at 16 spp: {ratio:.6f}")
    assert ratio < 1.0, ratio
    assert abs(ratio - TEST_SCENE_MSE_RATIO) <= 1e-4 * TEST_SCENE_MSE_RATIO, ratio
    chost = config_host(test_config_text)

    def config_camera(spp):
        """Frame 11's whole view at 48 x 32: the pose kept, the pixel deltas scaled, pixel 0's centre moved to the new grid."""
        full = chost.frame_camera(11)
        cam = rb.CameraData.from_buffer_copy(full)
        sx, sy = full.image_width / 48, full.image_height / 32
        for k in range(3):
            cam.pixel_delta_u.e[k] = full.pixel_delta_u.e[k] * sx
            cam.pixel_delta_v.e[k] = full.pixel_delta_v.e[k] * sy
            cam.pixel00_loc.e[k] = (full.pixel00_loc.e[k] - 0.5 * full.pixel_delta_u.e[k] - 0.5 * full.pixel_delta_v.e[k]
                                    + 0.5 * cam.pixel_delta_u.e[k] + 0.5 * cam.pixel_delta_v.e[k])
        cam.image_width, cam.image_height, cam.samples_per_pixel = 48, 32, spp
        return cam
    ratio = _mse_ratio(chost, config_camera)
    print(f"config scene MSE ratio glossy 1 / 0 at 16 spp: {ratio:.6f}")
    assert abs(ratio - CONFIG_MSE_RATIO) <= 1e-4 * CONFIG_MSE_RATIO, ratio


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _device_probe(dev, cam, ijs, call, kw, env):
    if call == "nee":
        return dev.trace_samples_nee(cam, ijs, **kw)
    if call == "env":
        return dev.trace_samples_env(cam, env, ijs, **kw)
    return dev.trace_samples_lit(cam, ijs, env=env, **kw)


def _device_frame(dev, cam, call, kw, env, **more):
    if call == "nee":
        return dev.render_nee_to_host(cam, **kw, **more)
    if call == "env":
        return dev.render_env_to_host(cam, env, **kw, **more)
    return dev.render_lit_to_host(cam, env=env, **kw, **more)


@pytest.mark.gpu
def test_refusals_and_the_old_size_caller():
    """glossy outside {0, 1} is RT_ERR_INVALID_ARG in every call that reads it, before the scene is looked at; a 16-byte rt_nee_params
    does not reach the field."""
    rb.amd_lib().rt_set_device(0)
    lib = rb.amd_lib()
    cam = camera(48, 32, 4)
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f, r, s = (C.c_float * 3)(), (C.c_int32 * 1)(), (C.c_uint32 * 1)()
    fake = C.c_void_p(1 << 32)
    with rb.Env(hot_map()) as env:
        for bad in (2, -1):
            p, e = rb.nee_params(glossy=bad), rb.env_params(glossy=bad)
            lit_n, lit_e = rb.lit_params(nee=p), rb.lit_params(emitters=False, env=env, env_params=e)
            ap = rb.adaptive_params(min_spp=4, batch_spp=4, max_spp=16, threshold=0.1)
            calls = [lambda: lib.rt_render_nee(None, C.byref(cam), C.byref(p), None, 0, fake, None, 1, None),
                     lambda: lib.rt_trace_samples_nee(None, C.byref(cam), C.byref(p), 1, ijs, f, r, s, s),
                     lambda: lib.rt_render_env(None, C.byref(cam), env._h, C.byref(e), None, 0, fake, None, 1, None),
                     lambda: lib.rt_trace_samples_env(None, C.byref(cam), env._h, C.byref(e), 1, ijs, f, r, s, s)]
            for lit in (lit_n, lit_e):
                calls += [lambda lit=lit: lib.rt_render_lit(None, C.byref(cam), C.byref(lit), None, 0, fake, None, 1, None),
                          lambda lit=lit: lib.rt_trace_samples_lit(None, C.byref(cam), C.byref(lit), 1, ijs, f, r, s, s, s),
                          lambda lit=lit: lib.rt_render_lit_adaptive(None, C.byref(cam), C.byref(lit), C.byref(ap), None, 0, fake, fake, None, None, 1, None)]
            for k, call in enumerate(calls):
                st, msg = call(), lib.rt_get_last_error_string().decode()
                assert st == INVALID and "glossy" in msg, (bad, k, st, msg)
        # the checks before it still come first
        assert lib.rt_render_nee(None, C.byref(cam), C.byref(rb.nee_params(select=2, glossy=2)), None, 0, fake, None, 1, None) == INVALID
        assert "select" in lib.rt_get_last_error_string().decode()
        # good values reach the scene check
        for good in (0, 1):
            assert lib.rt_render_nee(None, C.byref(cam), C.byref(rb.nee_params(glossy=good)), None, 0, fake, None, 1, None) == INVALID
            assert "null scene" in lib.rt_get_last_error_string().decode()
        # an older caller's 16-byte struct: the word behind its end is not read — not refused, and not switched on
        host = scene()
        dev = rb.DeviceScene(host, device=0)
        off, _ = dev.render_nee_to_host(cam, params=rb.nee_params(glossy=0))
        on, _ = dev.render_nee_to_host(cam, params=rb.nee_params(glossy=1))
        for word in (1, 2):
            old = rb.nee_params(glossy=word)
            old.struct_bytes = 16
            assert_same(dev.render_nee_to_host(cam, params=old)[0], off, f"16-byte struct with {word} behind its end")
        assert_same(dev.render_nee_to_host(cam, params=rb.nee_params())[0], off, "nee_params()")
        assert_same(dev.render_nee_to_host(cam)[0], off, "NULL params")
        assert not np.array_equal(on, off)
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 50])
def test_probe_samples_equal_the_restatement(depth):
    """10^4 probed samples per case equal gloss_ref.c bit for bit — radiance, rays and every final stream state — over the four emitter
    tables in both modes, the environment in both modes, and lit from a lens with one switch on at a time and both; at max_depth 50 every
    counter a case can move is > 0 in it (test_probe_sets_reach_every_counter explains which), and the lit case with both switches moves
    all six."""
    rb.amd_lib().rt_set_device(0)
    host = scene()
    cam = camera(96, 64, 1, depth)
    ijs = probe_set()
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(hot_map()) as env:
        for name, (rkw, call, kw) in probe_cases().items():
            want = probe_reference(name, depth)
            if depth == 50:
                cnt = dict(zip(gr.COUNTERS, (int(x) for x in want[5].sum(0))))
                for k in possible_counters(name):
                    assert cnt[k] > 0, (name, k, cnt)
            got = _device_probe(dev, cam, ijs, call, kw, env)
            cols = ("radiance", "rays", "seed") + (("nee seed",) if call == "nee" else ("env seed",) if call == "env" else ("nee seed", "env seed"))
            refs = want[:3] + ((want[3],) if call == "nee" else (want[4],) if call == "env" else (want[3], want[4]))
            for g, w, what in zip(got, refs, cols):
                assert_same(g, w, f"{name} depth={depth}: {what}")
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", ["default", "exact"])
def test_frames_equal_the_restatement(traversal):
    rb.amd_lib().rt_set_device(0)
    host = scene()
    dev = rb.DeviceScene(host, device=0, **({} if traversal == "default" else {"traversal": rb.TRAVERSAL_EXACT}))
    shard = rb.Shard(4, 3, 2)
    cam = camera(48, 32, 8)
    cases = probe_cases()
    with rb.Env(hot_map()) as env:
        for name in ("nee planes=0 select=0 mis=1", "nee planes=1 select=1 mis=0", "env mis", "lit glossy=11"):
            rkw, call, kw = cases[name]
            for sh, first in ((None, 0), (shard, 0), (None, 37)):
                got, t = _device_frame(dev, cam, call, kw, env, shard=sh, sample_first=first)
                want = gr.frame(host, cam, shard=sh, sample_first=first, **rkw)
                assert_same(got, want, f"{traversal} {name} shard={sh is not None} first={first}")
                assert t.guarded == 0 and t.trace_scratch_bytes == 0
    dev.close()


@pytest.mark.gpu
def test_device_identities():
    """No rough METAL: glossy = 1 is glossy = 0 bit for bit (night rtiow with every fuzz 0).  And rt_render_lit_adaptive with both
    switches on gives every pixel rt_render_lit's sum at that pixel's own count."""
    rb.amd_lib().rt_set_device(0)
    host = mirror_night_rtiow()
    cam = night_camera(96, 64, 4)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(hot_map()) as env:
        for mis in (1, 0):
            assert_same(dev.render_nee_to_host(cam, params=dict(mis=mis, glossy=1))[0], dev.render_nee_to_host(cam, params=dict(mis=mis))[0],
                        f"nee mis={mis}")
        assert_same(dev.render_env_to_host(cam, env, params=dict(glossy=1))[0], dev.render_env_to_host(cam, env)[0], "env")
        assert_same(dev.render_lit_to_host(cam, env=env, nee=dict(glossy=1), env_params=dict(glossy=1))[0], dev.render_lit_to_host(cam, env=env)[0], "lit")
        dev.close()
        # the light off or empty: nothing to sample, the switch changes nothing (the test scene, rough METAL everywhere)
        host = scene()
        cam = camera(48, 32, 4)
        dev = rb.DeviceScene(host, device=0)
        assert_same(dev.render_env_to_host(cam, env, params=dict(mode=0, glossy=1))[0], dev.render_env_to_host(cam, env, params=dict(mode=0))[0], "env mode 0")
        assert_same(dev.render_lit_to_host(cam, emitters=False, env=env, env_params=dict(mode=0, glossy=1))[0],
                    dev.render_lit_to_host(cam, emitters=False, env=env, env_params=dict(mode=0))[0], "lit with both lights off")
        # adaptive: each pixel is rt_render_lit at its own count
        _, call, kw = probe_cases()["lit glossy=11"]
        cam = camera(32, 24, 1)
        for t in (0.1, 0.05, 0.2, 0.03, 0.3):
            fb, spp, _, _ = dev.render_lit_adaptive_to_host(cam, env=env, min_spp=4, batch_spp=4, max_spp=16, threshold=t, **kw)
            if len(np.unique(spp)) >= 3:
                break
        levels = np.unique(spp)
        assert len(levels) >= 3 and set(levels) <= {4, 8, 12, 16}, levels
        for n in levels:
            c = rb.CameraData.from_buffer_copy(cam)
            c.samples_per_pixel = int(n)
            uniform, _ = dev.render_lit_to_host(c, env=env, **kw)
            assert_same(fb[spp == n], uniform[spp == n], f"pixels that stopped at {n}")
        want = gr.frame(host, camera(32, 24, 4), **probe_cases()["lit glossy=11"][0])
        assert_same(fb[spp == 4], want[spp == 4], "the restatement at min_spp")
    dev.close()


@pytest.mark.gpu
def test_handle_state():
    """A glossy = 1 call between two glossy = 0 calls leaves the latter identical, and the emitter table and tree are not rebuilt."""
    rb.amd_lib().rt_set_device(0)
    host = scene()
    cam = camera(48, 32, 4)
    params = dict(sample_planes=1, select=1)
    fresh = []
    for g in (0, 1):
        dev = rb.DeviceScene(host, device=0)
        fresh.append(dev.render_nee_to_host(cam, params=dict(glossy=g, **params))[0])
        dev.close()
    assert not np.array_equal(fresh[0], fresh[1])
    dev = rb.DeviceScene(host, device=0)
    first, _ = dev.render_to_host(cam)
    before = dev.last_timing()
    assert_same(dev.render_nee_to_host(cam, params=dict(glossy=0, **params))[0], fresh[0], "glossy=0 first")
    table, tree = dev.nee_emitter_table(params), dev.nee_light_tree(params)
    assert_same(dev.render_nee_to_host(cam, params=dict(glossy=1, **params))[0], fresh[1], "glossy=1 between")
    assert_same(dev.render_nee_to_host(cam, params=dict(glossy=0, **params))[0], fresh[0], "glossy=0 after")
    for g, w in zip(dev.nee_emitter_table(dict(glossy=1, **params)), table):
        assert_same(g, w, "emitter table after a glossy call")
    after = dev.nee_light_tree(dict(glossy=1, **params))
    for k in tree:
        assert_same(after[k], tree[k], f"light tree after a glossy call: {k}")
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    assert_same(dev.render_to_host(cam)[0], first, "rt_render after the glossy calls")
    dev.close()
