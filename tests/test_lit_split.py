"""rt_render_lit_split / rt_trace_samples_lit_split / rt_denoise_split: rt_render_lit's frame as its direct and its indirect light
(include/rtp_amd.h, "direct and indirect light in separate frames").

The header defines the two components by a stage of the path; tests/cpu_native/lit_split_ref.c restates that on the oracle
(lit_split_reference.py), and probed samples and frames must equal it byte for byte.  On the CPU: the ABI and the argument checks, the
restatement against lit_reference (bit for bit where the split cannot reorder a sum, within the bound of two summing orders where it
can), the all-LAMBERTIAN identity and the CLI refusals.

The bound of "direct + indirect against the beauty sample": both are sums of the same at most 3 * max_depth + 1 non-negative floats (per
vertex an emission or miss term and two light samples) in two orders, each with at most 3 * max_depth roundings of relative size 2^-24
on partial sums no larger than the total; per pixel the same over spp samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import env_reference as er
import lit_reference as lr
import lit_split_reference as lsr
import rtp_bindings as rb
import test_glossy as tg
from test_lit import (EXE, HERE, INVALID, LENS, MAT_LAMBERTIAN, MAT_LIGHT, assert_same, config_camera, config_host, dev_args, four_settings, material,
                      night_camera, night_rtiow, ref_args, scaled, setting, three_ball_scene, write_pfm)

SKY_MIS = dict(mode=1, scale=0.75)
N = 4000


def sample_bound(depth):
    return 2.0 * (3 * depth) * 2.0 ** -24


def assert_sum_within(direct, indirect, beauty, rel, what):
    got = direct.astype(np.float64) + indirect.astype(np.float64)
    err = np.abs(got - beauty.astype(np.float64))
    lim = rel * beauty.astype(np.float64)
    worst = (err / np.maximum(beauty.astype(np.float64), 1e-300)).max() if err.size else 0.0
    print(f"{what}: worst |direct + indirect - beauty| / beauty = {worst:.3e} (bound {rel:.3e})")
    assert (err <= lim).all(), f"{what}: {(err > lim).sum()} components outside the bound, worst {worst:.3e} against {rel:.3e}"


def random_ijs(cam, rng, n=N):
    return np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)


def lambert_scene():
    """A LAMBERTIAN floor sphere, three LAMBERTIAN balls and one DIFFUSE_LIGHT sphere: every scattering vertex is a diffuse event."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_LAMBERTIAN, (0.8, 0.3, 0.3)), material(MAT_LAMBERTIAN, (0.3, 0.8, 0.3)),
            material(MAT_LAMBERTIAN, (0.3, 0.3, 0.8)), material(MAT_LIGHT, emit=(8.0, 6.0, 4.0))]
    sph = [[0, -100, 0, 100, 0], [-2.1, 1, 0, 1, 1], [0, 1, 0, 1, 2], [2.1, 1, 0, 1, 3], [0, 3.2, 0.5, 0.4, 4]]
    return rb.HostScene.from_arrays(np.array(sph, np.float32), np.zeros((0, 11), np.float32), mats)


def lambert_camera(w, h, spp, depth):
    return rb.make_camera(w, h, 40.0, (0, 2, 8), (0, 1, 0), (0.02, 0.03, 0.05), spp, depth)


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_symbols():
    lib = rb.amd_lib()
    for s in ("rt_render_lit_split", "rt_trace_samples_lit_split", "rt_denoise_split", "rt_denoise_split_workspace_bytes"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert len(lib.rt_render_lit_split.argtypes) == 10 and len(lib.rt_trace_samples_lit_split.argtypes) == 11
    assert len(lib.rt_denoise_split.argtypes) == 11
    for name in ("render_lit_split", "render_lit_split_to_host", "trace_samples_lit_split"):
        assert hasattr(rb.DeviceScene, name)
    assert hasattr(rb, "denoise_split") and hasattr(rb, "denoise_split_to_host")
    assert lib.rt_denoise_split_workspace_bytes(77, 45) == lib.rt_denoise_workspace_bytes(77, 45) + 77 * 45 * 12
    assert lib.rt_denoise_split_workspace_bytes(0, 45) == 0 and lib.rt_denoise_split_workspace_bytes(3, -1) == 0


def _calls(cam, lit):
    """(status, message) of rt_render_lit_split and of rt_trace_samples_lit_split with a null scene."""
    lib = rb.amd_lib()
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f, g = (C.c_float * 3)(), (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    pc = C.byref(cam) if cam is not None else None
    pl = C.byref(lit) if lit is not None else None
    out = [lib.rt_render_lit_split(None, pc, pl, None, 0, C.c_void_p(1 << 32), C.c_void_p(1 << 33), None, 1, None), lib.rt_get_last_error_string().decode()]
    out += [lib.rt_trace_samples_lit_split(None, pc, pl, 1, ijs, f, g, r, s, s, s), lib.rt_get_last_error_string().decode()]
    return out


def test_argument_checks_are_rt_render_lits_in_its_order():
    """The checks that need no device: every parameter refusal of rt_render_lit comes first, lens before emitters before environment, then
    the null scene — also with NULL outputs, whose refusal comes after rt_render_lit's own."""
    cam = rb.rtiow_camera(8, 4, 2)
    fake_env = 1 << 32

    def refused(word, cam=cam, **kw):
        lit = kw.pop("lit", None) or rb.lit_params(**kw)
        st1, m1, st2, m2 = _calls(cam, lit)
        assert st1 == INVALID and word in m1 and "rt_render_lit_split" in m1, (word, kw, m1)
        assert st2 == INVALID and word in m2 and "rt_trace_samples_lit_split" in m2, (word, kw, m2)

    def with_env(**kw):
        lit = rb.lit_params(**kw)
        lit.env = fake_env
        return lit
    short = rb.lit_params()
    short.struct_bytes = 4
    refused("struct_bytes", lit=short)
    two = rb.lit_params()
    two.sample_emitters = 2
    refused("sample_emitters", lit=two)
    assert "null camera" in _calls(None, rb.lit_params())[1] and "null camera" in _calls(None, rb.lit_params())[3]
    close = rb.CameraData.from_buffer_copy(cam)
    close.image_width = 9
    refused("cam_close", cam_close=close)
    refused("lens_radius", lens=dict(lens_radius=-0.1))
    refused("focus_distance", lens=dict(lens_radius=0.1, focus_distance=0.0))
    refused("mis", nee=dict(mis=2))
    refused("mode", lit=with_env(env_params=dict(mode=3)))
    refused("scale", lit=with_env(env_params=dict(scale=-0.5)))
    assert "lens_radius" in _calls(cam, with_env(lens=dict(lens_radius=-1.0), nee=dict(mis=2), env_params=dict(mode=3)))[1]
    assert "mis" in _calls(cam, with_env(nee=dict(mis=2), env_params=dict(mode=3)))[1]
    for lit in (None, rb.lit_params(), rb.lit_params(emitters=False), with_env(env_params=dict(mode=2, rot=er.Z_UP))):
        st1, m1, st2, m2 = _calls(cam, lit)
        assert st1 == INVALID and "null scene" in m1, m1
        assert st2 == INVALID, m2
    lib = rb.amd_lib()
    # the outputs are looked at after rt_render_lit's checks: bad parameters and the null scene outrank a NULL output
    assert lib.rt_render_lit_split(None, C.byref(cam), C.byref(rb.lit_params(nee=dict(mis=2))), None, 0, None, None, None, 1, None) == INVALID
    assert "mis" in lib.rt_get_last_error_string().decode()
    assert lib.rt_render_lit_split(None, C.byref(cam), None, None, 0, None, None, None, 1, None) == INVALID
    assert "null scene" in lib.rt_get_last_error_string().decode()
    assert lib.rt_trace_samples_lit_split(None, C.byref(cam), None, -1, None, None, None, None, None, None, None) == INVALID
    assert lib.rt_trace_samples_lit_split(None, C.byref(cam), None, 1, (C.c_int32 * 3)(), None, None, None, None, None, None) == INVALID
    assert "null argument" in lib.rt_get_last_error_string().decode()
    # rt_denoise_split: a NULL component first, then rt_denoise's own checks under its own name
    one = C.c_void_p(1 << 32)
    b = rb.AovBuffers()
    assert lib.rt_denoise_split(None, one, C.byref(b), 4, 4, 1, None, one, 1 << 20, one, None) == INVALID
    assert "rt_denoise_split: null argument" in lib.rt_get_last_error_string().decode()
    assert lib.rt_denoise_split(one, None, C.byref(b), 4, 4, 1, None, one, 1 << 20, one, None) == INVALID
    assert lib.rt_denoise_split(one, one, C.byref(b), 4, 4, 1, None, one, 1 << 20, one, None) == INVALID
    assert "rt_denoise_split" in lib.rt_get_last_error_string().decode() and "required" in lib.rt_get_last_error_string().decode()


def _cpu_cases(test_config_text):
    night = night_rtiow()
    yield "night rtiow", night, lambda d: night_camera(320, 180, 1, d), None
    host, cam = three_ball_scene(spp=1, lamp=True, w=64, h=48)
    yield "three balls with a lamp", host, lambda d, c=cam: scaled(c, 64, 48, 1, d), None
    cfg = config_host(test_config_text)
    yield "config frame 11", cfg, lambda d: config_camera(cfg, 11, 96, 64, 1, d), er.Z_UP


def test_restatement_against_lit_reference(test_config_text):
    """lit_split_ref.c against lit_ref.c, 4000 random samples per scene, emitters plus the sun-and-sky map with MIS, pinhole and lens:
    max_depth <= 2 cannot cross before the last vertex — direct is the beauty sample bit for bit and indirect is zero; deeper, rays and
    the three streams are bit for bit, both components are non-negative and their sum is the beauty sample within the bound."""
    m = er.sun_and_sky(256)
    rng = np.random.default_rng(41)
    for name, host, camera, rot in _cpu_cases(test_config_text):
        ep = dict(SKY_MIS, **({"rot": rot} if rot is not None else {}))
        ijs = random_ijs(camera(1), rng)
        for lens in (None, LENS):
            kw = dict(lens=lens, emitters=True, nee_mis=1, rgb=m, env_params=ep)
            for depth in (0, 1, 2, 3, 50):
                what = f"{name} lens={lens is not None} depth={depth}"
                cam = camera(depth)
                direct, indirect, *rest = lsr.trace(host, cam, ijs, **kw)
                beauty, *want = lr.trace(host, cam, ijs, **kw)
                for g, w, col in zip(rest, want, ("rays", "seed", "nee seed", "env seed")):
                    assert_same(g, w, f"{what}: {col}")
                if depth <= 2:
                    assert_same(direct, beauty, f"{what}: direct is the beauty sample")
                    assert not indirect.any(), f"{what}: indirect is zero"
                    continue
                assert (direct >= 0).all() and (indirect >= 0).all(), what
                assert_sum_within(direct, indirect, beauty, sample_bound(depth), what)
                lit = (indirect > 0).any(1).mean()
                print(f"{what}: samples with indirect > 0: {lit:.4f}")
                if name == "night rtiow" and depth == 50 and lens is None:
                    assert lit >= 0.20, lit          # (not vacuous: the restatement gives 0.271 here)


def test_all_lambertian_direct_is_depth_two():
    """Where every scattering vertex is a diffuse event the crossing comes behind the second vertex: direct at max_depth 50 is
    rt_render_lit's sample at max_depth 2, bit for bit."""
    host = lambert_scene()
    rng = np.random.default_rng(43)
    m = er.sun_and_sky(256)
    ijs = random_ijs(lambert_camera(64, 48, 1, 50), rng)
    for kw in (dict(), dict(rgb=m, env_params=SKY_MIS), dict(rgb=m, env_params=SKY_MIS, lens=LENS, nee_mis=0)):
        direct, indirect = lsr.trace(host, lambert_camera(64, 48, 1, 50), ijs, **kw)[:2]
        assert_same(direct, lr.trace(host, lambert_camera(64, 48, 1, 2), ijs, **kw)[0], f"direct at depth 50, {sorted(kw)}")
        assert (indirect > 0).any(), "the scene has indirect light"


def test_cli_refusals(test_config_text, tmp_path):
    before = sorted(os.listdir(tmp_path))

    def run(args, env=None):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                              env={**os.environ, **(env or {})})
    cases = [(["--split"], {}), (["--nee", "--split"], {}), (["--lit", "--split", "--fog", "0.1"], {}), (["--lit", "--split", "--fog-denoise"], {}),
             (["--lit", "--fog", "0.1", "--fog-tint", "1,1,1", "--split"], {}), (["--lit", "--split", "--fog-adaptive", "0.1"], {}),
             (["--lit", "--split", "--noise-target", "0.1"], {}), (["--lit", "--split", "--adaptive", "0.1"], {}),
             (["--lit", "--split", "--devices", "2"], {}), (["--lit", "--split", "--shard", "2"], {}), (["--lit", "--split"], {"RTP_DEVICES": "2"}),
             (["--lit", "--split", "--denoise-temporal"], {}), (["--lit", "--split", "--denoise-adaptive"], {}),
             (["--lit", "--split", "--denoise-adaptive-temporal"], {}), (["--lit", "--split", "--noise-target", "0.1", "--denoise-adaptive"], {}),
             (["--lit", "--split", "--stop-rule", "near"], {}), (["--lit", "--split", "--stop-history"], {})]
    for args, env in cases:
        r = run(args, env)
        assert r.returncode == 99 and "--split" in r.stderr, (args, env, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _gpu_scenes(test_config_text, w, h, spp, depth, config_frame=11):
    host = config_host(test_config_text)
    cam = scaled(host.frame_camera(config_frame), w, h, spp, depth)
    close = scaled(host.frame_camera_at(config_frame + 0.5), w, h, spp, depth)
    yield "config", host, cam, close, er.Z_UP
    yield "night rtiow", night_rtiow(), night_camera(w, h, spp, depth), night_camera(w, h, spp, depth, eye=(12.6, 3.2, 2.5)), None


SPLIT_COLUMNS = ("direct", "indirect", "rays", "seed", "nee seed", "env seed")


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [3, 50])
def test_probe_equals_the_restatement(test_config_text, depth):
    rb.amd_lib().rt_set_device(0)
    rng = np.random.default_rng(45)
    m = er.sun_and_sky(256)
    with rb.Env(m) as env:
        for name, host, cam, close, rot in _gpu_scenes(test_config_text, 320, 180, 1, depth):
            dev = rb.DeviceScene(host, device=0)
            ijs = random_ijs(cam, rng)
            for what, s in four_settings(m, close, rot):
                got = dev.trace_samples_lit_split(cam, ijs, **dev_args(s, env))
                want = lsr.trace(host, cam, ijs, **ref_args(s))
                for g, w_, col in zip(got, want, SPLIT_COLUMNS):
                    assert_same(g, w_, f"{name} depth={depth}, {what}: {col}")
            dev.close()


FRAME_CASES = {"whole": dict(), "shard": dict(shard=(4, 3, 2)), "sample_first": dict(sample_first=37), "pass_spp": dict(config=dict(pass_spp=3)),
               "tiny": dict(size=(7, 5, 1))}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FRAME_CASES))
def test_frames_equal_the_restatement(test_config_text, case):
    rb.amd_lib().rt_set_device(0)
    how = FRAME_CASES[case]
    w, h, spp = how.get("size", (64, 48, 4))
    shard = rb.Shard(*how["shard"]) if "shard" in how else None
    first = how.get("sample_first", 0)
    m = er.sun_and_sky(256)
    with rb.Env(m) as env:
        for depth in (1, 2, 3, 50):
            for name, host, cam, close, rot in _gpu_scenes(test_config_text, w, h, spp, depth):
                dev = rb.DeviceScene(host, device=0, **how.get("config", {}))
                for what, s in four_settings(m, close, rot)[:2]:
                    direct, indirect, t = dev.render_lit_split_to_host(cam, shard=shard, sample_first=first, **dev_args(s, env))
                    want = lsr.frame(host, cam, shard=shard, sample_first=first, **ref_args(s))
                    assert_same(direct, want[0], f"{case} {name} depth={depth}, {what}: direct")
                    assert_same(indirect, want[1], f"{case} {name} depth={depth}, {what}: indirect")
                    assert t.guarded == 0 and t.trace_scratch_bytes == 0, (t.guarded, t.trace_scratch_bytes)
                    assert t.trace_launches == (2 if case == "pass_spp" else 1), t.trace_launches
                dev.close()


def _switch_cases():
    lens = dict(lens_radius=tg.LENS[0], focus_distance=tg.LENS[1])
    cases = {"planes": dict(nee=dict(sample_planes=1)), "select": dict(nee=dict(select=1)), "glossy": dict(nee=dict(glossy=1)),
             "all three": dict(nee=dict(sample_planes=1, select=1, glossy=1)),
             "planes, tree": dict(nee=dict(sample_planes=1, select=1)), "planes, glossy": dict(nee=dict(sample_planes=1, glossy=1)),
             "env glossy": dict(env_params=dict(glossy=1, **tg.ENV_MIS)),
             "all, env glossy, lens": dict(nee=dict(sample_planes=1, select=1, glossy=1), env_params=dict(glossy=1, **tg.ENV_MIS), lens=lens),
             "select, lens": dict(nee=dict(select=1), lens=lens), "select, glossy, lens": dict(nee=dict(select=1, glossy=1), lens=lens)}
    return cases


@pytest.mark.gpu
def test_identities_over_every_table_and_switch():
    """What needs no restatement, on test_glossy.py's scene (emissive planes, rough METAL) under its hot map, for every emitter table
    (sample_planes x select), the glossy switches and the lens: max_depth 1 and 2 are rt_render_lit bit for bit with a zero indirect
    frame; at depth 50 the probe's rays and streams are rt_trace_samples_lit's and the sum is the beauty sample within the bound, per
    sample and per pixel."""
    rb.amd_lib().rt_set_device(0)
    host = tg.scene()
    dev = rb.DeviceScene(host, device=0)
    rng = np.random.default_rng(47)
    w, h, spp = 48, 32, 4
    with rb.Env(tg.hot_map()) as env:
        for name, kw in _switch_cases().items():
            kw = dict(env=env, **kw)
            kw.setdefault("env_params", tg.ENV_MIS)
            for depth in (1, 2):
                cam = tg.camera(w, h, spp, depth)
                direct, indirect, _ = dev.render_lit_split_to_host(cam, **kw)
                assert_same(direct, dev.render_lit_to_host(cam, **kw)[0], f"{name} depth={depth}: direct is rt_render_lit")
                assert not indirect.any(), f"{name} depth={depth}: indirect is zero"
            cam = tg.camera(w, h, spp, 50)
            ijs = random_ijs(cam, rng)
            direct, indirect, *rest = dev.trace_samples_lit_split(cam, ijs, **kw)
            beauty, *want = dev.trace_samples_lit(cam, ijs, **kw)
            for g, w_, col in zip(rest, want, SPLIT_COLUMNS[2:]):
                assert_same(g, w_, f"{name}: {col}")
            assert (direct >= 0).all() and (indirect >= 0).all(), name
            assert_sum_within(direct, indirect, beauty, sample_bound(50), f"{name}: probe")
            assert (indirect > 0).any(), name
            direct, indirect, t = dev.render_lit_split_to_host(cam, **kw)
            assert t.trace_scratch_bytes == 0, (name, t.trace_scratch_bytes)
            assert_sum_within(direct, indirect, dev.render_lit_to_host(cam, **kw)[0], 2.0 * spp * (3 * 50 + 1) * 2.0 ** -24, f"{name}: frame")
    dev.close()
    # the all-LAMBERTIAN identity, on the device and for the frame call
    host = lambert_scene()
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(er.sun_and_sky(256)) as env:
        for kw in (dict(), dict(env=env, env_params=SKY_MIS), dict(env=env, env_params=SKY_MIS, nee=dict(select=1), lens=dict(lens_radius=0.1, focus_distance=8.0))):
            direct, indirect, _ = dev.render_lit_split_to_host(lambert_camera(64, 48, 4, 50), **kw)
            assert_same(direct, dev.render_lit_to_host(lambert_camera(64, 48, 4, 2), **kw)[0], f"all LAMBERTIAN, {sorted(kw)}")
            assert indirect.any()
    dev.close()


def _split_frames(w, h, spp):
    host, cam = three_ball_scene(spp=spp, depth=8, lamp=True, w=w, h=h)
    dev = rb.DeviceScene(host, device=0)
    direct, indirect, _ = dev.render_lit_split_to_host(cam)
    aov, _ = dev.render_aov_to_host(cam)
    dev.close()
    return direct, indirect, aov


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(77, 45, 8), (1, 1, 8)])
def test_denoise_split_is_two_denoise_calls_added(size):
    rb.amd_lib().rt_set_device(0)
    w, h, spp = size
    direct, indirect, aov = _split_frames(w, h, spp)
    for iterations in (0, 5):
        got = rb.denoise_split_to_host(direct, indirect, aov, spp, iterations=iterations)
        want = rb.denoise_to_host(direct, aov, spp, iterations=iterations) + rb.denoise_to_host(indirect, aov, spp, iterations=iterations)
        assert want.dtype == np.float32
        assert_same(got, want, f"{w} x {h}, iterations={iterations}")


@pytest.mark.gpu
def test_denoise_split_argument_checks():
    import torch
    rb.amd_lib().rt_set_device(0)
    lib = rb.amd_lib()
    w, h = 16, 8
    need = lib.rt_denoise_split_workspace_bytes(w, h)
    fb = torch.zeros((3, h, w, 3), device="cuda:0")
    guides = torch.zeros((4, h, w, 3), device="cuda:0")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    aov = {"albedo": guides[0].data_ptr(), "normal": guides[1].data_ptr(), "depth": guides[2].data_ptr(), "hits": guides[3].data_ptr()}
    a, b, out = fb[0].data_ptr(), fb[1].data_ptr(), fb[2].data_ptr()

    def refused(word, **kw):
        args = dict(d_direct=a, d_indirect=b, aov_ptrs=aov, width=w, height=h, spp=4, d_out=out, workspace=(ws.data_ptr(), need))
        args.update(kw)
        with pytest.raises(rb.RtError) as e:
            rb.denoise_split(**args)
        assert word in str(e.value) and "rt_denoise_split" in str(e.value), (word, str(e.value))
    refused("workspace_bytes", workspace=(ws.data_ptr(), lib.rt_denoise_workspace_bytes(w, h)))
    refused("overlaps an input", d_out=a)
    refused("overlaps an input", d_out=b)
    refused("overlaps", d_out=ws.data_ptr())
    refused("samples_per_pixel", spp=0)
    refused("width", width=0)
    refused("iterations", iterations=9)
    refused("required", aov_ptrs={k: v for k, v in aov.items() if k != "depth"})
    rb.denoise_split(a, b, aov, w, h, 4, out, workspace=(ws.data_ptr(), need))          # the good call, and one component twice
    rb.denoise_split(a, a, aov, w, h, 4, out, workspace=(ws.data_ptr(), need))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_cli_split_files_are_the_python_paths(test_config_text, tmp_path):
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    out = subprocess.run([EXE, "--gpu", "--lit", "--nee", "--split", "--denoise"], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    for f in range(info.num_frames):
        cam = host.frame_camera_at(float(f))
        direct, indirect, _ = dev.render_lit_split_to_host(cam, nee=dict(mis=1))
        aov, _ = dev.render_aov_lens_to_host(cam)          # (the driver's AOV call, with its pinhole and closed shutter)
        denoised = rb.denoise_split_to_host(direct, indirect, aov, cam.samples_per_pixel)
        for suffix, fb in (("", direct + indirect), (".direct", direct), (".indirect", indirect), (".denoised", denoised)):
            want = rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp)
            assert open(tmp_path / f"f_{f}.png{suffix}", "rb").read() == want, (f, suffix)
    dev.close()


@pytest.mark.gpu
def test_handle_state():
    """A split frame between two rt_render_lit frames and two default rt_render frames on one handle changes neither: the slab is the
    handle's, shared and regrown for two components."""
    rb.amd_lib().rt_set_device(0)
    m = er.sun_and_sky(256)
    host = night_rtiow()
    cam = night_camera(128, 72, 8)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(m) as env:
        kw = dict(env=env, env_params=SKY_MIS)
        lit_before = dev.render_lit_to_host(cam, **kw)[0]
        plain_before = dev.render_to_host(cam)[0]
        timing_before = bytes(dev.last_timing())
        direct, indirect, t = dev.render_lit_split_to_host(cam, **kw)
        assert t.kernel_ms > 0 and t.trace_launches >= 1
        assert bytes(dev.last_timing()) == timing_before, "rt_last_timing still reports the last rt_render"
        assert_same(dev.render_lit_to_host(cam, **kw)[0], lit_before, "rt_render_lit after rt_render_lit_split")
        assert_same(dev.render_to_host(cam)[0], plain_before, "rt_render after rt_render_lit_split")
        again = dev.render_lit_split_to_host(cam, **kw)
        assert_same(again[0], direct, "direct, again")
        assert_same(again[1], indirect, "indirect, again")
        assert_sum_within(direct, indirect, lit_before, 2.0 * 8 * (3 * 50 + 1) * 2.0 ** -24, "night rtiow frame")
        # overlapping and NULL outputs are refused once rt_render_lit's checks have passed
        lib = rb.amd_lib()
        lit = rb.lit_params()
        for a, b in ((1 << 32, (1 << 32) + 12), (1 << 32, 1 << 32), (0, 1 << 32), (1 << 32, 0)):
            st = lib.rt_render_lit_split(dev._h, C.byref(cam), C.byref(lit), None, 0, C.c_void_p(a), C.c_void_p(b), None, 1, None)
            assert st == INVALID and "rt_render_lit_split" in lib.rt_get_last_error_string().decode(), (a, b)
    dev.close()
