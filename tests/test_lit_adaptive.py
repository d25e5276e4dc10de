"""rt_render_lit_adaptive: rt_render_adaptive's rounds on rt_render_lit's estimator (include/rtp_amd.h).

The promise is §11's: every pixel is, bit for bit, rt_render_lit at that pixel's own sample count.  The reference
(lit_adaptive_reference.py) is composition — tree_reference.trace's per-sample radiances, test_adaptive.reference's rule and moments,
float32 sums in sample order — and the device must equal it in fb, spp and moments byte for byte, in five lit settings that between
them use the light tree, the two-kind table, the power table sampled alone, the lens and an environment.  On the CPU: the ABI, every
refusal and their order, the condition on the inputs (every stop level is populated in every setting), the helper's own identity, the
CLI's refusals and what the rule buys at equal samples."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import env_reference as er
import lit_adaptive_reference as lar
import rtp_bindings as rb
import test_adaptive as ta
import test_light_tree as tl
import tree_reference as tr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
FAKE = 1 << 32          # a device address that is never dereferenced
OK, INVALID, UNSUPPORTED = 0, 1, 4
F = np.float32
SPP, THRESHOLD, SIZE = lar.SPP, lar.THRESHOLD, lar.SIZE
LEVELS = list(range(4, 33, 4))
LIGHT_BLOCK, LIGHT_CHUNK = 256, 128          # rt_light.hip.inc: kLightBlock, kLightChunk
assert_same = ta.assert_same


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_symbol_argtypes_and_methods():
    lib = rb.amd_lib()
    assert hasattr(lib, "rt_render_lit_adaptive") and "rt_render_lit_adaptive" in rb.RTP_AMD_SYMBOLS
    assert len(lib.rt_render_lit_adaptive.argtypes) == 12
    for name in ("render_lit_adaptive", "render_lit_adaptive_to_host"):
        assert hasattr(rb.DeviceScene, name)
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        assert "rt_status rt_render_lit_adaptive(" in f.read()


def _params(**kw):
    return rb.adaptive_params(**{**dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1), **kw})


def _call(params="default", lit="default", scene=None, cam="default", fb=FAKE, spp=2 * FAKE, mom=None, sample_first=0):
    lib = rb.amd_lib()
    if params == "default":
        params = _params()
    if lit == "default":
        lit = rb.lit_params()
    if cam == "default":
        cam = rb.make_camera(8, 4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    st = lib.rt_render_lit_adaptive(scene, C.byref(cam) if cam is not None else None, C.byref(lit) if lit is not None else None,
                                    C.byref(params) if params is not None else None, None, sample_first, C.c_void_p(fb), C.c_void_p(spp),
                                    C.c_void_p(mom), None, 1, None)
    return st, lib.rt_get_last_error_string().decode()


def _fake_env_lit(**env_params):
    lit = rb.lit_params(env_params=env_params)
    lit.env = FAKE          # (never dereferenced: the scene is null)
    return lit


def test_refusals_and_their_order():
    """Every refusal that needs no scene, with its code and a word of its message — and the order: adaptive parameters, then lit
    parameters (lens, nee, env_params), then the sample range, then the buffers, then the scene."""
    # 1. rt_render_adaptive's parameter checks
    assert _call(params=None)[0] == INVALID
    short = _params()
    short.struct_bytes = 4
    assert _call(params=short)[0] == INVALID
    for kw, code, word in ((dict(min_spp=1), INVALID, "min_spp"), (dict(min_spp=-5), INVALID, "min_spp"), (dict(batch_spp=0), INVALID, "batch_spp"),
                           (dict(max_spp=3), INVALID, "max_spp"), (dict(threshold=-0.01), INVALID, "threshold"),
                           (dict(threshold=float("nan")), INVALID, "threshold"), (dict(threshold=float("inf")), INVALID, "threshold"),
                           (dict(max_spp=65537), UNSUPPORTED, "65536"), (dict(min_spp=70000, max_spp=70000), UNSUPPORTED, "65536")):
        st, msg = _call(params=_params(**kw))
        assert st == code and word in msg and "rt_render_lit_adaptive" in msg, (kw, st, msg)
    # 2. rt_render_lit's, in its order: lens, nee (only with emitters), env_params (only with an environment)
    bad_lens, bad_nee = dict(lens_radius=-1.0), dict(mis=3)
    for lit, word in ((rb.lit_params(lens=bad_lens, nee=bad_nee), "lens_radius"), (rb.lit_params(nee=bad_nee), "mis"),
                      (rb.lit_params(nee=dict(select=2)), "select"), (_fake_env_lit(mode=5), "mode"),
                      (rb.lit_params(emitters=2), "sample_emitters")):
        st, msg = _call(lit=lit)
        assert st == INVALID and word in msg, (word, st, msg)
    lit = rb.lit_params(nee=bad_nee)
    lit.env = FAKE
    bad_ep = rb.env_params_of(mode=5)
    lit.env_params = C.pointer(bad_ep)
    assert "mis" in _call(lit=lit)[1], "nee before env_params"
    assert "null scene" in _call(lit=rb.lit_params(emitters=False, nee=bad_nee))[1], "nee is read only when emitters are sampled"
    assert "null scene" in _call(lit=rb.lit_params(env_params=dict(mode=5)))[1], "env_params is read only with an environment"
    assert "null scene" in _call(lit=None)[1], "lit NULL means the defaults"
    assert _call(cam=None)[0] == INVALID
    short_lit = rb.lit_params()
    short_lit.struct_bytes = 4
    assert _call(lit=short_lit)[0] == INVALID
    # 3. the sample range: sample_first + min_spp + R * batch_spp (here 4 + 15 * 4 = 64)
    st, msg = _call(sample_first=-1)
    assert st == INVALID and "sample_first" in msg, msg
    assert _call(sample_first=(1 << 30) - 64)[1].find("null scene") >= 0
    st, msg = _call(sample_first=(1 << 30) - 63)
    assert st == UNSUPPORTED and "2^30" in msg, msg
    assert "null scene" in _call(params=_params(max_spp=67), sample_first=(1 << 30) - 64)[1], "R * batch, not max_spp, counts"
    # 4. the buffers
    for kw in (dict(fb=0), dict(spp=0)):
        st, msg = _call(**kw)
        assert st == INVALID and "null framebuffer or sample counts" in msg, (kw, msg)
    # 5. the scene
    st, msg = _call()
    assert st == INVALID and "null scene" in msg, msg
    # the order
    assert "min_spp" in _call(params=_params(min_spp=1), lit=rb.lit_params(lens=bad_lens), fb=0, sample_first=-1)[1]
    assert "lens_radius" in _call(lit=rb.lit_params(lens=bad_lens), fb=0, sample_first=-1)[1]
    assert "sample_first" in _call(fb=0, sample_first=-1)[1]
    assert "null framebuffer" in _call(fb=0)[1]
    # a short struct of an older caller: its fields, defaults for the rest (batch_spp 0 is past its end: 16)
    p = _params(batch_spp=0)
    p.struct_bytes = 8
    st, msg = _call(params=p)
    assert st == INVALID and "null scene" in msg, msg


@pytest.mark.parametrize("setting", list(lar.SETTINGS))
def test_every_stop_level_is_populated(setting):
    """The condition on the inputs of the GPU tests: each of the 8 levels 4, 8, …, 32 holds at least 5 pixels, so every round's list is
    non-trivial and every stop level is compared."""
    _, spp, _ = lar.setting_reference(setting)
    counts = [int((spp == n).sum()) for n in LEVELS]
    print(f"setting {setting}: pixels per level {dict(zip(LEVELS, counts))}")
    assert sum(counts) == spp.size
    assert min(counts) >= 5, counts


def test_helper_identity_with_everything_off():
    """e': emitters off, no map, no lens, sample_first = 0 — the reference's counts and moments are test_adaptive.reference's over the
    same radiances, and its sums the restatement's frame at each pixel's own count."""
    host, cam = tl.scene("lamp"), tl.camera("lamp", *SIZE, 1)
    kw = dict(select=0, emitters=False)
    fb, spp, mom = lar.reference(host, cam, threshold=THRESHOLD, **SPP, **kw)
    rad = lar.radiances(host, cam, SPP["max_spp"], **kw)
    n, s1, s2 = ta.reference(rad.reshape(-1, SPP["max_spp"], 3), SPP["min_spp"], SPP["batch_spp"], SPP["max_spp"], THRESHOLD)
    assert_same(spp.ravel(), n, "counts")
    assert_same(mom.reshape(-1, 2)[:, 0], s1, "S1")
    assert_same(mom.reshape(-1, 2)[:, 1], s2, "S2")
    assert len(np.unique(spp)) >= 2
    for level in np.unique(spp):
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = int(level)
        sel = spp == level
        assert_same(fb[sel], tr.frame(host, c, **kw)[sel], f"sums at {level} samples")


def test_cli_refusals(test_config_text, tmp_path):
    before = sorted(os.listdir(tmp_path))

    def run(args):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    for args, word in ((["--noise-target", "0.3"], "--noise-target"), (["--nee", "--noise-target", "0.3"], "--noise-target"),
                       (["--lit", "--noise-target", "0.3", "--adaptive", "0.1"], "--noise-target"),
                       (["--lit", "--noise-target", "0.3", "--denoise"], "--noise-target"), (["--lit", "--noise-target", "0.3", "--aov"], "--noise-target"),
                       (["--lit", "--noise-target", "x"], "--noise-target"), (["--lit", "--noise-target", "-0.1"], "--noise-target"),
                       (["--lit", "--noise-target", "nan"], "--noise-target"), (["--lit", "--noise-target", "inf"], "--noise-target"),
                       (["--lit", "--noise-target"], "--noise-target"), (["--lit", "--noise-target", "0.3", "--noise-spp", "4x4x32"], "--noise-spp"),
                       (["--lit", "--noise-target", "0.3", "--noise-spp", "4:4"], "--noise-spp"),
                       (["--lit", "--noise-target", "0.3", "--noise-spp", "1:4:32"], "--noise-spp"),
                       (["--lit", "--noise-target", "0.3", "--noise-spp", "4:0:32"], "--noise-spp"),
                       (["--lit", "--noise-target", "0.3", "--noise-spp", "8:4:4"], "--noise-spp"),
                       (["--lit", "--noise-target", "0.3", "--noise-spp", "4:4:70000"], "--noise-spp"),
                       (["--lit", "--noise-target", "0.3", "--noise-spp", "4:4:32x"], "--noise-spp"),
                       (["--lit", "--noise-spp", "4:4:32"], "--noise-spp"), (["--noise-spp", "4:4:32"], "--noise-spp")):
        r = run(args)
        assert r.returncode == 99 and word in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    r = run(["--lit", "--adaptive", "0.1"])
    assert r.returncode == 99 and "--lit" in r.stderr and "--noise" not in r.stderr, (r.returncode, r.stderr)


# ---- quality, on the reference: what the rule buys at equal samples ---------------------------------------------------------------
# MSE of the per-pixel mean clamped to [0, 1] (§11's metric), adaptive over uniform rt_render_lit at the rounded mean spp; 48 x 32,
# min 8, batch 8, max 128.  Deterministic (the restatement's bits): pinned at relative 1e-4, and recorded in DESIGN.md §19.
QUALITY_SPP = dict(min_spp=8, batch_spp=8, max_spp=128)
QUALITY_RATIOS = {("a", 0.05): 0.821978, ("a", 0.2): 0.946892, ("b", 0.05): 1.350935, ("b", 0.2): 1.083142}


@functools.lru_cache(maxsize=None)
def _quality_inputs(setting):
    name = lar.SETTINGS[setting][0]
    host, kw = tl.scene(name), lar.reference_keywords(setting)
    halves = [tr.frame(host, tl.camera(name, 48, 32, 4096), sample_first=first, **kw).astype(np.float64) / 4096 for first in (1 << 20, 1 << 21)]
    truth = np.clip((halves[0] + halves[1]) / 2, 0, 1)
    truth_var = float(np.mean((np.clip(halves[0], 0, 1) - np.clip(halves[1], 0, 1)) ** 2)) / 4
    rad = lar.radiances(host, tl.camera(name, 48, 32, 1), QUALITY_SPP["max_spp"], **kw)
    return truth, truth_var, rad


def _mse(fb, spp, truth):
    return float(np.mean((np.clip(fb.astype(np.float64) / np.asarray(spp, np.float64)[..., None], 0, 1) - truth) ** 2))


@pytest.mark.parametrize("setting,t", list(QUALITY_RATIOS))
def test_quality_against_uniform_at_the_same_sample_count(setting, t):
    name = lar.SETTINGS[setting][0]
    truth, truth_var, rad = _quality_inputs(setting)
    fb, spp, _ = lar.from_radiances(rad, threshold=t, **QUALITY_SPP)
    mean_spp = float(spp.mean())
    uniform_n = max(1, int(round(mean_spp)))
    ufb = tr.frame(tl.scene(name), tl.camera(name, 48, 32, uniform_n), **lar.reference_keywords(setting))
    adaptive, uniform = _mse(fb, spp, truth), _mse(ufb, np.full(spp.shape, uniform_n), truth)
    ratio = adaptive / uniform
    print(f"quality {name} t={t}: adaptive MSE {adaptive:.6g} at {mean_spp:.2f} spp mean ({np.unique(spp).size} levels), uniform {uniform:.6g} at "
          f"{uniform_n} spp, ratio {ratio:.6f}; the truth's own variance {truth_var:.3g} = {100 * truth_var / min(adaptive, uniform):.2f} % of the smaller")
    assert truth_var < 0.05 * min(adaptive, uniform), "the ratio would measure the truth"
    want = QUALITY_RATIOS[(setting, t)]
    assert abs(ratio - want) <= 1e-4 * want, ratio


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _scene_cam(setting, size=SIZE):
    name = lar.SETTINGS[setting][0]
    return tl.scene(name), tl.camera(name, size[0], size[1], 1)


def _check_triple(got, want, what):
    for g, w, col in zip(got[:3], want, ("fb", "spp", "moments")):
        assert_same(g, w, f"{what}: {col}")


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(lar.SETTINGS))
def test_equals_the_reference(setting):
    """fb, spp and moments byte for byte: the whole frame and a row shard, sample_first 0 and 37, on the default handle, a
    TRAVERSAL_EXACT one and one whose min_spp frame takes two passes (pass_spp = 3: the moments cross a pass boundary)."""
    rb.amd_lib().rt_set_device(0)
    host, cam = _scene_cam(setting)
    shard = rb.Shard(4, 3, 2)
    with rb.Env(lar.sky()) as env:
        kw = lar.device_keywords(setting, env)
        for config in (dict(), dict(traversal=rb.TRAVERSAL_EXACT), dict(pass_spp=3)):
            dev = rb.DeviceScene(host, device=0, **config)
            for first in (0, 37):
                for sh in (None, shard):
                    got = dev.render_lit_adaptive_to_host(cam, shard=sh, sample_first=first, threshold=THRESHOLD, **SPP, **kw)
                    _check_triple(got, lar.setting_reference(setting, first, sh), f"{setting} {config} first={first} shard={sh is not None}")
                    t = got[3]
                    assert t.trace_launches == (2 if config.get("pass_spp") else 1) + 7 and t.guarded == 0 and t.trace_scratch_bytes == 0
                    assert t.traced_samples == got[1].size * SPP["min_spp"] and t.kernel_ms > 0
            dev.close()


@pytest.mark.gpu
def test_per_pixel_parity_device_against_device():
    rb.amd_lib().rt_set_device(0)
    host, cam = _scene_cam("a", (64, 48))
    kw = lar.device_keywords("a", None)
    spp_kw = dict(min_spp=4, batch_spp=4, max_spp=64)
    dev = rb.DeviceScene(host, device=0)
    for t in (0.1, 0.05, 0.2, 0.03, 0.3, 0.02, 0.5):          # (test_adaptive._levels_threshold's candidates)
        fb, spp, _, _ = dev.render_lit_adaptive_to_host(cam, threshold=t, **spp_kw, **kw)
        if len(np.unique(spp)) >= 3:
            break
    levels = np.unique(spp)
    assert len(levels) >= 3 and ((levels - 4) % 4 == 0).all() and levels.min() >= 4 and levels.max() <= 64, levels
    covered = np.zeros(spp.shape, bool)
    for n in levels:
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = int(n)
        want, _ = dev.render_lit_to_host(c, **kw)
        sel = spp == n
        assert_same(fb[sel], want[sel], f"pixels with {n} samples")
        covered |= sel
    assert covered.all()
    dev.close()


@pytest.mark.gpu
def test_waves_refill_from_a_list():
    """One round of 32 samples of every pixel: more work than one chunk per resident wave, so some wave fetches a second chunk."""
    rb.amd_lib().rt_set_device(0)
    w, h = 192, 128
    host, cam = _scene_cam("a", (w, h))
    kw = lar.device_keywords("a", None)
    dev = rb.DeviceScene(host, device=0)
    fb, spp, _, t = dev.render_lit_adaptive_to_host(cam, min_spp=4, batch_spp=32, max_spp=36, threshold=0.0, **kw)
    print(f"waves that refill: {t.num_workgroups} workgroups x {LIGHT_BLOCK // 64} waves x {LIGHT_CHUNK} = "
          f"{t.num_workgroups * (LIGHT_BLOCK // 64) * LIGHT_CHUNK} against {w * h * 32} work indices")
    assert t.num_workgroups * (LIGHT_BLOCK // 64) * LIGHT_CHUNK < w * h * 32, "no wave needs a second chunk: enlarge the image"
    assert (spp == 36).all() and t.trace_launches == 2
    c = rb.CameraData.from_buffer_copy(cam)
    c.samples_per_pixel = 36
    assert_same(fb, dev.render_lit_to_host(c, **kw)[0], "threshold 0 = rt_render_lit at 36 samples")
    dev.close()


@pytest.mark.gpu
def test_edges():
    import torch
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    host, cam = _scene_cam("a")
    kw = lar.device_keywords("a", None)
    dev = rb.DeviceScene(host, device=0)

    def uniform(n, first=0):
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = int(n)
        return dev.render_lit_to_host(c, sample_first=first, **kw)[0]
    # seven empty rounds terminate, and nothing is added
    fb, spp, mom, t = dev.render_lit_adaptive_to_host(cam, threshold=1e30, **SPP, **kw)
    assert (spp == 4).all() and t.trace_launches == 8
    assert_same(fb, uniform(4), "huge threshold = rt_render_lit at min_spp")
    _check_triple((fb, spp, mom), lar.setting_reference("a", threshold=1e30), "huge threshold")
    # min == max: no round
    same = dev.render_lit_adaptive_to_host(cam, min_spp=4, batch_spp=4, max_spp=4, threshold=THRESHOLD, **kw)
    _check_triple(same, (fb, spp, mom), "min == max")
    assert same[3].trace_launches == 1
    # threshold 0: rt_render_lit at min + R * batch, from sample 5
    fb0, spp0, _, _ = dev.render_lit_adaptive_to_host(cam, min_spp=4, batch_spp=5, max_spp=32, threshold=0.0, sample_first=5, **kw)
    assert (spp0 == 29).all()
    assert_same(fb0, uniform(29, 5), "threshold 0, cap not reached")
    # (max - min) no multiple of batch
    got = dev.render_lit_adaptive_to_host(cam, min_spp=4, batch_spp=7, max_spp=32, threshold=THRESHOLD, **kw)
    want = lar.setting_reference("a", batch_spp=7)
    assert np.unique(want[1]).tolist() == [4, 11, 18, 25, 32]
    _check_triple(got, want, "batch 7")
    # d_moments = NULL
    want = lar.setting_reference("a")
    d_fb = torch.full((SIZE[1], SIZE[0], 3), float("nan"), device="cuda:0")
    d_spp = torch.full((SIZE[1], SIZE[0]), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dev.render_lit_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), None, threshold=THRESHOLD, **SPP, **kw)
    assert_same(d_fb.cpu().numpy(), want[0], "null moments: fb")
    assert_same(d_spp.cpu().numpy(), want[1], "null moments: spp")
    # max_depth <= 0: zero sums and moments, counts by the rule
    flat = tl.camera("night rtiow", *SIZE, 1, 0)
    fbz, sppz, momz, _ = dev.render_lit_adaptive_to_host(flat, threshold=THRESHOLD, **SPP, **kw)
    assert not fbz.any() and not momz.any() and (sppz == 4).all()
    assert (dev.render_lit_adaptive_to_host(flat, threshold=0.0, **SPP, **kw)[1] == 32).all()
    # pixels x batch_spp beyond the work index arithmetic: refused with a scene, before anything is enqueued (2^24 pixels x 128)
    big = tl.camera("night rtiow", 16384, 1024, 1)
    p = rb.adaptive_params(min_spp=4, batch_spp=128, max_spp=132, threshold=0.1)
    lit = rb.lit_params()
    st = lib.rt_render_lit_adaptive(dev._h, C.byref(big), C.byref(lit), C.byref(p), None, 0, C.c_void_p(FAKE), C.c_void_p(2 * FAKE), None, None, 1, None)
    assert st == UNSUPPORTED and "batch_spp" in lib.rt_get_last_error_string().decode()
    dev.close()


@pytest.mark.gpu
def test_identity_with_rt_render_adaptive():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(48, 27, 1, 50)
    dev = rb.DeviceScene(host, device=0)
    params = dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1)
    want = dev.render_adaptive_to_host(cam, **params)
    assert len(np.unique(want[1])) >= 3
    _check_triple(dev.render_lit_adaptive_to_host(cam, emitters=False, **params), want[:3], "emitters off, no map, no lens")
    dev.close()
    host.close()


@pytest.mark.gpu
def test_handle_state():
    import torch
    rb.amd_lib().rt_set_device(0)
    host, cam = _scene_cam("b")
    cam4 = rb.CameraData.from_buffer_copy(cam)
    cam4.samples_per_pixel = 4
    fresh = {}
    for setting in ("b", "c"):
        dev = rb.DeviceScene(host, device=0)
        fresh[setting] = dev.render_lit_adaptive_to_host(cam, threshold=THRESHOLD, **SPP, **lar.device_keywords(setting, None))[:3]
        dev.close()
    dev = rb.DeviceScene(host, device=0)
    want_render = dev.render_to_host(cam4)[0]
    want_adaptive = dev.render_adaptive_to_host(cam, threshold=THRESHOLD, **SPP)[:3]
    want_lit = dev.render_lit_to_host(cam4, **lar.device_keywords("b", None))[0]
    dev.close()
    dev = rb.DeviceScene(host, device=0)
    dev.render_to_host(cam4)
    before = dev.last_timing()
    for setting in ("b", "c", "b"):
        got = dev.render_lit_adaptive_to_host(cam, threshold=THRESHOLD, **SPP, **lar.device_keywords(setting, None))
        _check_triple(got, fresh[setting], f"{setting} on one handle")
    assert not np.array_equal(fresh["b"][0], fresh["c"][0])
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    assert_same(dev.render_to_host(cam4)[0], want_render, "rt_render after the call")
    _check_triple(dev.render_adaptive_to_host(cam, threshold=THRESHOLD, **SPP), want_adaptive, "rt_render_adaptive after the call")
    assert_same(dev.render_lit_to_host(cam4, **lar.device_keywords("b", None))[0], want_lit, "rt_render_lit after the call")
    # sync = 0 on a side stream
    s = torch.cuda.Stream()
    d_fb = torch.full((SIZE[1], SIZE[0], 3), float("nan"), device="cuda:0")
    d_spp = torch.full((SIZE[1], SIZE[0]), -1, dtype=torch.int32, device="cuda:0")
    d_mom = torch.full((SIZE[1], SIZE[0], 2), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dev.render_lit_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), d_mom.data_ptr(), stream=s.cuda_stream, sync=False, threshold=THRESHOLD, **SPP,
                                **lar.device_keywords("b", None))
    s.synchronize()
    _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), fresh["b"], "sync = 0 on a side stream")
    dev.close()


@pytest.mark.gpu
def test_cli_noise_target_frames_are_the_python_path(test_config_text, tmp_path):
    import torch
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera(0)
    out = subprocess.run([EXE, "--gpu", "--lit", "--nee", "--light-tree", "--noise-target", "0.3", "--noise-spp", "4:4:32"], input=text,
                         capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    fb, spp, _, _ = dev.render_lit_adaptive_to_host(host.frame_camera_at(0.0), nee=dict(select=1), threshold=0.3, **SPP)
    assert len(np.unique(spp)) >= 2
    d_fb, d_spp = torch.from_numpy(fb).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
    rgb = torch.zeros(fb.shape, dtype=torch.uint8, device="cuda:0")
    assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == OK
    torch.cuda.synchronize()
    want = np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes()
    assert open(tmp_path / "f_0.png", "rb").read() == want
    assert int(out.stdout.split("\n")[0].split("\t")[2]) == int(spp.sum())
    dev.close()
