"""rt_render_volume_adaptive (include/rtp_amd.h, "adaptive sampling under fog"): rt_render_lit_adaptive_prior's rule, rounds
and prior on rt_render_volume's estimator.  The reference is tests/volume_adaptive_reference.py, a composition of the restatements the
project already has; the CPU tests check the ABI, the refusals and the condition on the GPU tests' inputs, the GPU tests the sixteen list
kernels and the call against the reference and against the calls it is made of, byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lit_adaptive_reference as lar
import rtp_bindings as rb
import volume_adaptive_reference as var
from test_lit import assert_same
from test_medium import FAR_BALL, dev_kw, ref_kw, scenes
from test_volume import BOX, GRIDS, random_grid

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
FAKE = 1 << 32          # a device address that is never dereferenced
OK, INVALID, UNSUPPORTED = 0, 1, 4
SPP, LEVELS, SIZE = var.SPP, var.LEVELS, var.SIZE
LIGHT_BLOCK, LIGHT_CHUNK = 256, 128          # rt_light.hip.inc: kLightBlock, kLightChunk
NAME = "rt_render_volume_adaptive"


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_symbol_argtypes_and_methods():
    lib = rb.amd_lib()
    assert hasattr(lib, NAME) and NAME in rb.RTP_AMD_SYMBOLS
    assert len(lib.rt_render_volume_adaptive.argtypes) == 16
    for name in ("render_volume_adaptive", "render_volume_adaptive_to_host"):
        assert hasattr(rb.DeviceScene, name)
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        header = f.read()
    assert "rt_status rt_render_volume_adaptive(" in header
    assert "~~rt_render_lit_adaptive with a\n *   medium~~" in header and "~~rt_render_lit_adaptive with a grid~~" in header


def _params(**kw):
    return rb.adaptive_params(**{**dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1), **kw})


BOX_MEDIUM = dict(sigma_t=1.0, box=(0, 0, 0, 1, 1, 1))


def _call(params="default", lit="default", medium="default", volume=None, stop=None, prior=None, scene=None, cam="default", fb=FAKE, spp=2 * FAKE,
          mom=None, sample_first=0):
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    if params == "default":
        params = _params()
    if lit == "default":
        lit = rb.lit_params()
    if medium == "default":
        medium = rb.medium_params(**BOX_MEDIUM)
    if cam == "default":
        cam = rb.make_camera(8, 4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    st = lib.rt_render_volume_adaptive(scene, C.byref(cam) if cam is not None else None, C.byref(lit) if lit is not None else None,
                                       C.byref(medium) if medium is not None else None, volume, C.byref(params) if params is not None else None,
                                       C.byref(stop) if stop is not None else None, C.c_void_p(prior), None, sample_first, C.c_void_p(fb),
                                       C.c_void_p(spp), C.c_void_p(mom), None, 1, None)
    return st, lib.rt_get_last_error_string().decode()


def test_refusals_and_their_order():
    """Every refusal that needs no scene, with its code and a word of its message, and the order: adaptive parameters, stop parameters, the
    prior, lit parameters, the medium, the volume, the sample range, the buffers, the scene.  The volume's handle is never read."""
    handle = C.c_void_p(FAKE)
    nan, inf = float("nan"), float("inf")
    # 1. rt_render_adaptive's parameter checks
    assert _call(params=None)[0] == INVALID
    short = _params()
    short.struct_bytes = 4
    assert _call(params=short)[0] == INVALID
    for kw, code, word in ((dict(min_spp=1), INVALID, "min_spp"), (dict(batch_spp=0), INVALID, "batch_spp"), (dict(max_spp=3), INVALID, "max_spp"),
                           (dict(threshold=-0.01), INVALID, "threshold"), (dict(threshold=nan), INVALID, "threshold"),
                           (dict(threshold=inf), INVALID, "threshold"), (dict(max_spp=65537), UNSUPPORTED, "65536")):
        st, msg = _call(params=_params(**kw))
        assert st == code and word in msg and NAME in msg, (kw, st, msg)
    # 2. the stop parameters
    bad_stop = rb.stop_params(rule=2)
    st, msg = _call(stop=bad_stop)
    assert st == INVALID and "rule" in msg and NAME in msg and "_rule" not in msg, msg
    short_stop = rb.stop_params()
    short_stop.struct_bytes = 4
    st, msg = _call(stop=short_stop)
    assert st == INVALID and "struct_bytes" in msg and NAME in msg, msg
    for rule in (0, 1):
        assert "null scene" in _call(stop=rb.stop_params(rule=rule))[1]
    # 3. the prior: it shares no byte with an output
    for kw in (dict(prior=FAKE), dict(prior=2 * FAKE), dict(prior=3 * FAKE, mom=3 * FAKE), dict(prior=FAKE + 8 * 4 * 12 - 8)):
        st, msg = _call(**kw)
        assert st == INVALID and "overlaps" in msg and NAME in msg, (kw, msg)
    assert "null scene" in _call(prior=FAKE + 8 * 4 * 12)[1]
    # 4. rt_render_lit's
    bad_lens, bad_nee = dict(lens_radius=-1.0), dict(mis=3)
    for lit, word in ((rb.lit_params(lens=bad_lens, nee=bad_nee), "lens_radius"), (rb.lit_params(nee=bad_nee), "mis"),
                      (rb.lit_params(nee=dict(select=2)), "select"), (rb.lit_params(emitters=2), "sample_emitters")):
        st, msg = _call(lit=lit)
        assert st == INVALID and word in msg and NAME in msg, (word, st, msg)
    assert "null scene" in _call(lit=None)[1], "lit NULL means the defaults"
    assert _call(cam=None)[0] == INVALID
    # 5. the medium's
    short_medium = rb.medium_params(**BOX_MEDIUM)
    short_medium.struct_bytes = 4
    for medium, word in ((short_medium, "struct_bytes"), (rb.medium_params(sigma_t=-0.5), "sigma_t"), (rb.medium_params(sigma_t=nan), "sigma_t"),
                         (rb.medium_params(sigma_t=1.0, albedo=(0.5, 1.5, 0.5)), "albedo"), (rb.medium_params(sigma_t=1.0, g=0.96), "|g|"),
                         (rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, -1)), "radius"), (rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, -1, 1)), "lo < hi")):
        for volume in (None, handle):
            st, msg = _call(medium=medium, volume=volume)
            assert st == INVALID and word in msg and NAME in msg, (word, st, msg)
    # 6. the volume's: a medium with region 2, or no volume
    for medium in (None, rb.medium_params(sigma_t=1.0), rb.medium_params(sigma_t=0.0), rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1))):
        st, msg = _call(medium=medium, volume=handle)
        assert st == INVALID and "region 2" in msg and NAME in msg, msg
    # 7. the sample range: sample_first + min_spp + R * batch_spp (here 4 + 15 * 4 = 64)
    st, msg = _call(sample_first=-1)
    assert st == INVALID and "sample_first" in msg and NAME in msg, msg
    assert "null scene" in _call(sample_first=(1 << 30) - 64)[1]
    st, msg = _call(sample_first=(1 << 30) - 63)
    assert st == UNSUPPORTED and "2^30" in msg, msg
    assert "null scene" in _call(params=_params(max_spp=67), sample_first=(1 << 30) - 64)[1], "R * batch, not max_spp, counts"
    # 8. the buffers
    for kw in (dict(fb=0), dict(spp=0)):
        st, msg = _call(**kw)
        assert st == INVALID and "null framebuffer or sample counts" in msg and NAME in msg, (kw, msg)
    # 9. the scene: what passes reaches it, under this call's name — without a medium as well (the lit call takes over after the checks)
    for medium, volume in ((rb.medium_params(**BOX_MEDIUM), None), (rb.medium_params(**BOX_MEDIUM), handle), (None, None),
                           (rb.medium_params(sigma_t=0.0, box=(0, 0, 0, 1, 1, 1)), handle), (rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), None)):
        st, msg = _call(medium=medium, volume=volume)
        assert st == INVALID and "null scene" in msg and NAME in msg, msg
    # the order, each refusal with everything after it wrong as well
    wrong = dict(stop=bad_stop, prior=2 * FAKE, lit=rb.lit_params(lens=bad_lens), medium=rb.medium_params(sigma_t=-1.0), volume=handle, sample_first=-1, fb=0)
    words = ["min_spp", "rule", "overlaps", "lens_radius", "sigma_t", "region 2", "sample_first", "null framebuffer", "null scene"]
    assert words[0] in _call(params=_params(min_spp=1), **wrong)[1]
    assert words[1] in _call(**wrong)[1]
    del wrong["stop"]
    assert words[2] in _call(**wrong)[1]
    del wrong["prior"]
    assert words[3] in _call(**wrong)[1]
    del wrong["lit"]
    assert words[4] in _call(**wrong)[1]
    wrong["medium"] = rb.medium_params(sigma_t=1.0)
    assert words[5] in _call(**wrong)[1]
    del wrong["medium"]
    assert words[6] in _call(**wrong)[1]
    del wrong["sample_first"]
    assert words[7] in _call(**wrong)[1]
    del wrong["fb"]
    assert words[8] in _call(**wrong)[1]


def test_cli_refusals(test_config_text, tmp_path):
    """--fog-noise-target needs --fog, takes T[:min:batch:max], and is refused with --adaptive, --denoise*, --aov, --stop-rule,
    --stop-history and --noise-target: exit code 99 and a message that names the flag, nothing written.  The old refusal of --fog with
    --noise-target stays and points to the new flag."""
    before = sorted(os.listdir(tmp_path))
    fog = ["--lit", "--fog", "0.5"]
    target = ["--fog-noise-target", "0.3"]

    def run(args):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    cases = [["--lit"] + target, target, ["--fog-noise-target"] + fog]
    cases += [fog + ["--fog-noise-target", bad] for bad in ("x", "-0.1", "nan", "inf", "0.3:4:4", "0.3:1:4:32", "0.3:4:0:32", "0.3:8:4:4", "0.3:4:4:70000",
                                                             "0.3:4:4:32x", "0.3x", "")]
    cases += [fog + target + other for other in (["--adaptive", "0.1"], ["--denoise"], ["--denoise-temporal"], ["--denoise-adaptive"],
                                                 ["--denoise-adaptive-temporal"], ["--aov"], ["--stop-rule", "near"], ["--stop-history"],
                                                 ["--noise-target", "0.3"])]
    for args in cases:
        r = run(args)
        assert r.returncode == 99 and "--fog-noise-target" in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    for other in (["--adaptive", "0.1"], ["--aov"], ["--stop-rule", "near"]):
        r = run(fog + target + other)
        assert other[0] in r.stderr, (other, r.stderr)
    r = run(fog + ["--noise-target", "0.3"])
    assert r.returncode == 99 and "--noise-target" in r.stderr and "--fog-noise-target" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("setting", list(var.SETTINGS))
def test_levels_are_populated_and_fog_is_in_them(setting):
    """The condition on the inputs of the GPU tests, on the restatement: at least 5 pixels stop at min_spp, at least 5 reach max_spp, at least
    5 stop at each of at least three levels in between, and at least 10 pixels that stop above min_spp have a medium event among their
    samples — the comparison cannot pass with nothing adaptive, or nothing fogged, in it."""
    _, spp, _ = var.setting_reference(setting)
    events = var.setting_radiances(setting)[1]
    counts = [int((spp == n).sum()) for n in LEVELS]
    taken = np.arange(events.shape[2])[None, None, :] < spp[..., None]
    fogged = int((((events > 0) & taken).any(axis=2) & (spp > SPP["min_spp"])).sum())
    print(f"setting {setting} t={var.THRESHOLDS[setting]}: pixels per level {dict(zip(LEVELS, counts))}, smallest {min(counts)}; "
          f"pixels above min_spp with a medium event: {fogged}")
    assert sum(counts) == spp.size
    assert counts[0] >= 5 and counts[-1] >= 5, counts
    assert sum(c >= 5 for c in counts[1:-1]) >= 3, counts
    assert fogged >= 10, fogged


def test_helper_with_the_fog_off_is_the_lit_reference():
    host, cam = var.scene_cam("b")
    kw = dict(select=1, planes=1)
    want = lar.reference(host, cam, threshold=0.2, **SPP, **kw)
    assert len(np.unique(want[1])) >= 3
    for medium in (None, dict(sigma_t=0.0, box=BOX)):
        got = var.reference(host, cam, medium=medium, threshold=0.2, **SPP, **kw)
        for g, w, col in zip(got, want, ("fb", "spp", "moments")):
            assert_same(g, w, f"fog off ({medium}): {col}")


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _check_triple(got, want, what):
    for g, w, col in zip(got[:3], want[:3], ("fb", "spp", "moments")):
        assert_same(g, w, f"{what}: {col}")


def _volume(setting):
    d = var.density_of(setting)
    return rb.Volume(d) if d is not None else None


def _close(volume):
    if volume is not None:
        volume.close()


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(var.SETTINGS))
def test_equals_the_reference(setting):
    """fb, spp and moments byte for byte: the whole frame and a row shard, sample_first 0 and 37, on the default handle and on one whose
    min_spp frame takes two passes (pass_spp = 3: the moments cross a pass boundary)."""
    rb.amd_lib().rt_set_device(0)
    host, cam = var.scene_cam(setting)
    shard = rb.Shard(4, 3, 2)
    vol = _volume(setting)
    with rb.Env(lar.sky()) as env:
        kw = var.device_keywords(setting, env, vol)
        for config in (dict(), dict(pass_spp=3)):
            dev = rb.DeviceScene(host, device=0, **config)
            for first in (0, 37):
                for sh in (None, shard):
                    got = dev.render_volume_adaptive_to_host(cam, shard=sh, sample_first=first, threshold=var.THRESHOLDS[setting], **SPP, **kw)
                    _check_triple(got, var.setting_reference(setting, first, sh), f"{setting} {config} first={first} shard={sh is not None}")
                    t = got[3]
                    assert t.trace_launches == (2 if config.get("pass_spp") else 1) + 7 and t.guarded == 0
                    assert t.traced_samples == got[1].size * SPP["min_spp"] and t.kernel_ms > 0
            dev.close()
    _close(vol)


@pytest.mark.gpu
def test_rule_and_prior_equal_their_references():
    """rule = 1 in (a) and a non-zero prior in (b) (rule 0 and rule 1), the whole frame and a row shard."""
    rb.amd_lib().rt_set_device(0)
    shard = rb.Shard(4, 3, 2)
    for setting, cases in (("a", [dict(rule=1)]), ("b", [dict(prior=True), dict(prior=True, rule=1)])):
        host, cam = var.scene_cam(setting)
        vol = _volume(setting)
        dev = rb.DeviceScene(host, device=0)
        kw = var.device_keywords(setting, None, vol)
        plain = var.setting_reference(setting)
        for case in cases:
            for sh in (None, shard):
                rows = rb.amd_lib().rt_shard_rows(cam.image_height, C.byref(sh) if sh else None)
                more = {k: v for k, v in case.items() if k == "rule"}
                if case.get("prior"):
                    more["prior"] = var.prior_of(rows, cam.image_width)
                got = dev.render_volume_adaptive_to_host(cam, shard=sh, threshold=var.THRESHOLDS[setting], **SPP, **more, **kw)
                want = var.setting_reference(setting, shard=sh, **more)
                _check_triple(got, want, f"{setting} {case} shard={sh is not None}")
                if sh is None:
                    assert not np.array_equal(want[1], plain[1]), f"{case}: the counts are those without it"
        dev.close()
        _close(vol)


@pytest.mark.gpu
def test_per_pixel_parity_device_against_device():
    """64 x 48: each pixel equals rt_render_volume at its own count, for every level."""
    rb.amd_lib().rt_set_device(0)
    host, cam = var.scene_cam("a", (64, 48))
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(var.density_of("a")) as vol:
        kw = var.device_keywords("a", None, vol)
        fb, spp, _, _ = dev.render_volume_adaptive_to_host(cam, threshold=var.THRESHOLDS["a"], **SPP, **kw)
        assert np.unique(spp).tolist() == LEVELS
        for n in LEVELS:
            c = rb.CameraData.from_buffer_copy(cam)
            c.samples_per_pixel = n
            want, _ = dev.render_volume_to_host(c, **kw)
            sel = spp == n
            assert_same(fb[sel], want[sel], f"pixels with {n} samples")
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [True, False])
def test_waves_refill_from_a_list(grid):
    """192 x 128, one round of 32 samples of every pixel: more work indices than one chunk per wave of the grid, so waves refill from the
    list; the frame is rt_render_volume's at 36 samples."""
    rb.amd_lib().rt_set_device(0)
    w, h = 192, 128
    host, cam = var.scene_cam("a", (w, h))
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(var.density_of("a")) as vol:
        kw = var.device_keywords("a", None, vol if grid else None)
        fb, spp, _, t = dev.render_volume_adaptive_to_host(cam, min_spp=4, batch_spp=32, max_spp=36, threshold=0.0, **kw)
        print(f"waves that refill: {t.num_workgroups} workgroups x {LIGHT_BLOCK // 64} waves x {LIGHT_CHUNK} = "
              f"{t.num_workgroups * (LIGHT_BLOCK // 64) * LIGHT_CHUNK} against {w * h * 32} work indices")
        assert t.num_workgroups * (LIGHT_BLOCK // 64) * LIGHT_CHUNK < w * h * 32, "no wave needs a second chunk: enlarge the image"
        assert (spp == 36).all() and t.trace_launches == 2
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = 36
        assert_same(fb, dev.render_volume_to_host(c, **kw)[0], "threshold 0 = rt_render_volume at 36 samples")
    dev.close()


@pytest.mark.gpu
def test_identities():
    """Section by section of the header's identities, bit for bit in all three outputs, each through the kernels named there."""
    rb.amd_lib().rt_set_device(0)
    setting = "b"
    host, cam = var.scene_cam(setting)
    t = var.THRESHOLDS[setting]
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(var.density_of(setting)) as vol, rb.Volume(np.ones((1, 1, 1), np.float32)) as one, rb.Volume(np.zeros((5, 3, 2), np.float32)) as zero:
        kw = var.device_keywords(setting, None, vol)
        lit_kw = {k: v for k, v in kw.items() if k not in ("medium", "volume")}
        medium = kw["medium"]

        def uniform(n, first=0, **more):
            c = rb.CameraData.from_buffer_copy(cam)
            c.samples_per_pixel = int(n)
            return dev.render_volume_to_host(c, sample_first=first, **{**kw, **more})[0]
        # threshold 0: rt_render_volume at min + R * batch (here 4 + 5 * 5 = 29), from sample 5 — the grid's kernels, then the medium's
        for more in (dict(), dict(volume=None), dict(volume=None, medium=var.medium_of("d"))):
            fb0, spp0, mom0, _ = dev.render_volume_adaptive_to_host(cam, min_spp=4, batch_spp=5, max_spp=32, threshold=0.0, sample_first=5, **{**kw, **more})
            assert (spp0 == 29).all()
            assert_same(fb0, uniform(29, 5, **more), f"threshold 0 {list(more)}")
        assert_same(mom0, dev.render_volume_adaptive_to_host(cam, min_spp=29, batch_spp=1, max_spp=29, threshold=t, sample_first=5,
                                                             **{**kw, **more})[2], "threshold 0: the moments of 29 samples")
        # a 1 x 1 x 1 grid of density 1 (the grid's kernels) = no volume with the same box (the medium's kernels)
        hom = dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **{**kw, "volume": None})
        assert len(np.unique(hom[1])) >= 4
        _check_triple(dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **{**kw, "volume": one}), hom, "1^3 grid = the box")
        _check_triple(hom, var.reference(host, cam, medium=medium, threshold=t, **SPP, **var.SETTINGS[setting][3]), "the box = the reference")
        # no medium, or sigma_t = 0 (with and without a volume): rt_render_lit_adaptive_prior with the remaining arguments
        prior = var.prior_of(cam.image_height, cam.image_width)
        for more in (dict(), dict(rule=1), dict(prior=prior), dict(rule=1, prior=prior)):
            want = dev.render_lit_adaptive_to_host(cam, threshold=t, **SPP, **more, **lit_kw)
            assert len(np.unique(want[1])) >= 3
            for fog_off in (dict(medium=None, volume=None), dict(medium=dict(medium, sigma_t=0.0), volume=None), dict(medium=dict(medium, sigma_t=0.0), volume=vol)):
                _check_triple(dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **more, **lit_kw, **fog_off), want,
                              f"fog off {more.keys()} {fog_off['medium'] is None} {fog_off['volume'] is None}")
        # a grid of zeros (the grid's kernels) and a region no ray touches (the medium's): rt_render_lit_adaptive_prior's outputs
        want = dev.render_lit_adaptive_to_host(cam, threshold=t, **SPP, **lit_kw)
        _check_triple(dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **{**kw, "volume": zero}), want, "a grid of zeros")
        _check_triple(dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **{**kw, "volume": None, "medium": FAR_BALL}), want, "a far ball")
    dev.close()


@pytest.mark.gpu
def test_edges():
    import torch
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    setting = "a"
    host, cam = var.scene_cam(setting)
    t = var.THRESHOLDS[setting]
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(var.density_of(setting)) as vol:
        kw = var.device_keywords(setting, None, vol)
        # seven empty rounds terminate, and nothing is added
        fb, spp, mom, tm = dev.render_volume_adaptive_to_host(cam, threshold=1e30, **SPP, **kw)
        assert (spp == 4).all() and tm.trace_launches == 8
        _check_triple((fb, spp, mom), var.setting_reference(setting, threshold=1e30), "huge threshold")
        c4 = rb.CameraData.from_buffer_copy(cam)
        c4.samples_per_pixel = 4
        assert_same(fb, dev.render_volume_to_host(c4, **kw)[0], "huge threshold = rt_render_volume at min_spp")
        # min == max: no round
        same = dev.render_volume_adaptive_to_host(cam, min_spp=4, batch_spp=4, max_spp=4, threshold=t, **kw)
        _check_triple(same, (fb, spp, mom), "min == max")
        assert same[3].trace_launches == 1
        # (max - min) no multiple of batch
        got = dev.render_volume_adaptive_to_host(cam, min_spp=4, batch_spp=7, max_spp=32, threshold=t, **kw)
        want = var.setting_reference(setting, batch_spp=7)
        assert np.unique(want[1]).tolist() == [4, 11, 18, 25, 32]
        _check_triple(got, want, "batch 7")
        # d_moments = NULL
        want = var.setting_reference(setting)
        d_fb = torch.full((SIZE[1], SIZE[0], 3), float("nan"), device="cuda:0")
        d_spp = torch.full((SIZE[1], SIZE[0]), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        dev.render_volume_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), None, threshold=t, **SPP, **kw)
        assert_same(d_fb.cpu().numpy(), want[0], "null moments: fb")
        assert_same(d_spp.cpu().numpy(), want[1], "null moments: spp")
        # max_depth <= 0: zero sums and moments, counts by the rule
        flat = var.scene_cam(setting, depth=0)[1]
        fbz, sppz, momz, _ = dev.render_volume_adaptive_to_host(flat, threshold=t, **SPP, **kw)
        assert not fbz.any() and not momz.any() and (sppz == 4).all()
        assert (dev.render_volume_adaptive_to_host(flat, threshold=0.0, **SPP, **kw)[1] == 32).all()
        # pixels x batch_spp beyond the work index arithmetic: refused with a scene, before anything is enqueued (2^24 pixels x 128)
        big = var.scene_cam(setting, (16384, 1024))[1]
        p = rb.adaptive_params(min_spp=4, batch_spp=128, max_spp=132, threshold=0.1)
        lit, medium = rb.lit_params(), rb.medium_params(**var.medium_of(setting))
        st = lib.rt_render_volume_adaptive(dev._h, C.byref(big), C.byref(lit), C.byref(medium), vol._h, C.byref(p), None, None, None, 0, C.c_void_p(FAKE),
                                           C.c_void_p(2 * FAKE), None, None, 1, None)
        msg = lib.rt_get_last_error_string().decode()
        assert st == UNSUPPORTED and "batch_spp" in msg and NAME in msg, msg
    # a volume on the handle's device only
    if torch.cuda.device_count() > 1:
        lib.rt_set_device(1)
        other = rb.Volume(var.density_of(setting))
        lib.rt_set_device(0)
        with pytest.raises(rb.RtError, match="another device"):
            dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **var.device_keywords(setting, None, other))
        other.close()
    # a 256 x 1 x 1 grid
    density = random_grid((1, 1, 256), 41)
    with rb.Volume(density) as wide:
        got = dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **var.device_keywords(setting, None, wide))
        want = var.reference(host, cam, threshold=t, **SPP, **{**var.reference_keywords(setting), "density": density})
        assert len(np.unique(want[1])) >= 3
        _check_triple(got, want, "256 x 1 x 1")
    dev.close()


@pytest.mark.gpu
def test_each_of_the_sixteen_list_kernels():
    """A small frame through medium_list_render_kernel and volume_list_render_kernel under each of the four emitter tables, pinhole and
    lens (with motion): the scene with planes, select and sample_planes in {0, 1}^2."""
    rb.amd_lib().rt_set_device(0)
    scene = "fuzz planes"
    host, camera, _ = scenes()[scene]
    w, h = 24, 13
    params = dict(min_spp=2, batch_spp=2, max_spp=6, threshold=0.3)
    medium = dict(sigma_t=0.5, albedo=(0.95, 0.9, 0.8), g=0.3, box=BOX)
    dev = rb.DeviceScene(host, device=0)
    levels = set()
    with rb.Volume(GRIDS["2x3x5"]) as vol:
        for density, volume in ((None, None), (GRIDS["2x3x5"], vol)):
            for lens in (False, True):
                for select, planes in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    setting = "lens + motion" if lens else "mis"
                    cam = camera(w, h, 1, 12)
                    kw_r = {**ref_kw(scene, setting, w, h, 1, 12), "select": select, "planes": planes}
                    kw_d = dev_kw(scene, setting, None, w, h, 1, 12)
                    kw_d["nee"] = dict(select=select, sample_planes=planes)
                    want = var.reference(host, cam, medium=medium, density=density, **params, **kw_r)
                    got = dev.render_volume_adaptive_to_host(cam, medium=medium, volume=volume, **params, **kw_d)
                    _check_triple(got, want, f"grid={volume is not None} lens={lens} select={select} planes={planes}")
                    assert got[3].trace_scratch_bytes == 0
                    levels |= set(np.unique(want[1]).tolist())
    assert levels == {2, 4, 6}
    dev.close()


@pytest.mark.gpu
def test_handle_state():
    import torch
    rb.amd_lib().rt_set_device(0)
    host, cam = var.scene_cam("b")
    cam4 = rb.CameraData.from_buffer_copy(cam)
    cam4.samples_per_pixel = 4
    t = var.THRESHOLDS["b"]
    with rb.Volume(var.density_of("b")) as vol:
        settings = {"grid": var.device_keywords("b", None, vol), "ball": dict(medium=var.medium_of("d"), volume=None, nee=dict(mis=0))}
        lit_kw = dict(nee=dict(select=1, sample_planes=1))
        fresh = {}
        for name, kw in settings.items():
            dev = rb.DeviceScene(host, device=0)
            fresh[name] = dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **kw)[:3]
            dev.close()
        dev = rb.DeviceScene(host, device=0)
        want_render = dev.render_to_host(cam4)[0]
        want_adaptive = dev.render_lit_adaptive_to_host(cam, threshold=t, **SPP, **lit_kw)[:3]
        want_volume = dev.render_volume_to_host(cam4, **settings["grid"])[0]
        dev.close()
        dev = rb.DeviceScene(host, device=0)
        dev.render_to_host(cam4)
        before = dev.last_timing()
        for name in ("grid", "ball", "grid"):
            _check_triple(dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **settings[name]), fresh[name], f"{name} on one handle")
        assert not np.array_equal(fresh["grid"][0], fresh["ball"][0])
        assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
        assert_same(dev.render_to_host(cam4)[0], want_render, "rt_render after the call")
        _check_triple(dev.render_lit_adaptive_to_host(cam, threshold=t, **SPP, **lit_kw), want_adaptive, "rt_render_lit_adaptive after the call")
        assert_same(dev.render_volume_to_host(cam4, **settings["grid"])[0], want_volume, "rt_render_volume after the call")
        # sync = 0 on a side stream
        s = torch.cuda.Stream()
        d_fb = torch.full((SIZE[1], SIZE[0], 3), float("nan"), device="cuda:0")
        d_spp = torch.full((SIZE[1], SIZE[0]), -1, dtype=torch.int32, device="cuda:0")
        d_mom = torch.full((SIZE[1], SIZE[0], 2), float("nan"), device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            dev.render_volume_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), d_mom.data_ptr(), stream=s.cuda_stream, sync=False, threshold=t, **SPP,
                                       **settings["grid"])
        s.synchronize()
        _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), fresh["grid"], "sync = 0 on a side stream")
        dev.close()


@pytest.mark.gpu
def test_cli_fog_noise_target_frames_are_the_python_path(test_config_text, tmp_path):
    import torch
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera(0)
    density = GRIDS["2x3x5"]
    with open(tmp_path / "grid.vol", "wb") as f:
        f.write(b"VOL1\n2 3 5\n" + np.asarray(density, "<f4").tobytes())
    box = (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0)
    for grid in (True, False):
        args = ["--lit", "--nee", "--light-tree", "--fog", "0.4:0.9:0.3", "--fog-box", ",".join(str(x) for x in box), "--fog-noise-target", "0.3:4:4:32"]
        if grid:
            args += ["--fog-grid", str(tmp_path / "grid.vol")]
        out = subprocess.run([EXE, "--gpu", *args], input=text, capture_output=True, text=True, timeout=200)
        assert out.returncode == 0, out.stderr
        with rb.Volume(density) as vol:
            fb, spp, _, _ = dev.render_volume_adaptive_to_host(host.frame_camera_at(0.0), nee=dict(select=1), threshold=0.3, **SPP,
                                                               medium=dict(sigma_t=0.4, albedo=0.9, g=0.3, box=box), volume=vol if grid else None)
        assert len(np.unique(spp)) >= 2
        d_fb, d_spp = torch.from_numpy(fb).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
        rgb = torch.zeros(fb.shape, dtype=torch.uint8, device="cuda:0")
        assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == OK
        torch.cuda.synchronize()
        want = np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes()
        assert open(tmp_path / "f_0.png", "rb").read() == want
        assert int(out.stdout.split("\n")[0].split("\t")[2]) == int(spp.sum())
    dev.close()
