"""rt_render_fog_adaptive (include/rtp_amd.h, "adaptive sampling on every fog rung"): rt_render_volume_adaptive's rule,
rounds and prior on the estimator of rt_render_chroma, rt_render_glow and rt_render_glow_sampled.  The reference is
tests/fog_adaptive_reference.py, a composition of the restatements the project already has; the CPU tests check the ABI, the refusals and
the condition on the GPU tests' inputs, the GPU tests the forty list kernels and the call against the reference and against the calls it is
made of, byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fog_adaptive_reference as far
import lit_adaptive_reference as lar
import rtp_bindings as rb
import volume_adaptive_reference as var
from test_chroma import TINTS, scaled
from test_glow import GLOWS, HEATS
from test_lit import assert_same
from test_medium import dev_kw, scenes
from test_volume import BOX, GRIDS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
FAKE = 1 << 32          # a device address that is never dereferenced
OK, INVALID, UNSUPPORTED = 0, 1, 4
SPP, LEVELS, SIZE = far.SPP, far.LEVELS, far.SIZE
LIGHT_BLOCK, LIGHT_CHUNK = 256, 128          # rt_light.hip.inc: kLightBlock, kLightChunk
NAME = "rt_render_fog_adaptive"
ONE_PER_RUNG = {"tint": "tint b", "glow": "glow a", "sampled": "sampled b"}


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_symbol_argtypes_and_methods():
    lib = rb.amd_lib()
    for s in (NAME, "rt_fog_params_init"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert len(lib.rt_render_fog_adaptive.argtypes) == 15
    for name in ("render_fog_adaptive", "render_fog_adaptive_to_host"):
        assert hasattr(rb.DeviceScene, name)
    assert C.sizeof(rb.FogParams) == 64
    assert [getattr(rb.FogParams, f).offset for f in ("struct_bytes", "medium", "volume", "chroma", "glow", "heat", "sample", "sampler")] == list(range(0, 64, 8))
    p = rb.fog_params()
    assert p.struct_bytes == 64 and not any((p.medium, p.volume, p.chroma, p.glow, p.heat, p.sample, p.sampler))
    q = rb.fog_params(medium=dict(sigma_t=0.5), tint=(1, 2, 3))
    assert q.medium.contents.sigma_t == 0.5 and list(q.chroma.contents.tint) == [1.0, 2.0, 3.0] and not q.glow
    g = rb.fog_params(glow=dict(radiance=2.0, source=1), sample="light")
    assert g.glow.contents.source == 1 and g.sample.contents.sample == 1 and g.sample.contents.mis == 0
    lib.rt_fog_params_init(None)
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        header = f.read()
    assert "rt_status rt_render_fog_adaptive(" in header and "~~the adaptive call with a tint~~" in header
    lib.rt_version_string.restype = C.c_char_p
    assert b"0.5" in lib.rt_version_string()


def _params(**kw):
    return rb.adaptive_params(**{**dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1), **kw})


BOX_MEDIUM = dict(sigma_t=1.0, box=(0, 0, 0, 1, 1, 1))


def _call(params="default", lit="default", fog="default", stop=None, prior=None, scene=None, cam="default", fb=FAKE, spp=2 * FAKE, mom=None, sample_first=0,
          **fog_kw):
    """(status, message) of the call; fog_kw: fog_params' keywords (medium defaults to a box of sigma_t 1; volume, heat and sampler may be
    integers that stand for handles)."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    if params == "default":
        params = _params()
    if lit == "default":
        lit = rb.lit_params()
    if fog == "default":
        handles = {k: fog_kw.pop(k) for k in ("volume", "heat", "sampler") if k in fog_kw}
        fog = rb.fog_params(**{"medium": rb.medium_params(**BOX_MEDIUM), **fog_kw})
        for k, v in handles.items():
            setattr(fog, k, v)
    if cam == "default":
        cam = rb.make_camera(8, 4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    st = lib.rt_render_fog_adaptive(scene, C.byref(cam) if cam is not None else None, C.byref(lit) if lit is not None else None,
                                    C.byref(fog) if fog is not None else None, C.byref(params) if params is not None else None,
                                    C.byref(stop) if stop is not None else None, C.c_void_p(prior), None, sample_first, C.c_void_p(fb), C.c_void_p(spp),
                                    C.c_void_p(mom), None, 1, None)
    return st, lib.rt_get_last_error_string().decode()


def _refused(word, code=INVALID, **kw):
    st, msg = _call(**kw)
    assert st == code and word in msg and NAME in msg, (word, kw, st, msg)


def test_refusals_and_their_order():
    """Every refusal that needs no scene, with its code and a word of its message, in the header's order: adaptive parameters, stop
    parameters, the prior, rt_fog_params itself, a tint together with a glow, fog_setup's layers at the rung the pointers ask for, the sample
    range, the buffers, the scene.  No handle is ever read."""
    nan, inf = float("nan"), float("inf")
    # 1. rt_render_adaptive's parameter checks
    assert _call(params=None)[0] == INVALID
    short = _params()
    short.struct_bytes = 4
    assert _call(params=short)[0] == INVALID
    for kw, code, word in ((dict(min_spp=1), INVALID, "min_spp"), (dict(batch_spp=0), INVALID, "batch_spp"), (dict(max_spp=3), INVALID, "max_spp"),
                           (dict(threshold=-0.01), INVALID, "threshold"), (dict(threshold=nan), INVALID, "threshold"),
                           (dict(threshold=inf), INVALID, "threshold"), (dict(max_spp=65537), UNSUPPORTED, "65536")):
        _refused(word, code, params=_params(**kw))
    # 2. the stop parameters
    bad_stop = rb.stop_params(rule=2)
    _refused("rule", stop=bad_stop)
    assert "_rule" not in _call(stop=bad_stop)[1]
    short_stop = rb.stop_params()
    short_stop.struct_bytes = 4
    _refused("struct_bytes", stop=short_stop)
    for rule in (0, 1):
        _refused("null scene", stop=rb.stop_params(rule=rule))
    # 3. the prior: it shares no byte with an output
    for kw in (dict(prior=FAKE), dict(prior=2 * FAKE), dict(prior=3 * FAKE, mom=3 * FAKE), dict(prior=FAKE + 8 * 4 * 12 - 8)):
        _refused("overlaps", **kw)
    _refused("null scene", prior=FAKE + 8 * 4 * 12)
    # 4. rt_fog_params itself; a shorter struct ends before its later fields
    _refused("rt_fog_params", fog=None)
    tiny = rb.fog_params()
    tiny.struct_bytes = 4
    _refused("rt_fog_params", fog=tiny)
    cut = rb.fog_params(medium=rb.medium_params(sigma_t=-1.0), tint=(nan, 1, 1))
    cut.struct_bytes = 16          # (struct_bytes and medium)
    _refused("sigma_t", fog=cut)
    cut.struct_bytes = 8
    _refused("null scene", fog=cut)
    # 5. a tint or a glow, not both: by the pointers alone (a grey tint, a dark glow, a sample that is off)
    _refused("a tint or a glow", tint=1.0, glow=0.0)
    _refused("a tint or a glow", tint=(1, 2, 3), glow=1.0, sample="mis")
    # (a sample beside a tint has no glow to aim at: the tint's call, and neither the sample nor the sampler is looked at)
    _refused("null scene", tint=(1, 2, 3), sample=dict(sample=2, mis=2), sampler=FAKE)
    _refused("tint", tint=(nan, 1, 1), sample="mis")
    # 6. fog_setup's layers: rt_render_lit's, the medium's, the volume's, then the rung's
    bad_lens, bad_nee = dict(lens_radius=-1.0), dict(mis=3)
    for lit, word in ((rb.lit_params(lens=bad_lens, nee=bad_nee), "lens_radius"), (rb.lit_params(nee=bad_nee), "mis"),
                      (rb.lit_params(nee=dict(select=2)), "select"), (rb.lit_params(emitters=2), "sample_emitters")):
        _refused(word, lit=lit)
    _refused("null scene", lit=None)
    assert _call(cam=None)[0] == INVALID
    for medium, word in ((rb.medium_params(sigma_t=-0.5), "sigma_t"), (rb.medium_params(sigma_t=nan), "sigma_t"),
                         (rb.medium_params(sigma_t=1.0, albedo=(0.5, 1.5, 0.5)), "albedo"), (rb.medium_params(sigma_t=1.0, g=0.96), "|g|"),
                         (rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, -1, 1)), "lo < hi")):
        for rung in (dict(), dict(tint=(nan, 1, 1)), dict(glow=dict(radiance=-1.0, source=3)), dict(glow=-1.0, sample=dict(sample=2))):
            _refused(word, medium=medium, volume=FAKE, **rung)
    for medium in (rb.medium_params(sigma_t=1.0), rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1))):
        for rung in (dict(), dict(tint=(nan, 1, 1)), dict(glow=dict(radiance=-1.0, source=3))):
            _refused("region 2", medium=medium, volume=FAKE, **rung)
    # … the tint's
    short_tint = rb.chroma_params()
    short_tint.struct_bytes = 4
    _refused("rt_chroma_params", tint=short_tint)
    for tint in ((1, -1, 1), (nan, 1, 1), (1, 1, inf)):
        _refused("tint", tint=tint)
    _refused("not finite", medium=rb.medium_params(sigma_t=3e38, box=(0, 0, 0, 1, 1, 1)), tint=(1, 2, 4))
    # … the glow's (heat and the sampler are not looked at below their rung: a tint call ignores them)
    _refused("source must", glow=dict(radiance=-1.0, source=3))
    _refused("radiance", glow=(1, -1, 1))
    _refused("sigma_t > 0", medium=rb.medium_params(sigma_t=0.0, box=(0, 0, 0, 1, 1, 1)), glow=1.0)
    _refused("need a volume", glow=dict(radiance=1.0, source=1))
    _refused("needs a heat grid", glow=dict(radiance=1.0, source=2), volume=FAKE)
    _refused("source 2 only", glow=1.0, heat=FAKE)
    _refused("null scene", tint=(1, 2, 3), heat=FAKE, sampler=FAKE)
    # … the sample's
    _refused("sample must", glow=1.0, sample=dict(sample=2, mis=2))
    _refused("mis must", glow=1.0, sample=dict(sample=1, mis=2))
    _refused("need a volume", glow=1.0, sample="mis")
    _refused("needs a sampler", glow=1.0, sample="mis", volume=FAKE)
    # 7. the sample range: sample_first + min_spp + R * batch_spp (here 4 + 15 * 4 = 64), on every rung
    for rung in (dict(), dict(tint=(1, 2, 3)), dict(glow=1.0)):
        _refused("sample_first", sample_first=-1, **rung)
        _refused("null scene", sample_first=(1 << 30) - 64, **rung)
        _refused("2^30", UNSUPPORTED, sample_first=(1 << 30) - 63, **rung)
    # 8. the buffers
    for kw in (dict(fb=0), dict(spp=0)):
        _refused("null framebuffer or sample counts", tint=(1, 2, 3), **kw)
    # 9. the scene: what passes reaches it under this call's name — grey, dark and unsampled arguments too, and no medium at all
    for kw in (dict(), dict(medium=None), dict(volume=FAKE), dict(tint=(1, 2, 3)), dict(tint=2.0), dict(tint=(1, 2, 3), medium=None),
               dict(glow=1.0), dict(glow=0.0), dict(glow=0.0, medium=None), dict(glow=dict(radiance=1.0, source=1), volume=FAKE),
               dict(glow=1.0, sample=dict(sample=0)), dict(glow=0.0, sample=dict(sample=0)), dict(sample=dict(sample=0)), dict(sample=None, glow=None)):
        _refused("null scene", **kw)
    # the order, each refusal with everything after it wrong as well
    wrong = dict(stop=bad_stop, prior=2 * FAKE, fog=None, sample_first=-1, fb=0)
    _refused("min_spp", params=_params(min_spp=1), **wrong)
    _refused("rule", **wrong)
    del wrong["stop"]
    _refused("overlaps", **wrong)
    del wrong["prior"]
    _refused("rt_fog_params", **wrong)
    del wrong["fog"]
    wrong.update(lit=rb.lit_params(lens=bad_lens), medium=rb.medium_params(sigma_t=-1.0), volume=FAKE, tint=(nan, 1, 1))
    _refused("a tint or a glow", glow=-1.0, **wrong)
    _refused("lens_radius", **wrong)
    del wrong["lit"]
    _refused("sigma_t", **wrong)
    wrong["medium"] = rb.medium_params(sigma_t=1.0)
    _refused("region 2", **wrong)
    del wrong["medium"], wrong["volume"]
    _refused("tint", **wrong)
    wrong["tint"] = (1, 2, 3)
    _refused("sample_first", **wrong)
    del wrong["sample_first"]
    _refused("null framebuffer", **wrong)
    del wrong["fb"]
    _refused("null scene", **wrong)
    # the glow's layers before the sample's, the sample's before the range
    wrong = dict(sample_first=-1, fb=0, volume=FAKE, medium=rb.medium_params(**BOX_MEDIUM))
    _refused("radiance", glow=-1.0, sample=dict(sample=2), **wrong)
    _refused("sample must", glow=1.0, sample=dict(sample=2), **wrong)
    _refused("needs a sampler", glow=1.0, sample="mis", **wrong)


def test_cli_refusals(test_config_text, tmp_path):
    """--fog-adaptive needs --lit --fog, takes T[:min:batch:max], and is refused with --fog-noise-target, --fog-denoise and everything
    --fog-noise-target is refused with: exit code 99 and a message that names the flag, nothing written.  The tint, the glow and its
    samples are not among them."""
    before = sorted(os.listdir(tmp_path))
    fog = ["--lit", "--fog", "0.5"]
    target = ["--fog-adaptive", "0.3"]

    def run(args):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    cases = [["--lit"] + target, target, ["--fog", "0.5"] + target, ["--fog-adaptive"] + fog]
    cases += [fog + ["--fog-adaptive", bad] for bad in ("x", "-0.1", "nan", "inf", "0.3:4:4", "0.3:1:4:32", "0.3:4:0:32", "0.3:8:4:4", "0.3:4:4:70000",
                                                        "0.3:4:4:32x", "0.3x", "")]
    others = (["--fog-noise-target", "0.3"], ["--fog-denoise"], ["--adaptive", "0.1"], ["--denoise"], ["--denoise-temporal"], ["--denoise-adaptive"],
              ["--denoise-adaptive-temporal"], ["--aov"], ["--stop-rule", "near"], ["--stop-history"], ["--noise-target", "0.3"])
    cases += [fog + target + other for other in others]
    cases += [fog + ["--fog-tint", "1,2,3"] + target + ["--aov"], fog + ["--fog-glow", "1,1,1"] + target + ["--denoise"]]
    for args in cases:
        r = run(args)
        assert r.returncode == 99 and "--fog-adaptive" in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    for other in others:
        assert other[0] in run(fog + target + other).stderr, other


@pytest.mark.parametrize("setting", list(far.SETTINGS))
def test_levels_are_populated_and_the_rung_is_in_them(setting):
    """The condition on the inputs of the GPU tests, on the restatement: at least 5 pixels stop at min_spp, at least 5 reach max_spp, at least
    5 stop at each of at least three levels in between, and at least 10 pixels that stop above min_spp hold the rung's own effect among the
    samples they took: under a tint a medium event (and the frame is not the grey frame at the mean extinction), under a glow a
    glow_length above 0, with samples of the glow a glow shadow ray."""
    _, spp, _ = far.setting_reference(setting)
    extra = far.setting_radiances(setting)[1]
    counts = [int((spp == n).sum()) for n in LEVELS]
    taken = np.arange(extra.shape[2])[None, None, :] < spp[..., None]
    with_effect = int((((extra > 0) & taken).any(axis=2) & (spp > SPP["min_spp"])).sum())
    print(f"setting {setting} t={far.THRESHOLDS[setting]}: pixels per level {dict(zip(LEVELS, counts))}, smallest {min(counts)}; "
          f"pixels above min_spp with the rung's effect: {with_effect}")
    assert sum(counts) == spp.size
    assert counts[0] >= 5 and counts[-1] >= 5, counts
    assert sum(c >= 5 for c in counts[1:-1]) >= 3, counts
    assert with_effect >= 10, with_effect
    if far.rung_of(setting) == "tint":
        host, cam = far.scene_cam(setting)
        kw = far.reference_keywords(setting)
        mean = float(np.mean(np.asarray(kw.pop("tint"), np.float32)))
        grey = var.reference(host, cam, threshold=far.THRESHOLDS[setting], **SPP, **{**kw, "medium": scaled(kw["medium"], mean)})
        assert not np.array_equal(grey[0], far.setting_reference(setting)[0]), "the tint changes nothing in this frame"


def test_helper_with_the_rungs_off_is_the_volume_reference():
    host, cam = var.scene_cam("b")
    kw = var.reference_keywords("b")
    want = var.reference(host, cam, threshold=var.THRESHOLDS["b"], **SPP, **kw)
    assert len(np.unique(want[1])) >= 3
    got = far.reference(host, cam, rung=None, threshold=var.THRESHOLDS["b"], **SPP, **kw)
    for g, w, col in zip(got, want, ("fb", "spp", "moments")):
        assert_same(g, w, f"no rung: {col}")
    # and the restatements' own hand-overs: equal tints, radiance 0 and no sample, through the rung's tracer
    grey = var.reference(host, cam, threshold=var.THRESHOLDS["b"], **SPP, **{**kw, "medium": scaled(kw["medium"], 2.0)})
    for rung, more, target in (("tint", dict(tint=2.0), grey), ("glow", dict(radiance=0.0, source=1), want), ("sampled", dict(radiance=0.0, source=1, sample="mis"), want)):
        got = far.reference(host, cam, rung=rung, threshold=var.THRESHOLDS["b"], **SPP, **kw, **more)
        for g, w, col in zip(got, target, ("fb", "spp", "moments")):
            assert_same(g, w, f"{rung} handed over: {col}")


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _check_triple(got, want, what):
    for g, w, col in zip(got[:3], want[:3], ("fb", "spp", "moments")):
        assert_same(g, w, f"{what}: {col}")


def _at(cam, n):
    c = rb.CameraData.from_buffer_copy(cam)
    c.samples_per_pixel = int(n)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(far.SETTINGS))
def test_equals_the_reference(setting):
    """fb, spp and moments byte for byte: the whole frame and a row shard, sample_first 0 and 37, on the default handle and on one whose
    min_spp frame takes two passes (pass_spp = 3: the moments cross a pass boundary)."""
    rb.amd_lib().rt_set_device(0)
    host, cam = far.scene_cam(setting)
    shard = rb.Shard(4, 3, 2)
    with rb.Env(lar.sky()) as env, far.device_objects(setting) as objects:
        kw = far.device_keywords(setting, env, objects)
        for config in (dict(), dict(pass_spp=3)):
            dev = rb.DeviceScene(host, device=0, **config)
            for first in (0, 37):
                for sh in (None, shard):
                    got = dev.render_fog_adaptive_to_host(cam, shard=sh, sample_first=first, threshold=far.THRESHOLDS[setting], **SPP, **kw)
                    _check_triple(got, far.setting_reference(setting, first, sh), f"{setting} {config} first={first} shard={sh is not None}")
                    t = got[3]
                    assert t.trace_launches == (2 if config.get("pass_spp") else 1) + 7 and t.guarded == 0 and t.trace_scratch_bytes == 0
                    assert t.traced_samples == got[1].size * SPP["min_spp"] and t.kernel_ms > 0
            dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rung", far.RUNGS)
def test_rule_and_prior_equal_their_references(rung):
    """rule = 1, and a non-zero prior under both rules, the whole frame and a row shard; the counts differ from the plain run's."""
    rb.amd_lib().rt_set_device(0)
    setting = ONE_PER_RUNG[rung]
    shard = rb.Shard(4, 3, 2)
    host, cam = far.scene_cam(setting)
    dev = rb.DeviceScene(host, device=0)
    plain = far.setting_reference(setting)
    with far.device_objects(setting) as objects:
        kw = far.device_keywords(setting, None, objects)
        for case in (dict(rule=1), dict(prior=True), dict(prior=True, rule=1)):
            for sh in (None, shard):
                rows = rb.amd_lib().rt_shard_rows(cam.image_height, C.byref(sh) if sh else None)
                more = {k: v for k, v in case.items() if k == "rule"}
                if case.get("prior"):
                    more["prior"] = var.prior_of(rows, cam.image_width)
                got = dev.render_fog_adaptive_to_host(cam, shard=sh, threshold=far.THRESHOLDS[setting], **SPP, **more, **kw)
                want = far.setting_reference(setting, shard=sh, **more)
                _check_triple(got, want, f"{setting} {case} shard={sh is not None}")
                if sh is None:
                    assert not np.array_equal(want[1], plain[1]), f"{case}: the counts are those without it"
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rung", far.RUNGS)
def test_per_pixel_parity_device_against_device(rung):
    """64 x 48: each pixel equals the rung's frame call at its own count, for every level."""
    rb.amd_lib().rt_set_device(0)
    setting = ONE_PER_RUNG[rung]
    host, cam = far.scene_cam(setting, (64, 48))
    dev = rb.DeviceScene(host, device=0)
    with far.device_objects(setting) as objects:
        kw = far.device_keywords(setting, None, objects)
        fb, spp, _, _ = dev.render_fog_adaptive_to_host(cam, threshold=far.THRESHOLDS[setting], **SPP, **kw)
        assert np.unique(spp).tolist() == LEVELS
        for n in LEVELS:
            want, _ = far.frame_call(dev, setting)(_at(cam, n), **kw)
            sel = spp == n
            assert_same(fb[sel], want[sel], f"pixels with {n} samples")
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rung,grid", [("tint", True), ("tint", False), ("glow", True), ("glow", False), ("sampled", True)])
def test_waves_refill_from_a_list(rung, grid):
    """192 x 128, one round of 32 samples of every pixel: more work indices than one chunk per wave of the grid, so waves refill from the
    list — in the sampled rung through the wave loop with the third shadow phase; the frame is the rung's frame call at 36 samples."""
    rb.amd_lib().rt_set_device(0)
    w, h = 192, 128
    setting = ONE_PER_RUNG[rung]
    host, cam = far.scene_cam(setting, (w, h))
    dev = rb.DeviceScene(host, device=0)
    with far.device_objects(setting) as objects:
        kw = far.device_keywords(setting, None, objects)
        if not grid:
            kw.update(volume=None, glow=dict(radiance=GLOWS[0], source=0)) if rung == "glow" else kw.update(volume=None)
        fb, spp, _, t = dev.render_fog_adaptive_to_host(cam, min_spp=4, batch_spp=32, max_spp=36, threshold=0.0, **kw)
        print(f"waves that refill: {t.num_workgroups} workgroups x {LIGHT_BLOCK // 64} waves x {LIGHT_CHUNK} = "
              f"{t.num_workgroups * (LIGHT_BLOCK // 64) * LIGHT_CHUNK} against {w * h * 32} work indices")
        assert t.num_workgroups * (LIGHT_BLOCK // 64) * LIGHT_CHUNK < w * h * 32, "no wave needs a second chunk: enlarge the image"
        assert (spp == 36).all() and t.trace_launches == 2
        assert_same(fb, far.frame_call(dev, setting)(_at(cam, 36), **kw)[0], "threshold 0 = the rung's frame call at 36 samples")
    dev.close()


@pytest.mark.gpu
def test_identities():
    """The header's identities, bit for bit in all three outputs, each through the kernels it names; where a rung was left, the probe of
    the call's own rung shows the column it lost at 0."""
    rb.amd_lib().rt_set_device(0)
    setting = "sampled b"
    host, cam = far.scene_cam(setting)
    t = far.THRESHOLDS[setting]
    dev = rb.DeviceScene(host, device=0)
    ijs = np.stack(np.meshgrid(np.arange(0, 32, 5), np.arange(0, 24, 5), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    with far.device_objects(setting) as objects, rb.GlowSampler(objects[0], 1) as q1, rb.Volume(np.zeros_like(var.density_of("b"))) as cold:
        vol = objects[0]
        base = var.device_keywords("b", None, vol)
        medium = base["medium"]
        glow = dict(radiance=GLOWS[0], source=1)

        def adaptive(**more):
            return dev.render_fog_adaptive_to_host(cam, threshold=t, **SPP, **{**base, **more})
        # threshold 0: the rung's frame call at min + R * batch (4 + 5 * 5 = 29), from sample 5, on each rung
        for more, frame in ((dict(tint=TINTS[0]), dev.render_chroma_to_host), (dict(glow=glow), dev.render_glow_to_host),
                            (dict(glow=glow, sample="mis", sampler=q1), dev.render_glow_sampled_to_host)):
            fb0, spp0, mom0, _ = dev.render_fog_adaptive_to_host(cam, min_spp=4, batch_spp=5, max_spp=32, threshold=0.0, sample_first=5, **base, **more)
            assert (spp0 == 29).all()
            assert_same(fb0, frame(_at(cam, 29), sample_first=5, **base, **more)[0], f"threshold 0 {list(more)}")
            assert_same(mom0, dev.render_fog_adaptive_to_host(cam, min_spp=29, batch_spp=1, max_spp=29, threshold=t, sample_first=5, **base, **more)[2],
                        "threshold 0: the moments of 29 samples")
        # no tint, no glow, no sample: rt_render_volume_adaptive with the remaining arguments — grid, no grid, no medium; rules and priors
        prior = var.prior_of(cam.image_height, cam.image_width)
        for rest in (dict(), dict(volume=None), dict(volume=None, medium=None), dict(medium=dict(medium, sigma_t=0.0))):
            for more in (dict(), dict(rule=1, prior=prior)):
                want = dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **{**base, **rest}, **more)
                assert len(np.unique(want[1])) >= 3
                _check_triple(adaptive(**rest, **more), want, f"no rung {list(rest)} {list(more)}")
        grey = dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **base)
        # equal tints e: the grey call at sigma_t * e (chroma NULL, the default tint and e = 0 among them)
        for e in (1.0, 2.5, 0.0):
            want = dev.render_volume_adaptive_to_host(cam, threshold=t, **SPP, **{**base, "medium": scaled(medium, e)})
            _check_triple(adaptive(tint=e), want, f"equal tints {e}")
        _check_triple(adaptive(tint=TINTS[0], medium=dict(medium, sigma_t=0.0)), adaptive(medium=None, volume=None), "a tint without extinction")
        # radiance 0: the call without a glow; sample = 0, an empty sampler, a dark glow: the call without a sample
        _check_triple(adaptive(glow=dict(radiance=0.0, source=1)), grey, "radiance 0")
        lit_glow = adaptive(glow=glow)
        assert len(np.unique(lit_glow[1])) >= 3 and not np.array_equal(lit_glow[0], grey[0])
        _check_triple(adaptive(glow=glow, sample=dict(sample=0, mis=0), sampler=q1), lit_glow, "sample = 0")
        _check_triple(adaptive(glow=glow, sample=None), lit_glow, "sample NULL")
        with rb.GlowSampler(vol, 2, cold) as q_cold:
            _check_triple(adaptive(glow=dict(radiance=GLOWS[0], source=2), heat=cold, sample="mis", sampler=q_cold),
                          adaptive(glow=dict(radiance=GLOWS[0], source=2), heat=cold), "an empty sampler")
        _check_triple(adaptive(glow=dict(radiance=0.0, source=1), sample="light", sampler=q1), grey, "a dark glow with samples")
        # a sample beside a tint: the tint's call
        _check_triple(adaptive(tint=TINTS[0], sample="mis", sampler=q1), adaptive(tint=TINTS[0]), "a sample beside a tint")
        # the columns a left rung loses, through the probes of the call's own rung
        assert not dev.trace_samples_glow_sampled(cam, ijs, **base, glow=glow, sample=dict(sample=0), sampler=q1)[9].any()
        assert not dev.trace_samples_glow(cam, ijs, **base, glow=dict(radiance=0.0, source=1))[8].any()
        assert dev.trace_samples_glow_sampled(cam, ijs, **base, glow=glow, sample="mis", sampler=q1)[9].any()
        # a 1 x 1 x 1 grid of density 1 under a tint = the homogeneous box under the same tint (the grid's chroma kernels, the medium's)
        with rb.Volume(np.ones((1, 1, 1), np.float32)) as one:
            hom = adaptive(tint=TINTS[0], volume=None)
            assert len(np.unique(hom[1])) >= 3
            _check_triple(adaptive(tint=TINTS[0], volume=one), hom, "1^3 grid = the box, tinted")
    dev.close()


@pytest.mark.gpu
def test_edges():
    import torch
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    for setting in ("tint b", "sampled b"):
        host, cam = far.scene_cam(setting)
        t = far.THRESHOLDS[setting]
        dev = rb.DeviceScene(host, device=0)
        with far.device_objects(setting) as objects:
            kw = far.device_keywords(setting, None, objects)
            # seven empty rounds terminate, and nothing is added
            fb, spp, mom, tm = dev.render_fog_adaptive_to_host(cam, threshold=1e30, **SPP, **kw)
            assert (spp == 4).all() and tm.trace_launches == 8
            _check_triple((fb, spp, mom), far.setting_reference(setting, threshold=1e30), "huge threshold")
            assert_same(fb, far.frame_call(dev, setting)(_at(cam, 4), **kw)[0], "huge threshold = the frame call at min_spp")
            # min == max: no round
            same = dev.render_fog_adaptive_to_host(cam, min_spp=4, batch_spp=4, max_spp=4, threshold=t, **kw)
            _check_triple(same, (fb, spp, mom), "min == max")
            assert same[3].trace_launches == 1
            # (max - min) no multiple of batch
            got = dev.render_fog_adaptive_to_host(cam, min_spp=4, batch_spp=7, max_spp=32, threshold=t, **kw)
            want = far.setting_reference(setting, batch_spp=7)
            assert np.unique(want[1]).tolist() == [4, 11, 18, 25, 32]
            _check_triple(got, want, "batch 7")
            # d_moments = NULL
            want = far.setting_reference(setting)
            d_fb = torch.full((SIZE[1], SIZE[0], 3), float("nan"), device="cuda:0")
            d_spp = torch.full((SIZE[1], SIZE[0]), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            dev.render_fog_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), None, threshold=t, **SPP, **kw)
            assert_same(d_fb.cpu().numpy(), want[0], "null moments: fb")
            assert_same(d_spp.cpu().numpy(), want[1], "null moments: spp")
            # max_depth <= 0: zero sums and moments, counts by the rule
            flat = far.scene_cam(setting, depth=0)[1]
            fbz, sppz, momz, _ = dev.render_fog_adaptive_to_host(flat, threshold=t, **SPP, **kw)
            assert not fbz.any() and not momz.any() and (sppz == 4).all()
            assert (dev.render_fog_adaptive_to_host(flat, threshold=0.0, **SPP, **kw)[1] == 32).all()
            # pixels x batch_spp beyond the work index arithmetic: refused with a scene, before anything is enqueued (2^24 pixels x 128)
            big = far.scene_cam(setting, (16384, 1024))[1]
            with pytest.raises(rb.RtError, match="batch_spp") as err:
                dev.render_fog_adaptive(big, FAKE, 2 * FAKE, None, min_spp=4, batch_spp=128, max_spp=132, threshold=0.1, **kw)
            assert NAME in str(err.value)
            # sync = 0 on a side stream
            s = torch.cuda.Stream()
            d_mom = torch.full((SIZE[1], SIZE[0], 2), float("nan"), device="cuda:0")
            d_fb.fill_(float("nan"))
            d_spp.fill_(-1)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                dev.render_fog_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), d_mom.data_ptr(), stream=s.cuda_stream, sync=False, threshold=t, **SPP, **kw)
            s.synchronize()
            _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), want, "sync = 0 on a side stream")
            # handles of another device
            if torch.cuda.device_count() > 1 and setting == "sampled b":
                lib.rt_set_device(1)
                other = rb.Volume(var.density_of("b"))
                other_q = rb.GlowSampler(other, 1)
                lib.rt_set_device(0)
                with pytest.raises(rb.RtError, match=NAME + ": the heat grid was created on another device"):
                    dev.render_fog_adaptive_to_host(cam, threshold=t, **SPP, **{**kw, "glow": dict(radiance=GLOWS[0], source=2), "heat": other, "sample": None})
                # (a sampler lives on its volume's device and is refused with any other volume before the scene is looked at, so the
                # volume's device is the first to be found wrong; the sampler's own refusal stands behind it)
                with pytest.raises(rb.RtError, match=NAME + ": the volume was created on another device"):
                    dev.render_fog_adaptive_to_host(cam, threshold=t, **SPP, **{**kw, "volume": other, "sampler": other_q})
                other_q.close()
                other.close()
        dev.close()


@pytest.mark.gpu
def test_rungs_alternate_on_one_handle():
    """tint, sampled glow, glow and the grey call in turn on one handle: each equals its result on a fresh handle, and rt_last_timing still
    reports the last rt_render."""
    rb.amd_lib().rt_set_device(0)
    host, cam = far.scene_cam("tint b")
    names = ("tint b", "sampled b")
    with far.device_objects("sampled b") as objects:
        kws = {n: far.device_keywords(n, None, objects) for n in names}
        kws["glow"] = {k: v for k, v in kws["sampled b"].items() if k not in ("sample", "sampler")}
        kws["grey"] = var.device_keywords("b", None, objects[0])
        fresh = {}
        for n, kw in kws.items():
            dev = rb.DeviceScene(host, device=0)
            fresh[n] = dev.render_fog_adaptive_to_host(cam, threshold=0.15, **SPP, **kw)[:3]
            dev.close()
        dev = rb.DeviceScene(host, device=0)
        dev.render_to_host(_at(cam, 4))
        before = dev.last_timing()
        for n in ("tint b", "sampled b", "glow", "grey", "sampled b", "tint b"):
            _check_triple(dev.render_fog_adaptive_to_host(cam, threshold=0.15, **SPP, **kws[n]), fresh[n], f"{n} on one handle")
        assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
        assert len({fresh[n][0].tobytes() for n in kws}) == 4
        dev.close()


@pytest.mark.gpu
def test_each_of_the_forty_list_kernels():
    """A 7 x 5 frame with one round through chroma_list_render_kernel and glow_list_render_kernel (homogeneous and grid base) and
    glow_sample_list_render_kernel, under each of the four emitter tables, pinhole and lens (with motion): the scene with planes, select and
    sample_planes in {0, 1}^2 — each against its frame twin at the full count, and without scratch."""
    rb.amd_lib().rt_set_device(0)
    scene = "fuzz planes"
    host, camera, _ = scenes()[scene]
    w, h = 7, 5
    params = dict(min_spp=2, batch_spp=3, max_spp=5, threshold=0.0)
    medium = dict(sigma_t=0.5, albedo=(0.95, 0.9, 0.8), g=0.3, box=BOX)
    dev = rb.DeviceScene(host, device=0)
    seen = 0
    with rb.Volume(GRIDS["2x3x5"]) as vol, rb.Volume(HEATS["2x3x5"]) as hv, rb.GlowSampler(vol, 2, hv) as q:
        rungs = [(dev.render_chroma_to_host, dict(tint=TINTS[0]), (None, vol)), (dev.render_glow_to_host, dict(glow=GLOWS[0]), (None,)),
                 (dev.render_glow_to_host, dict(glow=dict(radiance=GLOWS[0], source=2), heat=hv), (vol,)),
                 (dev.render_glow_sampled_to_host, dict(glow=dict(radiance=GLOWS[0], source=2), heat=hv, sample="mis", sampler=q), (vol,))]
        for frame, more, volumes in rungs:
            for volume in volumes:
                for lens in (False, True):
                    for select, planes in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        nee = dict(select=select, sample_planes=planes, glossy=(select + planes) % 2)
                        # (the closing camera of a shutter carries the call's own sample count)
                        kw1, kw5 = (dict(dev_kw(scene, "lens + motion" if lens else "mis", None, w, h, n, 12), nee=nee) for n in (1, 5))
                        got = dev.render_fog_adaptive_to_host(camera(w, h, 1, 12), medium=medium, volume=volume, **params, **more, **kw1)
                        what = f"{list(more)} grid={volume is not None} lens={lens} select={select} planes={planes}"
                        assert (got[1] == 5).all() and got[3].trace_launches == 2, what
                        assert_same(got[0], frame(camera(w, h, 5, 12), medium=medium, volume=volume, **more, **kw5)[0], what)
                        assert got[3].trace_scratch_bytes == 0, what
                        seen += 1
    assert seen == 40
    dev.close()


def _cli_frame(tmp_path, text, args):
    out = subprocess.run([EXE, "--gpu", *args], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    return open(tmp_path / "f_0.png", "rb").read(), int(out.stdout.split("\n")[0].split("\t")[2])


@pytest.mark.gpu
def test_cli_fog_adaptive_frames_are_the_python_path(test_config_text, tmp_path):
    """rtp_main --fog-adaptive with a tint in a box, with --fog-glow over --fog-grid, and with --fog-glow-sample mis: the file's bytes and
    the printed count are the Python path's."""
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
    common = ["--lit", "--nee", "--light-tree", "--fog", "0.4:0.9:0.3", "--fog-box", ",".join(str(x) for x in box), "--fog-adaptive", "0.3:4:4:32"]
    medium = dict(sigma_t=0.4, albedo=0.9, g=0.3, box=box)
    with rb.Volume(density) as vol, rb.GlowSampler(vol, 1) as q:
        for args, kw in ((["--fog-tint", "0.25,1,4"], dict(tint=(0.25, 1.0, 4.0))),
                         (["--fog-glow", "0.2,1,3:density", "--fog-grid", str(tmp_path / "grid.vol")], dict(volume=vol, glow=dict(radiance=(0.2, 1.0, 3.0), source=1))),
                         (["--fog-glow", "0.2,1,3:density", "--fog-grid", str(tmp_path / "grid.vol"), "--fog-glow-sample", "mis"],
                          dict(volume=vol, glow=dict(radiance=(0.2, 1.0, 3.0), source=1), sample="mis", sampler=q))):
            got, printed = _cli_frame(tmp_path, text, common + args)
            fb, spp, _, _ = dev.render_fog_adaptive_to_host(host.frame_camera_at(0.0), nee=dict(select=1), threshold=0.3, **SPP, medium=medium, **kw)
            assert len(np.unique(spp)) >= 2
            d_fb, d_spp = torch.from_numpy(fb).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
            rgb = torch.zeros(fb.shape, dtype=torch.uint8, device="cuda:0")
            assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == OK
            torch.cuda.synchronize()
            want = np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes()
            assert got == want, args
            assert printed == int(spp.sum()), args
    dev.close()
