"""The history-aware stopping rule (include/rtp_amd.h "a history-aware stopping rule"): rt_adaptive_prior turns the
history of rt_denoise_temporal_spp into a prior (ch, vh) per pixel, and rt_render_adaptive_prior / rt_render_lit_adaptive_prior /
rt_adaptive_judge_prior judge by the variance the denoiser's blend will carry.  Every device result is compared byte for byte with the
restatements of tests/adaptive_prior_reference.py: the prior from device histories, single judgements, whole frames of both render
calls under both rules, and the loop prior → render → rt_denoise_temporal_spp over four frames, through Python and through rtp_main.
On the CPU: the ABI, every refusal (they come before any HIP call, so fake addresses do), the restatement's identities, the coverage
of the rendered setting, and the saving and the quality of §24's experiment with the prior, measured and pinned."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import adaptive_prior_reference as apr
import adaptive_rule_reference as arr
import denoise_temporal_reference as dtr
import denoise_temporal_spp_reference as dtsr
import lit_adaptive_reference as lar
import rtp_bindings as rb
import test_adaptive as ta
import test_denoise_temporal_spp as tdts
import test_light_tree as tl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
FAKE = 1 << 32          # a device address that is never dereferenced: every check comes before any HIP call
OK, INVALID, UNSUPPORTED = 0, 1, 4
F = np.float32
SPP, A = tdts.SPP, tdts.A
_oracle_orbit, _orbit_cam, _with_spp = tdts._oracle_orbit, tdts._orbit_cam, tdts._with_spp
# The orbit's threshold in this file.  At tests/test_denoise_temporal_spp.py's 0.3 rule 1 is nearly done at min_spp (4.3 spp on
# average) and the prior changes the count of 8.2 % of the hit pixels only (rule 0: 45.6 %); at 0.2 it changes 56.9 % under rule 0 and 53.7 %
# under rule 1, so the coverage condition below (10 %) holds under both.
ORBIT_T = 0.2
W, H = 77, 45
assert_same = ta.assert_same


# ---- no GPU needed: the ABI and the refusals --------------------------------------------------------------------------

def test_abi_symbols_argtypes_and_functions():
    lib = rb.amd_lib()
    for s in ("rt_adaptive_prior", "rt_render_adaptive_prior", "rt_render_lit_adaptive_prior", "rt_adaptive_judge_prior"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    at = lib.rt_adaptive_prior.argtypes
    assert len(at) == 7 and at[0]._type_ is rb.AovBuffers and at[1] is C.c_int32 and at[2]._type_ is rb.CameraData and at[4] is C.c_uint64
    assert lib.rt_render_adaptive_prior.argtypes == lib.rt_render_adaptive_rule.argtypes + [C.c_void_p] and len(lib.rt_render_adaptive_prior.argtypes) == 12
    assert lib.rt_render_lit_adaptive_prior.argtypes == lib.rt_render_lit_adaptive_rule.argtypes + [C.c_void_p]
    assert len(lib.rt_render_lit_adaptive_prior.argtypes) == 14
    assert lib.rt_adaptive_judge_prior.argtypes == lib.rt_adaptive_judge.argtypes + [C.c_void_p] and len(lib.rt_adaptive_judge_prior.argtypes) == 11
    assert C.sizeof(rb.StopParams) == 16 and C.sizeof(rb.AdaptiveParams) == 20
    assert callable(rb.adaptive_prior) and callable(rb.TemporalDenoiser.prior) and callable(rb.TemporalDenoiser.prior_to_host)
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        header = f.read()
    for decl in ("rt_status rt_adaptive_prior(", "rt_status rt_render_adaptive_prior(", "rt_status rt_render_lit_adaptive_prior(",
                 "rt_status rt_adaptive_judge_prior("):
        assert decl in header, decl
    assert lib.rt_version_string().decode().startswith("rtp_amd 0.5")


W8, H4 = 8, 4
PIX = W8 * H4
# fake addresses of rt_adaptive_prior's arguments: albedo 2, normal 3, depth 4, hits 5, prim 6, history 9, prior 13 (x FAKE)


def _aov(**put):
    b = rb.AovBuffers()
    b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count, b.first_prim = 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE, 6 * FAKE
    for field, value in put.items():
        setattr(b, field, value)
    return b


def _cam(**fields):
    cam = rb.make_camera(W8, H4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    for k, v in fields.items():
        setattr(cam, k, v)
    return cam


def _prior_call(aov="full", aov_spp=4, cam="default", prev=9 * FAKE, hist_bytes=None, prior=13 * FAKE):
    lib = rb.amd_lib()
    aov = _aov() if aov == "full" else aov
    cam = _cam() if cam == "default" else cam
    w, h = (cam.image_width, cam.image_height) if cam is not None else (W8, H4)
    hist_bytes = lib.rt_denoise_history_bytes(w, h) if hist_bytes is None else hist_bytes
    st = lib.rt_adaptive_prior(C.byref(aov) if aov is not None else None, aov_spp, C.byref(cam) if cam is not None else None, C.c_void_p(prev),
                               hist_bytes, C.c_void_p(prior), None)
    return st, lib.rt_get_last_error_string().decode()


def test_prior_refusals_need_no_device():
    """No call here may pass every check (the addresses are fake): what is allowed is shown by a later check's refusal."""
    hist = rb.amd_lib().rt_denoise_history_bytes(W8, H4)
    cases = [(dict(aov=None), "null"), (dict(cam=None), "null"), (dict(prior=0), "null"),
             (dict(cam=_cam(image_width=0)), "width and height"), (dict(cam=_cam(image_height=-3)), "width and height"),
             (dict(aov_spp=0), "aov_samples"), (dict(aov_spp=65537), "aov_samples"), (dict(aov_spp=-4), "aov_samples"),
             (dict(hist_bytes=hist - 1), "history_bytes"), (dict(hist_bytes=0), "history_bytes"), (dict(prev=9 * FAKE + 4), "16-byte aligned"),
             (dict(prev=9 * FAKE + 8), "16-byte aligned")]
    for field in ("albedo_sum", "normal_sum", "depth_sum", "hit_count", "first_prim"):
        cases.append((dict(aov=_aov(**{field: None})), "first_prim are required"))
    short = _aov()
    short.struct_bytes = 40                                           # first_prim lies past struct_bytes: it counts as NULL
    cases.append((dict(aov=short), "first_prim are required"))
    for kw, word in cases:
        st, msg = _prior_call(**kw)
        assert st == INVALID and msg.startswith("rt_adaptive_prior:") and word in msg, (kw, st, msg)
    for w, h in ((4097, 4096), (1 << 24, 2)):
        st, msg = _prior_call(cam=_cam(image_width=w, image_height=h))
        assert st == UNSUPPORTED and "2^24" in msg and msg.startswith("rt_adaptive_prior:"), (w, h, st, msg)
    # allowed: no history (its size is then nobody's), the ends of A's range, cam's samples_per_pixel — a later check refuses
    late = dict(prior=6 * FAKE)                                       # "d_prior overlaps an input"
    for kw in (dict(prev=0, hist_bytes=0), dict(prev=0), dict(aov_spp=1), dict(aov_spp=65536), dict(cam=_cam(samples_per_pixel=0)),
               dict(cam=_cam(samples_per_pixel=65537)), dict(hist_bytes=1 << 40)):
        st, msg = _prior_call(**late, **kw)
        assert st == INVALID and msg == "rt_adaptive_prior: d_prior overlaps an input", (kw, st, msg)


def test_prior_overlaps_to_the_byte():
    """d_prior is 8 bytes per pixel: the last byte that overlaps is refused on both sides, the first that does not passes that check and
    fails a later one (the last input's free sides cannot be shown without a launch)."""
    hist = rb.amd_lib().rt_denoise_history_bytes(W8, H4)
    for kw in (dict(prior=9 * FAKE + hist - 1), dict(prior=9 * FAKE - 8 * PIX + 1), dict(prior=9 * FAKE)):
        st, msg = _prior_call(**kw)
        assert st == INVALID and msg == "rt_adaptive_prior: d_prior overlaps history_prev", (kw, st, msg)
    fields = (("albedo_sum", 2, 12), ("normal_sum", 3, 12), ("depth_sum", 4, 4), ("hit_count", 5, 4), ("first_prim", 6, 4))
    for field, k, size in fields:
        for prior in (k * FAKE + size * PIX - 1, k * FAKE - 8 * PIX + 1):
            st, msg = _prior_call(prior=prior)
            assert st == INVALID and msg == "rt_adaptive_prior: d_prior overlaps an input", (field, hex(prior), st, msg)
    # free of the history (and without one, inside where it would lie) and of every input but the last, which sits on d_prior
    for prior in (9 * FAKE + hist, 9 * FAKE - 8 * PIX):
        st, msg = _prior_call(prior=prior, aov=_aov(first_prim=prior))
        assert st == INVALID and msg.endswith("d_prior overlaps an input"), (hex(prior), st, msg)
    st, msg = _prior_call(prev=0, prior=9 * FAKE + 16, aov=_aov(first_prim=9 * FAKE + 16))
    assert st == INVALID and msg.endswith("d_prior overlaps an input"), (st, msg)
    for field, k, size in fields[:4]:
        for prior in (k * FAKE + size * PIX, k * FAKE - 8 * PIX):
            st, msg = _prior_call(prior=prior, aov=_aov(first_prim=prior + 8 * PIX - 1))
            assert st == INVALID and msg.endswith("d_prior overlaps an input"), (field, hex(prior), st, msg)
            # … and with the last input out of the way too, only the history's check is left to refuse
            st, msg = _prior_call(prior=prior, prev=prior + 8 * PIX - 16 if prior % 16 == 0 else prior + 8 * PIX - 8)
            assert st == INVALID and msg.endswith("d_prior overlaps history_prev"), (field, hex(prior), st, msg)


def test_prior_order_of_the_checks():
    """Arguments, AOV buffers, image size, aov_samples, pixel limit, history size, alignment, the history's overlap, the inputs'."""
    big = _cam(image_width=1 << 24, image_height=2)
    rest = dict(hist_bytes=0, prev=9 * FAKE + 4, prior=9 * FAKE + 4)
    assert "null" in _prior_call(cam=None, aov=_aov(first_prim=None), aov_spp=0, **rest)[1]
    assert "first_prim are required" in _prior_call(aov=_aov(first_prim=None), cam=_cam(image_width=0), aov_spp=0, **rest)[1]
    assert "width and height" in _prior_call(cam=_cam(image_width=0), aov_spp=0, **rest)[1]
    assert "aov_samples" in _prior_call(cam=big, aov_spp=0, **rest)[1]
    assert "2^24" in _prior_call(cam=big, **rest)[1]
    assert "history_bytes" in _prior_call(**rest)[1]
    assert "16-byte aligned" in _prior_call(**{**rest, "hist_bytes": None})[1]
    assert "overlaps history_prev" in _prior_call(prev=6 * FAKE, prior=6 * FAKE)[1]
    assert "overlaps an input" in _prior_call(prior=6 * FAKE)[1]


def _params(**kw):
    return rb.adaptive_params(**{**dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1), **kw})


def _stop(rule=1, struct_bytes=None):
    s = rb.stop_params(rule=rule)
    if struct_bytes is not None:
        s.struct_bytes = struct_bytes
    return s


# fake addresses of the render calls' arguments: fb 1, spp 2, moments 3, prior 4 (x FAKE); the scene is NULL throughout

def _call_plain(params="default", stop=None, cam="default", shard=None, fb=FAKE, spp=2 * FAKE, mom=3 * FAKE, prior=4 * FAKE):
    lib = rb.amd_lib()
    params = _params() if params == "default" else params
    cam = _cam() if cam == "default" else cam
    st = lib.rt_render_adaptive_prior(None, C.byref(cam) if cam is not None else None, C.byref(shard) if shard is not None else None,
                                      C.byref(params) if params is not None else None, C.byref(stop) if stop is not None else None, C.c_void_p(fb),
                                      C.c_void_p(spp), C.c_void_p(mom), None, 1, None, C.c_void_p(prior))
    return st, lib.rt_get_last_error_string().decode()


def _call_lit(params="default", stop=None, lit="default", cam="default", shard=None, fb=FAKE, spp=2 * FAKE, mom=3 * FAKE, prior=4 * FAKE,
              sample_first=0):
    lib = rb.amd_lib()
    params = _params() if params == "default" else params
    lit = rb.lit_params() if lit == "default" else lit
    cam = _cam() if cam == "default" else cam
    st = lib.rt_render_lit_adaptive_prior(None, C.byref(cam) if cam is not None else None, C.byref(lit) if lit is not None else None,
                                          C.byref(params) if params is not None else None, C.byref(stop) if stop is not None else None,
                                          C.byref(shard) if shard is not None else None, sample_first, C.c_void_p(fb), C.c_void_p(spp),
                                          C.c_void_p(mom), None, 1, None, C.c_void_p(prior))
    return st, lib.rt_get_last_error_string().decode()


@pytest.mark.parametrize("call,name", [(_call_plain, "rt_render_adaptive_prior"), (_call_lit, "rt_render_lit_adaptive_prior")])
def test_render_refusals_with_a_null_scene(call, name):
    """The _rule call's checks keep their codes and words; the overlap of d_prior comes right after the stop checks, to the byte on
    both sides of each buffer, under the new call's name; what passes it is refused for the scene."""
    assert call(params=None)[0] == INVALID
    for kw, code, word in ((dict(min_spp=1), INVALID, "min_spp"), (dict(batch_spp=0), INVALID, "batch_spp"), (dict(max_spp=3), INVALID, "max_spp"),
                           (dict(threshold=float("nan")), INVALID, "threshold"), (dict(max_spp=65537), UNSUPPORTED, "65536")):
        st, msg = call(params=_params(**kw), stop=_stop(5), prior=FAKE)
        assert st == code and word in msg, (kw, st, msg)
    for stop, word in ((_stop(1, struct_bytes=4), "struct_bytes"), (_stop(2), "rule"), (_stop(-1), "rule")):
        st, msg = call(stop=stop, prior=FAKE)                         # (a bad prior does not overtake a bad rule)
        assert st == INVALID and word in msg and name.replace("_prior", "_rule") in msg, (st, msg)
    text = name + ": d_prior overlaps d_fb_sum, d_spp or d_moments"
    for base, size in ((FAKE, 12 * PIX), (2 * FAKE, 4 * PIX), (3 * FAKE, 8 * PIX)):
        for stop in (None, _stop(0), _stop(1)):
            for prior in (base, base + size - 1, base - 8 * PIX + 1):
                st, msg = call(stop=stop, prior=prior)
                assert st == INVALID and msg == text, (hex(prior), st, msg)
            for prior in (base + size, base - 8 * PIX):
                st, msg = call(stop=stop, prior=prior)
                assert st == INVALID and "null scene" in msg, (hex(prior), st, msg)
    # before the buffers and the scene; without moments their range is nobody's; no prior, no check
    assert call(prior=FAKE, fb=FAKE, spp=0)[1] == text
    assert "null scene" in call(mom=0, prior=3 * FAKE)[1]
    assert "null scene" in call(prior=0, fb=FAKE, spp=FAKE)[1]
    # the size is the part's: rows 0-1 of 4 under bands of 2 rows over 2 parts are 16 pixels
    part = rb.Shard(2, 2, 0)
    assert call(shard=part, prior=FAKE + 12 * 16 - 1)[1] == text
    assert "null scene" in call(shard=part, prior=FAKE + 12 * 16, mom=0)[1]
    assert call(shard=part, prior=2 * FAKE - 8 * 16 + 1)[1] == text
    assert "null scene" in call(shard=part, prior=2 * FAKE - 8 * 16)[1]


def test_lit_call_checks_the_prior_before_the_lit_parameters():
    bad_lens = rb.lit_params(lens=dict(lens_radius=-1.0))
    assert "rule" in _call_lit(stop=_stop(2), lit=bad_lens, sample_first=-1, prior=FAKE)[1]
    assert "d_prior overlaps" in _call_lit(stop=_stop(1), lit=bad_lens, sample_first=-1, prior=FAKE)[1]
    assert "lens_radius" in _call_lit(stop=_stop(1), lit=bad_lens, sample_first=-1)[1]
    assert "sample_first" in _call_lit(stop=_stop(1), sample_first=-1, fb=0)[1]
    assert "null framebuffer" in _call_lit(stop=_stop(1), fb=0)[1]
    assert "null scene" in _call_lit(stop=_stop(1))[1]


def test_judge_prior_refusals():
    lib = rb.amd_lib()

    def judge(width=4, rows=3, shard=None, params="default", stop="default", n=4, mom=FAKE, out=2 * FAKE, prior=3 * FAKE):
        params = _params() if params == "default" else params
        stop = _stop(1) if stop == "default" else stop
        st = lib.rt_adaptive_judge_prior(width, rows, C.byref(shard) if shard is not None else None, C.byref(params) if params is not None else None,
                                         C.byref(stop) if stop is not None else None, n, C.c_void_p(mom), None, C.c_void_p(out), None, C.c_void_p(prior))
        return st, lib.rt_get_last_error_string().decode()
    for kw, code, word in ((dict(params=None), INVALID, "params"), (dict(params=_params(batch_spp=0)), INVALID, "batch_spp"),
                           (dict(stop=_stop(2)), INVALID, "rule"), (dict(stop=_stop(1, struct_bytes=4)), INVALID, "struct_bytes"),
                           (dict(width=0), INVALID, "width"), (dict(rows=0), INVALID, "rows"), (dict(width=1 << 13, rows=(1 << 11) + 1), UNSUPPORTED, "2^24"),
                           (dict(n=1), INVALID, "n below 2"), (dict(shard=rb.Shard(4, 3, 7)), INVALID, "shard"), (dict(mom=0), INVALID, "null"),
                           (dict(out=0), INVALID, "null"), (dict(prior=2 * FAKE), INVALID, "d_prior overlaps d_goes_on_out"),
                           (dict(prior=2 * FAKE + 11), INVALID, "d_prior overlaps"), (dict(prior=2 * FAKE - 8 * 12 + 1), INVALID, "d_prior overlaps")):
        st, msg = judge(**kw)
        assert st == code and word in msg and msg.startswith("rt_adaptive_judge_prior:"), (kw, st, msg)
    # the order: the other checks first, the overlap last
    assert "null" in judge(out=0, prior=0)[1] and "n below 2" in judge(n=1, prior=2 * FAKE)[1]


def test_cli_refusals(test_config_text, tmp_path):
    before = sorted(os.listdir(tmp_path))
    flag, dat = "--stop-history", "--denoise-adaptive-temporal"

    def run(args, env=None):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                              env={**os.environ, **(env or {})})
    ad, lit = ["--adaptive", "0.3"], ["--lit", "--noise-target", "0.3"]
    for args in ([flag], ad + [flag], lit + [flag], ad + ["--denoise-adaptive", flag], ["--denoise", flag], ["--denoise-temporal", flag],
                 ad + ["--stop-rule", "near", flag], ["--lit", "--fog", "0.1", flag]):
        r = run(args)
        assert r.returncode == 2 and flag in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    # with the flag it needs, that flag's own refusals are what they were
    for args, env in (([dat, flag], None), (ad + [dat, flag, "--denoise"], None), (lit + [dat, flag, "--lens", "0.1:10"], None),
                      (ad + [dat, flag], {"RTP_DEVICES": "2"})):
        r = run(args, env)
        assert r.returncode == 2 and dat in r.stderr and flag not in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before
    # every refusal that was there keeps its text and code without the flag
    r = run(ad + ["--denoise-adaptive", "--denoise-temporal"])
    assert r.returncode == 2 and "--denoise-adaptive writes" in r.stderr and flag not in r.stderr, (r.returncode, r.stderr)
    r = run(["--adaptive", "0.1", "--denoise-temporal"])
    assert r.returncode == 2 and "--adaptive renders frame after frame" in r.stderr and flag not in r.stderr, (r.returncode, r.stderr)
    r = run(["--lit", "--denoise-temporal"])
    assert r.returncode == 99 and "--lit renders frame after frame" in r.stderr, (r.returncode, r.stderr)
    r = run(["--adaptive", "0.1", "--stop-rule", "far"])
    assert r.returncode == 2 and "--stop-rule" in r.stderr and flag not in r.stderr, (r.returncode, r.stderr)
    r = run([dat])
    assert r.returncode == 2 and "it needs --adaptive T or --lit --noise-target T" in r.stderr and flag not in r.stderr


# ---- the restatement's identities --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _orbit_radiances():
    """The oracle's per-sample radiances of _oracle_orbit's four frames, (H, W, 32, 3) each (shared: do not write)."""
    import oracle_bindings as ob
    host = rb.HostScene.rtiow()
    s = SPP["max_spp"]
    jj, ii, ss = np.meshgrid(np.arange(H), np.arange(W), np.arange(s), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], axis=1).astype(np.int32)
    rads = []
    for k in range(4):
        rad = ob.trace_samples(host, _orbit_cam(k), ijs)[0].reshape(H, W, s, 3)
        rad.setflags(write=False)
        rads.append(rad)
    return rads


@functools.lru_cache(maxsize=None)
def _chain(rule, with_prior, t=ORBIT_T):
    """The chained CPU model over the oracle orbit: the prior from the restated history (none without with_prior), the rule with it,
    rt_denoise_temporal_spp's restatement.  Per frame a dict of prior, fb, spp, mom, out, hist, aov, cam (shared: do not write)."""
    prev, frames = None, []
    for rad, (_, _, _, aov, cam) in zip(_orbit_radiances(), _oracle_orbit()):
        pr = apr.prior(aov, A, cam, prev) if with_prior else None
        fb, spp, mom = apr.from_radiances(rad, None, threshold=t, rule=rule, pr=pr, **SPP)
        out, prev = dtsr.reference(fb, spp, mom, aov, A, cam, prev)
        for a in (pr, fb, spp, mom, out, prev):
            if a is not None:
                a.setflags(write=False)
        frames.append(dict(prior=pr, fb=fb, spp=spp, mom=mom, out=out, hist=prev, aov=aov, cam=cam))
    return frames


def test_zero_prior_is_the_rule_restatement_exactly():
    rad = _orbit_radiances()[0]
    rng = np.random.default_rng(3)
    for rule in (0, 1):
        for shard in (None, (3, 2, 1)):
            rows = rad[12:36] if shard else rad
            want = arr.from_radiances(rows, shard, threshold=ORBIT_T, rule=rule, **SPP)
            assert len(np.unique(want[1])) >= 3
            zero = np.zeros(rows.shape[:2] + (2,), F)
            # (0, 0), a negative zero and what else fails ch > 0 && vh >= 0: a zero count with any variance
            odd = zero.copy()
            odd[..., 0] = np.where(rng.random(rows.shape[:2]) < 0.5, F(-0.0), F(0))
            odd[..., 1] = rng.uniform(0, 10, rows.shape[:2]).astype(F)
            for pr, what in ((None, "no prior"), (zero, "a zero prior"), (odd, "zero counts")):
                got = apr.from_radiances(rows, shard, threshold=ORBIT_T, rule=rule, pr=pr, **SPP)
                for g, w_, col in zip(got, want, ("fb", "spp", "moments")):
                    assert_same(g, w_, f"rule {rule}, shard {shard}, {what}: {col}")
    # the judgement itself: rule 0 is test_adaptive's, rule 1 adaptive_rule_reference's
    mom = rng.uniform(0, 30, (6, 67, 2)).astype(F)
    s1, s2, z = mom[..., 0].ravel(), mom[..., 1].ravel(), np.zeros((6 * 67, 2), F)
    assert np.array_equal(apr.goes_on(s1, s2, z, 8, 4, 64, 0.1), ta.goes_on(s1, s2, 8, 4, 64, 0.1))
    assert np.array_equal(apr.noisy(s1, s2, z, 8, 0.1), arr.noisy(s1, s2, 8, 0.1))


def test_empty_histories_give_an_all_zero_prior_and_sky_gets_none():
    frames = _chain(0, True)
    f0, f1 = frames[0], frames[1]
    aov, cam = f1["aov"], f1["cam"]
    hit = aov["hits"] > 0
    assert (~hit).any() and hit.any()
    own = apr.prior(aov, A, cam, f0["hist"])
    assert (own[hit][:, 0] > 0).sum() > hit.sum() // 2 and not own[~hit].any(), "its own history is taken; sky pixels get (0, 0)"
    assert not f0["prior"].any(), "frame 0 has no history"
    # NULL, all zero, another size, rt_denoise_temporal's magic, mode 1 (written without moments)
    zero = np.zeros_like(f0["hist"])
    other = f0["hist"].copy()
    other.view(np.int32)[1] = W + 1
    old = f0["hist"].copy()
    old.view(np.uint32)[0] = tdts.OLD_MAGIC
    spatial = dtsr.reference(f0["fb"], f0["spp"], None, f0["aov"], A, f0["cam"], None)[1]
    assert dtsr.header(spatial) == (dtsr.MAGIC, W, H, dtsr.MODE_SPATIAL) and dtsr.header(f0["hist"]) == (dtsr.MAGIC, W, H, dtsr.MODE_MOMENTS)
    for prev, what in ((None, "NULL"), (zero, "all zero"), (other, "another size"), (old, "rt_denoise_temporal's magic"), (spatial, "mode 1")):
        assert not apr.prior(aov, A, cam, prev).view(np.uint32).any(), what
    # a camera that looks away: every pixel projects outside
    away = rb.make_camera(W, H, 20.0, (-50, 3, 0), (-100, 3, 0), (0.7, 0.8, 1.0), 1, 50)
    assert not apr.prior(aov, A, cam, _rehead(f0["hist"], away)).any()


def _rehead(history, cam):
    """The history with another camera in its header."""
    h = np.array(history, copy=True)
    h[16:16 + C.sizeof(cam)] = np.frombuffer(bytes(cam), np.uint8)
    return h


def test_prior_on_single_taps_recomputed_in_numpy():
    """ch and vh for the pixels whose reprojection lands on one tap of weight 1 (u and v whole numbers under a still camera: W = 1 and
    every sum is the tap's own value), from the history planes, one float32 operation at a time — on the synthetic 130 x 9 frames of
    tests/test_denoise_temporal_spp.py, whose camera looks along an axis (the orbit's has 19 such pixels)."""
    (fb, spp, mom, aov), _, a = tdts._synthetic_frames()
    cam = tdts._synthetic_cam()
    w, h = cam.image_width, cam.image_height
    _, hist = dtsr.reference(fb, spp, mom, aov, a, cam, None)
    hit = aov["hits"] > 0
    z = np.where(hit, aov["depth"] / np.maximum(aov["hits"], 1).astype(F), 0).astype(F)
    u, v, t = tdts._reprojection(cam, cam, z)
    yy, xx = np.mgrid[0:h, 0:w].astype(F)
    got = apr.prior(aov, a, cam, hist)                                # the same frame again: a hit pixel finds itself
    p = dtr.planes(hist, w, h)
    whole = (u == xx) & (v == yy) & (t > 0) & hit & (p["moments"][..., 2] > 0) & (np.abs(aov["normal"]).sum(-1) > 0)
    print(f"{int(whole.sum())} of {int(hit.sum())} hit pixels reproject onto one tap of weight 1")
    assert whole.sum() >= 50
    d = np.fmax((aov["albedo"] * F(1.0 / a)).astype(F), F(1e-3))
    dl = ((F(0.2126) * d[..., 0] + F(0.7152) * d[..., 1]).astype(F) + (F(0.0722) * d[..., 2]).astype(F)).astype(F)
    assert_same(got[..., 0][whole], p["position"][..., 3][whole], "ch = cnt_q")
    assert_same(got[..., 1][whole], (p["normal"][..., 3] * (dl * dl).astype(F)).astype(F)[whole], "vh = V_q * (dl * dl)")
    assert_same(got[..., 0][whole], spp.astype(F)[whole], "cnt of a first frame is its count")
    assert (got[..., 0][whole] > 0).all() and (got[..., 1][whole] > 0).any()
    # a hit pixel whose count was 0 left no record: nothing to reproject onto
    gone = hit & (spp < 1) & (u == xx) & (v == yy)
    assert gone.any() and not got[gone].any()


def _one(vm_samples, pr, rule, n=8, t=0.1, max_spp=64):
    """One pixel's judgement: samples of luminance y (n of them) and a prior."""
    y = np.asarray(vm_samples, F)
    s1, s2 = F(0), F(0)
    for s in y:
        s1, s2 = F(s1 + s), F(s2 + F(s * s))
    mom = np.array([[[s1, s2]]], F)
    return bool(apr.judge(mom, np.asarray(pr, F).reshape(1, 1, 2), n, None, None, rule, 4, max_spp, t)[0, 0])


def test_judgement_fallbacks_floor_and_both_directions():
    noisy_y = [0.1, 0.9] * 4          # mean 0.5, vm = 0.1829 / 8: goes on at t = 0.1 under both rules
    quiet_y = [0.5, 0.52] * 4         # vm ~ 1.4e-5: stops at t = 0.1 under both rules
    for rule in (0, 1):
        assert _one(noisy_y, (0, 0), rule) and not _one(quiet_y, (0, 0), rule)
        # a NaN vh, a NaN ch, a negative ch or vh: the pixel's own samples judge
        for pr in ((64, np.nan), (np.nan, 0), (-4, 0), (64, -1e-3), (np.nan, np.nan), (0, 1e9), (-np.inf, 0)):
            assert _one(noisy_y, pr, rule) and not _one(quiet_y, pr, rule), (rule, pr)
        # vh = 0 and a large count silence a pixel that goes on without the prior …
        assert not _one(noisy_y, (1e6, 0), rule)
        # … but never below the floor's share: a = 0.2 keeps (0.2 * 0.2) * vm, which a smaller threshold still sees
        assert _one(noisy_y, (1e6, 0), rule, t=0.03)
        # a large vh keeps a pixel going that stops without it, and +inf does
        assert _one(quiet_y, (64, 1.0), rule) and _one(quiet_y, (64, np.inf), rule)
        # the cap and t = 0 are untouched
        assert not _one(quiet_y, (64, 1.0), rule, max_spp=11) and _one(quiet_y, (1e6, 0), rule, t=0.0)
    # the floor itself: ch = 1e6 gives a = 0.2 exactly, so ve = (0.8f * 0.8f) * vh + (0.2f * 0.2f) * vm
    vm, nf = np.array([0.37], F), np.array([8], F)
    a = F(0.2)
    b = F(F(1) - a)
    want = F(F(F(b * b) * F(2.5)) + F(F(a * a) * vm[0]))
    assert apr.blended_variance(vm, nf, np.array([1e6], F), np.array([2.5], F))[0] == want
    assert F(nf[0] / F(1e6 + 8)) < a
    # above the floor a = nf / (ch + nf): ch = 8 = nf gives a = b = 0.5
    assert apr.blended_variance(vm, nf, np.array([8], F), np.array([2.5], F))[0] == F(F(F(0.25) * F(2.5)) + F(F(0.25) * vm[0]))


def test_rule_1_prior_silences_the_pixel_whose_flag_keeps_a_neighbour_going():
    rows, width, n = 6, 67, 8
    s1 = np.full((rows, width), F(0.5) * F(n), F)
    s2 = np.full((rows, width), F(0.25) * F(n), F)
    s1[2, 30], s2[2, 30] = F(4) * F(n // 2), F(16) * F(n // 2)          # one noisy pixel: half its samples 0, half 4
    mom = np.stack([s1, s2], axis=-1)
    none = np.zeros((rows, width, 2), F)
    # vm = 4.571 / 8 is above (t * t) * (2 + 0.01) = 0.0804 at t = 0.2 and the floor's share of it, 0.04 * vm = 0.0229, is below
    p = dict(batch_spp=4, max_spp=64, threshold=0.2)
    on = apr.judge(mom, none, n, None, None, 1, **p)
    assert on.sum() == 9 and on[1:4, 29:32].all()
    silenced = none.copy()
    silenced[2, 30] = (1e6, 0)
    assert not apr.judge(mom, silenced, n, None, None, 1, **p).any(), "the window goes quiet with its one noisy pixel"
    elsewhere = none.copy()
    elsewhere[2, 31] = (1e6, 0)
    assert np.array_equal(apr.judge(mom, elsewhere, n, None, None, 1, **p), on), "a quiet neighbour's prior changes nothing"
    # bands of 2 rows over 3 parts: row 2 is the first row of band 1 — the rows above are another band's
    banded = apr.judge(mom, none, n, None, (2, 3, 0), 1, **p)
    assert banded.sum() == 6 and banded[2:4, 29:32].all()


def test_the_rendered_setting_covers_the_cases_on_the_cpu():
    """Over frames 2-4 of the oracle orbit: sky pixels, hit pixels without a prior (disoccluded) and accepted priors all occur, and
    under each rule at least 10 % of the hit pixels end with another count than without the prior — else the GPU comparisons with the
    restatement would prove nothing about the prior."""
    for rule in (0, 1):
        with_p, without = _chain(rule, True), _chain(rule, False)
        assert not with_p[0]["prior"].any()
        assert_same(with_p[0]["spp"], without[0]["spp"], "frame 1 has no history")
        sky = none = accepted = hits = differ = 0
        for a, b in zip(with_p[1:], without[1:]):
            hit = a["aov"]["hits"] > 0
            ch, vh = a["prior"][..., 0], a["prior"][..., 1]
            assert np.isfinite(a["prior"]).all() and (ch >= 0).all() and (vh >= 0).all() and not a["prior"][~hit].any()
            sky += int((~hit).sum())
            none += int((hit & (ch == 0)).sum())
            accepted += int((hit & (ch > 0)).sum())
            hits += int(hit.sum())
            differ += int((hit & (a["spp"] != b["spp"])).sum())
        mean = lambda frames: [round(float(f["spp"].mean()), 3) for f in frames]
        print(f"oracle orbit, rule {rule}, t = {ORBIT_T}: sky {sky}, hit pixels without a prior {none}, accepted priors {accepted}; {differ} of {hits} "
              f"hit pixels ({differ / hits:.3f}) end with another count; mean spp per frame with the prior {mean(with_p)}, without {mean(without)}")
        assert sky > 0 and none > 0 and accepted > 0
        assert differ >= 0.10 * hits


# ---- §24's experiment with the prior ------------------------------------------------------------------------
# rtiow 320 x 180, eight still frames at 4:4:32, t = 0.1, frame k from sample 32 k, with moments, the MSE of the clamped mean against
# 1024 spp from sample 2^20 — computed on the CPU from the restatements alone by tools/adaptive_prior_quality.py
# (profiles/r26/adaptive_prior_quality.json).  Per rule: the samples of every frame with the prior and without, which the device must
# reproduce exactly, and the two ratios prior / no prior the test pins at these values plus 10 %: the samples over frames 2-8 and the MSE
# after frame 8.  At this setting the prior halves the samples and costs quality: the MSE ratios are above 1 (no constant was tuned).
QUALITY_SAMPLES = {
    0: ([1078272, 662736, 590356, 546212, 531720, 526124, 524524, 521360], [1078272, 1081976, 1078540, 1078364, 1079648, 1082372, 1081388, 1080920]),
    1: ([753040, 332184, 294636, 274840, 271112, 265556, 265996, 267992], [753040, 753100, 752788, 750644, 751240, 754136, 752864, 753448]),
}
SAMPLES_RATIO = {0: 0.516055, 1: 0.374380}
MSE_RATIO = {0: 1.587887, 1: 1.609499}          # (MSE after frame 8 with the prior 3.88019e-4 / 3.42256e-4, without 2.44362e-4 / 2.12648e-4)


@functools.lru_cache(maxsize=None)
def _quality_truth():
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    gt, _ = dev.render_to_host(rb.rtiow_camera(320, 180, 1024, 50), sample_first=1 << 20)
    dev.close()
    truth = np.clip(gt / F(1024), 0, 1)
    truth.setflags(write=False)
    return truth


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [0, 1])
def test_saving_and_quality_against_a_1024_spp_ground_truth(rule):
    """Measured, not promised: §24's experiment with the prior and without.  The device reproduces the CPU model's
    samples per frame exactly; the two ratios are pinned at the CPU model's values plus 10 %, so that a regression shows."""
    truth = _quality_truth()
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    cam = rb.rtiow_camera(320, 180, 1, 50)
    aov, _ = dev.render_aov_to_host(_with_spp(cam, A))
    samples, mse = {}, {}
    try:
        for with_prior in (True, False):
            td = rb.TemporalDenoiser(320, 180)
            try:
                samples[with_prior] = []
                for k in range(8):
                    pr = td.prior_to_host(aov, A, cam) if with_prior else None
                    fb, spp, mom, _ = dev.render_lit_adaptive_to_host(cam, emitters=False, sample_first=32 * k, threshold=0.1, rule=rule, prior=pr, **SPP)
                    out = td.step_spp_to_host(fb, spp, mom, aov, A, cam)
                    samples[with_prior].append(int(spp.sum()))
                mse[with_prior] = tdts._mse(out, spp, truth)
            finally:
                td.close()
    finally:
        dev.close()
    s_ratio, m_ratio = sum(samples[True][1:]) / sum(samples[False][1:]), mse[True] / mse[False]
    print(f"rule {rule}: mean spp per frame with the prior {[round(x / 57600, 2) for x in samples[True]]}, without "
          f"{[round(x / 57600, 2) for x in samples[False]]}; samples over frames 2-8 ratio {s_ratio:.4f}; MSE after frame 8 with the prior "
          f"{mse[True]:.6g}, without {mse[False]:.6g}, ratio {m_ratio:.4f}")
    assert (samples[True], samples[False]) == QUALITY_SAMPLES[rule]
    assert s_ratio <= 1.1 * SAMPLES_RATIO[rule]
    assert m_ratio <= 1.1 * MSE_RATIO[rule]


# ---- on the GPU ----------------------------------------------------------------------------------------------------------

def _upload(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")          # (a copy: the shared arrays are read-only)


def _aov_tensors(aov):
    return {key: _upload(aov[key].view(np.float32) if dtype != np.float32 else aov[key]) for key, _, dtype, _ in rb.AOV_CHANNELS}


def _device_prior(aov, cam, history, stream=None, fill=float("nan")):
    """rb.adaptive_prior over a host history (None: NULL) into a buffer filled with `fill`."""
    import torch
    t = _aov_tensors(aov)
    d_hist = None if history is None else _upload(history)
    out = torch.full((cam.image_height, cam.image_width, 2), fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rb.adaptive_prior({k: v.data_ptr() for k, v in t.items()}, A, cam, None if d_hist is None else d_hist.data_ptr(),
                      0 if d_hist is None else d_hist.numel(), out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
def test_prior_from_device_histories_with_a_reset():
    """TemporalDenoiser.prior on the histories the device itself wrote, frame by frame, with a reset after frame 2."""
    rb.amd_lib().rt_set_device(0)
    frames = _chain(0, False)
    td = rb.TemporalDenoiser(W, H)
    prev = None
    try:
        for n, f in enumerate(frames):
            if n == 2:
                td.reset()
                prev = None
            got = td.prior_to_host(f["aov"], A, f["cam"])
            assert_same(got, apr.prior(f["aov"], A, f["cam"], prev), f"prior of frame {n}")
            assert got.any() == (prev is not None)
            td.step_spp_to_host(f["fb"], f["spp"], f["mom"], f["aov"], A, f["cam"])
            _, prev = dtsr.reference(f["fb"], f["spp"], f["mom"], f["aov"], A, f["cam"], prev)
            assert_same(td.history_to_host(), prev, f"history of frame {n}")
    finally:
        td.close()


@pytest.mark.gpu
def test_prior_sub_images_empty_histories_and_a_camera_that_looks_away():
    rb.amd_lib().rt_set_device(0)
    frames = _chain(0, False)
    full = [(f["fb"], f["spp"], f["mom"], f["aov"], f["cam"]) for f in frames[:2]]
    for what, ys, xs in (("45x1 column", slice(None), slice(30, 31)), ("1x77 row", slice(22, 23), slice(None)), ("1x1", slice(22, 23), slice(40, 41))):
        (fb, spp, mom, aov, cam), (_, _, _, aov1, cam1) = [tdts._cut(f, ys, xs) for f in full]
        assert (aov1["hits"] > 0).any()
        _, hist = dtsr.reference(fb, spp, mom, aov, A, cam, None)
        want = apr.prior(aov1, A, cam1, hist)
        assert_same(_device_prior(aov1, cam1, hist), want, what)
        assert want.any() or what == "1x1"
    f0, f1 = frames[0], frames[1]
    zero = np.zeros_like(f0["hist"])
    other = f0["hist"].copy()
    other.view(np.int32)[1] = W + 1
    old = f0["hist"].copy()
    old.view(np.uint32)[0] = tdts.OLD_MAGIC
    spatial = dtsr.reference(f0["fb"], f0["spp"], None, f0["aov"], A, f0["cam"], None)[1]
    for prev, what in ((None, "NULL"), (zero, "all zero"), (other, "another size"), (old, "rt_denoise_temporal's magic"), (spatial, "mode 1")):
        assert not _device_prior(f1["aov"], f1["cam"], prev).view(np.uint32).any(), what
    away = rb.make_camera(W, H, 20.0, (-50, 3, 0), (-100, 3, 0), (0.7, 0.8, 1.0), 1, 50)
    looked = _rehead(f0["hist"], away)
    assert_same(_device_prior(f1["aov"], f1["cam"], looked), apr.prior(f1["aov"], A, f1["cam"], looked), "a camera that looks away")
    assert not _device_prior(f1["aov"], f1["cam"], looked).any()


@pytest.mark.gpu
def test_prior_on_a_side_stream_into_a_nan_filled_buffer():
    import torch
    rb.amd_lib().rt_set_device(0)
    w, h = 200, 120
    frames = tdts._still_frames(w, h, 2)
    (fb, spp, mom, aov, cam), (_, _, _, aov1, cam1) = frames
    _, hist = dtsr.reference(fb, spp, mom, aov, A, cam, None)
    want = apr.prior(aov1, A, cam1, hist)
    assert (want[..., 0] > 0).any() and not want[aov1["hits"] == 0].any()
    stream = torch.cuda.Stream()
    for run in range(2):
        with torch.cuda.stream(stream):
            got = _device_prior(aov1, cam1, hist, stream=stream.cuda_stream)
        assert_same(got, want, f"side stream, run {run}")


def _judge_moments(rng, rows, width, n):
    """Moments of n samples per pixel: quiet and noisy pixels mixed, then NaN, zero, huge and negative ones sprinkled in."""
    y = np.where(rng.random((rows, width, 1)) < 0.3, rng.uniform(0, 4, (rows, width, n)), rng.uniform(0.4, 0.6, (rows, width, 1)) + np.zeros(n)).astype(F)
    s1, s2 = np.zeros((rows, width), F), np.zeros((rows, width), F)
    for s in range(n):
        s1 = (s1 + y[..., s]).astype(F)
        s2 = (s2 + (y[..., s] * y[..., s]).astype(F)).astype(F)
    mom = np.stack([s1, s2], axis=-1)
    special = np.array([[np.nan, 1], [1, np.nan], [0, 0], [3e38, 3e38], [np.inf, np.inf], [1e-30, 1e-38], [-4, 8]], F)
    k = rows * width // 8
    at = rng.choice(rows * width, k, replace=False)
    mom.reshape(-1, 2)[at] = special[rng.integers(0, len(special), k)]
    return mom


def _judge_priors(rng, rows, width):
    """Priors nobody reprojected: none, counts from below one sample to far past the floor, variances from 0 to huge, and the values
    that must fall back to the pixel's own samples."""
    ch = np.where(rng.random((rows, width)) < 0.3, 0, rng.choice([0.5, 4, 8, 31.5, 64, 1e6], (rows, width))).astype(F)
    vh = (rng.choice([0, 1e-6, 1e-3, 0.05, 1.0, 1e30], (rows, width)) * rng.uniform(0.5, 1.5, (rows, width))).astype(F)
    pr = np.stack([ch, vh], axis=-1)
    special = np.array([[np.nan, 0], [8, np.nan], [-8, 0], [8, -1], [np.inf, 1], [8, np.inf], [-0.0, 5]], F)
    k = rows * width // 8
    at = rng.choice(rows * width, k, replace=False)
    pr.reshape(-1, 2)[at] = special[rng.integers(0, len(special), k)]
    return pr


@pytest.mark.gpu
def test_judge_prior_against_the_restatement():
    """67 x 6 pixels in bands of 2 rows over 3 parts (and the whole frame): first-judgement masks and list masks, both rules, the cap
    and t = 0; a zero prior and no prior are rt_adaptive_judge's result."""
    rb.amd_lib().rt_set_device(0)
    rows, width, n = 6, 67, 8
    rng = np.random.default_rng(26)
    mom, pr = _judge_moments(rng, rows, width, n), _judge_priors(rng, rows, width)
    masks = [None, rng.random((rows, width)) < 0.7, rng.random((rows, width)) < 0.1, np.zeros((rows, width), bool)]
    changed = 0
    for triple in ((2, 3, 1), None):
        shard = rb.Shard(*triple) if triple else None
        for mask in masks:
            for t, max_spp in ((0.05, 64), (0.3, 64), (0.0, 64), (0.05, 11), (0.05, 12)):
                p = dict(min_spp=4, batch_spp=4, max_spp=max_spp, threshold=t)
                for rule in (0, 1):
                    got = rb.adaptive_judge(mom, n, mask, shard=shard, rule=rule, prior=pr, **p)
                    want = apr.judge(mom, pr, n, mask, triple, rule, **p)
                    assert np.array_equal(got, want), (triple, rule, t, max_spp, np.argwhere(got != want)[:5])
                    plain = rb.adaptive_judge(mom, n, mask, shard=shard, rule=rule, **p)
                    assert np.array_equal(rb.adaptive_judge(mom, n, mask, shard=shard, rule=rule, prior=np.zeros_like(pr), **p), plain), "a zero prior"
                    changed += int((got != plain).sum())
    assert changed > 100, "the priors decide"


@pytest.mark.gpu
def test_judge_prior_silences_the_noisy_pixel_on_the_device():
    rb.amd_lib().rt_set_device(0)
    rows, width, n = 6, 67, 8
    s1 = np.full((rows, width), F(0.5) * F(n), F)
    s2 = np.full((rows, width), F(0.25) * F(n), F)
    s1[2, 30], s2[2, 30] = F(4) * F(n // 2), F(16) * F(n // 2)
    mom = np.stack([s1, s2], axis=-1)
    p = dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.2)
    for triple in (None, (2, 3, 0)):
        shard = rb.Shard(*triple) if triple else None
        for at, quiet in (((2, 30), True), ((2, 31), False)):
            pr = np.zeros((rows, width, 2), F)
            pr[at] = (1e6, 0)
            lists = np.arange(rows * width).reshape(rows, width) % 7 != 5          # (the noisy pixel is 2 * 67 + 30 = 164 = 3 mod 7: listed)
            assert lists[2, 30] and lists[2, 31]
            for mask in (None, lists):          # every pixel, and a list that holds the noisy one
                got = rb.adaptive_judge(mom, n, mask, shard=shard, rule=1, prior=pr, **p)
                assert np.array_equal(got, apr.judge(mom, pr, n, mask, triple, 1, **p)), (triple, at)
                assert got.any() != quiet, (triple, at)


def _check_triple(got, want, what):
    for g, w_, col in zip(got[:3], want, ("fb", "spp", "moments")):
        assert_same(g, w_, f"{what}: {col}")


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [0, 1])
def test_render_adaptive_prior_frame_by_frame(rule):
    """The orbit through rt_render_adaptive_prior with the restated prior of each frame: d_fb_sum, d_spp and d_moments are
    from_radiances' with that prior; the zero-prior and NULL-prior frames are the _rule call's, device against device."""
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    p = dict(threshold=ORBIT_T, rule=rule, **SPP)
    try:
        for n, f in enumerate(_chain(rule, True)):
            got = dev.render_adaptive_to_host(f["cam"], prior=f["prior"], **p)
            _check_triple(got, (f["fb"], f["spp"], f["mom"]), f"rule {rule}, frame {n}")
            if n in (0, 2):
                plain = dev.render_adaptive_to_host(f["cam"], **p)
                _check_triple(dev.render_adaptive_to_host(f["cam"], prior=np.zeros((H, W, 2), F), **p), plain, "a zero prior = the _rule call")
                if n == 2:
                    assert (got[1] != plain[1]).any(), "the prior decides"
    finally:
        dev.close()


@pytest.mark.gpu
def test_render_adaptive_prior_null_shard_stream_and_replay():
    import torch
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    cam = _orbit_cam(1)
    rad = _orbit_radiances()[1]
    rng = np.random.default_rng(9)
    try:
        # d_prior == NULL through the new entry point is the _rule call
        for rule in (0, 1):
            p = dict(threshold=ORBIT_T, **SPP)
            plain = dev.render_adaptive_to_host(cam, rule=rule, **p)
            d_fb = torch.full((H, W, 3), float("nan"), device="cuda:0")
            d_spp = torch.full((H, W), -1, dtype=torch.int32, device="cuda:0")
            d_mom = torch.full((H, W, 2), float("nan"), device="cuda:0")
            ap, stop = rb.adaptive_params(**p), rb.stop_params(rule=rule)
            torch.cuda.synchronize()
            assert lib.rt_render_adaptive_prior(dev._h, C.byref(cam), None, C.byref(ap), C.byref(stop), C.c_void_p(d_fb.data_ptr()),
                                                C.c_void_p(d_spp.data_ptr()), C.c_void_p(d_mom.data_ptr()), None, 1, None, None) == OK
            _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), plain, f"NULL prior, rule {rule}")
        # one shard (bands of 4 rows, part 1 of 2) with a synthetic prior: the part's rows, compacted like d_spp
        shard = rb.Shard(4, 2, 1)
        import emit_reference as er
        rows = er.image_rows(cam, shard)
        pr = _judge_priors(rng, len(rows), W)
        for rule in (0, 1):
            got = dev.render_adaptive_to_host(cam, shard=shard, prior=pr, threshold=ORBIT_T, rule=rule, **SPP)
            want = apr.from_radiances(rad[rows], (4, 2, 1), threshold=ORBIT_T, rule=rule, pr=pr, **SPP)
            _check_triple(got, want, f"shard, rule {rule}")
            assert (want[1] != arr.from_radiances(rad[rows], (4, 2, 1), threshold=ORBIT_T, rule=rule, **SPP)[1]).any()
        # sync = 0 on a torch stream, and the same call again
        pr = _judge_priors(rng, H, W)
        want = apr.from_radiances(rad, None, threshold=ORBIT_T, rule=1, pr=pr, **SPP)
        d_pr = _upload(pr)
        stream = torch.cuda.Stream()
        for run in range(2):
            d_fb = torch.full((H, W, 3), float("nan"), device="cuda:0")
            d_spp = torch.full((H, W), -1, dtype=torch.int32, device="cuda:0")
            d_mom = torch.full((H, W, 2), float("nan"), device="cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                dev.render_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), d_mom.data_ptr(), stream=stream.cuda_stream, sync=False, prior=d_pr.data_ptr(),
                                    threshold=ORBIT_T, rule=1, **SPP)
            stream.synchronize()
            _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), want, f"side stream without sync, run {run}")
        # max_depth <= 0: the prior is not read
        flat = rb.CameraData.from_buffer_copy(cam)
        flat.max_depth = 0
        fbz, sppz, momz, _ = dev.render_adaptive_to_host(flat, prior=pr, threshold=ORBIT_T, rule=1, **SPP)
        assert not fbz.any() and not momz.any() and (sppz == SPP["min_spp"]).all()
    finally:
        dev.close()


@pytest.mark.gpu
def test_render_lit_adaptive_prior():
    """The still camera with every light off at sample_first = 32 k, at 77 x 45, against the restatement, the priors from the device's
    own histories; with each of those priors the call from sample 0 equals the unlit call; §19's setting d at 32 x 24 without its lens
    against the restatement."""
    rb.amd_lib().rt_set_device(0)
    rng = np.random.default_rng(19)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    cam = rb.rtiow_camera(W, H, 1, 50)
    td = rb.TemporalDenoiser(W, H)
    try:
        aov, _ = dev.render_aov_to_host(_with_spp(cam, A))
        for k in range(3):
            pr = td.prior_to_host(aov, A, cam)
            assert pr.any() == (k > 0)
            for rule in (0, 1):
                p = dict(threshold=ORBIT_T, rule=rule, **SPP)
                lit = dev.render_lit_adaptive_to_host(cam, emitters=False, sample_first=32 * k, prior=pr, **p)
                rad = lar.radiances(rb.HostScene.rtiow(), cam, SPP["max_spp"], sample_first=32 * k, emitters=False)
                _check_triple(lit, apr.from_radiances(rad, None, threshold=ORBIT_T, rule=rule, pr=pr, **SPP), f"lights off, frame {k}, rule {rule}")
                # the unlit call has no sample_first: it takes the samples the lit call takes from sample 0, whatever the prior's frame
                lit0 = lit if k == 0 else dev.render_lit_adaptive_to_host(cam, emitters=False, prior=pr, **p)
                _check_triple(dev.render_adaptive_to_host(cam, prior=pr, **p), lit0, f"the unlit call with the prior of frame {k}, rule {rule}")
                if k == 0:
                    _check_triple(dev.render_lit_adaptive_to_host(cam, emitters=False, **p), lit, "no history yet: the _rule call")
            td.step_spp_to_host(lit[0], lit[1], lit[2], aov, A, cam)
    finally:
        td.close()
        dev.close()
    name = lar.SETTINGS["d"][0]
    host, cam = tl.scene(name), tl.camera(name, *lar.SIZE, 1)
    pr = _judge_priors(rng, lar.SIZE[1], lar.SIZE[0])
    with rb.Env(lar.sky()) as env:
        kw = lar.device_keywords("d", env)
        kw.pop("lens")
        ref_kw = lar.reference_keywords("d")
        ref_kw.pop("lens", None)
        dev = rb.DeviceScene(host, device=0)
        try:
            rad = lar.radiances(host, cam, lar.SPP["max_spp"], **ref_kw)
            for rule in (0, 1):
                got = dev.render_lit_adaptive_to_host(cam, threshold=lar.THRESHOLD, rule=rule, prior=pr, **lar.SPP, **kw)
                want = apr.from_radiances(rad, None, threshold=lar.THRESHOLD, rule=rule, pr=pr, **lar.SPP)
                _check_triple(got, want, f"setting d without its lens, rule {rule}")
                assert (want[1] != arr.from_radiances(rad, None, threshold=lar.THRESHOLD, rule=rule, **lar.SPP)[1]).any()
        finally:
            dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [0, 1])
def test_the_whole_loop_against_the_chained_cpu_model(rule):
    """TemporalDenoiser.prior → render → step_spp on device buffers for four frames: priors, frames, outputs and histories."""
    import torch
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    td = rb.TemporalDenoiser(W, H)
    d_fb = torch.empty((H, W, 3), device="cuda:0")
    d_spp = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
    d_mom, d_pr, d_out = torch.empty((H, W, 2), device="cuda:0"), torch.empty((H, W, 2), device="cuda:0"), torch.empty((H, W, 3), device="cuda:0")
    d_aov = {key: torch.empty((H, W) + ((3,) if n == 3 else ()), dtype=torch.float32, device="cuda:0") for key, _, _, n in rb.AOV_CHANNELS}
    ptrs = {k: v.data_ptr() for k, v in d_aov.items()}
    try:
        for n, f in enumerate(_chain(rule, True)):
            cam = f["cam"]
            dev.render_aov(_with_spp(cam, A), ptrs)
            td.prior(ptrs, A, cam, d_pr.data_ptr())
            dev.render_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), d_mom.data_ptr(), prior=d_pr.data_ptr(), threshold=ORBIT_T, rule=rule, **SPP)
            td.step_spp(d_fb.data_ptr(), d_spp.data_ptr(), d_mom.data_ptr(), ptrs, A, cam, d_out.data_ptr())
            torch.cuda.synchronize()
            assert_same(d_pr.cpu().numpy(), f["prior"], f"prior of frame {n}")
            _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), (f["fb"], f["spp"], f["mom"]), f"frame {n}")
            assert_same(d_out.cpu().numpy(), f["out"], f"output of frame {n}")
            assert_same(td.history_to_host(), f["hist"], f"history of frame {n}")
    finally:
        td.close()
        dev.close()


@pytest.mark.gpu
def test_cli_stop_history_writes_the_python_paths_files(test_config_text, tmp_path):
    import torch
    lines = test_config_text.split("\n")
    lines[0] = "3"
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    out = subprocess.run([EXE, "--gpu", "--adaptive", "0.3", "--adaptive-spp", "4:4:32", "--denoise-adaptive-temporal", "--stop-history"], input=text,
                         capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.from_config(text)
    dev = rb.DeviceScene(host, device=0)
    cam0 = host.frame_camera(0)
    td = rb.TemporalDenoiser(cam0.image_width, cam0.image_height)

    def file_bytes(frame, spp, cam):
        d_fb, d_spp = torch.from_numpy(np.ascontiguousarray(frame)).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
        rgb = torch.zeros(frame.shape, dtype=torch.uint8, device="cuda:0")
        assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == 0
        torch.cuda.synchronize()
        return np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes()
    try:
        saved = 0
        for n in range(3):
            cam = _with_spp(host.frame_camera(n), A)
            aov, _ = dev.render_aov_to_host(cam)
            pr = td.prior_to_host(aov, A, cam)
            fb, spp, mom, _ = dev.render_adaptive_to_host(cam, threshold=0.3, prior=pr, **SPP)
            got = td.step_spp_to_host(fb, spp, mom, aov, A, cam)
            assert open(tmp_path / f"f_{n}.png.denoised", "rb").read() == file_bytes(got, spp, cam), n
            assert open(tmp_path / f"f_{n}.png", "rb").read() == file_bytes(fb, spp, cam), n
            saved += int((spp != dev.render_adaptive_to_host(cam, threshold=0.3, **SPP)[1]).sum())
        assert saved > 0, "the prior changed counts"
        # the lit path
        lines[0] = "2"
        lines[1] = str(tmp_path / "lit_%d.png")
        text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
        out = subprocess.run([EXE, "--gpu", "--lit", "--nee", "--light-tree", "--noise-target", "0.3", "--noise-spp", "4:4:32", "--denoise-adaptive-temporal",
                              "--stop-history"], input=text, capture_output=True, text=True, timeout=200)
        assert out.returncode == 0, out.stderr
        td.reset()
        for n in range(2):
            cam = host.frame_camera_at(float(n))
            aov, _ = dev.render_aov_to_host(_with_spp(cam, A))
            pr = td.prior_to_host(aov, A, cam)
            fb, spp, mom, _ = dev.render_lit_adaptive_to_host(cam, nee=dict(select=1), threshold=0.3, prior=pr, **SPP)
            got = td.step_spp_to_host(fb, spp, mom, aov, A, cam)
            assert open(tmp_path / f"lit_{n}.png.denoised", "rb").read() == file_bytes(got, spp, cam), f"lit frame {n}"
            assert open(tmp_path / f"lit_{n}.png", "rb").read() == file_bytes(fb, spp, cam), f"lit frame {n}"
    finally:
        td.close()
        dev.close()
