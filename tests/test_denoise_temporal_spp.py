"""rt_denoise_temporal_spp: rt_denoise_temporal for adaptively sampled frames — the history blended with the frame by the samples
behind each, the variance of the blend propagated through it (include/rtp_amd.h).  The device output and the whole
history buffer are compared byte for byte with the C restatement of the header's arithmetic
(tests/denoise_temporal_spp_reference.py) over sequences of rendered adaptive frames (the pinhole path and the lit path), their
sub-images, synthetic inputs at the edges of the contract, mixed calls on shared buffers, a replay, a side stream and the CLI's files;
the restatement itself is checked for the header's identities; and the quality against a 1024-spp ground truth is measured and pinned.
On the CPU: the ABI, every refusal (they come before any HIP call, so fake addresses do), the identities and the CLI's refusals."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_spp_reference as dsr
import denoise_temporal_reference as dtr
import denoise_temporal_spp_reference as dtsr
import lit_adaptive_reference as lar
import rtp_bindings as rb
import test_adaptive as ta
import test_denoise_spp as tds
import test_light_tree as tl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
FAKE = 1 << 32          # a device address that is never dereferenced: every check comes before any HIP call
INVALID, UNSUPPORTED = 1, 4
F = np.float32
SPP = dict(min_spp=4, batch_spp=4, max_spp=32)
A = SPP["min_spp"]                                  # the AOVs' samples per pixel
LEVELS = tuple(range(SPP["min_spp"], SPP["max_spp"] + 1, SPP["batch_spp"]))
THRESHOLD = 0.3
OTHER = dict(iterations=3, sigma_depth=0.25, sigma_luminance=40.0, normal_squarings=2)      # one non-default set
MIN_ALPHA = F(0.2)
OLD_MAGIC = 0x31485452
assert_same = ta.assert_same


# ---- no GPU needed: the ABI and the refusals --------------------------------------------------------------------------

def test_abi_symbol_argtypes_and_functions():
    lib = rb.amd_lib()
    assert hasattr(lib, "rt_denoise_temporal_spp") and "rt_denoise_temporal_spp" in rb.RTP_AMD_SYMBOLS
    at = lib.rt_denoise_temporal_spp.argtypes
    assert len(at) == 14 and at[4] is C.c_int32 and at[9] is C.c_uint64 and at[11] is C.c_uint64
    assert at[3]._type_ is rb.AovBuffers and at[5]._type_ is rb.CameraData and at[6]._type_ is rb.DenoiseParams
    assert callable(rb.denoise_temporal_spp) and callable(rb.TemporalDenoiser.step_spp) and callable(rb.TemporalDenoiser.step_spp_to_host)
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        text = f.read()
    assert "rt_status rt_denoise_temporal_spp(" in text and "0x32485452" in text
    assert dtsr.MAGIC == 0x32485452 != OLD_MAGIC
    assert rb.amd_lib().rt_version_string().decode().startswith("rtp_amd 0.5")


W8, H4 = 8, 4
PIX = W8 * H4
# fake addresses: fb 1, albedo 2, normal 3, depth 4, hits 5, prim 6, workspace 7, out 8, prev 9, next 10, spp 11, moments 12 (x FAKE)


def _aov(**drop):
    b = rb.AovBuffers()
    b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count, b.first_prim = 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE, 6 * FAKE
    for field in drop:
        setattr(b, field, None)
    return b


def _cam(**fields):
    cam = rb.make_camera(W8, H4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4)
    for k, v in fields.items():
        setattr(cam, k, v)
    return cam


def _call(fb=FAKE, spp=11 * FAKE, mom=12 * FAKE, aov="full", aov_spp=4, cam="default", params=None, prev=9 * FAKE, nxt=10 * FAKE, hist_bytes=None,
          ws=7 * FAKE, ws_bytes=None, out=8 * FAKE):
    lib = rb.amd_lib()
    if aov == "full":
        aov = _aov()
    if cam == "default":
        cam = _cam()
    w, h = (cam.image_width, cam.image_height) if cam is not None else (W8, H4)
    hist_bytes = lib.rt_denoise_history_bytes(w, h) if hist_bytes is None else hist_bytes
    ws_bytes = lib.rt_denoise_workspace_bytes(w, h) if ws_bytes is None else ws_bytes
    st = lib.rt_denoise_temporal_spp(C.c_void_p(fb), C.c_void_p(spp), C.c_void_p(mom), C.byref(aov) if aov is not None else None, aov_spp,
                                     C.byref(cam) if cam is not None else None, C.byref(params) if params else None, C.c_void_p(prev),
                                     C.c_void_p(nxt), hist_bytes, C.c_void_p(ws), ws_bytes, C.c_void_p(out), None)
    return st, lib.rt_get_last_error_string().decode()


def test_refusals_need_no_device():
    lib = rb.amd_lib()
    hist = lib.rt_denoise_history_bytes(W8, H4)
    need = lib.rt_denoise_workspace_bytes(W8, H4)
    # rt_denoise_temporal's cases …
    cases = [dict(fb=0), dict(aov=None), dict(cam=None), dict(nxt=0), dict(ws=0), dict(out=0),
             dict(cam=_cam(image_width=0)), dict(cam=_cam(image_height=-3)), dict(ws_bytes=need - 1), dict(hist_bytes=hist - 1),
             dict(prev=9 * FAKE + 4), dict(nxt=10 * FAKE + 8),
             dict(nxt=9 * FAKE + hist - 16), dict(nxt=9 * FAKE - hist + 16), dict(nxt=6 * FAKE + 4 * PIX - 16), dict(nxt=FAKE + 368),
             dict(nxt=7 * FAKE + need - 16), dict(nxt=8 * FAKE + 12 * PIX - 16),
             dict(out=6 * FAKE + 4), dict(out=2 * FAKE + 12), dict(out=7 * FAKE + 100), dict(out=9 * FAKE + hist - 4),
             dict(ws=5 * FAKE + 124), dict(ws=9 * FAKE + 64),
             # … d_spp required, aov_samples where samples_per_pixel was
             dict(spp=0), dict(aov_spp=0), dict(aov_spp=65537), dict(aov_spp=-4)]
    for field in ("albedo_sum", "normal_sum", "depth_sum", "hit_count", "first_prim"):
        cases.append(dict(aov=_aov(**{field: 1})))
    short = _aov()
    short.struct_bytes = 40                                           # first_prim lies past struct_bytes: it counts as NULL
    cases.append(dict(aov=short))
    for field, bad in (("iterations", -1), ("iterations", 9), ("sigma_depth", 0.0), ("sigma_depth", float("nan")), ("sigma_luminance", 0.0),
                       ("sigma_luminance", float("inf")), ("normal_squarings", -1), ("normal_squarings", 11), ("struct_bytes", 4)):
        p = rb.denoise_params()
        setattr(p, field, bad)
        cases.append(dict(params=p))
    for kw in cases:
        st, msg = _call(**kw)
        assert st == INVALID and msg.startswith("rt_denoise_temporal_spp:"), (kw, st, msg)
    for kw, word in ((dict(spp=0), "null"), (dict(aov_spp=0), "aov_samples"), (dict(aov=_aov(first_prim=1)), "first_prim"),
                     (dict(prev=9 * FAKE + 4), "16-byte aligned"), (dict(nxt=10 * FAKE + 8), "16-byte aligned"),
                     (dict(hist_bytes=hist - 1), "history_bytes"), (dict(ws_bytes=need - 1), "workspace_bytes")):
        assert word in _call(**kw)[1], (kw, _call(**kw))
    # cam's samples_per_pixel is ignored: 0 and 65537 pass that check and fail a later one
    for s in (0, 65537, -1):
        st, msg = _call(cam=_cam(samples_per_pixel=s), hist_bytes=hist - 1)
        assert st == INVALID and "history_bytes" in msg, (s, st, msg)
    for w, h in ((4097, 4096), (1 << 24, 2)):
        st, msg = _call(cam=_cam(image_width=w, image_height=h))
        assert st == UNSUPPORTED and "2^24" in msg and msg.startswith("rt_denoise_temporal_spp:"), (w, h, st, msg)
    # what is allowed passes its check and fails a later one (nothing here may reach a launch: the addresses are fake)
    for kw in (dict(prev=0), dict(mom=0), dict(aov_spp=65536), dict(aov_spp=1), dict(params=rb.denoise_params(iterations=0)),
               dict(params=rb.denoise_params(iterations=8, normal_squarings=10)),
               dict(cam=_cam(image_width=4096, image_height=4096), ws_bytes=1 << 40)):
        st, msg = _call(hist_bytes=hist - 1, **kw)
        assert st == INVALID and "history_bytes" in msg, (kw, st, msg)


def test_overlaps_with_the_counts_and_the_moments_to_the_byte():
    """d_spp is 4 bytes per pixel and d_moments 8 in every overlap check: the last byte that overlaps is refused with that check's text,
    the first that does not passes it and fails a later check (d_out over the workspace, which comes after every check of an input)."""
    lib = rb.amd_lib()
    hist = lib.rt_denoise_history_bytes(W8, H4)
    need = lib.rt_denoise_workspace_bytes(W8, H4)
    late = dict(out=7 * FAKE + 100)                                    # "d_out overlaps the workspace"
    for base, size in ((11 * FAKE, 4 * PIX), (12 * FAKE, 8 * PIX)):
        for kw, word in ((dict(nxt=base + size - 16), "history_next overlaps an input"), (dict(nxt=base - hist + 16), "history_next overlaps an input"),
                         (dict(out=base + size - 1), "d_out overlaps an input"), (dict(out=base - 12 * PIX + 1), "d_out overlaps an input"),
                         (dict(ws=base + size - 1), "the workspace overlaps an input"), (dict(ws=base - need + 1), "the workspace overlaps an input")):
            st, msg = _call(**kw)
            assert st == INVALID and msg == "rt_denoise_temporal_spp: " + word, (hex(base), kw, st, msg)
        for kw in (dict(nxt=base + size), dict(nxt=base - hist)):
            st, msg = _call(**late, **kw)
            assert st == INVALID and msg.endswith("d_out overlaps the workspace"), (hex(base), kw, st, msg)
        for kw in (dict(out=base + size), dict(out=base - 12 * PIX), dict(ws=base + size), dict(ws=base - need)):
            st, msg = _call(nxt=8 * FAKE + 12 * PIX - 16 if "ws" in kw else 7 * FAKE + need - 16, **kw)     # a later check: history_next over d_out / the workspace
            assert st == INVALID and "history_next overlaps " in msg and "input" not in msg, (hex(base), kw, st, msg)
    # without moments their range is nobody's: d_out, the workspace or history_next there passes every check of an input and is refused
    # by a later one, placed on purpose (no call of this file may pass all checks: the addresses are fake)
    st, msg = _call(mom=0, out=12 * FAKE, ws=12 * FAKE + 16)
    assert st == INVALID and msg == "rt_denoise_temporal_spp: d_out overlaps the workspace", (st, msg)
    st, msg = _call(mom=0, ws=12 * FAKE + 16, nxt=8 * FAKE + 16)
    assert st == INVALID and msg == "rt_denoise_temporal_spp: history_next overlaps d_out", (st, msg)
    st, msg = _call(mom=0, nxt=12 * FAKE, out=7 * FAKE + 100)
    assert st == INVALID and msg == "rt_denoise_temporal_spp: d_out overlaps the workspace", (st, msg)


def test_the_order_of_the_checks():
    """Arguments, AOV buffers, image size, aov_samples, parameters, pixel limit, workspace, history size, alignment, overlaps."""
    bad = rb.denoise_params(iterations=9)
    big = _cam(image_width=1 << 24, image_height=2)
    rest = dict(ws_bytes=0, hist_bytes=0, prev=9 * FAKE + 4, out=FAKE)
    assert "null" in _call(spp=0, aov=_aov(first_prim=1), cam=_cam(image_width=0), aov_spp=0, params=bad, **rest)[1]
    assert "first_prim are required" in _call(aov=_aov(first_prim=1), cam=_cam(image_width=0), aov_spp=0, params=bad, **rest)[1]
    assert "width and height" in _call(cam=_cam(image_width=0), aov_spp=0, params=bad, **rest)[1]
    assert "aov_samples" in _call(cam=big, aov_spp=0, params=bad, **rest)[1]
    assert "iterations" in _call(cam=big, params=bad, **rest)[1]
    assert "2^24" in _call(cam=big, **rest)[1]
    assert "workspace_bytes" in _call(**rest)[1]
    assert "history_bytes" in _call(**{**rest, "ws_bytes": None})[1]
    assert "16-byte aligned" in _call(prev=9 * FAKE + 4, out=FAKE)[1]
    assert "d_out overlaps an input" in _call(out=FAKE, ws=9 * FAKE + 64)[1]
    # per input: history_next, then d_out, then the workspace
    assert "history_next overlaps an input" in _call(nxt=11 * FAKE, out=11 * FAKE, ws=11 * FAKE)[1]
    assert "d_out overlaps an input" in _call(out=11 * FAKE, ws=11 * FAKE)[1]


def test_cli_refusals(test_config_text, tmp_path):
    before = sorted(os.listdir(tmp_path))
    flag = "--denoise-adaptive-temporal"

    def run(args, env=None):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                              env={**os.environ, **(env or {})})
    ad, lit = ["--adaptive", "0.3"], ["--lit", "--noise-target", "0.3"]
    runs = [([flag], None), (["--denoise", flag], None), (["--nee", flag], None), (["--lit", flag], None), (["--noise-target", "0.3", flag], None),
            (["--lens", "0.1:10", flag], None), (ad + [flag], {"RTP_DEVICES": "2"}), (lit + [flag], {"RTP_DEVICES": "1"})]
    for mode in (ad, lit):
        runs += [(mode + [flag, extra], None) for extra in ("--denoise", "--denoise-temporal", "--denoise-adaptive", "--aov")]
        runs += [(mode + [flag, *extra], None) for extra in (["--lens", "0.1:10"], ["--motion-blur", "0.5"], ["--devices", "2"], ["--shard", "2"])]
    # with several of them at once, or with a flag whose own refusal would come first, the message still names this flag
    runs += [(ad + ["--denoise-adaptive", flag, extra], None) for extra in ("--denoise-temporal", "--aov", "--denoise")]
    runs += [(lit + ["--denoise-adaptive", flag, "--denoise-temporal"], None), (["--denoise-adaptive", flag], None),
             (ad + [flag, "--denoise", "--denoise-temporal"], None), (ad + [flag, "--aov", "--devices", "2"], None)]
    for args, env in runs:
        r = run(args, env)
        assert r.returncode == 2 and flag in r.stderr, (args, env, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    # the refusals that were there stay what they were
    r = run(["--adaptive", "0.3", "--denoise-adaptive", "--denoise-temporal"])
    assert r.returncode == 2 and "--denoise-adaptive writes" in r.stderr and flag not in r.stderr, (r.returncode, r.stderr)
    r = run(["--adaptive", "0.1", "--denoise-temporal"])
    assert r.returncode == 2 and "--adaptive renders frame after frame" in r.stderr and flag not in r.stderr, (r.returncode, r.stderr)
    r = run(["--lit", "--denoise-temporal"])
    assert r.returncode == 99 and "--lit renders frame after frame" in r.stderr, (r.returncode, r.stderr)


# ---- the restatement's identities (synthetic frames) ---------------------------------------------------------------------

def _synthetic_cam(w=130, h=9, away=False):
    return rb.make_camera(w, h, 40.0, (-50, 0, 0) if away else (0, 0, 0), (-100, 0, 0) if away else (-1, 0, 0), (0.2, 0.3, 0.4), 1, 8)


@functools.lru_cache(maxsize=None)
def _synthetic_frames():
    """Two frames of tests/test_denoise_spp.py's synthetic inputs (130 x 9: sky holes and a sky column on the tile boundary, counts from
    {0, 1, 2, 3, 17, 65536}, zero and clamped moments) over the same surfaces — the first frame's AOVs with a primitive id per 8-pixel
    block — so that a still camera reprojects every pixel onto itself.  Shared: do not write to them."""
    fb, spp, mom, aov, a = tds._synthetic()
    fb2, spp2, mom2, _, _ = tds._synthetic(seed=12)
    h, w = spp.shape
    aov = {**aov, "prim": np.broadcast_to((np.arange(w, dtype=np.int32) // 8)[None, :], (h, w)).copy()}
    for arr in (fb, spp, mom, fb2, spp2, mom2, *aov.values()):
        arr.setflags(write=False)
    return (fb, spp, mom, aov), (fb2, spp2, mom2, aov), a


def test_reference_empty_history_is_rt_denoise_spp():
    (fb, spp, mom, aov), (fb2, spp2, mom2, _), a = _synthetic_frames()
    cam = _synthetic_cam()
    w, h = cam.image_width, cam.image_height
    # real histories of this size made unusable: all-zero, rt_denoise_temporal's, the other use of moments, another size
    uniform = rb.CameraData.from_buffer_copy(cam)
    uniform.samples_per_pixel = a
    _, old = dtr.reference(fb2, aov, uniform)
    assert dtsr.header(old)[0] == OLD_MAGIC
    other_cam = _synthetic_cam(131, 9)
    pad = lambda x: np.pad(x, [(0, 0), (0, 1)] + [(0, 0)] * (x.ndim - 2), mode="edge")
    _, other = dtsr.reference(pad(fb2), pad(spp2), pad(mom2), {k: pad(v) for k, v in aov.items()}, a, other_cam)
    for moments, mode in ((mom, dtsr.MODE_MOMENTS), (None, dtsr.MODE_SPATIAL)):
        _, crossed = dtsr.reference(fb2, spp2, None if moments is not None else mom2, aov, a, cam)
        assert dtsr.header(crossed) == (dtsr.MAGIC, w, h, 3 - mode)
        for it in (1, 5, 8):
            want = dsr.reference(fb, spp, moments, aov, a, iterations=it)
            got, nxt = dtsr.reference(fb, spp, moments, aov, a, cam, None, iterations=it)
            assert_same(got, want, f"empty history, {it} iterations, mode {mode}")
            assert dtsr.header(nxt) == (dtsr.MAGIC, w, h, mode)
            for prev, what in ((np.zeros_like(nxt), "all-zero history"), (old, "rt_denoise_temporal's history"), (crossed, "the other moments word"),
                               (other, "history of another size")):
                g, n = dtsr.reference(fb, spp, moments, aov, a, cam, prev, iterations=it)
                assert_same(g, want, f"{what}, {it} iterations, mode {mode}")
                assert_same(n, nxt, f"{what} (next history)")
        assert_same(dtsr.reference(fb, spp, moments, aov, a, cam, None, **OTHER)[0], dsr.reference(fb, spp, moments, aov, a, **OTHER), "other settings")
        # … while its own history is taken
        _, own = dtsr.reference(fb2, spp2, None if moments is None else mom2, aov, a, cam)
        g, n = dtsr.reference(fb, spp, moments, aov, a, cam, own)
        assert (dtr.planes(n, w, h)["moments"][..., 2] == 2).any()
        assert (g != dsr.reference(fb, spp, moments, aov, a)).any()


def test_reference_rt_denoise_temporal_takes_the_new_history_as_empty():
    (fb, spp, mom, aov), _, a = _synthetic_frames()
    cam = _synthetic_cam()
    cam.samples_per_pixel = a
    for moments in (mom, None):
        _, new = dtsr.reference(fb, spp, moments, aov, a, cam)
        want, want_next = dtr.reference(fb, aov, cam, None)
        got, nxt = dtr.reference(fb, aov, cam, new)
        assert_same(got, want, "rt_denoise_temporal over a history of rt_denoise_temporal_spp")
        assert_same(nxt, want_next, "its next history")


def test_reference_non_hit_pixels_pass_through_write_zero_records_and_are_no_taps():
    (fb, spp, mom, aov), (fb2, spp2, mom2, _), a = _synthetic_frames()
    cam = _synthetic_cam()
    w, h = cam.image_width, cam.image_height
    gone, gone2 = (aov["hits"] == 0) | (spp < 1), (aov["hits"] == 0) | (spp2 < 1)
    assert ((aov["hits"] > 0) & (spp == 0)).sum() >= 20 and (~gone & gone2).any() and (gone & ~gone2).any()
    rng = np.random.default_rng(1)
    for moments, moments2 in ((mom, mom2), (None, None)):
        for it in (0, 1, 5):
            out, hist = dtsr.reference(fb, spp, moments, aov, a, cam, None, iterations=it)
            out2, hist2 = dtsr.reference(fb2, spp2, moments2, aov, a, cam, hist, iterations=it)
            for o, f, g, hh in ((out, fb, gone, hist), (out2, fb2, gone2, hist2)):
                assert_same(o[g], f[g], "out == fb_sum where the pixel is no hit pixel")
                for name, plane in dtr.planes(hh, w, h).items():
                    assert not plane.view(np.uint32)[g].any(), f"{name} records of pixels that are no hit pixels"
                    assert plane[..., :3].view(np.uint32)[~g].any()
            # whatever a pixel that is no hit pixel of the first frame holds, the second frame does not see it
            fb1, mom1 = fb.copy(), mom.copy()
            fb1[gone] = rng.uniform(-1e6, 1e6, (gone.sum(), 3)).astype(F)
            mom1[gone] = rng.uniform(0, 1e6, (gone.sum(), 2)).astype(F)
            aov1 = {k: v.copy() for k, v in aov.items()}
            for key in ("albedo", "normal", "depth"):
                aov1[key][gone] = 7.5
            aov1["hits"] = np.where(spp < 1, 0, aov["hits"]).astype(np.uint32)          # a count of 0 is the same as no hit count
            o1, h1 = dtsr.reference(fb1, np.maximum(spp, 1), None if moments is None else mom1, aov1, a, cam, None, iterations=it)
            assert_same(o1[~gone], out[~gone], "hit pixels of the first frame")
            assert_same(h1[dtr.HEADER_BYTES:], hist[dtr.HEADER_BYTES:], "the first frame's history records")
            o2, h2 = dtsr.reference(fb2, spp2, moments2, aov, a, cam, h1, iterations=it)
            assert_same(o2, out2, "the second frame")
            assert_same(h2, hist2, "the second frame's history")
            # … and a pixel of the second frame whose own pixel was none in the first is disoccluded (a still camera: its taps are itself
            # with all the weight but a rounding's worth, and neighbours)
            length = dtr.planes(hist2, w, h)["moments"][..., 2]
            assert set(np.unique(length[~gone2 & ~gone]).tolist()) <= {1.0, 2.0} and (length[~gone2 & ~gone] == 2).sum() >= 100


def _flat(w, h, n, rng, a=A):
    """A frame whose every pixel is a hit pixel of one flat surface facing a still camera, n samples each (an int or an array)."""
    n = np.broadcast_to(np.asarray(n, np.int32), (h, w)).copy()
    nf = n.astype(F)
    aov = {"albedo": np.full((h, w, 3), 0.5 * a, F), "normal": np.tile(np.array([0, 0, a], F), (h, w, 1)), "depth": np.full((h, w), 8.0 * a, F),
           "hits": np.full((h, w), a, np.uint32), "prim": np.full((h, w), 3, np.int32)}
    fb = (rng.exponential(0.4, (h, w, 3)).astype(F) * nf[..., None]).astype(F)
    s1 = (rng.exponential(0.6, (h, w)).astype(F) * nf).astype(F)
    s2 = ((s1 * s1 / nf).astype(F) * rng.uniform(1.0, 3.0, (h, w)).astype(F)).astype(F)
    return fb, n, np.stack([s1, s2], axis=-1).astype(F), aov


def test_reference_alpha_floor_and_a_large_count_over_a_short_history():
    rng = np.random.default_rng(5)
    w, h = 40, 24
    cam = _synthetic_cam(w, h)
    for with_moments in (True, False):
        pick = lambda m: m if with_moments else None
        # a long history of 32-sample frames, then one sample: a = nf / (ch + nf) is far below min_alpha, so a = 0.2 and cnt = nf / 0.2f
        hist = None
        for _ in range(6):
            fb, n, mom, aov = _flat(w, h, 32, rng)
            _, hist = dtsr.reference(fb, n, pick(mom), aov, A, cam, hist, iterations=0)
        p = dtr.planes(hist, w, h)
        assert np.abs(p["moments"][..., 2] - 6).max() < 1e-4 and (p["position"][..., 3] >= 64).all()      # (bilinear means of 5s, +1)
        fb, n, mom, aov = _flat(w, h, 1, rng)
        _, hist = dtsr.reference(fb, n, pick(mom), aov, A, cam, hist, iterations=0)
        p = dtr.planes(hist, w, h)
        assert np.abs(p["moments"][..., 2] - 7).max() < 1e-4
        assert_same(p["position"][..., 3], np.full((h, w), F(1) / MIN_ALPHA, F), "cnt = nf / min_alpha")
        # a = 0.2 itself: with the colour history constant over the image, L = 0.8f * Lh + 0.2f * L_cur whatever the bilinear weights
        const = np.frombuffer(hist, np.uint8).copy()
        body = const[dtr.HEADER_BYTES:].view(F).reshape(4, h, w, 4)
        body[0, ..., :3] = F(0.75)
        fb, n, mom, aov = _flat(w, h, 1, rng)
        _, nxt = dtsr.reference(fb, n, pick(mom), aov, A, cam, const, iterations=0)
        L_cur = ((fb * F(1.0)).astype(F) / np.fmax((aov["albedo"] * F(1.0 / A)).astype(F), F(1e-3))).astype(F)
        b = F(F(1) - MIN_ALPHA)
        want = ((b * F(0.75)) + (MIN_ALPHA * L_cur).astype(F)).astype(F)
        got = dtr.planes(nxt, w, h)["colour"][..., :3]
        assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * float(np.abs(want).max()), "L = b * Lh + a * L_cur with a = 0.2"
        # 65536 samples over a fresh one-sample history: a = 65536 / 65537 > 0.99 and cnt = 65537
        fb, n, mom, aov = _flat(w, h, 1, rng)
        _, fresh = dtsr.reference(fb, n, pick(mom), aov, A, cam, None, iterations=0)
        assert (dtr.planes(fresh, w, h)["position"][..., 3] == 1).all()
        const = np.frombuffer(fresh, np.uint8).copy()
        const[dtr.HEADER_BYTES:].view(F).reshape(4, h, w, 4)[0, ..., :3] = F(0.75)
        fb, n, mom, aov = _flat(w, h, 65536, rng)
        _, nxt = dtsr.reference(fb, n, pick(mom), aov, A, cam, const, iterations=0)
        p = dtr.planes(nxt, w, h)
        assert (p["moments"][..., 2] == 2).all() and (p["position"][..., 3] == 65537).all()
        a = F(F(65536) / F(65537))
        L_cur = ((fb * F(1.0 / 65536)).astype(F) / np.fmax((aov["albedo"] * F(1.0 / A)).astype(F), F(1e-3))).astype(F)
        want = ((F(F(1) - a) * F(0.75)) + (a * L_cur).astype(F)).astype(F)
        assert np.abs(p["colour"][..., :3] - want).max() <= 4 * 2.0 ** -24 * float(np.abs(want).max())
        # a itself, from the restatement's output: L = (1 - a) * 0.75 + a * L_cur, where L_cur is far enough from 0.75 to tell
        far = np.abs(L_cur - F(0.75)) > 0.5
        a_out = (p["colour"][..., :3][far].astype(np.float64) - 0.75) / (L_cur[far].astype(np.float64) - 0.75)
        assert far.sum() >= 100 and a_out.min() > 0.99 and a_out.max() < 1.0 + 1e-5, (far.sum(), a_out.min(), a_out.max())


def _dot(a, b):
    return ((a[0] * b[0] + a[1] * b[1]).astype(F) + (a[2] * b[2]).astype(F)).astype(F)


def _reprojection(cam, hcam, z):
    """The header's (u, v) per pixel for depth z (H, W) float32, one float32 operation at a time."""
    h, w = z.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(F)
    vec = lambda v: [F(v.e[k]) for k in range(3)]
    O, P00, du, dv = vec(cam.origin), vec(cam.pixel00_loc), vec(cam.pixel_delta_u), vec(cam.pixel_delta_v)
    X = []
    for k in range(3):
        pc = ((P00[k] + (xx * du[k]).astype(F)).astype(F) + (yy * dv[k]).astype(F)).astype(F)
        X.append((O[k] + (z * (pc - O[k]).astype(F)).astype(F)).astype(F))
    O2, P2, du2, dv2 = vec(hcam.origin), vec(hcam.pixel00_loc), vec(hcam.pixel_delta_u), vec(hcam.pixel_delta_v)
    N = [F(F(du2[1] * dv2[2]) - F(du2[2] * dv2[1])), F(F(du2[2] * dv2[0]) - F(du2[0] * dv2[2])), F(F(du2[0] * dv2[1]) - F(du2[1] * dv2[0]))]
    E = [F(P2[k] - O2[k]) for k in range(3)]
    D = [(X[k] - O2[k]).astype(F) for k in range(3)]
    one = np.ones_like(z)
    with np.errstate(all="ignore"):                                     # (sky pixels: z = 0 puts X on the camera)
        t = (_dot([e * one for e in E], [n * one for n in N]) / _dot(D, [n * one for n in N])).astype(F)
        R = [((t * D[k]).astype(F) - E[k]).astype(F) for k in range(3)]
    u = (_dot(R, [d * one for d in du2]) / _dot([d * one for d in du2], [d * one for d in du2])).astype(F)
    v = (_dot(R, [d * one for d in dv2]) / _dot([d * one for d in dv2], [d * one for d in dv2])).astype(F)
    return u, v, t


def test_reference_propagated_variance_after_two_frames_restated_in_numpy():
    """V, cnt and len of the second frame under a still camera, written once more in numpy float32 for the pixels whose reprojection
    lands on one tap of weight 1 (u and v whole numbers: fx = fy = 0, so W = 1 and every sum is the tap's own value)."""
    (fb, spp, mom, aov), (fb2, spp2, mom2, _), a = _synthetic_frames()
    cam = _synthetic_cam()
    w, h = cam.image_width, cam.image_height
    hit1, hit2 = (aov["hits"] > 0) & (spp >= 1), (aov["hits"] > 0) & (spp2 >= 1)
    z = np.where(aov["hits"] > 0, aov["depth"] / np.maximum(aov["hits"], 1).astype(F), 0).astype(F)
    u, v, t = _reprojection(cam, cam, z)
    yy, xx = np.mgrid[0:h, 0:w].astype(F)
    whole = (u == xx) & (v == yy) & (t > 0) & hit1 & hit2 & (np.abs(aov["normal"]).sum(-1) > 0)
    print(f"{int(whole.sum())} of {int((hit1 & hit2).sum())} pixels reproject onto one tap of weight 1")
    assert whole.sum() >= 50
    for moments, moments2 in ((mom, mom2), (None, None)):
        _, var1 = dsr.reference(fb, spp, moments, aov, a, want_var=True, iterations=1)
        _, var2 = dsr.reference(fb2, spp2, moments2, aov, a, want_var=True, iterations=1)
        _, hist = dtsr.reference(fb, spp, moments, aov, a, cam, None)
        p1 = dtr.planes(hist, w, h)
        assert_same(p1["normal"][..., 3][hit1], var1[hit1], "V of a first frame is var_cur")
        assert_same(p1["position"][..., 3][hit1], spp[hit1].astype(F), "cnt of a first frame is nf")
        assert (p1["moments"][..., 2][hit1] == 1).all()
        _, hist2 = dtsr.reference(fb2, spp2, moments2, aov, a, cam, hist)
        p2 = dtr.planes(hist2, w, h)
        nf = spp2.astype(F)
        s = (spp.astype(F) + nf).astype(F)
        alpha = (nf / np.maximum(s, 1)).astype(F)
        floored = ~(alpha >= MIN_ALPHA)
        assert (floored & whole).any() and (~floored & whole).any()
        cnt = np.where(floored, (nf / MIN_ALPHA).astype(F), s).astype(F)
        alpha = np.where(floored, MIN_ALPHA, alpha).astype(F)
        beta = (F(1) - alpha).astype(F)
        V = (((beta * beta).astype(F) * var1).astype(F) + ((alpha * alpha).astype(F) * var2).astype(F)).astype(F)
        assert (p2["moments"][..., 2][whole] == 2).all()
        assert_same(p2["position"][..., 3][whole], cnt[whole], "cnt")
        assert_same(p2["normal"][..., 3][whole], V[whole], "V")


# ---- the rendered setting of the GPU tests, restated on the CPU --------------------------------------------------------

def _orbit_cam(k, w=77, h=45, spp=1):
    r, a0 = float(np.hypot(13, 2)), float(np.arctan2(2, 13))
    return rb.make_camera(w, h, 20.0, (r * np.cos(a0 + 0.004 * k), 3, r * np.sin(a0 + 0.004 * k)), (0, 0, 0), (0.7, 0.8, 1.0), spp, 50)


def _with_spp(cam, spp):
    c = rb.CameraData.from_buffer_copy(cam)
    c.samples_per_pixel = spp
    return c


@functools.lru_cache(maxsize=None)
def _oracle_orbit():
    """The GPU tests' orbit restated on the CPU: rtiow 77 x 45 at 4:4:32, t = 0.3, four frames 0.004 rad apart, from the oracle's
    per-sample radiances (test_adaptive.reference's rule) and the AOV restatement at 4 samples."""
    import aov_reference as ar
    import oracle_bindings as ob
    host = rb.HostScene.rtiow()
    w, h, s = 77, 45, SPP["max_spp"]
    jj, ii, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(s), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], axis=1).astype(np.int32)
    frames = []
    for k in range(4):
        cam = _orbit_cam(k)
        rad, _, _ = ob.trace_samples(host, cam, ijs)
        fb, spp, mom = lar.from_radiances(rad.reshape(h, w, s, 3), threshold=THRESHOLD, **SPP)
        frames.append((fb, spp, mom, ar.reference(host, _with_spp(cam, A)), cam))
    return frames


def test_the_rendered_setting_covers_the_cases_on_the_cpu():
    frames = _oracle_orbit()
    w, h = 77, 45
    for with_moments in (True, False):
        prev = None
        sky = disoccluded = accepted = floored = 0
        levels = {n: 0 for n in LEVELS}
        for k, (fb, spp, mom, aov, cam) in enumerate(frames):
            out, prev = dtsr.reference(fb, spp, mom if with_moments else None, aov, A, cam, prev)
            hit = aov["hits"] > 0
            assert_same(out[~hit], fb[~hit], "sky")
            p = dtr.planes(prev, w, h)
            assert np.isfinite(out).all() and all(np.isfinite(v[..., :3] if k == "moments" else v).all() for k, v in p.items())   # (moments.w: prim's bits)
            length, cnt = p["moments"][..., 2], p["position"][..., 3]
            sky += int((~hit).sum())
            for n in LEVELS:
                levels[n] += int((hit & (spp == n)).sum())
            if k > 0:
                disoccluded += int((hit & (length == 1)).sum())
                accepted += int((hit & (length > 1)).sum())
                floored += int((hit & (length > 1) & (cnt == (spp.astype(F) / MIN_ALPHA).astype(F))).sum())
            else:
                assert (length[hit] == 1).all() and (cnt[hit] == spp[hit]).all()
        print(f"oracle orbit, moments {with_moments}: sky {sky}, disoccluded {disoccluded}, accepted {accepted}, floored alphas {floored}, "
              f"hit pixels per count {levels}")
        assert sky > 0 and disoccluded > 0 and accepted > 0 and floored > 0
        assert all(v > 0 for v in levels.values()), levels


# ---- on the GPU --------------------------------------------------------------------------------------------------------

def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _orbit_frames():
    """Four adaptive frames of rtiow 77 x 45 along the small orbit with their moments and AOVs at min_spp (shared: do not write)."""
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    frames = []
    for k in range(4):
        cam = _orbit_cam(k)
        fb, spp, mom, _ = dev.render_adaptive_to_host(cam, threshold=THRESHOLD, **SPP)
        aov, _ = dev.render_aov_to_host(_with_spp(cam, A))
        _freeze(fb, spp, mom, *aov.values())
        frames.append((fb, spp, mom, aov, cam))
    dev.close()
    return frames


@functools.lru_cache(maxsize=None)
def _still_frames(w=77, h=45, count=3, threshold=THRESHOLD):
    """Adaptive frames of rtiow under a still camera through rt_render_lit_adaptive with every light off, frame k from sample 32 k."""
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    cam = rb.rtiow_camera(w, h, 1, 50)
    frames = []
    for k in range(count):
        fb, spp, mom, _ = dev.render_lit_adaptive_to_host(cam, emitters=False, sample_first=32 * k, threshold=threshold, **SPP)
        aov, _ = dev.render_aov_to_host(_with_spp(cam, A), sample_first=32 * k)
        _freeze(fb, spp, mom, *aov.values())
        frames.append((fb, spp, mom, aov, cam))
    dev.close()
    return frames


def _sequence(frames, with_moments, what, resets=(), aov_spp=A, **params):
    """The device TemporalDenoiser.step_spp against the C restatement, output and whole history, frame by frame."""
    rb.amd_lib().rt_set_device(0)
    cam0 = frames[0][4]
    td = rb.TemporalDenoiser(cam0.image_width, cam0.image_height, **params)
    prev = None
    outs = []
    try:
        for n, (fb, spp, mom, aov, cam) in enumerate(frames):
            if n in resets:
                td.reset()
                prev = None
            m = mom if with_moments else None
            got = td.step_spp_to_host(fb, spp, m, aov, aov_spp, cam)
            want, prev = dtsr.reference(fb, spp, m, aov, aov_spp, cam, prev, **params)
            tag = f"{what}: frame {n} {'with' if with_moments else 'without'} moments {params}"
            assert_same(got, want, tag)
            assert_same(td.history_to_host(), prev, tag + " (history)")
            outs.append(got)
    finally:
        td.close()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("moments", [True, False])
def test_rtiow_orbit_of_adaptive_frames(moments):
    frames = _orbit_frames()
    w, h = 77, 45
    hit = frames[0][3]["hits"] > 0
    assert (~hit).any() and len(np.unique(frames[0][1][hit])) >= 3
    for it in (0, 1, 5, 8):                  # at 8 the step of 128 exceeds the image
        outs = _sequence(frames, moments, "rtiow orbit", iterations=it)
        for out, (fb, _, _, aov, _) in zip(outs, frames):
            assert_same(out[aov["hits"] == 0], fb[aov["hits"] == 0], "sky pixels")
    _sequence(frames, moments, "rtiow orbit", **OTHER)
    _sequence(frames, moments, "rtiow orbit with a reset", resets=(2,))


@pytest.mark.gpu
def test_still_camera_through_the_lit_path_with_sample_offsets():
    frames = _still_frames()
    assert any((a[1] != b[1]).any() for a, b in zip(frames, frames[1:])), "the frames' counts differ"
    for moments in (True, False):
        _sequence(frames, moments, "rtiow still, lit path")
        _sequence(frames, moments, "rtiow still, lit path", iterations=1, sigma_luminance=2.0, normal_squarings=3)


def _cut(frame, ys, xs):
    """The sub-image [ys, xs] of a frame, with the camera of exactly those pixels."""
    fb, spp, mom, aov, cam = frame
    c = lambda a: np.ascontiguousarray(a[ys, xs])
    sub = rb.CameraData.from_buffer_copy(cam)
    x0, y0 = F(xs.start or 0), F(ys.start or 0)
    for k in range(3):
        sub.pixel00_loc.e[k] = F(F(F(cam.pixel00_loc.e[k]) + F(x0 * F(cam.pixel_delta_u.e[k]))) + F(y0 * F(cam.pixel_delta_v.e[k])))
    sub.image_height, sub.image_width = c(spp).shape
    return c(fb), c(spp), c(mom), {k: c(v) for k, v in aov.items()}, sub


@pytest.mark.gpu
def test_sub_images_one_pixel_wide_high_and_alone():
    frames = _orbit_frames()
    for what, ys, xs, params in (("45x1 column", slice(None), slice(30, 31), {}), ("1x77 row", slice(22, 23), slice(None), dict(iterations=8)),
                                 ("1x1", slice(22, 23), slice(40, 41), {})):
        cut = [_cut(f, ys, xs) for f in frames[:3]]
        assert (cut[0][3]["hits"] > 0).any()
        for moments in (True, False):
            _sequence(cut, moments, what, **params)


@pytest.mark.gpu
def test_lit_adaptive_frames_of_the_panel_box_without_the_lens():
    """DESIGN.md §19's setting d at 32 x 24 without its lens: panel box, planes, tree, MIS and the sun-and-sky map through
    rt_render_lit_adaptive, two frames of a still camera (the second from sample 32), the AOVs through rt_render_aov_samples."""
    rb.amd_lib().rt_set_device(0)
    name = lar.SETTINGS["d"][0]
    host = tl.scene(name)
    cam = tl.camera(name, *lar.SIZE, 1)
    frames = []
    with rb.Env(lar.sky()) as env:
        kw = lar.device_keywords("d", env)
        kw.pop("lens")
        dev = rb.DeviceScene(host, device=0)
        for k in range(2):
            fb, spp, mom, _ = dev.render_lit_adaptive_to_host(cam, sample_first=32 * k, threshold=lar.THRESHOLD, **lar.SPP, **kw)
            aov, _ = dev.render_aov_to_host(_with_spp(cam, lar.SPP["min_spp"]), sample_first=32 * k)
            frames.append((fb, spp, mom, aov, cam))
        dev.close()
    assert len(np.unique(frames[0][1])) >= 3 and (frames[0][3]["hits"] > 0).any()
    for moments in (True, False):
        _sequence(frames, moments, "lit setting d", aov_spp=lar.SPP["min_spp"])
        _sequence(frames, moments, "lit setting d", aov_spp=lar.SPP["min_spp"], iterations=2, sigma_luminance=1.5)


@pytest.mark.gpu
def test_synthetic_inputs_every_count_and_moment_case_and_a_camera_that_looks_away():
    (fb, spp, mom, aov), (fb2, spp2, mom2, _), a = _synthetic_frames()
    cam, away = _synthetic_cam(), _synthetic_cam(away=True)
    frames = [(fb, spp, mom, aov, cam), (fb2, spp2, mom2, aov, cam), (fb, spp, mom, aov, away), (fb2, spp2, mom2, aov, cam)]
    for moments in (True, False):
        for it in (0, 1, 5):
            outs = _sequence(frames, moments, "synthetic 130x9", aov_spp=a, iterations=it)
            for out, f in zip(outs, frames):
                gone = (aov["hits"] == 0) | (f[1] < 1)
                assert_same(out[gone], f[0][gone], "pixels that are no hit pixels")
            # nothing of the camera that looks away reprojects: the last frame is a first frame
            want = rb.denoise_spp_to_host(fb2, spp2, mom2 if moments else None, aov, a, iterations=it) if it else None
            if it:
                assert_same(outs[3], want, "after the camera that looks away")
        _sequence(frames, moments, "synthetic 130x9", aov_spp=a, **OTHER)


@pytest.mark.gpu
def test_mixed_calls_restart_the_history():
    """rt_denoise_temporal, then this call, then rt_denoise_temporal, then this call without moments, on one object's buffers: each
    finds a history that is not its own and starts again; rt_denoise_temporal's outputs are its own restatement's."""
    rb.amd_lib().rt_set_device(0)
    frames = _still_frames()
    fb, spp, mom, aov, cam = frames[0]
    ucam = _with_spp(cam, A)
    ufb = np.ascontiguousarray(frames[1][0] * (F(A) / frames[1][1].astype(F))[..., None], F)          # some frame at a uniform count
    td = rb.TemporalDenoiser(cam.image_width, cam.image_height)
    try:
        old_want, old_hist = dtr.reference(ufb, aov, ucam, None)
        assert_same(td.step_to_host(ufb, aov, ucam), old_want, "rt_denoise_temporal first")
        assert_same(td.history_to_host(), old_hist, "its history")
        want, hist = dtsr.reference(fb, spp, mom, aov, A, cam, None)
        assert_same(td.step_spp_to_host(fb, spp, mom, aov, A, cam), want, "rt_denoise_temporal_spp over rt_denoise_temporal's history")
        assert_same(td.history_to_host(), hist, "its history")
        assert_same(td.step_to_host(ufb, aov, ucam), old_want, "rt_denoise_temporal over rt_denoise_temporal_spp's history")
        assert_same(td.history_to_host(), old_hist, "its history")
        assert_same(td.step_to_host(ufb, aov, ucam), dtr.reference(ufb, aov, ucam, old_hist)[0], "rt_denoise_temporal over its own")
        td.step_spp_to_host(fb, spp, mom, aov, A, cam)
        want, hist = dtsr.reference(fb, spp, None, aov, A, cam, None)
        assert_same(td.step_spp_to_host(fb, spp, None, aov, A, cam), want, "without moments over a history with")
        assert_same(td.history_to_host(), hist, "its history")
        want2, hist2 = dtsr.reference(fb, spp, None, aov, A, cam, hist)
        assert_same(td.step_spp_to_host(fb, spp, None, aov, A, cam), want2, "without moments over its own")
        assert (want2 != want).any()
    finally:
        td.close()


@pytest.mark.gpu
def test_side_stream_replay_and_nan_filled_output():
    import torch
    w, h = 200, 120
    frames = _still_frames(w, h, 2)
    lib = rb.amd_lib()
    hist_bytes = lib.rt_denoise_history_bytes(w, h)
    hist = [torch.zeros(hist_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    ws = torch.empty(lib.rt_denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    prev = None
    for n, (fb, spp, mom, aov, cam) in enumerate(frames):
        t = {"fb": torch.from_numpy(fb.copy()).to("cuda:0"), "spp": torch.from_numpy(spp.copy()).to("cuda:0"), "mom": torch.from_numpy(mom.copy()).to("cuda:0")}
        for key, _, dtype, _ in rb.AOV_CHANNELS:
            t[key] = torch.from_numpy((aov[key].view(np.float32) if dtype != np.float32 else aov[key]).copy()).to("cuda:0")
        want, prev = dtsr.reference(fb, spp, mom, aov, A, cam, prev, iterations=4)
        for replay in range(2):              # the two histories are distinct buffers: the same call again gives the same bytes
            out = torch.full_like(t["fb"], float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                # frame 0 reads the zero-filled buffer: an empty history
                rb.denoise_temporal_spp(t["fb"].data_ptr(), t["spp"].data_ptr(), t["mom"].data_ptr(), {k: t[k].data_ptr() for k, _, _, _ in rb.AOV_CHANNELS},
                                        A, cam, hist[(n + 1) & 1].data_ptr(), hist[n & 1].data_ptr(), hist_bytes, out.data_ptr(),
                                        (ws.data_ptr(), ws.numel()), stream=stream.cuda_stream, iterations=4)
            stream.synchronize()
            assert_same(out.cpu().numpy(), want, f"side stream frame {n} run {replay}")
            assert_same(hist[n & 1].cpu().numpy(), prev, f"side stream history {n} run {replay}")


@pytest.mark.gpu
def test_empty_history_on_the_device_is_rt_denoise_spp():
    fb, spp, mom, aov, cam = _orbit_frames()[0]
    for m in (mom, None):
        for params in (dict(iterations=1), dict(), OTHER):
            td = rb.TemporalDenoiser(cam.image_width, cam.image_height, **params)
            try:
                assert_same(td.step_spp_to_host(fb, spp, m, aov, A, cam), rb.denoise_spp_to_host(fb, spp, m, aov, A, **params), f"empty history {params}")
            finally:
                td.close()


@pytest.mark.gpu
def test_cli_writes_the_python_paths_denoised_files(test_config_text, tmp_path):
    import torch
    lines = test_config_text.split("\n")
    lines[0] = "3"
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    out = subprocess.run([EXE, "--gpu", "--adaptive", "0.3", "--adaptive-spp", "4:4:32", "--denoise-adaptive-temporal"], input=text, capture_output=True,
                         text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.from_config(text)
    dev = rb.DeviceScene(host, device=0)
    cam0 = host.frame_camera(0)
    td = rb.TemporalDenoiser(cam0.image_width, cam0.image_height)
    prev = None

    def file_bytes(frame, spp, cam):
        d_fb, d_spp = torch.from_numpy(np.ascontiguousarray(frame)).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
        rgb = torch.zeros(frame.shape, dtype=torch.uint8, device="cuda:0")
        assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == 0
        torch.cuda.synchronize()
        return np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes()
    try:
        for n in range(3):
            cam = _with_spp(host.frame_camera(n), A)
            fb, spp, mom, _ = dev.render_adaptive_to_host(cam, threshold=0.3, **SPP)
            aov, _ = dev.render_aov_to_host(cam)
            got = td.step_spp_to_host(fb, spp, mom, aov, A, cam)
            want, prev = dtsr.reference(fb, spp, mom, aov, A, cam, prev)
            assert_same(got, want, f"the Python path, frame {n}")
            assert open(tmp_path / f"f_{n}.png.denoised", "rb").read() == file_bytes(got, spp, cam), n
            assert open(tmp_path / f"f_{n}.png", "rb").read() == file_bytes(fb, spp, cam), "the frame itself is --adaptive's"
        assert (dtr.planes(prev, cam.image_width, cam.image_height)["moments"][..., 2] > 1).any(), "the history was carried"
        # the lit path (a pinhole, a closed shutter): rt_render_lit_adaptive's frames, the AOVs through rt_render_aov
        lines[0] = "2"
        lines[1] = str(tmp_path / "lit_%d.png")
        text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
        out = subprocess.run([EXE, "--gpu", "--lit", "--nee", "--light-tree", "--noise-target", "0.3", "--noise-spp", "4:4:32", "--denoise-adaptive-temporal"],
                             input=text, capture_output=True, text=True, timeout=200)
        assert out.returncode == 0, out.stderr
        td.reset()
        for n in range(2):
            cam = host.frame_camera_at(float(n))
            fb, spp, mom, _ = dev.render_lit_adaptive_to_host(cam, nee=dict(select=1), threshold=0.3, **SPP)
            aov, _ = dev.render_aov_to_host(_with_spp(cam, A))
            got = td.step_spp_to_host(fb, spp, mom, aov, A, cam)
            assert open(tmp_path / f"lit_{n}.png.denoised", "rb").read() == file_bytes(got, spp, cam), f"lit frame {n}"
            assert open(tmp_path / f"lit_{n}.png", "rb").read() == file_bytes(fb, spp, cam), "the frame itself is --lit --noise-target's"
    finally:
        td.close()
        dev.close()


def _mse(fb, spp, truth):
    return float(np.mean((np.clip(fb / np.asarray(spp, F)[..., None], 0, 1) - truth) ** 2))


# rt_denoise_temporal_spp with moments after eight frames over rt_denoise_spp (with moments) of the eighth frame alone, as computed with
# the restatements from oracle radiances (with moments 2.44362e-4, without 3.57082e-4, rt_denoise_spp alone 6.89623e-4
# (without moments 6.56271e-4), the noisy frame 1.54317e-3)
QUALITY_RATIO = 0.3543


@pytest.mark.gpu
def test_quality_against_a_1024_spp_ground_truth():
    """Measured, not promised: rtiow 320 x 180, eight still frames at 4:4:32 and t = 0.1, frame k from sample 32 k, the
    AOVs at 4 spp; the MSE of the clamped mean against 1024 spp from sample 2^20 after frame 8 with and without moments, of
    rt_denoise_spp on frame 8 alone and of the noisy frame 8.  The with-moments figure is pinned against rt_denoise_spp alone at the
    measured ratio (0.3543) plus 10 %, so that a regression shows."""
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    cam = rb.rtiow_camera(320, 180, 1, 50)
    gt, _ = dev.render_to_host(rb.rtiow_camera(320, 180, 1024, 50), sample_first=1 << 20)
    truth = np.clip(gt / F(1024), 0, 1)
    aov, _ = dev.render_aov_to_host(_with_spp(cam, A))
    with_m, without_m = rb.TemporalDenoiser(320, 180), rb.TemporalDenoiser(320, 180)
    try:
        for k in range(8):
            fb, spp, mom, _ = dev.render_lit_adaptive_to_host(cam, emitters=False, sample_first=32 * k, threshold=0.1, **SPP)
            out_with = with_m.step_spp_to_host(fb, spp, mom, aov, A, cam)
            out_without = without_m.step_spp_to_host(fb, spp, None, aov, A, cam)
    finally:
        with_m.close()
        without_m.close()
        dev.close()
    temporal, temporal_without = _mse(out_with, spp, truth), _mse(out_without, spp, truth)
    alone = _mse(rb.denoise_spp_to_host(fb, spp, mom, aov, A), spp, truth)
    alone_without = _mse(rb.denoise_spp_to_host(fb, spp, None, aov, A), spp, truth)
    noisy = _mse(fb, spp, truth)
    print(f"quality: frame 8 at {float(spp.mean()):.2f} spp mean: noisy MSE {noisy:.6g}; rt_denoise_spp alone {alone:.6g} (without moments "
          f"{alone_without:.6g}); rt_denoise_temporal_spp with moments {temporal:.6g} (ratio {temporal / alone:.4f}), without {temporal_without:.6g} "
          f"(ratio {temporal_without / alone:.4f})")
    assert temporal <= 1.1 * QUALITY_RATIO * alone
