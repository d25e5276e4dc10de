"""rt_denoise_spp: rt_denoise for adaptively sampled frames — each pixel normalised and remodulated by its own count, the luminance
edge-stopping steered by the variance of the pixel's own samples (include/rtp_amd.h).  The device output is compared
byte for byte with the C restatement of the header's arithmetic (tests/denoise_spp_reference.py) on rendered adaptive frames (the
pinhole path and the lit path), their sub-images, synthetic inputs at the edges of the contract, a side stream and the CLI's file; the
restatement itself is checked for the header's identities; and the quality against a 1024-spp ground truth is measured and pinned.
On the CPU: the ABI, every refusal (they come before any HIP call, so fake addresses do), the identities and the CLI's refusals."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as dr
import denoise_spp_reference as dsr
import lit_adaptive_reference as lar
import rtp_bindings as rb
import test_adaptive as ta
import test_light_tree as tl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
FAKE = 1 << 32          # a device address that is never dereferenced: every check comes before any HIP call
INVALID, UNSUPPORTED = 1, 4
F = np.float32
SPP = dict(min_spp=4, batch_spp=4, max_spp=32)
THRESHOLD = 0.3
OTHER = dict(iterations=3, sigma_depth=0.25, sigma_luminance=40.0, normal_squarings=2)      # one non-default set
assert_same = ta.assert_same


# ---- no GPU needed -----------------------------------------------------------------------------------------------------

def test_abi_symbol_argtypes_and_functions():
    lib = rb.amd_lib()
    assert hasattr(lib, "rt_denoise_spp") and "rt_denoise_spp" in rb.RTP_AMD_SYMBOLS
    assert len(lib.rt_denoise_spp.argtypes) == 12
    assert callable(rb.denoise_spp) and callable(rb.denoise_spp_to_host)
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        assert "rt_status rt_denoise_spp(" in f.read()


def _full_aov():
    b = rb.AovBuffers()
    b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count = 2 * FAKE, 3 * FAKE, 4 * FAKE, 5 * FAKE
    return b


def _call(fb=FAKE, spp=8 * FAKE, mom=9 * FAKE, aov="full", aov_spp=4, width=8, height=4, params=None, ws=None, ws_bytes=None, out=None):
    lib = rb.amd_lib()
    b = _full_aov() if aov == "full" else aov
    ws = 6 * FAKE if ws is None else ws
    ws_bytes = lib.rt_denoise_workspace_bytes(width, height) if ws_bytes is None else ws_bytes
    out = 7 * FAKE if out is None else out
    lib.rt_get_last_error_string()
    st = lib.rt_denoise_spp(C.c_void_p(fb), C.c_void_p(spp), C.c_void_p(mom), C.byref(b) if b is not None else None, aov_spp, width, height,
                            C.byref(params) if params else None, C.c_void_p(ws), ws_bytes, C.c_void_p(out), None)
    return st, lib.rt_get_last_error_string().decode()


def test_refusals_need_no_device():
    lib = rb.amd_lib()
    px = 8 * 4
    cases = [dict(fb=0), dict(spp=0), dict(aov=None), dict(ws=0), dict(out=0), dict(width=0), dict(height=-3), dict(aov_spp=0),
             dict(aov_spp=65537), dict(aov_spp=-4), dict(ws_bytes=lib.rt_denoise_workspace_bytes(8, 4) - 1),
             # d_out or the workspace over an input: fb, an AOV, the counts (4 bytes per pixel) and the moments (8 per pixel)
             dict(out=2 * FAKE + 12), dict(out=FAKE - px * 12 + 4), dict(out=5 * FAKE + 124), dict(ws=FAKE + 64),
             dict(out=8 * FAKE), dict(out=8 * FAKE + 4 * px - 4), dict(out=8 * FAKE - 12 * px + 4), dict(ws=8 * FAKE + 64),
             dict(out=9 * FAKE), dict(out=9 * FAKE + 8 * px - 4), dict(out=9 * FAKE - 12 * px + 4), dict(ws=9 * FAKE + 8 * px - 1),
             dict(out=6 * FAKE + 100)]
    for field in ("albedo_sum", "normal_sum", "depth_sum", "hit_count"):
        b = _full_aov()
        setattr(b, field, None)
        cases.append(dict(aov=b))
    short = _full_aov()
    short.struct_bytes = 32                                           # hit_count lies past struct_bytes: it counts as NULL
    cases.append(dict(aov=short))
    for field, bad in (("iterations", -1), ("iterations", 9), ("sigma_depth", 0.0), ("sigma_depth", float("nan")), ("sigma_luminance", 0.0),
                       ("sigma_luminance", float("inf")), ("normal_squarings", -1), ("normal_squarings", 11), ("struct_bytes", 4)):
        p = rb.denoise_params()
        setattr(p, field, bad)
        cases.append(dict(params=p))
    for kw in cases:
        st, msg = _call(**kw)
        assert st == INVALID and msg.startswith("rt_denoise_spp:"), (kw, st, msg)
    for kw, word in ((dict(spp=0), "null"), (dict(aov_spp=0), "aov_samples"), (dict(out=8 * FAKE), "d_out overlaps an input"),
                     (dict(out=9 * FAKE + 8 * px - 4), "d_out overlaps an input"), (dict(ws=8 * FAKE + 64), "the workspace overlaps an input"),
                     (dict(ws=9 * FAKE + 8 * px - 1), "the workspace overlaps an input"), (dict(out=6 * FAKE + 100), "d_out overlaps the workspace")):
        assert word in _call(**kw)[1], (kw, _call(**kw))
    for w, h in ((4097, 4096), (1 << 24, 2), (1, (1 << 24) + 1)):
        st, msg = _call(width=w, height=h)
        assert st == UNSUPPORTED and "2^24" in msg and msg.startswith("rt_denoise_spp:"), (w, h, st, msg)
    # what is allowed passes its check and fails a later one (nothing here may reach a launch: the addresses are fake)
    short_ws = lib.rt_denoise_workspace_bytes(8, 4) - 1
    for kw in (dict(aov_spp=65536), dict(aov_spp=1), dict(mom=0), dict(params=rb.denoise_params(iterations=0, normal_squarings=0)),
               dict(width=4096, height=4096, ws_bytes=64 << 24)):
        st, msg = _call(ws_bytes=kw.pop("ws_bytes", short_ws), **kw)
        assert st == INVALID and "workspace_bytes" in msg, (kw, st, msg)
    # d_out right after / right before the counts and the moments; without moments their range is nobody's
    for out in (8 * FAKE + 4 * px, 8 * FAKE - 12 * px, 9 * FAKE + 8 * px, 9 * FAKE - 12 * px):
        st, msg = _call(out=out, ws=5 * FAKE + 64)
        assert st == INVALID and "the workspace overlaps an input" in msg, (out, st, msg)
    st, msg = _call(mom=0, out=9 * FAKE, ws=5 * FAKE + 64)
    assert st == INVALID and "the workspace overlaps an input" in msg, (st, msg)
    # the order: arguments before parameters before the pixel limit before the workspace before the overlaps
    bad = rb.denoise_params(iterations=9)
    assert "aov_samples" in _call(aov_spp=0, params=bad, width=1 << 24, height=2, ws_bytes=0, out=FAKE)[1]
    assert "iterations" in _call(params=bad, width=1 << 24, height=2, ws_bytes=0, out=FAKE)[1]
    assert "2^24" in _call(width=1 << 24, height=2, ws_bytes=0, out=FAKE)[1]
    assert "workspace_bytes" in _call(ws_bytes=0, out=FAKE)[1]


def _synthetic(w=130, h=9, seed=11, aov_spp=4):
    """Random inputs of the filter: AOVs with sky holes, counts from {0, 1, 2, 3, 17, 65536}, moments with S2 < S1^2 / n (the clamp) and
    exact zeros.  Everything finite, and no negative zero among the moments."""
    rng = np.random.default_rng(seed)
    hits = rng.integers(1, aov_spp + 1, (h, w)).astype(np.uint32)
    hits[rng.random((h, w)) < 0.15] = 0
    hits[:, 64] = 0                                                   # a whole column of sky at the tile boundary
    hf = hits.astype(F)
    aov = {"albedo": (rng.uniform(0.0, 1.0, (h, w, 3)).astype(F) * hf[..., None]).astype(F),
           "normal": (rng.normal(0.0, 1.0, (h, w, 3)).astype(F) * hf[..., None]).astype(F),
           "depth": (rng.uniform(1.0, 30.0, (h, w)).astype(F) * hf).astype(F), "hits": hits}
    aov["albedo"][0, :5] = 0                                          # the 1e-3 floor of the divisor
    aov["normal"][1, :5] = 0                                          # len2 == 0
    spp = rng.choice(np.array([0, 1, 2, 3, 17, 65536], np.int32), (h, w)).astype(np.int32)
    nf = np.maximum(spp, 1).astype(F)
    fb = (rng.exponential(0.7, (h, w, 3)).astype(F) * nf[..., None]).astype(F)
    s1 = (rng.exponential(0.6, (h, w)).astype(F) * nf).astype(F)
    s2 = ((s1 * s1 / nf).astype(F) * rng.uniform(0.5, 3.0, (h, w)).astype(F)).astype(F)       # below S1^2 / n for a fifth of them
    kind = rng.integers(0, 8, (h, w))
    s1[kind == 0], s2[kind == 0] = 0, 0                               # exact zeros
    s2[kind == 1] = 0                                                 # S2 = 0 under a positive S1: the clamp
    mom = np.stack([s1, s2], axis=-1).astype(F)
    return fb, spp, mom, aov, aov_spp


def test_synthetic_inputs_reach_every_case():
    fb, spp, mom, aov, _ = _synthetic()
    hit = aov["hits"] > 0
    assert (~hit).any() and set(np.unique(spp[hit]).tolist()) == {0, 1, 2, 3, 17, 65536}
    n = np.maximum(spp, 2).astype(F)
    under = mom[..., 1] < (mom[..., 0] * (mom[..., 0] / n).astype(F)).astype(F)
    assert (under & hit & (spp >= 2)).sum() >= 20 and ((mom[..., 0] == 0) & (mom[..., 1] == 0) & hit & (spp >= 2)).sum() >= 20
    assert np.isfinite(fb).all() and np.isfinite(mom).all() and not np.signbit(mom).any()


def test_reference_uniform_counts_without_moments_is_rt_denoise():
    fb, _, _, aov, _ = _synthetic(w=70, h=11, seed=3, aov_spp=8)
    for it in (0, 1, 5, 8):
        spp = np.full(aov["hits"].shape, 8, np.int32)
        assert_same(dsr.reference(fb, spp, None, aov, 8, iterations=it), dr.reference(fb, aov, 8, iterations=it), f"iterations {it}")
    assert_same(dsr.reference(fb, spp, None, aov, 8, **OTHER), dr.reference(fb, aov, 8, **OTHER), "other settings")


def test_reference_non_hit_pixels_pass_through_and_leak_nowhere():
    fb, spp, mom, aov, a = _synthetic()
    gone = (aov["hits"] == 0) | (spp < 1)
    assert ((aov["hits"] > 0) & (spp == 0)).sum() >= 20, "n = 0 on pixels with a hit count"
    rng = np.random.default_rng(1)
    for moments in (mom, None):
        for it in (0, 1, 5):
            out = dsr.reference(fb, spp, moments, aov, a, iterations=it)
            assert_same(out[gone], fb[gone], "out == fb_sum where the pixel is no hit pixel")
            # whatever such a pixel holds — sums, moments, AOVs — no hit pixel sees it
            fb2, mom2 = fb.copy(), mom.copy()
            fb2[gone] = rng.uniform(-1e6, 1e6, (gone.sum(), 3)).astype(F)
            mom2[gone] = rng.uniform(0, 1e6, (gone.sum(), 2)).astype(F)
            aov2 = {k: v.copy() for k, v in aov.items()}
            for key in ("albedo", "normal", "depth"):
                aov2[key][gone] = 7.5
            out2 = dsr.reference(fb2, spp, None if moments is None else mom2, aov2, a, iterations=it)
            assert_same(out2[~gone], out[~gone], f"iterations {it}: hit pixels")
            assert_same(out2[gone], fb2[gone], f"iterations {it}: the others")
            # a count of 0 on a pixel with a hit count is the same as no hit count
            aov3 = {**aov, "hits": np.where(gone, 0, aov["hits"]).astype(np.uint32)}
            assert_same(dsr.reference(fb, np.maximum(spp, 1), moments, aov3, a, iterations=it), out, f"iterations {it}: n = 0 is sky")


def _sample_variance(spp, mom, aov, a):
    """The header's v per pixel, one float32 operation at a time (0 where n < 2; not masked by hit pixels)."""
    inv = F(1.0 / float(a))
    d = np.fmax((aov["albedo"] * inv).astype(F), F(1e-3))
    dl = ((F(0.2126) * d[..., 0] + F(0.7152) * d[..., 1]).astype(F) + F(0.0722) * d[..., 2]).astype(F)
    n = np.maximum(spp, 2)
    s1, s2 = mom[..., 0], mom[..., 1]
    mean = (s1 / n.astype(F)).astype(F)
    vs = np.fmax(F(0), ((s2 - (s1 * mean).astype(F)).astype(F) / (n - 1).astype(F)).astype(F))
    vm = (vs / n.astype(F)).astype(F)
    return np.where(spp >= 2, (vm / (dl * dl).astype(F)).astype(F), F(0)).astype(F)


def _gauss(v, hit):
    """The header's 3x3 Gaussian of v over hit pixels, in its order (dy outer, dx inner), float32."""
    h, w = v.shape
    k = (F(0.5), F(0.25))
    out = np.zeros((h, w), F)
    for y in range(h):
        for x in range(w):
            if not hit[y, x]:
                continue
            G, SV = F(0), F(0)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and hit[yy, xx]:
                        g = F(k[abs(dx)] * k[abs(dy)])
                        G = F(G + g)
                        SV = F(SV + F(g * v[yy, xx]))
            out[y, x] = F(SV / G)
    return out


def test_reference_gaussian_of_a_constant_variance_is_that_variance():
    """A flat scene whose every pixel has the same moments: v is one number, and its Gaussian returns it at interior, edge and corner
    pixels (G = 1, 3/4, 9/16).  G is exact (sums of powers of two), each product g * v is exact, so var differs from v by the
    roundings of at most 8 additions of positive terms and one division: at most 9 * 2^-24 relative to first order; 10 * 2^-24 is asked."""
    h, w, a, n = 7, 9, 4, 12
    aov = {"albedo": np.full((h, w, 3), 0.5 * a, F), "normal": np.tile(np.array([0, 0, a], F), (h, w, 1)),
           "depth": np.full((h, w), 5.0 * a, F), "hits": np.full((h, w), a, np.uint32)}
    spp = np.full((h, w), n, np.int32)
    mom = np.tile(np.array([7.3, 9.1], F), (h, w, 1))
    fb = np.full((h, w, 3), 0.3 * n, F)
    v = _sample_variance(spp, mom, aov, a)
    assert (v == v[0, 0]).all() and v[0, 0] > 0
    _, var = dsr.reference(fb, spp, mom, aov, a, want_var=True, iterations=1)
    for name, (y, x) in (("interior", (3, 4)), ("edge", (0, 4)), ("edge", (3, 0)), ("corner", (0, 0)), ("corner", (h - 1, w - 1))):
        assert abs(float(var[y, x]) - float(v[0, 0])) <= 10 * 2.0 ** -24 * float(v[0, 0]), (name, var[y, x], v[0, 0])
    assert_same(var, _gauss(v, aov["hits"] > 0), "the Gaussian, restated")


def test_reference_variance_and_single_sample_pixels():
    """var of the restatement equals the header's v and Gaussian restated in numpy over the synthetic inputs, byte for byte; and a pixel
    with one sample (v = 0) takes its neighbours' variance."""
    fb, spp, mom, aov, a = _synthetic()
    hit = (aov["hits"] > 0) & (spp >= 1)
    v = _sample_variance(spp, mom, aov, a)
    _, var = dsr.reference(fb, spp, mom, aov, a, want_var=True, iterations=1)
    assert_same(var, _gauss(v, hit), "var")
    # n = 1 among neighbours with a positive variance
    h, w = 5, 6
    aov1 = {"albedo": np.full((h, w, 3), 0.5 * a, F), "normal": np.tile(np.array([0, 0, a], F), (h, w, 1)),
            "depth": np.full((h, w), 5.0 * a, F), "hits": np.full((h, w), a, np.uint32)}
    spp1 = np.full((h, w), 8, np.int32)
    spp1[2, 3] = 1
    mom1 = np.tile(np.array([4.0, 6.0], F), (h, w, 1))
    mom1[2, 3] = (0.5, 0.25)
    v1 = _sample_variance(spp1, mom1, aov1, a)
    assert v1[2, 3] == 0 and v1[2, 2] > 0
    _, var1 = dsr.reference(np.full((h, w, 3), 2.0, F), spp1, mom1, aov1, a, want_var=True, iterations=1)
    assert_same(var1, _gauss(v1, np.ones((h, w), bool)), "var around the n = 1 pixel")
    # the centre's weight 1/4 holds no variance, the other 3/4 is the neighbours' (8 additions and a division by 1: 9 roundings)
    assert abs(float(var1[2, 3]) - 0.75 * float(v1[2, 2])) <= 10 * 2.0 ** -24 * float(v1[2, 2])
    # without moments the same pixel gets rt_denoise's spatial variance (its mean, 2 / 0.5, differs from its neighbours' 0.25 / 0.5)
    _, spatial = dsr.reference(np.full((h, w, 3), 2.0, F), spp1, None, aov1, a, want_var=True, iterations=1)
    assert spatial[2, 3] > 1


@functools.lru_cache(maxsize=None)
def _oracle_inputs():
    """The GPU tests' rendered input restated on the CPU: rtiow 77 x 45 at 4:4:32, t = 0.3, from the oracle's per-sample radiances
    (test_adaptive.reference's rule) and the AOV restatement at 4 samples."""
    import aov_reference as ar
    import oracle_bindings as ob
    host = rb.HostScene.rtiow()
    w, h, s = 77, 45, SPP["max_spp"]
    jj, ii, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(s), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], axis=1).astype(np.int32)
    rad, _, _ = ob.trace_samples(host, rb.rtiow_camera(w, h, 1, 50), ijs)
    fb, spp, mom = lar.from_radiances(rad.reshape(h, w, s, 3), threshold=THRESHOLD, **SPP)
    aov = ar.reference(host, rb.rtiow_camera(w, h, SPP["min_spp"], 50))
    return fb, spp, mom, aov


def _assert_input_covers(spp, aov, what):
    """Sky pixels, at least 3 count levels with at least 5 hit pixels each, hit pixels at the minimum and at the cap."""
    hit = aov["hits"] > 0
    levels, counts = np.unique(spp[hit], return_counts=True)
    print(f"{what}: {int((~hit).sum())} sky pixels; hit pixels per count {dict(zip(levels.tolist(), counts.tolist()))}")
    assert (~hit).any() and (counts >= 5).sum() >= 3, (levels, counts)
    assert (spp[hit] == SPP["min_spp"]).any() and (spp[hit] == SPP["max_spp"]).any()


def test_the_rendered_setting_covers_the_cases_on_the_cpu():
    fb, spp, mom, aov = _oracle_inputs()
    _assert_input_covers(spp, aov, "oracle rtiow 77x45")
    gone = aov["hits"] == 0
    for moments in (mom, None):
        out = dsr.reference(fb, spp, moments, aov, SPP["min_spp"])
        assert_same(out[gone], fb[gone], "sky")
        assert np.isfinite(out).all() and (out[~gone] != fb[~gone]).any()
    _, var = dsr.reference(fb, spp, mom, aov, SPP["min_spp"], want_var=True)
    assert_same(var, _gauss(_sample_variance(spp, mom, aov, SPP["min_spp"]), ~gone), "var of a rendered frame")


def test_cli_refusals(test_config_text, tmp_path):
    before = sorted(os.listdir(tmp_path))

    def run(args):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    for args in (["--denoise-adaptive"], ["--denoise", "--denoise-adaptive"], ["--nee", "--denoise-adaptive"], ["--lit", "--denoise-adaptive"],
                 ["--lens", "0.1:10", "--denoise-adaptive"], ["--noise-target", "0.3", "--denoise-adaptive"],
                 ["--adaptive", "0.3", "--denoise-adaptive", "--denoise"], ["--adaptive", "0.3", "--denoise-adaptive", "--denoise-temporal"],
                 ["--adaptive", "0.3", "--denoise-adaptive", "--aov"], ["--lit", "--noise-target", "0.3", "--denoise-adaptive", "--denoise"],
                 ["--lit", "--noise-target", "0.3", "--denoise-adaptive", "--aov"],
                 ["--lit", "--noise-target", "0.3", "--denoise-adaptive", "--denoise-temporal"]):
        r = run(args)
        assert r.returncode == 2 and "--denoise-adaptive" in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    # the refusals that were there stay what they were
    r = run(["--adaptive", "0.1", "--denoise"])
    assert r.returncode == 2 and "adaptive" in r.stderr and "--denoise-adaptive" not in r.stderr, (r.returncode, r.stderr)
    r = run(["--lit", "--noise-target", "0.3", "--denoise"])
    assert r.returncode == 99 and "--noise-target" in r.stderr, (r.returncode, r.stderr)
    # the drivers --adaptive cannot be combined with refuse it with the flag as without
    for extra in (["--devices", "2"], ["--shard", "2"]):
        r = run(["--adaptive", "0.3", "--denoise-adaptive", *extra])
        assert r.returncode == 2 and "adaptive" in r.stderr, (extra, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before


# ---- on the GPU --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rtiow_frame(w=77, h=45):
    """An adaptive frame of rtiow with its moments and the AOVs at min_spp (shared: do not write to it)."""
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    fb, spp, mom, _ = dev.render_adaptive_to_host(rb.rtiow_camera(w, h, 1, 50), threshold=THRESHOLD, **SPP)
    aov, _ = dev.render_aov_to_host(rb.rtiow_camera(w, h, SPP["min_spp"], 50))
    dev.close()
    for a in (fb, spp, mom, *aov.values()):
        a.setflags(write=False)
    return fb, spp, mom, aov


def _check(fb, spp, mom, aov, aov_spp, what, **params):
    got = rb.denoise_spp_to_host(fb, spp, mom, aov, aov_spp, **params)
    assert_same(got, dsr.reference(fb, spp, mom, aov, aov_spp, **params), f"{what} {'with' if mom is not None else 'without'} moments {params}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("moments", [True, False])
def test_rendered_adaptive_frame_odd_size(moments):
    fb, spp, mom, aov = _rtiow_frame()
    _assert_input_covers(spp, aov, "rtiow 77x45")
    mom = mom if moments else None
    gone = aov["hits"] == 0
    for it in (0, 1, 5, 8):                  # at 8 the step of 128 exceeds the image
        got = _check(fb, spp, mom, aov, SPP["min_spp"], "rtiow 77x45", iterations=it)
        assert_same(got[gone], fb[gone], "sky pixels")
    _check(fb, spp, mom, aov, SPP["min_spp"], "rtiow 77x45", **OTHER)


@pytest.mark.gpu
def test_sub_images_one_pixel_wide_high_and_alone():
    fb, spp, mom, aov = _rtiow_frame()

    def cut(ys, xs):
        c = lambda a: np.ascontiguousarray(a[ys, xs])
        return c(fb), c(spp), c(mom), {k: c(v) for k, v in aov.items()}
    for what, ys, xs, params in (("45x1 column", slice(None), slice(30, 31), {}), ("1x77 row", slice(22, 23), slice(None), dict(iterations=8)),
                                 ("1x1", slice(22, 23), slice(40, 41), {})):
        f, n, m, a = cut(ys, xs)
        assert (a["hits"] > 0).any()
        _check(f, n, m, a, SPP["min_spp"], what, **params)
        _check(f, n, None, a, SPP["min_spp"], what, **params)


@pytest.mark.gpu
def test_lit_adaptive_frame_with_lens_and_environment():
    """DESIGN.md §19's setting d at 32 x 24: panel box, planes, tree, MIS, lens and the sun-and-sky map through rt_render_lit_adaptive,
    the AOVs through rt_render_aov_lens."""
    rb.amd_lib().rt_set_device(0)
    name = lar.SETTINGS["d"][0]
    host = tl.scene(name)
    with rb.Env(lar.sky()) as env:
        kw = lar.device_keywords("d", env)
        dev = rb.DeviceScene(host, device=0)
        fb, spp, mom, _ = dev.render_lit_adaptive_to_host(tl.camera(name, *lar.SIZE, 1), threshold=lar.THRESHOLD, **lar.SPP, **kw)
        aov, _ = dev.render_aov_lens_to_host(tl.camera(name, *lar.SIZE, lar.SPP["min_spp"]), lens=kw["lens"])
        dev.close()
    assert len(np.unique(spp)) >= 3 and (aov["hits"] > 0).any()
    for mom_ in (mom, None):
        _check(fb, spp, mom_, aov, lar.SPP["min_spp"], "lit setting d")
        _check(fb, spp, mom_, aov, lar.SPP["min_spp"], "lit setting d", iterations=2, sigma_luminance=1.5)


@pytest.mark.gpu
def test_synthetic_inputs_every_count_and_moment_case():
    fb, spp, mom, aov, a = _synthetic()
    gone = (aov["hits"] == 0) | (spp < 1)
    for mom_ in (mom, None):
        for it in (0, 1, 5):
            got = _check(fb, spp, mom_, aov, a, "synthetic 130x9", iterations=it)
            assert_same(got[gone], fb[gone], "pixels that are no hit pixels")
    _check(fb, spp, mom, aov, a, "synthetic 130x9", **OTHER)


@pytest.mark.gpu
def test_uniform_counts_without_moments_is_rt_denoise_device_against_device():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(77, 45, 8, 50)
    fb, _ = dev.render_to_host(cam)
    aov, _ = dev.render_aov_to_host(cam)
    dev.close()
    spp = np.full(fb.shape[:2], 8, np.int32)
    for params in (dict(), dict(iterations=0), dict(iterations=1), OTHER):
        assert_same(rb.denoise_spp_to_host(fb, spp, None, aov, 8, **params), rb.denoise_to_host(fb, aov, 8, **params), f"rt_denoise at 8 {params}")


@pytest.mark.gpu
def test_enqueued_on_a_side_stream():
    import torch
    w, h = 200, 120
    fb, spp, mom, aov = _rtiow_frame(w, h)
    want = dsr.reference(fb, spp, mom, aov, SPP["min_spp"], iterations=4)
    t = {"fb": torch.from_numpy(fb.copy()).to("cuda:0"), "spp": torch.from_numpy(spp.copy()).to("cuda:0"), "mom": torch.from_numpy(mom.copy()).to("cuda:0")}
    for key in ("albedo", "normal", "depth"):
        t[key] = torch.from_numpy(aov[key].copy()).to("cuda:0")
    t["hits"] = torch.from_numpy(aov["hits"].view(np.int32).copy()).to("cuda:0")
    out = torch.full_like(t["fb"], float("nan"))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rb.denoise_spp(t["fb"].data_ptr(), t["spp"].data_ptr(), t["mom"].data_ptr(), {k: t[k].data_ptr() for k in ("albedo", "normal", "depth", "hits")},
                       SPP["min_spp"], w, h, out.data_ptr(), stream=stream.cuda_stream, iterations=4)
    stream.synchronize()
    assert_same(out.cpu().numpy(), want, "side stream")


def _mse(fb, spp, truth):
    return float(np.mean((np.clip(fb / np.asarray(spp, F)[..., None], 0, 1) - truth) ** 2))


# rt_denoise_spp with moments over the noisy adaptive frame, as measured (noisy 1.53459e-3, with moments 6.93877e-4,
# without 6.68837e-4; uniform 19 spp 9.03043e-4, rt_denoise of it 3.95343e-4)
QUALITY_RATIO = 0.4522


@pytest.mark.gpu
def test_quality_against_a_1024_spp_ground_truth():
    """Measured, not promised: rtiow 320 x 180, 4:4:32 at t = 0.1, the MSE of the clamped mean against 1024 spp from
    sample 2^20 of the noisy adaptive frame, rt_denoise_spp with and without moments, and rt_denoise of a uniform frame at the rounded
    mean spp.  The with-moments figure is pinned against the noisy frame's at the measured ratio plus 10 %, so that a regression shows."""
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    cam = rb.rtiow_camera(320, 180, 1, 50)
    gt, _ = dev.render_to_host(rb.rtiow_camera(320, 180, 1024, 50), sample_first=1 << 20)
    truth = np.clip(gt / F(1024), 0, 1)
    fb, spp, mom, _ = dev.render_adaptive_to_host(cam, threshold=0.1, **SPP)
    aov, _ = dev.render_aov_to_host(rb.rtiow_camera(320, 180, SPP["min_spp"], 50))
    uniform_n = max(1, int(round(float(spp.mean()))))
    ucam = rb.rtiow_camera(320, 180, uniform_n, 50)
    ufb, _ = dev.render_to_host(ucam)
    uaov, _ = dev.render_aov_to_host(ucam)
    dev.close()
    noisy = _mse(fb, spp, truth)
    with_moments = _mse(rb.denoise_spp_to_host(fb, spp, mom, aov, SPP["min_spp"]), spp, truth)
    without = _mse(rb.denoise_spp_to_host(fb, spp, None, aov, SPP["min_spp"]), spp, truth)
    uniform = np.full(spp.shape, uniform_n, np.int32)
    uniform_noisy = _mse(ufb, uniform, truth)
    uniform_denoised = _mse(rb.denoise_to_host(ufb, uaov, uniform_n), uniform, truth)
    print(f"quality: adaptive frame at {float(spp.mean()):.2f} spp mean: noisy MSE {noisy:.6g}, rt_denoise_spp with moments {with_moments:.6g} "
          f"(ratio {with_moments / noisy:.4f}), without moments {without:.6g} (ratio {without / noisy:.4f}); uniform at {uniform_n} spp: noisy "
          f"{uniform_noisy:.6g}, rt_denoise {uniform_denoised:.6g}")
    assert with_moments <= 1.1 * QUALITY_RATIO * noisy


@pytest.mark.gpu
def test_cli_writes_the_python_paths_denoised_file(test_config_text, tmp_path):
    import torch
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    out = subprocess.run([EXE, "--gpu", "--adaptive", "0.3", "--adaptive-spp", "4:4:32", "--denoise-adaptive"], input=text, capture_output=True,
                         text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.from_config(text)
    cam = host.frame_camera(0)
    dev = rb.DeviceScene(host, device=0)
    fb, spp, mom, _ = dev.render_adaptive_to_host(cam, threshold=0.3, **SPP)
    cam4 = rb.CameraData.from_buffer_copy(cam)
    cam4.samples_per_pixel = SPP["min_spp"]
    aov, _ = dev.render_aov_to_host(cam4)
    dev.close()
    assert len(np.unique(spp)) >= 2
    want = dsr.reference(fb, spp, mom, aov, SPP["min_spp"])

    def file_bytes(frame):
        d_fb, d_spp = torch.from_numpy(np.ascontiguousarray(frame)).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
        rgb = torch.zeros(frame.shape, dtype=torch.uint8, device="cuda:0")
        assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == 0
        torch.cuda.synchronize()
        return np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes()
    assert_same(rb.denoise_spp_to_host(fb, spp, mom, aov, SPP["min_spp"]), want, "the Python path")
    assert open(tmp_path / "f_0.png.denoised", "rb").read() == file_bytes(want)
    assert open(tmp_path / "f_0.png", "rb").read() == file_bytes(fb), "the frame itself is --adaptive's"
    assert int(out.stdout.split("\n")[0].split("\t")[2]) == int(spp.sum())
