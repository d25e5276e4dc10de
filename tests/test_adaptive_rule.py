"""rt_render_adaptive_rule, rt_render_lit_adaptive_rule and rt_adaptive_judge: the neighbourhood stopping rule (include/rtp_amd.h "the
stopping rule of the adaptive calls").

Rule 1 changes goes_on alone, so the promises are §11's and §19's: fb, spp and moments equal the restatement
(adaptive_rule_reference.py) byte for byte, each stop level's pixels equal the uniform frame at that count, rule 0 and a NULL stop are
the old calls bit for bit.  The window logic — clipping at the buffer's border, rows of another band of a shard — is fed moments that
nobody rendered through rt_adaptive_judge.  On the CPU: the ABI, every refusal and its place in the order, the restatement on
synthetic moments, rule 0 of the new restatement against the old one, the CLI's refusals, the populations of the stop levels in every
GPU parity setting and what the rule buys at equal samples on the lit settings (pinned)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import adaptive_rule_reference as arr
import env_reference as er
import lit_adaptive_reference as lar
import rtp_bindings as rb
import test_adaptive as ta
import test_light_tree as tl
import test_lit_adaptive as tla
import tree_reference as tr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
FAKE = 1 << 32          # a device address that is never dereferenced
OK, INVALID, UNSUPPORTED = 0, 1, 4
F = np.float32
assert_same = ta.assert_same

SPP = dict(min_spp=4, batch_spp=4, max_spp=32)
LEVELS = list(range(4, 33, 4))
RTIOW_SIZE, RTIOW_T = (77, 45), 0.1
SHARDS = {"whole": None, "bands of 3": (3, 2, 1), "single rows": (1, 2, 0)}          # (single rows: no vertical neighbours at all)
LIT_T = {"a": 0.2, "b": 0.2, "c": 0.2, "d": 0.3, "e": 0.3}


def _shard(triple):
    return rb.Shard(*triple) if triple else None


# ---- the ABI and the refusals --------------------------------------------------------------------------------------------------

def test_abi_symbols_sizes_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_stop_params_init", "rt_render_adaptive_rule", "rt_render_lit_adaptive_rule", "rt_adaptive_judge"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.StopParams) == 16 and C.sizeof(rb.AdaptiveParams) == 20
    assert len(lib.rt_render_adaptive_rule.argtypes) == 11 and len(lib.rt_render_lit_adaptive_rule.argtypes) == 13
    assert len(lib.rt_adaptive_judge.argtypes) == 10
    p = rb.StopParams()
    p.rule, p.reserved[0], p.reserved[1] = 7, 7, 7
    lib.rt_stop_params_init(C.byref(p))
    assert (p.struct_bytes, p.rule, p.reserved[0], p.reserved[1]) == (16, 0, 0, 0)
    assert rb.stop_params(rule=1).rule == 1
    with pytest.raises(rb.RtError):
        rb.stop_params(window=5)
    assert lib.rt_version_string().decode().startswith("rtp_amd 0.5")
    with open(os.path.join(ROOT, "include", "rtp_amd.h")) as f:
        header = f.read()
    for decl in ("rt_status rt_render_adaptive_rule(", "rt_status rt_render_lit_adaptive_rule(", "rt_status rt_adaptive_judge(", "} rt_stop_params;"):
        assert decl in header, decl


def _params(**kw):
    return rb.adaptive_params(**{**dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.1), **kw})


def _stop(rule=1, struct_bytes=None):
    s = rb.stop_params(rule=rule)
    if struct_bytes is not None:
        s.struct_bytes = struct_bytes
    return s


def _call_plain(params="default", stop=None, cam="default", fb=FAKE, spp=2 * FAKE):
    lib = rb.amd_lib()
    params = _params() if params == "default" else params
    cam = rb.make_camera(8, 4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4) if cam == "default" else cam
    st = lib.rt_render_adaptive_rule(None, C.byref(cam) if cam is not None else None, None, C.byref(params) if params is not None else None,
                                     C.byref(stop) if stop is not None else None, C.c_void_p(fb), C.c_void_p(spp), None, None, 1, None)
    return st, lib.rt_get_last_error_string().decode()


def _call_lit(params="default", stop=None, lit="default", cam="default", fb=FAKE, spp=2 * FAKE, sample_first=0):
    lib = rb.amd_lib()
    params = _params() if params == "default" else params
    lit = rb.lit_params() if lit == "default" else lit
    cam = rb.make_camera(8, 4, 30.0, (0, 0, 0), (-1, 0, 0), spp=4) if cam == "default" else cam
    st = lib.rt_render_lit_adaptive_rule(None, C.byref(cam) if cam is not None else None, C.byref(lit) if lit is not None else None,
                                         C.byref(params) if params is not None else None, C.byref(stop) if stop is not None else None, None,
                                         sample_first, C.c_void_p(fb), C.c_void_p(spp), None, None, 1, None)
    return st, lib.rt_get_last_error_string().decode()


@pytest.mark.parametrize("call,name", [(_call_plain, "rt_render_adaptive_rule"), (_call_lit, "rt_render_lit_adaptive_rule")])
def test_refusals_and_their_order(call, name):
    """The rt_adaptive_params checks keep their codes and words; the stop checks come right after them and before everything else."""
    assert call(params=None)[0] == INVALID
    short = _params()
    short.struct_bytes = 4
    assert call(params=short)[0] == INVALID
    for kw, code, word in ((dict(min_spp=1), INVALID, "min_spp"), (dict(batch_spp=0), INVALID, "batch_spp"), (dict(max_spp=3), INVALID, "max_spp"),
                           (dict(threshold=-0.01), INVALID, "threshold"), (dict(threshold=float("nan")), INVALID, "threshold"),
                           (dict(threshold=float("inf")), INVALID, "threshold"), (dict(max_spp=65537), UNSUPPORTED, "65536")):
        for stop in (None, _stop(1), _stop(5)):          # (a bad rule does not overtake a bad parameter)
            st, msg = call(params=_params(**kw), stop=stop)
            assert st == code and word in msg, (kw, st, msg)
    # the stop checks: struct_bytes below 8, a rule outside {0, 1}; the message names the call
    for stop, word in ((_stop(1, struct_bytes=4), "struct_bytes"), (_stop(0, struct_bytes=0), "struct_bytes"), (_stop(2), "rule"), (_stop(-1), "rule"),
                       (_stop(1 << 20), "rule")):
        st, msg = call(stop=stop)
        assert st == INVALID and word in msg and name in msg, (stop.struct_bytes, stop.rule, st, msg)
        # … before the camera, the buffers and the scene
        st, msg = call(stop=stop, cam=None, fb=0)
        assert st == INVALID and word in msg and name in msg, msg
    # accepted: NULL, rule 0, rule 1, a struct of 8 bytes (an older caller's) — the next refusal is the scene's
    for stop in (None, _stop(0), _stop(1), _stop(1, struct_bytes=8), _stop(0, struct_bytes=8)):
        st, msg = call(stop=stop)
        assert st == INVALID and "null scene" in msg, msg
    garbage = _stop(1)
    garbage.reserved[0], garbage.reserved[1] = -3, 99          # (reserved is not read)
    assert "null scene" in call(stop=garbage)[1]


def test_lit_call_checks_stop_before_the_lit_parameters():
    bad_lens = rb.lit_params(lens=dict(lens_radius=-1.0))
    assert "rule" in _call_lit(stop=_stop(2), lit=bad_lens, sample_first=-1, fb=0)[1]
    assert "lens_radius" in _call_lit(stop=_stop(1), lit=bad_lens, sample_first=-1, fb=0)[1]
    assert "sample_first" in _call_lit(stop=_stop(1), sample_first=-1, fb=0)[1]
    assert "null framebuffer" in _call_lit(stop=_stop(1), fb=0)[1]
    assert "min_spp" in _call_lit(params=_params(min_spp=1), stop=_stop(2), lit=bad_lens)[1]


def test_judge_probe_refusals():
    lib = rb.amd_lib()

    def judge(width=4, rows=3, shard=None, params="default", stop="default", n=4, mom=FAKE, out=2 * FAKE):
        params = _params() if params == "default" else params
        stop = _stop(1) if stop == "default" else stop
        st = lib.rt_adaptive_judge(width, rows, C.byref(shard) if shard is not None else None, C.byref(params) if params is not None else None,
                                   C.byref(stop) if stop is not None else None, n, C.c_void_p(mom), None, C.c_void_p(out), None)
        return st, lib.rt_get_last_error_string().decode()
    for kw, code, word in ((dict(params=None), INVALID, "params"), (dict(params=_params(batch_spp=0)), INVALID, "batch_spp"),
                           (dict(stop=_stop(2)), INVALID, "rule"), (dict(stop=_stop(1, struct_bytes=4)), INVALID, "struct_bytes"),
                           (dict(width=0), INVALID, "width"), (dict(rows=0), INVALID, "rows"), (dict(width=1 << 13, rows=(1 << 11) + 1), UNSUPPORTED, "2^24"),
                           (dict(n=1), INVALID, "n below 2"), (dict(shard=rb.Shard(4, 3, 7)), INVALID, "shard"), (dict(mom=0), INVALID, "null"),
                           (dict(out=0), INVALID, "null")):
        st, msg = judge(**kw)
        assert st == code and word in msg and "rt_adaptive_judge" in msg, (kw, st, msg)


def test_cli_refusals(test_config_text, tmp_path):
    before = sorted(os.listdir(tmp_path))

    def run(args):
        return subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
    for args in (["--stop-rule", "near"], ["--stop-rule", "own"], ["--lit", "--stop-rule", "near"], ["--nee", "--stop-rule", "near"],
                 ["--noise-target", "0.3", "--stop-rule", "near"], ["--denoise", "--stop-rule", "near"],
                 ["--adaptive", "0.1", "--stop-rule", "far"], ["--adaptive", "0.1", "--stop-rule", "1"], ["--adaptive", "0.1", "--stop-rule"],
                 ["--lit", "--noise-target", "0.3", "--stop-rule", "Near"], ["--lit", "--noise-target", "0.3", "--stop-rule"]):
        r = run(args)
        assert r.returncode == 2 and "--stop-rule" in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))
    # the neighbouring refusals stay what they were, with the flag as without
    r = run(["--adaptive", "0.1", "--stop-rule", "near", "--denoise"])
    assert r.returncode == 2 and "adaptive" in r.stderr and "--stop-rule" not in r.stderr, (r.returncode, r.stderr)
    r = run(["--lit", "--noise-target", "0.3", "--stop-rule", "near", "--aov"])
    assert r.returncode == 99 and "--noise-target" in r.stderr, (r.returncode, r.stderr)


# ---- the restatement on synthetic moments ---------------------------------------------------------------------------------------

def _moments(rows, width, noisy_at, n=8):
    """Moments of n samples: quiet everywhere (a constant 0.5) but noisy at the given (row, column)s (half the samples 0, half 4)."""
    s1 = np.full((rows, width), F(0.5) * F(n), F)
    s2 = np.full((rows, width), F(0.25) * F(n), F)
    for r, c in noisy_at:
        s1[r, c] = F(4) * F(n // 2)
        s2[r, c] = F(16) * F(n // 2)
    return s1.ravel(), s2.ravel()


def _near(s1, s2, going_on, width, rows, shard=None, n=8, batch=4, max_spp=64, t=0.05):
    return arr.goes_on_near(s1, s2, going_on, n, width, rows, shard, batch, max_spp, t).reshape(rows, width)


def _window(rows, width, r, c, same_band=lambda a, b: True):
    want = np.zeros((rows, width), bool)
    for rr in range(max(r - 1, 0), min(r + 2, rows)):
        if rr == r or same_band(r, rr):
            want[rr, max(c - 1, 0):min(c + 2, width)] = True
    return want


def test_restatement_a_single_noisy_pixel_keeps_its_window_going():
    rows, width = 7, 9
    everyone = np.ones(rows * width, bool)
    for r, c in ((3, 4), (0, 0), (0, 8), (6, 0), (6, 8), (0, 4), (6, 3), (2, 0), (4, 8)):          # inside, the corners, the edges
        got = _near(*_moments(rows, width, [(r, c)]), everyone, width, rows)
        assert np.array_equal(got, _window(rows, width, r, c)), (r, c)
        assert got.sum() == (3 if 0 < r < rows - 1 else 2) * (3 if 0 < c < width - 1 else 2)
    assert not _near(*_moments(rows, width, []), everyone, width, rows).any()
    # a noisy pixel that has stopped keeps nobody going, and a stopped pixel does not resume beside a noisy one
    stopped = everyone.copy().reshape(rows, width)
    stopped[3, 4] = False
    assert not _near(*_moments(rows, width, [(3, 4)]), stopped.ravel(), width, rows).any()
    stopped = everyone.copy().reshape(rows, width)
    stopped[2, 3] = False
    want = _window(rows, width, 3, 4)
    want[2, 3] = False
    assert np.array_equal(_near(*_moments(rows, width, [(3, 4)]), stopped.ravel(), width, rows), want)


def test_restatement_nan_zero_threshold_and_cap():
    rows, width = 5, 6
    everyone = np.ones(rows * width, bool)
    s1, s2 = _moments(rows, width, [(2, 2)])
    for bad1, bad2 in ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.inf), (np.inf, 1.0)):
        a, b = s1.copy(), s2.copy()
        a[2 * width + 2], b[2 * width + 2] = bad1, bad2
        assert not _near(a, b, everyone, width, rows).any(), (bad1, bad2)          # the NaN pixel is quiet, and so is its window
    # huge but finite moments: S1 * mean overflows, var is fmaxf(0, -inf or NaN) = 0
    a, b = s1.copy(), s2.copy()
    a[0], b[0] = F(3e38), F(3e38)
    assert np.array_equal(_near(a, b, everyone, width, rows), _window(rows, width, 2, 2))
    # zero moments (a black pixel): quiet, by the floor
    assert not _near(np.zeros(rows * width, F), np.zeros(rows * width, F), everyone, width, rows).any()
    # t = 0: whoever is going on goes on, as long as the cap allows
    mask = np.arange(rows * width) % 3 != 0
    assert np.array_equal(_near(s1, s2, mask, width, rows, t=0.0).ravel(), mask)
    assert not _near(s1, s2, mask, width, rows, t=0.0, n=61).any()          # 61 + 4 > 64
    assert _near(s1, s2, everyone, width, rows, n=60).any() and not _near(s1, s2, everyone, width, rows, n=61).any()
    # a huge threshold: nothing is noisy
    assert not _near(s1, s2, everyone, width, rows, t=1e30).any()


def test_restatement_degenerate_images():
    for rows, width, at in ((1, 1, (0, 0)), (1, 7, (0, 0)), (1, 7, (0, 3)), (1, 7, (0, 6)), (7, 1, (0, 0)), (7, 1, (3, 0)), (7, 1, (6, 0))):
        got = _near(*_moments(rows, width, [at]), np.ones(rows * width, bool), width, rows)
        assert np.array_equal(got, _window(rows, width, *at)), (rows, width, at)


def test_restatement_shards():
    width = 5
    # {1, 2, 0}: bands of one row — no vertical neighbours at all
    rows = 6
    for r in range(rows):
        got = _near(*_moments(rows, width, [(r, 2)]), np.ones(rows * width, bool), width, rows, shard=(1, 2, 0))
        assert np.array_equal(got, _window(rows, width, r, 2, lambda a, b: False)), r
    # {3, 2, 1}: neighbours inside a band of three buffer rows only; 8 rows = bands 0 0 0 1 1 1 2 2 (the last one cut by the image)
    rows = 8
    for r in range(rows):
        got = _near(*_moments(rows, width, [(r, 0)]), np.ones(rows * width, bool), width, rows, shard=rb.Shard(3, 2, 1))
        assert np.array_equal(got, _window(rows, width, r, 0, lambda a, b: a // 3 == b // 3)), r
    # one part, or no shard: the whole image
    for shard in (None, (3, 1, 0), (0, 2, 0)):
        got = _near(*_moments(rows, width, [(3, 2)]), np.ones(rows * width, bool), width, rows, shard=shard)
        assert np.array_equal(got, _window(rows, width, 3, 2)), shard


def test_restatement_rounds_on_synthetic_samples():
    """The rounds: counts are levels, a quiet pixel beside a noisy one goes on with it, one far away stops at min_spp, and a pixel that
    stopped never resumes."""
    rng = np.random.default_rng(11)
    rows, width = 6, 8
    rad = np.full((rows * width, 64, 3), F(0.5))
    rad[2 * width + 3] = rng.uniform(0, 4, (64, 3)).astype(F)
    n, s1, s2 = arr.reference(rad, width, rows, None, 4, 4, 64, 0.05, 1)
    n = n.reshape(rows, width)
    assert ((n - 4) % 4 == 0).all() and n.max() <= 64
    assert n[2, 3] > 4 and (n[1:4, 2:5] == n[2, 3]).all()
    outside = ~_window(rows, width, 2, 3)
    assert (n[outside] == 4).all()
    assert (arr.reference(rad, width, rows, None, 4, 4, 64, 0.0, 1)[0] == 64).all()
    assert (arr.reference(rad, width, rows, None, 4, 7, 64, 0.0, 1)[0] == 60).all()
    assert (arr.reference(rad, width, rows, None, 4, 4, 64, 1e30, 1)[0] == 4).all()
    assert (arr.reference(rad, width, rows, None, 6, 4, 6, 0.05, 1)[0] == 6).all()
    # single-row bands: the rows above and below stop at min_spp
    n1 = arr.reference(rad, width, rows, (1, 2, 0), 4, 4, 64, 0.05, 1)[0].reshape(rows, width)
    assert (n1[2, 2:5] == n[2, 3]).all() and (np.delete(n1, 2, axis=0) == 4).all()


@functools.lru_cache(maxsize=None)
def _rtiow_radiances():
    """The oracle's per-sample radiances of rtiow at RTIOW_SIZE, (H, W, 32, 3) (shared: do not write to it)."""
    import oracle_bindings as ob
    w, h = RTIOW_SIZE
    jj, ii, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(SPP["max_spp"]), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], axis=1).astype(np.int32)
    rad = ob.trace_samples(rb.HostScene.rtiow(), rb.rtiow_camera(w, h, 1, 50), ijs)[0].reshape(h, w, SPP["max_spp"], 3)
    rad.setflags(write=False)
    return rad


@functools.lru_cache(maxsize=None)
def _rtiow_reference(shard_name, rule=1, t=RTIOW_T):
    w, h = RTIOW_SIZE
    rows = er.image_rows(rb.rtiow_camera(w, h, 1, 50), _shard(SHARDS[shard_name]))
    return arr.from_radiances(_rtiow_radiances()[rows], SHARDS[shard_name], threshold=t, rule=rule, **SPP)


@functools.lru_cache(maxsize=None)
def _lit_reference(setting, sample_first=0, shard_name="whole", rule=1):
    rows = er.image_rows(tl.camera(lar.SETTINGS[setting][0], lar.SIZE[0], lar.SIZE[1], 1), _shard(SHARDS[shard_name]))
    rad = lar.setting_radiances(setting, sample_first)[rows]
    return arr.from_radiances(rad, SHARDS[shard_name], threshold=LIT_T[setting], rule=rule, **SPP)


def test_rule_0_of_the_new_restatement_is_the_old_one():
    w, h = RTIOW_SIZE
    flat = _rtiow_radiances().reshape(h * w, SPP["max_spp"], 3)
    for t, spp in ((0.1, SPP), (0.3, SPP), (0.0, SPP), (1e30, SPP), (0.2, dict(min_spp=2, batch_spp=3, max_spp=32))):
        for shard in SHARDS.values():          # (rule 0 does not look at the buffer's shape)
            got = arr.reference(flat, w, h, shard, spp["min_spp"], spp["batch_spp"], spp["max_spp"], t, 0)
            want = ta.reference(flat, spp["min_spp"], spp["batch_spp"], spp["max_spp"], t)
            for g, x, what in zip(got, want, ("counts", "S1", "S2")):
                assert_same(g, x, f"t={t} {what}")
    for setting in ("a", "e"):
        rad = lar.setting_radiances(setting)
        got = arr.from_radiances(rad, None, threshold=lar.THRESHOLD, rule=0, **SPP)
        for g, x, what in zip(got, lar.from_radiances(rad, threshold=lar.THRESHOLD, **SPP), ("fb", "spp", "moments")):
            assert_same(g, x, f"setting {setting} {what}")


@pytest.mark.parametrize("shard_name", list(SHARDS))
def test_every_stop_level_is_populated_rtiow(shard_name):
    """The condition on the inputs of the GPU tests: each of the 8 levels holds at least 5 pixels under rule 1."""
    _, spp, _ = _rtiow_reference(shard_name)
    counts = [int((spp == n).sum()) for n in LEVELS]
    print(f"rtiow {RTIOW_SIZE} {shard_name}: pixels per level {dict(zip(LEVELS, counts))}")
    assert sum(counts) == spp.size and min(counts) >= 5, counts
    if shard_name == "whole":
        assert min(counts) == 116          # (the figure the rule was prototyped with: a disagreement is one with the rule as written)


@pytest.mark.parametrize("setting,smallest", [("a", 21), ("b", 23), ("c", 16), ("d", 48), ("e", 18)])
def test_every_stop_level_is_populated_lit(setting, smallest):
    _, spp, _ = _lit_reference(setting)
    counts = [int((spp == n).sum()) for n in LEVELS]
    print(f"setting {setting} t={LIT_T[setting]}: pixels per level {dict(zip(LEVELS, counts))}")
    assert sum(counts) == spp.size and min(counts) >= 5, counts
    assert min(counts) == smallest


# ---- quality, on the restatement: what rule 1 buys at equal samples --------------------------------------------------
# §19's metric, truth protocol and sizes (48 x 32, 8:8:128, two 4096-spp halves — test_lit_adaptive._quality_inputs, shared with §19's
# own test), rule 1 at t = 0.05.  Deterministic: pinned at relative 1e-4.  The conditions: below 1, and below rule 0's ratio at the t
# of RULE_0_THRESHOLDS whose mean spp is nearest.
QUALITY_SPP = tla.QUALITY_SPP
QUALITY_T = 0.05
QUALITY_RATIOS = {"a": 0.717752, "b": 0.681116}
RULE_0_THRESHOLDS = (0.02, 0.03, 0.05, 0.1, 0.2)


def _lit_ratio(setting, fb, spp, truth):
    name = lar.SETTINGS[setting][0]
    mean_spp = float(spp.mean())
    uniform_n = max(1, int(round(mean_spp)))
    ufb = tr.frame(tl.scene(name), tl.camera(name, 48, 32, uniform_n), **lar.reference_keywords(setting))
    adaptive, uniform = tla._mse(fb, spp, truth), tla._mse(ufb, np.full(spp.shape, uniform_n), truth)
    return mean_spp, uniform_n, adaptive, uniform


@pytest.mark.parametrize("setting", list(QUALITY_RATIOS))
def test_quality_against_uniform_and_against_rule_0(setting):
    truth, truth_var, rad = tla._quality_inputs(setting)
    fb, spp, _ = arr.from_radiances(rad, None, threshold=QUALITY_T, rule=1, **QUALITY_SPP)
    mean_spp, uniform_n, adaptive, uniform = _lit_ratio(setting, fb, spp, truth)
    ratio = adaptive / uniform
    own = []
    for t in RULE_0_THRESHOLDS:
        fb0, spp0, _ = arr.from_radiances(rad, None, threshold=t, rule=0, **QUALITY_SPP)
        m0, n0, a0, u0 = _lit_ratio(setting, fb0, spp0, truth)
        own.append((abs(m0 - mean_spp), t, m0, a0 / u0))
    _, t0, m0, ratio0 = min(own)
    print(f"quality {lar.SETTINGS[setting][0]} rule 1 t={QUALITY_T}: adaptive MSE {adaptive:.6g} at {mean_spp:.2f} spp mean ({np.unique(spp).size} levels), "
          f"uniform {uniform:.6g} at {uniform_n} spp, ratio {ratio:.6f}; rule 0 at t={t0} ({m0:.2f} spp mean): ratio {ratio0:.6f}; the truth's own "
          f"variance {truth_var:.3g} = {100 * truth_var / min(adaptive, uniform):.2f} % of the smaller")
    assert truth_var < 0.05 * min(adaptive, uniform), "the ratio would measure the truth"
    assert ratio < 1 and ratio < ratio0, (ratio, ratio0)
    want = QUALITY_RATIOS[setting]
    assert abs(ratio - want) <= 1e-4 * want, ratio


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def _check_triple(got, want, what):
    for g, w, col in zip(got[:3], want, ("fb", "spp", "moments")):
        assert_same(g, w, f"{what}: {col}")


@pytest.mark.gpu
def test_rtiow_equals_the_restatement():
    """fb, spp and moments byte for byte: the whole frame and both shards, on the default handle and a TRAVERSAL_EXACT one."""
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(*RTIOW_SIZE, 1, 50)
    for config in (dict(), dict(traversal=rb.TRAVERSAL_EXACT)):
        dev = rb.DeviceScene(host, device=0, **config)
        for name, triple in SHARDS.items():
            got = dev.render_adaptive_to_host(cam, shard=_shard(triple), threshold=RTIOW_T, rule=1, **SPP)
            _check_triple(got, _rtiow_reference(name), f"rtiow {config} {name}")
        _check_triple(dev.render_adaptive_to_host(cam, threshold=RTIOW_T, rule=0, **SPP), _rtiow_reference("whole", 0), f"rtiow {config} rule 0")
        dev.close()
    # a sharded frame is not the whole frame's rows (the header says so): the parts see no rows of each other
    rows = er.image_rows(cam, _shard(SHARDS["single rows"]))
    assert not np.array_equal(_rtiow_reference("single rows")[1], _rtiow_reference("whole")[1][rows])


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(lar.SETTINGS))
def test_lit_equals_the_restatement(setting):
    rb.amd_lib().rt_set_device(0)
    name = lar.SETTINGS[setting][0]
    host, cam = tl.scene(name), tl.camera(name, lar.SIZE[0], lar.SIZE[1], 1)
    with rb.Env(lar.sky()) as env:
        kw = lar.device_keywords(setting, env)
        dev = rb.DeviceScene(host, device=0)
        for first in (0, 37):
            for shard_name in ("whole", "bands of 3") if first == 0 else ("whole",):
                got = dev.render_lit_adaptive_to_host(cam, shard=_shard(SHARDS[shard_name]), sample_first=first, threshold=LIT_T[setting], rule=1, **SPP,
                                                      **kw)
                _check_triple(got, _lit_reference(setting, first, shard_name), f"{setting} first={first} {shard_name}")
                assert got[3].trace_launches == 1 + 7 and got[3].traced_samples == got[1].size * SPP["min_spp"]
        dev.close()


@pytest.mark.gpu
def test_per_pixel_parity_device_against_device():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(*RTIOW_SIZE, 1, 50)
    dev = rb.DeviceScene(host, device=0)
    for name, triple in SHARDS.items():
        fb, spp, _ = ta._check_parity(dev, cam, f"rtiow rule 1 {name}", shard=_shard(triple), threshold=RTIOW_T, rule=1, **SPP)
        assert np.unique(spp).tolist() == LEVELS
    dev.close()
    name = lar.SETTINGS["b"][0]
    host, cam = tl.scene(name), tl.camera(name, lar.SIZE[0], lar.SIZE[1], 1)
    kw = lar.device_keywords("b", None)
    dev = rb.DeviceScene(host, device=0)
    fb, spp, _, _ = dev.render_lit_adaptive_to_host(cam, threshold=LIT_T["b"], rule=1, **SPP, **kw)
    assert np.unique(spp).tolist() == LEVELS
    for n in LEVELS:
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = n
        sel = spp == n
        assert_same(fb[sel], dev.render_lit_to_host(c, **kw)[0][sel], f"lit pixels with {n} samples")
    dev.close()


@pytest.mark.gpu
def test_identities():
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(64, 36, 1, 50)
    dev = rb.DeviceScene(host, device=0)
    p = dict(threshold=0.1, **SPP)
    old = dev.render_adaptive_to_host(cam, **p)
    assert len(np.unique(old[1])) >= 3
    _check_triple(dev.render_adaptive_to_host(cam, rule=0, **p), old, "rule 0 = rt_render_adaptive")
    # stop == NULL through the new entry point
    import torch
    d_fb = torch.full((36, 64, 3), float("nan"), device="cuda:0")
    d_spp = torch.full((36, 64), -1, dtype=torch.int32, device="cuda:0")
    d_mom = torch.full((36, 64, 2), float("nan"), device="cuda:0")
    ap = rb.adaptive_params(**p)
    torch.cuda.synchronize()
    assert lib.rt_render_adaptive_rule(dev._h, C.byref(cam), None, C.byref(ap), None, C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()),
                                       C.c_void_p(d_mom.data_ptr()), None, 1, None) == OK
    _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), old, "stop NULL = rt_render_adaptive")
    assert not np.array_equal(dev.render_adaptive_to_host(cam, rule=1, **p)[1], old[1]), "rule 1 is another rule"

    def uniform(n):
        return ta._uniform(dev, cam, n)
    fb, spp, _, _ = dev.render_adaptive_to_host(cam, rule=1, min_spp=4, batch_spp=4, max_spp=32, threshold=0.0)
    assert (spp == 32).all()
    assert_same(fb, uniform(32), "rule 1, threshold 0 = rt_render at the cap")
    fb, spp, _, _ = dev.render_adaptive_to_host(cam, rule=1, min_spp=4, batch_spp=5, max_spp=32, threshold=0.0)
    assert (spp == 29).all()
    assert_same(fb, uniform(29), "rule 1, threshold 0, cap not reached")
    huge = dev.render_adaptive_to_host(cam, rule=1, min_spp=6, batch_spp=4, max_spp=64, threshold=1e30)
    assert (huge[1] == 6).all()
    assert_same(huge[0], uniform(6), "rule 1, huge threshold = rt_render at min_spp")
    _check_triple(dev.render_adaptive_to_host(cam, rule=1, min_spp=6, batch_spp=4, max_spp=6, threshold=0.05), huge, "min == max")
    # max_depth <= 0: counts by the rule
    flat = rb.rtiow_camera(64, 36, 1, 0)
    fbz, sppz, momz, _ = dev.render_adaptive_to_host(flat, rule=1, **p)
    assert not fbz.any() and not momz.any() and (sppz == 4).all()
    assert (dev.render_adaptive_to_host(flat, rule=1, threshold=0.0, **SPP)[1] == 32).all()
    dev.close()
    # the lit call: rule 0 and the old call; rule 1 at threshold 0 = rt_render_lit at the cap
    name = lar.SETTINGS["a"][0]
    host, cam = tl.scene(name), tl.camera(name, lar.SIZE[0], lar.SIZE[1], 1)
    kw = lar.device_keywords("a", None)
    dev = rb.DeviceScene(host, device=0)
    old = dev.render_lit_adaptive_to_host(cam, threshold=lar.THRESHOLD, **SPP, **kw)
    _check_triple(dev.render_lit_adaptive_to_host(cam, threshold=lar.THRESHOLD, rule=0, **SPP, **kw), old, "lit rule 0 = rt_render_lit_adaptive")
    fb, spp, _, _ = dev.render_lit_adaptive_to_host(cam, threshold=0.0, rule=1, sample_first=5, **SPP, **kw)
    c = rb.CameraData.from_buffer_copy(cam)
    c.samples_per_pixel = 32
    assert (spp == 32).all()
    assert_same(fb, dev.render_lit_to_host(c, sample_first=5, **kw)[0], "lit rule 1, threshold 0 = rt_render_lit at the cap")
    fb, spp, _, t = dev.render_lit_adaptive_to_host(cam, threshold=1e30, rule=1, **SPP, **kw)
    c.samples_per_pixel = 4
    assert (spp == 4).all() and t.trace_launches == 8
    assert_same(fb, dev.render_lit_to_host(c, **kw)[0], "lit rule 1, huge threshold = rt_render_lit at min_spp")
    dev.close()


def _judge_moments(rng, rows, width, n):
    """Moments of n samples per pixel: quiet and noisy pixels mixed, then NaN, zero, huge and negative ones sprinkled in."""
    y = np.where(rng.random((rows, width, 1)) < 0.3, rng.uniform(0, 4, (rows, width, n)), rng.uniform(0.4, 0.6, (rows, width, 1)) + np.zeros(n)).astype(F)
    s1, s2 = np.zeros((rows, width), F), np.zeros((rows, width), F)
    for s in range(n):
        s1 = (s1 + y[..., s]).astype(F)
        s2 = (s2 + (y[..., s] * y[..., s]).astype(F)).astype(F)
    mom = np.stack([s1, s2], axis=-1)
    special = np.array([[np.nan, 1], [1, np.nan], [np.nan, np.nan], [0, 0], [3e38, 3e38], [np.inf, np.inf], [1e-30, 1e-38], [-4, 8], [1e20, 1e38]], F)
    k = max(1, rows * width // 6)
    at = rng.choice(rows * width, k, replace=False)
    mom.reshape(-1, 2)[at] = special[rng.integers(0, len(special), k)]
    return mom


@pytest.mark.gpu
@pytest.mark.parametrize("width,rows", [(130, 9), (1, 1), (1, 77), (45, 1), (257, 3)])
def test_judge_against_the_restatement(width, rows):
    """One judgement over moments nobody rendered: widths that are no multiple of the block of 256 and rows that straddle a
    workgroup, random going-on masks (a round's launches) and every pixel (the first judgement's), both rules, the whole frame and
    both shards, the cap and t = 0."""
    rb.amd_lib().rt_set_device(0)
    rng = np.random.default_rng(width * 1000 + rows)
    n = 8
    mom = _judge_moments(rng, rows, width, n)
    s1, s2 = mom[..., 0].ravel(), mom[..., 1].ravel()
    masks = [None, rng.random((rows, width)) < 0.7, rng.random((rows, width)) < 0.1, np.zeros((rows, width), bool)]
    for triple in SHARDS.values():
        for mask in masks:
            going = np.ones(rows * width, bool) if mask is None else mask.ravel()
            for t, batch, max_spp in ((0.05, 4, 64), (0.3, 4, 64), (0.0, 4, 64), (0.05, 4, 11), (0.05, 4, 12), (1e30, 4, 64)):
                p = dict(min_spp=4, batch_spp=batch, max_spp=max_spp, threshold=t)
                got = rb.adaptive_judge(mom, n, mask, shard=_shard(triple), rule=1, **p)
                want = arr.goes_on_near(s1, s2, going, n, width, rows, triple, batch, max_spp, t).reshape(rows, width)
                assert np.array_equal(got, want), (triple, t, max_spp, None if mask is None else int(mask.sum()), np.argwhere(got != want)[:5])
                got0 = rb.adaptive_judge(mom, n, mask, shard=_shard(triple), rule=0, **p)
                want0 = (going & ta.goes_on(s1, s2, n, batch, max_spp, t)).reshape(rows, width)
                assert np.array_equal(got0, want0), (triple, t, max_spp, "rule 0")


@pytest.mark.gpu
def test_judge_single_noisy_pixels_on_the_device():
    """The synthetic windows of the CPU tests, through the kernels: corners, edges, band borders."""
    rb.amd_lib().rt_set_device(0)
    rows, width = 8, 9
    p = dict(min_spp=4, batch_spp=4, max_spp=64, threshold=0.05)
    for triple, same in ((None, lambda a, b: True), ((3, 2, 1), lambda a, b: a // 3 == b // 3), ((1, 2, 0), lambda a, b: False)):
        for r, c in ((3, 4), (0, 0), (0, 8), (7, 0), (7, 8), (2, 4), (5, 0), (6, 8)):
            s1, s2 = _moments(rows, width, [(r, c)])
            got = rb.adaptive_judge(np.stack([s1, s2], axis=1).reshape(rows, width, 2), 8, None, shard=_shard(triple), rule=1, **p)
            assert np.array_equal(got, _window(rows, width, r, c, same)), (triple, r, c)


@pytest.mark.gpu
def test_handle_state():
    import torch
    rb.amd_lib().rt_set_device(0)
    name = lar.SETTINGS["b"][0]
    host, cam = tl.scene(name), tl.camera(name, lar.SIZE[0], lar.SIZE[1], 1)
    cam4 = rb.CameraData.from_buffer_copy(cam)
    cam4.samples_per_pixel = 4
    kw = lar.device_keywords("b", None)
    p = dict(threshold=LIT_T["b"], **SPP)
    dev = rb.DeviceScene(host, device=0)
    want_own = dev.render_adaptive_to_host(cam, rule=0, **p)[:3]
    dev.close()
    dev = rb.DeviceScene(host, device=0)
    want_near = dev.render_adaptive_to_host(cam, rule=1, **p)[:3]
    dev.close()
    dev = rb.DeviceScene(host, device=0)
    dev.render_to_host(cam4)
    before = dev.last_timing()
    _check_triple(dev.render_lit_adaptive_to_host(cam, rule=1, **p, **kw), _lit_reference("b"), "lit rule 1")
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    _check_triple(dev.render_adaptive_to_host(cam, rule=0, **p), want_own, "rule 0 after a rule-1 call, as on a fresh handle")
    _check_triple(dev.render_adaptive_to_host(cam, rule=1, **p), want_near, "rule 1 after a rule-0 call, as on a fresh handle")
    _check_triple(dev.render_adaptive_to_host(cam, **p), want_own, "rt_render_adaptive after a rule-1 call")
    # a larger frame after a smaller one (the flag buffer grows), then the smaller one again
    big = tl.camera(name, 96, 64, 1)
    fresh = rb.DeviceScene(host, device=0)
    want_big = fresh.render_lit_adaptive_to_host(big, rule=1, **p, **kw)[:3]
    fresh.close()
    _check_triple(dev.render_lit_adaptive_to_host(big, rule=1, **p, **kw), want_big, "a larger frame on a used handle")
    _check_triple(dev.render_lit_adaptive_to_host(cam, rule=1, **p, **kw), _lit_reference("b"), "the smaller frame again")
    # sync = 0 on a side stream
    s = torch.cuda.Stream()
    h, w = lar.SIZE[1], lar.SIZE[0]
    d_fb = torch.full((h, w, 3), float("nan"), device="cuda:0")
    d_spp = torch.full((h, w), -1, dtype=torch.int32, device="cuda:0")
    d_mom = torch.full((h, w, 2), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dev.render_lit_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), d_mom.data_ptr(), stream=s.cuda_stream, sync=False, rule=1, **p, **kw)
    s.synchronize()
    _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy(), d_mom.cpu().numpy()), _lit_reference("b"), "lit, sync = 0 on a side stream")
    d_fb.fill_(float("nan"))
    d_spp.fill_(-1)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dev.render_adaptive(cam, d_fb.data_ptr(), d_spp.data_ptr(), None, stream=s.cuda_stream, sync=False, rule=1, **p)
    s.synchronize()
    _check_triple((d_fb.cpu().numpy(), d_spp.cpu().numpy()), want_near[:2], "sync = 0 on a side stream, null moments")
    # a refused call enqueues nothing
    d_fb.fill_(float("nan"))
    torch.cuda.synchronize()
    ap, bad = rb.adaptive_params(**p), rb.stop_params(rule=2)
    assert rb.amd_lib().rt_render_adaptive_rule(dev._h, C.byref(cam), None, C.byref(ap), C.byref(bad), C.c_void_p(d_fb.data_ptr()),
                                                C.c_void_p(d_spp.data_ptr()), None, None, 1, None) == INVALID
    torch.cuda.synchronize()
    assert torch.isnan(d_fb).all()
    dev.close()


@pytest.mark.gpu
def test_cli_stop_rule_near_frames_are_the_python_path(test_config_text, tmp_path):
    import torch
    text = test_config_text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    rb.amd_lib().rt_set_device(0)

    def file_bytes(cam, fb, spp):
        d_fb, d_spp = torch.from_numpy(fb).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
        rgb = torch.zeros(fb.shape, dtype=torch.uint8, device="cuda:0")
        assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == OK
        torch.cuda.synchronize()
        return np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes()

    def run(directory, args):
        directory.mkdir()
        ls = text.split("\n")
        ls[1] = str(directory / "f_%d.png")
        out = subprocess.run([EXE, "--gpu", *args], input="\n".join(ls), capture_output=True, text=True, timeout=200)
        assert out.returncode == 0, out.stderr
        return open(directory / "f_0.png", "rb").read(), int(out.stdout.split("\n")[0].split("\t")[2])
    host = rb.HostScene.from_config(text)
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera(0)
    # --adaptive
    near, samples = run(tmp_path / "near", ["--adaptive", "0.3", "--adaptive-spp", "4:4:32", "--stop-rule", "near"])
    fb, spp, _, _ = dev.render_adaptive_to_host(cam, threshold=0.3, rule=1, **SPP)
    assert len(np.unique(spp)) >= 2
    assert near == file_bytes(cam, fb, spp) and samples == int(spp.sum())
    own, _ = run(tmp_path / "own", ["--adaptive", "0.3", "--adaptive-spp", "4:4:32", "--stop-rule", "own"])
    plain, _ = run(tmp_path / "plain", ["--adaptive", "0.3", "--adaptive-spp", "4:4:32"])
    assert own == plain and own != near
    # --lit --noise-target
    lit_args = ["--lit", "--nee", "--light-tree", "--noise-target", "0.3", "--noise-spp", "4:4:32"]
    near, samples = run(tmp_path / "lit_near", [*lit_args, "--stop-rule", "near"])
    fb, spp, _, _ = dev.render_lit_adaptive_to_host(host.frame_camera_at(0.0), nee=dict(select=1), threshold=0.3, rule=1, **SPP)
    assert near == file_bytes(cam, fb, spp) and samples == int(spp.sum())
    own, _ = run(tmp_path / "lit_own", [*lit_args, "--stop-rule", "own"])
    plain, _ = run(tmp_path / "lit_plain", lit_args)
    assert own == plain
    dev.close()


@pytest.mark.gpu
def test_cli_denoise_adaptive_works_with_the_rule(test_config_text, tmp_path):
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    out = subprocess.run([EXE, "--gpu", "--adaptive", "0.3", "--adaptive-spp", "4:4:32", "--stop-rule", "near", "--denoise-adaptive"], input=text,
                         capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    frame, denoised = open(tmp_path / "f_0.png", "rb").read(), open(tmp_path / "f_0.png.denoised", "rb").read()
    assert len(frame) == len(denoised) and frame != denoised


# rtiow 320 x 180 from the device: rule 1's ratio to uniform rt_render at the rounded mean spp, as measured —
# deterministic, the device's bits are the restatement's.  Two truths.  §11's (1024 spp from sample 2^20) gives the pinned figures that
# compare with §11's and §20's.  Its own variance cannot be below 5 % of an 80-spp frame's MSE — a 1024-spp mean has 80 / 1024 = 7.8 % of
# an 80-spp mean's variance: measured 8.95 % at 8:8:128 (2.17 % at 4:4:32) — so the 5 % condition is asserted under a second truth made by
# §19's protocol, two 2048-spp halves from samples 2^20 and 2^21, under which the conditions (below 1, below rule 0) are asserted again
# and the ratio pinned too.  A truth's variance adds the same amount to both MSEs and so moves a ratio towards 1: the figures under
# §11's truth understate the win.
RTIOW_QUALITY = {(8, 8, 128, 0.03): (0.803077, 0.791248), (4, 4, 32, 0.08): (0.756517, 0.754083)}          # (§11's truth, the fine truth)


@functools.lru_cache(maxsize=None)
def _rtiow_truths():
    """(§11's truth, its variance from its two 512-spp halves, the fine truth, its variance from its two 2048-spp halves) (shared)."""
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)

    def mean(n, first):
        return dev.render_to_host(rb.rtiow_camera(320, 180, n, 50), sample_first=first)[0].astype(np.float64) / n

    def variance(a, b):
        return float(np.mean((np.clip(a, 0, 1) - np.clip(b, 0, 1)) ** 2)) / 4
    truth = np.clip(mean(1024, 1 << 20), 0, 1)
    var = variance(mean(512, 1 << 20), mean(512, (1 << 20) + 512))
    halves = [mean(2048, 1 << 20), mean(2048, 1 << 21)]
    dev.close()
    return truth, var, np.clip((halves[0] + halves[1]) / 2, 0, 1), variance(*halves)


@pytest.mark.gpu
@pytest.mark.parametrize("mn,batch,mx,t", list(RTIOW_QUALITY))
def test_quality_rtiow_on_the_device(mn, batch, mx, t):
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(320, 180, 1, 50)
    truth, truth_var, fine, fine_var = _rtiow_truths()
    dev = rb.DeviceScene(host, device=0)

    def frames(rule, threshold):
        fb, spp, _, _ = dev.render_adaptive_to_host(cam, min_spp=mn, batch_spp=batch, max_spp=mx, threshold=threshold, rule=rule)
        mean_spp = float(spp.mean())
        uniform_n = max(1, int(round(mean_spp)))
        return mean_spp, uniform_n, fb, spp, ta._uniform(dev, cam, uniform_n)
    mean_spp, uniform_n, fb, spp, ufb = frames(1, t)
    own = [(abs(f[0] - mean_spp), t0, f) for t0, f in ((t0, frames(0, t0)) for t0 in RULE_0_THRESHOLDS)]
    _, t0, (m0, n0, fb0, spp0, ufb0) = min(own, key=lambda o: o[:2])
    dev.close()
    got = []
    for name, tr_, var in (("§11's truth", truth, truth_var), ("the fine truth", fine, fine_var)):
        adaptive, uniform = tla._mse(fb, spp, tr_), tla._mse(ufb, np.full(spp.shape, uniform_n), tr_)
        ratio0 = tla._mse(fb0, spp0, tr_) / tla._mse(ufb0, np.full(spp0.shape, n0), tr_)
        print(f"quality rtiow {mn}:{batch}:{mx} rule 1 t={t}, {name}: adaptive MSE {adaptive:.6g} at {mean_spp:.2f} spp mean, uniform {uniform:.6g} at "
              f"{uniform_n} spp, ratio {adaptive / uniform:.6f}; rule 0 at t={t0} ({m0:.2f} spp mean): ratio {ratio0:.6f}; the truth's own variance "
              f"{var:.3g} = {100 * var / min(adaptive, uniform):.2f} % of the smaller")
        assert adaptive / uniform < 1 and adaptive / uniform < ratio0, (name, adaptive / uniform, ratio0)
        got.append((adaptive / uniform, var / min(adaptive, uniform)))
    assert got[1][1] < 0.05, "the ratio would measure the truth"
    want = RTIOW_QUALITY[(mn, batch, mx, t)]
    for (ratio, _), pin in zip(got, want):
        assert ratio <= 1.1 * pin, "a regression against the measured ratio"
        assert abs(ratio - pin) <= 1e-4 * pin, ratio
