"""Random lit scenes for the glossy and the medium kernels: test_lit_fuzz.py's protocol on the 34 glossy instantiations of
§23 and the 16 medium instantiations of §25, on scenes nobody arranged — tests/lit_fuzz.py's glossy twins (gloss_case: a trial's geometry,
table, tree, camera and map with its dull materials made METAL of fuzz 0 … 1.5) under lit_fuzz.fuzz_medium's media.

On the CPU: the twins and media have the properties they aim at, the GPU tests' own call lists reach all 50 kernels through
rt_capi.hip's dispatch rule, the restatements' tallies are all met, medium_reference.intervals agrees with a float64 statement of the
region's geometry within a derived bound, and the restatements have rt_render's expectation on every twin.  On the GPU: probed samples,
frames and adaptive frames equal the restatements bit for bit.

Four tallies of medium_ref.c that no random medium reaches, and what covers them.  `u_zero`: the free-flight draw is (float)state / 2^32,
which is 0 only for state == 0 — one state in 2^32, and wang_hash is a bijection, so exactly one sample index per pixel starts its medium
stream there: u_zero_probes() inverts the hash and finds it (a crafted case; the device runs it too).  `box_parallel_in` and
`box_parallel_out`: a direction component of exactly 0 never comes from a jittered camera; the fan camera (fan_camera) makes every
primary ray have d.x == 0.  `black` needs an albedo of (0, 0, 0): the crafted ball with albedo 0 around the camera.  Every other tally is
met on the random media.  No tally is provably unreachable."""
import functools

import numpy as np
import pytest

import emit_reference as emr
import gloss_reference as gr
import lit_adaptive_reference as lar
import lit_fuzz as lf
import medium_reference as mr
import nee_reference as nr
import rtp_bindings as rb
from test_glossy import possible_counters
from test_lit_fuzz import FRAME, PROBE_SIZE, _blocks, _compare, probe_set
from test_light_tree import LUM, _zscores, assert_same
from test_medium import rb_wang

U = 2.0 ** -24          # the unit roundoff of float32
TARGET = "lit_gloss_render_kernel<true, TreeTable>"          # the one pair held to 3 waves per SIMD


# ---- B.1 the twins and the media ------------------------------------------------------------------------------------------------------------
def _bytes_of(host):
    d = host.desc
    return (bytes(np.ctypeslib.as_array(d.spheres, shape=(d.num_spheres,)).view(np.uint8)),
            bytes(np.ctypeslib.as_array(d.planes, shape=(d.num_planes,)).view(np.uint8)) if d.num_planes else b"",
            bytes(np.ctypeslib.as_array(d.materials, shape=(d.num_materials,)).view(np.uint8)))


def _glossy_share(c, ijs):
    cam = c.camera(*PROBE_SIZE, 1, 50)
    kw = dict(glossy=1, select=1, planes=1, lens=c.lens, cam_close=c.close(*PROBE_SIZE, 1, 50))
    if c.env is not None:
        kw.update(glossy_env=1, rgb=c.env, env_params=c.env_params(1))
    out = gr.trace(c.host, cam, ijs, **kw)
    assert np.isfinite(out[0]).all(), c.name
    return float((out[5][:, 0] > 0).mean()), out[5].sum(0)


def test_twins():
    """A twin takes its trial's draws: the camera, lens, map and rotation are the original's, its table and tree equal the original's
    in every column, it adds at most one sphere (non-emissive, the last), and case(trial)'s own bytes are what a fresh Case gives
    (making the twin did not move them).  Over the eight twins the METAL fuzz values are exactly lit_fuzz.GLOSS_FUZZ, every one of them
    on a primitive; and at least 10 % of probe_set()'s samples take a glossy light sample with both switches on, on every twin."""
    fuzz = set()
    for t in lf.TRIALS:
        before = _bytes_of(lf.case(t).host)
        c, o = lf.gloss_case(t), lf.case(t)
        assert _bytes_of(lf.Case(t).host) == before == _bytes_of(o.host), "case(trial) moved"
        assert _bytes_of(lf.Case(t, remat=lf.gloss_rule(lf.SEEDS[t], t)).host) == _bytes_of(c.host), "the twin is no function of (seed, trial)"
        assert (c.eye, c.eye_close, c.background, c.vfov, c.lens, c.rot, c.motion) == (o.eye, o.eye_close, o.background, o.vfov, o.lens, o.rot, o.motion)
        assert (c.env is None) == (o.env is None) and (c.env is None or np.array_equal(c.env, o.env))
        d, od = c.host.desc, o.host.desc
        assert d.num_planes == od.num_planes and d.num_spheres - od.num_spheres == (t % 2)
        if t % 2:
            assert max(d.materials[d.spheres[d.num_spheres - 1].material_idx].emit.e[:]) == 0
        for planes in (0, 1):
            for a, b in zip(emr.table(c.host, planes), emr.table(o.host, planes)):
                assert np.array_equal(a, b), (t, planes)
            ta, tb = lf.tr.tree(c.host, planes), lf.tr.tree(o.host, planes)
            for col in lf.tr.COLUMNS:
                assert np.array_equal(ta[col], tb[col]), (t, planes, col)
        used = {d.spheres[k].material_idx for k in range(d.num_spheres)} | {d.planes[k].material_idx for k in range(d.num_planes)}
        fuzz |= {float(d.materials[k].fuzz) for k in used if d.materials[k].type == lf.MAT_METAL}
        assert {float(d.materials[k].fuzz) for k in range(d.num_materials) if d.materials[k].type == lf.MAT_METAL} <= set(np.float32(lf.GLOSS_FUZZ).tolist())
        share, cnt = _glossy_share(c, probe_set())
        print(f"{c.name}: {share:.4f} of the probes take a glossy light sample; counters {dict(zip(gr.COUNTERS, cnt.tolist()))}")
        assert share >= 0.10, (c.name, share)
    assert fuzz == set(np.float32(lf.GLOSS_FUZZ).tolist()), sorted(fuzz)
    assert 2.0 ** -11 < lf.RT_GLOSSY_MIN_FUZZ == 2.0 ** -10 and sum(0.3 <= f <= 0.4 for f in fuzz) == 1


def test_media():
    """fuzz_medium over the eight trials: every region at least twice; the eye inside a ball and inside a box; the eye outside a region
    that holds some emitters and not others; g over {0, 0.7, -0.5, 0.95, -0.95}; an albedo channel of exactly 0 and one of exactly 1;
    sigma_t from 0.02 to 5 with one optically thick region; all space on a trial with a map."""
    media = [lf.fuzz_medium(t) for t in lf.TRIALS]
    assert media == [lf.fuzz_medium(t) for t in lf.TRIALS]
    kinds = ["ball" if m.get("ball") else "box" if m.get("box") else "all" for m in media]
    assert all(kinds.count(k) >= 2 for k in ("all", "ball", "box")), kinds
    inside = {k: 0 for k in ("ball", "box")}
    partial = thick = 0
    for t, (m, kind) in enumerate(zip(media, kinds)):
        c = lf.gloss_case(t)
        rb.medium_params(**m)
        assert 0.02 <= m["sigma_t"] <= 5.0 and abs(m["g"]) <= 0.95
        if kind == "all":
            assert c.env is not None, "all space goes with a map: the environment is not sampled there"
            continue
        eye_in = lf.inside_medium(m, c.eye)
        inside[kind] += eye_in
        kd, idx = emr.table(c.host, 1)[:2]
        d = c.host.desc
        held = [lf.inside_medium(m, d.spheres[i].center.e[:]) for k, i in zip(kd, idx) if k == 0]
        partial += (not eye_in) and 0 < sum(held) < len(held)
        thick += lf.medium_extent(m) * m["sigma_t"] >= 10.0
        print(t, kind, "eye inside", eye_in, "emitting spheres inside / outside", sum(held), len(held) - sum(held))
    assert inside["ball"] >= 1 and inside["box"] >= 1 and partial >= 1 and thick >= 1, (inside, partial, thick)
    assert {m["g"] for m in media} == {0.0, 0.7, -0.5, 0.95, -0.95}
    channels = [x for m in media for x in np.broadcast_to(np.asarray(m["albedo"], np.float32), (3,)).tolist()]
    assert 0.0 in channels and 1.0 in channels
    assert min(m["sigma_t"] for m in media) == 0.02 and max(m["sigma_t"] for m in media) == 5.0


# ---- B.2 coverage --------------------------------------------------------------------------------------------------------------------------
def test_every_gloss_and_medium_kernel_is_reached():
    """The GPU tests' own call lists, through lit_fuzz.kernels_of and each twin's own table, launch all 34 + 16 instantiations and no
    other; every frame kernel meets a whole frame, a shard and sample_first = 37; every lit_gloss_* and medium_* kernel meets an
    environment and its absence, and every lit_gloss_* kernel each of (gn, ge) = (1, 0), (0, 1), (1, 1)."""
    reached, shards, envs, switches = {}, {}, {}, {}
    for call in lf.gloss_calls():
        for k in lf.kernels_of_gcall(call):
            reached.setdefault(k, set()).add((call.test, call.trial))
            envs.setdefault(k, set()).add(call.env is not None)
            switches.setdefault(k, set()).add((call.gn, call.ge if call.env is not None else 0))
            if call.test.endswith("frames"):
                shards.setdefault(k, set()).add(call.shard)
    gloss, medium = lf.all_gloss_kernels(), lf.all_medium_kernels()
    assert len(gloss) == 34 == len(set(gloss)) and len(medium) == 16 == len(set(medium)) and len(lf.all_kernels()) == 34
    assert not set(gloss) & set(medium) and not set(gloss + medium) & set(lf.all_kernels())
    want = sorted(gloss + medium)
    assert sorted(reached) == want, (sorted(set(want) - set(reached)), sorted(set(reached) - set(want)))
    for k, s in shards.items():
        assert s == {0, 1, 2}, (k, s)
    assert sorted(shards) == sorted(k for k in want if "_render_kernel" in k and "list" not in k)
    for k in want:
        if k.startswith(("lit_gloss_", "medium_")):
            assert envs[k] == {True, False}, (k, envs[k])
        if k.startswith("lit_gloss_"):
            assert switches[k] >= {(1, 0), (0, 1), (1, 1)}, (k, switches[k])
    assert _target_frame_calls(), "no frame call reaches " + TARGET + " on a twin without planes or with sample_planes = 0"
    # the rule itself, on the cases its inputs distinguish
    K = lf.kernels_of
    assert K(lf.LIT_FRAME, glossy_nee=1, emitters=False) == ("lit_render_kernel<false, NeeTable>",)
    assert K(lf.LIT_FRAME, glossy_env=1, env=False) == ("lit_render_kernel<false, NeeTable>",)
    assert K(lf.LIT_FRAME, True, 1, 1, True, glossy_env=1, env=True, emitters=False) == ("lit_gloss_render_kernel<true, NeeTable>",)
    assert K(lf.LIT_PROBE, True, 0, 1, True, glossy_nee=1) == ("lit_gloss_probe_kernel<true, TreeTable>",)
    assert K(lf.LIT_ADAPTIVE, False, 1, 0, True, glossy_nee=1) == ("lit_gloss_render_kernel<false, EmitTable>", "lit_gloss_list_render_kernel<false, EmitTable>")
    assert K(lf.NEE_FRAME, sample_planes=1, select=1, table_has_plane=True, glossy_nee=1) == ("light_gloss_render_kernel<TreeEmitTable>",)
    assert K(lf.NEE_PROBE, glossy_nee=0, glossy_env=1) == ("light_probe_kernel<NeeTable>",)
    assert K(lf.ENV_PROBE, glossy_env=1, env=True) == ("light_gloss_probe_kernel<EnvDev>",) and K(lf.ENV_FRAME, glossy_nee=1) == ("light_render_kernel<EnvDev>",)
    assert K(lf.MEDIUM_FRAME, True, 1, 1, True, medium_on=True) == ("medium_render_kernel<true, TreeEmitTable>",)
    assert K(lf.MEDIUM_PROBE, False, 1, 1, True, medium_on=True, emitters=False, glossy_nee=1) == ("medium_probe_kernel<false, NeeTable>",)
    assert K(lf.MEDIUM_FRAME, True, 1, 1, True, medium_on=False) == ("lit_render_kernel<true, TreeEmitTable>",)
    assert K(lf.MEDIUM_PROBE, medium_on=False, glossy_nee=1) == ("lit_gloss_probe_kernel<false, NeeTable>",)
    for k in want:
        print(k, sorted(reached[k], key=str)[:3])


def _target_frame_calls():
    return [c for t in lf.TRIALS for c in lf.gloss_frame_calls(t)
            if TARGET in lf.kernels_of_gcall(c) and (c.planes == 0 or not lf.gloss_case(t).has_planes(1))]


# ---- B.3 tallies ---------------------------------------------------------------------------------------------------------------------------
def _gloss_probe_reference(call, ijs):
    """gloss_reference.trace's columns for a nee, env or lit probe call on a twin."""
    c = lf.gloss_case(call.trial)
    w, h = PROBE_SIZE
    cam = c.camera(w, h, 1, 50)
    if call.entry in (lf.NEE_PROBE, lf.NEE_FRAME):
        return gr.trace(c.host, cam, ijs, glossy=1, select=call.select, nee_mis=call.mis, planes=call.planes)
    if call.entry in (lf.ENV_PROBE, lf.ENV_FRAME):
        return gr.trace(c.host, cam, ijs, glossy=0, glossy_env=1, emitters=False, rgb=c.env, env_params=c.env_params(call.env))
    return gr.trace(c.host, cam, ijs, **lf.gloss_reference_keywords(call, w, h, 1, 50))


def _counter_class(call):
    if call.entry in (lf.NEE_PROBE, lf.NEE_FRAME) or (call.gn, call.ge) == (1, 0):
        return "nee"
    if call.entry in (lf.ENV_PROBE, lf.ENV_FRAME) or (call.gn, call.ge) == (0, 1):
        return "env"
    return "lit glossy=11"


def test_gloss_tallies():
    """gloss_ref.c's six tallies over the twins' own probe calls: all six > 0 for the lit calls with both switches; for the nee and env
    calls (and the lit calls with one switch) the ones test_glossy.possible_counters allows."""
    total = {k: dict.fromkeys(gr.COUNTERS, 0) for k in ("nee", "env", "lit glossy=11")}
    for t in lf.TRIALS:
        for call in lf.gloss_probe_calls(t):
            cnt = _gloss_probe_reference(call, probe_set())[5].sum(0)
            for k, v in zip(gr.COUNTERS, cnt.tolist()):
                total[_counter_class(call)][k] += v
    for name, cnt in total.items():
        print(name, cnt)
        for k in possible_counters(name):
            assert cnt[k] > 0, (name, k, cnt)
    assert possible_counters("lit glossy=11") == gr.COUNTERS


def fan_camera(w=16, h=16, spp=8, depth=12):
    """A pinhole camera whose every primary ray has d.x == 0 exactly: pixel_delta_u = 0 and pixel00_loc.x == origin.x (built from a view
    direction that is not parallel to the up vector)."""
    cam = rb.make_camera(w, h, 40.0, (0.5, 1.0, 9.0), (0.5, 1.2, 0.0), (0.1, 0.2, 0.3), spp, depth)
    for k in range(3):
        cam.pixel_delta_u.e[k] = 0.0
    cam.pixel00_loc.e[0] = cam.origin.e[0]
    return cam


FAN_BOXES = {"inside": (-1.0, -4.0, -4.0, 1.0, 4.0, 4.0), "on the face": (0.5, -4.0, -4.0, 2.0, 4.0, 4.0), "beside": (1.0, -4.0, -4.0, 2.0, 4.0, 4.0)}
FAN_TRIAL = 2


def fan_medium(name):
    return dict(sigma_t=0.5, albedo=0.9, g=0.3, box=FAN_BOXES[name])


def all_ijs(w, h, spp):
    i, j, s = np.meshgrid(np.arange(w), np.arange(h), np.arange(spp), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), s.ravel()], 1).astype(np.int32)


BALL_TRIAL = 4


def ball_camera_case(albedo):
    """A camera inside a ball: twin BALL_TRIAL, a ball of radius 5 around its eye."""
    c = lf.gloss_case(BALL_TRIAL)
    return c, dict(sigma_t=0.35, albedo=albedo, g=0.7, ball=c.eye + (5.0,))


def _unwang(y):
    """wang_hash's inverse (every step of the hash is a bijection of the 32-bit words)."""
    y &= 0xFFFFFFFF
    x = y
    for _ in range(3):
        x = y ^ (x >> 15)
    y = (x * pow(0x27D4EB2D, -1, 1 << 32)) & 0xFFFFFFFF
    x = y
    for _ in range(8):
        x = y ^ (x >> 4)
    y = (x * pow(9, -1, 1 << 32)) & 0xFFFFFFFF
    hi = y >> 16
    return (hi << 16) | ((y & 0xFFFF) ^ hi ^ 61)


def u_zero_probes(w, h, count=4):
    """(i, j, s) whose medium stream's first draw is exactly 0: the stream starts at wang(seed ^ key) and a draw is wang(state) / 2^32, so
    seed = unwang(unwang(0)) ^ key and s = unwang(seed) - wang(i * w + j), for the pixels where that is a valid index (< 2^31)."""
    seed = _unwang(_unwang(0)) ^ 0x4D454431
    assert rb_wang(rb_wang(seed ^ 0x4D454431)) == 0
    out = []
    for i in range(w):
        for j in range(h):
            s = (_unwang(seed) - rb_wang(i * w + j)) & 0xFFFFFFFF
            if s < (1 << 31) and len(out) < count:
                assert rb_wang(rb_wang(i * w + j) + s) == seed
                out.append((i, j, s))
    return np.array(out, np.int32)


def _medium_probe_reference(call, ijs, stats=False):
    c = lf.gloss_case(call.trial)
    w, h = PROBE_SIZE
    return mr.trace(c.host, c.camera(w, h, 1, 50), ijs, stats=stats, **lf.gloss_reference_keywords(call, w, h, 1, 50))


def test_medium_tallies():
    """medium_ref.c's tallies (they only count: test_medium.py passes unchanged, and every column here is the same with and without
    them) over the twins' own medium probe calls and the crafted cases — the fan camera, the camera inside a ball with albedo 0, and the
    probes whose free-flight draw is exactly 0: every tally > 0 somewhere."""
    total = dict.fromkeys(mr.STATS, 0)

    def add(st):
        for k, v in st.items():
            total[k] += v
    for t in lf.TRIALS:
        per = dict.fromkeys(mr.STATS, 0)
        for call in lf.medium_probe_calls(t):
            out = _medium_probe_reference(call, probe_set(), stats=True)
            assert np.isfinite(out[0]).all(), call
            for k, v in out[5].items():
                per[k] += v
        print(lf.gloss_case(t).name, lf.fuzz_medium(t), per)
        add(per)
    call = lf.medium_probe_calls(3)[0]
    plain = _medium_probe_reference(call, probe_set())
    for a, b in zip(plain, _medium_probe_reference(call, probe_set(), stats=True)[:5]):
        assert_same(a, b, "the tallies only count")
    random_only = dict(total)
    host = lf.gloss_case(FAN_TRIAL).host
    for name in FAN_BOXES:
        add(mr.trace(host, fan_camera(), all_ijs(16, 16, 8), medium=fan_medium(name), stats=True)[5])
    c, m = ball_camera_case(0.0)
    out = mr.trace(c.host, c.camera(*PROBE_SIZE, 1, 50), probe_set(), medium=m, stats=True)
    assert (out[3][out[2] > 0] == mr.END_BLACK).all() and out[5]["black"] == int((out[2] > 0).sum()) > 0
    add(out[5])
    c, m = ball_camera_case((0.9, 0.8, 0.7))
    zero = u_zero_probes(*PROBE_SIZE)
    out = mr.trace(c.host, c.camera(*PROBE_SIZE, 1, 50), zero, medium=m, stats=True)
    assert len(zero) == 4 and out[5]["u_zero"] >= 4 and out[5]["event_first_ray"] == 0
    add(out[5])
    print("random media", random_only)
    print("with the crafted cases", total)
    for k in mr.STATS:
        assert total[k] > 0, (k, total)
    for k in ("box_parallel_in", "box_parallel_out", "u_zero", "black"):
        assert random_only[k] == 0, (k, "a random medium reaches it now: say so in the module's docstring")


# ---- B.4 the region's interval ---------------------------------------------------------------------------------------------------------------
BOX = dict(sigma_t=1.0, box=(-1.0, -2.0, -0.5, 2.0, 1.0, 3.0))
BALL = dict(sigma_t=1.0, ball=(0.5, -1.0, 2.0, 1.5))
INF = float("inf")


def _one(medium, o, d, t_end=INF):
    hit, t0, t1 = mr.intervals(medium, [o], [d], t_end)
    return int(hit[0]), float(t0[0]), float(t1[0])


def test_intervals_exact_cases():
    # box, a direction component exactly 0, the origin strictly inside that slab: the axis does not clip
    assert _one(BOX, (0.0, -4.0, 1.0), (0.0, 2.0, 0.0)) == (1, 1.0, 2.5)
    assert _one(BOX, (1.9999999, -4.0, 1.0), (0.0, 2.0, 0.0)) == (1, 1.0, 2.5)
    assert _one(BOX, (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)) == (1, 0.0, 1.5), "both other axes parallel and inside, the origin inside: t0 == 0"
    # … the origin exactly on a face, or outside: empty
    for x in (-1.0, 2.0, 2.5, -1.5):
        assert _one(BOX, (x, -4.0, 1.0), (0.0, 2.0, 0.0))[0] == 0, x
    assert _one(BOX, (0.0, 1.0, 1.0), (1.0, 0.0, 0.0))[0] == 0 and _one(BOX, (0.0, -2.0, 1.0), (1.0, 0.0, 0.5))[0] == 0
    # a ray pointing away
    assert _one(BOX, (0.0, -4.0, 1.0), (0.0, -2.0, 0.0))[0] == 0 and _one(BOX, (5.0, 0.0, 1.0), (1.0, 0.25, 0.125))[0] == 0
    assert _one(BALL, (0.5, -1.0, 6.0), (0.0, 0.0, 1.0))[0] == 0
    # t_end <= t0: empty; just behind it: cut there
    assert _one(BOX, (0.0, -4.0, 1.0), (0.0, 2.0, 0.0), 1.0)[0] == 0 and _one(BOX, (0.0, -4.0, 1.0), (0.0, 2.0, 0.0), 0.5)[0] == 0
    assert _one(BOX, (0.0, -4.0, 1.0), (0.0, 2.0, 0.0), 1.25) == (1, 1.0, 1.25)
    assert _one(BALL, (0.5, -1.0, 6.0), (0.0, 0.0, -2.0), 1.25)[0] == 0 and _one(BALL, (0.5, -1.0, 6.0), (0.0, 0.0, -2.0), 1.5) == (1, 1.25, 1.5)
    assert _one(None, (1.0, 2.0, 3.0), (0.0, 0.0, 1.0), 0.0)[0] == 0 and _one(dict(sigma_t=1.0), (1.0, 2.0, 3.0), (0.0, 0.0, 1.0), 7.0) == (1, 0.0, 7.0)
    # t_end = inf
    assert _one(BOX, (0.0, -4.0, 1.0), (0.0, 2.0, 0.0), INF) == (1, 1.0, 2.5) and _one(BALL, (0.5, -1.0, 6.0), (0.0, 0.0, -2.0)) == (1, 1.25, 2.75)
    assert _one(dict(sigma_t=1.0), (1.0, 2.0, 3.0), (0.0, 0.0, 1.0)) == (1, 0.0, INF)
    # the origin inside: t0 == 0
    assert _one(BOX, (0.0, 0.0, 1.0), (1.0, 0.5, 0.25)) == (1, 0.0, 2.0) and _one(BALL, (0.5, -1.0, 2.0), (0.0, 0.0, 4.0)) == (1, 0.0, 0.375)
    # ball, disc <= 0: a tangent from exactly representable numbers (the ray x = 2, y = -1 touches the ball of radius 1.5 about (0.5, -1, 2))
    assert _one(BALL, (2.0, -1.0, -3.0), (0.0, 0.0, 1.0))[0] == 0 and _one(BALL, (2.5, -1.0, -3.0), (0.0, 0.0, 1.0))[0] == 0
    assert _one(BALL, (1.75, -1.0, -3.0), (0.0, 0.0, 1.0))[0] == 1


def _random_rays(rng, centre, radius, n):
    """n rays: origins inside the region's bounding ball, outside within 4 radii, and 10^3 radii away, in thirds; two thirds aimed at a
    point near the region, the rest anywhere; one ray in 16 has a direction component of exactly 0."""
    unit = rng.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1)[:, None]
    third = np.arange(n) % 3
    dist = np.where(third == 0, rng.uniform(0.0, 1.0, n) ** (1 / 3), np.where(third == 1, rng.uniform(1.0, 4.0, n), 1000.0 * rng.uniform(0.9, 1.1, n)))
    o = (centre + radius * dist[:, None] * unit).astype(np.float32)
    aim = centre + radius * rng.uniform(-1.2, 1.2, (n, 3))
    d = np.where((np.arange(n) % 4 == 3)[:, None], rng.normal(size=(n, 3)), (aim - o) * rng.uniform(0.2, 3.0, n)[:, None]).astype(np.float32)
    zero = np.arange(n) % 16 == 5
    d[zero, rng.integers(0, 3, int(zero.sum()))] = 0.0
    t_end = np.where(np.arange(n) % 5 == 0, rng.uniform(0.0, 2.0, n) * dist * radius / np.maximum(np.linalg.norm(d, axis=1), 1e-30), np.inf).astype(np.float32)
    return o, d, t_end


def _box64(box, o, d, t_end):
    """The box's interval in float64 → (t0, t1, e0, e1, empty): e0, e1 bound |float32 - float64| for t0, t1; empty: a parallel axis
    outside its slab."""
    a, b = np.array(box[:3], np.float64), np.array(box[3:], np.float64)
    o, d, t_end = o.astype(np.float64), d.astype(np.float64), t_end.astype(np.float64)
    par = d == 0.0
    empty = (par & ~((a < o) & (o < b))).any(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (a - o) / d, (b - o) / d
    lo, hi = np.where(par, -np.inf, np.minimum(ta, tb)), np.where(par, np.inf, np.maximum(ta, tb))
    t0, t1 = np.maximum(0.0, lo.max(1)), np.minimum(t_end, hi.min(1))
    # each bound is fl(fl(a - o) / d): two correctly rounded operations, (1 + e1)(1 + e2) - 1 <= 2 U + U^2 relative (results are normal
    # or 0 here; 2^-149 covers a subnormal quotient); max and min are 1-Lipschitz in the sup norm, so the largest candidate's bound holds
    rel = 2.0 * U + U * U
    e0 = rel * np.where(par, 0.0, np.abs(np.minimum(ta, tb))).max(1) + 2.0 ** -149
    e1 = rel * np.where(par, 0.0, np.abs(np.maximum(ta, tb))).max(1) + 2.0 ** -149
    return t0, t1, e0, e1, empty


def _ball64(ball, o, d, t_end):
    """The ball's interval in float64 → (t0, t1, e0, e1, disc, edisc): the forward error of the float32 expressions, term by term."""
    c, R = np.array(ball[:3], np.float64), float(ball[3])
    o, d, t_end = o.astype(np.float64), d.astype(np.float64), t_end.astype(np.float64)
    oc = o - c
    A, hb, oo = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1)
    cc = oo - R * R
    disc = hb * hb - A * cc

    def gamma(k):
        return k * U / (1.0 - k * U)
    # oc_i = fl(o_i - c_i): relative U each.  A three-term dot product in float32: gamma(3) x the sum of the terms' magnitudes
    eA = gamma(3) * A
    ehb = gamma(4) * (np.abs(oc) * np.abs(d)).sum(1)                    # U from oc, gamma(3) from the dot
    ecc = gamma(5) * oo + U * R * R                                       # oc twice, the dot; fl(R * R)
    ecc = ecc + U * (np.abs(cc) + ecc)                                    # the subtraction
    e1 = (2.0 * np.abs(hb) + ehb) * ehb
    e1 = e1 + U * (hb * hb + e1)                                          # fl(hb * hb)
    e2 = A * ecc + np.abs(cc) * eA + eA * ecc
    e2 = e2 + U * (A * np.abs(cc) + e2)                                   # fl(A * cc)
    edisc = e1 + e2
    edisc = edisc + U * (np.abs(disc) + edisc)                            # the subtraction: the forward error of hb^2 - A cc
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(np.maximum(disc, 0.0))
        # |sqrt(x) - sqrt(y)| <= |x - y| / sqrt(max(x, y)) and <= sqrt|x - y|; then the root's own rounding
        esq = np.minimum(edisc / np.maximum(sq, 1e-300), np.sqrt(edisc))
        esq = esq + U * (sq + esq)
        out = []
        for sign in (-1.0, 1.0):
            num = -hb + sign * sq
            en = ehb + esq
            en = en + U * (np.abs(num) + en)                              # fl(-hb -+ sq)
            t = num / A
            et = (en + np.abs(t) * eA) / (A - eA)                         # the quotient of two perturbed numbers
            et = et + U * (np.abs(t) + et) + 2.0 ** -149                  # its rounding
            out.append((t, et))
    (ta, ea), (tb, eb) = out
    return np.maximum(ta, 0.0), np.minimum(tb, t_end), ea, eb, disc, edisc


@pytest.mark.parametrize("region", ["box", "ball", "all space"])
def test_intervals_against_float64(region):
    """10^5 random rays per region — origins inside, outside and 10^3 radii away — against the same geometry in float64: the hit flag is
    the float64 one wherever the float64 interval is longer (or, where empty, more overlapped) than the bound, and t0, t1 lie within the
    bound derived beside _box64 / _ball64 from the float32 expressions' roundings.  Nothing is tuned: the ratio printed is observed
    error over bound (DESIGN.md §27 records it)."""
    rng = np.random.default_rng([26, len(region)])
    n = 100000
    if region == "box":
        centre, radius = (np.array(BOX["box"][:3]) + np.array(BOX["box"][3:])) / 2, float(np.linalg.norm(np.array(BOX["box"][3:]) - np.array(BOX["box"][:3])) / 2)
    else:
        centre, radius = np.array(BALL["ball"][:3]), BALL["ball"][3]
    o, d, t_end = _random_rays(rng, centre, radius, n)
    d[np.abs(d).sum(1) == 0] = 1.0
    medium = BOX if region == "box" else BALL if region == "ball" else dict(sigma_t=1.0)
    hit, t0, t1 = mr.intervals(medium, o, d, t_end)
    t0, t1 = t0.astype(np.float64), t1.astype(np.float64)
    if region == "all space":
        assert (t0 == 0).all() and (t1 == t_end).all() and (hit == (t_end > 0)).all()
        return
    if region == "box":
        w0, w1, e0, e1, empty = _box64(BOX["box"], o, d, t_end)
        assert not hit[empty].any() and empty.sum() > 100
        decided = ~empty
    else:
        w0, w1, e0, e1, disc, edisc = _ball64(BALL["ball"], o, d, t_end)
        assert not hit[disc < -edisc].any(), "a ray that misses the ball by more than the bound"
        decided = disc > edisc
        print(f"ball: disc decided on {int((np.abs(disc) > edisc).sum())} of {n} rays")
    length = w1 - w0
    bound = e0 + e1
    must_hit, must_miss = decided & (length > bound), decided & (length < -bound)
    assert hit[must_hit].all() and not hit[must_miss].any()
    inside, far = (np.arange(n) % 3 == 0) & (hit == 1), (np.arange(n) % 3 == 2) & (hit == 1)
    assert must_hit.sum() > 20000 and must_miss.sum() > 1000 and inside.sum() > 10000 and far.sum() > 1000, (must_hit.sum(), must_miss.sum(), inside.sum(), far.sum())
    if region == "ball":
        assert (t0[inside & (np.linalg.norm(o - centre, axis=1) < 0.99 * radius)] == 0).all(), "an origin inside starts at 0"
    ok = must_hit & (hit == 1)
    r0 = np.abs(t0 - w0)[ok] / e0[ok]
    fin = np.isfinite(w1[ok])
    r1 = np.abs(t1 - w1)[ok][fin] / e1[ok][fin]
    assert (t1[ok][~fin] == np.inf).all()
    print(f"{region}: {int(ok.sum())} rays compared; largest |t0 - float64| / bound {r0.max():.4f}, |t1 - float64| / bound {r1.max():.4f}")
    assert r0.max() <= 1.0 and r1.max() <= 1.0, (r0.max(), r1.max())


def test_fan_camera():
    """Every primary ray of the fan camera has d.x == 0 exactly, so the box's parallel branch decides the camera ray: a box whose x-slab
    holds origin.x has events; a box with a.x == origin.x and one beside it have no event on any sample's first ray."""
    cam = fan_camera()
    assert cam.pixel00_loc.e[0] == cam.origin.e[0] == 0.5 and not any(cam.pixel_delta_u.e[:]) and cam.pixel_delta_v.e[0] == 0.0
    assert all(np.isfinite(cam.pixel00_loc.e[:])) and all(np.isfinite(cam.pixel_delta_v.e[:])) and any(cam.pixel_delta_v.e[:])
    host = lf.gloss_case(FAN_TRIAL).host
    ijs = all_ijs(16, 16, 8)
    for name in FAN_BOXES:
        out = mr.trace(host, cam, ijs, medium=fan_medium(name), stats=True)
        st = out[5]
        print(name, "events", st["events"], "on the first ray", st["event_first_ray"], "parallel in / out", st["box_parallel_in"], st["box_parallel_out"])
        assert np.isfinite(out[0]).all()
        if name == "inside":
            assert st["events"] > 0 and st["event_first_ray"] > 0 and st["box_parallel_in"] >= len(ijs) and int(out[2].sum()) == st["events"]
        else:
            assert st["event_first_ray"] == 0 and st["box_parallel_out"] >= len(ijs)


# ---- B.5 expectation -------------------------------------------------------------------------------------------------------------------------
SPP = 16384
SHARE = 0.05
# The light-only comparisons (glossy = 1, mis = 0 against ray_color; select = 1, §21's, and select = 0) are made per 2 x 2 block, where
# they are valid:
#   (a) on the twins without a narrow lobe (lit_fuzz.NARROW_TRIALS apart).  A light-only weight at a glossy event is pg / pl, and pg reaches
#       (3 + f^2) / (2 pi f^2): 5.0e5 at fuzz 2^-10, 191 at 0.05, 4.05 at 0.35.  The lobe of fuzz 2^-10 covers 3e-6 sr, so a light
#       sample falls into it a few times in a block's 65536 samples or not at all; then the block's mean misses the lobe's whole
#       contribution while its variance estimate and its largest share look harmless.  Measured on the first rule (narrow lobes on every
#       twin): trial 4, block (3, 2), share 0.017, z -17.5; trial 5, block (2, 3), share 0.006, z -20.5; the same blocks with glossy = 0:
#       |z| <= 1.8 and 3.2.  That this is the tail and no bias: the trial-5 block at 65536 / 524288 / 4194304 samples per pixel gave
#       1.61 +- 1.40, 1.17 +- 0.59, 2.74 +- 1.16 against the path's 0.2629 (MIS: 0.2626), single samples up to 1.2e7 carrying 41 to 100 %
#       of the sum of squares; the trial-4 block gave 0.157 +- 0.001 (z -39, share 0.008) at 65536 and 7.9 +- 7.7 at 524288.
#   (b) in the blocks where the largest single sample carries <= 5 % of the block's sum of squared luminances in both frames.
# A trial admits the comparison when (a) holds and at least half of its 16 blocks pass (b) — with fewer, "the image" is no longer the
# image; its image z is taken over the admitted blocks.  The condition: at least five of the eight trials admit §21's light-only
# comparison (select = 1).  With the table's pick (select = 0) the pmf ignores the distance, pl gets small next to a small emitter and
# fewer blocks pass (b): trials 1, 2, 4 and 5 admit it (trial 3 has 7 blocks within the share); it is compared where admitted.
LIGHT_ONLY_MIN_TRIALS = 5
LIGHT_ONLY_MIN_BLOCKS = 8


def _trace_moments(host, cam, first, tracer, **kw):
    """The 8 x 8 x SPP samples first … of an estimator through its trace → (moments (8, 8, 6) as frame(moments=True) gives them, the
    largest single sample's share of the sum of squared luminances per 2 x 2 block (4, 4))."""
    i, j, s = np.meshgrid(np.arange(8), np.arange(8), first + np.arange(SPP), indexing="ij")
    rad = tracer(host, cam, np.stack([i.ravel(), j.ravel(), s.ravel()], 1).astype(np.int32), **kw)[0].astype(np.float64).reshape(8, 8, SPP, 3)
    mom = np.concatenate([rad.sum(2), (rad * rad).sum(2)], -1).transpose(1, 0, 2)
    y2 = ((rad @ LUM) ** 2).transpose(1, 0, 2).reshape(4, 2, 4, 2, SPP)
    share = y2.max((1, 3, 4)) / np.maximum(y2.sum((1, 3, 4)), 1e-300)
    return mom, share


@functools.lru_cache(maxsize=None)
def light_only(trial, select=1):
    """(admitted, largest |z| over the admitted blocks, z of the admitted blocks together, blocks admitted, the largest shares of the
    two frames) of the light-only comparison on a twin."""
    c = lf.gloss_case(trial)
    cam = c.camera(8, 8, SPP, 6)
    plain, share_p = _trace_moments(c.host, cam, 0, gr.trace, glossy=0, emitters=False)
    light, share_l = _trace_moments(c.host, cam, (3 if select else 12) * SPP, gr.trace, glossy=1, select=select, nee_mis=0, planes=1)
    ok = (share_p <= SHARE) & (share_l <= SHARE)
    zb = np.abs(_zscores(_blocks(light), _blocks(plain), SPP * 4))
    n = int(ok.sum())
    z = float(zb[ok].max()) if n else 0.0
    za = float(_zscores(_blocks(light)[ok].sum(0), _blocks(plain)[ok].sum(0), SPP * 4 * n)) if n else 0.0
    admitted = trial not in lf.NARROW_TRIALS and n >= LIGHT_ONLY_MIN_BLOCKS
    print(f"{c.name} glossy select={select} mis=0 (light-only) / plain: {n} of 16 blocks within the share (largest share: path {share_p.max():.4f}, light-only "
          f"{share_l.max():.4f}); over them max |z| {z:.3f}, together z {za:.3f}; over all 16 max |z| {zb.max():.3f} → {'admitted' if admitted else 'not admitted'}")
    return admitted, z, za, n, float(share_p.max()), float(share_l.max())


@pytest.mark.parametrize("trial", lf.TRIALS)
def test_unbiased_on_the_twins(trial):
    """test_lit_fuzz.test_unbiased_against_the_path_alone's protocol and bounds on every twin: 8 x 8 pixels, depth 6, 16384 samples per
    estimator from disjoint ranges, 2 x 2 block |z| < 5 and image |z| < 4, every control held to the same bounds.  glossy = 1 at
    (select, mis) = (1, 1) and (0, 1) with planes against ray_color; under a map glossy_env = 1 (mode 1, lens, motion) against the path
    alone; under fuzz_medium(trial) the estimator with tree, planes and both switches against the path alone under the same medium;
    light-only (mis = 0) where it is valid (the comment above light_only)."""
    c = lf.gloss_case(trial)
    spp = SPP
    cam = c.camera(8, 8, spp, 6)
    worst = []

    def check(what, x, y):
        z, za = _compare(f"{c.name} {what}", x, y, spp)
        worst.append((what, z, za))

    plain = nr.frame(c.host, cam, nr.PLAIN, sample_first=0, moments=True)[1]
    check("control plain/plain", nr.frame(c.host, cam, nr.PLAIN, sample_first=4 * spp, moments=True)[1], plain)
    for k, (select, mis) in enumerate(((1, 1), (0, 1))):
        check(f"glossy select={select} mis={mis} / plain",
              gr.frame(c.host, cam, glossy=1, select=select, nee_mis=mis, planes=1, sample_first=(k + 1) * spp, moments=True)[1], plain)
    for select in (1, 0):
        admitted, z, za = light_only(trial, select)[:3]
        if admitted:
            worst.append((f"glossy select={select} light-only / plain", z, za))
    if c.env is not None:
        kw = dict(lens=c.lens, cam_close=c.close(8, 8, spp, 6), rgb=c.env)
        alone = gr.frame(c.host, cam, glossy=0, emitters=False, env_params=c.env_params(0), sample_first=5 * spp, moments=True, **kw)[1]
        check("control path/path under the map", gr.frame(c.host, cam, glossy=0, emitters=False, env_params=c.env_params(0), sample_first=8 * spp,
                                                          moments=True, **kw)[1], alone)
        check("glossy both switches select=1 mode=1 lens / path", gr.frame(c.host, cam, glossy=1, glossy_env=1, select=1, nee_mis=1, planes=1,
                                                                           env_params=c.env_params(1), sample_first=6 * spp, moments=True, **kw)[1], alone)
    m = lf.fuzz_medium(trial)
    kw = dict(rgb=c.env) if c.env is not None else {}
    ep = (lambda mode: c.env_params(mode)) if c.env is not None else (lambda mode: None)
    alone = mr.frame(c.host, cam, medium=m, emitters=False, env_params=ep(0), sample_first=9 * spp, moments=True, **kw)[1]
    check("control path/path under the medium", mr.frame(c.host, cam, medium=m, emitters=False, env_params=ep(0), sample_first=10 * spp, moments=True, **kw)[1], alone)
    check("medium: tree, planes, both switches / path", mr.frame(c.host, cam, medium=m, glossy=1, glossy_env=1 if c.env is not None else 0, select=1, planes=1,
                                                                 env_params=ep(1), sample_first=11 * spp, moments=True, **kw)[1], alone)
    for what, z, za in worst:
        assert z < 5.0 and abs(za) < 4.0, (c.name, what, z, za)


def test_light_only_is_admitted_often_enough():
    """The cap on exclusions: at least five of the eight twins admit the light-only comparison."""
    admitted = [t for t in lf.TRIALS if light_only(t, 1)[0]]
    print("light-only admitted on trials: select = 1", admitted, "select = 0", [t for t in lf.TRIALS if light_only(t, 0)[0]])
    assert len(admitted) >= LIGHT_ONLY_MIN_TRIALS, admitted


# ---- B.6 adaptive ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _adaptive_reference(call):
    c = lf.gloss_case(call.trial)
    w, h = lar.SIZE
    return lar.reference(c.host, c.camera(w, h, 1, 50), threshold=lar.THRESHOLD, tracer=gr.trace, **lar.SPP, **lf.gloss_reference_keywords(call, w, h, 1, 50))


@pytest.mark.parametrize("trial", lf.ADAPTIVE_TRIALS)
def test_adaptive_reference_uses_its_lists(trial):
    """The reference stops pixels at three or more different counts on every adaptive call of a twin — otherwise the list kernels never
    run; and the tracer keyword's default is the old behaviour."""
    c = lf.gloss_case(trial)
    for call in lf.gloss_adaptive_calls(trial):
        spp = _adaptive_reference(call)[1]
        print(c.name, f"lens={int(call.lens)} planes={call.planes} select={call.select} env={call.env} gn={call.gn} ge={call.ge}: counts", np.unique(spp).tolist())
        assert len(np.unique(spp)) >= 3, (call, np.unique(spp))
    w, h = lar.SIZE
    cam = c.camera(w, h, 1, 50)
    a = lar.radiances(c.host, cam, 2, select=1, planes=1)
    assert_same(a, lar.radiances(c.host, cam, 2, tracer=lf.tr.trace, select=1, planes=1), "tracer's default")
    assert_same(a, lar.radiances(c.host, cam, 2, tracer=gr.trace, glossy=0, select=1, planes=1), "gloss_reference with the switch off")


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------------------
def _initial_env_seeds(ijs, w):
    return np.array([rb_wang(rb_wang(rb_wang(int(i) * w + int(j)) + int(s)) ^ 0x454E5631) for i, j, s in ijs], np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_gloss_probes_equal_the_restatement(trial):
    """Every call of gloss_probe_calls on the twin: radiance, rays and every final seed equal gloss_reference.trace."""
    rb.amd_lib().rt_set_device(0)
    c = lf.gloss_case(trial)
    ijs = probe_set()
    w, h = PROBE_SIZE
    cam = c.camera(w, h, 1, 50)
    dev = rb.DeviceScene(c.host, device=0)
    env = rb.Env(c.env) if c.env is not None else None
    try:
        for call in lf.gloss_probe_calls(trial):
            want = _gloss_probe_reference(call, ijs)
            if call.entry == lf.NEE_PROBE:
                got = dev.trace_samples_nee(cam, ijs, params={"mis": call.mis, "sample_planes": call.planes, "select": call.select, "glossy": 1})
                refs, cols = want[:4], ("radiance", "rays", "seed", "nee seed")
            elif call.entry == lf.ENV_PROBE:
                got = dev.trace_samples_env(cam, env, ijs, params=dict(glossy=1, **c.env_params(call.env)))
                refs, cols = want[:3] + (want[4],), ("radiance", "rays", "seed", "env seed")
            else:
                got = dev.trace_samples_lit(cam, ijs, **lf.gloss_device_keywords(call, env, w, h, 1, 50))
                refs, cols = want[:5], ("radiance", "rays", "seed", "nee seed", "env seed")
            assert len(got) == len(refs)
            for g, x, col in zip(got, refs, cols):
                assert_same(g, x, f"{c.name} {call}: {col}")
    finally:
        if env is not None:
            env.close()
        dev.close()


def _run_gloss_frame(dev, c, call, depth, env):
    w, h, spp = FRAME
    cam = c.camera(w, h, spp, depth)
    shard, first = lf.SHARDS[call.shard]
    if call.entry == lf.NEE_FRAME:
        got = dev.render_nee_to_host(cam, params={"mis": call.mis, "sample_planes": call.planes, "select": call.select, "glossy": 1}, shard=shard, sample_first=first)[0]
        return got, gr.frame(c.host, cam, glossy=1, select=call.select, nee_mis=call.mis, planes=call.planes, shard=shard, sample_first=first)
    if call.entry == lf.ENV_FRAME:
        p = c.env_params(call.env)
        got = dev.render_env_to_host(cam, env, params=dict(glossy=1, **p), shard=shard, sample_first=first)[0]
        return got, gr.frame(c.host, cam, glossy=0, glossy_env=1, emitters=False, rgb=c.env, env_params=p, shard=shard, sample_first=first)
    kw = lf.gloss_device_keywords(call, env, w, h, spp, depth)
    rkw = lf.gloss_reference_keywords(call, w, h, spp, depth)
    if call.medium:
        return dev.render_medium_to_host(cam, shard=shard, sample_first=first, **kw)[0], mr.frame(c.host, cam, shard=shard, sample_first=first, **rkw)
    return dev.render_lit_to_host(cam, shard=shard, sample_first=first, **kw)[0], gr.frame(c.host, cam, shard=shard, sample_first=first, **rkw)


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", ["default", "exact"])
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_gloss_frames_equal_the_restatement(trial, traversal):
    """Every call of gloss_frame_calls on the twin, depths 2 and 50, each with its shard or sample_first = 37.  Among them, over the
    trials, is lit_gloss_render_kernel<true, TreeTable> — the pair held to 3 waves per SIMD — on a twin without planes or with
    sample_planes = 0 (asserted)."""
    rb.amd_lib().rt_set_device(0)
    assert _target_frame_calls()
    c = lf.gloss_case(trial)
    dev = rb.DeviceScene(c.host, device=0, **({} if traversal == "default" else {"traversal": rb.TRAVERSAL_EXACT}))
    env = rb.Env(c.env) if c.env is not None else None
    try:
        for call in lf.gloss_frame_calls(trial):
            for depth in (2, 50):
                got, want = _run_gloss_frame(dev, c, call, depth, env)
                assert_same(got, want, f"{c.name} {traversal} depth={depth} {call}")
    finally:
        if env is not None:
            env.close()
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.ADAPTIVE_TRIALS)
def test_gloss_adaptive_frames_equal_the_reference(trial):
    """rt_render_lit_adaptive with the switches on a twin: fb, spp and moments equal the reference built on gloss_reference.trace — the
    eight lit_gloss_list_render_kernels against a restatement."""
    rb.amd_lib().rt_set_device(0)
    c = lf.gloss_case(trial)
    w, h = lar.SIZE
    dev = rb.DeviceScene(c.host, device=0)
    env = rb.Env(c.env)
    try:
        for call in lf.gloss_adaptive_calls(trial):
            fb, spp, mom, _ = dev.render_lit_adaptive_to_host(c.camera(w, h, 1, 50), threshold=lar.THRESHOLD, **lar.SPP,
                                                              **lf.gloss_device_keywords(call, env, w, h, 1, 50))
            want = _adaptive_reference(call)
            assert len(np.unique(want[1])) >= 3, (call, np.unique(want[1]))
            for g, x, col in zip((fb, spp, mom), want, ("fb", "spp", "moments")):
                assert_same(g, x, f"{c.name} {call}: {col}")
    finally:
        env.close()
        dev.close()


def _compare_medium_probe(got, want, what):
    rad, rays, events, seeds, ns, es, ms = got
    assert_same(rad, want[0], what + ": radiance")
    assert_same(rays, want[1], what + ": rays")
    assert_same(events, want[2], what + ": medium events")
    for k, col in enumerate((seeds, ns, es, ms)):
        assert_same(col, want[4][:, k], what + f": final seed {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_medium_probes_equal_the_restatement(trial):
    """The twin under fuzz_medium(trial) through every (kLens, Table): radiance, rays, events and the four seeds equal
    medium_reference.trace; where the medium fills all space under a map the environment's stream is never drawn from."""
    rb.amd_lib().rt_set_device(0)
    c = lf.gloss_case(trial)
    ijs = probe_set()
    w, h = PROBE_SIZE
    cam = c.camera(w, h, 1, 50)
    dev = rb.DeviceScene(c.host, device=0)
    env = rb.Env(c.env) if c.env is not None else None
    all_space = lf.medium_extent(lf.fuzz_medium(trial)) is None
    try:
        for call in lf.medium_probe_calls(trial):
            want = _medium_probe_reference(call, ijs)
            got = dev.trace_samples_medium(cam, ijs, **lf.gloss_device_keywords(call, env, w, h, 1, 50))
            _compare_medium_probe(got, want, f"{c.name} {call}")
            if all_space and call.env is not None:
                assert_same(got[5], _initial_env_seeds(ijs, w), f"{c.name} {call}: the env stream as initialised")
            assert int(want[2].sum()) > 0
    finally:
        if env is not None:
            env.close()
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_medium_frames_equal_the_restatement(trial):
    """Every medium render kernel on the twin under fuzz_medium(trial), each call with its shard turn."""
    rb.amd_lib().rt_set_device(0)
    c = lf.gloss_case(trial)
    dev = rb.DeviceScene(c.host, device=0)
    env = rb.Env(c.env) if c.env is not None else None
    try:
        for call in lf.medium_frame_calls(trial):
            got, want = _run_gloss_frame(dev, c, call, 50, env)
            assert_same(got, want, f"{c.name} {call}")
    finally:
        if env is not None:
            env.close()
        dev.close()


@pytest.mark.gpu
def test_fan_camera_and_camera_inside_a_ball_on_the_device():
    """The box's parallel branch on the camera ray (the three boxes of test_fan_camera), a camera inside a ball (albedo 0: every event
    ends the path; and a scattering one), and the probes whose free-flight draw is exactly 0: probes and one frame each."""
    rb.amd_lib().rt_set_device(0)
    host = lf.gloss_case(FAN_TRIAL).host
    dev = rb.DeviceScene(host, device=0)
    ijs = all_ijs(16, 16, 8)
    nee = dict(select=1, sample_planes=1, glossy=1)
    rkw = dict(select=1, planes=1, glossy=1)
    for name in FAN_BOXES:
        m = fan_medium(name)
        _compare_medium_probe(dev.trace_samples_medium(fan_camera(), ijs, medium=m, nee=nee), mr.trace(host, fan_camera(), ijs, medium=m, **rkw), f"fan camera, box {name}")
    cam = fan_camera(16, 16, 3)
    assert_same(dev.render_medium_to_host(cam, medium=fan_medium("inside"), nee=nee)[0], mr.frame(host, cam, medium=fan_medium("inside"), **rkw), "fan camera frame")
    dev.close()
    w, h = PROBE_SIZE
    for albedo in (0.0, (0.9, 0.8, 0.7)):
        c, m = ball_camera_case(albedo)
        dev = rb.DeviceScene(c.host, device=0)
        probes = np.concatenate([probe_set()[:1000], u_zero_probes(w, h)])
        with rb.Env(c.env) as env:
            kw = dict(nee=nee, lens=c.lens_dict(), env=env, env_params=dict(glossy=1, **c.env_params(1)))
            rk = dict(lens=c.lens, rgb=c.env, env_params=c.env_params(1), glossy_env=1, **rkw)
            pcam = c.camera(w, h, 1, 50)
            _compare_medium_probe(dev.trace_samples_medium(pcam, probes, medium=m, **kw), mr.trace(c.host, pcam, probes, medium=m, **rk), f"camera inside a ball, albedo {albedo}")
            cam = c.camera(*FRAME, 50)
            assert_same(dev.render_medium_to_host(cam, medium=m, **kw)[0], mr.frame(c.host, cam, medium=m, **rk), f"camera inside a ball, albedo {albedo}: frame")
        dev.close()
