"""rt_render_chroma / rt_trace_samples_chroma (include/rtp_amd.h, "chromatic extinction"): fog whose extinction differs
per colour channel.  The contract's restatement is tests/cpu_native/chroma_ref.c (tests/chroma_reference.py); the CPU tests check the
restatement and the ABI, the GPU tests the kernels against the restatement, bit for bit.  Scenes, settings and protocols are
tests/test_medium.py's and tests/test_volume.py's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import chroma_reference as cr
import medium_reference as mr
import rtp_bindings as rb
import volume_reference as vr
from test_lit import assert_same
from test_medium import (ABSORB_N, BACKGROUND, EQUAL_SPP, FOG_BOX, PROBE_VIEW, SETTINGS, _channel_z, _fog_ball_scene, all_ijs, dev_kw, media, ref_kw,
                         scenes, sun_map)
from test_volume import BOX, GRIDS, IDENTITY_VIEW, _compare_probe, fog, random_grid, special_camera

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
INVALID = 1
TINTS = ((0.25, 1.0, 4.0), (0.0, 1.0, 3.0), (2.0, 2.0, 0.5))


def scaled(medium, e):
    """The medium with sigma_t replaced by the float32 product sigma_t * e."""
    return dict(medium, sigma_t=float(np.float32(medium["sigma_t"]) * np.float32(e)))


# ---- no GPU needed ---------------------------------------------------------------------------------------------------------------------

def test_abi_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_chroma_params_init", "rt_render_chroma", "rt_trace_samples_chroma"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert len(lib.rt_render_chroma.argtypes) == 12 and len(lib.rt_trace_samples_chroma.argtypes) == 16
    for name in ("render_chroma", "render_chroma_to_host", "trace_samples_chroma"):
        assert hasattr(rb.DeviceScene, name)
    assert C.sizeof(rb.ChromaParams) == 16 and C.sizeof(rb.MediumParams) == 52
    p = rb.chroma_params()
    assert p.struct_bytes == 16 and list(p.tint) == [1.0, 1.0, 1.0]
    assert list(rb.chroma_params(tint=(0.5, 1, 2)).tint) == [0.5, 1.0, 2.0] and list(rb.chroma_params(tint=3).tint) == [3.0] * 3
    lib.rt_chroma_params_init(None)
    lib.rt_version_string.restype = C.c_char_p
    assert lib.rt_version_string()


def _calls(cam, lit, medium, volume, chroma):
    """(status, message) of rt_render_chroma and of rt_trace_samples_chroma with a null scene."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    pl = C.byref(lit) if lit is not None else None
    pm = C.byref(medium) if medium is not None else None
    pc = C.byref(chroma) if chroma is not None else None
    out = [lib.rt_render_chroma(None, C.byref(cam), pl, pm, volume, pc, None, 0, C.c_void_p(1 << 32), None, 1, None), lib.rt_get_last_error_string().decode()]
    out += [lib.rt_trace_samples_chroma(None, C.byref(cam), pl, pm, volume, pc, 1, ijs, f, r, r, s, s, s, s, r), lib.rt_get_last_error_string().decode()]
    return out


def test_refusals_before_the_scene_is_looked_at():
    """rt_render_volume's refusals in its order, then the tint's, all with a null scene — nothing can have been enqueued, and the volume's
    handle is never read (it is not one).  What passes reaches the null-scene check.  Every message names the chroma call."""
    cam = rb.rtiow_camera(8, 4, 2)
    handle = C.c_void_p(1 << 32)
    nan, inf = float("nan"), float("inf")
    box = dict(box=(0, 0, 0, 1, 1, 1))
    good = rb.medium_params(sigma_t=1.0, **box)

    def refused(word, medium=good, lit=None, volume=handle, chroma=None):
        st1, m1, st2, m2 = _calls(cam, lit, medium, volume, chroma)
        assert st1 == INVALID and word in m1 and "rt_render_chroma" in m1, (word, m1)
        assert st2 == INVALID and word in m2 and "rt_trace_samples_chroma" in m2, (word, m2)
    bad_tint = rb.chroma_params(tint=(1, -1, 1))
    for volume in (handle, None):
        short = rb.medium_params(sigma_t=1.0, **box)
        short.struct_bytes = 4
        refused("rt_medium_params", short, volume=volume)
        for s in (-0.5, nan, inf):
            refused("sigma_t", rb.medium_params(sigma_t=s, **box), volume=volume, chroma=bad_tint)
        refused("albedo", rb.medium_params(sigma_t=1.0, albedo=(0.5, 1.5, 0.5), **box), volume=volume, chroma=bad_tint)
        refused("|g|", rb.medium_params(sigma_t=1.0, g=0.96, **box), volume=volume, chroma=bad_tint)
        refused("lo < hi", rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, -1, 1)), volume=volume, chroma=bad_tint)
        # rt_render_lit's come first, the medium's before the volume's, the volume's before the tint's
        refused("mis", rb.medium_params(sigma_t=-1.0), lit=rb.lit_params(nee=dict(mis=2)), volume=volume, chroma=bad_tint)
        # the tint's own
        short = rb.chroma_params()
        short.struct_bytes = 4
        refused("rt_chroma_params", volume=volume, chroma=short)
        for t in ((-0.5, 1, 1), (1, nan, 1), (1, 1, inf), (-0.0 - 1e-30, 1, 1)):
            refused("tint", volume=volume, chroma=rb.chroma_params(tint=t))
        refused("not finite", rb.medium_params(sigma_t=3e38, **box), volume=volume, chroma=rb.chroma_params(tint=(1, 1, 2)))
        refused("not finite", rb.medium_params(sigma_t=3e38, **box), volume=volume, chroma=rb.chroma_params(tint=2))
    refused("region 2", None, chroma=bad_tint)
    refused("region 2", rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), chroma=bad_tint)
    # what passes reaches the scene
    for m, volume, chroma in ((good, handle, rb.chroma_params(tint=(0.25, 1, 4))), (good, handle, None), (None, None, rb.chroma_params(tint=(0, 1, 3))),
                              (rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), None, rb.chroma_params(tint=0)), (good, None, rb.chroma_params(tint=(0, 0, 1)))):
        st1, m1, st2, m2 = _calls(cam, None, m, volume, chroma)
        assert st1 == INVALID and "rt_render_chroma: null scene" in m1, m1
        assert st2 == INVALID and "tint" not in m2 and "sigma_t" not in m2 and "region" not in m2, m2


def test_cli_refusals(test_config_text, tmp_path):
    fog_args = ["--lit", "--fog", "0.5"]
    cases = [(["--lit", "--fog-tint", "0.5,1,2"], "needs --lit --fog"),
             (fog_args + ["--fog-tint", "0.5,1,2", "--fog-noise-target", "0.1"], "--fog-noise-target"),
             (fog_args + ["--fog-tint", "0.5,1,2", "--fog-denoise"], "--fog-denoise"),
             (fog_args + ["--fog-tint", "0.5,1"], "R,G,B"), (fog_args + ["--fog-tint", "0.5,-1,2"], "R,G,B"), (fog_args + ["--fog-tint", "0.5,1,2,3"], "R,G,B"),
             (fog_args + ["--fog-tint", "0.5,nan,2"], "R,G,B"), (fog_args + ["--fog-tint"], "R,G,B")]
    for extra, word in cases:
        res = subprocess.run([EXE, "--gpu"] + extra, input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert res.returncode == 99 and word in res.stderr and "--fog-tint" in res.stderr, (extra, res.returncode, res.stderr[-300:])


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_equal_tints_are_the_grey_restatement(scene):
    """Equal tints e hand the call over: every probe column and a whole frame equal volume_reference / medium_reference at the float
    product sigma_t * e, bit for bit — regions 0 / 1 / 2 without a grid and the box with one; tint None is e = 1."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    ijs = all_ijs(w, h, spp)
    cases = [(m, None) for m in media(scene).values()] + [(fog(0.3), GRIDS["2x3x5"])]
    for k, (medium, density) in enumerate(cases):
        setting = list(SETTINGS)[k % len(SETTINGS)]
        cam = camera(w, h, spp, 12)
        kw = ref_kw(scene, setting, w, h, spp, 12)
        for e in (0.0, 0.5, 1.0, 3.0, None):
            grey = scaled(medium, 1.0 if e is None else e)
            if density is None:
                want = mr.trace(host, cam, ijs, medium=grey, **kw) + (np.zeros(len(ijs), np.int32),)
                want_frame = mr.frame(host, cam, medium=grey, **kw)
            else:
                want = vr.trace(host, cam, ijs, medium=grey, density=density, **kw)
                want_frame = vr.frame(host, cam, medium=grey, density=density, **kw)
            got = cr.trace(host, cam, ijs, medium=medium, density=density, tint=e, **kw)
            for a, b, col in zip(got, want, ("radiance", "rays", "events", "ends", "seeds", "cells")):
                assert_same(a, b, f"{scene} / {setting} / case {k} / e {e}: {col}")
            assert_same(cr.frame(host, cam, medium=medium, density=density, tint=e, **kw), want_frame, f"{scene} / {setting} / case {k} / e {e}: frame")
            if e == 0.0:
                assert not got[2].any()


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_one_cell_of_density_one_is_the_homogeneous_box(scene):
    """A 1 x 1 x 1 grid of density 1.0 equals the homogeneous box under the same tint, in every column but cells and in whole frames, in
    every setting of tests/test_medium.py."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    ijs = all_ijs(w, h, spp)
    one = np.ones((1, 1, 1), np.float32)
    seen_events = seen_cells = 0
    for k, setting in enumerate(SETTINGS):
        medium = dict(sigma_t=0.25, albedo=(0.9, 0.85, 0.8), g=(-0.5, 0.0, 0.7)[k % 3], box=BOX)
        tint = TINTS[k % 3]
        cam = camera(w, h, spp, 12)
        kw = ref_kw(scene, setting, w, h, spp, 12)
        want = cr.trace(host, cam, ijs, medium=medium, tint=tint, **kw)
        got = cr.trace(host, cam, ijs, medium=medium, density=one, tint=tint, **kw)
        for a, b, col in zip(got[:5], want, ("radiance", "rays", "events", "ends", "seeds")):
            assert_same(a, b, f"{scene} / {setting}: {col}")
        assert not want[5].any()
        seen_events += int(got[2].sum())
        seen_cells += int(got[5].sum())
        assert_same(cr.frame(host, cam, medium=medium, density=one, tint=tint, **kw), cr.frame(host, cam, medium=medium, tint=tint, **kw), f"{scene} / {setting}: frame")
    assert seen_events > 100 and seen_cells > seen_events


def test_weights_are_bounded():
    """10^5 random (u, uc, A, tint), a zero channel, two equal channels and ratios up to 64 among the tints: every factor on beta is finite
    and lies in [0, 3], den > 0, and the sampled channel's Tr is positive.  (The bound itself: each term of den is a numerator over 3.)"""
    n = 100000
    rng = np.random.default_rng(7)
    u = rng.random(n).astype(np.float32)
    u[u == 0] = np.float32(2.0 ** -24)          # (u == 0 never reaches the weights: no event, nothing drawn)
    u[:64] = np.float32(2.0 ** -24)             # the smallest draw there is
    uc = rng.random(n).astype(np.float32)
    uc[64:128] = np.float32(1.0 - 2.0 ** -24)   # (uc * 3.0f rounds to 3.0f: the min with 2)
    A = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), n)).astype(np.float32)
    A[128:192] = np.inf                         # region 0, a miss
    A[192:256] = np.float32(1e-30)
    tint = np.exp2(rng.uniform(-3, 3, (n, 3))).astype(np.float32)          # ratios up to 64
    for c in range(3):                                                     # a zero channel (or two, or all three: no fog at all)
        tint[rng.random(n) < 0.1, c] = 0.0
    eq = rng.random(n) < 0.25                                              # two equal channels
    tint[eq, 1] = tint[eq, 0]
    tint[:8] = (1.0, 64.0, 0.0)
    sigma = tint * rng.choice(np.array([0.05, 1.0, 20.0], np.float32), (n, 1))
    out = cr.weights(u, uc, A, sigma)
    w, den = out["w"], out["den"]
    print(f"events {int(out['event'].sum())} of {n}; weights in [{w.min()}, {w.max()}]; smallest den {den.min():.3e}; smallest Tr_j {out['trj'].min():.3e}")
    assert np.isfinite(w).all() and (w >= 0).all() and (w <= 3).all()
    assert np.isfinite(den).all() and (den > 0).all() and (out["trj"] > 0).all()
    assert 0.2 * n < out["event"].sum() < 0.8 * n
    # a channel without extinction never scatters: its weight at an event is exactly 0, and without one 3 / den >= 1
    zero = sigma == 0
    ev = out["event"] == 1
    assert (w[zero & ev[:, None]] == 0).all() and (w[zero & ~ev[:, None]] >= 1).all()
    # the three weights of a draw average to 1 where the channels are equal (a grey medium has weight 1)
    same = np.repeat(sigma[:1000, :1], 3, axis=1)
    assert (cr.weights(u[:1000], uc[:1000], A[:1000], same)["w"] == np.float32(1.0)).all()


TINT_SLAB = (0.25, 1.0, 4.0)


def test_beer_lambert_per_channel():
    """albedo = 0, a slab (a box of thickness 2 across x) in front of a constant background, tint (0.25, 1, 4), no emitters, pinhole: per
    channel the mean over ABSORB_N samples lies within |z| <= 4.5 of background_k * exp(-sigma_k L), L in float64 from the pixel-centre ray,
    with the channel's own sample variance (a sample of channel k is no longer 0 or the background: it carries the weight 3 Tr_k / den).
    Pixels: those whose rays enter by the face x = -1 and leave by x = 1 at the centre and the four corners, and whose length varies by
    < 1 % over the corners (tests/test_volume.py's two-slab protocol)."""
    host = _fog_ball_scene()
    w = h = 9
    cam = rb.make_camera(w, h, 8.0, (-9, 0.4, 0.3), (0, 0, 0), BACKGROUND, ABSORB_N, 8)
    sigma = 0.45
    medium = dict(sigma_t=sigma, albedo=0.0, box=(-1, -1, -1, 1, 1, 1))
    o = np.array([cam.origin.e[k] for k in range(3)], np.float64)
    p00 = np.array([cam.pixel00_loc.e[k] for k in range(3)], np.float64)
    du = np.array([cam.pixel_delta_u.e[k] for k in range(3)], np.float64)
    dv = np.array([cam.pixel_delta_v.e[k] for k in range(3)], np.float64)

    def length(i, j):
        dd = p00 + i * du + j * dv - o
        dd /= np.linalg.norm(dd)
        t = [(x - o[0]) / dd[0] for x in (-1.0, 1.0)]
        for tt in t:
            p = o + tt * dd
            if not (abs(p[1]) < 1.0 and abs(p[2]) < 1.0):
                return None
        return t[1] - t[0]
    fb, mom = cr.frame(host, cam, medium=medium, tint=TINT_SLAB, emitters=False, moments=True)
    checked = 0
    for j in range(h):
        for i in range(w):
            ll = length(i, j)
            corners = [length(i + a, j + b) for a in (-0.5, 0.5) for b in (-0.5, 0.5)]
            if ll is None or None in corners or (max(corners) - min(corners)) > 0.01 * ll:
                continue
            checked += 1
            for k in range(3):
                want = BACKGROUND[k] * np.exp(-sigma * TINT_SLAB[k] * ll)
                mean = mom[j, i, k] / ABSORB_N
                var = max(mom[j, i, 3 + k] / ABSORB_N - mean * mean, 0.0) * (ABSORB_N / (ABSORB_N - 1.0)) / ABSORB_N
                z = (mean - want) / np.sqrt(var)
                print(f"pixel ({i}, {j}) channel {k} length {ll:.4f} mean {mean:.5f} want {want:.5f} z {z:+.2f}")
                assert abs(z) <= 4.5, (i, j, k, z)
    assert checked >= 9


EQUIV_MEDIA = {
    "ball": (dict(sigma_t=0.3, albedo=(0.9, 0.9, 0.9), ball=(0.0, 1.0, 0.0, 3.0)), None, (0, 2, 7)),
    "box, camera inside": (dict(FOG_BOX, sigma_t=0.2), None, (0, 2, 3)),
    "all space": (dict(sigma_t=0.1, albedo=(0.9, 0.9, 0.9)), None, (0, 2, 7)),
    "grid": (dict(FOG_BOX, sigma_t=0.25), "random 8^3", (0, 2, 7)),
}
EQUIV_SETTINGS = (("mis", dict(nee_mis=1)), ("light", dict(nee_mis=0)), ("off", dict(emitters=False)), ("select", dict(nee_mis=1, select=1)))


@pytest.mark.parametrize("tint", [(0.25, 1.0, 4.0), (0.0, 1.0, 3.0)])
@pytest.mark.parametrize("where", list(EQUIV_MEDIA))
def test_channel_equals_the_grey_medium_of_its_extinction(tint, where):
    """The test that pins the estimator: channel k of the chroma restatement against channel k of the GREY restatement at sigma_t * tint[k],
    per pixel and channel, |z| <= 4.5 with each frame's own sample variance at EQUAL_SPP — tests/test_medium.py's and tests/test_volume.py's
    equal-expectation protocol and bound.  Settings mis / light-only / off / select, each with g = 0 and g = 0.7."""
    host, _, _ = scenes()["three balls"]
    medium, density, eye = EQUIV_MEDIA[where]
    if density is not None:
        density = random_grid((8, 8, 8), 31)
        assert abs((density == 0).mean() - 1 / 3) < 0.06
    cam = rb.make_camera(4, 4, 40.0, eye, (0, 1, 0), (0.05, 0.05, 0.05), EQUAL_SPP, 6)
    worst = 0.0
    for name, kw in EQUIV_SETTINGS:
        for g in (0.0, 0.7):
            m = dict(medium, g=g)
            a = cr.frame(host, cam, medium=m, density=density, tint=tint, moments=True, **kw)[1]
            assert a[..., :3].sum() > 0
            for k in range(3):
                b = vr.frame(host, cam, medium=scaled(m, tint[k]), density=density, moments=True, **kw)[1]
                z = _channel_z(a, b, EQUAL_SPP)[..., k]
                worst = max(worst, float(np.abs(z).max()))
                print(f"{where} / tint {tint} / {name} / g {g} / channel {k}: max |z| {float(np.abs(z).max()):.2f}")
                assert np.abs(z).max() <= 4.5, (where, tint, name, g, k, z)
    print("worst |z|", worst)


@pytest.mark.parametrize("g", [0.0, 0.7])
def test_white_furnace(g):
    """albedo = 1 under a tint, in a fog ball of optical diameter 2 (at tint 1) under background 1, max_depth = 200.  A path that ends by a
    miss is NO LONGER exactly 1.0f: it carries the product of its flights' channel weights, each in [0, 3] with mean 1.  What holds is the
    mean: per channel 1 within |z| <= 4.5 of the samples' own standard error, and at most 0.1 % of the samples are cut by depth."""
    host = _fog_ball_scene()
    cam = rb.make_camera(16, 16, 20.0, (0, 1, 8), (0, 0, 0), (1.0, 1.0, 1.0), 16, 200)
    ijs = all_ijs(16, 16, 16)
    rad, rays, events, ends, seeds, cells = cr.trace(host, cam, ijs, medium=dict(sigma_t=1.0, albedo=1.0, g=g, ball=(0, 0, 0, 1.0)), tint=(0.25, 1.0, 4.0),
                                                     emitters=False)
    missed = ends == mr.END_MISS
    assert (~missed).mean() <= 0.001, (~missed).mean()
    assert events.max() >= 3 and (events > 0).mean() > 0.1
    x = rad.astype(np.float64)
    assert (x != 1.0).any() and (x >= 0).all()
    z = (x.mean(0) - 1.0) / (x.std(0, ddof=1) / np.sqrt(len(x)))
    print("mean", x.mean(0), "z", z)
    assert (np.abs(z) <= 4.5).all(), z


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------

def _probe_cases(scene):
    """(medium name or grid, tint, setting, g, depth, camera): every setting on every scene — the regions 0 / 1 / 2 without a grid and the
    four grids in turn, the three tints, g in {0, +-0.95} and the depths {1, 2, 12} spread over them — then the special cameras."""
    si = ["three balls", "night rtiow", "fuzz planes"].index(scene)
    where = ["all space", "ball", "box"] + list(GRIDS)
    out = []
    for k, setting in enumerate(SETTINGS):
        out.append((where[(k + 2 * si) % 7], TINTS[(k + si) % 3], setting, (0.0, 0.95, -0.95)[(k + si) % 3], (12, 2, 1)[(k + si) % 3] if k % 2 else 12, "scene"))
    out += [("16", TINTS[si], "mis", 0.0, 12, "inside"), ("box", TINTS[(si + 1) % 3], "glossy", 0.95, 12, "inside"),
            ("16", TINTS[(si + 2) % 3], "glossy", 0.95, 12, "fan"), ("1x1x64", TINTS[si], "mis", 0.0, 12, "fan"), ("box", TINTS[(si + 1) % 3], "select", -0.95, 2, "fan")]
    return out


def _medium_of(where, g):
    """(medium, density) of a probe case."""
    if where == "all space":
        return dict(sigma_t=0.08, albedo=(0.9, 0.85, 0.8), g=g), None
    if where == "ball":
        return dict(sigma_t=0.35, albedo=(0.95, 0.9, 0.8), g=g, ball=(0.0, 1.0, 0.0, 3.0)), None
    return fog(g), (None if where == "box" else GRIDS[where])


def _camera(scene, kind, w, h, spp, depth):
    return scenes()[scene][1](w, h, spp, depth) if kind == "scene" else special_camera(kind, w, h, spp, depth)


def test_probe_cases_cover_the_issue():
    """(no GPU) the probe cases hold every region, grid, tint, g, depth and setting on every scene."""
    for scene in ("three balls", "night rtiow", "fuzz planes"):
        cases = _probe_cases(scene)
        assert {c[2] for c in cases} == set(SETTINGS) and {c[1] for c in cases} == set(TINTS)
        assert {c[3] for c in cases} == {0.0, 0.95, -0.95} and {c[4] for c in cases} == {1, 2, 12} and {c[5] for c in cases} == {"scene", "inside", "fan"}
    assert {c[0] for s in ("three balls", "night rtiow", "fuzz planes") for c in _probe_cases(s)} == {"all space", "ball", "box"} | set(GRIDS)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow", "fuzz planes"])
def test_probe_samples_equal_the_restatement(scene):
    host = scenes()[scene][0]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    seen_events = seen_cells = 0
    volumes = {name: rb.Volume(g) for name, g in GRIDS.items()}
    with rb.Env(sun_map()) as env:
        for where, tint, setting, g, depth, kind in _probe_cases(scene):
            medium, density = _medium_of(where, g)
            cam = _camera(scene, kind, w, h, spp, depth)
            want = cr.trace(host, cam, ijs, medium=medium, density=density, tint=tint, **ref_kw(scene, setting, w, h, spp, depth))
            got = dev.trace_samples_chroma(cam, ijs, medium=medium, volume=volumes.get(where), tint=tint, **dev_kw(scene, setting, env, w, h, spp, depth))
            _compare_probe(got, want, f"{scene} / {where} / tint {tint} / {setting} / g {g} / depth {depth} / camera {kind}")
            seen_events += int(want[2].sum())
            seen_cells += int(want[5].sum())
    assert seen_events > 100 and seen_cells > 1000          # (the cases did scatter, and those with a grid did walk it; the others count no cell)
    for v in volumes.values():
        v.close()
    dev.close()


@pytest.mark.gpu
def test_frames_equal_the_restatement():
    """40 x 27 x 3 spp, 7 x 5 x 1, a 3-row shard of the first, sample_first = 5, sync = 0 on a torch stream, and one small frame through
    each of the sixteen instantiations of chroma_render_kernel: pinhole / lens x the four emitter tables x no grid / grid."""
    import torch
    scene, setting = "three balls", "glossy"
    host, camera, _ = scenes()[scene]
    medium, density, tint = fog(0.7), GRIDS["2x3x5"], TINTS[0]
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env, rb.Volume(density) as vol, rb.Volume(GRIDS["16"]) as vol16:
        for (w, h, spp), more in (((40, 27, 3), {}), ((7, 5, 1), {}), ((40, 27, 3), dict(shard=rb.Shard(3, 1, 4))), ((40, 27, 3), dict(sample_first=5))):
            cam = camera(w, h, spp, 12)
            want = cr.frame(host, cam, medium=medium, density=density, tint=tint, **more, **ref_kw(scene, setting, w, h, spp, 12))
            got, _ = dev.render_chroma_to_host(cam, medium=medium, volume=vol, tint=tint, **more, **dev_kw(scene, setting, env, w, h, spp, 12))
            assert_same(got, want, f"frame {w}x{h}x{spp} {more}")
        # lens + motion with the light tree over the two-kind table, on a stream, without waiting inside the call
        scene2 = "fuzz planes"
        host2, camera2, _ = scenes()[scene2]
        dev2 = rb.DeviceScene(host2, device=0)
        w, h, spp = 40, 27, 3
        cam = camera2(w, h, spp, 12)
        kw_r = {**ref_kw(scene2, "lens + motion", w, h, spp, 12), "select": 1, "planes": 1}
        kw_d = dev_kw(scene2, "lens + motion", env, w, h, spp, 12)
        kw_d["nee"] = dict(select=1, sample_planes=1)
        want = cr.frame(host2, cam, medium=fog(-0.5), density=GRIDS["16"], tint=TINTS[1], **kw_r)
        stream = torch.cuda.Stream()
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        with torch.cuda.stream(stream):
            dev2.render_chroma(cam, fb.data_ptr(), medium=fog(-0.5), volume=vol16, tint=TINTS[1], stream=stream.cuda_stream, sync=False, **kw_d)
        stream.synchronize()
        assert_same(fb.cpu().numpy(), want, "sync = 0 on a torch stream")
        # the sixteen instantiations, each on a small frame
        w, h, spp = 24, 13, 2
        k = 0
        for grid in (None, "2x3x5"):
            for lens in (False, True):
                for select, planes in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    setting = "lens + motion" if lens else "mis"
                    cam = camera2(w, h, spp, 12)
                    kw_r = {**ref_kw(scene2, setting, w, h, spp, 12), "select": select, "planes": planes}
                    kw_d = dev_kw(scene2, setting, env, w, h, spp, 12)
                    kw_d["nee"] = dict(select=select, sample_planes=planes)
                    want = cr.frame(host2, cam, medium=fog(0.3), density=None if grid is None else GRIDS[grid], tint=TINTS[k % 3], **kw_r)
                    got, _ = dev2.render_chroma_to_host(cam, medium=fog(0.3), volume=None if grid is None else vol, tint=TINTS[k % 3], **kw_d)
                    assert_same(got, want, f"frame grid={grid} lens={lens} select={select} planes={planes}")
                    k += 1
        dev2.close()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_device_identities(scene):
    """Equal tints e are rt_render_volume at sigma_t * e — frames and probes, through the grey kernels (tint None, e = 0 included); a 1^3
    grid of density 1 is the homogeneous box under the same tint, each through its own chroma kernels; volume == NULL runs in any region."""
    host, camera, _ = scenes()[scene]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env, rb.Volume(np.ones((1, 1, 1), np.float32)) as one, rb.Volume(GRIDS["2x3x5"]) as vol:
        for k, setting in enumerate(SETTINGS):
            kw = dev_kw(scene, setting, env, w, h, spp, 12)
            cam = camera(w, h, spp, 12)
            medium = fog((0.0, 0.7, -0.95)[k % 3])
            what = f"{scene} / {setting}"
            # the handover
            e = (None, 0.0, 0.5, 3.0)[k % 4]
            grey = scaled(medium, 1.0 if e is None else e)
            volume = vol if k % 2 else None
            for a, b in zip(dev.trace_samples_chroma(cam, ijs, medium=medium, volume=volume, tint=e, **kw), dev.trace_samples_volume(cam, ijs, medium=grey, volume=volume, **kw)):
                assert_same(a, b, f"{what}: equal tints {e}")
            assert_same(dev.render_chroma_to_host(cam, medium=medium, volume=volume, tint=e, **kw)[0], dev.render_volume_to_host(cam, medium=grey, volume=volume, **kw)[0],
                        f"{what}: equal tints {e}, frame")
            # the 1^3 grid
            tint = TINTS[k % 3]
            hom = dev.trace_samples_chroma(cam, ijs, medium=medium, tint=tint, **kw)
            got = dev.trace_samples_chroma(cam, ijs, medium=medium, volume=one, tint=tint, **kw)
            for a, b, col in zip(got[:7], hom[:7], ("radiance", "rays", "events", "seed", "nee seed", "env seed", "med seed")):
                assert_same(a, b, f"{what}: 1^3 grid, {col}")
            assert got[7].sum() > 0 and not hom[7].any() and hom[2].sum() > 0
            assert_same(dev.render_chroma_to_host(cam, medium=medium, volume=one, tint=tint, **kw)[0], dev.render_chroma_to_host(cam, medium=medium, tint=tint, **kw)[0],
                        f"{what}: 1^3 grid, frame")
            # no volume, a ball: the homogeneous chroma kernels against the restatement
            ball = media(scene)["ball g=0.7"]
            assert_same(dev.render_chroma_to_host(cam, medium=ball, tint=tint, **kw)[0], cr.frame(host, cam, medium=ball, tint=tint, **ref_kw(scene, setting, w, h, spp, 12)),
                        f"{what}: volume == NULL, a ball")
    dev.close()


@pytest.mark.gpu
def test_handle_state_is_left_alone():
    """rt_render and rt_render_lit of a handle after a chroma call equal a fresh handle's."""
    host, camera, _ = scenes()["three balls"]
    cam = camera(24, 16, 2, 12)
    fresh = rb.DeviceScene(host, device=0)
    want_render, _ = fresh.render_to_host(cam)
    want_lit, _ = fresh.render_lit_to_host(cam)
    fresh.close()
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(GRIDS["16"]) as vol:
        dev.render_chroma_to_host(cam, medium=fog(0.3), volume=vol, tint=TINTS[0])
        dev.render_chroma_to_host(cam, medium=fog(0.3), tint=TINTS[1])
    got_render, _ = dev.render_to_host(cam)
    got_lit, _ = dev.render_lit_to_host(cam)
    assert_same(got_render, want_render, "rt_render after rt_render_chroma")
    assert_same(got_lit, want_lit, "rt_render_lit after rt_render_chroma")
    dev.close()


@pytest.mark.gpu
def test_cli_fog_tint_frames_are_the_python_path(test_config_text, tmp_path):
    """rtp_main --fog-tint with and without a grid file, and in a ball: the frame file holds the bytes of the Python path."""
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera_at(0.0)
    density = GRIDS["2x3x5"]
    with open(tmp_path / "grid.vol", "wb") as f:
        f.write(b"VOL1\n2 3 5\n" + np.asarray(density, "<f4").tobytes())
    box = (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0)
    with rb.Volume(density) as vol:
        for region, grid in (("box", True), ("box", False), ("ball", False)):
            where = ["--fog-box", ",".join(str(x) for x in box)] if region == "box" else ["--fog-ball", "0,0,0,3"]
            args = ["--lit", "--nee", "--light-tree", "--fog", "0.4:0.9:0.3", *where, "--fog-tint", "0.5,1,2"]
            args += ["--fog-grid", str(tmp_path / "grid.vol")] if grid else []
            out = subprocess.run([EXE, "--gpu", *args], input=text, capture_output=True, text=True, timeout=200)
            assert out.returncode == 0, out.stderr
            medium = dict(sigma_t=0.4, albedo=0.9, g=0.3, **(dict(box=box) if region == "box" else dict(ball=(0, 0, 0, 3))))
            fb, _ = dev.render_chroma_to_host(cam, nee=dict(select=1), medium=medium, volume=vol if grid else None, tint=(0.5, 1, 2))
            grey, _ = dev.render_volume_to_host(cam, nee=dict(select=1), medium=medium, volume=vol if grid else None)
            assert (fb != grey).any()
            assert open(tmp_path / "f_0.png", "rb").read() == rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp), (region, grid)
            os.remove(tmp_path / "f_0.png")
    dev.close()
