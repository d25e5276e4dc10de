"""rt_render_glow / rt_trace_samples_glow (include/rtp_amd.h, "emission in the medium"): a medium that emits.  The
contract's restatement is tests/cpu_native/glow_ref.c (tests/glow_reference.py); the CPU tests check the restatement and the ABI, the GPU
tests the kernels against the restatement, bit for bit.  Scenes, settings and protocols are tests/test_medium.py's and
tests/test_volume.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import glow_reference as gr
import medium_reference as mr
import rtp_bindings as rb
import volume_reference as vr
from test_lit import assert_same
from test_medium import (ABSORB_N, EQUAL_SPP, FOG_BOX, PROBE_VIEW, SETTINGS, _channel_z, _fog_ball_scene, all_ijs, dev_kw, media, ref_kw, scenes,
                         sun_map)
from test_nee_planes import MAT_LAMBERTIAN, MAT_LIGHT, material
from test_volume import BOX, GRIDS, IDENTITY_VIEW, WALK_TOL, fog, random_grid, special_camera

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
INVALID = 1
GLOWS = ((0.2, 1.0, 3.0), (0.0, 0.5, 0.0), (2.0, 0.1, 0.7))
# the heat grids of the probe and frame cases: random_grid with other seeds than GRIDS' (11, 12, 13)
HEATS = {"1": np.full((1, 1, 1), 0.75, np.float32), "2x3x5": random_grid((5, 3, 2), 111), "16": random_grid((16, 16, 16), 112),
         "1x1x64": random_grid((64, 1, 1), 113)}
COLUMNS = ("radiance", "rays", "events", "ends", "seeds", "cells", "glow_length")


# ---- no GPU needed ---------------------------------------------------------------------------------------------------------------------

def test_abi_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_glow_params_init", "rt_render_glow", "rt_trace_samples_glow"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert len(lib.rt_render_glow.argtypes) == 13 and len(lib.rt_trace_samples_glow.argtypes) == 18
    for name in ("render_glow", "render_glow_to_host", "trace_samples_glow"):
        assert hasattr(rb.DeviceScene, name)
    assert C.sizeof(rb.GlowParams) == 20
    assert [rb.GlowParams.__dict__[f].offset for f in ("struct_bytes", "source", "radiance")] == [0, 4, 8]
    p = rb.glow_params()
    assert p.struct_bytes == 20 and p.source == 0 and list(p.radiance) == [0.0, 0.0, 0.0]
    q = rb.glow_params(radiance=(0.5, 1, 2), source=2)
    assert list(q.radiance) == [0.5, 1.0, 2.0] and q.source == 2 and list(rb.glow_params(radiance=3).radiance) == [3.0] * 3
    lib.rt_glow_params_init(None)
    lib.rt_version_string.restype = C.c_char_p
    assert lib.rt_version_string()


def _calls(cam, lit, medium, volume, glow, heat):
    """(status, message) of rt_render_glow and of rt_trace_samples_glow with a null scene."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    pl = C.byref(lit) if lit is not None else None
    pm = C.byref(medium) if medium is not None else None
    pg = C.byref(glow) if glow is not None else None
    out = [lib.rt_render_glow(None, C.byref(cam), pl, pm, volume, pg, heat, None, 0, C.c_void_p(1 << 32), None, 1, None), lib.rt_get_last_error_string().decode()]
    out += [lib.rt_trace_samples_glow(None, C.byref(cam), pl, pm, volume, pg, heat, 1, ijs, f, r, r, s, s, s, s, r, f), lib.rt_get_last_error_string().decode()]
    return out


def test_refusals_before_the_scene_is_looked_at():
    """rt_render_volume's refusals in its order, then the glow's in the header's order, all with a null scene — nothing can have been
    enqueued, and a handle is never read (they are not handles; the one refusal that reads two, the heat grid's dimensions, is
    test_heat_dimensions_and_devices' on the GPU).  Each case also breaks every LATER rule it can, so the word it is refused with shows the order.
    What passes reaches the null-scene check.  Every message names the glow call."""
    cam = rb.rtiow_camera(8, 4, 2)
    handle = C.c_void_p(1 << 32)
    nan, inf = float("nan"), float("inf")
    box = dict(box=(0, 0, 0, 1, 1, 1))
    good = rb.medium_params(sigma_t=1.0, **box)
    thin = rb.medium_params(sigma_t=0.0, **box)

    def refused(word, medium=good, lit=None, volume=handle, glow=None, heat=None):
        st1, m1, st2, m2 = _calls(cam, lit, medium, volume, glow, heat)
        assert st1 == INVALID and word in m1 and "rt_render_glow" in m1, (word, m1)
        assert st2 == INVALID and word in m2 and "rt_trace_samples_glow" in m2, (word, m2)
    bad_glow = rb.glow_params(radiance=(1, -1, 1), source=3)
    for volume in (handle, None):
        short = rb.medium_params(sigma_t=1.0, **box)
        short.struct_bytes = 4
        refused("rt_medium_params", short, volume=volume, glow=bad_glow)
        for s in (-0.5, nan, inf):
            refused("sigma_t must", rb.medium_params(sigma_t=s, **box), volume=volume, glow=bad_glow)
        refused("albedo", rb.medium_params(sigma_t=1.0, albedo=(0.5, 1.5, 0.5), **box), volume=volume, glow=bad_glow)
        refused("|g|", rb.medium_params(sigma_t=1.0, g=0.96, **box), volume=volume, glow=bad_glow)
        refused("lo < hi", rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, -1, 1)), volume=volume, glow=bad_glow)
        # rt_render_lit's come first, the medium's before the volume's, the volume's before the glow's
        refused("mis", rb.medium_params(sigma_t=-1.0), lit=rb.lit_params(nee=dict(mis=2)), volume=volume, glow=bad_glow)
        # the glow's own, in order: struct_bytes, source, radiance, a glow without extinction, the grids
        short = rb.glow_params(radiance=(1, -1, 1), source=3)
        short.struct_bytes = 4
        refused("rt_glow_params", thin, volume=volume, glow=short, heat=handle)
        for source in (-1, 3):
            refused("source must", thin, volume=volume, glow=rb.glow_params(radiance=(1, -1, 1), source=source), heat=handle)
        for r in ((-0.5, 1, 1), (1, nan, 1), (1, 1, inf), (-1e-30, 1, 1)):
            refused("radiance", thin, volume=volume, glow=rb.glow_params(radiance=r, source=0), heat=handle)
        refused("sigma_t > 0", thin, volume=volume, glow=rb.glow_params(radiance=(0, 0, 1e-30), source=0), heat=handle)
        refused("is for source 2 only", volume=volume, glow=rb.glow_params(radiance=1, source=0), heat=handle)
        refused("is for source 2 only", volume=volume, glow=None, heat=handle)          # (no glow: heat is still checked)
    refused("without extinction", None, volume=None, glow=rb.glow_params(radiance=1, source=1), heat=handle)
    refused("region 2", None, glow=bad_glow)
    refused("region 2", rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), glow=bad_glow)
    for source in (1, 2):
        refused("need a volume", volume=None, glow=rb.glow_params(radiance=1, source=source), heat=handle if source == 1 else None)
    refused("needs a heat grid", glow=rb.glow_params(radiance=1, source=2))
    refused("is for source 2 only", glow=rb.glow_params(radiance=1, source=1), heat=handle)
    # what passes reaches the scene
    for m, volume, glow in ((good, handle, rb.glow_params(radiance=(0.25, 1, 4), source=1)), (good, handle, None), (None, None, rb.glow_params(radiance=0)),
                            (rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), None, rb.glow_params(radiance=(0, 0, 1))), (good, handle, rb.glow_params(radiance=2)),
                            (thin, handle, rb.glow_params(radiance=0, source=1))):
        st1, m1, st2, m2 = _calls(cam, None, m, volume, glow, None)
        assert st1 == INVALID and "rt_render_glow: null scene" in m1, m1
        assert st2 == INVALID and "rt_trace_samples_glow: null scene" in m2, m2


def _grid_file(path, density):
    nz, ny, nx = density.shape
    with open(path, "wb") as f:
        f.write(b"VOL1\n" + ("%d %d %d\n" % (nx, ny, nz)).encode() + np.asarray(density, "<f4").tobytes())
    return str(path)


def test_cli_refusals(test_config_text, tmp_path):
    grid = _grid_file(tmp_path / "grid.vol", GRIDS["2x3x5"])
    other = _grid_file(tmp_path / "other.vol", GRIDS["1"])
    fog_args = ["--lit", "--fog", "0.5"]
    box = fog_args + ["--fog-box", "0,0,0,1,1,1"]
    cases = [(["--lit", "--fog-glow", "0.5,1,2"], "needs --lit --fog"),
             (fog_args + ["--fog-glow", "0.5,1,2", "--fog-tint", "1,2,3"], "--fog-tint"),
             (fog_args + ["--fog-glow", "0.5,1,2", "--fog-noise-target", "0.1"], "--fog-noise-target"),
             (fog_args + ["--fog-glow", "0.5,1,2", "--fog-denoise"], "--fog-denoise"),
             (box + ["--fog-glow", "0.5,1,2:density"], "needs --fog-grid"),
             (box + ["--fog-glow", "0.5,1,2", "--fog-heat", grid], "needs --fog-grid"),
             (box + ["--fog-grid", grid, "--fog-glow", "0.5,1,2:density", "--fog-heat", grid], "exclude each other"),
             (box + ["--fog-grid", grid, "--fog-heat", grid], "needs --fog-glow"),
             (box + ["--fog-grid", grid, "--fog-glow", "0.5,1,2", "--fog-heat", other], "dimensions"),
             (box + ["--fog-grid", grid, "--fog-glow", "0.5,1,2", "--fog-heat", str(tmp_path / "none.vol")], "--fog-grid's format"),
             (["--lit", "--fog", "0", "--fog-glow", "0.5,1,2"], "SIGMA > 0"),
             (fog_args + ["--fog-glow", "0.5,1"], "R,G,B"), (fog_args + ["--fog-glow", "0.5,-1,2"], "R,G,B"), (fog_args + ["--fog-glow", "0.5,1,2,3"], "R,G,B"),
             (fog_args + ["--fog-glow", "0.5,nan,2"], "R,G,B"), (fog_args + ["--fog-glow", "0.5,1,2:heat"], "R,G,B"), (fog_args + ["--fog-glow"], "R,G,B")]
    for extra, word in cases:
        res = subprocess.run([EXE, "--gpu"] + extra, input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert res.returncode == 99 and word in res.stderr and ("--fog-glow" in res.stderr or "--fog-heat" in res.stderr), (extra, res.returncode, res.stderr[-300:])


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_no_glow_is_the_grey_restatement(scene):
    """Radiance 0, 0, 0 (and no glow at all) hands the call over: every probe column and a whole frame equal volume_reference /
    medium_reference, bit for bit, and glow_length is 0 — regions 0 / 1 / 2 without a grid and the box with one."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    ijs = all_ijs(w, h, spp)
    cases = [(m, None) for m in media(scene).values()] + [(fog(0.3), GRIDS["2x3x5"])]
    for k, (medium, density) in enumerate(cases):
        setting = list(SETTINGS)[(2 * k + 1) % len(SETTINGS)]
        cam = camera(w, h, spp, 12)
        kw = ref_kw(scene, setting, w, h, spp, 12)
        if density is None:
            want = mr.trace(host, cam, ijs, medium=medium, **kw) + (np.zeros(len(ijs), np.int32),)
            want_frame = mr.frame(host, cam, medium=medium, **kw)
        else:
            want = vr.trace(host, cam, ijs, medium=medium, density=density, **kw)
            want_frame = vr.frame(host, cam, medium=medium, density=density, **kw)
        want = want + (np.zeros(len(ijs), np.float32),)
        for radiance in (None, 0.0, (0.0, -0.0, 0.0)):
            source = 1 if (density is not None and radiance is not None) else 0
            got = gr.trace(host, cam, ijs, medium=medium, density=density, radiance=radiance, source=source, **kw)
            for a, b, col in zip(got, want, COLUMNS):
                assert_same(a, b, f"{scene} / {setting} / case {k} / radiance {radiance}: {col}")
            assert_same(gr.frame(host, cam, medium=medium, density=density, radiance=radiance, source=source, **kw), want_frame,
                        f"{scene} / {setting} / case {k} / radiance {radiance}: frame")
        assert want[2].sum() > 0


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_restatement_identities(scene):
    """A 1 x 1 x 1 grid of density 1 under source 0 and under source 1 is the homogeneous box under source 0, in every column but cells and in
    whole frames; source 2 with the density as the heat is source 1, in every column — in every setting of tests/test_medium.py."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    ijs = all_ijs(w, h, spp)
    one = np.ones((1, 1, 1), np.float32)
    seen_events = seen_cells = 0
    for k, setting in enumerate(SETTINGS):
        medium = dict(sigma_t=0.25, albedo=(0.9, 0.85, 0.8), g=(-0.5, 0.0, 0.7)[k % 3], box=BOX)
        radiance = GLOWS[k % 3]
        cam = camera(w, h, spp, 12)
        kw = ref_kw(scene, setting, w, h, spp, 12)
        want = gr.trace(host, cam, ijs, medium=medium, radiance=radiance, **kw)
        want_frame = gr.frame(host, cam, medium=medium, radiance=radiance, **kw)
        assert not want[5].any() and (want[6] > 0).any()
        for source in (0, 1):
            got = gr.trace(host, cam, ijs, medium=medium, density=one, radiance=radiance, source=source, **kw)
            for j in (0, 1, 2, 3, 4, 6):
                assert_same(got[j], want[j], f"{scene} / {setting} / 1^3, source {source}: {COLUMNS[j]}")
            seen_events += int(got[2].sum())
            seen_cells += int(got[5].sum())
            assert_same(gr.frame(host, cam, medium=medium, density=one, radiance=radiance, source=source, **kw), want_frame, f"{scene} / {setting} / 1^3, source {source}: frame")
        density = GRIDS[("2x3x5", "16", "1x1x64")[k % 3]]
        a = gr.trace(host, cam, ijs, medium=medium, density=density, radiance=radiance, source=1, **kw)
        b = gr.trace(host, cam, ijs, medium=medium, density=density, radiance=radiance, source=2, heat=density.copy(), **kw)
        for x, y, col in zip(a, b, COLUMNS):
            assert_same(y, x, f"{scene} / {setting} / heat = density: {col}")
        c = gr.trace(host, cam, ijs, medium=medium, density=density, radiance=radiance, source=0, **kw)
        assert (c[6] != a[6]).any() and (c[0] != a[0]).any()          # (the source does matter)
    assert seen_events > 100 and seen_cells > seen_events


SLAB_GLOW = (0.2, 1.0, 3.0)


def _slab_camera(background=(0.0, 0.0, 0.0)):
    """tests/test_chroma.py's slab view: 9 x 9 pixels at ABSORB_N samples down the x axis onto the box (-1, 1)^3."""
    cam = rb.make_camera(9, 9, 8.0, (-9, 0.4, 0.3), (0, 0, 0), background, ABSORB_N, 8)
    o = np.array([cam.origin.e[k] for k in range(3)], np.float64)
    p00 = np.array([cam.pixel00_loc.e[k] for k in range(3)], np.float64)
    du = np.array([cam.pixel_delta_u.e[k] for k in range(3)], np.float64)
    dv = np.array([cam.pixel_delta_v.e[k] for k in range(3)], np.float64)

    def crossing(i, j):
        """(t at x = -1, t at x = 1, the unit direction's x) of the ray through (i, j), or None unless it runs from face to face."""
        dd = p00 + i * du + j * dv - o
        dd /= np.linalg.norm(dd)
        t = [(x - o[0]) / dd[0] for x in (-1.0, 1.0)]
        for tt in t:
            p = o + tt * dd
            if not (abs(p[1]) < 1.0 and abs(p[2]) < 1.0):
                return None
        return t[0], t[1], dd[0]
    return cam, crossing


def _check_pixels(mom, expected, what):
    """Per pixel and channel: the mean within |z| <= 4.5 of expected(i, j)[k] with the channel's own sample variance; pixels by
    tests/test_chroma.py's 1 % rule (the expected value varies by < 1 % over the pixel's corners), at least 9 of them."""
    checked = 0
    for j in range(9):
        for i in range(9):
            want = expected(i, j)
            corners = [expected(i + a, j + b) for a in (-0.5, 0.5) for b in (-0.5, 0.5)]
            if want is None or any(c is None for c in corners):
                continue
            cs = np.array(corners)
            if ((cs.max(0) - cs.min(0)) > 0.01 * want).any():
                continue
            checked += 1
            for k in range(3):
                mean = mom[j, i, k] / ABSORB_N
                var = max(mom[j, i, 3 + k] / ABSORB_N - mean * mean, 0.0) * (ABSORB_N / (ABSORB_N - 1.0)) / ABSORB_N
                z = (mean - want[k]) / np.sqrt(var)
                print(f"{what} pixel ({i}, {j}) channel {k} mean {mean:.5f} want {want[k]:.5f} z {z:+.2f}")
                assert abs(z) <= 4.5, (what, i, j, k, z)
    assert checked >= 9, checked


@pytest.mark.parametrize("sigma", [0.05, 0.5, 1.5])
def test_closed_form_homogeneous(sigma):
    """albedo = 0, a slab (a box of thickness 2 across x) in front of a black background, no emitters, pinhole, radiance (0.2, 1, 3): per
    pixel and channel the mean over ABSORB_N samples lies within |z| <= 4.5 of radiance_k / sigma * (1 - exp(-sigma L)), L in float64 from
    the pixel-centre ray.  And every sample is radiance_k * min(s, L_sample): glow_length > 0, the path ends at its first event, and the
    radiance is the float32 product exactly."""
    host = _fog_ball_scene()
    cam, crossing = _slab_camera()
    medium = dict(sigma_t=sigma, albedo=0.0, box=(-1, -1, -1, 1, 1, 1))

    def expected(i, j):
        c = crossing(i, j)
        return None if c is None else np.array(SLAB_GLOW) / sigma * (1.0 - np.exp(-sigma * (c[1] - c[0])))
    fb, mom = gr.frame(host, cam, medium=medium, radiance=SLAB_GLOW, emitters=False, moments=True)
    _check_pixels(mom, expected, f"sigma {sigma}")
    rad, rays, events, ends, seeds, cells, length = gr.trace(host, cam, all_ijs(9, 9, 16), medium=medium, radiance=SLAB_GLOW, emitters=False)
    assert (length > 0).all() and (events <= 1).all() and (rays == 1).all()
    assert (ends[events == 1] == mr.END_BLACK).all() and (ends[events == 0] == mr.END_MISS).all() and (events == 1).any() and (events == 0).any()
    assert_same(rad, np.float32(SLAB_GLOW)[None, :] * length[:, None], "a sample is radiance * glow_length")
    assert length.max() < 2.1 and (length[events == 0] > 1.99).all()


def test_closed_form_grid():
    """The same slab as a 64 x 1 x 1 grid along the ray, a random density (a third of the cells empty) and a different random heat: source
    2 and source 1 against sum_c Tr_before(c) h_c (1 - exp(-sigma_c seg_c)) / sigma_c (h_c seg_c where sigma_c == 0) in float64."""
    host = _fog_ball_scene()
    cam, crossing = _slab_camera()
    sigma = 1.2
    medium = dict(sigma_t=sigma, albedo=0.0, box=(-1, -1, -1, 1, 1, 1))
    density, heat = random_grid((1, 1, 64), 41), random_grid((1, 1, 64), 42)
    rho, hh = density.ravel().astype(np.float64), heat.ravel().astype(np.float64)
    assert abs((rho == 0).mean() - 1 / 3) < 0.1 and ((rho == 0) & (hh > 0)).any() and ((hh == 0) & (rho > 0)).any() and (rho != hh).any()

    def expected_of(h):
        def expected(i, j):
            c = crossing(i, j)
            if c is None:
                return None
            seg = (2.0 / 64.0) / c[2]
            total, tau = 0.0, 0.0
            for k in range(64):
                s = sigma * rho[k]
                total += np.exp(-tau) * (h[k] * (1.0 - np.exp(-s * seg)) / s if s > 0 else h[k] * seg)
                tau += s * seg
            return np.array(SLAB_GLOW) * total
        return expected
    for source, h, kw in ((2, hh, dict(heat=heat)), (1, rho, {})):
        fb, mom = gr.frame(host, cam, medium=medium, density=density, radiance=SLAB_GLOW, source=source, emitters=False, moments=True, **kw)
        _check_pixels(mom, expected_of(h), f"source {source}")


FURNACE_B = (0.5, 1.0, 2.0)
FURNACE_A = (0.3, 0.6, 0.9)


def _furnace_scene(lamp):
    """tests/test_medium.py's fog-ball scene; lamp: with a DIFFUSE_LIGHT sphere of emit B inside the ball."""
    if not lamp:
        return _fog_ball_scene()
    spheres = np.array([[0, 1000, 0, 0.5, 0], [0.2, -0.1, 0.1, 0.3, 1]], np.float32)
    return rb.HostScene.from_arrays(spheres, np.zeros((0, 11), np.float32), [material(MAT_LAMBERTIAN), material(MAT_LIGHT, emit=FURNACE_B)])


@pytest.mark.parametrize("g", [0.0, 0.7])
@pytest.mark.parametrize("lamp", [None, 1, 0], ids=["no lamp", "lamp, mis", "lamp, light-only"])
def test_grey_body_furnace(g, lamp):
    """The test that pins the estimator together with scattering: a ball of optical diameter 2, albedo (0.3, 0.6, 0.9), under a background
    B = (0.5, 1, 2), emitting sigma_t (1 - a_k) B_k — what it absorbs of B.  The radiance is B everywhere, so the mean of the samples is
    B_k per channel within |z| <= 4.5 of their own standard error, and at most 0.1 % of them are cut by depth (max_depth = 200).  With a
    DIFFUSE_LIGHT sphere of emit B inside the ball (a black body at the same radiance), light samples with and without MIS: the same."""
    host = _furnace_scene(lamp is not None)
    cam = rb.make_camera(16, 16, 20.0, (0, 1, 8), (0, 0, 0), FURNACE_B, 16, 200)
    ijs = all_ijs(16, 16, 16)
    sigma_t = 1.0
    radiance = tuple(float(np.float32(sigma_t) * (np.float32(1.0) - np.float32(a)) * np.float32(b)) for a, b in zip(FURNACE_A, FURNACE_B))
    kw = dict(emitters=False) if lamp is None else dict(nee_mis=lamp)
    rad, rays, events, ends, seeds, cells, length = gr.trace(host, cam, ijs, medium=dict(sigma_t=sigma_t, albedo=FURNACE_A, g=g, ball=(0, 0, 0, 1.0)),
                                                             radiance=radiance, **kw)
    assert (ends == mr.END_DEPTH).mean() <= 0.001, (ends == mr.END_DEPTH).mean()
    assert events.max() >= 3 and (events > 0).mean() > 0.1 and (length > 0).mean() > 0.2
    if lamp is not None:
        assert (ends == mr.END_ABSORBED).mean() > 0.01          # (paths do reach the lamp)
    x = rad.astype(np.float64)
    z = (x.mean(0) - np.array(FURNACE_B)) / (x.std(0, ddof=1) / np.sqrt(len(x)))
    print("mean", x.mean(0), "z", z)
    assert (np.abs(z) <= 4.5).all(), z


def test_refined_grid_has_the_same_glow():
    """A grid pair (density, heat) and its 2 x nearest-neighbour refinement describe the same medium: glow_length of a sample's first path
    ray (max_depth = 1: a later ray may fall on the other side of a verdict) equal within tests/test_volume.py's WALK_TOL, relative to the
    largest emission-weighted length a ray through the box can have; and the radiance of whole paths per pixel and channel within |z| <= 4.5."""
    host, camera, _ = scenes()["three balls"]
    density, heat = random_grid((4, 3, 5), 51), random_grid((4, 3, 5), 52)
    fine = lambda a: a.repeat(2, 0).repeat(2, 1).repeat(2, 2)
    medium = dict(FOG_BOX, sigma_t=0.25)
    w, h, spp = PROBE_VIEW
    cam = camera(w, h, spp, 1)
    ijs = all_ijs(w, h, spp)
    diag = float(np.linalg.norm(np.array(BOX[3:]) - np.array(BOX[:3])))
    for source, hmax in ((0, 1.0), (1, float(density.max())), (2, float(heat.max()))):
        kw = dict(heat=heat) if source == 2 else {}
        kwf = dict(heat=fine(heat)) if source == 2 else {}
        a = gr.trace(host, cam, ijs, medium=medium, density=density, radiance=1.0, source=source, **kw)
        b = gr.trace(host, cam, ijs, medium=medium, density=fine(density), radiance=1.0, source=source, **kwf)
        err = np.abs(a[6].astype(np.float64) - b[6]) / (hmax * diag)
        print(f"source {source}: refinement max relative difference {err.max():.3e}")
        assert err.max() <= WALK_TOL, (source, err.max())
        assert (b[5] >= a[5]).all() and (a[6] > 0).mean() > 0.5
    cam = rb.make_camera(4, 4, 40.0, (0, 2, 7), (0, 1, 0), (0.05, 0.05, 0.05), EQUAL_SPP, 6)
    a = gr.frame(host, cam, medium=medium, density=density, radiance=GLOWS[0], source=2, heat=heat, moments=True)[1]
    b = gr.frame(host, cam, medium=medium, density=fine(density), radiance=GLOWS[0], source=2, heat=fine(heat), moments=True)[1]
    z = _channel_z(a, b, EQUAL_SPP)
    print("max |z|", float(np.abs(z).max()))
    assert np.abs(z).max() <= 4.5 and a[..., :3].sum() > 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------

def _probe_cases(scene):
    """(medium name or grid, source, radiance, setting, g, depth, camera): every setting on every scene — the regions 0 / 1 / 2 without a
    grid and the four grids in turn, the sources over the grids, g in {0, +-0.95} and the depths {1, 2, 12} spread over them — then the
    special cameras."""
    si = ["three balls", "night rtiow", "fuzz planes"].index(scene)
    where = ["all space", "ball", "box"] + list(GRIDS)
    out = []
    for k, setting in enumerate(SETTINGS):
        at = where[(k + 2 * si) % 7]
        out.append((at, (k + si) % 3 if at in GRIDS else 0, GLOWS[(k + si) % 3], setting, (0.0, 0.95, -0.95)[(k + si) % 3], (12, 2, 1)[(k + si) % 3] if k % 2 else 12, "scene"))
    out += [("16", 2, GLOWS[si], "mis", 0.0, 12, "inside"), ("box", 0, GLOWS[(si + 1) % 3], "glossy", 0.95, 12, "inside"),
            ("16", 1, GLOWS[(si + 2) % 3], "glossy", 0.95, 12, "fan"), ("1x1x64", (2, 0, 1)[si], GLOWS[si], "mis", 0.0, 12, "fan"),
            ("box", 0, GLOWS[(si + 1) % 3], "select", -0.95, 2, "fan"), ("1", (1, 2, 0)[si], GLOWS[si], "light-only", 0.0, 12, "scene")]
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
    """(no GPU) the probe cases hold every region, grid, source, g, depth, setting and camera on every scene."""
    names = ("three balls", "night rtiow", "fuzz planes")
    for scene in names:
        cases = _probe_cases(scene)
        assert {c[3] for c in cases} == set(SETTINGS) and {c[2] for c in cases} == set(GLOWS)
        assert {c[4] for c in cases} == {0.0, 0.95, -0.95} and {c[5] for c in cases} == {1, 2, 12} and {c[6] for c in cases} == {"scene", "inside", "fan"}
        assert {c[1] for c in cases if c[0] in GRIDS} == {0, 1, 2} and all(c[1] == 0 for c in cases if c[0] not in GRIDS)
    every = [c for s in names for c in _probe_cases(s)]
    assert {c[0] for c in every} == {"all space", "ball", "box"} | set(GRIDS)
    assert {(c[0], c[1]) for c in every if c[0] in GRIDS} == {(grid, source) for grid in GRIDS for source in (0, 1, 2)}
    for name, grid in GRIDS.items():
        assert HEATS[name].shape == grid.shape and (HEATS[name] != grid).any()


def _compare_probe(got, want, what):
    rad, rays, events, seeds, ns, es, ms, cells, length = got
    wrad, wrays, wevents, wends, wseeds, wcells, wlength = want
    assert_same(rad, wrad, what + ": radiance")
    assert_same(rays, wrays, what + ": rays")
    assert_same(events, wevents, what + ": medium events")
    assert_same(cells, wcells, what + ": cells")
    assert_same(length, wlength, what + ": glow_length")
    for k, col in enumerate((seeds, ns, es, ms)):
        assert_same(col, wseeds[:, k], what + f": final seed {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow", "fuzz planes"])
def test_probe_samples_equal_the_restatement(scene):
    host = scenes()[scene][0]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    seen_events = seen_cells = 0
    seen_length = 0.0
    volumes = {name: rb.Volume(g) for name, g in GRIDS.items()}
    heats = {name: rb.Volume(g) for name, g in HEATS.items()}
    with rb.Env(sun_map()) as env:
        for where, source, radiance, setting, g, depth, kind in _probe_cases(scene):
            medium, density = _medium_of(where, g)
            cam = _camera(scene, kind, w, h, spp, depth)
            want = gr.trace(host, cam, ijs, medium=medium, density=density, radiance=radiance, source=source, heat=HEATS[where] if source == 2 else None,
                            **ref_kw(scene, setting, w, h, spp, depth))
            got = dev.trace_samples_glow(cam, ijs, medium=medium, volume=volumes.get(where), glow=dict(radiance=radiance, source=source),
                                         heat=heats[where] if source == 2 else None, **dev_kw(scene, setting, env, w, h, spp, depth))
            _compare_probe(got, want, f"{scene} / {where} / source {source} / radiance {radiance} / {setting} / g {g} / depth {depth} / camera {kind}")
            seen_events += int(want[2].sum())
            seen_cells += int(want[5].sum())
            seen_length += float(want[6][np.isfinite(want[6])].sum())
    assert seen_events > 100 and seen_cells > 1000 and seen_length > 100.0
    for v in list(volumes.values()) + list(heats.values()):
        v.close()
    dev.close()


@pytest.mark.gpu
def test_frames_equal_the_restatement():
    """40 x 27 x 3 spp, 7 x 5 x 1, a 3-row shard of the first, sample_first = 5, sync = 0 on a torch stream, and one small frame through
    each of the sixteen instantiations of glow_render_kernel: pinhole / lens x the four emitter tables x no grid / grid."""
    import torch
    scene, setting = "three balls", "glossy"
    host, camera, _ = scenes()[scene]
    medium, density, radiance = fog(0.7), GRIDS["2x3x5"], GLOWS[0]
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env, rb.Volume(density) as vol, rb.Volume(HEATS["2x3x5"]) as heat, rb.Volume(GRIDS["16"]) as vol16, rb.Volume(HEATS["16"]) as heat16:
        for (w, h, spp), more in (((40, 27, 3), {}), ((7, 5, 1), {}), ((40, 27, 3), dict(shard=rb.Shard(3, 1, 4))), ((40, 27, 3), dict(sample_first=5))):
            cam = camera(w, h, spp, 12)
            want = gr.frame(host, cam, medium=medium, density=density, radiance=radiance, source=2, heat=HEATS["2x3x5"], **more, **ref_kw(scene, setting, w, h, spp, 12))
            got, _ = dev.render_glow_to_host(cam, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=heat, **more,
                                             **dev_kw(scene, setting, env, w, h, spp, 12))
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
        want = gr.frame(host2, cam, medium=fog(-0.5), density=GRIDS["16"], radiance=GLOWS[1], source=2, heat=HEATS["16"], **kw_r)
        stream = torch.cuda.Stream()
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        with torch.cuda.stream(stream):
            dev2.render_glow(cam, fb.data_ptr(), medium=fog(-0.5), volume=vol16, glow=dict(radiance=GLOWS[1], source=2), heat=heat16, stream=stream.cuda_stream,
                             sync=False, **kw_d)
        stream.synchronize()
        assert_same(fb.cpu().numpy(), want, "sync = 0 on a torch stream")
        # the sixteen instantiations, each on a small frame; the grid's with the three sources in turn
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
                    source = 0 if grid is None else k % 3
                    want = gr.frame(host2, cam, medium=fog(0.3), density=None if grid is None else GRIDS[grid], radiance=GLOWS[k % 3], source=source,
                                    heat=HEATS[grid] if source == 2 else None, **kw_r)
                    got, _ = dev2.render_glow_to_host(cam, medium=fog(0.3), volume=None if grid is None else vol, glow=dict(radiance=GLOWS[k % 3], source=source),
                                                      heat=heat if source == 2 else None, **kw_d)
                    assert_same(got, want, f"frame grid={grid} lens={lens} select={select} planes={planes} source={source}")
                    k += 1
        dev2.close()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_device_identities(scene):
    """No glow (None, radiance 0) is rt_render_volume — frames and probes, through the grey kernels, glow_length 0; a 1^3 grid of density 1
    under source 0 and 1 is the homogeneous box under source 0, each through its own glow kernels; source 2 with the density as the heat
    is source 1; volume == NULL runs in any region."""
    host, camera, _ = scenes()[scene]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env, rb.Volume(np.ones((1, 1, 1), np.float32)) as one, rb.Volume(GRIDS["2x3x5"]) as vol, rb.Volume(GRIDS["2x3x5"].copy()) as twin:
        for k, setting in enumerate(SETTINGS):
            kw = dev_kw(scene, setting, env, w, h, spp, 12)
            cam = camera(w, h, spp, 12)
            medium = fog((0.0, 0.7, -0.95)[k % 3])
            what = f"{scene} / {setting}"
            # the handover
            glow = (None, 0.0, dict(radiance=0.0, source=1))[k % 3]
            volume = vol if (k % 2 or k % 3 == 2) else None
            got = dev.trace_samples_glow(cam, ijs, medium=medium, volume=volume, glow=glow, **kw)
            for a, b in zip(got[:8], dev.trace_samples_volume(cam, ijs, medium=medium, volume=volume, **kw)):
                assert_same(a, b, f"{what}: no glow {glow}")
            assert not got[8].any()
            assert_same(dev.render_glow_to_host(cam, medium=medium, volume=volume, glow=glow, **kw)[0], dev.render_volume_to_host(cam, medium=medium, volume=volume, **kw)[0],
                        f"{what}: no glow {glow}, frame")
            # the 1^3 grid
            radiance = GLOWS[k % 3]
            hom = dev.trace_samples_glow(cam, ijs, medium=medium, glow=radiance, **kw)
            hom_frame = dev.render_glow_to_host(cam, medium=medium, glow=radiance, **kw)[0]
            for source in (0, 1):
                got = dev.trace_samples_glow(cam, ijs, medium=medium, volume=one, glow=dict(radiance=radiance, source=source), **kw)
                for j, col in zip((0, 1, 2, 3, 4, 5, 6, 8), ("radiance", "rays", "events", "seed", "nee seed", "env seed", "med seed", "glow_length")):
                    assert_same(got[j], hom[j], f"{what}: 1^3 grid, source {source}, {col}")
                assert got[7].sum() > 0 and not hom[7].any() and hom[2].sum() > 0 and (hom[8] > 0).any()
                assert_same(dev.render_glow_to_host(cam, medium=medium, volume=one, glow=dict(radiance=radiance, source=source), **kw)[0], hom_frame,
                            f"{what}: 1^3 grid, source {source}, frame")
            # heat = density
            a = dev.trace_samples_glow(cam, ijs, medium=medium, volume=vol, glow=dict(radiance=radiance, source=1), **kw)
            b = dev.trace_samples_glow(cam, ijs, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=twin, **kw)
            for j, (x, y) in enumerate(zip(a, b)):
                assert_same(y, x, f"{what}: heat = density, column {j}")
            assert_same(dev.render_glow_to_host(cam, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=twin, **kw)[0],
                        dev.render_glow_to_host(cam, medium=medium, volume=vol, glow=dict(radiance=radiance, source=1), **kw)[0], f"{what}: heat = density, frame")
            # no volume, a ball: the homogeneous glow kernels against the restatement
            ball = media(scene)["ball g=0.7"]
            assert_same(dev.render_glow_to_host(cam, medium=ball, glow=radiance, **kw)[0], gr.frame(host, cam, medium=ball, radiance=radiance, **ref_kw(scene, setting, w, h, spp, 12)),
                        f"{what}: volume == NULL, a ball")
    dev.close()


@pytest.mark.gpu
def test_heat_dimensions_and_devices():
    """A heat grid of other dimensions than the volume's is refused before the scene is looked at (a null scene: the dimensions' word, not
    the scene's), and with a scene as well; the same grids with equal dimensions reach the null-scene check."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    cam = rb.rtiow_camera(8, 4, 2)
    medium = rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, 1, 1))
    glow = rb.glow_params(radiance=1.0, source=2)
    with rb.Volume(GRIDS["2x3x5"]) as vol, rb.Volume(HEATS["2x3x5"]) as heat, rb.Volume(np.ones((5, 3, 3), np.float32)) as wide:
        for h, word in ((wide, "dimensions differ"), (heat, "null scene")):
            st = lib.rt_render_glow(None, C.byref(cam), None, C.byref(medium), vol._h, C.byref(glow), h._h, None, 0, C.c_void_p(1 << 32), None, 1, None)
            msg = lib.rt_get_last_error_string().decode()
            assert st == INVALID and word in msg and "rt_render_glow" in msg, msg
        host, camera, _ = scenes()["three balls"]
        dev = rb.DeviceScene(host, device=0)
        with pytest.raises(rb.RtError, match="dimensions differ"):
            dev.render_glow_to_host(camera(8, 4, 1, 4), medium=fog(0.0), volume=vol, glow=dict(radiance=1.0, source=2), heat=wide)
        dev.close()


@pytest.mark.gpu
def test_handle_state_is_left_alone():
    """rt_render and rt_render_lit of a handle after a glow call equal a fresh handle's."""
    host, camera, _ = scenes()["three balls"]
    cam = camera(24, 16, 2, 12)
    fresh = rb.DeviceScene(host, device=0)
    want_render, _ = fresh.render_to_host(cam)
    want_lit, _ = fresh.render_lit_to_host(cam)
    fresh.close()
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(GRIDS["16"]) as vol, rb.Volume(HEATS["16"]) as heat:
        dev.render_glow_to_host(cam, medium=fog(0.3), volume=vol, glow=dict(radiance=GLOWS[0], source=2), heat=heat)
        dev.render_glow_to_host(cam, medium=fog(0.3), glow=GLOWS[1])
    got_render, _ = dev.render_to_host(cam)
    got_lit, _ = dev.render_lit_to_host(cam)
    assert_same(got_render, want_render, "rt_render after rt_render_glow")
    assert_same(got_lit, want_lit, "rt_render_lit after rt_render_glow")
    dev.close()


@pytest.mark.gpu
def test_cli_fog_glow_frames_are_the_python_path(test_config_text, tmp_path):
    """rtp_main --fog-glow in a ball, with :density and a grid file, and with --fog-heat: the frame file holds the bytes of the Python path."""
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera_at(0.0)
    density, heat_grid = GRIDS["2x3x5"], HEATS["2x3x5"]
    grid_file, heat_file = _grid_file(tmp_path / "grid.vol", density), _grid_file(tmp_path / "heat.vol", heat_grid)
    box = (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0)
    with rb.Volume(density) as vol, rb.Volume(heat_grid) as heat:
        for region, source in (("ball", 0), ("box", 1), ("box", 2)):
            where = ["--fog-box", ",".join(str(x) for x in box)] if region == "box" else ["--fog-ball", "0,0,0,3"]
            args = ["--lit", "--nee", "--light-tree", "--fog", "0.4:0.9:0.3", *where, "--fog-glow", "0.5,0.25,0.125" + (":density" if source == 1 else "")]
            args += ["--fog-grid", grid_file] if source else []
            args += ["--fog-heat", heat_file] if source == 2 else []
            out = subprocess.run([EXE, "--gpu", *args], input=text, capture_output=True, text=True, timeout=200)
            assert out.returncode == 0, out.stderr
            medium = dict(sigma_t=0.4, albedo=0.9, g=0.3, **(dict(box=box) if region == "box" else dict(ball=(0, 0, 0, 3))))
            fb, _ = dev.render_glow_to_host(cam, nee=dict(select=1), medium=medium, volume=vol if source else None, glow=dict(radiance=(0.5, 0.25, 0.125), source=source),
                                            heat=heat if source == 2 else None)
            grey, _ = dev.render_volume_to_host(cam, nee=dict(select=1), medium=medium, volume=vol if source else None)
            assert (fb != grey).any()
            assert open(tmp_path / "f_0.png", "rb").read() == rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp), (region, source)
            os.remove(tmp_path / "f_0.png")
    dev.close()
