"""rt_nee_params.sample_planes: light samples of emissive QUAD, ELLIPSE and TRIANGLE planes in rt_render_nee and rt_render_lit
(include/rtp_amd.h).

The header fixes the two-kind emitter table (spheres, then planes), the area sample of a plane (steps 2p … 4p) and the weight of a BSDF
hit on a table plane in float32 order; tests/cpu_native/emit_ref.c restates rt_render_lit with that table on the oracle
(emit_reference.py), and the table, probed samples and frames of the device must equal it bit for bit.  On the CPU: the ABI and every
refusal, the restatement's identities against the two older restatements, its table, its scale (an analytic case), its expectation
(against the oracle's ray_color, by z-scores) and what it gains at equal samples."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import emit_reference as emr
import env_reference as er
import lens_reference as lensr
import lit_reference as lr
import nee_reference as nr
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID = 0, 1
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_LIGHT = 0, 1, 2, 3
QUAD, ELLIPSE, TRIANGLE = 0, 1, 2
LUM = np.array([0.2126, 0.7152, 0.0722])
LENS = (0.2, 12.0)


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} bytes differ (first at {np.argwhere(bad)[0]})"


def config_host(text):
    return rb.HostScene.from_config(text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg")))


def material(kind, albedo=(0.5, 0.5, 0.5), emit=(0, 0, 0), fuzz=0.0, ir=1.5):
    m = rb.Material()
    m.type = kind
    m.fuzz = fuzz
    m.ir = ir
    for k in range(3):
        m.albedo.e[k] = albedo[k]
        m.emit.e[k] = emit[k]
    return m


def night_rtiow():
    """rtiow with every eighth small sphere made DIFFUSE_LIGHT (test_nee.py's)."""
    base = rb.HostScene.rtiow()          # (kept alive: desc points into it)
    d = base.desc
    spheres, mats = [], []
    for i in range(d.num_spheres):
        s = d.spheres[i]
        m = d.materials[s.material_idx]
        if 0 < i < d.num_spheres - 3 and i % 8 == 5:
            m = material(MAT_LIGHT, emit=(6.0, 4.5, 3.0) if i % 16 == 5 else (1.5, 2.0, 3.0))
        spheres.append([s.center.e[0], s.center.e[1], s.center.e[2], s.radius, len(mats)])
        mats.append(rb.Material.from_buffer_copy(m))
    night = rb.HostScene.from_arrays(np.array(spheres, np.float32), np.zeros((0, 11), np.float32), mats)
    base.close()
    return night


def night_camera(w, h, spp, max_depth=50, eye=(13, 3, 2)):
    return rb.make_camera(w, h, 20.0, eye, (0, 0, 0), (0, 0, 0), spp, max_depth)


# ---- panel box ---------------------------------------------------------------------------------------------------------------------
# planes, in plane order (base, u, v, material, type)
FLOOR, WALL, PANEL, DISC, TRI, HIDDEN, OCCLUDER, GLOW = range(8)
PANEL_BOX_PLANES = np.array([
    [-6, 0, 6, 12, 0, 0, 0, 0, -12, 0, QUAD],                # LAMBERTIAN floor, normal +y
    [-6, 0, -4, 12, 0, 0, 0, 4.3, 0, 1, QUAD],               # LAMBERTIAN back wall, normal +z
    [-2, 5, 1.5, 4, 0, 0, 0, 0, -3, 5, QUAD],                # the ceiling panel
    [1.5, 1.2, -3.9, 3, 0, 0, 0, 2.6, 0, 6, ELLIPSE],        # an ellipse light in front of the wall
    [-4.5, 0, 0.5, 1.6, 0, 1.6, 0, 2.8, 0, 7, TRIANGLE],     # a triangle light standing on the floor: surfaces on both of its sides
    [3, 4.5, -1, 2, 0, 0, 0, 0, -2, 9, QUAD],                # a panel no scattering surface can see: the occluder lies just below it
    [2.5, 4.4, -0.5, 3, 0, 0, 0, 0, -3, 10, QUAD],           # … the occluder (the wall ends below both)
    [-1.2, 0.01, 5, 2.4, 0, 0, 0, 0, -1.6, 11, QUAD],        # a LAMBERTIAN quad that emits: vertices lie on an emitter itself
], np.float32)
PANEL_BOX_SPHERES = np.array([[-1.6, 1, 0, 1, 2], [1.6, 1, -0.5, 1, 3], [0, 0.6, 2.2, 0.6, 4], [3.6, 0.5, 2, 0.5, 8]], np.float32)


def panel_box():
    """A floor and a back wall, a LAMBERTIAN, a METAL (fuzz 0.4) and a DIELECTRIC ball, and six emitters: a QUAD ceiling panel, an ELLIPSE
    on the wall, a TRIANGLE standing on the floor, a sphere, a hidden panel and a LAMBERTIAN quad with emission; black background."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_LAMBERTIAN, (0.7, 0.5, 0.4)), material(MAT_LAMBERTIAN, (0.3, 0.5, 0.8)),
            material(MAT_METAL, (0.8, 0.7, 0.5), fuzz=0.4), material(MAT_DIELECTRIC, ir=1.5), material(MAT_LIGHT, emit=(6, 5, 4)),
            material(MAT_LIGHT, emit=(2, 3, 4)), material(MAT_LIGHT, emit=(4, 2, 3)), material(MAT_LIGHT, emit=(5, 5, 3)),
            material(MAT_LIGHT, emit=(3, 3, 3)), material(MAT_LAMBERTIAN, (0.5, 0.5, 0.5)),
            material(MAT_LAMBERTIAN, (0.5, 0.4, 0.3), emit=(0.8, 1.0, 0.6))]
    return rb.HostScene.from_arrays(PANEL_BOX_SPHERES, PANEL_BOX_PLANES, mats)


def box_camera(w, h, spp, depth=50):
    return rb.make_camera(w, h, 50.0, (0, 3, 10), (0, 1.8, 0), (0, 0, 0), spp, depth)


def _zscores(m_a, m_b, spp):
    """Per-pixel luminance z-scores of two estimators from their per-pixel channel sums and sums of squares (test_nee.py's)."""
    def stats(m):
        mean = m[..., :3] / spp
        ex2 = m[..., 3:] / spp
        var = np.maximum(ex2 - mean * mean, 0) * spp / (spp - 1)
        return mean @ LUM, var @ (LUM * LUM)
    ma, va = stats(m_a)
    mb, vb = stats(m_b)
    return (ma - mb) / np.sqrt((va + vb) / spp + 1e-30)


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_and_refusals():
    """The symbol and the struct; sample_planes outside {0, 1} is refused by all four calls (and the table probe) before the scene is
    looked at, naming the field; an 8-byte struct does not reach it; good parameters get as far as the null scene."""
    lib = rb.amd_lib()
    assert hasattr(lib, "rt_nee_emitter_table") and "rt_nee_emitter_table" in rb.RTP_AMD_SYMBOLS
    assert len(lib.rt_nee_emitter_table.argtypes) == 9
    assert C.sizeof(rb.NeeParams) == 16
    p = rb.nee_params(sample_planes=1)
    assert (p.struct_bytes, p.mis, p.sample_planes, p.reserved[0], p.reserved[1]) == (16, 1, 1, 1, 0)     # (one word, two views)
    assert rb.nee_params().sample_planes == 0
    assert bytes(p)[8:12] == (1).to_bytes(4, "little")
    assert hasattr(rb.DeviceScene, "nee_emitter_table")
    cam = rb.rtiow_camera(8, 4, 2)
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    n = C.c_int32()

    def calls(p):
        """(status, message) of the four calls and the table probe with nee parameters p and a null scene."""
        lit = rb.lit_params(nee=p)
        out = []
        for call in (lambda: lib.rt_render_nee(None, C.byref(cam), C.byref(p), None, 0, C.c_void_p(1 << 32), None, 1, None),
                     lambda: lib.rt_trace_samples_nee(None, C.byref(cam), C.byref(p), 1, ijs, f, r, s, s),
                     lambda: lib.rt_render_lit(None, C.byref(cam), C.byref(lit), None, 0, C.c_void_p(1 << 32), None, 1, None),
                     lambda: lib.rt_trace_samples_lit(None, C.byref(cam), C.byref(lit), 1, ijs, f, r, s, s, s),
                     lambda: lib.rt_nee_emitter_table(None, C.byref(p), 0, None, None, None, None, None, C.byref(n))):
            out.append((call(), lib.rt_get_last_error_string().decode()))
        return out
    for bad in (-1, 2):
        for st, msg in calls(rb.nee_params(sample_planes=bad)):
            assert st == INVALID and "sample_planes" in msg, (bad, msg)
    for good in (0, 1):
        for st, msg in calls(rb.nee_params(sample_planes=good)):
            assert st == INVALID and "sample_planes" not in msg, (good, msg)
        assert "null scene" in calls(rb.nee_params(sample_planes=good))[0][1]
    # an older caller's 8-byte struct: the field behind its end is not read
    old = rb.nee_params(sample_planes=2)
    old.struct_bytes = 8
    for st, msg in calls(old):
        assert st == INVALID and "sample_planes" not in msg, msg
    # … and a 12-byte one has it
    mid = rb.nee_params(sample_planes=2)
    mid.struct_bytes = 12
    assert all("sample_planes" in msg for _, msg in calls(mid))
    # mis is still checked, and first
    assert all("mis" in msg for _, msg in calls(rb.nee_params(mis=3, sample_planes=2)))
    # the lit calls read the nee parameters only when they sample emitters
    lit = rb.lit_params(emitters=False, nee=rb.nee_params(sample_planes=2))
    assert lib.rt_render_lit(None, C.byref(cam), C.byref(lit), None, 0, C.c_void_p(1 << 32), None, 1, None) == INVALID
    assert "null scene" in lib.rt_get_last_error_string().decode()


@pytest.mark.parametrize("depth", [2, 50])
def test_restatement_identities(test_config_text, depth):
    """emit_ref.c with sample_planes = 0 is nee_ref.c (pinhole, no environment) and lit_ref.c (environment and lens) bit for bit, and
    sample_planes = 1 changes nothing where no plane emits: the config scene and night rtiow."""
    m = er.sun_and_sky(64)
    shard = rb.Shard(4, 3, 2)
    chost = config_host(test_config_text)
    ccam = rb.CameraData.from_buffer_copy(chost.frame_camera(11))
    ccam.image_width, ccam.image_height, ccam.samples_per_pixel, ccam.max_depth = 32, 24, 4, depth
    for name, host, cam in (("config", chost, ccam), ("night rtiow", night_rtiow(), night_camera(32, 24, 4, depth))):
        assert emr.table(host, 1)[0].max() == 0, name          # (no plane in either table)
        for sh, first in ((None, 0), (shard, 0), (None, 37)):
            for mis in (1, 0):
                want = nr.frame(host, cam, mis, shard=sh, sample_first=first)
                for planes in (0, 1):
                    assert_same(emr.frame(host, cam, nee_mis=mis, planes=planes, shard=sh, sample_first=first), want,
                                f"{name} depth={depth} mis={mis} planes={planes} shard={sh is not None} first={first}: nee_ref")
            kw = dict(lens=LENS, nee_mis=1, rgb=m, env_params=dict(mode=1, scale=0.75), shard=sh, sample_first=first)
            want = lr.frame(host, cam, **kw)
            for planes in (0, 1):
                assert_same(emr.frame(host, cam, planes=planes, **kw), want, f"{name} depth={depth} planes={planes} first={first}: lit_ref")


def test_table_of_panel_box():
    host = panel_box()
    kind, idx, cdf, pmf, area = emr.table(host, 1)
    assert list(zip(kind, idx)) == [(0, 3), (1, PANEL), (1, DISC), (1, TRI), (1, HIDDEN), (1, GLOW)]
    assert cdf[-1] == 1.0 and (np.diff(cdf) > 0).all()
    assert_same(pmf, np.diff(np.concatenate([[np.float32(0)], cdf])).astype(np.float32), "pmf = cdf difference")
    d = host.desc
    want_area, w = [0.0], [sum(d.materials[8].emit.e) * 0.5 ** 2]
    for i in idx[1:]:
        row = PANEL_BOX_PLANES[i].astype(np.float64)
        k = {QUAD: 1.0, ELLIPSE: np.pi / 4, TRIANGLE: 0.5}[int(row[10])]
        a = k * np.linalg.norm(np.cross(row[3:6], row[6:9]))
        want_area.append(a)
        w.append(sum(d.materials[int(row[9])].emit.e) * float(np.float32(a)) / np.pi)
    w = np.array(w)
    assert np.allclose(pmf, w / w.sum(), rtol=1e-5, atol=0)
    want_area = np.array(want_area)
    assert (np.abs(area.astype(np.float64) - want_area) <= np.spacing(want_area.astype(np.float32))).all(), (area, want_area)
    assert area[0] == 0.0
    # sample_planes = 0: the sphere alone, as nee_ref.c has it
    k0, i0, c0, p0, a0 = emr.table(host, 0)
    assert (list(k0), list(i0), list(c0), list(p0), list(a0)) == ([0], [3], [1.0], [1.0], [0.0])
    assert_same(i0, nr.table(host)[0], "sphere-only table")


def test_analytic_mean():
    """A w x d QUAD panel of radiance L at height h, centred above a large LAMBERTIAN floor (albedo a), light sampling alone, max_depth
    2: a sample whose camera ray lands below the panel's centre has the mean a * L * Omega / (2 pi), Omega the panel's solid angle from
    there — within 4 standard errors (estimated from the samples), which N makes less than 1 % of the value."""
    w, d, h = 2.0, 3.0, 2.0
    L, a = np.array([4.0, 2.0, 1.0]), np.array([0.6, 0.5, 0.4])
    mats = [material(MAT_LAMBERTIAN, tuple(a)), material(MAT_LIGHT, emit=tuple(L))]
    planes = np.array([[-20, 0, 20, 40, 0, 0, 0, 0, -40, 0, QUAD], [-w / 2, h, d / 2, w, 0, 0, 0, 0, -d, 1, QUAD]], np.float32)
    host = rb.HostScene.from_arrays(np.zeros((0, 5), np.float32), planes, mats)
    # a narrow camera below the panel's height that looks down at the point under its centre: pixel (1, 1) of 3 x 3
    cam = rb.make_camera(3, 3, 0.5, (0, 1.0, 0.6), (0, 0, 0), (0, 0, 0), 1, 2)
    n = 1 << 16
    ijs = np.stack([np.full(n, 1), np.full(n, 1), np.arange(n)], 1).astype(np.int32)
    o, dr, _, _, _ = lensr.rays(cam, None, 0.0, 10.0, ijs)
    o, dr = o.astype(np.float64), dr.astype(np.float64)
    t = -o[:, 1] / dr[:, 1]
    x = o + t[:, None] * dr
    assert ((t > 0) & (np.hypot(x[:, 0], x[:, 2]) < 0.01)).all()          # every sample lands on the floor below the centre
    kind, idx, _ = emr.first_hit(host, cam, ijs)
    assert (kind == 1).all() and (idx == 0).all()
    rad, rays, _, _ = emr.trace(host, cam, ijs, nee_mis=0, planes=1)[:4]
    omega = 4 * np.arctan(w * d / (4 * h * np.sqrt(w * w / 4 + d * d / 4 + h * h)))
    want = a * L * omega / (2 * np.pi)
    got = rad.astype(np.float64)
    mean, se = got.mean(0), got.std(0, ddof=1) / np.sqrt(n)
    print("analytic mean: got", mean, "want", want, "4 se / value", 4 * se / want)
    assert (4 * se < 0.01 * want).all(), 4 * se / want
    assert (np.abs(mean - want) <= 4 * se).all(), (mean, want, se)
    assert (rays == 3).all()          # camera ray, shadow ray, BSDF ray
    # … and without sample_planes the same samples find the panel by the path alone: the same expectation, another estimator
    plain = emr.trace(host, cam, ijs, nee_mis=0, planes=0)[0].astype(np.float64)
    se0 = plain.std(0, ddof=1) / np.sqrt(n)
    assert (np.abs(plain.mean(0) - want) <= 4 * se0).all() and (se < se0).all()


UNBIASED_CAMERA = dict(w=8, h=8, spp=8192, depth=6)


def test_unbiased_against_the_oracle():
    """Panel box, 8 x 8 pixels x 8192 samples of each estimator from disjoint sample ranges (test_nee.py's protocol and bounds): the
    luminance means of every 2 x 2 block agree within 5 sigma and the whole image's within 4 — planes sampled with MIS against the
    oracle's ray_color, and planes sampled alone against MIS."""
    host = panel_box()
    c = UNBIASED_CAMERA
    cam = box_camera(c["w"], c["h"], c["spp"], c["depth"])
    spp = cam.samples_per_pixel
    _, plain = nr.frame(host, cam, nr.PLAIN, sample_first=0, moments=True)
    _, mis = emr.frame(host, cam, nee_mis=1, planes=1, sample_first=spp, moments=True)
    _, light = emr.frame(host, cam, nee_mis=0, planes=1, sample_first=2 * spp, moments=True)

    def blocks(m):
        return m.reshape(4, 2, 4, 2, 6).sum((1, 3))
    for name, x, y in (("mis/plain", mis, plain), ("light/mis", light, mis)):
        z = _zscores(blocks(x), blocks(y), spp * 4)
        za = _zscores(x.sum((0, 1)), y.sum((0, 1)), spp * 64)
        print(f"{name}: 2 x 2 blocks max |z| {np.abs(z).max():.3f}, image z {float(za):.3f}")
        assert np.abs(z).max() < 5.0, (name, np.abs(z).max())
        assert abs(za) < 4.0, (name, za)


# measured on the restatement, whose bits are the device's: luminance MSE of sample_planes = 1 over sample_planes = 0 at
# 16 spp, 48 x 32, against sample_planes = 1 at 8192 spp from a disjoint sample range
PANEL_BOX_MSE_RATIO = 0.668800


def test_quality_at_equal_samples():
    host = panel_box()
    truth = emr.frame(host, box_camera(48, 32, 8192), planes=1, sample_first=1 << 20).astype(np.float64) / 8192 @ LUM
    cam = box_camera(48, 32, 16)
    with_planes = emr.frame(host, cam, planes=1).astype(np.float64) / 16 @ LUM
    without = emr.frame(host, cam, planes=0).astype(np.float64) / 16 @ LUM
    ratio = float(((with_planes - truth) ** 2).mean() / ((without - truth) ** 2).mean())
    print(f"panel box MSE ratio sample_planes 1 / 0 at 16 spp: {ratio:.6f}")
    assert ratio < 1.0, ratio
    assert abs(ratio - PANEL_BOX_MSE_RATIO) <= 1e-4 * PANEL_BOX_MSE_RATIO, ratio


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _probe_set():
    """4 000 (i, j, s) of a 160 x 120 panel box view and where each first lands."""
    rng = np.random.default_rng(17)
    cam = box_camera(160, 120, 1)
    n = 4000
    ijs = np.stack([rng.integers(0, 160, n), rng.integers(0, 120, n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)
    return ijs, emr.first_hit(panel_box(), cam, ijs)


def _assert_probe_set_reaches(kind, idx, pt):
    on_floor = (kind == 1) & (idx == FLOOR)
    assert ((kind == 1) & (idx == GLOW)).sum() >= 20, "pixels on the emissive LAMBERTIAN quad"
    # the triangle's plane is x - z = -5 (normal (-1, 0, 1)): floor points close to it on either side
    side = pt[:, 2] - pt[:, 0] - 5.0
    near = on_floor & (np.abs(pt[:, 0] + 3.7) < 1.5) & (np.abs(pt[:, 2] - 1.3) < 1.5)
    assert (near & (side > 0)).sum() >= 10 and (near & (side < 0)).sum() >= 10, "floor on both sides of the triangle light"
    under = on_floor & (pt[:, 0] > 3) & (pt[:, 0] < 5) & (pt[:, 2] > -3) & (pt[:, 2] < -1)
    assert under.sum() >= 10, "floor under the hidden panel"


@pytest.mark.gpu
def test_emitter_tables_equal_the_restatement(test_config_text):
    rb.amd_lib().rt_set_device(0)
    for name, host in (("panel box", panel_box()), ("config", config_host(test_config_text))):
        dev = rb.DeviceScene(host, device=0)
        for planes in (1, 0):
            got = dev.nee_emitter_table({"sample_planes": planes})
            want = emr.table(host, planes)
            for g, w, what in zip(got, want, ("kind", "index", "cdf", "pmf", "area")):
                assert_same(g, w, f"{name} sample_planes={planes} {what}")
        assert_same(dev.nee_emitter_table()[1], dev.nee_light_table()[0], f"{name}: the default is the sphere-only table")
        assert (dev.nee_emitter_table({"sample_planes": 1})[0].max() == 1) == (name == "panel box")
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 50])
@pytest.mark.parametrize("mis", [1, 0])
def test_probe_samples_equal_the_restatement(mis, depth):
    rb.amd_lib().rt_set_device(0)
    ijs, (kind, idx, pt) = _probe_set()
    _assert_probe_set_reaches(kind, idx, pt)
    host = panel_box()
    cam = box_camera(160, 120, 1, depth)
    dev = rb.DeviceScene(host, device=0)
    got = dev.trace_samples_nee(cam, ijs, params={"mis": mis, "sample_planes": 1})
    want = emr.trace(host, cam, ijs, nee_mis=mis, planes=1)
    for g, w, what in zip(got, want, ("radiance", "rays", "seed", "nee seed")):
        assert_same(g, w, f"mis={mis} depth={depth} {what}")
    # the planes' samples were taken (the light stream draws differently than for the sphere alone), and the path's own stream is untouched
    alone = dev.trace_samples_nee(cam, ijs, params={"mis": mis})
    assert (got[3] != alone[3]).mean() > 0.2
    assert_same(got[2], alone[2], "path seeds")
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", ["default", "exact"])
def test_frames_equal_the_restatement(traversal):
    rb.amd_lib().rt_set_device(0)
    host = panel_box()
    dev = rb.DeviceScene(host, device=0, **({} if traversal == "default" else {"traversal": rb.TRAVERSAL_EXACT}))
    shard = rb.Shard(4, 3, 2)
    for mis in (1, 0):
        for depth in (2, 50):
            cam = box_camera(64, 48, 4, depth)
            for sh, first in ((None, 0), (shard, 0), (None, 37)):
                got, t = dev.render_nee_to_host(cam, params={"mis": mis, "sample_planes": 1}, shard=sh, sample_first=first)
                want = emr.frame(host, cam, nee_mis=mis, planes=1, shard=sh, sample_first=first)
                assert_same(got, want, f"{traversal} mis={mis} depth={depth} shard={sh is not None} first={first}")
                assert t.guarded == 0 and t.trace_scratch_bytes == 0
    dev.close()


@pytest.mark.gpu
def test_identities(test_config_text):
    rb.amd_lib().rt_set_device(0)
    chost = config_host(test_config_text)
    ccam = rb.CameraData.from_buffer_copy(chost.frame_camera(11))
    ccam.image_width, ccam.image_height, ccam.samples_per_pixel = 96, 64, 4
    # no plane emits: sample_planes = 1 is sample_planes = 0
    for name, host, cam in (("config", chost, ccam), ("night rtiow", night_rtiow(), night_camera(96, 64, 4))):
        dev = rb.DeviceScene(host, device=0)
        for mis in (1, 0):
            assert_same(dev.render_nee_to_host(cam, params={"mis": mis, "sample_planes": 1})[0], dev.render_nee_to_host(cam, params={"mis": mis})[0],
                        f"{name} mis={mis}")
        dev.close()
    host = panel_box()
    dev = rb.DeviceScene(host, device=0)
    for depth in (2, 50):
        cam = box_camera(64, 48, 4, depth)
        for mis in (1, 0):
            nee, _ = dev.render_nee_to_host(cam, params={"mis": mis, "sample_planes": 1}, sample_first=5)
            lit, _ = dev.render_lit_to_host(cam, nee={"mis": mis, "sample_planes": 1}, sample_first=5)
            assert_same(lit, nee, f"rt_render_lit (pinhole, no environment) depth={depth} mis={mis}")
            got, _ = dev.render_nee_to_host(cam, params={"mis": mis, "sample_planes": 0}, sample_first=5)
            assert_same(got, emr.frame(host, cam, nee_mis=mis, planes=0, sample_first=5), f"sample_planes = 0 depth={depth} mis={mis}")
            assert not np.array_equal(got, nee)
    dev.close()


@pytest.mark.gpu
def test_lit_with_planes_environment_and_lens():
    rb.amd_lib().rt_set_device(0)
    host = panel_box()
    m = er.sun_and_sky(256)
    ep = dict(mode=1, scale=0.75)
    ijs, _ = _probe_set()
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(m) as env:
        for mis, motion in ((1, False), (0, True)):
            def cameras(w, h, spp):
                close = rb.make_camera(w, h, 50.0, (0.3, 3.1, 10), (0, 1.8, 0), (0, 0, 0), spp, 50) if motion else None
                return box_camera(w, h, spp), close
            kw = dict(lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), nee={"mis": mis, "sample_planes": 1}, env=env, env_params=ep)
            rkw = dict(lens=LENS, nee_mis=mis, planes=1, rgb=m, env_params=ep)
            cam, close = cameras(64, 48, 4)
            got, _ = dev.render_lit_to_host(cam, cam_close=close, sample_first=3, **kw)
            assert_same(got, emr.frame(host, cam, cam_close=close, sample_first=3, **rkw), f"frame mis={mis} motion={motion}")
            cam, close = cameras(160, 120, 1)
            probed = dev.trace_samples_lit(cam, ijs, cam_close=close, **kw)
            want = emr.trace(host, cam, ijs, cam_close=close, **rkw)
            for g, w, col in zip(probed, want, ("radiance", "rays", "seed", "nee seed", "env seed")):
                assert_same(g, w, f"probe mis={mis} motion={motion}: {col}")
    dev.close()


@pytest.mark.gpu
def test_handle_state():
    rb.amd_lib().rt_set_device(0)
    host = panel_box()
    cam = box_camera(96, 64, 4)
    fresh = []
    for planes in (0, 1, 0):
        dev = rb.DeviceScene(host, device=0)
        fresh.append(dev.render_nee_to_host(cam, params={"sample_planes": planes})[0])
        dev.close()
    dev = rb.DeviceScene(host, device=0)
    first, _ = dev.render_to_host(cam)
    before = dev.last_timing()
    table = dev.nee_light_table()
    for planes, want in zip((0, 1, 0), fresh):
        assert_same(dev.render_nee_to_host(cam, params={"sample_planes": planes})[0], want, f"sample_planes={planes} on one handle")
    assert not np.array_equal(fresh[0], fresh[1])
    for g, w, what in zip(dev.nee_light_table(), table, ("index", "cdf", "pmf")):
        assert_same(g, w, f"rt_nee_light_table after a planes call: {what}")
    assert table[0].tolist() == [3]
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    again, _ = dev.render_to_host(cam)
    assert_same(again, first, "rt_render after the planes calls")
    dev.close()
