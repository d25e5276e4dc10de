"""rt_env / rt_render_env / rt_env_table / rt_env_lookup / rt_trace_samples_env: image-based lighting with importance sampling
(include/rtp_amd.h).

The header fixes the octahedral map, its sampling table, the light sample, the second RNG stream and both MIS weights in float32
order; tests/cpu_native/env_ref.c restates them on the oracle (env_reference.py) and the table, looked-up directions, probed samples and
frames must equal it bit for bit.  On the CPU: the ABI, every argument check, the map's geometry, the restatement's identities against
the oracle's ray_color, its scale (an analytic case) and its expectation (modes against each other, by z-scores), the image loaders
and the CLI refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import env_reference as er
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
OK, INVALID = 0, 1
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_LIGHT = 0, 1, 2, 3
LUM = np.array([0.2126, 0.7152, 0.0722])
MODES = (0, 1, 2)


def assert_same(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} bytes differ (first at {np.argwhere(bad)[0]})"


def config_host(text):
    return rb.HostScene.from_config(text.replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg")))


def config_camera(host, frame, w=96, h=64, spp=4, depth=50):
    cam = rb.CameraData.from_buffer_copy(host.frame_camera(frame))
    cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = w, h, spp, depth
    return cam


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
    """rtiow with every eighth small sphere made DIFFUSE_LIGHT (test_nee.py's scene): emitters the path finds beside the environment."""
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


def night_camera(w, h, spp, max_depth=50, background=(0, 0, 0)):
    return rb.make_camera(w, h, 20.0, (13, 3, 2), (0, 0, 0), background, spp, max_depth)


def three_ball_scene(spp=8192, depth=6):
    """LAMBERTIAN floor sphere, a METAL and a LAMBERTIAN ball, nothing emissive: lit by the environment alone."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_METAL, (0.8, 0.7, 0.5), fuzz=0.4), material(MAT_LAMBERTIAN, (0.3, 0.5, 0.8))]
    sph = np.array([[0, -100, 0, 100, 0], [-1.1, 1, 0, 1, 1], [1.1, 1, 0, 1, 2]], np.float32)
    cam = rb.make_camera(8, 8, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), spp, depth)
    return rb.HostScene.from_arrays(sph, np.zeros((0, 11), np.float32), mats), cam


def crafted_map():
    """4 x 4: row 2 black, texel (ix 1, iy 0) black, the rest distinct."""
    m = (np.arange(48, dtype=np.float32).reshape(4, 4, 3) + 1.0) / 8.0
    m[2] = 0.0
    m[0, 1] = 0.0
    return m


def probe_directions(n, count, seed):
    """Random directions plus the awkward ones: the axes, the fold lines (y = 0), the diagonals, and points on texel borders."""
    rng = np.random.default_rng(seed)
    d = [rng.normal(size=(count, 3))]
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [-1, 1, 0], [1, 0, -1],
                     [0, -1, 1], [1, 1, 1], [-1, -1, -1], [1, -1, 1], [-0.0, 1, 0.0], [0.0, -1, -0.0]], np.float64)
    d.append(axes)
    d.append(axes * 1e-20)
    d.append(axes * 1e18)
    fold = rng.normal(size=(count // 20, 3))
    fold[:, 1] = 0.0
    d.append(fold)
    near = rng.normal(size=(count // 20, 3))
    near[:, 1] *= 1e-8
    d.append(near)
    k = rng.integers(0, n + 1, size=(count // 10, 2))
    uv = (-1.0 + 2.0 * k / n).astype(np.float32)
    uv[:, 1] = np.where(rng.random(uv.shape[0]) < 0.5, uv[:, 1], rng.uniform(-1, 1, uv.shape[0]))
    d.append(er.decode(uv).astype(np.float64))
    return np.concatenate(d).astype(np.float32)


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_mirrors_symbols_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_env_params_init", "rt_env_create", "rt_env_destroy", "rt_env_table", "rt_env_lookup", "rt_env_from_equirect", "rt_render_env",
              "rt_trace_samples_env"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.EnvParams) == 64
    assert len(lib.rt_render_env.argtypes) == 10 and len(lib.rt_trace_samples_env.argtypes) == 10
    assert len(lib.rt_env_table.argtypes) == 7 and len(lib.rt_env_lookup.argtypes) == 6
    p = rb.env_params()
    assert (p.struct_bytes, p.mode, p.scale, p.camera_visible) == (64, 1, 1.0, 1)
    assert list(p.rot) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(p.reserved) == [0, 0, 0]
    assert rb.env_params(mode=2, scale=0.5, rot=er.Z_UP).rot[5] == 1.0
    with pytest.raises(rb.RtError):
        rb.env_params(mis=1)
    for name in ("render_env", "render_env_to_host", "trace_samples_env"):
        assert hasattr(rb.DeviceScene, name)
    for name in ("from_equirect", "table", "lookup", "close", "__enter__", "__exit__"):
        assert hasattr(rb.Env, name)
    assert lib.rt_version_string().decode().startswith("rtp_amd 0.5")


def test_env_create_refusals():
    lib = rb.amd_lib()
    h = C.c_void_p()
    good = np.ones((4, 4, 3), np.float32)

    def create(a, n):
        return lib.rt_env_create(a.ctypes.data if a is not None else None, n, C.byref(h))
    assert create(None, 4) == INVALID
    assert lib.rt_env_create(good.ctypes.data, 4, None) == INVALID
    for n in (0, -3, 4097):
        assert create(np.ones((1, 1, 3), np.float32), n) == INVALID and " n " in lib.rt_get_last_error_string().decode()
    for bad in (-1e-6, float("nan"), float("inf"), -float("inf")):
        a = good.copy()
        a[2, 1, 1] = bad
        assert create(a, 4) == INVALID and "texel" in lib.rt_get_last_error_string().decode(), bad
        assert not h.value
    assert lib.rt_env_destroy(None) == OK
    assert lib.rt_env_table(None, 0, None, None, None, None, None) == INVALID
    assert lib.rt_env_lookup(None, 1, good.ctypes.data, good.ctypes.data, good.ctypes.data, good.ctypes.data) == INVALID
    assert lib.rt_env_lookup(None, -1, None, None, None, None) == INVALID
    out = np.zeros((2, 2, 3), np.float32)
    assert lib.rt_env_from_equirect(None, 4, 4, 2, out.ctypes.data) == INVALID
    assert lib.rt_env_from_equirect(good.ctypes.data, 0, 4, 2, out.ctypes.data) == INVALID
    assert lib.rt_env_from_equirect(good.ctypes.data, 4, 4, 4097, out.ctypes.data) == INVALID
    with pytest.raises(rb.RtError):
        rb.Env(np.ones((4, 3, 3), np.float32))


def test_argument_checks_come_first():
    """Bad parameters are refused by both calls before the environment and the scene are looked at; good ones reach the null checks."""
    lib = rb.amd_lib()
    cam = rb.rtiow_camera(8, 4, 2)
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    fake_env = C.c_void_p(1 << 32)        # (never dereferenced: the scene is null)

    def calls(p, env=None):
        pp = C.byref(p) if p is not None else None
        out = [lib.rt_render_env(None, C.byref(cam), env, pp, None, 0, C.c_void_p(1 << 32), None, 1, None)]
        out.append(lib.rt_get_last_error_string().decode())
        out.append(lib.rt_trace_samples_env(None, C.byref(cam), env, pp, 1, ijs, f, r, s, s))
        out.append(lib.rt_get_last_error_string().decode())
        return out
    tilted = [1, 0, 0, 0, 1, 0, 0, 1e-3, 1]
    bad = [("mode", dict(mode=-1)), ("mode", dict(mode=3)), ("scale", dict(scale=-0.5)), ("scale", dict(scale=float("nan"))),
           ("scale", dict(scale=float("inf"))), ("camera_visible", dict(camera_visible=2)), ("rot", dict(rot=[0] * 9)),
           ("rot", dict(rot=[2, 0, 0, 0, 1, 0, 0, 0, 1])), ("rot", dict(rot=tilted)), ("rot", dict(rot=[float("nan")] + [0] * 8))]
    for word, kw in bad:
        st1, m1, st2, m2 = calls(rb.env_params(**kw), fake_env)
        assert st1 == INVALID and word in m1 and st2 == INVALID and word in m2, (kw, m1, m2)
    short = rb.env_params()
    short.struct_bytes = 4
    st1, m1, st2, m2 = calls(short, fake_env)
    assert st1 == INVALID and "struct_bytes" in m1 and st2 == INVALID and "struct_bytes" in m2
    almost = rb.env_params(rot=[1, 5e-5, 0, -5e-5, 1, 0, 0, 0, 1])       # within 1e-4: accepted
    for p in (None, rb.env_params(), rb.env_params(mode=0), rb.env_params(mode=2, scale=0.0, camera_visible=0, rot=er.Z_UP), almost):
        st1, m1, st2, m2 = calls(p)
        assert st1 == INVALID and "null environment" in m1 and st2 == INVALID and "null environment" in m2, (m1, m2)
        st1, m1, st2, m2 = calls(p, fake_env)
        assert st1 == INVALID and "null scene" in m1, m1
        assert st2 == INVALID, m2
    # an older caller's 8-byte struct: mode is read, the rest keeps its defaults
    p = rb.env_params(mode=5, scale=-1.0)
    p.struct_bytes = 8
    assert calls(p, fake_env)[0] == INVALID and "mode" in calls(p, fake_env)[1]
    p.mode = 2
    assert "null scene" in calls(p, fake_env)[1]
    assert lib.rt_trace_samples_env(None, C.byref(cam), fake_env, None, -1, None, None, None, None, None) == INVALID


def test_octahedral_map_round_trip_and_solid_angles():
    """decode∘encode is the identity on texel centres, and the texels' solid angles (2 / n)^2 / |p_c|^3 sum to 4 pi."""
    for n in (1, 2, 7, 64):
        c = (-1.0 + (2.0 * np.arange(n) + 1.0) / n).astype(np.float32)
        u, v = np.meshgrid(c, c, indexing="xy")
        dirs = er.decode(np.stack([u.ravel(), v.ravel()], 1))
        assert np.allclose(np.linalg.norm(dirs.astype(np.float64), axis=1), 1.0, atol=1e-6)
        rgb = np.arange(n * n * 3, dtype=np.float32).reshape(n, n, 3)
        tex, rad, _ = er.lookup(rgb, dirs)
        assert tex.tolist() == list(range(n * n)), n
        assert_same(rad, rgb.reshape(-1, 3), f"radiance n={n}")
        assert_same(er.lookup(rgb, dirs * np.float32(37.5))[0], tex, "the lookup ignores the direction's length")
        assert np.allclose(er.texel_directions(n).reshape(-1, 3), dirs, atol=1e-6)
    w = er.texel_weights(er.constant_map(8, (1.0, 0.0, 0.0)))
    assert abs(w.sum() / (4 * np.pi) - 1) < 1e-4
    assert np.allclose(w, er.texel_solid_angles(8), rtol=1e-12)
    assert abs(er.texel_solid_angles(64).sum() / (4 * np.pi) - 1) < 1e-7
    # the pole axis is +y; sign(0) = +1 on the lower fold
    tex, _, _ = er.lookup(np.zeros((4, 4, 3), np.float32), np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32))
    assert tex.tolist() == [2 * 4 + 2, 3 * 4 + 3, 2 * 4 + 3, 3 * 4 + 2]


def test_reference_table_of_a_crafted_map():
    m = crafted_map()
    count, rc, rp, cc, cp = er.table(m)
    assert count == 4
    assert rc[-1] == 1.0 and (np.diff(rc) >= 0).all() and rp[2] == 0.0 and rc[2] == rc[1]
    assert_same(rp, np.diff(np.concatenate([[np.float32(0)], rc])).astype(np.float32), "row pmf = cdf difference")
    assert abs(float(rp.astype(np.float64).sum()) - 1) < 1e-6
    for iy in (0, 1, 3):
        assert cc[iy, -1] == 1.0 and (np.diff(cc[iy]) >= 0).all()
        assert_same(cp[iy], np.diff(np.concatenate([[np.float32(0)], cc[iy]])).astype(np.float32), "conditional pmf = cdf difference")
        assert abs(float(cp[iy].astype(np.float64).sum()) - 1) < 1e-6
    assert (cc[2] == 0).all() and (cp[2] == 0).all() and cp[0, 1] == 0.0 and cc[0, 1] == cc[0, 0]
    w = er.texel_weights(m)
    assert np.allclose(rp[:, None] * cp, w / w.sum(), rtol=1e-5, atol=1e-8)
    # zero-weight texels are unreachable: a pick is the smallest entry with u < cdf, for every u in [0, 1]
    us = np.concatenate([np.linspace(0, 1, 4097), rc, cc.ravel()]).astype(np.float32)
    rows = np.searchsorted(rc, us, side="right")
    assert 2 not in rows and (rows[us < 1] < 4).all()
    assert 1 not in np.searchsorted(cc[0], us, side="right")
    # density: pl of a direction is its texel's pj * n^2 / 4 * |p|^3, and E[1 / pl] over the table is 4 pi (here: summed exactly)
    dirs = er.texel_directions(4).reshape(-1, 3)
    _, _, pl = er.lookup(m, dirs)
    pj = (rp[:, None] * cp).ravel()
    live = pj > 0
    assert (pl[~live] == 0).all() and live.sum() == 11
    assert np.allclose(pl[live] * er.texel_solid_angles(4).ravel()[live], pj[live], rtol=1e-5)
    # an all-black map has an empty table
    assert er.table(np.zeros((4, 4, 3), np.float32))[0] == 0


def test_reference_identities_against_the_oracle(test_config_text):
    """mode 0, a constant map c, scale 1, any rot = ray_color with background c; an all-black map, any mode = background 0;
    camera_visible = 0 changes the camera rays that miss, and nothing else."""
    import oracle_bindings as ob
    host = config_host(test_config_text)
    cam = config_camera(host, 5, 48, 32, 3)
    c = (0.25, 0.5, 0.75)
    cam.background.e[0], cam.background.e[1], cam.background.e[2] = c
    want = ob.render(host, cam, threads=8)
    assert_same(er.frame(host, cam, None, threads=8), want, "plain")
    for rot in (None, er.Z_UP, (0, 0, 1, 1, 0, 0, 0, 1, 0)):
        p = dict(mode=0) if rot is None else dict(mode=0, rot=rot)
        assert_same(er.frame(host, cam, er.constant_map(8, c), p, threads=8), want, f"constant map rot={rot}")
    black = rb.CameraData.from_buffer_copy(cam)
    black.background.e[0] = black.background.e[1] = black.background.e[2] = 0.0
    want0 = ob.render(host, black, threads=8)
    for mode in MODES:
        assert_same(er.frame(host, cam, np.zeros((8, 8, 3), np.float32), dict(mode=mode, rot=er.Z_UP), threads=8), want0, f"black map mode={mode}")
    # camera_visible = 0: the camera rays that miss add cam->background; every other sample is unchanged
    m = er.sun_and_sky(64)
    ii, jj, ss = np.meshgrid(np.arange(48), np.arange(32), np.arange(2), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], 1).astype(np.int32)
    for mode in MODES:
        vis = er.trace(host, cam, m, ijs, dict(mode=mode, rot=er.Z_UP))
        hid = er.trace(host, cam, m, ijs, dict(mode=mode, rot=er.Z_UP, camera_visible=0))
        first_miss = (vis[1] == 1) & (vis[0] != hid[0]).any(1)
        assert first_miss.sum() > 50, first_miss.sum()
        assert_same(hid[0][first_miss], np.broadcast_to(np.array(c, np.float32), (first_miss.sum(), 3)), f"hidden camera misses mode={mode}")
        assert_same(hid[0][~first_miss], vis[0][~first_miss], f"other samples mode={mode}")
        for k in (1, 2, 3):
            assert_same(hid[k], vis[k], f"rays and seeds mode={mode}")


def _analytic_scene(a):
    host = rb.HostScene.from_arrays(np.array([[0, 0, 0, 1, 0]], np.float32), np.zeros((0, 11), np.float32), [material(MAT_LAMBERTIAN, tuple(a))])
    cam = rb.make_camera(32, 32, 16.0, (4, 0, 0), (0, 0, 0), (9, 9, 9), 16, 2)      # the whole image lies inside the sphere's outline
    return host, cam


def test_reference_analytic_scale():
    """One LAMBERTIAN sphere of albedo a under a constant map of radiance 1, max_depth 2, every camera ray on the sphere: the convex
    sphere never sees itself, so every estimator's expectation is a.  Mode 0 returns a for every sample (the bounce always misses);
    modes 1 and 2 by z-score: the mean over 64 blocks of 256 samples against a, sigma from the blocks' spread, |z| < 4 per channel."""
    a = np.array([0.6, 0.5, 0.4])
    host, cam = _analytic_scene(a)
    ii, jj, ss = np.meshgrid(np.arange(32), np.arange(32), np.arange(16), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], 1).astype(np.int32)
    rng = np.random.default_rng(1)
    ijs = ijs[rng.permutation(len(ijs))]
    for rot in (None, er.Z_UP):
        for mode in MODES:
            p = dict(mode=mode) if rot is None else dict(mode=mode, rot=rot)
            rad, rays, _, _ = er.trace(host, cam, er.constant_map(16), ijs, p)
            rad = rad.astype(np.float64)
            if mode == 0:
                assert (rays == 2).all() and np.abs(rad - a[None, :]).max() < 1e-6
                continue
            assert set(np.unique(rays)) <= {2, 3} and (rays == 3).mean() > 0.3
            blocks = rad.reshape(64, -1, 3).mean(1)
            z = (blocks.mean(0) - a) / (blocks.std(0, ddof=1) / np.sqrt(64))
            assert np.abs(z).max() < 4.0, (mode, rot, z)
            assert np.abs(blocks.mean(0) / a - 1).max() < 0.02, (mode, blocks.mean(0))


def _zscores(m_a, m_b, spp):
    """Luminance z-scores of two estimators from their channel sums and sums of squares (test_nee.py's)."""
    def stats(m):
        mean = m[..., :3] / spp
        ex2 = m[..., 3:] / spp
        var = np.maximum(ex2 - mean * mean, 0) * spp / (spp - 1)
        return mean @ LUM, var @ (LUM * LUM)
    ma, va = stats(m_a)
    mb, vb = stats(m_b)
    return (ma - mb) / np.sqrt((va + vb) / spp + 1e-30)


def test_reference_is_unbiased_across_modes():
    """8 x 8 pixels x 8192 samples of each mode under the sun-and-sky map, from disjoint sample ranges: the luminance means of modes 1
    and 2 agree per 2 x 2 block of pixels within 5 sigma, and each agrees with mode 0 per 4 x 4 block within 5 sigma and over the whole
    image within 4.  (Larger blocks against mode 0: it finds the sun by chance only — a few hits per pixel here — and a block's sample
    variance is a fair estimate only once it holds some tens of them.)"""
    host, cam = three_ball_scene()
    spp = cam.samples_per_pixel
    m = er.sun_and_sky(256)
    mom = {}
    for mode in MODES:
        _, mom[mode] = er.frame(host, cam, m, dict(mode=mode), sample_first=mode * spp, moments=True)

    def blocks(x, b):
        return x.reshape(8 // b, b, 8 // b, b, 6).sum((1, 3))
    for a, b, size in ((1, 2, 2), (1, 0, 4), (2, 0, 4)):
        z = _zscores(blocks(mom[a], size), blocks(mom[b], size), spp * size * size)
        assert np.abs(z).max() < 5.0, (a, b, np.abs(z).max())
        za = _zscores(mom[a].sum((0, 1)), mom[b].sum((0, 1)), spp * 64)
        assert abs(za) < 4.0, (a, b, za)


def test_reference_picks_by_bisection_equal_the_linear_scan(test_config_text):
    host = config_host(test_config_text)
    cam = config_camera(host, 5, 48, 32, 1)
    rng = np.random.default_rng(5)
    ijs = np.stack([rng.integers(0, 48, 3000), rng.integers(0, 32, 3000), rng.integers(0, 1 << 20, 3000)], 1).astype(np.int32)
    m = er.sun_and_sky(256)
    for mode in (1, 2):
        p = dict(mode=mode, rot=er.Z_UP, scale=0.5)
        for g, w in zip(er.trace(host, cam, m, ijs, p, linear=False), er.trace(host, cam, m, ijs, p, linear=True)):
            assert_same(g, w, "bisection against linear scan")


def write_pfm(path, img, little=True):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n{'-1.0' if little else '1.0'}\n".encode())
        f.write(img[::-1].astype("<f4" if little else ">f4").tobytes())


def to_rgbe(img):
    """float RGB → RGBE bytes (h, w, 4), the classic rule: the largest channel's exponent, mantissas truncated."""
    v = img.max(-1)
    mant, expo = np.frexp(v)
    scale = np.where(v > 1e-32, mant * 256.0 / np.maximum(v, 1e-38), 0.0)
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    out[..., :3] = (img * scale[..., None]).astype(np.uint8)
    out[..., 3] = np.where(v > 1e-32, expo + 128, 0).astype(np.uint8)
    return out


def write_hdr(path, img, rle):
    h, w, _ = img.shape
    px = to_rgbe(img)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\n# written by a test\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n" + f"-Y {h} +X {w}\n".encode())
        for y in range(h):
            if not rle:
                f.write(px[y].tobytes())
                continue
            f.write(bytes([2, 2, w >> 8, w & 255]))
            for c in range(4):
                col = px[y, :, c]
                x = 0
                while x < w:
                    run = 1
                    while x + run < w and run < 127 and col[x + run] == col[x]:
                        run += 1
                    if run >= 3:
                        f.write(bytes([128 + run, int(col[x])]))
                        x += run
                    else:
                        lit = 1
                        while x + lit < w and lit < 128 and not (x + lit + 2 < w and col[x + lit] == col[x + lit + 1] == col[x + lit + 2]):
                            lit += 1
                        f.write(bytes([lit]) + col[x:x + lit].tobytes())
                        x += lit


def test_image_loaders(tmp_path):
    rng = np.random.default_rng(9)
    img = (rng.random((12, 20, 3)) ** 4 * 50).astype(np.float32)
    img[3:6, 2:15] = (4.0, 2.0, 0.5)         # (runs for the encoder)
    img[7, :] = 0.0
    for little in (True, False):
        p = str(tmp_path / f"a{int(little)}.pfm")
        write_pfm(p, img, little)
        assert_same(rb.load_hdr_image(p), img, f"PFM little={little}")
    for rle in (False, True):
        p = str(tmp_path / f"b{int(rle)}.hdr")
        write_hdr(p, img, rle)
        got = rb.load_hdr_image(p)
        # RGBE: a shared exponent and 8-bit truncated mantissas — each channel within 2^-7 of the pixel's largest one
        assert got.shape == img.shape and (np.abs(got - img) <= img.max(-1, keepdims=True) / 128 + 1e-30).all(), rle
        assert_same(got, to_rgbe(img)[..., :3] * np.ldexp(np.float32(1), to_rgbe(img)[..., 3].astype(np.int32) - 136)[..., None] *
                    (to_rgbe(img)[..., 3:] > 0), f"RGBE decode rle={rle}")
    assert os.path.getsize(tmp_path / "b1.hdr") < os.path.getsize(tmp_path / "b0.hdr")
    # truncated and bad-magic files are refused
    whole = open(tmp_path / "a1.pfm", "rb").read()
    hdr = open(tmp_path / "b1.hdr", "rb").read()
    flat = open(tmp_path / "b0.hdr", "rb").read()
    for name, data in (("cut.pfm", whole[:-5]), ("cut.hdr", hdr[:-3]), ("cutflat.hdr", flat[:-1]), ("magic.pfm", b"PG" + whole[2:]),
                       ("magic.hdr", b"#?RADIANCX" + hdr[10:]), ("head.hdr", hdr.replace(b"-Y 12 +X 20", b"+Y 12 +X 20")),
                       ("format.hdr", hdr.replace(b"rle_rgbe", b"rle_xyze")), ("empty.pfm", b""), ("jpeg.pfm", b"\xff\xd8\xff\xe0")):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(rb.RtError):
            rb.load_hdr_image(str(tmp_path / name))
    with pytest.raises(rb.RtError):
        rb.load_hdr_image(str(tmp_path / "missing.hdr"))


def test_from_equirect_integrates_the_upper_hemisphere():
    """A lat-long image that is 1 above the horizon and 0 below, resampled to n = 64: radiance x solid angle sums to 2 pi within 1 %."""
    img = np.zeros((64, 128, 3), np.float32)
    img[:32] = 1.0
    m = rb.Env.equirect_to_octahedral(img, 64)
    assert m.shape == (64, 64, 3) and m.min() >= 0 and m.max() <= 1
    total = (m[..., 0].astype(np.float64) * er.texel_solid_angles(64)).sum()
    assert abs(total / (2 * np.pi) - 1) < 0.01, total
    # the pole axis is +y and u follows get_sphere_uv: a map that is 1 where phi = atan2(-z, x) + pi lies in the first quarter
    img = np.zeros((32, 64, 3), np.float32)
    img[:, :16] = 1.0
    m = rb.Env.equirect_to_octahedral(img, 32)
    d = er.texel_directions(32)
    phi = np.arctan2(-d[..., 2], d[..., 0]) + np.pi
    inside = (phi > 0.2) & (phi < np.pi / 2 - 0.2) & (np.abs(d[..., 1]) < 0.9)
    outside = (phi > np.pi / 2 + 0.2) & (phi < 2 * np.pi - 0.2) & (np.abs(d[..., 1]) < 0.9)
    assert (m[inside] == 1).all() and (m[outside] == 0).all()


def test_cli_refusals(test_config_text, tmp_path):
    img = np.ones((4, 8, 3), np.float32)
    good = str(tmp_path / "sky.pfm")
    write_pfm(good, img)
    (tmp_path / "cut.pfm").write_bytes(open(good, "rb").read()[:-7])
    (tmp_path / "bad.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 4 +X\n")
    neg = img.copy()
    neg[1, 1, 1] = -1.0
    write_pfm(str(tmp_path / "neg.pfm"), neg)
    before = sorted(os.listdir(tmp_path))
    cases = [(["--env", good, "--nee"], {}), (["--env", good, "--lens", "0.1:10"], {}), (["--env", good, "--motion-blur", "0.5"], {}),
             (["--env", good, "--adaptive", "0.1"], {}), (["--env", good, "--denoise-temporal"], {}), (["--env", good, "--devices", "2"], {}),
             (["--env", good, "--shard", "2"], {}), (["--env", good], {"RTP_DEVICES": "2"}), (["--env", good, "--env-mode", "both"], {}),
             (["--env", good, "--env-scale", "-1"], {}), (["--env", good, "--env-scale", "x"], {}), (["--env", good, "--env-up", "x"], {}),
             (["--env", good + ":0"], {}), (["--env", good + ":5000"], {}), (["--env"], {}), (["--env-mode", "mis"], {}),
             (["--env", str(tmp_path / "missing.hdr")], {}), (["--env", str(tmp_path / "cut.pfm") + ":8"], {}),
             (["--env", str(tmp_path / "bad.hdr")], {}), (["--env", str(tmp_path / "neg.pfm") + ":8"], {})]
    for args, env in cases:
        r = subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                           env={**os.environ, **env})
        assert r.returncode == 99 and "--env" in r.stderr, (args, env, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (args, os.listdir(tmp_path))


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def quality_scene():
    host, _ = three_ball_scene()
    return host, rb.make_camera(48, 32, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), 8192, 6)


@pytest.mark.gpu
def test_tables_and_lookups_equal_the_reference():
    rb.amd_lib().rt_set_device(0)
    for name, m in (("crafted", crafted_map()), ("sun and sky", er.sun_and_sky(256)), ("constant 7", er.constant_map(7, (0.5, 1, 2))),
                    ("one texel", er.constant_map(1)), ("black", np.zeros((5, 5, 3), np.float32))):
        n = m.shape[0]
        with rb.Env(m) as env:
            count, rc, rp, cc, cp = er.table(m)
            for row in sorted({0, n // 2, n - 1, 2 % n}):
                got = env.table(row)
                assert got[0] == count, name
                for g, w, what in zip(got[1:], (rc, rp, cc[row], cp[row]), ("row cdf", "row pmf", "conditional cdf", "conditional pmf")):
                    assert_same(g, w, f"{name} row {row} {what}")
            dirs = probe_directions(n, 100000, 11)
            for g, w, what in zip(env.lookup(dirs), er.lookup(m, dirs), ("texel", "radiance", "pl")):
                assert_same(g, w, f"{name} lookup {what}")
    with pytest.raises(rb.RtError):
        rb.Env(er.constant_map(4)).table(4)


@pytest.mark.gpu
def test_probe_samples_equal_the_reference(test_config_text):
    rb.amd_lib().rt_set_device(0)
    rng = np.random.default_rng(3)
    n = 10000
    m = er.sun_and_sky(256)
    with rb.Env(m) as env:
        for name, host, cam, rot in (("config", config_host(test_config_text), None, er.Z_UP), ("night rtiow", night_rtiow(), night_camera(320, 180, 1), None)):
            if cam is None:
                cam = host.frame_camera(5)
            dev = rb.DeviceScene(host, device=0)
            ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)
            plain = dev.trace_samples(cam, ijs)
            for mode in MODES:
                p = dict(mode=mode, scale=0.75)
                if rot is not None:
                    p["rot"] = rot
                got = dev.trace_samples_env(cam, env, ijs, params=p)
                want = er.trace(host, cam, m, ijs, p)
                for g, w, what in zip(got, want, ("radiance", "rays", "seed", "env seed")):
                    assert_same(g, w, f"{name} mode={mode} {what}")
                # the path's own stream is rt_trace_samples's; light samples were taken in modes 1 and 2 only
                assert_same(got[2], plain[2], f"{name} path seeds")
                if mode == 0:
                    assert_same(got[1], plain[1], f"{name} mode 0 rays")
                else:
                    assert (got[1] > plain[1]).mean() > 0.02
            dev.close()


@pytest.mark.gpu
def test_frames_equal_the_reference(test_config_text):
    rb.amd_lib().rt_set_device(0)
    m = er.sun_and_sky(256)
    env = rb.Env(m)
    host = night_rtiow()
    dev = rb.DeviceScene(host, device=0)
    for mode in MODES:
        for visible in (1, 0):
            cam = night_camera(96, 64, 8, background=(0.1, 0.2, 0.3))
            p = dict(mode=mode, camera_visible=visible, scale=1.5 if visible else 1.0)
            got, t = dev.render_env_to_host(cam, env, params=p)
            assert_same(got, er.frame(host, cam, m, p), f"night rtiow mode={mode} visible={visible}")
            assert t.trace_launches >= 1 and t.guarded == 0 and t.trace_scratch_bytes == 0
    dev.close()
    host = config_host(test_config_text)
    dev = rb.DeviceScene(host, device=0)
    shard = rb.Shard(4, 3, 2)
    for mode in MODES:
        for depth in (2, 50):
            cam = config_camera(host, 11, 96, 64, 4, depth)
            p = dict(mode=mode, rot=er.Z_UP)
            for sh, first in ((None, 0), (shard, 0), (None, 37)):
                got, _ = dev.render_env_to_host(cam, env, params=p, shard=sh, sample_first=first)
                want = er.frame(host, cam, m, p, shard=sh, sample_first=first)
                assert_same(got, want, f"config mode={mode} depth={depth} shard={sh is not None} first={first}")
    dev.close()
    env.close()


@pytest.mark.gpu
def test_identities_against_rt_render_samples(test_config_text):
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    c = (0.7, 0.8, 1.0)
    cam = rb.rtiow_camera(160, 90, 8)
    black = rb.make_camera(160, 90, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), 8, 50)
    with rb.Env(er.constant_map(16, c)) as sky, rb.Env(np.zeros((16, 16, 3), np.float32)) as night:
        for config in (dict(), dict(traversal=rb.TRAVERSAL_EXACT)):
            dev = rb.DeviceScene(host, device=0, **config)
            for first in (0, 5):
                want, _ = dev.render_to_host(cam, sample_first=first)
                for rot in (None, er.Z_UP):
                    p = dict(mode=0) if rot is None else dict(mode=0, rot=rot)
                    got, t = dev.render_env_to_host(cam, sky, params=p, sample_first=first)
                    assert_same(got, want, f"rtiow constant map {config} rot={rot} first={first}")
                    assert t.workgroup_size == 256
                want0, _ = dev.render_to_host(black, sample_first=first)
                for mode in MODES:
                    got, _ = dev.render_env_to_host(cam, night, params=dict(mode=mode), sample_first=first)
                    assert_same(got, want0, f"rtiow black map {config} mode={mode} first={first}")
            dev.close()
    # camera_visible = 0 (no call to equal: against the restatement), on the config scene with its rotation
    chost = config_host(test_config_text)
    ccam = config_camera(chost, 3, 96, 64, 4)
    ccam.background.e[0], ccam.background.e[1], ccam.background.e[2] = 0.3, 0.1, 0.2
    m = er.sun_and_sky(256)
    dev = rb.DeviceScene(chost, device=0)
    with rb.Env(m) as env:
        for mode in MODES:
            p = dict(mode=mode, rot=er.Z_UP, camera_visible=0)
            got, _ = dev.render_env_to_host(ccam, env, params=p)
            assert_same(got, er.frame(chost, ccam, m, p), f"config camera_visible=0 mode={mode}")
    dev.close()


# the restatement's ratio at this size (48 x 32, 16 spp against 8192, the seeds are fixed)
SUN_MSE_RATIO_RESTATEMENT = 0.00244964


@pytest.mark.gpu
def test_quality_at_equal_samples():
    """The sun-and-sky map over the three-ball scene at equal samples: luminance MSE of mode 1 over mode 0 at 16 spp, against a mode-1
    frame at 8192 spp from a disjoint sample range.  The frames are bit-identical to the restatement's, so the ratio is the
    restatement's: 0.00245 (MSE 5.94 against 2423; mode 2: 5.94 as well).  What is left of mode 1's error sits in
    the few pixels that see the sun mirrored in the METAL ball's specular lobe, which only the path can find."""
    rb.amd_lib().rt_set_device(0)
    host, cam = quality_scene()
    m = er.sun_and_sky(256)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(m) as env:
        truth_fb, _ = dev.render_env_to_host(cam, env, params=dict(mode=1))
        assert_same(truth_fb, er.frame(host, cam, m, dict(mode=1)), "the 8192 spp frame")
        truth = truth_fb.astype(np.float64) / cam.samples_per_pixel @ LUM
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = 16
        mse = {}
        for mode in (0, 1):
            fb, _ = dev.render_env_to_host(c, env, params=dict(mode=mode), sample_first=1 << 24)
            assert_same(fb, er.frame(host, c, m, dict(mode=mode), sample_first=1 << 24), f"mode {mode} at 16 spp")
            mse[mode] = float(((fb.astype(np.float64) / 16 @ LUM - truth) ** 2).mean())
    ratio = mse[1] / mse[0]
    print(f"sun-and-sky MSE ratio mode 1 / mode 0 at 16 spp: {ratio:.6g}")
    assert ratio < 1.0
    assert abs(ratio / SUN_MSE_RATIO_RESTATEMENT - 1) < 1e-4, ratio
    dev.close()


@pytest.mark.gpu
def test_handle_state_streams_and_sharing():
    import torch
    rb.amd_lib().rt_set_device(0)
    m = er.sun_and_sky(256)
    env = rb.Env(m)
    host = night_rtiow()
    cam = night_camera(128, 72, 8)
    dev = rb.DeviceScene(host, device=0)
    first, _ = dev.render_to_host(cam)
    before = dev.last_timing()
    lit, _ = dev.render_env_to_host(cam, env)
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    again, _ = dev.render_to_host(cam)
    assert_same(again, first, "rt_render after rt_render_env")
    # a fresh handle's rt_render equals that of a handle that rendered the environment first
    fresh = rb.DeviceScene(host, device=0)
    fresh.render_env_to_host(cam, env)
    assert_same(fresh.render_to_host(cam)[0], first, "a fresh handle's rt_render after rt_render_env")
    # one environment, two scenes, two side streams, sync = 0
    host2, cam2 = three_ball_scene(spp=8)
    cam2 = rb.make_camera(128, 72, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), 8, 6)
    dev2 = rb.DeviceScene(host2, device=0)
    lit2, _ = dev2.render_env_to_host(cam2, env)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fb1 = torch.full((72, 128, 3), float("nan"), device="cuda:0")
    fb2 = torch.full((72, 128, 3), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        dev.render_env(cam, env, fb1.data_ptr(), stream=s1.cuda_stream, sync=False)
    with torch.cuda.stream(s2):
        dev2.render_env(cam2, env, fb2.data_ptr(), stream=s2.cuda_stream, sync=False)
    s1.synchronize()
    s2.synchronize()
    assert_same(fb1.cpu().numpy(), lit, "scene 1 on its stream")
    assert_same(fb2.cpu().numpy(), lit2, "scene 2 on its stream")
    assert_same(lit2, er.frame(host2, cam2, m), "scene 2 against the restatement")
    # shards assemble to the whole frame
    rows = np.zeros_like(lit)
    for part in range(3):
        sh = rb.Shard(5, 3, part)
        got, _ = dev.render_env_to_host(cam, env, shard=sh)
        rows[er.image_rows(cam, sh)] = got
    assert_same(rows, lit, "shards")
    # destroy order: a scene before the environment it used, and the environment before another scene that used it
    dev.close()
    fresh.close()
    env.close()
    assert_same(dev2.render_to_host(cam2)[0], dev2.render_to_host(cam2)[0], "the second scene lives on")
    dev2.close()
    env.close()       # (closing twice is harmless)


@pytest.mark.gpu
def test_cli_env_frames_are_the_python_paths(test_config_text, tmp_path):
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    # a lat-long sky with a bright patch, as a Radiance file and as a PFM
    v, u = np.meshgrid((np.arange(32) + 0.5) / 32, (np.arange(64) + 0.5) / 64, indexing="ij")
    img = np.stack([0.4 + 0.3 * u, 0.5 + 0.4 * (1 - v), 0.9 - 0.5 * v], -1).astype(np.float32)
    img[6:9, 20:24] += 400.0
    write_hdr(str(tmp_path / "sky.hdr"), img, rle=True)
    write_pfm(str(tmp_path / "sky.pfm"), img, little=False)
    for file, extra, params in (("sky.hdr:64", ["--env-up", "z", "--aov", "--denoise"], dict(mode=1, rot=er.Z_UP)),
                                ("sky.pfm:32", ["--env-mode", "light", "--env-scale", "0.5"], dict(mode=2, scale=0.5)),
                                ("sky.pfm:32", ["--env-mode", "path", "--env-up", "y"], dict(mode=0))):
        for f in tmp_path.glob("f_0*"):
            f.unlink()
        out = subprocess.run([EXE, "--gpu", "--env", str(tmp_path / file), *extra], input=text, capture_output=True, text=True, timeout=200)
        assert out.returncode == 0, out.stderr
        host = rb.HostScene.from_config(text)
        info = host.info
        dev = rb.DeviceScene(host, device=0)
        cam = host.frame_camera(0)
        name, n = file.split(":")
        with rb.Env.from_equirect(rb.load_hdr_image(str(tmp_path / name)), int(n)) as env:
            fb, _ = dev.render_env_to_host(cam, env, params=params)
        want = rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp)
        assert open(tmp_path / "f_0.png", "rb").read() == want, (file, extra)
        if "--aov" in extra:
            assert os.path.getsize(tmp_path / "f_0.png.aov") > 12 and os.path.getsize(tmp_path / "f_0.png.denoised") > 8
        dev.close()
