"""rt_render_nee / rt_nee_light_table / rt_trace_samples_nee: next-event estimation with MIS (include/rtp_amd.h).

The header fixes the light sample, the second RNG stream and both MIS weights in float32 order; tests/cpu_native/nee_ref.c restates
them on the oracle (nee_reference.py) and the table, probed samples and frames must equal it bit for bit.  Where no diffuse event takes
a light sample the call is rt_render_samples.  On the CPU: the ABI, every argument check, the CLI refusals, the restatement's scale
(an analytic case) and its expectation (against the oracle's ray_color, by z-scores)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nee_reference as nr
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, INVALID = 0, 1
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_LIGHT = 0, 1, 2, 3


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
    """rtiow with every eighth small sphere made DIFFUSE_LIGHT (two powers), for a black background."""
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


def night_camera(w, h, spp, max_depth=50):
    return rb.make_camera(w, h, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), spp, max_depth)


def two_light_scene():
    """LAMBERTIAN floor sphere, a METAL and a LAMBERTIAN ball, two emitters of different size and power; black background."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_METAL, (0.8, 0.7, 0.5), fuzz=0.4),
            material(MAT_LAMBERTIAN, (0.3, 0.5, 0.8)), material(MAT_LIGHT, emit=(8, 6, 4)), material(MAT_LIGHT, emit=(1, 2, 3))]
    sph = np.array([[0, -100, 0, 100, 0], [-1.1, 1, 0, 1, 1], [1.1, 1, 0, 1, 2], [0, 4, -1.5, 0.5, 3], [2.5, 0.6, 2, 0.6, 4]], np.float32)
    cam = rb.make_camera(8, 8, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), 8192, 6)
    return rb.HostScene.from_arrays(sph, np.zeros((0, 11), np.float32), mats), cam


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_mirrors_symbols_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_nee_params_init", "rt_render_nee", "rt_nee_light_table", "rt_trace_samples_nee"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert C.sizeof(rb.NeeParams) == 16
    assert len(lib.rt_render_nee.argtypes) == 9 and len(lib.rt_trace_samples_nee.argtypes) == 9
    assert len(lib.rt_nee_light_table.argtypes) == 6
    p = rb.nee_params()
    assert (p.struct_bytes, p.mis, p.reserved[0], p.reserved[1]) == (16, 1, 0, 0)
    assert rb.nee_params(mis=0).mis == 0
    with pytest.raises(rb.RtError):
        rb.nee_params(lens_radius=1.0)
    for name in ("render_nee", "render_nee_to_host", "trace_samples_nee", "nee_light_table"):
        assert hasattr(rb.DeviceScene, name)


def test_argument_checks_come_first():
    """Bad parameters are refused by both calls before the scene is looked at; good ones reach the scene check (null here)."""
    lib = rb.amd_lib()
    cam = rb.rtiow_camera(8, 4, 2)
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()

    def calls(p):
        pp = C.byref(p) if p is not None else None
        out = [lib.rt_render_nee(None, C.byref(cam), pp, None, 0, C.c_void_p(1 << 32), None, 1, None)]
        out.append(lib.rt_get_last_error_string().decode())
        out.append(lib.rt_trace_samples_nee(None, C.byref(cam), pp, 1, ijs, f, r, s, s))
        out.append(lib.rt_get_last_error_string().decode())
        return out
    for mis in (-1, 2, 7):
        st1, m1, st2, m2 = calls(rb.nee_params(mis=mis))
        assert st1 == INVALID and "mis" in m1 and st2 == INVALID and "mis" in m2, (mis, m1, m2)
    short = rb.nee_params()
    short.struct_bytes = 4
    st1, m1, st2, m2 = calls(short)
    assert st1 == INVALID and "struct_bytes" in m1 and st2 == INVALID and "struct_bytes" in m2
    for p in (None, rb.nee_params(), rb.nee_params(mis=0)):
        st1, m1, st2, m2 = calls(p)
        assert st1 == INVALID and "null scene" in m1, m1
        assert st2 == INVALID, m2
    # an older caller's 8-byte struct: mis is read, the rest keeps its defaults
    p = rb.nee_params(mis=5)
    p.struct_bytes = 8
    assert calls(p)[0] == INVALID and "mis" in calls(p)[1]
    n = C.c_int32()
    assert lib.rt_nee_light_table(None, 0, None, None, None, C.byref(n)) == INVALID
    assert lib.rt_trace_samples_nee(None, C.byref(cam), None, -1, None, None, None, None, None) == INVALID


def test_cli_refusals(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    for args, env in ((["--nee", "--lens", "0.1:10"], {}), (["--nee", "light", "--motion-blur", "0.5"], {}), (["--nee", "--adaptive", "0.1"], {}),
                      (["--nee", "--denoise-temporal"], {}), (["--nee", "mis", "--devices", "2"], {}), (["--nee", "--shard", "2"], {}),
                      (["--nee"], {"RTP_DEVICES": "2"}), (["--nee", "both"], {}), (["--nee", "--aov", "--devices", "1"], {})):
        r = subprocess.run([exe, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60,
                           env={**os.environ, **env})
        assert r.returncode == 99 and "--nee" in r.stderr, (args, env, r.returncode, r.stderr)
        assert not os.listdir(tmp_path), (args, os.listdir(tmp_path))


def test_reference_empty_table_is_the_oracles(test_config_text):
    """Without emitters no light sample is drawn: the restatement is orc_render bit for bit, in both modes."""
    import oracle_bindings as ob
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(40, 24, 3)
    assert nr.table(host)[0].size == 0
    want = ob.render(host, cam, threads=8)
    for mis in (1, 0):
        assert_same(nr.frame(host, cam, mis, threads=8), want, f"rtiow mis={mis}")
    assert_same(nr.frame(host, cam, nr.PLAIN, threads=8), want, "plain")


def test_reference_table_of_the_config_scene(test_config_text):
    host = config_host(test_config_text)
    idx, cdf, pmf = nr.table(host)
    d = host.desc
    lit = [i for i in range(d.num_spheres) if d.spheres[i].radius > 0 and max(d.materials[d.spheres[i].material_idx].emit.e) > 0]
    assert list(idx) == lit and len(lit) >= 94
    assert cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all()
    assert_same(pmf, np.diff(np.concatenate([[np.float32(0)], cdf])).astype(np.float32), "pmf = cdf difference")
    w = np.array([sum(d.materials[d.spheres[i].material_idx].emit.e) * d.spheres[i].radius ** 2 for i in lit])
    assert np.allclose(pmf, w / w.sum(), rtol=1e-5, atol=1e-7)


def test_reference_analytic_scale():
    """One emitter fully above a large LAMBERTIAN quad, black background, max_depth 2, light sampling alone: a camera sample whose
    first hit is the quad returns a * L * (1 - sqrt(1 - r^2 / |c - x|^2)), the radiance of a uniform cone over the hemisphere density."""
    c, r, L, a = np.array([0.0, 2.5, 0.0]), 1.5, np.array([4.0, 2.0, 1.0]), np.array([0.6, 0.5, 0.4])
    mats = [material(MAT_LAMBERTIAN, tuple(a)), material(MAT_LIGHT, emit=tuple(L))]
    quad = np.array([[-3, 0, 3, 6, 0, 0, 0, 0, -6, 0, 0]], np.float32)       # base, u, v, material, type: normal +y
    host = rb.HostScene.from_arrays(np.array([[*c, r, 1]], np.float32), quad, mats)
    cam = rb.make_camera(48, 32, 60.0, (0, 7, 7), (0, 0, 0), (0, 0, 0), 8, 2)
    n = 48 * 32 * 8
    ii, jj, ss = np.meshgrid(np.arange(48), np.arange(32), np.arange(8), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], 1).astype(np.int32)
    rad, rays, _, _ = nr.trace(host, cam, ijs, mis=0)
    import lens_reference as lr
    o, d, _, _, _ = lr.rays(cam, None, 0.0, 10.0, ijs)
    o, d = o.astype(np.float64), d.astype(np.float64)
    t = -o[:, 1] / d[:, 1]
    x = o + t[:, None] * d
    on_quad = (t > 0) & (np.abs(x[:, 0]) < 2.9) & (np.abs(x[:, 2]) < 2.9)
    oc = o - c                                                      # … and the camera ray does not meet the sphere first
    b = (oc * d).sum(1)
    disc = b * b - (d * d).sum(1) * ((oc * oc).sum(1) - r * r)
    on_quad &= disc < 0
    assert on_quad.sum() > n // 10
    d2 = ((c - x) ** 2).sum(1)
    want = a[None, :] * L[None, :] * (1 - np.sqrt(1 - r * r / d2))[:, None]
    got = rad.astype(np.float64)
    lit = on_quad & (got.max(1) > 0)
    assert lit.sum() >= on_quad.sum() - 2, (lit.sum(), on_quad.sum())       # (a shadow ray may graze past the sphere's rim)
    assert (np.abs(got[lit] - want[lit]) <= 1e-5 * want[lit]).all(), np.abs(got[lit] / want[lit] - 1).max()
    assert (rays[lit] == 3).all()         # camera ray, shadow ray, BSDF ray


def _zscores(m_a, m_b, spp):
    """Per-pixel luminance z-scores of two estimators from their per-pixel channel sums and sums of squares."""
    lum = np.array([0.2126, 0.7152, 0.0722])

    def stats(m):
        mean = m[..., :3] / spp
        ex2 = m[..., 3:] / spp
        var = np.maximum(ex2 - mean * mean, 0) * spp / (spp - 1)
        return mean @ lum, var @ (lum * lum)       # (channels treated as independent: a conservative-enough bound for a z-test)
    ma, va = stats(m_a)
    mb, vb = stats(m_b)
    return (ma - mb) / np.sqrt((va + vb) / spp + 1e-30)


def test_reference_is_unbiased_against_the_oracle():
    """8 x 8 pixels x 8192 samples of each estimator from disjoint sample ranges: the luminance means of every 2 x 2 block of pixels
    agree within 5 sigma, and the whole image's within 4.  (Blocks, not single pixels: where a pixel sees a small emitter only through
    rare BSDF hits, the plain estimator's sample variance misses the fireflies it has not drawn yet.)"""
    host, cam = two_light_scene()
    spp = cam.samples_per_pixel
    _, plain = nr.frame(host, cam, nr.PLAIN, sample_first=0, moments=True)
    _, mis = nr.frame(host, cam, 1, sample_first=spp, moments=True)
    _, light = nr.frame(host, cam, 0, sample_first=2 * spp, moments=True)

    def blocks(m):
        return m.reshape(4, 2, 4, 2, 6).sum((1, 3))
    for name, a, b in (("mis/plain", mis, plain), ("light/plain", light, plain), ("mis/light", mis, light)):
        z = _zscores(blocks(a), blocks(b), spp * 4)
        assert np.abs(z).max() < 5.0, (name, np.abs(z).max())
        za = _zscores(a.sum((0, 1)), b.sum((0, 1)), spp * 64)
        assert abs(za) < 4.0, (name, za)
    # … and NEE is the better estimator here: the median pixel's per-sample variance is less than half the plain estimator's
    lum = np.array([0.2126, 0.7152, 0.0722])

    def var(m):
        mean = m[..., :3] / spp
        return ((m[..., 3:] / spp - mean * mean) @ lum).ravel()
    seen = var(plain) > 0
    assert np.median(var(mis)[seen] / var(plain)[seen]) < 0.5


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_light_tables_equal_the_reference(test_config_text):
    rb.amd_lib().rt_set_device(0)
    for name, host in (("config", config_host(test_config_text)), ("night rtiow", night_rtiow()), ("rtiow", rb.HostScene.rtiow())):
        dev = rb.DeviceScene(host, device=0)
        got = dev.nee_light_table()
        want = nr.table(host)
        for g, w, what in zip(got, want, ("index", "cdf", "pmf")):
            assert_same(g, w, f"{name} {what}")
        assert (got[0].size == 0) == (name == "rtiow")
        dev.close()


@pytest.mark.gpu
def test_probe_samples_equal_the_reference(test_config_text):
    rb.amd_lib().rt_set_device(0)
    rng = np.random.default_rng(3)
    n = 10000
    for name, host, cam in (("config", config_host(test_config_text), None), ("night rtiow", night_rtiow(), night_camera(320, 180, 1))):
        if cam is None:
            cam = host.frame_camera(5)
        dev = rb.DeviceScene(host, device=0)
        ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)
        for mis in (1, 0):
            got = dev.trace_samples_nee(cam, ijs, params={"mis": mis})
            want = nr.trace(host, cam, ijs, mis=mis)
            for g, w, what in zip(got, want, ("radiance", "rays", "seed", "nee seed")):
                assert_same(g, w, f"{name} mis={mis} {what}")
            # light samples were taken, and the path's own stream is rt_trace_samples's
            assert (got[1] > dev.trace_samples(cam, ijs)[1]).mean() > 0.02
            assert_same(got[2], dev.trace_samples(cam, ijs)[2], f"{name} path seeds")
        dev.close()


@pytest.mark.gpu
def test_frames_equal_the_reference(test_config_text):
    rb.amd_lib().rt_set_device(0)
    host = night_rtiow()
    dev = rb.DeviceScene(host, device=0)
    for mis in (1, 0):
        cam = night_camera(96, 64, 8)
        got, t = dev.render_nee_to_host(cam, params={"mis": mis})
        assert_same(got, nr.frame(host, cam, mis), f"night rtiow mis={mis}")
        assert t.trace_launches >= 1 and t.guarded == 0
    dev.close()
    host = config_host(test_config_text)
    dev = rb.DeviceScene(host, device=0)
    shard = rb.Shard(4, 3, 2)
    for mis in (1, 0):
        for depth in (2, 50):
            cam = rb.CameraData.from_buffer_copy(host.frame_camera(11))
            cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth = 96, 64, 4, depth
            for sh, first in ((None, 0), (shard, 0), (None, 37)):
                got, _ = dev.render_nee_to_host(cam, params={"mis": mis}, shard=sh, sample_first=first)
                want = nr.frame(host, cam, mis, shard=sh, sample_first=first)
                assert_same(got, want, f"config mis={mis} depth={depth} shard={sh is not None} first={first}")
    dev.close()


@pytest.mark.gpu
def test_identity_where_no_light_sample_is_drawn():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(160, 90, 8)
    for config in (dict(), dict(traversal=rb.TRAVERSAL_EXACT)):
        dev = rb.DeviceScene(host, device=0, **config)
        for first in (0, 5):
            want, _ = dev.render_to_host(cam, sample_first=first)
            for mis in (1, 0):
                got, _ = dev.render_nee_to_host(cam, params={"mis": mis}, sample_first=first)
                assert_same(got, want, f"rtiow {config} mis={mis} first={first}")
        dev.close()
    # an emitter, and every other surface DIELECTRIC: the table is not empty (the NEE kernel runs) but no event is diffuse
    mats = [material(MAT_DIELECTRIC, ir=1.5), material(MAT_DIELECTRIC, ir=1.33), material(MAT_LIGHT, emit=(5, 5, 5))]
    sph = np.array([[0, -100, 0, 100, 0], [0, 1, 0, 1, 1], [1.5, 0.5, 1, 0.5, 0], [0, 4, 0, 1, 2]], np.float32)
    glass = rb.HostScene.from_arrays(sph, np.zeros((0, 11), np.float32), mats)
    cam = rb.make_camera(96, 64, 40.0, (0, 2, 8), (0, 1, 0), (0.1, 0.1, 0.2), 16, 20)
    dev = rb.DeviceScene(glass, device=0)
    assert dev.nee_light_table()[0].tolist() == [3]
    want, _ = dev.render_to_host(cam)
    for mis in (1, 0):
        got, t = dev.render_nee_to_host(cam, params={"mis": mis})
        assert_same(got, want, f"all-glass mis={mis}")
        assert t.workgroup_size == 256        # (the NEE kernel's block: it ran)
    dev.close()


def _batch_block_means(render, cam, batches, spp, block=8):
    """batches x (H / block) x (W / block) luminance means of independent batches of spp samples (disjoint sample ranges)."""
    lum = np.array([0.2126, 0.7152, 0.0722])
    out = []
    for b in range(batches):
        fb = render(b * spp).astype(np.float64) / spp @ lum
        h, w = fb.shape
        out.append(fb.reshape(h // block, block, w // block, block).mean((1, 3)))
    return np.array(out)


@pytest.mark.gpu
def test_unbiased_against_rt_render(test_config_text):
    """Per 8 x 8 block, the means of rt_render and of rt_render_nee in both modes agree within 5 sigma (sigma from the spread of 16
    independent batches of each, with a floor of 1e-3 of the image's mean)."""
    rb.amd_lib().rt_set_device(0)
    batches, spp = 16, 256
    chost = config_host(test_config_text)
    ccam = rb.CameraData.from_buffer_copy(chost.frame_camera(3))
    ccam.image_width, ccam.image_height, ccam.samples_per_pixel = 96, 64, spp
    for name, host, cam in (("config", chost, ccam), ("night rtiow", night_rtiow(), night_camera(96, 64, spp))):
        dev = rb.DeviceScene(host, device=0)
        offset = {"plain": 0, 1: 1 << 20, 0: 2 << 20}
        means = {}
        for mode in ("plain", 1, 0):
            if mode == "plain":
                fn = lambda first: dev.render_to_host(cam, sample_first=offset["plain"] + first)[0]
            else:
                fn = lambda first, m=mode: dev.render_nee_to_host(cam, params={"mis": m}, sample_first=offset[m] + first)[0]
            means[mode] = _batch_block_means(fn, cam, batches, spp)
        for a, b in ((1, "plain"), (0, "plain"), (1, 0)):
            ma, mb = means[a].mean(0), means[b].mean(0)
            va, vb = means[a].var(0, ddof=1) / batches, means[b].var(0, ddof=1) / batches
            # (a floor of 1e-3 of the image's mean: in a near-black block the plain estimator's batches may not have drawn the rare
            # fireflies yet, and its spread then understates its variance — tests/cpu_native restatement, 16384 spp: 1.5 sigma)
            floor = 1e-3 * means["plain"].mean()
            z = (ma - mb) / np.sqrt(va + vb + floor * floor)
            assert np.abs(z).max() < 5.0, (name, a, b, np.abs(z).max())
        dev.close()


def _mse_ratio(dev, cam, spp, truth):
    lum = np.array([0.2126, 0.7152, 0.0722])
    c = rb.CameraData.from_buffer_copy(cam)
    c.samples_per_pixel = spp
    plain = dev.render_to_host(c, sample_first=1 << 24)[0].astype(np.float64) / spp @ lum
    nee = dev.render_nee_to_host(c, sample_first=1 << 24)[0].astype(np.float64) / spp @ lum
    return float(((nee - truth) ** 2).mean() / ((plain - truth) ** 2).mean())


# measured at 16 spp against 8192 (0.8184, the seeds are fixed); pinned with a 10 % margin
NIGHT_RTIOW_MSE_RATIO = 0.8184


@pytest.mark.gpu
def test_quality_at_equal_samples():
    """Night rtiow at equal samples: the MIS estimator's MSE against a high-spp ground truth (a disjoint sample range) beats
    rt_render's outright, by the measured margin."""
    rb.amd_lib().rt_set_device(0)
    host = night_rtiow()
    cam = night_camera(192, 108, 8192)
    dev = rb.DeviceScene(host, device=0)
    lum = np.array([0.2126, 0.7152, 0.0722])
    truth = dev.render_nee_to_host(cam)[0].astype(np.float64) / cam.samples_per_pixel @ lum
    ratio = _mse_ratio(dev, cam, 16, truth)
    print(f"night rtiow MSE ratio nee/plain at 16 spp: {ratio:.4f}")
    assert ratio < 1.0
    assert ratio < 1.1 * NIGHT_RTIOW_MSE_RATIO, ratio
    dev.close()


@pytest.mark.gpu
def test_handle_state_and_streams():
    import torch
    rb.amd_lib().rt_set_device(0)
    host = night_rtiow()
    cam = night_camera(128, 72, 8)
    dev = rb.DeviceScene(host, device=0)
    first, _ = dev.render_to_host(cam)
    before = dev.last_timing()
    nee, _ = dev.render_nee_to_host(cam)
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    again, _ = dev.render_to_host(cam)
    assert_same(again, first, "rt_render after rt_render_nee")
    # sync = 0 on a side stream
    s = torch.cuda.Stream()
    fb = torch.full((72, 128, 3), float("nan"), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dev.render_nee(cam, fb.data_ptr(), stream=s.cuda_stream, sync=False)
    s.synchronize()
    assert_same(fb.cpu().numpy(), nee, "sync = 0 on a side stream")
    # shards assemble to the whole frame
    rows = np.zeros_like(nee)
    for part in range(3):
        sh = rb.Shard(5, 3, part)
        got, _ = dev.render_nee_to_host(cam, shard=sh)
        rows[nr.image_rows(cam, sh)] = got
    assert_same(rows, nee, "shards")
    dev.close()


@pytest.mark.gpu
def test_cli_nee_frames_are_the_python_paths(test_config_text, tmp_path):
    exe = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    for mode, mis in (("light", 0), (None, 1)):
        args = ["--nee"] + ([mode] if mode else []) + ["--aov", "--denoise"]
        out = subprocess.run([exe, "--gpu", *args], input=text, capture_output=True, text=True, timeout=200)
        assert out.returncode == 0, out.stderr
        host = rb.HostScene.from_config(text)
        info = host.info
        dev = rb.DeviceScene(host, device=0)
        cam = host.frame_camera(0)
        fb, _ = dev.render_nee_to_host(cam, params={"mis": mis})
        want = rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp)
        assert open(tmp_path / "f_0.png", "rb").read() == want, mode
        assert os.path.getsize(tmp_path / "f_0.png.aov") > 12 and os.path.getsize(tmp_path / "f_0.png.denoised") > 8
        dev.close()
