"""rt_nee_params.select = 1: the light tree — the emitter of a light sample picked by where the shaded point is (include/rtp_amd.h,
DESIGN.md §18).

The header fixes the tree's build (in double, on the host), the descent and the path product in float32 order;
tests/cpu_native/tree_ref.c restates rt_render_lit with them on the oracle (tree_reference.py), and the tree, probed samples and frames
of the device must equal it bit for bit.  On the CPU: the ABI and every refusal, the restatement's tree against an independent numpy
build, its pmf (sums and pick frequencies), its identities, its expectation (against the oracle's ray_color, by z-scores) and what it
gains at equal samples."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import emit_reference as emr
import env_reference as er
import nee_reference as nr
import rtp_bindings as rb
import tree_reference as tr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
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


def material(kind, albedo=(0.5, 0.5, 0.5), emit=(0, 0, 0), fuzz=0.0, ir=1.5):
    m = rb.Material()
    m.type = kind
    m.fuzz = fuzz
    m.ir = ir
    for k in range(3):
        m.albedo.e[k] = albedo[k]
        m.emit.e[k] = emit[k]
    return m


# ---- the scenes --------------------------------------------------------------------------------------------------------------------
def night_rtiow():
    """rtiow with every eighth small sphere made DIFFUSE_LIGHT (test_nee_planes.py's)."""
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


FLOOR, WALL, PANEL, DISC, TRI, HIDDEN, OCCLUDER, GLOW = range(8)
PANEL_BOX_PLANES = np.array([
    [-6, 0, 6, 12, 0, 0, 0, 0, -12, 0, QUAD],                # LAMBERTIAN floor, normal +y
    [-6, 0, -4, 12, 0, 0, 0, 4.3, 0, 1, QUAD],               # LAMBERTIAN back wall, normal +z
    [-2, 5, 1.5, 4, 0, 0, 0, 0, -3, 5, QUAD],                # the ceiling panel
    [1.5, 1.2, -3.9, 3, 0, 0, 0, 2.6, 0, 6, ELLIPSE],        # an ellipse light in front of the wall
    [-4.5, 0, 0.5, 1.6, 0, 1.6, 0, 2.8, 0, 7, TRIANGLE],     # a triangle light standing on the floor
    [3, 4.5, -1, 2, 0, 0, 0, 0, -2, 9, QUAD],                # a panel no scattering surface can see: the occluder lies just below it
    [2.5, 4.4, -0.5, 3, 0, 0, 0, 0, -3, 10, QUAD],           # … the occluder
    [-1.2, 0.01, 5, 2.4, 0, 0, 0, 0, -1.6, 11, QUAD],        # a LAMBERTIAN quad that emits
], np.float32)
PANEL_BOX_SPHERES = np.array([[-1.6, 1, 0, 1, 2], [1.6, 1, -0.5, 1, 3], [0, 0.6, 2.2, 0.6, 4], [3.6, 0.5, 2, 0.5, 8]], np.float32)


def panel_box():
    """test_nee_planes.py's: a floor and a back wall, three balls and six emitters — a sphere and five planes of all three types."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_LAMBERTIAN, (0.7, 0.5, 0.4)), material(MAT_LAMBERTIAN, (0.3, 0.5, 0.8)),
            material(MAT_METAL, (0.8, 0.7, 0.5), fuzz=0.4), material(MAT_DIELECTRIC, ir=1.5), material(MAT_LIGHT, emit=(6, 5, 4)),
            material(MAT_LIGHT, emit=(2, 3, 4)), material(MAT_LIGHT, emit=(4, 2, 3)), material(MAT_LIGHT, emit=(5, 5, 3)),
            material(MAT_LIGHT, emit=(3, 3, 3)), material(MAT_LAMBERTIAN, (0.5, 0.5, 0.5)),
            material(MAT_LAMBERTIAN, (0.5, 0.4, 0.3), emit=(0.8, 1.0, 0.6))]
    return rb.HostScene.from_arrays(PANEL_BOX_SPHERES, PANEL_BOX_PLANES, mats)


def box_camera(w, h, spp, depth=50):
    return rb.make_camera(w, h, 50.0, (0, 3, 10), (0, 1.8, 0), (0, 0, 0), spp, depth)


def ball_camera(w, h, spp, depth=50):
    return rb.make_camera(w, h, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), spp, depth)


def lamp_scene():
    """test_lit.py's lamp scene: a LAMBERTIAN floor sphere, a METAL and a LAMBERTIAN ball and one DIFFUSE_LIGHT sphere — one table entry."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_METAL, (0.8, 0.7, 0.5), fuzz=0.4), material(MAT_LAMBERTIAN, (0.3, 0.5, 0.8)),
            material(MAT_LIGHT, emit=(8.0, 6.0, 4.0))]
    sph = [[0, -100, 0, 100, 0], [-1.1, 1, 0, 1, 1], [1.1, 1, 0, 1, 2], [0, 2.6, 0.5, 0.3, 3]]
    return rb.HostScene.from_arrays(np.array(sph, np.float32), np.zeros((0, 11), np.float32), mats)


def three_lamps():
    """The lamp scene with three emissive spheres, two of them concentric (the smaller one inside the larger): an odd split, and a node
    whose centres coincide — no axis extends, so x is taken and the sort keeps list order."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_METAL, (0.8, 0.7, 0.5), fuzz=0.4), material(MAT_LAMBERTIAN, (0.3, 0.5, 0.8)),
            material(MAT_LIGHT, emit=(8.0, 6.0, 4.0)), material(MAT_LIGHT, emit=(1.0, 2.0, 4.0)), material(MAT_LIGHT, emit=(3.0, 5.0, 2.0))]
    sph = [[0, -100, 0, 100, 0], [-1.1, 1, 0, 1, 1], [1.1, 1, 0, 1, 2], [-1.0, 2.6, 0.5, 0.3, 3], [2.2, 1.4, 1.0, 0.25, 5], [-1.0, 2.6, 0.5, 0.15, 4]]
    return rb.HostScene.from_arrays(np.array(sph, np.float32), np.zeros((0, 11), np.float32), mats)


# name → (scene, camera(w, h, spp, depth))
SCENES = {"night rtiow": (night_rtiow, night_camera), "panel box": (panel_box, box_camera), "lamp": (lamp_scene, ball_camera),
          "three lamps": (three_lamps, ball_camera)}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][0]()


def camera(name, w, h, spp, depth=50):
    return SCENES[name][1](w, h, spp, depth)


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


numpy_tree = tr.numpy_tree          # (the independent numpy build lives beside the restatement's binding: test_lit_fuzz.py uses it too)


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------

def test_abi_and_refusals():
    """The symbol and the struct; select outside {0, 1} is refused by all six calls before the scene is looked at, naming the field; a
    12-byte struct does not reach it; mis and sample_planes are still checked first; the lit calls ignore it when they sample no
    emitters."""
    lib = rb.amd_lib()
    assert hasattr(lib, "rt_nee_light_tree") and "rt_nee_light_tree" in rb.RTP_AMD_SYMBOLS
    assert len(lib.rt_nee_light_tree.argtypes) == 14
    assert C.sizeof(rb.NeeParams) == 16
    p = rb.nee_params(select=1)
    assert (p.struct_bytes, p.mis, p.sample_planes, p.select, p.reserved[0], p.reserved[1]) == (16, 1, 0, 1, 0, 1)
    assert rb.nee_params().select == 0 and rb.nee_params().reserved[1] == 0
    assert bytes(p)[12:16] == (1).to_bytes(4, "little")
    assert "select" in rb.NeeParams.FIELDS and hasattr(rb.DeviceScene, "nee_light_tree")
    cam = rb.rtiow_camera(8, 4, 2)
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    n, n2 = C.c_int32(), C.c_int32()

    def calls(p):
        """(status, message) of the six calls with nee parameters p and a null scene."""
        lit = rb.lit_params(nee=p)
        out = []
        for call in (lambda: lib.rt_render_nee(None, C.byref(cam), C.byref(p), None, 0, C.c_void_p(1 << 32), None, 1, None),
                     lambda: lib.rt_trace_samples_nee(None, C.byref(cam), C.byref(p), 1, ijs, f, r, s, s),
                     lambda: lib.rt_nee_emitter_table(None, C.byref(p), 0, None, None, None, None, None, C.byref(n)),
                     lambda: lib.rt_nee_light_tree(None, C.byref(p), 0, 0, *([None] * 8), C.byref(n), C.byref(n2)),
                     lambda: lib.rt_render_lit(None, C.byref(cam), C.byref(lit), None, 0, C.c_void_p(1 << 32), None, 1, None),
                     lambda: lib.rt_trace_samples_lit(None, C.byref(cam), C.byref(lit), 1, ijs, f, r, s, s, s)):
            out.append((call(), lib.rt_get_last_error_string().decode()))
        assert len(out) == 6
        return out
    for bad in (-1, 2):
        for st, msg in calls(rb.nee_params(select=bad)):
            assert st == INVALID and "select" in msg, (bad, msg)
    for good in (0, 1):
        for planes in (0, 1):
            for st, msg in calls(rb.nee_params(select=good, sample_planes=planes)):
                assert st == INVALID and "select" not in msg, (good, msg)
        assert "null scene" in calls(rb.nee_params(select=good))[0][1]
    # an older caller's 12-byte struct: the field behind its end is not read
    old = rb.nee_params(select=2)
    old.struct_bytes = 12
    for st, msg in calls(old):
        assert st == INVALID and "select" not in msg, msg
    # mis and sample_planes are still checked, and first
    assert all("mis" in msg for _, msg in calls(rb.nee_params(mis=3, sample_planes=2, select=2)))
    assert all("sample_planes" in msg for _, msg in calls(rb.nee_params(sample_planes=2, select=2)))
    # the lit calls read the nee parameters only when they sample emitters
    lit = rb.lit_params(emitters=False, nee=rb.nee_params(select=2))
    assert lib.rt_render_lit(None, C.byref(cam), C.byref(lit), None, 0, C.c_void_p(1 << 32), None, 1, None) == INVALID
    assert "null scene" in lib.rt_get_last_error_string().decode()
    assert lib.rt_trace_samples_lit(None, C.byref(cam), C.byref(lit), 1, ijs, f, r, s, s, s) == INVALID
    assert "select" not in lib.rt_get_last_error_string().decode()


def test_cli_refusals(test_config_text, tmp_path):
    """--light-tree needs a call that samples emitters: exit 99, like the neighbouring flags, and nothing written."""
    before = sorted(os.listdir(tmp_path))
    for args in (["--light-tree"], ["--light-tree", "--aov"], ["--light-tree", "--lens", "0.2:12"]):
        r = subprocess.run([EXE, "--gpu", *args], input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert r.returncode == 99 and "--light-tree" in r.stderr, (args, r.returncode, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before


@pytest.mark.parametrize("planes", [0, 1])
@pytest.mark.parametrize("name", list(SCENES))
def test_tree_against_a_numpy_build(name, planes):
    host = scene(name)
    t = tr.tree(host, planes)
    want = numpy_tree(host, planes)
    n = len(want["path"])
    assert n == len(emr.table(host, planes)[0]) == {"night rtiow": 60, "panel box": 6 if planes else 1, "lamp": 1, "three lamps": 3}[name]
    assert len(t["entry"]) == 2 * n - 1 == len(want["entry"])
    for col in ("left", "right", "entry", "path", "depth"):
        assert t[col].tolist() == want[col].tolist(), (name, planes, col)
    assert t["depth"].max() <= int(np.ceil(np.log2(n))) if n > 1 else t["depth"].max() == 0
    # every leaf once, in the order the paths say
    leaves = t["entry"][t["entry"] >= 0]
    assert sorted(leaves.tolist()) == list(range(n))
    for e in range(n):
        node = 0
        for i in range(t["depth"][e]):
            node = (t["right"] if (t["path"][e] >> i) & 1 else t["left"])[node]
        assert t["entry"][node] == e
    # every entry's sphere inside every ancestor's, the root and its own leaf included
    sph = t["sphere"].astype(np.float64)
    for e in range(n):
        node = 0
        for i in range(t["depth"][e] + 1):
            reach = np.linalg.norm(want["c"][e] - sph[node, :3]) + want["rho"][e]
            assert reach <= sph[node, 3] * (1 + 1e-6), (name, planes, e, node, reach, sph[node, 3])
            if i < t["depth"][e]:
                node = (t["right"] if (t["path"][e] >> i) & 1 else t["left"])[node]
    assert np.allclose(sph[:, :3], want["centre"], rtol=1e-6, atol=1e-6)
    assert np.allclose(sph[:, 3], want["radius"], rtol=1e-6, atol=0) and (t["sphere"][:, 3] > want["radius"].astype(np.float32)).all()
    assert np.allclose(t["weight"], want["weight"], rtol=1e-6, atol=0)
    assert np.allclose(t["q"], want["q"], rtol=1e-6, atol=0)
    assert t["weight"][0] == 1.0
    if name == "three lamps":
        # entries: sphere 3 (0), sphere 4 (1), sphere 5 (2, concentric with 0).  The split on x puts the two concentric ones left — the
        # first ceil(3 / 2) — and their node, whose centres coincide, keeps list order
        assert t["entry"].tolist() == [-1, -1, 0, 2, 1] and t["path"].tolist() == [0, 1, 2] and t["depth"].tolist() == [2, 1, 2]


def _points(host, planes, rng, n):
    """n points: on and above the ground, and inside and outside node spheres."""
    t = tr.tree(host, planes)
    ground = np.stack([rng.uniform(-11, 11, n // 2), np.where(rng.random(n // 2) < 0.5, 0.0, rng.uniform(0, 3, n // 2)), rng.uniform(-11, 11, n // 2)], 1)
    k = rng.integers(0, len(t["entry"]), n - n // 2)
    d = rng.normal(size=(n - n // 2, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    near = t["sphere"][k, :3] + d * (t["sphere"][k, 3] * rng.uniform(0, 2, n - n // 2))[:, None]
    inside = (np.linalg.norm(near - t["sphere"][k, :3], axis=1) < t["sphere"][k, 3]).sum()
    assert n // 10 < inside < n - n // 2 - n // 10
    return np.concatenate([ground, near]).astype(np.float32)


def test_pmf_sums_to_one_and_the_pick_follows_it():
    host = scene("night rtiow")
    rng = np.random.default_rng(18)
    pts = _points(host, 0, rng, 1000)
    p = tr.pmf(host, pts).astype(np.float64)
    print("night rtiow: |sum pmf - 1| max", np.abs(p.sum(1) - 1).max(), "smallest pmf", p.min())
    assert np.abs(p.sum(1) - 1).max() < 1e-5
    assert (p >= 0).all()
    draws = 1 << 16
    worst = 0.0
    for k, x in enumerate(pts[[0, 1, 2, 3, 500, 501, 502, 503]]):
        counts, bad = tr.pick_counts(host, x, draws, 0x9E3779B9 + k)
        assert bad == 0, "the descent's p is the path product of its entry, bit for bit"
        q = tr.pmf(host, x[None]).astype(np.float64)[0]
        assert counts.sum() == draws
        sd = np.sqrt(draws * q * (1 - q))
        z = np.abs(counts - draws * q) / np.maximum(sd, 1e-300)
        z[(counts == 0) & (q == 0)] = 0
        worst = max(worst, z.max())
        assert (z < 5).all(), (k, x, np.argmax(z), counts[np.argmax(z)], draws * q[np.argmax(z)])
    print("pick frequencies: largest deviation in binomial standard deviations", worst)
    # the other scenes' sums (the two-kind table, and a tree of one entry: pmf = 1)
    for name, planes in (("panel box", 1), ("three lamps", 0), ("lamp", 0)):
        h = scene(name)
        s = tr.pmf(h, _points(h, planes, rng, 400) if name != "lamp" else pts[:400], planes).astype(np.float64).sum(1)
        assert np.abs(s - 1).max() < 1e-5, (name, np.abs(s - 1).max())
        if name == "lamp":
            assert (s == 1).all()


@pytest.mark.parametrize("depth", [2, 50])
def test_restatement_identities(depth):
    """select = 0 through tree_ref.c is emit_ref.c bit for bit (environment and lens, a shard, sample_first 37) — and select = 1 on rtiow,
    whose table is empty, is rt_render_samples."""
    m = er.sun_and_sky(64)
    shard = rb.Shard(4, 3, 2)
    for name, planes in (("night rtiow", 0), ("panel box", 1), ("three lamps", 0)):
        host, cam = scene(name), camera(name, 32, 24, 4, depth)
        for sh, first in ((None, 0), (shard, 0), (None, 37)):
            for mis in (1, 0):
                kw = dict(lens=LENS, nee_mis=mis, planes=planes, rgb=m, env_params=dict(mode=1, scale=0.75), shard=sh, sample_first=first)
                assert_same(tr.frame(host, cam, select=0, **kw), emr.frame(host, cam, **kw), f"{name} depth={depth} mis={mis} first={first}")
            kw = dict(nee_mis=1, planes=planes, shard=sh, sample_first=first)
            assert_same(tr.frame(host, cam, select=0, **kw), emr.frame(host, cam, **kw), f"{name} depth={depth} pinhole first={first}")
        assert not np.array_equal(tr.frame(host, cam, select=1, planes=planes), tr.frame(host, cam, select=0, planes=planes)), name
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(32, 24, 4, depth)
    assert len(tr.tree(host, 1)["entry"]) == 0
    for sh, first in ((None, 0), (shard, 0), (None, 37)):
        assert_same(tr.frame(host, cam, select=1, planes=1, shard=sh, sample_first=first), nr.frame(host, cam, nr.PLAIN, shard=sh, sample_first=first),
                    f"rtiow depth={depth} first={first}")
    host.close()


# night rtiow from the eye of its other tests: the oracle's ray_color against itself from two sample ranges stays inside the limits there
# (2 x 2 blocks 2.95, image -1.09) — the test repeats that comparison beside the two it is about
UNBIASED = {"night rtiow": dict(planes=0, cam=lambda spp: night_camera(8, 8, spp, 6)),
            "panel box": dict(planes=1, cam=lambda spp: box_camera(8, 8, spp, 6))}


@pytest.mark.parametrize("name", list(UNBIASED))
def test_unbiased_against_the_oracle(name):
    """8 x 8 pixels x 8192 samples of each estimator from disjoint sample ranges (test_nee_planes.py's protocol and bounds): the
    luminance means of every 2 x 2 block agree within 5 sigma and the whole image's within 4 — the tree with MIS against the oracle's
    ray_color, and the tree sampled alone against the tree with MIS."""
    host = scene(name)
    planes = UNBIASED[name]["planes"]
    spp = 8192
    cam = UNBIASED[name]["cam"](spp)
    _, plain = nr.frame(host, cam, nr.PLAIN, sample_first=0, moments=True)
    _, mis = tr.frame(host, cam, select=1, nee_mis=1, planes=planes, sample_first=spp, moments=True)
    _, light = tr.frame(host, cam, select=1, nee_mis=0, planes=planes, sample_first=2 * spp, moments=True)
    _, plain2 = nr.frame(host, cam, nr.PLAIN, sample_first=3 * spp, moments=True)

    def blocks(m):
        return m.reshape(4, 2, 4, 2, 6).sum((1, 3))
    for what, x, y in (("plain/plain", plain2, plain), ("mis/plain", mis, plain), ("light/mis", light, mis)):
        z = _zscores(blocks(x), blocks(y), spp * 4)
        za = _zscores(x.sum((0, 1)), y.sum((0, 1)), spp * 64)
        print(f"{name} {what}: 2 x 2 blocks max |z| {np.abs(z).max():.3f}, image z {float(za):.3f}")
        assert np.abs(z).max() < 5.0, (name, what, np.abs(z).max())
        assert abs(za) < 4.0, (name, what, za)


# measured on the restatement, whose bits are the device's: luminance MSE of select = 1 over select = 0 at 16 spp, 48 x 32,
# against select = 1 at 8192 spp from a disjoint sample range
NIGHT_RTIOW_MSE_RATIO = 0.937854
PANEL_BOX_MSE_RATIO = 0.917068


def _mse_ratio(name, planes):
    host = scene(name)
    truth = tr.frame(host, camera(name, 48, 32, 8192), select=1, planes=planes, sample_first=1 << 20).astype(np.float64) / 8192 @ LUM
    cam = camera(name, 48, 32, 16)
    tree = tr.frame(host, cam, select=1, planes=planes).astype(np.float64) / 16 @ LUM
    table = tr.frame(host, cam, select=0, planes=planes).astype(np.float64) / 16 @ LUM
    ratio = float(((tree - truth) ** 2).mean() / ((table - truth) ** 2).mean())
    print(f"{name} MSE ratio select 1 / 0 at 16 spp: {ratio:.6f}")
    return ratio


def test_quality_at_equal_samples_night_rtiow():
    ratio = _mse_ratio("night rtiow", 0)
    assert ratio < 1.0, ratio
    assert abs(ratio - NIGHT_RTIOW_MSE_RATIO) <= 1e-4 * NIGHT_RTIOW_MSE_RATIO, ratio


def test_quality_at_equal_samples_panel_box():
    """(few lights, all close: reported and pinned, no inequality)"""
    ratio = _mse_ratio("panel box", 1)
    assert abs(ratio - PANEL_BOX_MSE_RATIO) <= 1e-4 * PANEL_BOX_MSE_RATIO, ratio


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
PROBE_SIZE = (160, 120)


@functools.lru_cache(maxsize=None)
def _probe_set():
    rng = np.random.default_rng(18)
    n = 4000
    return np.stack([rng.integers(0, PROBE_SIZE[0], n), rng.integers(0, PROBE_SIZE[1], n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _want_probe(name, planes, mis, depth):
    return tr.trace(scene(name), camera(name, *PROBE_SIZE, 1, depth), _probe_set(), select=1, nee_mis=mis, planes=planes, stats=True)


@functools.lru_cache(maxsize=None)
def _want_frame(name, planes, mis, depth, sharded, first):
    return tr.frame(scene(name), camera(name, 64, 48, 4, depth), select=1, nee_mis=mis, planes=planes, shard=rb.Shard(4, 3, 2) if sharded else None,
                    sample_first=first)


@pytest.mark.gpu
def test_trees_equal_the_restatement():
    rb.amd_lib().rt_set_device(0)
    for name in SCENES:
        dev = rb.DeviceScene(scene(name), device=0)
        for planes in (1, 0):
            got = dev.nee_light_tree({"sample_planes": planes, "select": 1})
            want = tr.tree(scene(name), planes)
            for col in tr.COLUMNS:
                assert_same(got[col], want[col], f"{name} sample_planes={planes} {col}")
        assert_same(dev.nee_light_tree()["entry"], tr.tree(scene(name), 0)["entry"], f"{name}: the default parameters' tree")
        dev.close()
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    assert len(dev.nee_light_tree({"select": 1})["entry"]) == 0 and len(dev.nee_light_tree({"select": 1})["path"]) == 0
    dev.close()
    host.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 50])
@pytest.mark.parametrize("mis", [1, 0])
@pytest.mark.parametrize("name,planes", [("night rtiow", 0), ("panel box", 1), ("lamp", 0), ("three lamps", 1)])
def test_probe_samples_equal_the_restatement(name, planes, mis, depth):
    rb.amd_lib().rt_set_device(0)
    ijs = _probe_set()
    host = scene(name)
    cam = camera(name, *PROBE_SIZE, 1, depth)
    want = _want_probe(name, planes, mis, depth)
    inside, weighted = want[5]
    # what the set reaches: vertices inside the sphere of their picked lamp's parent (a tree of one entry has none), and weighted BSDF hits
    # on table entries (the lamp scenes' lamps are small: a handful)
    need = {"night rtiow": (50, 50), "panel box": (50, 50), "lamp": (0, 5), "three lamps": (50, 10)}[name]
    assert inside >= need[0] and weighted >= need[1], (inside, weighted)
    dev = rb.DeviceScene(host, device=0)
    got = dev.trace_samples_nee(cam, ijs, params={"mis": mis, "sample_planes": planes, "select": 1})
    for g, w, what in zip(got, want, ("radiance", "rays", "seed", "nee seed")):
        assert_same(g, w, f"{name} mis={mis} depth={depth} {what}")
    # the tree's draws are not the table's, and the path's own stream is untouched
    table = dev.trace_samples_nee(cam, ijs, params={"mis": mis, "sample_planes": planes})
    assert (got[3] != table[3]).mean() > 0.2
    assert_same(got[2], table[2], "path seeds")
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", ["default", "exact"])
@pytest.mark.parametrize("name,planes", [("night rtiow", 0), ("panel box", 1)])
def test_frames_equal_the_restatement(name, planes, traversal):
    rb.amd_lib().rt_set_device(0)
    host = scene(name)
    dev = rb.DeviceScene(host, device=0, **({} if traversal == "default" else {"traversal": rb.TRAVERSAL_EXACT}))
    shard = rb.Shard(4, 3, 2)
    for mis in (1, 0):
        for depth in (2, 50):
            cam = camera(name, 64, 48, 4, depth)
            for sh, first in ((None, 0), (shard, 0), (None, 37)):
                got, t = dev.render_nee_to_host(cam, params={"mis": mis, "sample_planes": planes, "select": 1}, shard=sh, sample_first=first)
                assert_same(got, _want_frame(name, planes, mis, depth, sh is not None, first),
                            f"{name} {traversal} mis={mis} depth={depth} shard={sh is not None} first={first}")
                assert t.guarded == 0 and t.trace_scratch_bytes == 0
    # rt_render_lit without a lens or an environment is the same frame
    cam = camera(name, 64, 48, 4, 50)
    lit, _ = dev.render_lit_to_host(cam, nee={"sample_planes": planes, "select": 1}, sample_first=37)
    assert_same(lit, _want_frame(name, planes, 1, 50, False, 37), f"{name} {traversal}: rt_render_lit, pinhole")
    dev.close()


@pytest.mark.gpu
def test_empty_table_is_rt_render_samples():
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(64, 48, 4, 50)
    dev = rb.DeviceScene(host, device=0)
    got, _ = dev.render_nee_to_host(cam, params={"select": 1, "sample_planes": 1}, sample_first=5)
    assert_same(got, nr.frame(host, cam, nr.PLAIN, sample_first=5), "select = 1 on rtiow")
    dev.close()
    host.close()


@pytest.mark.gpu
def test_lit_with_tree_planes_environment_and_lens():
    rb.amd_lib().rt_set_device(0)
    m = er.sun_and_sky(256)
    ep = dict(mode=1, scale=0.75)
    ijs = _probe_set()
    with rb.Env(m) as env:
        for name, planes in (("panel box", 1), ("night rtiow", 0)):
            host = scene(name)
            dev = rb.DeviceScene(host, device=0)
            for mis, motion in ((1, False), (0, True)):
                def cameras(w, h, spp):
                    cam = camera(name, w, h, spp)
                    close = None
                    if motion:
                        close = rb.make_camera(w, h, 50.0, (0.3, 3.1, 10), (0, 1.8, 0), (0, 0, 0), spp, 50) if name == "panel box" else \
                            night_camera(w, h, spp, eye=(13.2, 3.1, 2))
                    return cam, close
                kw = dict(lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), nee={"mis": mis, "sample_planes": planes, "select": 1}, env=env,
                          env_params=ep)
                rkw = dict(select=1, lens=LENS, nee_mis=mis, planes=planes, rgb=m, env_params=ep)
                cam, close = cameras(64, 48, 4)
                got, _ = dev.render_lit_to_host(cam, cam_close=close, sample_first=3, **kw)
                assert_same(got, tr.frame(host, cam, cam_close=close, sample_first=3, **rkw), f"{name} frame mis={mis} motion={motion}")
                cam, close = cameras(*PROBE_SIZE, 1)
                probed = dev.trace_samples_lit(cam, ijs, cam_close=close, **kw)
                want = tr.trace(host, cam, ijs, cam_close=close, **rkw)
                for g, w, col in zip(probed, want, ("radiance", "rays", "seed", "nee seed", "env seed")):
                    assert_same(g, w, f"{name} probe mis={mis} motion={motion}: {col}")
            dev.close()


@pytest.mark.gpu
def test_handle_state():
    """select 0, 1, 0 on one handle equals three fresh handles (select = 0 is the parent's frame: emit_ref.c's), and the handle's tables,
    rt_last_timing and rt_render are as before."""
    rb.amd_lib().rt_set_device(0)
    host = scene("panel box")
    cam = box_camera(96, 64, 4)
    fresh = []
    for select in (0, 1, 0):
        dev = rb.DeviceScene(host, device=0)
        fresh.append(dev.render_nee_to_host(cam, params={"sample_planes": 1, "select": select})[0])
        dev.close()
    assert_same(fresh[0], emr.frame(host, cam, planes=1), "select = 0 is the power table's frame")
    assert_same(fresh[1], tr.frame(host, cam, select=1, planes=1), "select = 1")
    dev = rb.DeviceScene(host, device=0)
    first, _ = dev.render_to_host(cam)
    before = dev.last_timing()
    table, etable = dev.nee_light_table(), dev.nee_emitter_table({"sample_planes": 1})
    for select, want in zip((0, 1, 0), fresh):
        assert_same(dev.render_nee_to_host(cam, params={"sample_planes": 1, "select": select})[0], want, f"select={select} on one handle")
    assert not np.array_equal(fresh[0], fresh[1])
    # both trees on one handle: the sphere-only table's after the two-kind one's
    assert_same(dev.render_nee_to_host(cam, params={"select": 1})[0], tr.frame(host, cam, select=1, planes=0), "the sphere-only tree")
    for g, w, what in zip(dev.nee_light_table(), table, ("index", "cdf", "pmf")):
        assert_same(g, w, f"rt_nee_light_table after a tree call: {what}")
    for g, w, what in zip(dev.nee_emitter_table({"sample_planes": 1, "select": 1}), etable, ("kind", "index", "cdf", "pmf", "area")):
        assert_same(g, w, f"rt_nee_emitter_table after a tree call: {what}")
    assert bytes(before) == bytes(dev.last_timing()), "rt_last_timing still reports the last rt_render"
    again, _ = dev.render_to_host(cam)
    assert_same(again, first, "rt_render after the tree calls")
    dev.close()


@pytest.mark.gpu
def test_cli_light_tree_frames_are_the_python_paths(test_config_text, tmp_path):
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera(0)
    assert len(dev.nee_light_tree({"select": 1})["path"]) >= 1          # (the config's lights are spheres: the flag has something to act on)
    out = subprocess.run([EXE, "--gpu", "--nee", "--light-tree"], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    fb, _ = dev.render_nee_to_host(cam, params={"select": 1})
    assert open(tmp_path / "f_0.png", "rb").read() == rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp)
    plain, _ = dev.render_nee_to_host(cam)
    assert not np.array_equal(plain, fb)
    out = subprocess.run([EXE, "--gpu", "--lit", "--light-tree", "--lens", "0.2:12"], input=text, capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr
    fb, _ = dev.render_lit_to_host(host.frame_camera_at(0.0), lens=dict(lens_radius=0.2, focus_distance=12.0), nee=dict(select=1))
    assert open(tmp_path / "f_0.png", "rb").read() == rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp)
    dev.close()
