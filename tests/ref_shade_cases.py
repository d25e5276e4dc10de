"""Inputs and drivers shared by tests/test_ref_shade.py and tests/golden/make_ref_shade_golden.py.

`Ref` wraps oracle/_ref/libref_shade.so — the reference's OWN random_utils.h, materials.h, camera.cuh and src/camera.cu compiled
host-only from where they lie (build container only; oracle/ref_shade.cpp) — and `Orc` the oracle's batched views of the functions
orc_render runs (oracle/rt_oracle.c, orc_shade_*) plus the host mirror's build_camera_data.  Both take the same arrays and return
dictionaries of numpy arrays with the same keys; outputs that exist only for some items name their mask in MASKED.
Every input is generated from a seed; nothing here reads the reference.
"""
import ctypes as C
import hashlib
import os
import tempfile

import numpy as np

from ref_geom_cases import _p, differing, f32, i32, same_bits   # noqa: F401  (differing: bit for bit, a NaN equals a NaN)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_shade.so")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT = 0, 1, 2, 3
QUAD, ELLIPSE, TRIANGLE = 0, 1, 2
# outputs written only where another output says so: attenuation and the scattered ray exist where material_scatter returned true
MASKED = {"att": "ret", "sc_o": "ret", "sc_d": "ret"}


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


# ---- the RNG in numpy / Python integers: used to CRAFT seeds (a state whose hash is a given word), never as a reference ------------
def wang_hash(s):
    s = u32(s).copy()
    s = (s ^ np.uint32(61)) ^ (s >> np.uint32(16))
    s *= np.uint32(9)
    s = s ^ (s >> np.uint32(4))
    s *= np.uint32(0x27d4eb2d)
    s = s ^ (s >> np.uint32(15))
    return s


def _unxorshift(v, shift):
    r = v
    for _ in range(32 // shift + 1):
        r = v ^ (r >> shift)
    return r


def wang_unhash(h):
    """The state s with wang_hash(s) == h (the hash is a bijection of 32-bit words)."""
    M = 0xFFFFFFFF
    s = _unxorshift(int(h) & M, 15)
    s = (s * pow(0x27d4eb2d, -1, 1 << 32)) & M
    s = _unxorshift(s, 4)
    s = (s * pow(9, -1, 1 << 32)) & M
    return _unxorshift(s ^ 61, 16)


def seed_for_draw(value, draw=1):
    """A state whose draw-th random_float is exactly the float `value` (needs value * 2^32 to be an integer below 2^32; 1.0 is
    reached by every hash >= 0xFFFFFF80)."""
    h = 0xFFFFFFC0 if value >= 1.0 else int(np.float64(np.float32(value)) * 4294967296.0)
    for _ in range(draw):
        h = wang_unhash(h)
    return h


def ulps(x, k):
    """The float32 k steps from x."""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


P8 = float(np.float32(0.8))
PINNED_STATES = [0, 1, 61, 12345, 4294967295, 3075307816]                  # tests/golden/survey_pins.json
SEED_SPECIALS = PINNED_STATES + [0, 0xFFFFFFFF] + \
    [wang_unhash(h) for h in (0xFFFFFF80, 0xFFFFFFC0, 0xFFFFFFFF, 0xFFFFFF7F, 0, 1, 0x80000000)] + \
    [wang_unhash(wang_unhash(h)) for h in (0xFFFFFF80, 0xFFFFFFFF, 0)] + \
    [seed_for_draw(ulps(P8, k)) for k in range(-3, 4)] + \
    [wang_unhash(0xCCCCCC00 + d) for d in (0x7F, 0x80, 0x81, 0x17F, 0x180, 0x181)]   # hashes that round onto / past 0.8f


def seeds(rng, n, special_share=0.05):
    s = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    mask = rng.random(n) < special_share
    s[mask] = rng.choice(np.array(SEED_SPECIALS, dtype=np.uint32), int(mask.sum()))
    s[:len(SEED_SPECIALS)] = SEED_SPECIALS[:n]
    return s


def unit_rows(a):
    a = np.asarray(a, dtype=np.float64)
    return f32(a / np.linalg.norm(a, axis=1, keepdims=True))


def long_rejection_seeds(rng, rounds=4, want=64):
    """States from which random_in_unit_sphere rejects at least `rounds` candidates (found with the numpy hash above)."""
    s0 = rng.integers(0, 1 << 32, 4_000_000, dtype=np.uint64).astype(np.uint32)
    s, ok = s0.copy(), np.ones(s0.size, bool)
    for _ in range(rounds):
        c = np.empty((s.size, 3), np.float32)
        for a in range(3):
            s = wang_hash(s)
            c[:, a] = np.float32(-1.0) + np.float32(2.0) * (s.astype(np.float32) / np.float32(4294967296.0))
        ok &= (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]) >= np.float32(1.0)
    return s0[ok][:want]


def rng_cases(rng, n):
    c = {"seeds": seeds(rng, n)}
    long = long_rejection_seeds(np.random.default_rng(5), want=min(64, n // 8))
    c["seeds"][-long.size:] = long
    c["n_long"] = np.array([long.size], np.int32)
    c["lo"] = np.where(rng.random(n) < 0.5, np.float32(-1.0), rng.normal(0, 3, n)).astype(np.float32)
    c["hi"] = np.where(rng.random(n) < 0.5, np.float32(1.0), rng.normal(0, 3, n)).astype(np.float32)
    nrm = rng.normal(0, 1, (n, 3))
    nrm[rng.random(n) < 0.05] = (0, 0, 0)
    c["normals"] = f32(nrm)
    return c


# ---- reflectance ---------------------------------------------------------------------------------------------------------------------
COSINES = [-0.0, 0.0, 1e-45, 1e-39, 1.0, float(ulps(1.0, 1)), 1.5, 3.0, np.nan, 0.5, float(ulps(1.0, -1)), -0.3, -1.0]
REF_IDX = [1.0, float(np.float32(1.0 / 1.5)), 1.5, 0.0, -1.0, 1e30, 1.0001, 2.4, float(np.float32(1.0 / 2.4))]


def reflectance_cases(rng, n):
    grid = np.array([(c, r) for c in COSINES for r in REF_IDX], np.float32)
    cos = np.where(rng.random(n) < 0.75, rng.uniform(0, 1, n), rng.uniform(-1, 2, n)).astype(np.float32)
    idx = rng.choice(np.array(REF_IDX, np.float32), n)
    rnd = rng.random(n) < 0.3
    idx[rnd] = (10.0 ** rng.uniform(-2, 2, int(rnd.sum()))).astype(np.float32)
    k = min(len(grid), n)
    cos[:k], idx[:k] = grid[:k, 0], grid[:k, 1]
    return {"cosine": f32(cos), "ref_idx": f32(idx)}


# ---- material_scatter ----------------------------------------------------------------------------------------------------------------
MATERIAL_DTYPE = np.dtype([("type", "<i4"), ("fuzz", "<f4"), ("ir", "<f4"), ("absorption", "<f4", 3), ("albedo", "<f4", 3), ("emit", "<f4", 3),
                           ("texture", "<u8"), ("reserved", "<u8")])          # rt_material (include/rtp_amd.h), 64 bytes
assert MATERIAL_DTYPE.itemsize == 64
TINY = [1.4e-45, 1.18e-38, 5.96e-8, 1.19e-7]
NORMALS = [(0, 0, 1), (0.6, 0, 0.8), (1 / 3, 2 / 3, 2 / 3), (0, 0, 2), (0.3, 0.4, 0.5), (0, 0, 1e-3)]               # unit and non-unit
DIRS = [(0, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1e18, -1e18, -1e18), (1e-20, 1e-20, -1e-20), (3, -2, -1), (0.2, 0.1, -5)] + \
    [(1, 0, sgn * t) for t in TINY for sgn in (1, -1)] + [(1, 0, 0.0), (1, 0, -0.0)]                                 # grazing: dot = +-1 step
IRS = [1.0, 1.0001, 1.5, 2.4]
ABSORPTIONS = [0.0, 0.6, 50.0, -0.5, -90.0]
BACK = [(0, 0, 0), (0.6, 0, 0.8), (4.38, 0, 5.84), (600, 0, 800)]       # hit point - ray origin: distances 0, 1, 7.3, 1000
FUZZES = [0.0, 0.7, 1.0, 5.0]
N_KEY_SEEDS = 32


def _product(*sizes):
    return [g.ravel() for g in np.meshgrid(*[np.arange(s) for s in sizes], indexing="ij")]


def _scatter_block(types, normals, dirs, fuzz, ir, absorption, back, seed, front):
    n = len(types)
    m = np.zeros(n, MATERIAL_DTYPE)
    m["type"], m["fuzz"], m["ir"] = types, fuzz, ir
    m["absorption"] = np.asarray(absorption, np.float32).reshape(n, -1) * np.array([1.0, 0.5, 0.25], np.float32)
    m["albedo"] = (0.8, 0.6, 0.3)
    m["emit"] = (4.0, 3.0, 2.0)
    point = np.broadcast_to(np.array([0.5, -1.25, 2.0], np.float32), (n, 3))
    out = {"normal": f32(np.broadcast_to(np.asarray(normals, np.float32), (n, 3))), "ray_d": f32(np.broadcast_to(np.asarray(dirs, np.float32), (n, 3))),
           "point": f32(point), "ray_o": f32(point - np.asarray(back, np.float32)), "front": i32(np.broadcast_to(front, (n,))), "mat": m,
           "seeds": u32(np.broadcast_to(np.asarray(seed, np.uint32), (n,)))}
    assert all(v.shape[0] == n for v in out.values())
    return out


def tir_sweep():
    """Inside glass (back face), incidence swept across the critical angle: sin(theta) in float steps around 1 / ir."""
    rows = []
    for ir in IRS[1:]:
        for nrm in ((0.0, 0.0, 1.0), (0.6, 0.0, 0.8)):
            nrm = np.array(nrm)
            t = np.cross(nrm, (0.0, 1.0, 0.0))
            t /= np.linalg.norm(t)
            for k in range(-48, 49):
                s = float(ulps(np.float32(1.0 / np.float32(ir)), k))
                d = s * t - np.sqrt(max(0.0, 1.0 - s * s)) * nrm           # unit, against the face-forwarded normal
                for sc in (1.0, 3.7):
                    rows.append((ir, nrm, d * sc))
    return rows


def scatter_cases(rng, n_random):
    key_seeds = np.array(SEED_SPECIALS[:N_KEY_SEEDS], np.uint32)
    N, D = np.array(NORMALS, np.float32), np.array(DIRS, np.float32)
    blocks = []
    a, b, c = _product(len(N), len(D), len(SEED_SPECIALS))                                                    # LAMBERTIAN, DIFFUSE_LIGHT
    for t in (LAMBERTIAN, DIFFUSE_LIGHT):
        blocks.append(_scatter_block(np.full(a.size, t), N[a], D[b], 0.0, 1.5, np.zeros(a.size), np.zeros((a.size, 3)), np.array(SEED_SPECIALS, np.uint32)[c], 1))
    a, b, c, d = _product(len(N), len(D), len(SEED_SPECIALS), len(FUZZES))                                    # METAL
    blocks.append(_scatter_block(np.full(a.size, METAL), N[a], D[b], np.array(FUZZES, np.float32)[d], 1.5, np.zeros(a.size), np.zeros((a.size, 3)),
                                 np.array(SEED_SPECIALS, np.uint32)[c], 1))
    a, b, c, d, e, f, g = _product(len(N), len(D), len(key_seeds), len(IRS), len(ABSORPTIONS), len(BACK), 2)   # DIELECTRIC
    blocks.append(_scatter_block(np.full(a.size, DIELECTRIC), N[a], D[b], 0.0, np.array(IRS, np.float32)[d], np.array(ABSORPTIONS, np.float32)[e],
                                 np.array(BACK, np.float32)[f], key_seeds[c], g))
    sweep = tir_sweep()                                                                                        # TIR boundary
    k = len(sweep)
    for s in (SEED_SPECIALS[3], SEED_SPECIALS[5], SEED_SPECIALS[8]):
        blocks.append(_scatter_block(np.full(k, DIELECTRIC), [r[1] for r in sweep], [r[2] for r in sweep], 0.0, [r[0] for r in sweep], np.full(k, 0.6),
                                     np.tile(BACK[1], (k, 1)), np.full(k, s), 0))
    blocks.append(near_reflectance_block())
    # random items of every type
    n = n_random
    nrm = unit_rows(rng.normal(0, 1, (n, 3)))
    nonunit = rng.random(n) < 0.1
    nrm[nonunit] *= rng.uniform(0.1, 3, (int(nonunit.sum()), 1)).astype(np.float32)
    dirs = f32(rng.normal(0, 1, (n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1)))
    flip = np.einsum("ij,ij->i", dirs, nrm) > 0                            # mostly against the normal, as set_face_normal leaves it
    dirs[flip & (rng.random(n) < 0.9)] *= -1
    back = f32(rng.normal(0, 3, (n, 3)))
    back[rng.random(n) < 0.05] = 0
    blocks.append(_scatter_block(rng.integers(0, 4, n), nrm, dirs, rng.choice(np.array(FUZZES + [0.3, 0.05], np.float32), n),
                                 rng.choice(np.array(IRS + [0.9, 1.33], np.float32), n), rng.choice(np.array(ABSORPTIONS + [0.1, 2.0], np.float32), n),
                                 back, seeds(rng, n, 0.1), rng.integers(0, 2, n)))
    out = {k: np.concatenate([blk[k] for blk in blocks]) for k in blocks[0]}
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def near_reflectance_block():
    """DIELECTRIC items whose Schlick draw lies within a few float steps of reflectance(cos_theta, ratio): cos and reflectance
    restated here in float32 (a few steps of slack cover any last-bit difference of this restatement), the draw forced by
    seed_for_draw."""
    rows = []
    for ir in (1.5, 2.4, 1.0001):
        for front in (1, 0):
            ratio = np.float32(1.0 / ir) if front else np.float32(ir)
            for cz in (1.0, 0.9, 0.5, 0.2, 0.05):
                sz = np.sqrt(1.0 - cz * cz)
                if float(ratio) * sz > 0.999:
                    continue
                d = np.array([sz, 0.0, -cz], np.float32)
                inv = np.float32(1.0 / np.float64(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], dtype=np.float32)))
                cos = min(np.float32(-(inv * d[2])), np.float32(1.0))
                r0 = (np.float32(1) - ratio) / (np.float32(1) + ratio)
                r0 = r0 * r0
                refl = np.float32(r0 + (np.float32(1) - r0) * np.power(np.float32(1) - cos, np.float32(5), dtype=np.float32))
                if not 2.0 ** -8 <= float(refl) < 1.0:
                    continue
                for k in range(-8, 9):
                    rows.append((ir, front, d, seed_for_draw(ulps(refl, k))))
    n = len(rows)
    return _scatter_block(np.full(n, DIELECTRIC), np.tile((0.0, 0.0, 1.0), (n, 1)), [r[2] for r in rows], 0.0, [r[0] for r in rows], np.full(n, 0.6),
                          np.tile(BACK[1], (n, 1)), [r[3] for r in rows], [r[1] for r in rows])


# ---- tex2D_cpu -------------------------------------------------------------------------------------------------------------------------
TEX_SIZES = [(1, 1), (4, 4), (5, 3), (256, 256)]        # (width, height)
SPARE_ROWS = 2          # rows after the image: the reference's read at 1.0 (row `height`, pixel `width`) stays inside this memory
UV_SPECIALS = [-0.0, 0.0, 1e-45, -1e-45, 1e-39, float(1 - 2.0 ** -24), -0.25, -1.75, -7.3, 1.25, 2.5, 17.01, 0.5, 1.0, -1.0, 3.0,
               float(2.0 ** -24), 0.999, 1e-8, -1e-8, 0.2, 0.4, 0.6, 0.8]


def make_texture(seed, width, height):
    """(height + SPARE_ROWS, width, 4) float32 RGBA rows, the spare rows zero; the image is [:height]."""
    t = np.zeros((height + SPARE_ROWS, width, 4), np.float32)
    t[:height] = np.random.default_rng(seed).random((height, width, 4), dtype=np.float32)
    return t


def fixture_texture(k):
    """Texture k of TEX_SIZES as the full runs and the fixture use it (made from a seed, not stored)."""
    return make_texture(7 + k, *TEX_SIZES[k])


def tex_cases(rng, n):
    g = np.array([(u, v) for u in UV_SPECIALS for v in UV_SPECIALS], np.float32)
    u = rng.uniform(-3, 3, n).astype(np.float32)
    v = rng.uniform(-3, 3, n).astype(np.float32)
    unit = rng.random(n) < 0.5
    u[unit], v[unit] = rng.random(int(unit.sum()), dtype=np.float32), rng.random(int(unit.sum()), dtype=np.float32)
    k = min(len(g), n // 64)
    u[:k], v[:k] = g[:k, 0], g[:k, 1]
    return f32(u), f32(v)


def tex_indices(u, v, width, height):
    """px, py, x0, y0 of tex2D_cpu in its own float32 arithmetic (include/materials.h:23-30)."""
    uu = u - np.floor(u)
    vv = v - np.floor(v)
    px = uu * np.float32(width)
    py = (np.float32(1.0) - vv) * np.float32(height)
    return px, py, px.astype(np.int32), py.astype(np.int32)


def tex_reads_outside(u, v, width, height):
    """Where the reference would read outside its rows: int(px) == width or int(py) == height."""
    _, _, x0, y0 = tex_indices(u, v, width, height)
    return (x0 >= width) | (y0 >= height)


def tex_wrapped(tex, u, v):
    """tex2D_cpu with x0 and y0 wrapped into the image ("wrap"), in float32 in the reference's order: what orc_tex2d documents for
    the coordinates the reference reads outside its rows at."""
    height, width = tex.shape[0] - SPARE_ROWS, tex.shape[1]
    px, py, x0, y0 = tex_indices(u, v, width, height)
    x1, y1 = (x0 + 1) % width, (y0 + 1) % height
    dx, dy = (px - x0.astype(np.float32))[:, None], (py - y0.astype(np.float32))[:, None]
    x0, y0 = x0 % width, y0 % height
    one = np.float32(1.0)
    c00, c10, c01, c11 = tex[y0, x0, :3], tex[y0, x1, :3], tex[y1, x0, :3], tex[y1, x1, :3]
    top = (one - dx) * c00 + dx * c10
    bot = (one - dx) * c01 + dx * c11
    return f32((one - dy) * top + dy * bot)


# ---- cameras -----------------------------------------------------------------------------------------------------------------------------
IMAGES = [(1, 1), (1920, 1080), (3840, 2160)]
VFOVS = [1.0, 60.0, 179.0, 20.0, 90.0, 33.3, 47.77, 120.1]


def orbit_pose(frame, frames=100):
    """Eye and target of tests/golden/config.txt's camera path at a frame (poses only: float64 here)."""
    t = frame / frames * 2 * np.pi
    z = 4.5 + 4.5 * np.sin(t - 1.57)
    return (15.0 * np.cos(3.14159 + t), 15.0 * np.sin(3.14159 + t), z), (0.0, 0.0, z)


POSES = [orbit_pose(f) for f in (0, 7, 25, 50, 99)] + [((0, 0, 10), (0, 0, 0)), ((0, 0, -3), (0, 0, 2)),        # vup parallel to w
                                                         ((1, 2, 3), (1, 2, 3)), ((13, 3, 2), (0, 0, 0)), ((1e-3, 0, 10), (0, 0, 0))]


def camera_cases():
    rows = [(p, v, wh) for p in POSES for v in VFOVS for wh in IMAGES]
    n = len(rows)
    return {"from": f32([r[0][0] for r in rows]), "at": f32([r[0][1] for r in rows]), "vfov": f32([r[1] for r in rows]),
            "whsd": i32([(r[2][0], r[2][1], 1 + k % 7, 1 + k % 50) for k, r in enumerate(rows)]),
            "background": f32(np.random.default_rng(9).random((n, 3)))}


def split_cameras(cam76):
    """The 76 bytes as their 15 floats and 4 integers (floats compare bit for bit, except that a NaN equals a NaN)."""
    words = np.ascontiguousarray(cam76).view(np.uint32).reshape(-1, 19)
    return {"cam": np.ascontiguousarray(cam76), "cam_floats": np.ascontiguousarray(words[:, :15]).view(np.float32), "cam_ints": np.ascontiguousarray(words[:, 15:]).view(np.int32)}


def get_ray_cases(rng, cams, n):
    """cams: (m, 76) uint8 CameraData records.  The first quarter of the items carry the seed render_cpu gives sample (i, j, s)
    (s in column 2 of "ijs"; -1 elsewhere) so that a device probe that seeds itself can be compared with them."""
    m = cams.shape[0]
    dims = cams.view(np.int32).reshape(m, 19)[:, 15:17]
    which = rng.integers(0, m, n)
    which[:m * 4] = np.repeat(np.arange(m), 4)[:n]
    w, h = dims[which, 0], dims[which, 1]
    i = (rng.random(n) * w).astype(np.int32)
    j = (rng.random(n) * h).astype(np.int32)
    ends = rng.random(n) < 0.2
    i[ends] = np.where(rng.random(int(ends.sum())) < 0.5, 0, w[ends] - 1)
    j[ends] = np.where(rng.random(int(ends.sum())) < 0.5, 0, h[ends] - 1)
    i[:m * 4] = np.tile([0, 0, 1, 1], m)[:n] * (w[:m * 4] - 1)
    j[:m * 4] = np.tile([0, 1, 0, 1], m)[:n] * (h[:m * 4] - 1)
    s = np.full(n, -1, np.int32)
    sd = seeds(rng, n, 0.1)
    q = n // 4
    s[:q] = rng.integers(0, 4096, q)
    sd[:q] = wang_hash(wang_hash(i[:q].astype(np.uint32) * w[:q].astype(np.uint32) + j[:q].astype(np.uint32)) + s[:q].astype(np.uint32))
    return {"cams": np.ascontiguousarray(cams[which]), "ij": i32(np.stack([i, j], 1)), "s": s, "seeds": u32(sd)}


# ---- writeColor ------------------------------------------------------------------------------------------------------------------------
SPPS = [1, 4, 100, 2500]


def write_color_cases(rng, n, spp):
    lim = np.float32(spp) * np.float32(0.999) * np.float32(0.999)
    special = [-0.0, -1.0, 0.0, 1e-45, 1e-39, float(spp), float(lim), np.nan, np.inf, -np.inf] + \
        [float(ulps(lim, k)) for k in range(-4, 5)] + [float(ulps(spp, k)) for k in (-2, -1, 1, 2)] + \
        [float(ulps(np.float32(spp) * np.float32(b / 256.0) ** 2, k)) for b in (1, 2, 17, 128, 200, 254, 255) for k in (-2, -1, 0, 1, 2)]
    x = (rng.random(n * 3) ** 2 * 1.3 * spp).astype(np.float32)
    wide = rng.random(n * 3) < 0.1
    x[wide] = (rng.normal(0, 1, int(wide.sum())) * 10.0 ** rng.uniform(-6, 6, int(wide.sum()))).astype(np.float32)
    x[:len(special)] = special
    return f32(x.reshape(n, 3))


# ---- scenes for whole paths ------------------------------------------------------------------------------------------------------------
def material(type=LAMBERTIAN, albedo=(0.7, 0.6, 0.5), fuzz=0.0, ir=1.5, absorption=(0, 0, 0), emit=(0, 0, 0), texture=0):
    m = np.zeros(1, MATERIAL_DTYPE)
    m["type"], m["fuzz"], m["ir"], m["absorption"], m["albedo"], m["emit"], m["texture"] = type, fuzz, ir, absorption, albedo, emit, texture
    return m


class PathScene:
    """A scene as plain arrays: spheres (n, 5), planes (n, 11), materials (MATERIAL_DTYPE), textures (make_texture arrays), the
    camera (eye, target, vfov, background).  host() gives the host mirror's scene (SphereData / PlaneData records, its build_bvh)
    with the textures attached, for the oracle and the device."""
    W, H, SPP = 48, 32, 4

    def __init__(self, name, spheres, planes, materials, eye, target, vfov=50.0, background=(0.7, 0.8, 1.0), textures=()):
        self.name = name
        self.spheres = f32(np.asarray(spheres, np.float32).reshape(-1, 5))
        self.planes = f32(np.asarray(planes, np.float32).reshape(-1, 11))
        self.materials = np.ascontiguousarray(np.concatenate(materials)) if isinstance(materials, (list, tuple)) else np.ascontiguousarray(materials)
        self.textures = [np.ascontiguousarray(t, dtype=np.float32) for t in textures]
        self.eye, self.target, self.vfov, self.background = f32(eye), f32(target), float(vfov), f32(background)
        self._host = None

    def tex_args(self):
        if not self.textures:
            return 0, np.zeros(1, np.float32), np.zeros(3, np.int64)
        data = np.concatenate([t.ravel() for t in self.textures])
        offs = np.cumsum([0] + [t.size for t in self.textures[:-1]])
        dims = np.array([(o, t.shape[1], t.shape[0] - SPARE_ROWS) for o, t in zip(offs, self.textures)], np.int64)
        return len(self.textures), f32(data), np.ascontiguousarray(dims)

    def host(self):
        import rtp_bindings as rb
        if self._host is None:
            mats = (rb.Material * len(self.materials)).from_buffer_copy(self.materials.tobytes())
            h = rb.HostScene.from_arrays(self.spheres, self.planes, list(mats))
            if self.textures:
                self._tex = (rb.Texture * len(self.textures))()
                for k, t in enumerate(self.textures):
                    self._tex[k].rgba = t.ctypes.data_as(C.POINTER(C.c_float))
                    self._tex[k].width, self._tex[k].height = t.shape[1], t.shape[0] - SPARE_ROWS
                h.desc.textures = C.cast(self._tex, C.POINTER(rb.Texture))
                h.desc.num_textures = len(self.textures)
            self._host = h
        return self._host

    def camera(self, depth=50, spp=None):
        import rtp_bindings as rb
        return rb.make_camera(self.W, self.H, self.vfov, tuple(map(float, self.eye)), tuple(map(float, self.target)), tuple(map(float, self.background)),
                              self.SPP if spp is None else spp, depth)

    def whsd(self, depth=50):
        return i32([self.W, self.H, self.SPP, depth])

    def samples(self, n, seed=0):
        rng = np.random.default_rng(1000 + seed)
        return i32(np.stack([rng.integers(0, self.W, n), rng.integers(0, self.H, n), rng.integers(0, 1000, n)], 1))

    def arrays(self):
        """What a fixture keeps of the scene."""
        d = {"spheres": self.spheres, "planes": self.planes, "materials": self.materials.view(np.uint8).reshape(-1, 64),
             "eye": self.eye, "target": self.target, "vfov": np.float32(self.vfov), "background": self.background}
        for k, t in enumerate(self.textures):
            d[f"tex{k}"] = t
        return d

    @classmethod
    def from_arrays(cls, name, d):
        tex = [d[f"tex{k}"] for k in range(8) if f"tex{k}" in d]
        return cls(name, d["spheres"], d["planes"], np.ascontiguousarray(d["materials"]).view(MATERIAL_DTYPE).reshape(-1), d["eye"], d["target"],
                   float(d["vfov"]), d["background"], tex)


def _sph(c, r, m):
    return [c[0], c[1], c[2], r, m]


def _pl(base, u, v, m, t):
    return list(base) + list(u) + list(v) + [m, t]


def _one_material_scene(name, mat, background):
    """One material alone: on a sphere, a quad floor, an ellipse and a triangle (irregular coordinates: no exact ties)."""
    sph = [_sph((0.13, -0.21, 1.07), 1.03, 0)]
    pl = [_pl((-6.1, -5.9, -0.03), (12.3, 0.2, 0.0), (-0.1, 11.7, 0.0), 0, QUAD),
          _pl((1.9, -2.4, 0.4), (0.1, 2.1, 0.3), (-0.3, 0.2, 2.2), 0, ELLIPSE),
          _pl((-2.6, 0.7, 0.2), (1.1, 1.9, 0.1), (0.2, -0.4, 2.3), 0, TRIANGLE)]
    return PathScene(name, sph, pl, [mat], (7.3, -4.1, 3.2), (0.1, 0.0, 0.9), 48.0, background)


def config_scene():
    """tests/golden/test_config.txt through the host mirror's parser, taken apart into plain arrays: the geometry and materials the
    reference's create_test_config.py printer describes.  The floor texture that file names (../floor2.jpg) does not exist, here or in
    the reference's tree: the parser says "Failed to load texture" on stderr at every run — that message is no failure — and leaves
    the floor untextured, so this scene has NO texture on either side (its material's texture index is set to 0 to say so; the
    textured scenes are "textured" and "forty_mixed")."""
    import rtp_bindings as rb
    with open(os.path.join(GOLDEN_DIR, "test_config.txt")) as f:
        h = rb.HostScene.from_config(f.read())
    d = h.desc
    sp = np.ctypeslib.as_array(C.cast(d.spheres, C.POINTER(C.c_float)), shape=(d.num_spheres, 8)) if d.num_spheres else np.zeros((0, 8), np.float32)
    spheres = np.concatenate([sp[:, :4], sp.view(np.int32)[:, 4:5].astype(np.float32)], 1)
    p = np.ctypeslib.as_array(C.cast(d.planes, C.POINTER(C.c_float)), shape=(d.num_planes, 20)) if d.num_planes else np.zeros((0, 20), np.float32)
    pi = p.view(np.int32)
    planes = np.concatenate([p[:, 12:15], p[:, 6:9], p[:, 9:12], pi[:, 2:3].astype(np.float32), pi[:, 0:1].astype(np.float32)], 1)
    mats = np.frombuffer(C.string_at(d.materials, 64 * d.num_materials), MATERIAL_DTYPE).copy()
    mats["texture"] = 0
    return PathScene("test_config", spheres.copy(), planes.copy(), mats, (-15.0, 0.0, 4.5), (0.0, 0.0, 4.5), 90.0, (0, 0, 0))


def path_scenes():
    sky, dark = (0.7, 0.8, 1.0), (0.02, 0.03, 0.05)
    out = [_one_material_scene("lambertian", material(LAMBERTIAN, (0.8, 0.3, 0.2)), sky),
           _one_material_scene("metal", material(METAL, (0.9, 0.8, 0.7), fuzz=0.3), sky),
           _one_material_scene("dielectric", material(DIELECTRIC, ir=1.5, absorption=(0.3, 0.1, 0.05)), sky),
           _one_material_scene("diffuse_light", material(DIFFUSE_LIGHT, emit=(3.0, 2.5, 2.0)), dark)]
    # glass inside glass: positive, zero and negative absorption
    mats = [material(LAMBERTIAN, (0.5, 0.55, 0.5))]
    sph = [_sph((0.0, 0.0, -200.31), 200.0, 0)]
    for k, (ab_out, ab_in) in enumerate((((0.6, 0.3, 0.1), (1.5, 0.2, 0.9)), ((0, 0, 0), (0, 0, 0)), ((-0.5, -0.2, -0.1), (-0.3, -0.6, -0.05)))):
        c = (-2.37 + 2.41 * k, 0.11 * k - 0.07, 0.83)
        mats += [material(DIELECTRIC, ir=1.5, absorption=ab_out), material(DIELECTRIC, ir=2.4 if k else 1.0001, absorption=ab_in)]
        sph += [_sph(c, 1.07, 1 + 2 * k), _sph((c[0] + 0.05, c[1] - 0.03, c[2] + 0.02), 0.61, 2 + 2 * k)]
    out.append(PathScene("glass_in_glass", sph, [], mats, (0.4, -8.2, 2.1), (0.05, 0.0, 0.7), 40.0, sky))
    # fuzzed metal floor at a grazing view
    out.append(PathScene("metal_floor_grazing",
                         [_sph((0.3, 4.1, 0.52), 0.5, 1), _sph((-1.2, 7.3, 0.77), 0.75, 2), _sph((1.9, 9.2, 0.41), 0.4, 3)],
                         [_pl((-20.3, -5.1, 0.013), (40.7, 0.3, 0.0), (-0.2, 60.1, 0.0), 0, QUAD)],
                         [material(METAL, (0.8, 0.8, 0.85), fuzz=0.7), material(LAMBERTIAN, (0.7, 0.2, 0.2)), material(DIELECTRIC, ir=1.5),
                          material(METAL, (0.9, 0.7, 0.3), fuzz=0.0)], (0.0, -6.0, 0.09), (0.1, 4.0, 0.3), 35.0, sky))
    # emitters in the dark
    out.append(PathScene("emitters",
                         [_sph((0.0, 0.0, -100.2), 100.0, 0), _sph((-1.3, 0.4, 0.9), 0.31, 1), _sph((1.6, -0.7, 1.4), 0.22, 2), _sph((0.2, 0.9, 0.55), 0.6, 3),
                          _sph((-0.6, -1.1, 0.45), 0.5, 4)],
                         [_pl((-1.1, 1.9, 2.6), (2.3, 0.1, 0.0), (0.1, -0.2, 1.3), 5, QUAD), _pl((2.2, 0.3, 0.1), (0.2, 1.4, 0.1), (0.0, 0.3, 1.6), 1, TRIANGLE)],
                         [material(LAMBERTIAN, (0.6, 0.6, 0.6)), material(DIFFUSE_LIGHT, emit=(12, 9, 4)), material(DIFFUSE_LIGHT, emit=(2, 6, 14)),
                          material(METAL, (0.9, 0.9, 0.9), fuzz=0.1), material(DIELECTRIC, ir=1.5, absorption=(0.2, 0.4, 0.1)),
                          material(DIFFUSE_LIGHT, emit=(5, 5, 5))], (4.9, -5.3, 2.4), (0.0, 0.0, 0.7), 42.0, (0, 0, 0)))
    # a textured quad and a textured sphere
    out.append(PathScene("textured",
                         [_sph((0.21, 0.13, 1.09), 1.05, 1), _sph((-2.2, 1.3, 0.6), 0.58, 2)],
                         [_pl((-7.3, -6.8, -0.02), (14.1, 0.4, 0.0), (-0.3, 13.2, 0.0), 0, QUAD)],
                         [material(LAMBERTIAN, (0.9, 0.9, 0.9), texture=1), material(LAMBERTIAN, (1.0, 0.8, 0.7), texture=2), material(METAL, (0.8, 0.8, 0.9), fuzz=0.05)],
                         (6.1, -5.2, 3.7), (0.0, 0.1, 0.8), 50.0, sky, [make_texture(41, 5, 3), make_texture(42, 16, 16)]))
    out.append(config_scene())
    # forty primitives of every kind and material
    rng = np.random.default_rng(8086)
    mats = [material(LAMBERTIAN, (0.5, 0.5, 0.5)), material(LAMBERTIAN, (0.2, 0.7, 0.3), texture=1), material(METAL, (0.8, 0.6, 0.4), fuzz=0.4),
            material(METAL, (0.95, 0.95, 0.95), fuzz=0.0), material(DIELECTRIC, ir=1.5), material(DIELECTRIC, ir=1.33, absorption=(0.8, 0.1, 0.1)),
            material(DIFFUSE_LIGHT, emit=(6, 5, 4))]
    sph = [_sph((0.0, 0.0, -500.17), 500.0, 0)] + [_sph((rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0.2, 1.6)), rng.uniform(0.15, 0.6), 1 + k % 6)
                                                   for k in range(27)]
    pl = [_pl(rng.uniform(-4, 4, 3) + (0, 0, 2), rng.uniform(-1.5, 1.5, 3), rng.uniform(-1.5, 1.5, 3), k % 7, k % 3) for k in range(12)]
    out.append(PathScene("forty_mixed", sph, pl, mats, (9.1, 2.3, 3.4), (0.0, 0.0, 0.8), 45.0, (0.3, 0.35, 0.45), [make_texture(43, 5, 3)]))
    return out


DEPTHS = (1, 2, 50)
N_SAMPLES = 4096


# ---- digests -----------------------------------------------------------------------------------------------------------------------------
def digests(out, keys=None, keep=None):
    """sha256 per output in the terms of `differing` (every NaN alike); MASKED outputs only where their mask is set; `keep`
    (a boolean array or None) selects the items that count."""
    d = {}
    for key in (out if keys is None else keys):
        a = np.ascontiguousarray(out[key])
        sel = np.ones(a.shape[0], bool) if keep is None else keep.copy()
        if key in MASKED:
            sel &= out[MASKED[key]] != 0
        a = np.ascontiguousarray(a[sel])
        if a.dtype == np.float32:
            a = a.copy()
            a[np.isnan(a)] = np.float32(np.nan)
        d[key] = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()
    return d


# ---- the full runs: what tests/test_ref_shade.py compares and tests/golden/make_ref_shade_golden.py records digests of ---------------------
TOPICS = ("rng", "reflectance", "scatter", "tex", "cameras", "write_color", "paths")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def full_cases(topic):
    """The inputs of a topic's full run, generated once per process."""
    if topic == "rng":
        return cached(topic, lambda: rng_cases(np.random.default_rng(101), 500_000))
    if topic == "reflectance":
        return cached(topic, lambda: reflectance_cases(np.random.default_rng(102), 200_000))
    if topic == "scatter":
        return cached(topic, lambda: scatter_cases(np.random.default_rng(103), 400_000))
    if topic == "tex":
        return cached(topic, lambda: [(fixture_texture(k),) + tex_cases(np.random.default_rng(200 + k), 100_000) for k in range(len(TEX_SIZES))])
    if topic == "write_color":
        return cached(topic, lambda: [(spp, write_color_cases(np.random.default_rng(300 + spp), 100_000, spp)) for spp in SPPS])
    if topic == "cameras":
        return cached(topic, camera_cases)
    if topic == "paths":
        return cached(topic, path_scenes)
    raise KeyError(topic)


def full_runs(topic, lib, orc):
    """(what, outputs of `lib` (a Ref or an Orc), keep) for every run of a topic.  keep: the items that count (None: all) — texture
    coordinates at which the reference stays inside its rows, path samples and pixels free of such a fetch, as `orc` reports them."""
    c = full_cases(topic)
    if topic in ("rng", "reflectance", "scatter"):
        yield topic, getattr(lib, topic)(c), None
    elif topic == "tex":
        for tex, u, v in c:
            inside = ~tex_reads_outside(u, v, tex.shape[1], tex.shape[0] - SPARE_ROWS)
            out = lib.tex2d(tex, u[inside], v[inside])
            yield f"tex {tex.shape[1]}x{tex.shape[0] - SPARE_ROWS}", {"tex": out["tex"]}, None
    elif topic == "cameras":
        out = lib.cameras(c)
        yield "cameras", {k: out[k] for k in ("cam_floats", "cam_ints")}, None
        cams = orc.cameras(c)["cam"]
        yield "get_ray", lib.get_ray(cached("get_ray", lambda: get_ray_cases(np.random.default_rng(104), cams, 200_000))), None
    elif topic == "write_color":
        for spp, sums in c:
            yield f"write_color {spp}", lib.write_color(sums, spp), None
    elif topic == "paths":
        for k, sc in enumerate(c):
            for depth in DEPTHS:
                ijs = sc.samples(N_SAMPLES, 10 * k + depth)
                flags = cached(("flags", k, depth), lambda: orc.trace(sc, depth, ijs)["flags"])
                out = lib.trace(sc, depth, ijs)
                yield f"{sc.name} depth {depth}", {"rad": out["rad"], "seed": out["seed"]}, (flags & 1) == 0
            wrapped = cached(("wrapped", k), lambda: orc.frame(sc)["wrapped"])
            yield f"{sc.name} frame", {"frame": lib.frame(sc)["frame"].reshape(-1, 3)}, ~wrapped.ravel()


# ---- the two libraries -------------------------------------------------------------------------------------------------------------------
class _Common:
    """The calls that differ only in the prefix of the exported names."""

    def rng(self, c):
        L, n, s = self.lib, c["seeds"].shape[0], c["seeds"]
        N, r = C.c_int64(n), {}
        r["hash"] = np.zeros(n, np.uint32); getattr(L, self.pre + "wang_hash")(N, _p(s), _p(r["hash"]))
        for name, extra, shape in (("random_float", (), (n,)), ("random_range", (_p(c["lo"]), _p(c["hi"])), (n,)), ("random_pm1", (), (n,)),
                                   ("random_in_unit_sphere", (), (n, 3)), ("random_unit_vector", (), (n, 3)),
                                   ("random_in_hemisphere", (_p(c["normals"]),), (n, 3))):
            r[name], r[name + "_seed"] = np.zeros(shape, np.float32), np.zeros(n, np.uint32)
            getattr(L, self.pre + name)(N, _p(s), *extra, _p(r[name]), _p(r[name + "_seed"]))
        return r

    def reflectance(self, c):
        out = np.zeros(c["cosine"].shape[0], np.float32)
        getattr(self.lib, self.pre + "reflectance")(C.c_int64(out.size), _p(c["cosine"]), _p(c["ref_idx"]), _p(out))
        return {"reflectance": out}

    def scatter(self, c):
        n = c["seeds"].shape[0]
        r = {"ret": np.zeros(n, np.int32), "att": np.zeros((n, 3), np.float32), "sc_o": np.zeros((n, 3), np.float32), "sc_d": np.zeros((n, 3), np.float32),
             "seed": np.zeros(n, np.uint32), "emit": np.zeros((n, 3), np.float32)}
        getattr(self.lib, self.pre + "material_scatter")(C.c_int64(n), _p(c["ray_o"]), _p(c["ray_d"]), _p(c["point"]), _p(c["normal"]), _p(c["front"]),
                                                         _p(c["mat"]), _p(c["seeds"]), _p(r["ret"]), _p(r["att"]), _p(r["sc_o"]), _p(r["sc_d"]), _p(r["seed"]))
        getattr(self.lib, self.pre + "material_emit")(C.c_int64(n), _p(c["mat"]), _p(r["emit"]))
        return r

    def get_ray(self, c):
        n = c["seeds"].shape[0]
        r = {"o": np.zeros((n, 3), np.float32), "d": np.zeros((n, 3), np.float32), "seed": np.zeros(n, np.uint32)}
        getattr(self.lib, self.pre + "get_ray")(C.c_int64(n), _p(c["cams"]), _p(c["ij"]), _p(c["seeds"]), _p(r["o"]), _p(r["d"]), _p(r["seed"]))
        return r


class Ref(_Common):
    """The reference's own code (oracle/_ref/libref_shade.so)."""
    pre = "ref_"

    def __init__(self, path=REF_LIB):
        self.lib = C.CDLL(path)
        self.lib.ref_write_color.restype = C.c_int32

    def sizes(self):
        return self.lib.ref_sizeof_camera_data(), self.lib.ref_sizeof_material_data()

    def tex2d(self, tex, u, v):
        """Only for (u, v) at which the reference stays inside its rows (tex_reads_outside is False)."""
        out = np.zeros((u.size, 3), np.float32)
        self.lib.ref_tex2d(_p(tex), tex.shape[1], tex.shape[0] - SPARE_ROWS, C.c_int64(u.size), _p(u), _p(v), _p(out))
        return {"tex": out}

    def cameras(self, c):
        out = np.zeros((c["vfov"].size, 76), np.uint8)
        self.lib.ref_build_camera_data(C.c_int64(c["vfov"].size), _p(c["from"]), _p(c["at"]), _p(c["vfov"]), _p(c["whsd"]), _p(c["background"]), _p(out))
        return split_cameras(out)

    def write_color(self, sums, spp):
        out = np.zeros((sums.shape[0], 3), np.uint8)
        with tempfile.TemporaryDirectory() as tmp:
            rc = self.lib.ref_write_color(C.c_int64(sums.shape[0]), _p(sums), spp, os.path.join(tmp, "saver.bin").encode(), _p(out))
        assert rc == 0, "BinarySaver's file is not a header and three bytes per pixel"
        return {"bytes": out}

    def _scene_args(self, sc):
        nt, data, dims = sc.tex_args()
        self._keep = (data, dims)
        return (sc.spheres.shape[0], _p(sc.spheres), sc.planes.shape[0], _p(sc.planes), sc.materials.shape[0], _p(sc.materials), nt, _p(data), _p(dims))

    def trace(self, sc, depth, ijs):
        cam = sc.camera(depth)
        rad, seed = np.zeros((ijs.shape[0], 3), np.float32), np.zeros(ijs.shape[0], np.uint32)
        self.lib.ref_trace_samples(*self._scene_args(sc), C.byref(cam), C.c_int64(ijs.shape[0]), _p(ijs), _p(rad), _p(seed))
        return {"rad": rad, "seed": seed}

    def frame(self, sc):
        fb = np.zeros((sc.H, sc.W, 3), np.float32)
        self.lib.ref_render_cpu(*self._scene_args(sc), _p(sc.eye), _p(sc.target), C.c_float(sc.vfov), _p(sc.whsd()), _p(sc.background), _p(fb))
        return {"frame": fb}


class Orc(_Common):
    """The oracle's views (oracle/librt_oracle.so) + the host mirror's camera (librtp_host.so)."""
    pre = "orc_shade_"

    def __init__(self):
        import oracle_bindings as ob
        import rtp_bindings as rb
        self.lib, self.ob, self.rb = ob.lib(), ob, rb

    def tex2d(self, tex, u, v):
        t = self.rb.Texture(tex.ctypes.data_as(C.POINTER(C.c_float)), tex.shape[1], tex.shape[0] - SPARE_ROWS)
        out, wrapped = np.zeros((u.size, 3), np.float32), np.zeros(u.size, np.int32)
        self.lib.orc_shade_tex2d(C.byref(t), C.c_int64(u.size), _p(u), _p(v), _p(out), _p(wrapped))
        return {"tex": out, "wrapped": wrapped}

    def cameras(self, c):
        out = np.zeros((c["vfov"].size, 76), np.uint8)
        for k in range(c["vfov"].size):
            w, h, s, d = (int(x) for x in c["whsd"][k])
            cam = self.rb.make_camera(w, h, float(c["vfov"][k]), tuple(map(float, c["from"][k])), tuple(map(float, c["at"][k])),
                                      tuple(map(float, c["background"][k])), s, d)
            out[k] = np.frombuffer(bytes(cam), np.uint8)
        return split_cameras(out)

    def write_color(self, sums, spp):
        out = np.zeros((sums.shape[0], 3), np.uint8)
        self.lib.orc_shade_write_color(C.c_int64(sums.shape[0]), _p(sums), spp, _p(out))
        return {"bytes": out}

    def trace(self, sc, depth, ijs):
        """+ "flags": bit 0 a texture fetch wrapped where the reference reads outside its rows, bit 1 a hit depended on visit order."""
        cam, host = sc.camera(depth), sc.host()
        rad, seed, flags = np.zeros((ijs.shape[0], 3), np.float32), np.zeros(ijs.shape[0], np.uint32), np.zeros(ijs.shape[0], np.int32)
        self.lib.orc_shade_trace_samples(C.byref(host.desc), C.byref(cam), C.c_int64(ijs.shape[0]), _p(ijs), _p(rad), _p(seed), _p(flags))
        return {"rad": rad, "seed": seed, "flags": flags}

    def frame(self, sc):
        """+ "wrapped": the pixels one of whose samples has flag bit 0."""
        fb = self.ob.render(sc.host(), sc.camera(50), threads=1)
        jj, ii, ss = np.meshgrid(np.arange(sc.H), np.arange(sc.W), np.arange(sc.SPP), indexing="ij")
        flags = self.trace(sc, 50, i32(np.stack([ii.ravel(), jj.ravel(), ss.ravel()], 1)))["flags"].reshape(sc.H, sc.W, sc.SPP)
        return {"frame": fb, "wrapped": (flags & 1).any(axis=2), "order": (flags & 2).any(axis=2)}
