"""The vertices of the light-sampling check (TEST INFRASTRUCTURE): named sets of vertices — pure functions of fixed seeds —
for the developer library's rt_debug_light_vertices, and the CPU statement of every word it writes (emit_ref.c, tree_ref.c, gloss_ref.c
and medium_ref.c's per-vertex exports).  tests/test_light_vertices.py checks on the CPU that the sets reach what they aim at;
tests/dev_light_vertex_checks.py compares the device with the statement word for word.

A Pass is one hook call: a scene, the call's parameters (select, sample_planes, mis, the environment and its parameters), a routine, a
Pb kind and the vertices — x, nv, v (3 floats each), s, seed — in the meaning the routine gives them (rt_capi.hip, above the hook)."""
import collections
import functools

import numpy as np

import emit_reference as emr
import env_reference as er
import gloss_reference as glr
import lit_fuzz
import medium_reference as mr
import rtp_bindings as rb
import test_light_tree as tl
import tree_reference as tr

AB = np.array([0.75, 0.5, 0.25, 1.0, 0.5, 2.0], np.float32)          # the calls' albedo a and throughput beta
MIN_FUZZ = np.float32(lit_fuzz.RT_GLOSSY_MIN_FUZZ)                      # 2^-10
NEE_PB = np.float32(0.15915494)                                       # RT_NEE_PB, 1 / (2 pi) as the header writes it
FUZZES = np.array([MIN_FUZZ, 0.05, 0.5, 1.0, 1.0 + 2.0 ** -23, 1.5, 4.0], np.float32)
GS = np.array([0.0, 0.5, -0.5, 0.95, -0.95], np.float32)
BASE = 4096
MAX_CALL = 65536
SCENES = ("lamp", "three lamps", "panel box", "night rtiow", "exact")
COLUMNS = {0: ("ok", "dir.x", "dir.y", "dir.z", "c.r", "c.g", "c.b", "code", "seed after"),
           1: ("ok", "dir.x", "dir.y", "dir.z", "c.r", "c.g", "c.b", "seed after"),
           2: ("diffuse.r", "diffuse.g", "diffuse.b", "carried.r", "carried.g", "carried.b"),
           3: ("d0 diffuse.r", "d0 diffuse.g", "d0 diffuse.b", "d1 diffuse.r", "d1 diffuse.g", "d1 diffuse.b", "d1 carried.r", "d1 carried.g",
               "d1 carried.b", "d0 carried.r", "d0 carried.g", "d0 carried.b"),
           4: ("entry", "tree entry", "p", "seed after", "tree_pmf", "found"),
           5: ("pg", "ph")}
FLOAT_COLUMNS = {0: range(1, 7), 1: range(1, 7), 2: range(6), 3: range(12), 4: (2, 4), 5: range(2)}
QUAD, ELLIPSE, TRIANGLE = 0, 1, 2

Pass = collections.namedtuple("Pass", "label scene cls routine pb select planes mis env env_params x nv v s seed")


# ---- the generator, in numpy ----------------------------------------------------------------------------------------------------------
def wang(s):
    s = np.asarray(s, np.uint32)
    s = (s ^ np.uint32(61)) ^ (s >> np.uint32(16))
    s = s * np.uint32(9)
    s = s ^ (s >> np.uint32(4))
    s = s * np.uint32(0x27d4eb2d)
    return s ^ (s >> np.uint32(15))


def draw(state):
    """orc_random_float: → (the draw, the state after it)."""
    state = wang(state)
    return state.astype(np.float32) / np.float32(4294967296.0), state


def unwang(e):
    """The state whose hash is e (every step of the hash is a bijection of the 32-bit words)."""
    e = int(e)
    d = e ^ (e >> 15) ^ (e >> 30)
    c = (d * pow(0x27d4eb2d, -1, 1 << 32)) & 0xffffffff
    b = c
    for k in range(4, 32, 4):
        b ^= c >> k
    a = (b * pow(9, -1, 1 << 32)) & 0xffffffff
    hi = a >> 16
    return (hi << 16) | ((a & 0xffff) ^ 61 ^ hi)


def ulps(x, k):
    """x moved by k units in the last place (k may be negative)."""
    x = np.asarray(x, np.float32)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def unit_vectors(rng, m):
    v = rng.normal(size=(m, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
EXACT_SPHERES = np.array([[0, 0, 0, 1, 1], [4, 0, -0.0, 0.5, 2], [0, 0, -8, 2.0 ** -10, 3], [0, -103, 0, 100, 0]], np.float32)
EXACT_PLANES = np.array([
    [2, 2, 0, 1, 0, 0, 0, 1, 0, 4, QUAD],                       # a unit QUAD in z = 0
    [-1, 2.5, 1, 0, 0, 1, 0, 1, 0, 0, QUAD],                    # a LAMBERTIAN quad between the emitters: a code the table does not hold
    [0, 3, 1, 0, 0, 1, 1, 0, 0, 5, TRIANGLE],                   # a unit TRIANGLE in y = 3
    [2, 4, 1, 1, 0, 0, 0, 0, 1, 7, QUAD],                       # a light whose emission is (0, 0, 0): skipped by the table
    [-3, 0, -1, 0, 1, 0, 0, 0, 1, 6, ELLIPSE],                  # a unit ELLIPSE in x = -3
    [2, -3, 0, 1, 0, 0, 1, 2.0 ** -20, 0, 4, QUAD],             # a sliver: v = u + (0, 2^-20, 0)
], np.float32)


@functools.lru_cache(maxsize=None)
def exact_scene():
    """Emitters of float-exact geometry: spheres at the origin (r 1), at (4, 0, -0) (r 0.5) and at (0, 0, -8) (r 2^-10), a unit quad, triangle
    and ellipse in axis planes, a sliver quad, and between them two planes the table skips (a LAMBERTIAN one and a light of emission 0)."""
    m = tl.material
    mats = [m(tl.MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), m(tl.MAT_LIGHT, emit=(4, 2, 1)), m(tl.MAT_LIGHT, emit=(1, 2, 4)), m(tl.MAT_LIGHT, emit=(3e5, 3e5, 3e5)),
            m(tl.MAT_LIGHT, emit=(2, 2, 2)), m(tl.MAT_LIGHT, emit=(6, 8, 6)), m(tl.MAT_LIGHT, emit=(5, 4, 3)), m(tl.MAT_LIGHT, emit=(0, 0, 0))]
    return rb.HostScene.from_arrays(EXACT_SPHERES, EXACT_PLANES, mats)


def scene(name):
    return exact_scene() if name == "exact" else tl.scene(name)


@functools.lru_cache(maxsize=None)
def camera(name):
    """The camera the hook fills its KParams from: the routines read its background alone."""
    return rb.make_camera(8, 8, 40.0, (0, 2, 7), (0, 1, 0), (0.125, 0.25, 0.5), 1, 50)


@functools.lru_cache(maxsize=None)
def bounds(name):
    d = scene(name).desc
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i in range(d.num_spheres):
        s = d.spheres[i]
        if s.radius > 50:          # (a floor sphere is no part of the scene's size)
            continue
        c = np.array(s.center.e[:])
        lo, hi = np.minimum(lo, c - s.radius), np.maximum(hi, c + s.radius)
    for i in range(d.num_planes):
        p = d.planes[i]
        b, u, v = (np.array(q.e[:]) for q in (p.base, p.u, p.v))
        for q in (b, b + u, b + v, b + u + v):
            lo, hi = np.minimum(lo, q), np.maximum(hi, q)
    return lo, hi


def size(name):
    lo, hi = bounds(name)
    return float(np.linalg.norm(hi - lo))


def sun_and_sky_16():
    """env_reference.sun_and_sky at n = 16.  Its disc covers no texel centre at that size (the function refuses n below 48), so the sun is
    placed by hand: the one texel whose centre is nearest the sun's direction carries the sun's share of the power."""
    n = 16
    d = er.texel_directions(n)
    y = d[..., 1]
    sky = np.array([0.5, 0.7, 1.0])[None, None, :] * (0.25 + 0.75 * np.maximum(y, 0.0))[..., None]
    sky = sky + np.array([0.1, 0.09, 0.08])[None, None, :] * np.maximum(-y, 0.0)[..., None]
    el, az = np.radians(er.SUN_ELEVATION_DEG), np.radians(30.0)
    sun_dir = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    iy, ix = np.unravel_index(np.argmax(d @ sun_dir), (n, n))
    omega = er.texel_solid_angles(n)
    colour = np.array([1.0, 0.9, 0.7])
    level = er.SUN_SHARE / (1.0 - er.SUN_SHARE) * (sky.sum(-1) * omega).sum() / (colour.sum() * omega[iy, ix])
    out = sky.copy()
    out[iy, ix] += level * colour
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def environment(which):
    """(rgb, params) of the two environments: the sun and sky at n = 16 (sun_and_sky_16) under a rotation whose nine entries are inexact,
    and a map of n = 2 with one texel of weight 0 under the identity."""
    if which == "sun":
        rot = lit_fuzz.random_rot(np.random.default_rng(4201))
        assert (np.abs(rot) > 0.05).all() and (np.abs(rot) < 0.99).all()
        return sun_and_sky_16(), dict(mode=1, scale=0.75, rot=[float(q) for q in rot.ravel()], camera_visible=0, glossy=1)
    rgb = np.array([[[1, 2, 3], [0, 0, 0]], [[0.5, 0.25, 4], [2, 2, 2]]], np.float32)
    return rgb, dict(mode=1, scale=1.0, camera_visible=1, glossy=1)


def table_configs(name):
    """(sample_planes, select) of the emitter tables a scene has: the sphere-only one and its tree, and — where a plane emits — the two-kind
    one and its tree."""
    two_kind = (emr.table(scene(name), 1)[0] == 1).any()
    return [(0, 0), (0, 1)] + ([(1, 0), (1, 1)] if two_kind else [])


def table_spheres(name, planes=0, most=6):
    """(centre (k, 3), radius (k,), entry (k,)) of up to `most` of the table's spheres, spread over the table."""
    kind, idx, *_ = emr.table(scene(name), planes)
    d = scene(name).desc
    es = [e for e in range(len(kind)) if kind[e] == 0]
    es = [es[k] for k in sorted(set(np.linspace(0, len(es) - 1, min(most, len(es))).astype(int)))]
    c = np.array([d.spheres[int(idx[e])].center.e[:] for e in es], np.float32)
    r = np.array([d.spheres[int(idx[e])].radius for e in es], np.float32)
    return c, r, np.array(es)


def table_planes(name):
    """[(entry, plane index, base, u, v, unit normal, type)] of the two-kind table's planes."""
    kind, idx, *_ = emr.table(scene(name), 1)
    d = scene(name).desc
    out = []
    for e in range(len(kind)):
        if kind[e] == 1:
            p = d.planes[int(idx[e])]
            out.append((e, int(idx[e]), *(np.array(q.e[:], np.float32) for q in (p.base, p.u, p.v, p.normal)), int(p.type)))
    return out


# ---- vertex sets: name → x, nv, seed (v and s come with the Pb kind) ---------------------------------------------------------------------
VSet = collections.namedtuple("VSet", "name x nv seed")


def _rng(*key):
    return np.random.default_rng([ord(c) for c in "/".join(str(k) for k in key)])


def _vset(scene_name, name, x, nv=None, seeds=1):
    """x (m, 3) with `seeds` random seeds each (the vertices repeated) and, unless given, a random unit nv per row."""
    rng = _rng(scene_name, name)
    x = np.repeat(np.asarray(x, np.float32).reshape(-1, 3), seeds, axis=0)
    nv = unit_vectors(rng, len(x)) if nv is None else np.repeat(np.asarray(nv, np.float32).reshape(-1, 3), seeds, axis=0)
    assert 64 <= len(x) <= 4096 and np.isfinite(x).all(), (name, len(x))
    return VSet(name, x, nv, rng.integers(0, 1 << 32, len(x), dtype=np.uint32))


def base_set(name):
    rng = _rng(name, "base")
    lo, hi = bounds(name)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    x = (mid + 1.5 * half * rng.uniform(-1, 1, (BASE, 3))).astype(np.float32)
    return VSet("base", x, unit_vectors(rng, BASE), rng.integers(0, 1 << 32, BASE, dtype=np.uint32))


def sphere_sets(name):
    """The classes aimed at nee_cone and the basis of nee_sample_sphere."""
    c, r, _ = table_spheres(name)
    rng = _rng(name, "sphere")
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    k = len(c)
    out = [_vset(name, "sphere: x inside", c[:, None, :] + (r[:, None, None] * rng.uniform(0, 0.99, (k, 16, 1)) * unit_vectors(rng, k * 16).reshape(k, 16, 3)), seeds=4)]
    # on the sphere along the six axes and its two float neighbours along the radius: d2 == rr exactly where the geometry is exact
    on = []
    for step in (0, -1, 1):
        for a in axes:
            on.append(c + ulps(r, step)[:, None] * a[None, :])
    out.append(_vset(name, "sphere: d2 == rr and neighbours", np.concatenate(on), seeds=max(1, 1024 // (18 * k) // 2)))
    far = [c + (np.float32(2.0 ** e) * r)[:, None] * np.array([[0.6, 0.0, 0.8]], np.float32) for e in range(1, 15)]
    out.append(_vset(name, "sphere: 2^k radii away", np.concatenate(far), seeds=max(1, 1024 // (14 * k))))
    along = np.concatenate([c - (3 * r)[:, None] * a[None, :] for a in axes])
    out.append(_vset(name, "sphere: w along an axis", along, seeds=max(1, 1024 // (6 * k))))
    # wn.z == +0 and -0: x in the sphere's z plane, with either sign of zero in x.z (a centre of -0 gives w.z = -0 - +0 = -0)
    ring = unit_vectors(rng, 16)
    ring[:, 2] = 0
    zero = np.concatenate([c[:, None, :] + 3 * r[:, None, None] * ring[None, :, :] for _ in range(2)], axis=1)
    zero[:, 16:, 2] = -zero[:, 16:, 2]
    zero[:, :16, 2] = np.abs(zero[:, :16, 2])
    out.append(_vset(name, "sphere: wn.z == +-0", zero, seeds=max(1, 1024 // (32 * k))))
    return out


def plane_sets(name):
    """The classes aimed at emit_plane_pa and the plane steps (scenes whose table holds a plane)."""
    P = table_planes(name)
    if not P:
        return []
    rng = _rng(name, "plane")
    inside, grazing, corners, far = [], [], [], []
    for e, i, b, u, v, n, t in P:
        for _ in range(8):
            a, c = rng.uniform(0.1, 0.4, 2).astype(np.float32)
            inside.append(b + a * u + c * v)
        # cos_l = h / D about 1e-8: D = 1000 plane sizes along u, h within a factor 2 either side
        D = np.float32(1000.0) * np.float32(np.linalg.norm(u))
        for f in np.geomspace(0.5, 2.0, 8):
            grazing.append(b + D * (u / np.float32(np.linalg.norm(u))) + np.float32(1e-8 * f) * D * n)
        corners += [b, b + u, b + v, b + u + v, b + n, b + u + v - n]
        ext = np.float32(1e6 * max(np.linalg.norm(u), np.linalg.norm(v)))
        far += [b + ext * w for w in unit_vectors(rng, 4)]
    m = len(P)
    return [_vset(name, "plane: x in the plane", inside, seeds=max(1, 1024 // (8 * m))), _vset(name, "plane: cos_l about 1e-8", grazing, seeds=max(1, 1024 // (8 * m))),
            _vset(name, "plane: x at a corner", corners, seeds=max(1, 1024 // (6 * m))), _vset(name, "plane: 1e6 sizes away", far, seeds=max(1, 1024 // (4 * m)))]


# ua + ub of a triangle's two draws is 1 exactly, its upper and its lower neighbour: the states before the draw of ua, from a search of
# the first 2^30 states (tools are not needed to repeat it: ua = float(s) / 2^32, ub = float(wang(s)) / 2^32)
SUM_ONE = (
    18696764, 24857821, 24905641, 25230765, 34039200, 38748126, 76450495, 83624066, 86374602, 90402689, 98826377, 107057376, 119375583, 130572521,
    132060779, 151617566, 161267379, 161979258, 167413486, 170912374, 174838467, 194158075, 195114227, 207910164, 209299451, 246088373, 252744449,
    257168551, 260627304, 284175272, 287676721, 295644811, 297136980, 299777986, 314015169, 317245700, 321618096, 342765528, 349217272, 360357579,
    380580690, 382184111, 394312648, 403713463, 416939989, 431596278, 468827211, 471747534,)
SUM_ABOVE = (
    27788349, 28113924, 29951878, 32048756, 38916946, 41544231, 51490764, 63290532, 80954015, 90428723, 96508632, 108098588, 119381592, 122989170,
    150494226, 160727088, 183780649, 191000049, 193798671, 199831571, 201432261, 204140049, 232177040, 233772034, 236007614, 258992459, 259115189,
    264655227, 265098193, 271111706, 285076864, 285365505, 289069227, 292071966, 313862936, 322107223, 323188639, 327371818, 339961514, 354798060,
    355496786, 365386701, 370136909, 378480270, 406422122, 416148406, 419793738, 421496234,)
SUM_BELOW = (
    19973688, 33047411, 35410392, 37960887, 43736386, 94772398, 97986907, 101085922, 116709970, 180559842, 181478374, 195012461, 281630658,
    304148634, 307658008, 318624780, 326591693, 336336980, 352304345, 353995970, 355731148, 378611012, 379799633, 407357920, 414176801, 418027753,
    440502418, 484977186, 513338854, 545423782, 550794317, 588301906, 615900739, 659367924, 659626954, 697653480, 710325298, 777985477, 798864424,
    810546196, 820264928, 834520665, 885470012, 932595506, 940273368, 958030587, 997686107, 1024666835,)


def triangle_sets(name):
    """Seeds whose cdf pick (select = 0) lands on a triangle and whose two draws then sum to 1, just above and just below."""
    P = [p for p in table_planes(name) if p[6] == TRIANGLE]
    if not P or not SUM_ONE:
        return []
    _, _, cdf, _, _ = emr.table(scene(name), 1)
    seeds = []
    for s2 in SUM_ONE + SUM_ABOVE + SUM_BELOW:
        s1 = unwang(s2)
        u = np.float32(s1) / np.float32(4294967296.0)
        if any((cdf[e - 1] if e else 0) <= u < cdf[e] for e, *_ in P):
            seeds.append(unwang(s1))
    if not seeds:
        return []
    rng = _rng(name, "triangle")
    lo, hi = bounds(name)
    reps = -(-64 // len(seeds))
    x = ((lo + hi) / 2 + (hi - lo) * rng.uniform(-1, 1, (len(seeds) * reps, 3))).astype(np.float32)
    return [VSet("plane: triangle ua + ub about 1", x, unit_vectors(rng, len(x)), np.tile(np.array(seeds, np.uint32), reps))]


def ellipse_sets(name):
    """Seeds whose cdf pick lands on an ellipse and whose rejection loop then takes four rounds or more (searched here, in numpy)."""
    P = [p for p in table_planes(name) if p[6] == ELLIPSE]
    if not P:
        return []
    _, _, cdf, _, _ = emr.table(scene(name), 1)
    seed = np.arange(1 << 20, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)
    u, st = draw(seed)
    good = np.zeros(len(seed), bool)
    for e, *_ in P:
        good |= (u >= (cdf[e - 1] if e else 0)) & (u < cdf[e])
    for _ in range(3):
        a, st = draw(st)
        b, st = draw(st)
        px, py = np.float32(-1) + np.float32(2) * a, np.float32(-1) + np.float32(2) * b
        good &= (px * px + py * py) >= np.float32(1)
    seeds = seed[good][:512]
    if len(seeds) < 64:
        return []
    rng = _rng(name, "ellipse")
    lo, hi = bounds(name)
    x = ((lo + hi) / 2 + (hi - lo) * rng.uniform(-1, 1, (len(seeds), 3))).astype(np.float32)
    return [VSet("plane: ellipse loop >= 4 rounds", x, unit_vectors(rng, len(x)), seeds)]


def tree_points(name, planes):
    """x for the tree's classes: every node's centre; on every node's sphere along +x and its neighbours; 1e10 and 1e20 scene sizes away
    (at 1e20, d2 is infinite and both importances are 0: the q fallback)."""
    t = tr.tree(scene(name), planes)
    c, r = t["sphere"][:, :3], t["sphere"][:, 3]
    if len(c) > 24:          # (a large tree: the root's levels and a spread of the rest)
        keep = sorted(set(range(8)) | set(np.linspace(8, len(c) - 1, 16).astype(int)))
        c, r = c[keep], r[keep]
    rng = _rng(name, "tree", planes)
    pts = {"tree: x at a node's centre": c}
    on = []
    for step in (0, -1, 1):
        on.append(np.stack([c[:, 0] + ulps(r, step), c[:, 1], c[:, 2]], axis=1))
    pts["tree: x on a node's sphere and neighbours"] = np.concatenate(on)
    sz = np.float32(size(name))
    mid = ((bounds(name)[0] + bounds(name)[1]) / 2).astype(np.float32)
    pts["tree: 1e10 sizes away"] = mid + np.float32(1e10) * sz * unit_vectors(rng, 32)
    pts["tree: 1e20 sizes away"] = mid + np.float32(1e20) * sz * unit_vectors(rng, 32)
    return pts


def root_ties(name, planes):
    """(x, seed) whose descent's first draw u equals the root's left probability pl from x exactly, and its two neighbours — the draw that
    `u < pl` sends right and `u <= pl` would send left.  u = float(s) / 2^32 is pl itself for s = pl 2^32 when that is an integer (pl >= 2^-8),
    and the seed is the state whose hash is s."""
    b = base_set(name)
    x = np.concatenate([b.x[:96]] + list(tree_points(name, planes).values())[:2])
    pl = tr.vertex_picks(scene(name), x, np.zeros(len(x), np.uint32), np.zeros(len(x), np.int32), planes=planes, root=True)[5]
    keep = (pl >= 2.0 ** -8) & (pl < 1)
    X, S = [], []
    for xi, p in zip(x[keep], pl[keep]):
        for q in (p, ulps(p, -1), ulps(p, 1)):
            s = float(q) * 4294967296.0
            if s == int(s) and 0 <= s < 4294967296.0:
                X.append(xi)
                S.append(unwang(int(s)))
    return np.array(X, np.float32).reshape(-1, 3), np.array(S, np.uint32)


def tree_sets(name, planes=0):
    out = []
    for cls, x in tree_points(name, planes).items():
        out.append(_vset(name, cls, x, seeds=max(2, -(-128 // len(x)))))
    x, seed = root_ties(name, planes)
    if len(x) >= 64:
        x, seed = x[:1023], seed[:1023]
        out.append(VSet("tree: u == pl at the root and neighbours", x, unit_vectors(_rng(name, "ties", planes), len(x)), seed))
    return out


def hemisphere_sets(name, planes, select):
    """nv chosen after the fact from the restatement's dir: dot(dir, nv) exactly 0, its two neighbours, and nv = -dir."""
    b = base_set(name)
    m = len(b.x)
    want, _ = reference(Pass("", name, "", 0, 0, select, planes, 1, None, None, b.x, b.nv, b.nv, np.zeros(m, np.float32), b.seed))
    ok = np.flatnonzero(want[:, 0] == 1)[:256]
    if len(ok) < 64:
        return []
    d = want[ok, 1:4].view(np.float32)
    x, seed = b.x[ok], b.seed[ok]
    zero = np.stack([-d[:, 1], d[:, 0], np.zeros(len(ok), np.float32)], axis=1)          # (-y) x + x y + 0 z: the two products cancel exactly
    tiny = np.float32(2.0 ** -100) * np.where(d[:, 2] >= 0, 1, -1).astype(np.float32)
    up, down = zero.copy(), zero.copy()
    up[:, 2], down[:, 2] = tiny, -tiny
    return [VSet("hemisphere: dot(dir, n) == 0 and neighbours", np.concatenate([x, x, x]), np.concatenate([zero, up, down]), np.concatenate([seed, seed, seed])),
            VSet("hemisphere: n = -dir", x, -d, seed)]


def sample_sets(name, planes, select):
    """Every vertex set routine 0 runs on for a scene's table."""
    sets = [base_set(name)] + sphere_sets(name) + hemisphere_sets(name, planes, select)
    if planes:
        sets += plane_sets(name)
        if not select:
            sets += triangle_sets(name) + ellipse_sets(name)
    if select:
        sets += tree_sets(name, planes)
    return sets


def _vs_of(vs, pb, key):
    """v and s of a vertex set under a Pb kind: r and fuzz (1), unused and g (2)."""
    rng = _rng(key, vs.name, pb)
    m = len(vs.x)
    v = unit_vectors(rng, m)
    if pb == 1:
        # (half of the mirror directions lie near nv, so that pg is not 0 everywhere)
        near = rng.random(m) < 0.5
        v[near] = (vs.nv[near] + 0.3 * v[near])
        return v.astype(np.float32), FUZZES[rng.integers(0, len(FUZZES), m)]
    if pb == 2:
        return v, GS[rng.integers(0, len(GS), m)]
    return v, np.zeros(m, np.float32)


# ---- the passes -----------------------------------------------------------------------------------------------------------------------
def _chunks(p):
    m = len(p.x)
    if m <= MAX_CALL:
        return [p]
    return [p._replace(label=f"{p.label} [{a // MAX_CALL}]", x=p.x[a:a + MAX_CALL], nv=p.nv[a:a + MAX_CALL], v=p.v[a:a + MAX_CALL], s=p.s[a:a + MAX_CALL],
                       seed=p.seed[a:a + MAX_CALL]) for a in range(0, m, MAX_CALL)]


def sample_passes(name):
    """Routine 0: every table of the scene, mis 1 and 0, the three Pb kinds, over sample_sets."""
    out = []
    for planes, select in table_configs(name):
        for vs in sample_sets(name, planes, select):
            for mis in (1, 0):
                for pb in (0, 1, 2):
                    if vs.name != "base" and mis == 0 and pb == 2:
                        continue          # (the aimed classes under the phase density: with the power heuristic only)
                    v, s = _vs_of(vs, pb, name)
                    out.append(Pass(f"{name}: light_sample, planes={planes} select={select} mis={mis} pb={pb}, {vs.name}", name, vs.name, 0, pb, select, planes,
                                    mis, None, None, vs.x, vs.nv, v, s, vs.seed))
    return out


def _env_seeds():
    """Random seeds, and those whose first draw is 1 - 2^-24 (the last row) and 1 (no row)."""
    rng = _rng("env seeds")
    seeds = rng.integers(0, 1 << 32, BASE, dtype=np.uint32)
    seeds[:32] = unwang(0xffffff00)
    seeds[32:64] = unwang(0xffffffff)
    return seeds


def env_passes():
    """Routine 1 and 3 on the two environments: mode 1 and 2, the three Pb kinds; the directions of env_directions."""
    out = []
    rng = _rng("env")
    seeds = _env_seeds()
    nv = unit_vectors(rng, BASE)
    x = rng.uniform(-5, 5, (BASE, 3)).astype(np.float32)
    vs = VSet("env: seeds", x, nv, seeds)
    for which in ("sun", "two"):
        rgb, params = environment(which)
        d = env_directions(rgb.shape[0], np.array(params.get("rot", np.eye(3).ravel()), np.float32).reshape(3, 3))
        for mode in (1, 2):
            ep = dict(params, mode=mode)
            for pb in (0, 1, 2):
                v, s = _vs_of(vs, pb, which)
                out.append(Pass(f"env {which}: light_sample, mode={mode} pb={pb}", "lamp", "env: seeds", 1, pb, 0, 0, 1, which, ep, x, nv, v, s, seeds))
            # the found side of the environment's own samples: every ok dir of routine 1 (PbDiffuse and PbGlossy) as the miss's direction
            fed = []
            for pb in (0, 1):
                v, s = _vs_of(vs, pb, which)
                want, _ = reference(Pass("", "lamp", "env: seeds", 1, pb, 0, 0, 1, which, ep, x, nv, v, s, seeds))
                fed.append(want[want[:, 0] == 1, 1:4].view(np.float32))
            fed = np.concatenate(fed)
            m = len(fed)
            carry = np.zeros((m, 3), np.float32)
            carry[:, 0] = CARRIES[np.arange(m) % len(CARRIES)]
            out.append(Pass(f"env {which}: light_miss of the ok samples, mode={mode}", "lamp", "found: ok samples of the environment fed back", 3, 0, 0, 0, 1, which,
                            dict(ep, camera_visible=1), np.zeros((m, 3), np.float32), carry, fed, np.zeros(m, np.float32), np.zeros(m, np.uint32)))
            for vis in (0, 1):
                m = len(d)
                carry = np.zeros((m, 3), np.float32)
                carry[:, 0] = CARRIES[np.arange(m) % len(CARRIES)]
                out.append(Pass(f"env {which}: light_miss, mode={mode} camera_visible={vis}", "lamp", "env: folds, edges and axes", 3, 0, 0, 0, 1, which,
                                dict(ep, camera_visible=vis), np.zeros((m, 3), np.float32), carry, d, np.zeros(m, np.float32), np.zeros(m, np.uint32)))
    return out


CARRIES = np.array([0.0, NEE_PB, 0.37, 2.0 ** -140, -0.0, 3.5e4, 1e-30], np.float32)          # none, diffuse, a pg, a denormal, -0, large and small pg


def env_directions(n, rot):
    """World directions whose environment-frame direction lies on the octahedron's folds and texel edges (u or v = k h - 1 exactly), on
    d.y == +-0, along the axes — and random ones."""
    h = 2.0 / n
    ks = (np.arange(n + 1) * h - 1).astype(np.float32)
    rng = _rng("env dirs", n)
    pts = []
    for u in ks:
        for v in np.concatenate([ks, rng.uniform(-1, 1, 4).astype(np.float32)]):
            for a, b in ((u, v), (v, u)):
                y = (np.float32(1) - abs(a)) - abs(b)
                if y >= 0:
                    pts.append((a, y, b))
                else:
                    pts.append(((np.float32(1) - abs(b)) * (1 if a >= 0 else -1), y, (np.float32(1) - abs(a)) * (1 if b >= 0 else -1)))
    pts = np.array(pts, np.float32)
    fold = pts[pts[:, 1] == 0].copy()
    fold[:, 1] = -0.0
    e = np.concatenate([pts, fold, np.eye(3, dtype=np.float32), -np.eye(3, dtype=np.float32), unit_vectors(rng, 256)])
    # the world direction of an environment-frame direction: the transpose of rot (rows: world → environment); under the identity it is exact
    w = (e.astype(np.float64) @ rot.astype(np.float64)).astype(np.float32) if not (rot == np.eye(3)).all() else e
    return np.concatenate([w, e])


def pick_passes(name):
    """Routine 4: u at every cdf entry, its neighbours, 0, 1 - 2^-24 and 1 (no entry); emit_find / nee_find of every primitive code, one
    below the first and one above the last; on the trees, tree_pick and tree_pmf of every entry from tree_points."""
    out = []
    d = scene(name).desc
    for planes, select in table_configs(name):
        kind, idx, cdf, pmf, area = emr.table(scene(name), planes)
        two_kind = planes == 1
        us = np.concatenate([cdf, ulps(cdf, -1), ulps(cdf[:-1], 1), np.array([0.0, 1 - 2.0 ** -24, 1.0], np.float32)])
        if two_kind:
            codes = np.concatenate([2 * np.arange(-1, d.num_spheres + 2), 2 * np.arange(-1, d.num_planes + 2) + 1]).astype(np.int32)
        else:
            codes = np.arange(-2, d.num_spheres + 2, dtype=np.int32)
        if select:
            X = np.concatenate(list(tree_points(name, planes).values()))
            cls = np.concatenate([[k] * len(v) for k, v in tree_points(name, planes).items()])
            n_e = len(kind)
            x = np.repeat(X, n_e, axis=0)
            e_in = np.tile(np.arange(n_e), len(X))
            m = len(x)
            rng = _rng(name, "picks", planes)
            nv = np.zeros((m, 3), np.float32)
            nv[:, 0] = e_in
            p = Pass(f"{name}: picks, planes={planes} select=1", name, "tree: every entry from every point", 4, 0, 1, planes, 1, None, None, x, nv, np.zeros((m, 3), np.float32),
                     us[np.arange(m) % len(us)], rng.integers(0, 1 << 32, m, dtype=np.uint32))
            out += _chunks(p)
            tx, ts = root_ties(name, planes)
            if len(tx) >= 64:
                m = len(tx)
                out.append(Pass(f"{name}: picks at the root's ties, planes={planes} select=1", name, "tree: u == pl at the root and neighbours", 4, 0, 1, planes, 1, None, None,
                                tx, np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), np.zeros(m, np.float32), ts))
            m = max(len(us), len(codes), 64)
            out.append(Pass(f"{name}: finds, planes={planes} select=1", name, "table: cdf entries and every code", 4, 0, 1, planes, 1, None, None, np.zeros((m, 3), np.float32),
                            np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), us[np.arange(m) % len(us)], codes[np.arange(m) % len(codes)].astype(np.uint32)))
        else:
            m = max(len(us), len(codes), 64)
            out.append(Pass(f"{name}: picks, planes={planes} select=0", name, "table: cdf entries and every code", 4, 0, 0, planes, 1, None, None, np.zeros((m, 3), np.float32),
                            np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), us[np.arange(m) % len(us)], codes[np.arange(m) % len(codes)].astype(np.uint32)))
    return out


def density_passes():
    """Routine 5: gloss_pg at disc == 0, at t1 == 0, their neighbours, every fuzz of FUZZES, w = +-r; PbPhase at every g, w parallel and
    perpendicular to ud, |w| in {2^-60, 1, 2^60}."""
    rng = _rng("densities")
    X, N, V, S, cls = [], [], [], [], []

    def add(name, w, ud, r, s):
        w, ud, r = (np.asarray(q, np.float32).reshape(-1, 3) for q in (w, ud, r))
        m = len(w)
        X.append(w); N.append(np.broadcast_to(ud, (m, 3))); V.append(np.broadcast_to(r, (m, 3))); S.append(np.broadcast_to(np.asarray(s, np.float32), (m,)))
        cls.extend([name] * m)
    ex = np.array([1, 0, 0], np.float32)
    none = np.zeros(3, np.float32)          # ud of the glossy classes: ph is then finite whatever the fuzz that stands in for g
    # disc = (c c - 1) + ff: 0 exactly at c = 0, fuzz = 1, and wherever a c next to sqrt(1 - ff) squares to 1 - ff
    for fuzz in FUZZES:
        for k in range(-3, 4):
            add("glossy: disc about 0", [0.0, 1.0, 0.0], none, ex, ulps(fuzz, k) if fuzz == 1 else fuzz)
        if fuzz < 1:
            c0 = np.float32(np.sqrt(1 - float(fuzz) ** 2))
            for k in range(-4, 5):
                c = ulps(c0, k)
                add("glossy: disc about 0", [c, np.float32(np.sqrt(max(0.0, 1 - float(c) ** 2))), 0.0], none, ex, fuzz)
    # t1 = c - sqrt((c c - 1) + ff): 0 at fuzz = 1 wherever sqrt(c c) == c, either side of 0 at the neighbours of 1
    for c in np.concatenate([rng.uniform(0.01, 1, 24).astype(np.float32), np.array([0.25, 0.5, 1.0], np.float32)]):
        for k in (-2, -1, 0, 1, 2):
            add("glossy: t1 about 0", [c, np.float32(np.sqrt(max(0.0, 1 - float(c) ** 2))), 0.0], none, ex, ulps(np.float32(1), k))
    # … and exactly 0 where c = k / 4096: c c, (c c - 1) + 1 and its root are exact, so s == c; the two branches' values then differ by the
    # rounding of 3 (c c) alone
    for k in rng.integers(2048, 4096, 256):
        c = np.float32(k / 4096.0)
        add("glossy: t1 == 0 exactly", [c, np.float32(np.sqrt(1 - float(c) ** 2)), 0.0], none, ex, 1.0)
    for fuzz in FUZZES:
        r = unit_vectors(rng, 32)
        add("glossy: every fuzz", unit_vectors(rng, 32), none, r, fuzz)
        near = r + 0.5 * float(fuzz) * unit_vectors(rng, 32)
        add("glossy: every fuzz", near / np.linalg.norm(near, axis=1, keepdims=True), none, r, fuzz)
        add("glossy: w = +-r", np.concatenate([r, -r]), none, np.concatenate([r, r]), fuzz)
    for g in GS:
        ud = unit_vectors(rng, 16)
        perp = np.cross(ud, unit_vectors(rng, 16)).astype(np.float32)
        for scale in (2.0 ** -60, 1.0, 2.0 ** 60):
            sc = np.float32(scale)
            add("phase: w parallel to ud", np.concatenate([sc * ud, -sc * ud]), np.concatenate([ud, ud]), np.concatenate([ud, ud]), g)
            add("phase: w perpendicular to ud", sc * perp, ud, ud, g)
            add("phase: random w", sc * unit_vectors(rng, 16), ud, ud, g)
    x, nv, v, s = np.concatenate(X).astype(np.float32), np.concatenate(N).astype(np.float32), np.concatenate(V).astype(np.float32), np.concatenate(S).astype(np.float32)
    return [Pass("densities: gloss_pg and PbPhase", "lamp", np.array(cls), 5, 0, 0, 0, 1, None, None, x, nv, v, s, np.zeros(len(x), np.uint32))]


def found_passes(name):
    """Routine 2.  For every ok sample of routine 0 under PbDiffuse, the same (x, dir, code) fed back — closest from the plane's equation
    (the routine reads it for a plane alone) — with the carried values of CARRIES in turn; random rays at every primitive's code, table
    entry or not; and rays from on a table sphere and its two float neighbours that find that sphere, under every carried value."""
    out = []
    d = scene(name).desc
    for planes, select in table_configs(name):
        for mis in (1, 0):
            X, V, S, C = [], [], [], []
            for vs in sample_sets(name, planes, select):
                v, s = _vs_of(vs, 0, name)
                want, _ = reference(Pass("", name, vs.name, 0, 0, select, planes, mis, None, None, vs.x, vs.nv, v, s, vs.seed))
                ok = want[:, 0] == 1
                X.append(vs.x[ok]); V.append(want[ok, 1:4].view(np.float32)); C.append(want[ok, 7])
            x, v, code = np.concatenate(X), np.concatenate(V), np.concatenate(C).astype(np.uint32)
            rng = _rng(name, "found", planes, select, mis)
            # hits on every primitive, table entry or not: random rays with that code
            k = 1024
            codes = np.concatenate([2 * np.arange(d.num_spheres), 2 * np.arange(d.num_planes) + 1])
            lo, hi = bounds(name)
            x = np.concatenate([x, ((lo + hi) / 2 + (hi - lo) * rng.uniform(-1, 1, (k, 3))).astype(np.float32)])
            v = np.concatenate([v, unit_vectors(rng, k)])
            code = np.concatenate([code, codes[rng.integers(0, len(codes), k)].astype(np.uint32)])
            # the found side's own cone: rays that leave a point on, one ulp inside and one ulp outside a table sphere and find that sphere
            sc, sr, se = table_spheres(name, planes)
            sidx = emr.table(scene(name), planes)[1][se]
            axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
            on = np.concatenate([sc + ulps(sr, step)[:, None] * a[None, :] for step in (0, -1, 1) for a in axes])
            reps = len(CARRIES)
            x = np.concatenate([x, np.repeat(on, reps, axis=0)])
            v = np.concatenate([v, unit_vectors(rng, len(on) * reps)])
            code = np.concatenate([code, np.repeat(np.tile(2 * sidx, 18), reps).astype(np.uint32)])
            m = len(x)
            s = closest_of(name, x, v, code)
            nv = np.zeros((m, 3), np.float32)
            nv[:, 0] = CARRIES[np.arange(m) % len(CARRIES)]
            out += _chunks(Pass(f"{name}: light_emitted, planes={planes} select={select} mis={mis}", name, "found: ok samples fed back, and every primitive", 2, 0, select,
                                planes, mis, None, None, x, nv, v, s, code))
    return out


def closest_of(name, x, v, code):
    """The t at which the ray (x, v) meets the plane of a plane's code (float64 arithmetic, rounded); 1 for a sphere's code, which the
    routine does not read."""
    d = scene(name).desc
    t = np.ones(len(x), np.float32)
    for k in np.flatnonzero(code & 1):
        p = d.planes[int(code[k]) >> 1]
        n, b = np.array(p.normal.e[:], np.float64), np.array(p.base.e[:], np.float64)
        den = n @ v[k].astype(np.float64)
        t[k] = np.float32((n @ (b - x[k])) / den) if den != 0 else np.float32(1)
    return np.where(np.isfinite(t), t, np.float32(1)).astype(np.float32)


def all_passes():
    out = []
    for name in SCENES:
        out += sample_passes(name) + pick_passes(name) + found_passes(name)
    return out + env_passes() + density_passes()


# ---- the CPU statement of a pass ---------------------------------------------------------------------------------------------------------
def reference(p, tallies=True, densities=False):
    """(m, 16) uint32 as the hook writes them, and the tallies' bits of every vertex (zeros with tallies=False); densities=True adds (pl, pb)."""
    host, cam = scene(p.scene), camera(p.scene)
    rgb, ep = (None, None)
    if p.env is not None:
        rgb, ep = environment(p.env)[0], p.env_params
    kw = dict(select=p.select, nee_mis=p.mis, planes=p.planes, rgb=rgb, env_params=ep)
    m = len(p.x)
    if p.routine == 4:
        out, flags = np.zeros((m, 16), np.uint32), np.zeros(m, np.uint32)
        entry, found = emr.vertex_picks(host, p.s, p.seed.view(np.int32), planes=p.planes)
        out[:, 0], out[:, 5] = entry.view(np.uint32), found.view(np.uint32)
        flags |= np.where(entry >= len(emr.table(host, p.planes)[0]), np.uint32(1 << 6), np.uint32(0)).astype(np.uint32)
        if p.select:
            e, pr, after, pmf, fell = tr.vertex_picks(host, p.x, p.seed, p.nv[:, 0].astype(np.int32), planes=p.planes)
            out[:, 1], out[:, 2], out[:, 3], out[:, 4] = e.view(np.uint32), pr.view(np.uint32), after, pmf.view(np.uint32)
            flags |= np.where(fell != 0, np.uint32(1 << 4), np.uint32(0)).astype(np.uint32)
        return (out, flags if tallies else np.zeros(m, np.uint32)) + ((np.zeros((m, 2), np.float32),) if densities else ())
    if p.pb == 2 or p.routine == 5:
        out, flags = mr.vertices(host, cam, p.routine, p.x, p.nv, p.s, p.seed, AB, tallies=tallies, **kw)
        if p.routine == 5:
            out[:, 0] = glr.vertices(host, cam, 5, 0, p.x, p.nv, p.v, p.s, p.seed, AB, tallies=tallies, **kw)[0][:, 0]
        return (out, flags) + ((np.zeros((m, 2), np.float32),) if densities else ())
    return glr.vertices(host, cam, p.routine, p.pb, p.x, p.nv, p.v, p.s, p.seed, AB, tallies=tallies, densities=densities, **kw)
