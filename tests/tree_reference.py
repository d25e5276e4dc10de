"""CPU reference of rt_nee_params.select — the light tree of rt_render_nee / rt_render_lit (TEST INFRASTRUCTURE):
tests/cpu_native/tree_ref.c, which includes emit_ref.c (and through it oracle/rt_oracle.c), built into a shared library (gcc
-ffp-contract=off, like the oracle) the first time it is needed, in a temporary directory.  Threads split the rows; every pixel is still
summed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import rtp_bindings as rb

COLUMNS = ("sphere", "weight", "q", "left", "right", "entry", "path", "depth")
# tree_ref.c's tallies, in its order (trace(stats=True) returns the first two, trace(stats="all") a dict of all of them)
STATS = ("inside_parent", "weighted", "drop_inside", "drop_omega", "drop_cos", "shadow_other_entry", "shadow_non_table", "hit_pl_zero",
         "q_fallback", "pick_none")


class TreeCfg(C.Structure):
    """tree_ref.c's tree_cfg."""
    _fields_ = [("base", emr.EmitCfg), ("select", C.c_int32)]


def lib():
    l = cpu_ref.build("tree_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(TreeCfg)
    l.tree_columns.restype = C.c_int32
    l.tree_columns.argtypes = [desc, C.c_int32] + [C.c_void_p] * 8 + [C.POINTER(C.c_int32)]
    l.tree_pmf_points.restype = None
    l.tree_pmf_points.argtypes = [desc, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
    l.tree_pick_counts.restype = C.c_int64
    l.tree_pick_counts.argtypes = [desc, C.c_int32, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]
    l.tree_vertex_picks.restype = None
    l.tree_vertex_picks.argtypes = [desc, C.c_int32, C.c_int64] + [C.c_void_p] * 9
    l.tree_trace.restype = None
    l.tree_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p]
    l.tree_frame.restype = None
    l.tree_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def tree(host, planes=0):
    """The tree over the table of sample_planes = planes: a dict of the columns DeviceScene.nee_light_tree returns."""
    cap = 2 * (host.desc.num_spheres + host.desc.num_planes) + 1
    t = {"sphere": np.zeros((cap, 4), np.float32), "weight": np.zeros(cap, np.float32), "q": np.zeros(cap, np.float32),
         "left": np.zeros(cap, np.int32), "right": np.zeros(cap, np.int32), "entry": np.zeros(cap, np.int32),
         "path": np.zeros(cap, np.uint32), "depth": np.zeros(cap, np.int32)}
    ne = C.c_int32()
    nn = lib().tree_columns(C.byref(host.desc), planes, *(t[k].ctypes.data for k in COLUMNS), C.byref(ne))
    return {k: (v[:ne.value] if k in ("path", "depth") else v[:nn]).copy() for k, v in t.items()}


def pmf(host, points, planes=0):
    """pmf_e(x) by the path product: points (m, 3) → (m, N) float32."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(emr.table(host, planes)[0])
    out = np.zeros((points.shape[0], n), np.float32)
    lib().tree_pmf_points(C.byref(host.desc), planes, points.shape[0], points.ctypes.data, out.ctypes.data)
    return out


def pick_counts(host, point, draws, seed, planes=0):
    """`draws` picks from one point → (counts (N,) int64, how many picks' p was not their entry's path product bit for bit)."""
    point = np.ascontiguousarray(point, dtype=np.float32)
    counts = np.zeros(len(emr.table(host, planes)[0]), np.int64)
    bad = lib().tree_pick_counts(C.byref(host.desc), planes, point.ctypes.data, draws, seed, counts.ctypes.data)
    return counts, bad


def vertex_picks(host, x, seed, e_in, planes=0, root=False):
    """Per vertex: tree_pick from x on the stream that starts at seed, and tree_pmf of entry e_in from the same x →
    (entry, p, seed after, pmf, fell: bit 0 the descent's, bit 1 the product's fallback); root=True adds the root's left probability."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3)
    seed, e_in = np.ascontiguousarray(seed, dtype=np.uint32).ravel(), np.ascontiguousarray(e_in, dtype=np.int32).ravel()
    m = len(x)
    assert len(seed) == len(e_in) == m and (e_in >= 0).all() and (e_in < max(1, len(emr.table(host, planes)[0]))).all()
    entry, p, after = np.zeros(m, np.int32), np.zeros(m, np.float32), np.zeros(m, np.uint32)
    pmf_, fell, pl = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.float32)
    lib().tree_vertex_picks(C.byref(host.desc), planes, m, x.ctypes.data, seed.ctypes.data, e_in.ctypes.data, entry.ctypes.data, p.ctypes.data,
                            after.ctypes.data, pmf_.ctypes.data, fell.ctypes.data, pl.ctypes.data if root else None)
    return (entry, p, after, pmf_, fell) + ((pl,) if root else ())


def _cfg(select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params):
    base, keep = emr._cfg(cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    c = TreeCfg()
    c.base = base
    c.select = select
    return c, keep


def trace(host, cam, ijs, select=1, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=0, rgb=None, env_params=None, linear=True, stats=False):
    """emit_reference.trace with the pick by select.  stats=True adds (sampling vertices inside the sphere of their picked leaf's parent,
    weighted BSDF hits on table entries); stats="all" adds a dict of every tally in STATS instead."""
    c, keep = _cfg(select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad, rays = np.empty((m, 3), np.float32), np.empty(m, np.int32)
    seeds, nee, env = np.empty(m, np.uint32), np.empty(m, np.uint32), np.empty(m, np.uint32)
    st = np.zeros(len(STATS), np.int64)
    lib().tree_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, seeds.ctypes.data,
                     nee.ctypes.data, env.ctypes.data, 1 if linear else 0, st.ctypes.data)
    if stats == "all":
        return rad, rays, seeds, nee, env, {k: int(x) for k, x in zip(STATS, st)}
    return (rad, rays, seeds, nee, env) + ((tuple(int(x) for x in st[:2]),) if stats else ())


def frame(host, cam, select=1, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=0, rgb=None, env_params=None, shard=None, sample_first=0,
          threads=16, moments=False):
    """emit_reference.frame with the pick by select."""
    c, keep = _cfg(select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().tree_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                     mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb


# ---- an independent build of the tree: numpy, double, from the scene's arrays ----------------------------------------------------------
def numpy_tree(host, planes):
    """The header's tree over the table of sample_planes = planes, as a dict of float64 / int columns (nothing rounded to float32)."""
    d = host.desc
    kind, idx, _, _, area = emr.table(host, planes)
    n = len(kind)
    c, rho, w = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    for e in range(n):
        if kind[e] == 0:
            s = d.spheres[int(idx[e])]
            c[e], rho[e] = np.array(s.center.e[:], np.float64), s.radius
            w[e] = np.float64(np.array(d.materials[s.material_idx].emit.e[:], np.float64).sum()) * np.float64(s.radius) ** 2
        else:
            p = d.planes[int(idx[e])]
            b, u, v = (np.array(x.e[:], np.float64) for x in (p.base, p.u, p.v))
            if p.type == 2:
                c[e] = b + (u + v) / 3
                rho[e] = max(np.linalg.norm(q - c[e]) for q in (b, b + u, b + v))
            else:
                c[e] = b + u / 2 + v / 2
                rho[e] = max(np.linalg.norm(u + v), np.linalg.norm(u - v)) / 2
            w[e] = np.array(d.materials[p.material_idx].emit.e[:], np.float64).sum() * np.float64(area[e]) / np.pi
    cols = {k: [] for k in ("centre", "radius", "weight", "q", "left", "right", "entry")}
    path, depth = np.zeros(n, np.uint32), np.zeros(n, np.int32)

    def node(S, bits, level):
        me = len(cols["entry"])
        lo, hi = (c[S] - rho[S, None]).min(0), (c[S] + rho[S, None]).max(0)
        m = (lo + hi) / 2
        for k, v in (("centre", m), ("radius", (np.linalg.norm(c[S] - m, axis=1) + rho[S]).max()), ("weight", w[S].sum() / w.sum()), ("q", 0.0),
                     ("left", -1), ("right", -1), ("entry", -1)):
            cols[k].append(v)
        if len(S) == 1:
            cols["entry"][me] = int(S[0])
            path[S[0]], depth[S[0]] = bits, level
            return me
        extent = c[S].max(0) - c[S].min(0)
        axis = int(np.argmax(extent))                      # (the first of equal maxima: x, then y, then z)
        S = S[np.argsort(c[S, axis], kind="stable")]
        nl = (len(S) + 1) // 2
        cols["left"][me] = node(S[:nl], bits, level + 1)
        cols["right"][me] = node(S[nl:], bits | (1 << level), level + 1)
        cols["q"][me] = w[S[:nl]].sum() / w[S].sum()
        return me
    if n:
        node(np.arange(n), 0, 0)
    out = {k: np.array(v) for k, v in cols.items()}
    out.update(path=path, depth=depth, c=c, rho=rho)
    return out
