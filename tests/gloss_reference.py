"""CPU reference of the glossy switch — rt_nee_params.glossy / rt_env_params.glossy in rt_render_nee, rt_render_env and rt_render_lit
(TEST INFRASTRUCTURE): tests/cpu_native/gloss_ref.c, which includes tree_ref.c (and through it emit_ref.c and oracle/rt_oracle.c), built
into a shared library (gcc -ffp-contract=off, like the oracle) the first time it is needed, in a temporary directory.  Threads split the
rows; every pixel is still summed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import rtp_bindings as rb
import tree_reference as tr

# gloss_ref.c's per-sample tallies, in its order
COUNTERS = ("samples", "absorbed", "pg_zero", "fuzz_gt1", "hit_carried", "miss_carried")


class GlossCfg(C.Structure):
    """gloss_ref.c's gloss_cfg."""
    _fields_ = [("base", tr.TreeCfg), ("glossy_nee", C.c_int32), ("glossy_env", C.c_int32)]


def lib():
    l = cpu_ref.build("gloss_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(GlossCfg)
    l.gloss_pg_many.restype = None
    l.gloss_pg_many.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    l.gloss_lobe_draws.restype = None
    l.gloss_lobe_draws.argtypes = [C.c_int64, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p]
    l.gloss_trace.restype = None
    l.gloss_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p]
    l.gloss_vertices.restype = None
    l.gloss_vertices.argtypes = [desc, cam, cfg, C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 9
    l.gloss_frame.restype = None
    l.gloss_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def pg(w, r, fuzz):
    """pg(w; r, fuzz) in the header's float32 order: w (m, 3), r (3,) → (m,) float32."""
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1, 3)
    r = np.ascontiguousarray(r, dtype=np.float32)
    out = np.empty(w.shape[0], np.float32)
    lib().gloss_pg_many(w.shape[0], w.ctypes.data, r.ctypes.data, fuzz, out.ctypes.data)
    return out


def lobe_draws(r, fuzz, count, seed):
    """dot(unit(r + fuzz * random_in_unit_sphere), r) of `count` draws of the oracle's own generator: (count,) float64."""
    r = np.ascontiguousarray(r, dtype=np.float32)
    out = np.empty(count, np.float64)
    lib().gloss_lobe_draws(count, r.ctypes.data, fuzz, seed, out.ctypes.data)
    return out


# gloss_ref.c's per-vertex tallies (the TL_ bits, in its order)
TALLIES = ("cone refused: inside", "om == 0", "hemisphere refused", "pb == 0 refused", "fallback taken", "triangle folded", "no entry", "pl^2 overflows",
           "plane refused: cos_l < 1e-8", "plane refused: the point is the vertex", "ellipse loop >= 4 rounds", "ok", "found: weighted", "found: pl == 0",
           "found: not a table entry", "basis: wn.z == +-0", "basis: wn.x == wn.y == 0", "om == 2^-24", "found: carry off", "a NaN in c", "triangle: ua + ub == 1")


def vertex_arrays(x, nv, v, s, seed, ab):
    """The per-vertex inputs as the C side and the developer hook take them: (m, 3) float32 three times, (m,) float32, (m,) uint32, (6,)."""
    x, nv, v = (np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3) for q in (x, nv, v))
    s, seed = np.ascontiguousarray(s, dtype=np.float32).ravel(), np.ascontiguousarray(seed, dtype=np.uint32).ravel()
    ab = np.ascontiguousarray(ab, dtype=np.float32).ravel()
    assert len(x) == len(nv) == len(v) == len(s) == len(seed) and ab.shape == (6,)
    return x, nv, v, s, seed, ab


def vertices(host, cam, routine, pb_kind, x, nv, v, s, seed, ab, glossy=1, glossy_env=1, select=0, nee_mis=1, planes=0, rgb=None, env_params=None,
             tallies=True, densities=False):
    """gloss_vertices: routine 0, 1, 2, 3 or 5 of rt_debug_light_vertices under Pb kind 0 or 1 on the CPU → (m, 16) uint32, the TL_ bits of
    each vertex (zeros with tallies=False: the C side is then handed no place to count) and, with densities=True, (pl, pb) of each weight."""
    c, keep = _cfg(glossy, glossy_env, select, None, None, True, nee_mis, planes, rgb, env_params)
    x, nv, v, s, seed, ab = vertex_arrays(x, nv, v, s, seed, ab)
    m = len(x)
    out, flags, plpb = np.zeros((m, 16), np.uint32), np.zeros(m, np.uint32), np.zeros((m, 2), np.float32)
    lib().gloss_vertices(C.byref(host.desc), C.byref(cam), C.byref(c), routine, pb_kind, m, x.ctypes.data, nv.ctypes.data, v.ctypes.data, s.ctypes.data,
                         seed.ctypes.data, ab.ctypes.data, out.ctypes.data, flags.ctypes.data if tallies else None, plpb.ctypes.data if densities else None)
    return (out, flags, plpb) if densities else (out, flags)


def _cfg(glossy, glossy_env, select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params):
    base, keep = tr._cfg(select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    c = GlossCfg()
    c.base = base
    c.glossy_nee, c.glossy_env = glossy, glossy_env
    return c, keep


def trace(host, cam, ijs, glossy=1, glossy_env=0, select=0, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=0, rgb=None, env_params=None,
          linear=True):
    """tree_reference.trace with the glossy switches (glossy: the emitters', glossy_env: the environment's) →
    (radiance, rays, seeds, nee seeds, env seeds, counters (m, 6) int32 in the order of COUNTERS)."""
    c, keep = _cfg(glossy, glossy_env, select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad, rays = np.empty((m, 3), np.float32), np.empty(m, np.int32)
    seeds, nee, env = np.empty(m, np.uint32), np.empty(m, np.uint32), np.empty(m, np.uint32)
    cnt = np.zeros((m, len(COUNTERS)), np.int32)
    lib().gloss_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, seeds.ctypes.data,
                      nee.ctypes.data, env.ctypes.data, 1 if linear else 0, cnt.ctypes.data)
    return rad, rays, seeds, nee, env, cnt


def frame(host, cam, glossy=1, glossy_env=0, select=0, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=0, rgb=None, env_params=None,
          shard=None, sample_first=0, threads=16, moments=False):
    """tree_reference.frame with the glossy switches."""
    c, keep = _cfg(glossy, glossy_env, select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().gloss_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                      mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
