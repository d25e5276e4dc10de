"""CPU reference of rt_render_medium / rt_trace_samples_medium (TEST INFRASTRUCTURE): tests/cpu_native/medium_ref.c, which includes
gloss_ref.c (and through it tree_ref.c, emit_ref.c and oracle/rt_oracle.c) and log_ref.h, built into a shared library (gcc
-ffp-contract=off, like the oracle) the first time it is needed, in a temporary directory.  Threads split the rows; every pixel is still
summed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import gloss_reference as glr
import rtp_bindings as rb

# how a path ended (medium_ref.c's med_out.end)
END_MISS, END_DEPTH, END_ABSORBED, END_BLACK = range(4)
# medium_ref.c's tallies, in its order (trace(stats=True) adds a dict of them; they only count)
STATS = ("events", "interval_empty", "origin_inside", "box_parallel_in", "box_parallel_out", "u_zero", "event_at_depth_cut", "black", "tr_emitter",
         "tr_env", "env_suppressed", "carry_hit", "carry_miss", "glossy_inside", "event_first_ray")


class MediumCfg(C.Structure):
    """medium_ref.c's medium_cfg."""
    _fields_ = [("base", glr.GlossCfg), ("medium", rb.MediumParams)]


def lib():
    l = cpu_ref.build("medium_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(MediumCfg)
    l.medium_ph_many.restype = None
    l.medium_ph_many.argtypes = [C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
    l.medium_cos_draws.restype = None
    l.medium_cos_draws.argtypes = [C.c_int64, C.c_float, C.c_uint32, C.c_void_p]
    l.medium_intervals.restype = None
    l.medium_intervals.argtypes = [C.POINTER(rb.MediumParams), C.c_int64] + [C.c_void_p] * 6
    l.medium_vertices.restype = None
    l.medium_vertices.argtypes = [desc, cam, C.POINTER(glr.GlossCfg), C.c_int32, C.c_int64] + [C.c_void_p] * 7
    l.medium_trace.restype = None
    l.medium_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32]
    l.medium_trace_stats.restype = None
    l.medium_trace_stats.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p]
    l.medium_frame.restype = None
    l.medium_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def medium_struct(medium):
    """None → no medium (sigma_t 0, written out: the reference does not need the library); a dict → rb.MediumParams by the same rules as
    rb.medium_params; a MediumParams as it is."""
    if isinstance(medium, rb.MediumParams):
        return medium
    kw = dict(medium or {})
    p = rb.MediumParams()
    p.sigma_t = float(kw.get("sigma_t", 0.0))
    alb = np.broadcast_to(np.asarray(kw.get("albedo", 1.0), dtype=np.float32), (3,))
    for k in range(3):
        p.albedo[k] = float(alb[k])
    p.g = float(kw.get("g", 0.0))
    if kw.get("ball") is not None:
        p.region = 1
        for k in range(3):
            p.a[k] = float(kw["ball"][k])
        p.b[0] = float(kw["ball"][3])
    elif kw.get("box") is not None:
        p.region = 2
        for k in range(3):
            p.a[k] = float(kw["box"][k])
            p.b[k] = float(kw["box"][3 + k])
    return p


def ph(g, c):
    """ph(c) in the header's float32 order: c (m,) → (m,) float32."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    out = np.empty(c.shape[0], np.float32)
    lib().medium_ph_many(c.shape[0], g, c.ctypes.data, out.ctypes.data)
    return out


def cos_draws(g, count, seed):
    """`count` draws of the next direction's cos_t from the oracle's generator started at `seed`: (count,) float32."""
    out = np.empty(count, np.float32)
    lib().medium_cos_draws(count, g, seed, out.ctypes.data)
    return out


def intervals(medium, o, d, t_end):
    """The region's interval on rays (o, d) (m, 3) over [0, t_end] (m,): (hit (m,) int32, t0, t1 (m,) float32)."""
    m = medium_struct(medium)
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    t_end = np.ascontiguousarray(np.broadcast_to(np.asarray(t_end, dtype=np.float32), (o.shape[0],)))
    hit, t0, t1 = np.empty(o.shape[0], np.int32), np.empty(o.shape[0], np.float32), np.empty(o.shape[0], np.float32)
    lib().medium_intervals(C.byref(m), o.shape[0], o.ctypes.data, d.ctypes.data, t_end.ctypes.data, hit.ctypes.data, t0.ctypes.data, t1.ctypes.data)
    return hit, t0, t1


def vertices(host, cam, routine, x, nv, s, seed, ab, select=0, nee_mis=1, planes=0, rgb=None, env_params=None, tallies=True):
    """medium_vertices: routine 0, 1 or 5 of rt_debug_light_vertices under Pb kind 2 — ph about ud = nv with g = s, no hemisphere — on the
    CPU → (m, 16) uint32 and gloss_reference.TALLIES' bits of each vertex (ok, no entry, fallback taken; zeros with tallies=False)."""
    c, keep = glr._cfg(0, 0, select, None, None, True, nee_mis, planes, rgb, env_params)
    x, nv, _, s, seed, ab = glr.vertex_arrays(x, nv, nv, s, seed, ab)
    m = len(x)
    out, flags = np.zeros((m, 16), np.uint32), np.zeros(m, np.uint32)
    lib().medium_vertices(C.byref(host.desc), C.byref(cam), C.byref(c), routine, m, x.ctypes.data, nv.ctypes.data, s.ctypes.data, seed.ctypes.data,
                          ab.ctypes.data, out.ctypes.data, flags.ctypes.data if tallies else None)
    return out, flags


def _cfg(medium, glossy, glossy_env, select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params):
    base, keep = glr._cfg(glossy, glossy_env, select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    c = MediumCfg()
    c.base = base
    c.medium = medium_struct(medium)
    return c, keep


def trace(host, cam, ijs, medium=None, glossy=0, glossy_env=0, select=0, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=0, rgb=None,
          env_params=None, linear=True, stats=False):
    """gloss_reference.trace under the medium → (radiance (m, 3), rays, medium events, ends (END_*), seeds (m, 4) uint32: path, nee, env,
    med); stats=True adds a dict of the tallies in STATS, summed over the samples."""
    c, keep = _cfg(medium, glossy, glossy_env, select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad = np.empty((m, 3), np.float32)
    rays, events, ends = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.int32)
    seeds = np.empty((m, 4), np.uint32)
    if stats:
        st = np.zeros(len(STATS), np.int64)
        lib().medium_trace_stats(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, events.ctypes.data,
                                 ends.ctypes.data, seeds.ctypes.data, 1 if linear else 0, st.ctypes.data)
        return rad, rays, events, ends, seeds, {k: int(x) for k, x in zip(STATS, st)}
    lib().medium_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, events.ctypes.data,
                       ends.ctypes.data, seeds.ctypes.data, 1 if linear else 0)
    return rad, rays, events, ends, seeds


def frame(host, cam, medium=None, glossy=0, glossy_env=0, select=0, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=0, rgb=None,
          env_params=None, shard=None, sample_first=0, threads=16, moments=False):
    """gloss_reference.frame under the medium."""
    c, keep = _cfg(medium, glossy, glossy_env, select, cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().medium_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                       mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
