"""CPU reference of rt_render_lit / rt_trace_samples_lit with rt_nee_params.sample_planes — and so of rt_render_nee, its pinhole case
without an environment — (TEST INFRASTRUCTURE): tests/cpu_native/emit_ref.c, which includes
oracle/rt_oracle.c (its ray_color and hit_bvh are static), built into a shared library (gcc -ffp-contract=off, like the oracle) the
first time it is needed, in a temporary directory.  Threads split the rows; every pixel is still summed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import env_reference as er
import rtp_bindings as rb


class EmitCfg(C.Structure):
    """emit_ref.c's lit_cfg."""
    _fields_ = [("cam_close", C.POINTER(rb.CameraData)), ("lens_radius", C.c_float), ("focus_distance", C.c_float),
                ("sample_emitters", C.c_int32), ("nee_mis", C.c_int32), ("sample_planes", C.c_int32), ("rgb", C.c_void_p), ("n", C.c_int32),
                ("ep", C.POINTER(rb.EnvParams))]


def lib():
    l = cpu_ref.build("emit_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(EmitCfg)
    l.emit_trace.restype = None
    l.emit_trace.argtypes = [desc, cam, cfg, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    l.emit_frame.restype = None
    l.emit_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    l.emit_table.restype = C.c_int32
    l.emit_table.argtypes = [desc, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.emit_vertex_picks.restype = None
    l.emit_vertex_picks.argtypes = [desc, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.emit_first_hit.restype = None
    l.emit_first_hit.argtypes = [desc, cam, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return l


image_rows = er.image_rows


def table(host, planes=1):
    """The emitter table of sample_planes = planes: (kind int32, index int32, cdf, pmf, area float32)."""
    n = host.desc.num_spheres + host.desc.num_planes + 1
    kind, idx = np.zeros(n, np.int32), np.zeros(n, np.int32)
    cdf, pmf, area = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    k = lib().emit_table(C.byref(host.desc), planes, kind.ctypes.data, idx.ctypes.data, cdf.ctypes.data, pmf.ctypes.data, area.ctypes.data)
    return kind[:k], idx[:k], cdf[:k], pmf[:k], area[:k]


def first_hit(host, cam, ijs):
    """Where the pinhole camera ray of ijs (m, 3) first lands: (kind (m,) — 0 sphere, 1 plane, -1 nothing —, index (m,), point (m, 3))."""
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    kind, idx, pt = np.empty(m, np.int32), np.empty(m, np.int32), np.zeros((m, 3), np.float32)
    lib().emit_first_hit(C.byref(host.desc), C.byref(cam), m, ijs.ctypes.data, kind.ctypes.data, idx.ctypes.data, pt.ctypes.data)
    return kind, idx, pt


def vertex_picks(host, u, code, planes=1):
    """Per vertex: the table's pick at u (the table's length: none) and the entry of primitive `code`, -1 when the table does not hold it.
    On the two-kind table (sample_planes = 1 and a plane in it) code is 2 * index + kind, else a sphere's index → (entry, found)."""
    u, code = np.ascontiguousarray(u, dtype=np.float32).ravel(), np.ascontiguousarray(code, dtype=np.int32).ravel()
    assert len(u) == len(code)
    two_kind = 1 if planes and (table(host, planes)[0] == 1).any() else 0
    entry, found = np.zeros(len(u), np.int32), np.zeros(len(u), np.int32)
    lib().emit_vertex_picks(C.byref(host.desc), planes, two_kind, len(u), u.ctypes.data, code.ctypes.data, entry.ctypes.data, found.ctypes.data)
    return entry, found


def _cfg(cam_close, lens, emitters, nee_mis, planes, rgb, env_params):
    """→ (EmitCfg, the objects it points into).  lens: None or (radius, focus); rgb: None or an (n, n, 3) map."""
    keep = []
    c = EmitCfg()
    if cam_close is not None:
        c.cam_close = C.pointer(cam_close)
    c.lens_radius, c.focus_distance = (0.0, 10.0) if lens is None else lens
    c.sample_emitters, c.nee_mis, c.sample_planes = (1 if emitters else 0), nee_mis, planes
    if rgb is not None:
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        assert rgb.ndim == 3 and rgb.shape[0] == rgb.shape[1] and rgb.shape[2] == 3, rgb.shape
        ep = er.params(env_params)
        keep += [rgb, ep]
        c.rgb, c.n, c.ep = rgb.ctypes.data, rgb.shape[0], C.pointer(ep)
    return c, keep


def trace(host, cam, ijs, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=1, rgb=None, env_params=None, linear=True):
    """ijs (m, 3) → (radiance (m, 3), rays (m,), final seeds (m,), final emitter-stream seeds (m,), final environment-stream seeds
    (m,)).  linear: the environment's cdf picks by linear scan (the header's words) instead of bisection."""
    c, keep = _cfg(cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad, rays = np.empty((m, 3), np.float32), np.empty(m, np.int32)
    seeds, nee, env = np.empty(m, np.uint32), np.empty(m, np.uint32), np.empty(m, np.uint32)
    lib().emit_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, seeds.ctypes.data,
                    nee.ctypes.data, env.ctypes.data, 1 if linear else 0)
    return rad, rays, seeds, nee, env


def frame(host, cam, cam_close=None, lens=None, emitters=True, nee_mis=1, planes=1, rgb=None, env_params=None, shard=None, sample_first=0, threads=16,
          moments=False):
    """The sums render_lit_to_host returns: (rows, W, 3) float32.  moments=True also returns the per-pixel double sums and sums of
    squares of each channel, (rows, W, 6)."""
    c, keep = _cfg(cam_close, lens, emitters, nee_mis, planes, rgb, env_params)
    rows = np.asarray(image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().emit_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                    mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
