"""CPU reference of rt_render_glow / rt_trace_samples_glow (TEST INFRASTRUCTURE): tests/cpu_native/glow_ref.c, which includes volume_ref.c
(and through it everything volume_reference.py's library holds), built into a shared library (gcc -ffp-contract=off, like the oracle) the
first time it is needed, in a temporary directory.  The library performs the handover itself: radiance 0, 0, 0 is volume_ref.c's own path.
radiance: None (no glow), one number or three; source 0, 1 or 2; heat: an (nz, ny, nx) grid like the density (source 2)."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import rtp_bindings as rb
import volume_reference as vr


class GlowCfg(C.Structure):
    """glow_ref.c's glow_cfg."""
    _fields_ = [("base", vr.VolumeCfg), ("source", C.c_int32), ("radiance", C.c_float * 3), ("heat", C.c_void_p)]


def lib():
    l = cpu_ref.build("glow_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(GlowCfg)
    l.glow_flights.restype = None
    l.glow_flights.argtypes = [C.POINTER(rb.MediumParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 9
    l.glow_trace.restype = None
    l.glow_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 8 + [C.c_int32]
    l.glow_frame.restype = None
    l.glow_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def radiance_of(radiance):
    """None → (0, 0, 0); one number or three → three float32."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(0.0 if radiance is None else radiance, dtype=np.float32), (3,)))


def flights(medium, density, o, d, t_end, u, source=0, heat=None):
    """glow_flight alone on rays (o, d) (m, 3) over [0, t_end] with the draws u (m,): the base is the homogeneous one (density None) or the
    grid, the cells' h by the source → dict: hit, event, t (0 without an event), E, cells."""
    import medium_reference as mr
    m = mr.medium_struct(medium)
    g, n = vr.grid_of(density) if density is not None else (None, None)
    h = None if source == 0 else vr.grid_of(density if source == 1 else heat)[0]
    o, d, t_end = vr._rays(o, d, t_end)
    k = o.shape[0]
    u = np.ascontiguousarray(np.broadcast_to(np.asarray(u, dtype=np.float32), (k,)))
    hit, event, cells = (np.empty(k, np.int32) for _ in range(3))
    t, E = np.empty(k, np.float32), np.empty(k, np.float32)
    lib().glow_flights(C.byref(m), g.ctypes.data if g is not None else None, h.ctypes.data if h is not None else None, n.ctypes.data if g is not None else None,
                       k, o.ctypes.data, d.ctypes.data, t_end.ctypes.data, u.ctypes.data, hit.ctypes.data, event.ctypes.data, t.ctypes.data, E.ctypes.data,
                       cells.ctypes.data)
    return dict(hit=hit, event=event, t=t, E=E, cells=cells)


def _cfg(medium, density, radiance, source, heat, kw):
    base, keep = vr._cfg(medium, density, kw)
    c = GlowCfg()
    c.base = base
    c.source = int(source)
    r = radiance_of(radiance)
    for k in range(3):
        c.radiance[k] = float(r[k])
    if source != 0:
        assert density is not None, "source 1 and 2 follow a grid"
    if source == 2:
        h, n = vr.grid_of(heat)
        assert (int(n[0]), int(n[1]), int(n[2])) == (c.base.nx, c.base.ny, c.base.nz), "the heat grid has the volume's dimensions"
        c.heat = h.ctypes.data
        keep = (keep, h)
    else:
        assert heat is None, "a heat grid is for source 2 only"
    return c, keep


def trace(host, cam, ijs, medium=None, density=None, radiance=None, source=0, heat=None, linear=True, **kw):
    """volume_reference.trace under the glow → its columns and glow_length: (radiance (m, 3), rays, medium events, ends, seeds (m, 4)
    uint32: path, nee, env, med, cells (m,), glow_length (m,) float32)."""
    c, keep = _cfg(medium, density, radiance, source, heat, kw)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad = np.empty((m, 3), np.float32)
    rays, events, ends, cells = (np.empty(m, np.int32) for _ in range(4))
    seeds = np.empty((m, 4), np.uint32)
    length = np.empty(m, np.float32)
    lib().glow_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, events.ctypes.data,
                     ends.ctypes.data, seeds.ctypes.data, cells.ctypes.data, length.ctypes.data, 1 if linear else 0)
    return rad, rays, events, ends, seeds, cells, length


def frame(host, cam, medium=None, density=None, radiance=None, source=0, heat=None, shard=None, sample_first=0, threads=16, moments=False, **kw):
    """volume_reference.frame under the glow."""
    c, keep = _cfg(medium, density, radiance, source, heat, kw)
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().glow_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                     mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
