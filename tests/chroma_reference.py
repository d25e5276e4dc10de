"""CPU reference of rt_render_chroma / rt_trace_samples_chroma (TEST INFRASTRUCTURE): tests/cpu_native/chroma_ref.c, which includes
volume_ref.c (and through it everything volume_reference.py's library holds), built into a shared library (gcc -ffp-contract=off, like the
oracle) the first time it is needed, in a temporary directory.  The library performs the handover itself: equal tints (and no medium) are
volume_ref.c's own path at sigma_t * e.  tint: None (grey), one number or three."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import rtp_bindings as rb
import volume_reference as vr


class ChromaCfg(C.Structure):
    """chroma_ref.c's chroma_cfg."""
    _fields_ = [("base", vr.VolumeCfg), ("tint", C.c_float * 3)]


def lib():
    l = cpu_ref.build("chroma_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(ChromaCfg)
    l.chroma_weights.restype = None
    l.chroma_weights.argtypes = [C.c_int64] + [C.c_void_p] * 8
    l.chroma_flights.restype = None
    l.chroma_flights.argtypes = [C.POINTER(rb.MediumParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 10
    l.chroma_trace.restype = None
    l.chroma_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 7 + [C.c_int32]
    l.chroma_frame.restype = None
    l.chroma_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def tint_of(tint):
    """None → (1, 1, 1); one number or three → three float32."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(1.0 if tint is None else tint, dtype=np.float32), (3,)))


def weights(u, uc, A, sigma):
    """The header's weights on m draws over a homogeneous interval of density length A: u, uc, A (m,), sigma (m, 3) → dict: event (m,),
    w (m, 3) float32 (the factors on beta), den (m,), trj (m,): Tr of the sampled channel."""
    u, uc, A = (np.ascontiguousarray(x, dtype=np.float32) for x in (u, uc, A))
    sigma = np.ascontiguousarray(sigma, dtype=np.float32).reshape(-1, 3)
    m = u.shape[0]
    event, w, den, trj = np.empty(m, np.int32), np.empty((m, 3), np.float32), np.empty(m, np.float32), np.empty(m, np.float32)
    lib().chroma_weights(m, u.ctypes.data, uc.ctypes.data, A.ctypes.data, sigma.ctypes.data, event.ctypes.data, w.ctypes.data, den.ctypes.data, trj.ctypes.data)
    return dict(event=event, w=w, den=den, trj=trj)


def flights(medium, density, tint, o, d, t_end, R):
    """chr_flight and chr_tr alone, as the vertex loop uses them, on rays (o, d) (m, 3) over [0, t_end] to the targets R (m,): the base
    (density None: the homogeneous one) at sigma_t = 1, the channels' extinctions the float32 products sigma_t * tint[k] → dict: hit, event,
    t (0 without an event), A (R at an event, else the interval's density length), cells, tr (m, 3)."""
    import medium_reference as mr
    m = mr.medium_struct(medium)
    sigma = (np.float32(m.sigma_t) * tint_of(tint)).astype(np.float32)
    g, n = vr.grid_of(density) if density is not None else (None, None)
    o, d, t_end = vr._rays(o, d, t_end)
    k = o.shape[0]
    R = np.ascontiguousarray(np.broadcast_to(np.asarray(R, dtype=np.float32), (k,)))
    hit, event, cells = (np.empty(k, np.int32) for _ in range(3))
    t, A, tr = np.empty(k, np.float32), np.empty(k, np.float32), np.empty((k, 3), np.float32)
    lib().chroma_flights(C.byref(m), g.ctypes.data if g is not None else None, n.ctypes.data if g is not None else None, sigma.ctypes.data, k, o.ctypes.data,
                         d.ctypes.data, t_end.ctypes.data, R.ctypes.data, hit.ctypes.data, event.ctypes.data, t.ctypes.data, A.ctypes.data, cells.ctypes.data,
                         tr.ctypes.data)
    return dict(hit=hit, event=event, t=t, A=A, cells=cells, tr=tr)


def _cfg(medium, density, tint, kw):
    base, keep = vr._cfg(medium, density, kw)
    c = ChromaCfg()
    c.base = base
    t = tint_of(tint)
    for k in range(3):
        c.tint[k] = float(t[k])
    return c, keep


def trace(host, cam, ijs, medium=None, density=None, tint=None, linear=True, **kw):
    """volume_reference.trace under the tint → its columns: (radiance (m, 3), rays, medium events, ends, seeds (m, 4) uint32: path, nee, env,
    med, cells (m,))."""
    c, keep = _cfg(medium, density, tint, kw)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad = np.empty((m, 3), np.float32)
    rays, events, ends, cells = (np.empty(m, np.int32) for _ in range(4))
    seeds = np.empty((m, 4), np.uint32)
    lib().chroma_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, events.ctypes.data,
                       ends.ctypes.data, seeds.ctypes.data, cells.ctypes.data, 1 if linear else 0)
    return rad, rays, events, ends, seeds, cells


def frame(host, cam, medium=None, density=None, tint=None, shard=None, sample_first=0, threads=16, moments=False, **kw):
    """volume_reference.frame under the tint."""
    c, keep = _cfg(medium, density, tint, kw)
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().chroma_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                       mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
