"""CPU reference of rt_render_volume / rt_trace_samples_volume (TEST INFRASTRUCTURE): tests/cpu_native/volume_ref.c, which includes
medium_ref.c (and through it everything medium_reference.py's library holds), built into a shared library (gcc -ffp-contract=off, like the
oracle) the first time it is needed, in a temporary directory.  A grid is an (nz, ny, nx) float32 array, as rb.Volume takes it."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import medium_reference as mr
import rtp_bindings as rb


class VolumeCfg(C.Structure):
    """volume_ref.c's volume_cfg."""
    _fields_ = [("base", mr.MediumCfg), ("rho", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32)]


def lib():
    l = cpu_ref.build("volume_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(VolumeCfg)
    l.volume_walks.restype = None
    l.volume_walks.argtypes = [C.POINTER(rb.MediumParams), C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 14
    l.volume_walks_f64.restype = None
    l.volume_walks_f64.argtypes = [C.POINTER(rb.MediumParams), C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    l.volume_trace.restype = None
    l.volume_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 7 + [C.c_int32]
    l.volume_frame.restype = None
    l.volume_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def grid_of(density):
    """(nz, ny, nx) → the contiguous float32 array and (nx, ny, nz) as int32."""
    g = np.ascontiguousarray(density, dtype=np.float32)
    assert g.ndim == 3, g.shape
    return g, np.array([g.shape[2], g.shape[1], g.shape[0]], np.int32)


def _rays(o, d, t_end):
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    t_end = np.ascontiguousarray(np.broadcast_to(np.asarray(t_end, dtype=np.float32), (o.shape[0],)))
    return o, d, t_end


# volume_ref.c's VT_* tallies, in its order: the bit k of walks()' `flags` is TALLIES[k].  The first seven are the walk's (either walk of the
# ray sets them), the last four the free flight's
TALLIES = ("two axes tie", "three axes tie", "clamp tb < ta", "entry cell clamped", "left by tb >= t1", "left by the index", "an axis with d_k == 0",
           "flight: empty cell crossed", "flight: event in the first cell", "flight: event after an empty cell", "flight: no event")


def walks(medium, density, o, d, t_end, rem=None, tallies=True):
    """The header's walk on rays (o, d) (m, 3) over [0, t_end] → dict: hit (the interval), acc (float32 optical depth), cells, seg_sum and
    seg_min (float64, of the float32 segments), length ((t1 - t0) * len in float32), tr (expf(-acc); 0 where the interval is empty), flags
    (the tallies of the ray's walks, TALLIES' bits); with rem (m,): event, t_event and rem_left (the rem a flight without an event ended
    with) and flight_cells of a free flight.  tallies=False: the library counts nothing (flags stays 0) — every other column is the same."""
    m = mr.medium_struct(medium)
    g, n = grid_of(density)
    o, d, t_end = _rays(o, d, t_end)
    k = o.shape[0]
    hit, acc, cells, segs = np.empty(k, np.int32), np.empty(k, np.float32), np.empty(k, np.int32), np.empty((k, 3), np.float64)
    event, t_event, rem_left = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k, np.float32)
    tr, flight_cells, flags = np.empty(k, np.float32), np.zeros(k, np.int32), np.zeros(k, np.int32)
    if rem is not None:
        rem = np.ascontiguousarray(np.broadcast_to(np.asarray(rem, dtype=np.float32), (k,)))
    lib().volume_walks(C.byref(m), g.ctypes.data, n.ctypes.data, k, o.ctypes.data, d.ctypes.data, t_end.ctypes.data, hit.ctypes.data, acc.ctypes.data,
                       cells.ctypes.data, segs.ctypes.data, rem.ctypes.data if rem is not None else None, event.ctypes.data, t_event.ctypes.data,
                       tr.ctypes.data, rem_left.ctypes.data, flight_cells.ctypes.data, flags.ctypes.data if tallies else None)
    return dict(hit=hit, acc=acc, cells=cells, seg_sum=segs[:, 0], seg_min=segs[:, 1], length=segs[:, 2], event=event, t_event=t_event, tr=tr,
                rem_left=rem_left, flight_cells=flight_cells, flags=flags)


def walks_f64(medium, density, o, d, t_end):
    """The same walk stated in float64 from the same float32 inputs → (hit, acc, (t1 - t0) * len), float64."""
    m = mr.medium_struct(medium)
    g, n = grid_of(density)
    o, d, t_end = _rays(o, d, t_end)
    k = o.shape[0]
    hit, acc, length = np.empty(k, np.int32), np.empty(k, np.float64), np.empty(k, np.float64)
    lib().volume_walks_f64(C.byref(m), g.ctypes.data, n.ctypes.data, k, o.ctypes.data, d.ctypes.data, t_end.ctypes.data, hit.ctypes.data,
                           acc.ctypes.data, length.ctypes.data)
    return hit, acc, length


def _cfg(medium, density, kw):
    base, keep = mr._cfg(medium, kw.pop("glossy", 0), kw.pop("glossy_env", 0), kw.pop("select", 0), kw.pop("cam_close", None), kw.pop("lens", None),
                         kw.pop("emitters", True), kw.pop("nee_mis", 1), kw.pop("planes", 0), kw.pop("rgb", None), kw.pop("env_params", None))
    assert not kw, kw
    c = VolumeCfg()
    c.base = base
    if density is not None:
        g, n = grid_of(density)
        c.rho = g.ctypes.data
        c.nx, c.ny, c.nz = (int(x) for x in n)
        keep = (keep, g)
    return c, keep


def trace(host, cam, ijs, medium=None, density=None, linear=True, **kw):
    """medium_reference.trace with the grid `density` (None: medium_reference's own path) → (radiance (m, 3), rays, medium events, ends,
    seeds (m, 4) uint32: path, nee, env, med, cells (m,))."""
    c, keep = _cfg(medium, density, kw)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad = np.empty((m, 3), np.float32)
    rays, events, ends, cells = (np.empty(m, np.int32) for _ in range(4))
    seeds = np.empty((m, 4), np.uint32)
    lib().volume_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, events.ctypes.data,
                       ends.ctypes.data, seeds.ctypes.data, cells.ctypes.data, 1 if linear else 0)
    return rad, rays, events, ends, seeds, cells


def frame(host, cam, medium=None, density=None, shard=None, sample_first=0, threads=16, moments=False, **kw):
    """medium_reference.frame with the grid."""
    c, keep = _cfg(medium, density, kw)
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().volume_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                       mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
