"""CPU reference of rt_render_glow_sampled / rt_trace_samples_glow_sampled and of rt_glow_sampler's table (TEST INFRASTRUCTURE):
tests/cpu_native/glow_sample_ref.c, which includes glow_ref.c (and through it everything glow_reference.py's library holds), built into a
shared library (gcc -ffp-contract=off, like the oracle) the first time it is needed, in a temporary directory.  The library builds the table
itself and performs the handover itself: sample 0, an empty table or no glow is glow_ref.c's own path.
sample: None (off), "mis" or "light"; the other arguments are glow_reference's."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import glow_reference as gr
import medium_reference as mr
import rtp_bindings as rb
import volume_reference as vr


class GlowSampleCfg(C.Structure):
    """glow_sample_ref.c's glow_sample_cfg."""
    _fields_ = [("base", gr.GlowCfg), ("sample", C.c_int32), ("mis", C.c_int32)]


def lib():
    l = cpu_ref.build("glow_sample_ref.c")
    desc, cam, cfg, med = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(GlowSampleCfg), C.POINTER(rb.MediumParams)
    l.glow_sample_table.restype = C.c_int32
    l.glow_sample_table.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 4
    l.glow_sample_pl.restype = None
    l.glow_sample_pl.argtypes = [med, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
    l.glow_sample_line.restype = None
    l.glow_sample_line.argtypes = [med, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    l.glow_sample_draws.restype = None
    l.glow_sample_draws.argtypes = [med, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64] + [C.c_void_p] * 4
    l.glow_sample_trace.restype = None
    l.glow_sample_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 9 + [C.c_int32]
    l.glow_sample_frame.restype = None
    l.glow_sample_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def h_of(density, source=0, heat=None):
    """The cells' h of a call: None (1 everywhere, source 0), the density (1) or the heat (2), as the contiguous float32 grid."""
    return None if source == 0 else vr.grid_of(density if source == 1 else heat)[0]


def table(density, source=0, heat=None):
    """The contract's table of a grid → dict: empty, slab_cdf (nz,), row_cdf (nz, ny), cell_cdf and pc (nz, ny, nx)."""
    nz, ny, nx = np.asarray(density).shape
    h = h_of(density, source, heat)
    slab, row, cell, pc = np.zeros(nz, np.float32), np.zeros((nz, ny), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32)
    empty = lib().glow_sample_table(h.ctypes.data if h is not None else None, nx, ny, nz, slab.ctypes.data, row.ctypes.data, cell.ctypes.data, pc.ctypes.data)
    return dict(empty=bool(empty), slab_cdf=slab, row_cdf=row, cell_cdf=cell, pc=pc)


def _grid_args(medium, density, source, heat):
    m = mr.medium_struct(medium)
    g, n = vr.grid_of(density)
    h = h_of(density, source, heat)
    return m, g, h, n


def pl(medium, density, o, d, source=0, heat=None):
    """glow_pl of rays (o, d) (m, 3) → (float32 (m,), the float64 sum over the same cells (m,))."""
    m, g, h, n = _grid_args(medium, density, source, heat)
    o, d, _ = vr._rays(o, d, 0.0)
    k = o.shape[0]
    out, out_d = np.empty(k, np.float32), np.empty(k, np.float64)
    lib().glow_sample_pl(C.byref(m), g.ctypes.data, h.ctypes.data if h is not None else None, n.ctypes.data, k, o.ctypes.data, d.ctypes.data, out.ctypes.data,
                         out_d.ctypes.data)
    return out, out_d


def line(medium, density, o, d, t_end, source=0, heat=None):
    """glow_line of rays (o, d) (m, 3) up to t_end → (float32 (m,), float64 over the same cells (m,), the number of the walks' cells whose
    x = sigma_c * seg took the series (x < 0.0625) and the number that took the closed form)."""
    m, g, h, n = _grid_args(medium, density, source, heat)
    o, d, t_end = vr._rays(o, d, t_end)
    k = o.shape[0]
    out, out_d, branches = np.empty(k, np.float32), np.empty(k, np.float64), np.zeros(2, np.int32)
    lib().glow_sample_line(C.byref(m), g.ctypes.data, h.ctypes.data if h is not None else None, n.ctypes.data, k, o.ctypes.data, d.ctypes.data,
                           t_end.ctypes.data, out.ctypes.data, out_d.ctypes.data, branches.ctypes.data)
    return out, out_d, int(branches[0]), int(branches[1])


def draws(medium, density, x, seed, count, source=0, heat=None):
    """`count` light samples of a vertex at x with no hemisphere and a constant pb, from the oracle's generator started at `seed` →
    (cell (count, 3) int32: x, y, z — -1 where the pick found nothing; taken (count,) bool; dir (count, 3); pl (count,))."""
    m, g, h, n = _grid_args(medium, density, source, heat)
    x = np.ascontiguousarray(x, dtype=np.float32)
    cell, taken, dirs, pls = np.empty((count, 3), np.int32), np.empty(count, np.int32), np.empty((count, 3), np.float32), np.empty(count, np.float32)
    lib().glow_sample_draws(C.byref(m), g.ctypes.data, h.ctypes.data if h is not None else None, n.ctypes.data, x.ctypes.data, seed, count, cell.ctypes.data,
                            taken.ctypes.data, dirs.ctypes.data, pls.ctypes.data)
    return cell, taken != 0, dirs, pls


def _cfg(medium, density, radiance, source, heat, sample, kw):
    base, keep = gr._cfg(medium, density, radiance, source, heat, kw)
    c = GlowSampleCfg()
    c.base = base
    c.sample = 0 if sample is None else 1
    c.mis = 0 if sample == "light" else 1
    assert sample in (None, "mis", "light"), sample
    return c, keep


def trace(host, cam, ijs, medium=None, density=None, radiance=None, source=0, heat=None, sample=None, linear=True, **kw):
    """glow_reference.trace with the light samples → its columns and glow_samples: (radiance (m, 3), rays, medium events, ends, seeds (m, 4)
    uint32: path, nee, env, med, cells (m,), glow_length (m,) float32, glow_samples (m,))."""
    c, keep = _cfg(medium, density, radiance, source, heat, sample, kw)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad = np.empty((m, 3), np.float32)
    rays, events, ends, cells, shots = (np.empty(m, np.int32) for _ in range(5))
    seeds = np.empty((m, 4), np.uint32)
    length = np.empty(m, np.float32)
    lib().glow_sample_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, events.ctypes.data,
                            ends.ctypes.data, seeds.ctypes.data, cells.ctypes.data, length.ctypes.data, shots.ctypes.data, 1 if linear else 0)
    return rad, rays, events, ends, seeds, cells, length, shots


def frame(host, cam, medium=None, density=None, radiance=None, source=0, heat=None, sample=None, shard=None, sample_first=0, threads=16, moments=False, **kw):
    """glow_reference.frame with the light samples."""
    c, keep = _cfg(medium, density, radiance, source, heat, sample, kw)
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().glow_sample_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                            mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
