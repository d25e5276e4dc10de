"""CPU reference of rt_render_nee / rt_nee_light_table / rt_trace_samples_nee (TEST INFRASTRUCTURE): tests/cpu_native/nee_ref.c, which
includes oracle/rt_oracle.c (its ray_color and hit_bvh are static), built into a shared library (gcc -ffp-contract=off, like the oracle)
the first time it is needed, in a temporary directory.  Threads split the rows; every pixel is still summed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import rtp_bindings as rb

PLAIN = -1          # mode of nee_frame: the oracle's ray_color (rt_render)


def lib():
    l = cpu_ref.build("nee_ref.c")
    desc, cam = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData)
    l.nee_table.restype = C.c_int32
    l.nee_table.argtypes = [desc, C.c_void_p, C.c_void_p, C.c_void_p]
    l.nee_trace.restype = None
    l.nee_trace.argtypes = [desc, cam, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.nee_frame.restype = None
    l.nee_frame.argtypes = [desc, cam, C.c_int32, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def image_rows(cam, shard=None):
    """The image rows rt_render writes for `shard` (rb.Shard or None), in the order it writes them."""
    if shard is None or shard.num_parts <= 1 or shard.band_rows <= 0:
        return list(range(cam.image_height))
    return [j for j in range(cam.image_height) if (j // shard.band_rows) % shard.num_parts == shard.part]


def table(host):
    """The emitter table: (sphere indices int32, cdf float32, pmf float32)."""
    n = max(host.desc.num_spheres, 1)
    idx, cdf, pmf = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    k = lib().nee_table(C.byref(host.desc), idx.ctypes.data, cdf.ctypes.data, pmf.ctypes.data)
    return idx[:k], cdf[:k], pmf[:k]


def trace(host, cam, ijs, mis=1):
    """ijs (n, 3) → (radiance (n, 3), rays (n,), final seeds (n,), final light-sample seeds (n,))."""
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    n = ijs.shape[0]
    rad, rays = np.empty((n, 3), np.float32), np.empty(n, np.int32)
    seeds, nee = np.empty(n, np.uint32), np.empty(n, np.uint32)
    lib().nee_trace(C.byref(host.desc), C.byref(cam), mis, n, ijs.ctypes.data, rad.ctypes.data, rays.ctypes.data, seeds.ctypes.data,
                    nee.ctypes.data)
    return rad, rays, seeds, nee


def frame(host, cam, mis=1, shard=None, sample_first=0, threads=16, moments=False):
    """The sums render_nee_to_host returns: (rows, W, 3) float32 (mis = PLAIN: rt_render's).  moments=True also returns the per-pixel
    double sums and sums of squares of each channel, (rows, W, 6)."""
    rows = np.asarray(image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().nee_frame(C.byref(host.desc), C.byref(cam), mis, rows.ctypes.data, len(rows), sample_first, threads, fb.ctypes.data,
                    mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb
