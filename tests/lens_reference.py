"""CPU reference of rt_render_lens / rt_render_aov_lens / rt_lens_camera_rays (TEST INFRASTRUCTURE): tests/cpu_native/lens_ref.c,
which includes oracle/rt_oracle.c (its ray_color is static), built into a shared library (gcc -ffp-contract=off, like the oracle) the
first time it is needed, in a temporary directory.  Threads split the rows; every pixel is still summed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import rtp_bindings as rb


def lib():
    l = cpu_ref.build("lens_ref.c")
    cam = C.POINTER(rb.CameraData)
    l.lens_rays.restype = None
    l.lens_rays.argtypes = [cam, cam, C.c_float, C.c_float, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p]
    l.lens_frame.restype = None
    l.lens_frame.argtypes = [C.POINTER(rb.SceneDesc), cam, cam, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    l.lens_aov.restype = None
    l.lens_aov.argtypes = [C.POINTER(rb.SceneDesc), cam, cam, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return l


def image_rows(cam, shard=None):
    """The image rows rt_render writes for `shard` (rb.Shard or None), in the order it writes them."""
    if shard is None or shard.num_parts <= 1 or shard.band_rows <= 0:
        return list(range(cam.image_height))
    return [j for j in range(cam.image_height) if (j // shard.band_rows) % shard.num_parts == shard.part]


def _close(cam_close):
    return C.byref(cam_close) if cam_close is not None else None


def rays(cam_open, cam_close, radius, focus, ijs):
    """Camera rays of ijs (n, 3) → (origins (n, 3), directions (n, 3), final seeds (n,) uint32, tau (n,), lens sample (n, 2))."""
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    n = ijs.shape[0]
    org, dirs = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    seeds, taus, lxy = np.empty(n, np.uint32), np.empty(n, np.float32), np.empty((n, 2), np.float32)
    lib().lens_rays(C.byref(cam_open), _close(cam_close), radius, focus, n, ijs.ctypes.data, org.ctypes.data, dirs.ctypes.data,
                    seeds.ctypes.data, taus.ctypes.data, lxy.ctypes.data)
    return org, dirs, seeds, taus, lxy


def frame(host, cam_open, cam_close=None, radius=0.0, focus=10.0, shard=None, sample_first=0, threads=16):
    """The sums render_lens_to_host returns: (rows, W, 3) float32."""
    rows = np.asarray(image_rows(cam_open, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam_open.image_width, 3), np.float32)
    lib().lens_frame(C.byref(host.desc), C.byref(cam_open), _close(cam_close), radius, focus, rows.ctypes.data, len(rows), sample_first,
                     threads, fb.ctypes.data)
    return fb


def aov(host, cam_open, cam_close=None, radius=0.0, focus=10.0, shard=None, sample_first=0, threads=16):
    """The AOV sums render_aov_lens_to_host returns: {"albedo", "normal", "depth", "hits", "prim"}."""
    rows = np.asarray(image_rows(cam_open, shard), dtype=np.int32)
    shape = (len(rows), cam_open.image_width)
    out = {"albedo": np.zeros(shape + (3,), np.float32), "normal": np.zeros(shape + (3,), np.float32), "depth": np.zeros(shape, np.float32),
           "hits": np.zeros(shape, np.uint32), "prim": np.zeros(shape, np.int32)}
    lib().lens_aov(C.byref(host.desc), C.byref(cam_open), _close(cam_close), radius, focus, rows.ctypes.data, len(rows), sample_first,
                   threads, out["albedo"].ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["hits"].ctypes.data,
                   out["prim"].ctypes.data)
    return out
