"""CPU reference of rt_denoise (TEST INFRASTRUCTURE): tests/cpu_native/denoise_ref.c, the header's arithmetic restated with libm's
expf, built into a shared library (gcc -ffp-contract=off -fno-fast-math, like aov_reference.py builds aov_ref.c) the first time it
is needed, in a temporary directory.  Threads split the rows of each pass."""
import ctypes as C

import numpy as np

import cpu_ref

DEFAULTS = {"iterations": 5, "sigma_depth": 1.0, "sigma_luminance": 4.0, "normal_squarings": 7}


def lib():
    l = cpu_ref.build("denoise_ref.c")
    l.denoise_reference.restype = C.c_int
    l.denoise_reference.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 6 + [C.c_int]
    return l


def reference(fb_sum, aov, spp, threads=16, **params):
    """What rt_denoise computes for fb_sum (H, W, 3) float32 and aov {"albedo", "normal", "depth", "hits"} (as render_to_host and
    render_aov_to_host return them): (H, W, 3) float32."""
    p = {**DEFAULTS, **params}
    fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
    h, w = fb.shape[:2]
    albedo = np.ascontiguousarray(aov["albedo"], dtype=np.float32)
    normal = np.ascontiguousarray(aov["normal"], dtype=np.float32)
    depth = np.ascontiguousarray(aov["depth"], dtype=np.float32)
    hits = np.ascontiguousarray(aov["hits"], dtype=np.uint32)
    assert albedo.shape == normal.shape == (h, w, 3) and depth.shape == hits.shape == (h, w)
    out = np.empty_like(fb)
    rc = lib().denoise_reference(w, h, spp, p["iterations"], p["sigma_depth"], p["sigma_luminance"], p["normal_squarings"], fb.ctypes.data,
                                 albedo.ctypes.data, normal.ctypes.data, depth.ctypes.data, hits.ctypes.data, out.ctypes.data, threads)
    assert rc == 0
    return out
