"""CPU reference of rt_denoise_spp (TEST INFRASTRUCTURE): tests/cpu_native/denoise_spp_ref.c, the header's arithmetic restated with
libm's expf on top of denoise_ref.c's passes, built into a shared library (gcc -ffp-contract=off -fno-fast-math, like
denoise_reference.py) the first time it is needed, in a temporary directory."""
import ctypes as C

import numpy as np

import cpu_ref
from denoise_reference import DEFAULTS


def lib():
    l = cpu_ref.build("denoise_spp_ref.c")
    l.denoise_spp_reference.restype = C.c_int
    l.denoise_spp_reference.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 9 + [C.c_int]
    return l


def reference(fb_sum, spp, moments, aov, aov_spp, threads=16, want_var=False, **params):
    """What rt_denoise_spp computes for fb_sum (H, W, 3) float32, spp (H, W) int32, moments (H, W, 2) float32 or None (as
    render_adaptive_to_host returns them) and aov {"albedo", "normal", "depth", "hits"} at aov_spp samples per pixel: (H, W, 3)
    float32.  want_var: (that, the second prepass's var (H, W) float32 — what steers the first iteration; 0 where no hit pixel)."""
    p = {**DEFAULTS, **params}
    fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
    h, w = fb.shape[:2]
    n = np.ascontiguousarray(spp, dtype=np.int32)
    mom = None if moments is None else np.ascontiguousarray(moments, dtype=np.float32)
    albedo = np.ascontiguousarray(aov["albedo"], dtype=np.float32)
    normal = np.ascontiguousarray(aov["normal"], dtype=np.float32)
    depth = np.ascontiguousarray(aov["depth"], dtype=np.float32)
    hits = np.ascontiguousarray(aov["hits"], dtype=np.uint32)
    assert albedo.shape == normal.shape == (h, w, 3) and depth.shape == hits.shape == n.shape == (h, w)
    assert mom is None or mom.shape == (h, w, 2)
    out = np.empty_like(fb)
    var = np.zeros((h, w), np.float32) if want_var else None
    rc = lib().denoise_spp_reference(w, h, aov_spp, p["iterations"], p["sigma_depth"], p["sigma_luminance"], p["normal_squarings"],
                                     fb.ctypes.data, n.ctypes.data, None if mom is None else mom.ctypes.data, albedo.ctypes.data,
                                     normal.ctypes.data, depth.ctypes.data, hits.ctypes.data, out.ctypes.data, None if var is None else var.ctypes.data, threads)
    assert rc == 0
    return (out, var) if want_var else out
