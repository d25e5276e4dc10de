"""CPU reference of rt_denoise_temporal_spp (TEST INFRASTRUCTURE): tests/cpu_native/denoise_temporal_spp_ref.c, the header's
arithmetic restated with libm's expf on top of denoise_ref.c's and denoise_spp_ref.c's passes, built into a shared library (gcc
-ffp-contract=off -fno-fast-math, like denoise_spp_reference.py) the first time it is needed, in a temporary directory."""
import ctypes as C

import numpy as np

import cpu_ref
from denoise_reference import DEFAULTS
from denoise_temporal_reference import HEADER_BYTES, history_bytes, planes  # noqa: F401  (same size and planes)

MAGIC = 0x32485452              # rt_denoise_temporal's is 0x31485452
MODE_SPATIAL, MODE_MOMENTS = 1, 2


def lib():
    l = cpu_ref.build("denoise_temporal_spp_ref.c")
    l.denoise_temporal_spp_reference.restype = C.c_int
    l.denoise_temporal_spp_reference.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 11 + [C.c_int]
    return l


def header(history):
    """(magic, width, height, fourth word) of a history buffer (uint8 array)."""
    return tuple(int(v) for v in np.frombuffer(bytes(history[:16]), np.uint32))


def reference(fb_sum, spp, moments, aov, aov_spp, cam, history_prev=None, threads=16, **params):
    """What rt_denoise_temporal_spp computes for fb_sum (H, W, 3) float32, spp (H, W) int32, moments (H, W, 2) float32 or None (as
    render_adaptive_to_host returns them), aov {"albedo", "normal", "depth", "hits", "prim"} at aov_spp samples per pixel, cam
    (rb.CameraData) and history_prev (a uint8 array of the header's layout, or None): ((H, W, 3) float32 output, the next history as
    a uint8 array)."""
    p = {**DEFAULTS, **params}
    fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
    h, w = fb.shape[:2]
    assert (cam.image_width, cam.image_height) == (w, h)
    n = np.ascontiguousarray(spp, dtype=np.int32)
    mom = None if moments is None else np.ascontiguousarray(moments, dtype=np.float32)
    arrays = [np.ascontiguousarray(aov[k], dtype=t) for k, t in (("albedo", np.float32), ("normal", np.float32), ("depth", np.float32),
                                                                  ("hits", np.uint32), ("prim", np.int32))]
    assert arrays[0].shape == arrays[1].shape == (h, w, 3) and arrays[2].shape == arrays[3].shape == arrays[4].shape == n.shape == (h, w)
    assert mom is None or mom.shape == (h, w, 2)
    prev = None if history_prev is None else np.ascontiguousarray(history_prev, dtype=np.uint8)
    assert prev is None or prev.nbytes >= history_bytes(w, h)
    nxt = np.zeros(history_bytes(w, h), np.uint8)
    out = np.empty_like(fb)
    cam_bytes = C.create_string_buffer(bytes(cam), C.sizeof(cam))
    rc = lib().denoise_temporal_spp_reference(cam_bytes, aov_spp, p["iterations"], p["sigma_depth"], p["sigma_luminance"], p["normal_squarings"],
                                              fb.ctypes.data, n.ctypes.data, None if mom is None else mom.ctypes.data,
                                              *[a.ctypes.data for a in arrays], None if prev is None else prev.ctypes.data,
                                              nxt.ctypes.data, out.ctypes.data, threads)
    assert rc == 0
    return out, nxt
