"""CPU reference of rt_denoise_temporal (TEST INFRASTRUCTURE): tests/cpu_native/denoise_temporal_ref.c, the header's arithmetic
restated with libm's expf on top of denoise_ref.c's spatial passes, built into a shared library (gcc -ffp-contract=off
-fno-fast-math, like denoise_reference.py) the first time it is needed, in a temporary directory."""
import ctypes as C

import numpy as np

import cpu_ref
from denoise_reference import DEFAULTS

HEADER_BYTES = 256


def lib():
    l = cpu_ref.build("denoise_temporal_ref.c")
    l.denoise_temporal_reference.restype = C.c_int
    l.denoise_temporal_reference.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 9 + [C.c_int]
    return l


def history_bytes(width, height):
    return HEADER_BYTES + 64 * width * height


def planes(history, width, height):
    """The four per-pixel planes of a history buffer (uint8 array): colour, moments, position, normal, each (H, W, 4) float32."""
    body = np.frombuffer(bytes(history[HEADER_BYTES:history_bytes(width, height)]), np.float32).reshape(4, height, width, 4)
    return {name: body[k] for k, name in enumerate(("colour", "moments", "position", "normal"))}


def reference(fb_sum, aov, cam, history_prev=None, threads=16, **params):
    """What rt_denoise_temporal computes for fb_sum (H, W, 3) float32, aov {"albedo", "normal", "depth", "hits", "prim"} (as
    render_to_host and render_aov_to_host return them), cam (rb.CameraData) and history_prev (a uint8 array of the header's layout,
    or None): ((H, W, 3) float32 output, the next history as a uint8 array)."""
    p = {**DEFAULTS, **params}
    fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
    h, w = fb.shape[:2]
    assert (cam.image_width, cam.image_height) == (w, h)
    arrays = [np.ascontiguousarray(aov[k], dtype=t) for k, t in (("albedo", np.float32), ("normal", np.float32), ("depth", np.float32),
                                                                  ("hits", np.uint32), ("prim", np.int32))]
    assert arrays[0].shape == arrays[1].shape == (h, w, 3) and arrays[2].shape == arrays[3].shape == arrays[4].shape == (h, w)
    prev = None if history_prev is None else np.ascontiguousarray(history_prev, dtype=np.uint8)
    nxt = np.zeros(history_bytes(w, h), np.uint8)
    out = np.empty_like(fb)
    cam_bytes = C.create_string_buffer(bytes(cam), C.sizeof(cam))
    rc = lib().denoise_temporal_reference(cam_bytes, p["iterations"], p["sigma_depth"], p["sigma_luminance"], p["normal_squarings"],
                                          fb.ctypes.data, *[a.ctypes.data for a in arrays], None if prev is None else prev.ctypes.data,
                                          nxt.ctypes.data, out.ctypes.data, threads)
    assert rc == 0
    return out, nxt
