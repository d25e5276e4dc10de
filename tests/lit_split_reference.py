"""CPU reference of rt_render_lit_split / rt_trace_samples_lit_split (TEST INFRASTRUCTURE): tests/cpu_native/lit_split_ref.c, which
includes lit_ref.c for everything but the path loop, built into a shared library the first time it is needed.  The interfaces are
lit_reference's trace and frame with two radiance outputs."""
import ctypes as C

import numpy as np

import cpu_ref
import lit_reference as lr
import rtp_bindings as rb


def lib():
    l = cpu_ref.build("lit_split_ref.c")
    desc, cam, cfg = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(lr.LitCfg)
    l.lit_split_trace.restype = None
    l.lit_split_trace.argtypes = [desc, cam, cfg, C.c_int64] + [C.c_void_p] * 7 + [C.c_int32]
    l.lit_split_frame.restype = None
    l.lit_split_frame.argtypes = [desc, cam, cfg, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def trace(host, cam, ijs, cam_close=None, lens=None, emitters=True, nee_mis=1, rgb=None, env_params=None, linear=True):
    """ijs (m, 3) → (direct (m, 3), indirect (m, 3), rays (m,), final seeds (m,), final emitter-stream seeds (m,), final
    environment-stream seeds (m,))."""
    c, keep = lr._cfg(cam_close, lens, emitters, nee_mis, rgb, env_params)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    direct, indirect, rays = np.empty((m, 3), np.float32), np.empty((m, 3), np.float32), np.empty(m, np.int32)
    seeds, nee, env = np.empty(m, np.uint32), np.empty(m, np.uint32), np.empty(m, np.uint32)
    lib().lit_split_trace(C.byref(host.desc), C.byref(cam), C.byref(c), m, ijs.ctypes.data, direct.ctypes.data, indirect.ctypes.data, rays.ctypes.data,
                          seeds.ctypes.data, nee.ctypes.data, env.ctypes.data, 1 if linear else 0)
    return direct, indirect, rays, seeds, nee, env


def frame(host, cam, cam_close=None, lens=None, emitters=True, nee_mis=1, rgb=None, env_params=None, shard=None, sample_first=0, threads=16):
    """The sums render_lit_split_to_host returns: (direct, indirect), (rows, W, 3) float32 each."""
    c, keep = lr._cfg(cam_close, lens, emitters, nee_mis, rgb, env_params)
    rows = np.asarray(lr.image_rows(cam, shard), dtype=np.int32)
    direct = np.zeros((len(rows), cam.image_width, 3), np.float32)
    indirect = np.zeros((len(rows), cam.image_width, 3), np.float32)
    lib().lit_split_frame(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads, direct.ctypes.data,
                          indirect.ctypes.data)
    return direct, indirect
