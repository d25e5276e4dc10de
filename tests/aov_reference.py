"""CPU reference of rt_render_aov (TEST INFRASTRUCTURE): tests/cpu_native/aov_ref.c on the oracle's exported functions —
orc_get_ray, orc_geom_hit_bvh (rec9 = t, point, normal, u, v) and orc_tex2d — built with oracle/rt_oracle.c into a shared library
(gcc -ffp-contract=off, like the oracle) the first time it is needed, in a temporary directory.  Threads split the pixels;
every pixel is still computed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import rtp_bindings as rb


def lib():
    l = cpu_ref.build("aov_ref.c", "oracle/rt_oracle.c")
    l.aov_reference.restype = C.c_int64
    l.aov_reference.argtypes = [C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.c_int64, C.c_void_p, C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return l


def image_rows(cam, shard=None):
    """The image rows rt_render writes for `shard` (rb.Shard or None), in the order it writes them."""
    if shard is None or shard.num_parts <= 1 or shard.band_rows <= 0:
        return list(range(cam.image_height))
    return [j for j in range(cam.image_height) if (j // shard.band_rows) % shard.num_parts == shard.part]


def reference(host, cam, rows=None, cols=None, threads=16):
    """AOVs of the pixels rows x cols (image coordinates; default: the whole image) as render_aov_to_host returns them:
    {"albedo": (R, W, 3), "normal": (R, W, 3), "depth": (R, W), "hits": (R, W) uint32, "prim": (R, W) int32}.  Asserts the
    self-check (orc_geom_hit_bvh and orc_closest_hit agree on every ray)."""
    rows = list(range(cam.image_height)) if rows is None else list(rows)
    cols = list(range(cam.image_width)) if cols is None else list(cols)
    jj, ii = np.meshgrid(np.asarray(rows, dtype=np.int32), np.asarray(cols, dtype=np.int32), indexing="ij")
    ij = np.ascontiguousarray(np.stack([ii.ravel(), jj.ravel()], axis=1), dtype=np.int32)
    n = ij.shape[0]
    out = {"albedo": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32), "depth": np.zeros(n, np.float32),
           "hits": np.zeros(n, np.uint32), "prim": np.zeros(n, np.int32)}
    bad = lib().aov_reference(C.byref(host.desc), C.byref(cam), n, ij.ctypes.data, threads, out["albedo"].ctypes.data,
                              out["normal"].ctypes.data, out["depth"].ctypes.data, out["hits"].ctypes.data, out["prim"].ctypes.data)
    assert bad == 0, f"orc_geom_hit_bvh and orc_closest_hit disagree on {bad} rays"
    shape = (len(rows), len(cols))
    return {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}
