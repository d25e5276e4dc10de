"""CPU reference of rt_render_aov_volume (TEST INFRASTRUCTURE): tests/cpu_native/aov_volume_ref.c, which includes volume_ref.c (and through
it everything volume_reference.py's library holds), built into a shared library (gcc -ffp-contract=off, like the oracle) the first time it
is needed, in a temporary directory.  Threads split the rows; every pixel is still summed in sample order."""
import ctypes as C

import numpy as np

import cpu_ref
import emit_reference as emr
import rtp_bindings as rb
import volume_reference as vr


def lib():
    l = cpu_ref.build("aov_volume_ref.c")
    l.aov_volume.restype = None
    l.aov_volume.argtypes = [C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(vr.VolumeCfg), C.c_void_p, C.c_int, C.c_int, C.c_int] + \
        [C.c_void_p] * 6
    return l


KEYS = ("albedo", "normal", "depth", "hits", "prim", "transmittance")


def aov(host, cam, medium=None, density=None, cam_close=None, lens=None, shard=None, sample_first=0, threads=16):
    """The sums render_aov_volume_to_host returns: {"albedo", "normal", "depth", "hits", "prim", "transmittance"}.  medium: None, a dict
    (medium_reference.medium_struct's) or an rb.MediumParams; density: None or an (nz, ny, nx) grid."""
    c, keep = vr._cfg(medium, density, dict(cam_close=cam_close, lens=lens))
    rows = np.asarray(emr.image_rows(cam, shard), dtype=np.int32)
    shape = (len(rows), cam.image_width)
    out = {"albedo": np.zeros(shape + (3,), np.float32), "normal": np.zeros(shape + (3,), np.float32), "depth": np.zeros(shape, np.float32),
           "hits": np.zeros(shape, np.uint32), "prim": np.zeros(shape, np.int32), "transmittance": np.zeros(shape, np.float32)}
    lib().aov_volume(C.byref(host.desc), C.byref(cam), C.byref(c), rows.ctypes.data, len(rows), sample_first, threads,
                     *(out[k].ctypes.data for k in KEYS))
    return out
