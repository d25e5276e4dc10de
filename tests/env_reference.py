"""CPU reference of rt_env / rt_render_env / rt_env_table / rt_env_lookup / rt_trace_samples_env (TEST INFRASTRUCTURE):
tests/cpu_native/env_ref.c, which includes oracle/rt_oracle.c (its ray_color and hit_bvh are static), built into a shared library
(gcc -ffp-contract=off, like the oracle) the first time it is needed, in a temporary directory.  Threads split the rows; every pixel is
still summed in sample order.  Also the synthetic maps the tests and tools/env_time.py share."""
import ctypes as C

import numpy as np

import cpu_ref
import rtp_bindings as rb


def lib():
    l = cpu_ref.build("env_ref.c")
    desc, cam, par = C.POINTER(rb.SceneDesc), C.POINTER(rb.CameraData), C.POINTER(rb.EnvParams)
    l.env_texel_weight.restype = C.c_double
    l.env_texel_weight.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    l.env_table.restype = C.c_int32
    l.env_table.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.env_lookup.restype = None
    l.env_lookup.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.env_decode.restype = None
    l.env_decode.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    l.env_trace.restype = None
    l.env_trace.argtypes = [desc, cam, C.c_void_p, C.c_int32, par, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_int32]
    l.env_frame.restype = None
    l.env_frame.argtypes = [desc, cam, C.c_void_p, C.c_int32, par, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def _map(rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    assert rgb.ndim == 3 and rgb.shape[0] == rgb.shape[1] and rgb.shape[2] == 3, rgb.shape
    return rgb, rgb.shape[0]


def params(p=None):
    """None / dict / rb.EnvParams → rb.EnvParams with the header's defaults filled in (without the library: the CPU tests' copy)."""
    if isinstance(p, rb.EnvParams):
        return p
    q = rb.EnvParams()
    q.mode, q.scale, q.camera_visible = 1, 1.0, 1
    q.rot[0] = q.rot[4] = q.rot[8] = 1.0
    for k, v in (p or {}).items():
        if k == "rot":
            for i, x in enumerate(np.asarray(v, dtype=np.float32).ravel()):
                q.rot[i] = x
        else:
            setattr(q, k, v)
    return q


def image_rows(cam, shard=None):
    """The image rows rt_render writes for `shard` (rb.Shard or None), in the order it writes them."""
    if shard is None or shard.num_parts <= 1 or shard.band_rows <= 0:
        return list(range(cam.image_height))
    return [j for j in range(cam.image_height) if (j // shard.band_rows) % shard.num_parts == shard.part]


def texel_weights(rgb):
    """(n, n) float64: radiance sum x solid angle of every texel, [iy, ix]."""
    rgb, n = _map(rgb)
    l = lib()
    return np.array([[l.env_texel_weight(rgb.ctypes.data, n, ix, iy) for ix in range(n)] for iy in range(n)], dtype=np.float64)


def table(rgb):
    """(count, row cdf (n,), row pmf (n,), conditional cdfs (n, n), conditional pmfs (n, n)); count = n, or 0: an empty table."""
    rgb, n = _map(rgb)
    rc, rp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    cc, cp = np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
    count = lib().env_table(rgb.ctypes.data, n, rc.ctypes.data, rp.ctypes.data, cc.ctypes.data, cp.ctypes.data)
    return count, rc, rp, cc, cp


def lookup(rgb, dirs):
    """dirs (m, 3) → (texel = iy * n + ix (m,), radiance (m, 3), pl (m,))."""
    rgb, n = _map(rgb)
    dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    m = dirs.shape[0]
    tex, rad, pl = np.empty(m, np.int32), np.empty((m, 3), np.float32), np.empty(m, np.float32)
    lib().env_lookup(rgb.ctypes.data, n, m, dirs.ctypes.data, tex.ctypes.data, rad.ctypes.data, pl.ctypes.data)
    return tex, rad, pl


def decode(uv):
    """uv (m, 2) in [-1, 1]^2 → unit directions (m, 3) by the header's float decode."""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    out = np.empty((uv.shape[0], 3), np.float32)
    lib().env_decode(uv.shape[0], uv.ctypes.data, out.ctypes.data)
    return out


def trace(host, cam, rgb, ijs, p=None, linear=True):
    """ijs (m, 3) → (radiance (m, 3), rays (m,), final seeds (m,), final light-sample seeds (m,)).  linear: the cdf picks by linear scan
    (the header's words) instead of bisection."""
    rgb, n = _map(rgb)
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    m = ijs.shape[0]
    rad, rays = np.empty((m, 3), np.float32), np.empty(m, np.int32)
    seeds, env = np.empty(m, np.uint32), np.empty(m, np.uint32)
    lib().env_trace(C.byref(host.desc), C.byref(cam), rgb.ctypes.data, n, C.byref(params(p)), m, ijs.ctypes.data, rad.ctypes.data,
                    rays.ctypes.data, seeds.ctypes.data, env.ctypes.data, 1 if linear else 0)
    return rad, rays, seeds, env


def frame(host, cam, rgb, p=None, shard=None, sample_first=0, threads=16, moments=False):
    """The sums render_env_to_host returns: (rows, W, 3) float32 (rgb None: rt_render's, the oracle's ray_color).  moments=True also
    returns the per-pixel double sums and sums of squares of each channel, (rows, W, 6)."""
    n = 0
    if rgb is not None:
        rgb, n = _map(rgb)
    rows = np.asarray(image_rows(cam, shard), dtype=np.int32)
    fb = np.zeros((len(rows), cam.image_width, 3), np.float32)
    mom = np.zeros((len(rows), cam.image_width, 6), np.float64) if moments else None
    lib().env_frame(C.byref(host.desc), C.byref(cam), rgb.ctypes.data if rgb is not None else None, n, C.byref(params(p)), rows.ctypes.data,
                    len(rows), sample_first, threads, fb.ctypes.data, mom.ctypes.data if moments else None)
    return (fb, mom) if moments else fb


# ---- the synthetic maps (fixed by formula: the restatement, the GPU tests and tools/env_time.py build the same arrays) ------------

def texel_directions(n):
    """(n, n, 3) float64 unit directions of the texel centres, [iy, ix]."""
    c = -1.0 + (2.0 * np.arange(n) + 1.0) / n
    u, v = np.meshgrid(c, c, indexing="xy")
    y = 1.0 - np.abs(u) - np.abs(v)
    sgn = lambda x: np.where(x >= 0, 1.0, -1.0)
    x = np.where(y >= 0, u, (1.0 - np.abs(v)) * sgn(u))
    z = np.where(y >= 0, v, (1.0 - np.abs(u)) * sgn(v))
    p = np.stack([x, y, z], -1)
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


def texel_solid_angles(n):
    """(n, n) float64: (2 / n)^2 / |p_c|^3."""
    c = -1.0 + (2.0 * np.arange(n) + 1.0) / n
    u, v = np.meshgrid(c, c, indexing="xy")
    y = 1.0 - np.abs(u) - np.abs(v)
    x = np.where(y >= 0, u, 1.0 - np.abs(v))
    z = np.where(y >= 0, v, 1.0 - np.abs(u))
    return (2.0 / n) ** 2 / (x * x + y * y + z * z) ** 1.5


SUN_ELEVATION_DEG, SUN_RADIUS, SUN_SHARE = 40.0, 0.02, 0.9


def sun_and_sky(n=256):
    """(n, n, 3) float32: a smooth gradient sky of order 1 — (0.5, 0.7, 1.0) * (0.25 + 0.75 * max(y, 0)) + (0.1, 0.09, 0.08) below the
    horizon's share — plus a disc of angular radius SUN_RADIUS around a direction SUN_ELEVATION_DEG above the horizon (azimuth: +x
    turned 30 degrees towards +z), whose texels carry SUN_SHARE of the map's total power (radiance x solid angle, summed over r, g, b)."""
    d = texel_directions(n)
    y = d[..., 1]
    sky = np.array([0.5, 0.7, 1.0])[None, None, :] * (0.25 + 0.75 * np.maximum(y, 0.0))[..., None]
    sky = sky + np.array([0.1, 0.09, 0.08])[None, None, :] * np.maximum(-y, 0.0)[..., None]
    el, az = np.radians(SUN_ELEVATION_DEG), np.radians(30.0)
    sun_dir = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    disc = (d @ sun_dir) >= np.cos(SUN_RADIUS)
    assert disc.sum() >= 1, "the sun's disc covers no texel centre at this n"
    omega = texel_solid_angles(n)
    sky_power = (sky.sum(-1) * omega).sum()
    sun_colour = np.array([1.0, 0.9, 0.7])
    # sun radiance L * colour over the disc's texels: L * sum(colour) * omega_disc = share / (1 - share) * sky power
    level = SUN_SHARE / (1.0 - SUN_SHARE) * sky_power / (sun_colour.sum() * omega[disc].sum())
    out = sky.copy()
    out[disc] += level * sun_colour
    return out.astype(np.float32)


def constant_map(n, c=(1.0, 1.0, 1.0)):
    return np.broadcast_to(np.asarray(c, np.float32), (n, n, 3)).copy()


Z_UP = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0)      # rows of the world → environment rotation of a z-up scene: env y = world z
