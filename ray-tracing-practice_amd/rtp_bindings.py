"""ctypes bindings of the product libraries (no oracle in here).

librtp_host.so  — pure host code: config parser, scene/BVH builders, camera, saver arithmetic
                  (ray-tracing-practice_amd/host/rtp_host.h).  Loads without a GPU.
librtp_amd.so   — the MI355X render library behind the C ABI of include/rtp_amd.h.  Loading it
                  needs the HIP runtime; every compute call needs a GPU and fails loudly without
                  one (there is no CPU fallback in the product).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class Vec3(C.Structure):
    _fields_ = [("e", C.c_float * 3)]


class Sphere(C.Structure):
    _fields_ = [("center", Vec3), ("radius", C.c_float), ("material_idx", C.c_int32), ("_pad", C.c_int32 * 3)]


class Plane(C.Structure):
    _fields_ = [("type", C.c_int32), ("D", C.c_float), ("material_idx", C.c_int32), ("w", Vec3), ("u", Vec3),
                ("v", Vec3), ("base", Vec3), ("normal", Vec3), ("_pad", C.c_int32 * 2)]


class Material(C.Structure):
    _fields_ = [("type", C.c_int32), ("fuzz", C.c_float), ("ir", C.c_float), ("absorption", Vec3), ("albedo", Vec3),
                ("emit", Vec3), ("texture_id", C.c_uint64), ("reserved", C.c_uint64)]


class BvhNode(C.Structure):
    _fields_ = [("box", C.c_float * 6), ("left", C.c_int32), ("right", C.c_int32), ("type", C.c_int32)]


class CameraData(C.Structure):
    _fields_ = [("origin", Vec3), ("pixel00_loc", Vec3), ("pixel_delta_u", Vec3), ("pixel_delta_v", Vec3),
                ("background", Vec3), ("image_width", C.c_int32), ("image_height", C.c_int32),
                ("samples_per_pixel", C.c_int32), ("max_depth", C.c_int32)]


class Texture(C.Structure):
    _fields_ = [("rgba", C.POINTER(C.c_float)), ("width", C.c_int32), ("height", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("spheres", C.POINTER(Sphere)), ("num_spheres", C.c_int32),
                ("planes", C.POINTER(Plane)), ("num_planes", C.c_int32),
                ("materials", C.POINTER(Material)), ("num_materials", C.c_int32),
                ("nodes", C.POINTER(BvhNode)), ("num_nodes", C.c_int32),
                ("textures", C.POINTER(Texture)), ("num_textures", C.c_int32)]


class Shard(C.Structure):
    _fields_ = [("band_rows", C.c_int32), ("num_parts", C.c_int32), ("part", C.c_int32)]


class _Sized(C.Structure):
    """A structure of the caller's size: struct_bytes is set on construction, to the size of the object's own type (a subclass that
    appends fields says its own)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_bytes = C.sizeof(type(self))


class Timing(_Sized):
    """rt_timing (include/rtp_amd.h): an out-structure of the caller's size — struct_bytes is set on construction."""
    _fields_ = [("struct_bytes", C.c_uint32), ("kernel_ms", C.c_float), ("num_workgroups", C.c_uint32), ("workgroup_size", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("scene_in_lds", C.c_uint32), ("trace_launches", C.c_uint32),
                ("trace_ms", C.c_float), ("guarded", C.c_uint32), ("flagged_samples", C.c_uint64), ("rework_ms", C.c_float),
                ("guard_unproven", C.c_uint32), ("kernel", C.c_uint32), ("guard_dynamic", C.c_uint32), ("wide_nodes", C.c_uint32),
                ("sphere_only", C.c_uint32), ("primary_visibility", C.c_uint32), ("primary_ms", C.c_float),
                ("trace_vgprs", C.c_uint32), ("trace_scratch_bytes", C.c_uint32), ("abandoned_passes", C.c_uint32),
                ("traced_samples", C.c_uint64), ("guard_paused", C.c_uint32), ("front_primitives", C.c_uint32),
                ("dark_kernel", C.c_uint32)]


class AovBuffers(_Sized):
    """rt_aov_buffers (include/rtp_amd.h): DEVICE addresses of the first-hit AOV sums, each may be NULL."""
    _fields_ = [("struct_bytes", C.c_uint32), ("reserved", C.c_uint32), ("albedo_sum", C.c_void_p), ("normal_sum", C.c_void_p),
                ("depth_sum", C.c_void_p), ("hit_count", C.c_void_p), ("first_prim", C.c_void_p)]


# rt_aov_buffers field of each AOV, its numpy type and its values per pixel (render_aov_to_host)
AOV_CHANNELS = (("albedo", "albedo_sum", np.float32, 3), ("normal", "normal_sum", np.float32, 3), ("depth", "depth_sum", np.float32, 1),
                ("hits", "hit_count", np.uint32, 1), ("prim", "first_prim", np.int32, 1))


def _fill(p, name, fields, given, unknown=None, setters={}):
    """Sets the `given` fields of p, the mirror of the C struct `name`: one outside `fields` raises unknown(field) (default: an RtError
    that names the struct); setters[field](p, value) stands in for plain assignment."""
    for k, v in given.items():
        if k not in fields:
            raise unknown(k) if unknown else RtError(f"{name} has no field {k}")
        if k in setters:
            setters[k](p, v)
        else:
            setattr(p, k, v)
    return p


def _params(kind, name, fields, given, **how):
    """kind() with the library's defaults (the call <name>_init), then the `given` fields as _fill sets them."""
    p = kind()
    getattr(amd_lib(), name + "_init")(C.byref(p))
    return _fill(p, name, fields, given, **how)


def _struct(value, kind, make):
    """An optional params argument of a call: None → NULL (the call's defaults); a `kind` as it is; a dict → make(**dict)."""
    return None if value is None else C.byref(value if isinstance(value, kind) else make(**value))


def _ref(struct):
    """An optional structure argument of a call (shard, cam_close): None → NULL."""
    return C.byref(struct) if struct else None


def _stream_sync(stream, sync):
    """The (hip_stream, sync) arguments of a render call: stream None = the default stream."""
    return C.c_void_p(stream or 0), 1 if sync else 0


def _probe(ijs, *columns):
    """The preamble of a probe call: ijs as contiguous (n, 3) int32, n, and one empty output array per column (dtype, trailing shape)."""
    ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
    n = ijs.shape[0]
    return ijs, n, tuple(np.empty((n, *shape), dtype=dtype) for dtype, shape in columns)


_RGB, _COUNT, _SEED = (np.float32, (3,)), (np.int32, ()), (np.uint32, ())          # the columns probes return


class DenoiseParams(_Sized):
    """rt_denoise_params (include/rtp_amd.h): an IN structure of the caller's size — struct_bytes is set on construction; the
    other fields are 0 until rt_denoise_params_init (denoise_params()) fills the defaults."""
    _fields_ = [("struct_bytes", C.c_uint32), ("iterations", C.c_int32), ("sigma_depth", C.c_float), ("sigma_luminance", C.c_float),
                ("normal_squarings", C.c_int32)]


class AdaptiveParams(_Sized):
    """rt_adaptive_params (include/rtp_amd.h): an IN structure of the caller's size — struct_bytes is set on construction; the other
    fields are 0 until rt_adaptive_params_init (adaptive_params()) fills the defaults."""
    _fields_ = [("struct_bytes", C.c_uint32), ("min_spp", C.c_int32), ("batch_spp", C.c_int32), ("max_spp", C.c_int32), ("threshold", C.c_float)]


def adaptive_params(**params):
    """rt_adaptive_params with the library's defaults, then the given fields (min_spp, batch_spp, max_spp, threshold)."""
    return _params(AdaptiveParams, "rt_adaptive_params", dict(AdaptiveParams._fields_), params)


class StopParams(_Sized):
    """rt_stop_params (include/rtp_amd.h): an IN structure of the caller's size — struct_bytes is set on construction."""
    _fields_ = [("struct_bytes", C.c_uint32), ("rule", C.c_int32), ("reserved", C.c_int32 * 2)]


def stop_params(**params):
    """rt_stop_params with the library's defaults, then the given fields (rule)."""
    return _params(StopParams, "rt_stop_params", ("rule",), params)


class LensParams(_Sized):
    """rt_lens_params (include/rtp_amd.h): an IN structure of the caller's size — struct_bytes is set on construction; the other
    fields are 0 until rt_lens_params_init (lens_params()) fills the defaults."""
    _fields_ = [("struct_bytes", C.c_uint32), ("lens_radius", C.c_float), ("focus_distance", C.c_float)]


def lens_params(**params):
    """rt_lens_params with the library's defaults, then the given fields (lens_radius, focus_distance)."""
    return _params(LensParams, "rt_lens_params", dict(LensParams._fields_), params)


def _lens_struct(lens):
    return _struct(lens, LensParams, lens_params)


def lens_camera_rays(cam_open, cam_close, lens, ijs):
    """rt_lens_camera_rays: ijs (n, 3) int32 (i, j, s) → (origins (n, 3) float32, directions (n, 3) float32, final seeds (n,) uint32)."""
    ijs, n, out = _probe(ijs, _RGB, _RGB, _SEED)
    _check(amd_lib().rt_lens_camera_rays(C.byref(cam_open), _ref(cam_close), _lens_struct(lens), n, ijs.ctypes.data,
                                         *(a.ctypes.data for a in out)), "rt_lens_camera_rays")
    return out


class NeeParams(_Sized):
    """rt_nee_params (include/rtp_amd.h): an IN structure of the caller's size — struct_bytes is set on construction; the other
    fields are 0 until rt_nee_params_init (nee_params()) fills the defaults."""
    class _Tail(C.Union):
        """The struct's last 8 bytes: sample_planes and select — and, over the same bytes, the two-word `reserved` view of the struct
        before the two were taken from it (reserved[1] is select: 0 by default)."""
        class _Words(C.Structure):
            _fields_ = [("sample_planes", C.c_int32), ("select", C.c_int32)]
        _anonymous_ = ("_words",)
        _fields_ = [("_words", _Words), ("reserved", C.c_int32 * 2)]
    _anonymous_ = ("_tail",)
    _fields_ = [("struct_bytes", C.c_uint32), ("mis", C.c_int32), ("_tail", _Tail)]
    FIELDS = ("struct_bytes", "mis", "sample_planes", "select")          # what nee_params() sets


class NeeParamsGlossy(NeeParams):
    """rt_nee_params as the library compiles it today: NeeParams — the 16-byte struct of a caller from before the glossy switch, which the
    library reads as glossy = 0 — and the trailing field `glossy` (read when struct_bytes >= 20)."""
    _fields_ = [("glossy", C.c_int32)]
    FIELDS = NeeParams.FIELDS + ("glossy",)


def nee_params(**params):
    """rt_nee_params with the library's defaults (mis = 1, sample_planes = 0, select = 0, glossy = 0), then the given fields.  Without
    `glossy` the result is the 16-byte NeeParams (an older caller's struct: glossy = 0); with it, the 20-byte NeeParamsGlossy."""
    if "glossy" in params:
        return _params(NeeParamsGlossy, "rt_nee_params", NeeParamsGlossy.FIELDS, params)
    p = NeeParams()          # (the library's init writes its own 20 bytes: the defaults come through the full struct)
    C.memmove(C.byref(p), C.byref(_params(NeeParamsGlossy, "rt_nee_params", (), {})), C.sizeof(NeeParams))
    p.struct_bytes = C.sizeof(NeeParams)
    return _fill(p, "rt_nee_params", NeeParams.FIELDS, params)


def _nee_struct(params):
    return _struct(params, NeeParams, nee_params)


class EnvParams(_Sized):
    """rt_env_params (include/rtp_amd.h): an IN structure of the caller's size — struct_bytes is set on construction; the other
    fields are 0 until rt_env_params_init (env_params()) fills the defaults."""
    class _Tail(C.Union):
        """The struct's last 12 bytes: glossy and the two words still reserved — and, over the same bytes, the three-word `reserved` view
        of the struct before the switch was taken from it (reserved[0] is glossy: 0 by default)."""
        class _Words(C.Structure):
            _fields_ = [("glossy", C.c_int32), ("reserved2", C.c_int32 * 2)]
        _anonymous_ = ("_words",)
        _fields_ = [("_words", _Words), ("reserved", C.c_int32 * 3)]
    _anonymous_ = ("_tail",)
    _fields_ = [("struct_bytes", C.c_uint32), ("mode", C.c_int32), ("scale", C.c_float), ("rot", C.c_float * 9),
                ("camera_visible", C.c_int32), ("_tail", _Tail)]
    FIELDS = ("struct_bytes", "mode", "scale", "rot", "camera_visible", "glossy")          # what env_params() sets


ENV_PATH, ENV_MIS, ENV_LIGHT = 0, 1, 2


def env_params(**params):
    """rt_env_params with the library's defaults (mode = 1, scale = 1, rot = identity, camera_visible = 1, glossy = 0), then the given fields
    (rot: nine numbers, the rows of the world → environment rotation)."""
    return _params(EnvParams, "rt_env_params", EnvParams.FIELDS, params, setters={"rot": _set_env_rot})


def _set_env_rot(p, v):
    v = np.asarray(v, dtype=np.float32).ravel()
    if v.size != 9:
        raise RtError("rt_env_params.rot takes nine numbers")
    for i in range(9):
        p.rot[i] = float(v[i])


env_params_of = env_params      # (lit_params has an argument of that name)


def _env_struct(params):
    return _struct(params, EnvParams, env_params)


class LitParams(_Sized):
    """rt_lit_params (include/rtp_amd.h): an IN structure of the caller's size — struct_bytes is set on construction; the other fields
    are 0 until rt_lit_params_init (lit_params()) fills the defaults.  The pointers are borrowed: lit_params() keeps what it points
    into alive in `_keep`."""
    _fields_ = [("struct_bytes", C.c_uint32), ("sample_emitters", C.c_int32), ("cam_close", C.POINTER(CameraData)),
                ("lens", C.POINTER(LensParams)), ("nee", C.POINTER(NeeParams)), ("env", C.c_void_p), ("env_params", C.POINTER(EnvParams))]


def lit_params(cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None):
    """rt_lit_params with the library's defaults, then: cam_close a CameraData (None: no motion); lens, nee, env_params None (the
    defaults), the params structure or a dict of its fields; emitters False: no light samples of the emitter table; env an Env."""
    p = _params(LitParams, "rt_lit_params", (), {})
    p.sample_emitters = int(emitters) if not isinstance(emitters, bool) else (1 if emitters else 0)
    keep = []
    if cam_close is not None:
        p.cam_close = C.pointer(cam_close)
    for field, value, kind, make in (("lens", lens, LensParams, lens_params), ("nee", nee, NeeParams, nee_params),
                                     ("env_params", env_params, EnvParams, env_params_of)):
        if value is not None:
            value = value if isinstance(value, kind) else make(**value)
            keep.append(value)
            setattr(p, field, C.cast(C.pointer(value), C.POINTER(kind)))          # (the field's type: value may be of a subclass)
    if env is not None:
        p.env = env._h
        keep.append(env)
    p._keep = keep
    return p


class MediumParams(_Sized):
    """rt_medium_params (include/rtp_amd.h, "participating medium"): an IN structure of the caller's size — struct_bytes is set on
    construction; the other fields are 0 until rt_medium_params_init (medium_params()) fills the defaults."""
    _fields_ = [("struct_bytes", C.c_uint32), ("region", C.c_int32), ("sigma_t", C.c_float), ("albedo", C.c_float * 3), ("g", C.c_float),
                ("a", C.c_float * 3), ("b", C.c_float * 3)]


def medium_params(sigma_t=0.0, albedo=1.0, g=0.0, ball=None, box=None):
    """rt_medium_params with the library's defaults, then: sigma_t; albedo one number or three; g; the region — ball=(cx, cy, cz, r) or
    box=(x0, y0, z0, x1, y1, z1), neither: all space.  Nothing is checked here: the library refuses what it does not take."""
    if ball is not None and box is not None:
        raise RtError("rt_medium_params takes one region: ball or box")
    p = _params(MediumParams, "rt_medium_params", (), {})
    p.sigma_t = float(sigma_t)
    alb = np.broadcast_to(np.asarray(albedo, dtype=np.float32), (3,))
    for k in range(3):
        p.albedo[k] = float(alb[k])
    p.g = float(g)
    if ball is not None:
        v = np.asarray(ball, dtype=np.float32).ravel()
        if v.size != 4:
            raise RtError("rt_medium_params: ball takes four numbers (cx, cy, cz, r)")
        p.region = 1
        for k in range(3):
            p.a[k] = float(v[k])
        p.b[0] = float(v[3])
    elif box is not None:
        v = np.asarray(box, dtype=np.float32).ravel()
        if v.size != 6:
            raise RtError("rt_medium_params: box takes six numbers (x0, y0, z0, x1, y1, z1)")
        p.region = 2
        for k in range(3):
            p.a[k] = float(v[k])
            p.b[k] = float(v[3 + k])
    return p


def _medium_struct(medium):
    return _struct(medium, MediumParams, medium_params)


class ChromaParams(_Sized):
    """rt_chroma_params (include/rtp_amd.h, "chromatic extinction"): an IN structure of the caller's size — struct_bytes is set on
    construction; tint is 0 until rt_chroma_params_init (chroma_params()) fills the defaults."""
    _fields_ = [("struct_bytes", C.c_uint32), ("tint", C.c_float * 3)]


def chroma_params(tint=1.0):
    """rt_chroma_params with the library's defaults, then tint: one number or three.  Nothing is checked here: the library refuses what it
    does not take."""
    p = _params(ChromaParams, "rt_chroma_params", (), {})
    t = np.broadcast_to(np.asarray(tint, dtype=np.float32), (3,))
    for k in range(3):
        p.tint[k] = float(t[k])
    return p


def _chroma_struct(chroma):
    """None → NULL (grey); a ChromaParams as it is; a dict → chroma_params(**dict); anything else is the tint itself."""
    if chroma is None or isinstance(chroma, (ChromaParams, dict)):
        return _struct(chroma, ChromaParams, chroma_params)
    return C.byref(chroma_params(tint=chroma))


class GlowParams(_Sized):
    """rt_glow_params (include/rtp_amd.h, "emission in the medium"): an IN structure of the caller's size — struct_bytes is set on
    construction; source and radiance are 0 until rt_glow_params_init (glow_params()) fills the defaults (which are 0 as well)."""
    _fields_ = [("struct_bytes", C.c_uint32), ("source", C.c_int32), ("radiance", C.c_float * 3)]


def glow_params(radiance=0.0, source=0):
    """rt_glow_params with the library's defaults, then radiance (one number or three) and source (0 uniform, 1 the density grid, 2 a heat
    grid).  Nothing is checked here: the library refuses what it does not take."""
    p = _params(GlowParams, "rt_glow_params", (), {})
    r = np.broadcast_to(np.asarray(radiance, dtype=np.float32), (3,))
    for k in range(3):
        p.radiance[k] = float(r[k])
    p.source = int(source)
    return p


def _glow_struct(glow):
    """None → NULL (no glow); a GlowParams as it is; a dict → glow_params(**dict); anything else is the radiance itself (source 0)."""
    if glow is None or isinstance(glow, (GlowParams, dict)):
        return _struct(glow, GlowParams, glow_params)
    return C.byref(glow_params(radiance=glow))


class GlowSampleParams(_Sized):
    """rt_glow_sample_params (include/rtp_amd.h, "light samples of the glow"): an IN structure of the caller's size — struct_bytes is set
    on construction; sample and mis are 0 until rt_glow_sample_params_init (glow_sample_params()) fills the defaults."""
    _fields_ = [("struct_bytes", C.c_uint32), ("sample", C.c_int32), ("mis", C.c_int32)]


def glow_sample_params(sample=0, mis=1):
    """rt_glow_sample_params with the library's defaults, then sample (0 off, 1 the glow is light-sampled) and mis (1 the power heuristic,
    0 light sampling alone).  Nothing is checked here: the library refuses what it does not take."""
    p = _params(GlowSampleParams, "rt_glow_sample_params", (), {})
    p.sample = int(sample)
    p.mis = int(mis)
    return p


def _glow_sample_struct(sample):
    """None → NULL (no light samples); a GlowSampleParams as it is; a dict → glow_sample_params(**dict); "mis" and "light" → sample = 1
    with mis 1 and 0."""
    if isinstance(sample, str):
        return C.byref(glow_sample_params(sample=1, mis={"mis": 1, "light": 0}[sample]))
    return _struct(sample, GlowSampleParams, glow_sample_params)


class Env:
    """rt_env: an octahedral environment map with its sampling table on the current device.  Env(rgb) takes an (n, n, 3) array;
    Env.from_equirect(image, n) resamples a lat-long image first.  A context manager; close() destroys the object."""

    def __init__(self, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[0] != rgb.shape[1] or rgb.shape[2] != 3:
            raise RtError(f"Env takes an (n, n, 3) array, not {rgb.shape}")
        self.n = int(rgb.shape[0])
        h = C.c_void_p()
        _check(amd_lib().rt_env_create(rgb.ctypes.data, self.n, C.byref(h)), "rt_env_create")
        self._h = h

    @staticmethod
    def equirect_to_octahedral(image, n=1024):
        """rt_env_from_equirect: (h, w, 3) lat-long → (n, n, 3) octahedral (host only)."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        if image.ndim != 3 or image.shape[2] != 3:
            raise RtError(f"a lat-long image is (h, w, 3), not {image.shape}")
        out = np.empty((n, n, 3), dtype=np.float32)
        _check(amd_lib().rt_env_from_equirect(image.ctypes.data, image.shape[1], image.shape[0], n, out.ctypes.data), "rt_env_from_equirect")
        return out

    @classmethod
    def from_equirect(cls, image, n=1024):
        return cls(cls.equirect_to_octahedral(image, n))

    def table(self, row=0):
        """rt_env_table: (count, row cdf, row pmf, row `row`'s conditional cdf, its pmf); count = n, or 0 for an empty table."""
        n = self.n
        out = [np.zeros(n, dtype=np.float32) for _ in range(4)]
        count = C.c_int32()
        _check(amd_lib().rt_env_table(self._h, row, *(a.ctypes.data for a in out), C.byref(count)), "rt_env_table")
        return (count.value, *out)

    def lookup(self, dirs):
        """rt_env_lookup: dirs (m, 3) → (texel = iy * n + ix (m,), radiance (m, 3), pl (m,)), computed on the device."""
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        m = dirs.shape[0]
        tex, rad, pl = np.empty(m, np.int32), np.empty((m, 3), np.float32), np.empty(m, np.float32)
        _check(amd_lib().rt_env_lookup(self._h, m, dirs.ctypes.data, tex.ctypes.data, rad.ctypes.data, pl.ctypes.data), "rt_env_lookup")
        return tex, rad, pl

    def close(self):
        if self._h is not None:
            amd_lib().rt_env_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Volume:
    """rt_volume: a density grid on the current device.  Volume(density) takes an (nz, ny, nx) float32 array — x fastest, as the library
    reads it.  A context manager; close() destroys the object."""

    def __init__(self, density):
        density = np.ascontiguousarray(density, dtype=np.float32)
        if density.ndim != 3:
            raise RtError(f"Volume takes an (nz, ny, nx) array, not {density.shape}")
        self.nz, self.ny, self.nx = (int(n) for n in density.shape)
        h = C.c_void_p()
        _check(amd_lib().rt_volume_create(density.ctypes.data, self.nx, self.ny, self.nz, C.byref(h)), "rt_volume_create")
        self._h = h

    def close(self):
        if self._h is not None:
            amd_lib().rt_volume_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GlowSampler:
    """rt_glow_sampler: the table that light samples of a glow pick their cell from, on the volume's device.  GlowSampler(volume, source,
    heat) takes the Volumes of the call it is for (heat: source 2 only) and is closed before them.  A context manager."""

    def __init__(self, volume, source=0, heat=None):
        self.nx, self.ny, self.nz = volume.nx, volume.ny, volume.nz
        h = C.c_void_p()
        _check(amd_lib().rt_glow_sampler_create(_volume_handle(volume), int(source), _volume_handle(heat), C.byref(h)), "rt_glow_sampler_create")
        self._h = h

    def table(self, z=0, y=0):
        """rt_glow_sampler_table: (count, slab cdf (nz), slab z's row cdf (ny), row (z, y)'s cell cdf and its cells' pc (nx each));
        count = nx * ny * nz, or 0 for an empty sampler."""
        out = [np.zeros(n, dtype=np.float32) for n in (self.nz, self.ny, self.nx, self.nx)]
        count = C.c_int32()
        _check(amd_lib().rt_glow_sampler_table(self._h, z, y, *(a.ctypes.data for a in out), C.byref(count)), "rt_glow_sampler_table")
        return (count.value, *out)

    def close(self):
        if self._h is not None:
            amd_lib().rt_glow_sampler_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _sampler_handle(sampler):
    """None → NULL; a GlowSampler → its handle."""
    if sampler is None:
        return None
    if not isinstance(sampler, GlowSampler) or sampler._h is None:
        raise RtError("sampler must be an open rtp_bindings.GlowSampler (or None)")
    return sampler._h


def _volume_handle(volume):
    """None → NULL (no grid: rt_render_medium itself); a Volume → its handle."""
    if volume is None:
        return None
    if not isinstance(volume, Volume) or volume._h is None:
        raise RtError("volume must be an open rtp_bindings.Volume (or None)")
    return volume._h


class FogParams(_Sized):
    """rt_fog_params (include/rtp_amd.h, "adaptive sampling on every fog rung"): what a fog call is made of, by pointers — an IN structure
    of the caller's size.  struct_bytes is set on construction; every pointer is NULL until fog_params() sets it."""
    _fields_ = [("struct_bytes", C.c_uint32), ("medium", C.POINTER(MediumParams)), ("volume", C.c_void_p), ("chroma", C.POINTER(ChromaParams)),
                ("glow", C.POINTER(GlowParams)), ("heat", C.c_void_p), ("sample", C.POINTER(GlowSampleParams)), ("sampler", C.c_void_p)]


def fog_params(medium=None, volume=None, tint=None, glow=None, heat=None, sample=None, sampler=None):
    """rt_fog_params with the library's defaults (every pointer NULL), then the given parts: medium, tint, glow and sample as
    render_medium, render_chroma, render_glow and render_glow_sampled take them; volume and heat a Volume, sampler a GlowSampler.  The
    structure keeps what it points to alive.  Nothing is checked here: the library refuses what it does not take."""
    p = _params(FogParams, "rt_fog_params", (), {})
    keep = []

    def point(field, kind, value):
        keep.append(value)
        setattr(p, field, C.cast(C.pointer(value), C.POINTER(kind)))
    if medium is not None:
        point("medium", MediumParams, medium if isinstance(medium, MediumParams) else medium_params(**medium))
    if tint is not None:
        point("chroma", ChromaParams, tint if isinstance(tint, ChromaParams) else chroma_params(**tint) if isinstance(tint, dict) else chroma_params(tint=tint))
    if glow is not None:
        point("glow", GlowParams, glow if isinstance(glow, GlowParams) else glow_params(**glow) if isinstance(glow, dict) else glow_params(radiance=glow))
    if sample is not None:
        if isinstance(sample, str):
            sample = glow_sample_params(sample=1, mis={"mis": 1, "light": 0}[sample])
        point("sample", GlowSampleParams, sample if isinstance(sample, GlowSampleParams) else glow_sample_params(**sample))
    for field, handle, value in (("volume", _volume_handle, volume), ("heat", _volume_handle, heat), ("sampler", _sampler_handle, sampler)):
        h = handle(value)
        if h is not None:
            keep.append(value)
            setattr(p, field, h if isinstance(h, int) else C.cast(h, C.c_void_p).value)
    p._keep = keep
    return p


TRAVERSAL_AUTO, TRAVERSAL_EXACT, TRAVERSAL_GUARDED = 0, 1, 2
BUILD_HOST_SAH, BUILD_DEVICE_LBVH = 0, 1
KERNEL_AUTO, KERNEL_MEGA, KERNEL_WAVEFRONT = 0, 1, 2


class Config(C.Structure):
    """rt_config (include/rtp_amd.h)."""
    _fields_ = [("struct_bytes", C.c_uint32), ("tree_build", C.c_int32), ("guard_gamma_ulps", C.c_float),
                ("guard_exact_leaf_table", C.c_int32), ("traversal", C.c_int32), ("guard_min_primitives", C.c_int32),
                ("guard_keep", C.c_int32), ("guard_repack", C.c_int32), ("kernel", C.c_int32), ("workspace_bytes", C.c_uint64),
                ("pass_spp", C.c_int32), ("stack_levels", C.c_int32), ("flag_capacity", C.c_uint32), ("scene_in_lds", C.c_int32),
                ("lds_treelet", C.c_int32), ("workgroups_per_cu", C.c_int32), ("k_inner", C.c_int32), ("k_shade", C.c_int32),
                ("reserve_chunk", C.c_int32), ("reserve_taper", C.c_int32), ("wavefront_paths", C.c_int32),
                ("wavefront_exchange", C.c_int32), ("wide_nodes", C.c_int32), ("guard_dynamic_margins", C.c_int32),
                ("sphere_only_kernel", C.c_int32), ("overlap_rework", C.c_int32), ("primary_visibility", C.c_int32),
                ("guard_bail_share", C.c_int32), ("guard_front_primitives", C.c_int32), ("reuse_view_lists", C.c_int32), ("resume_flagged", C.c_int32),
                ("dark_kernel", C.c_int32)]


def new_config():
    """rt_config with the library's defaults (what the header's rt_config_init macro does: the CALLER's struct size travels along)."""
    cfg = Config()
    lib = amd_lib()
    if hasattr(lib, "rt_config_init_sized"):
        lib.rt_config_init_sized(C.byref(cfg), C.sizeof(Config))
        assert cfg.struct_bytes == C.sizeof(Config) or os.environ.get("RTP_AMD_LIB"), (cfg.struct_bytes, C.sizeof(Config))
    else:       # an OLDER build loaded through RTP_AMD_LIB for an A/B run (developer tools): it fills the fields it has
        assert os.environ.get("RTP_AMD_LIB")
        lib.rt_config_init(C.byref(cfg))
    return cfg


class ConfigInfo(C.Structure):
    _fields_ = [("num_frames", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("max_depth", C.c_int32),
                ("sqrt_spp", C.c_int32), ("fov_degrees", C.c_float)]


assert C.sizeof(Sphere) == 32 and C.sizeof(Plane) == 80 and C.sizeof(Material) == 64
assert C.sizeof(BvhNode) == 36 and C.sizeof(CameraData) == 76

# The C ABI as ctypes has to be told it: function → (restype — None: void —, argtypes).  A call without a row still "works" (ctypes
# passes a Python int as a 32-bit C int and cuts a device address short), so tests/test_bindings_abi.py holds AMD_ABI against
# include/rtp_amd.h, prototype by prototype.  A new call of the library is one row here and one short method below.
_P, _VP, _STR, _INT, _I32, _U32, _I64, _U64 = C.POINTER, C.c_void_p, C.c_char_p, C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64
_STATUS = C.c_int
_DESC, _CFG, _CAM, _SHARD, _TIMING, _AOV = _P(SceneDesc), _P(Config), _P(CameraData), _P(Shard), _P(Timing), _P(AovBuffers)
_DENOISE, _ADAPTIVE, _STOP, _LENS, _NEE, _ENV = _P(DenoiseParams), _P(AdaptiveParams), _P(StopParams), _P(LensParams), _P(NeeParams), _P(EnvParams)
_LIT, _MEDIUM, _CHROMA, _GLOW, _GLOW_SAMPLE = _P(LitParams), _P(MediumParams), _P(ChromaParams), _P(GlowParams), _P(GlowSampleParams)
_FOG = _P(FogParams)
_OUT = [_VP, _I32, _TIMING]          # how a render call ends: void *hip_stream, int32_t sync, rt_timing *timing

# the calls every build has: a library without one of them fails at load
_AMD_CORE = {
    "rt_timing_init": (None, [_TIMING]),
    "rt_set_device": (_STATUS, [_I32]),
    "rt_scene_create": (_STATUS, [_DESC, _P(_VP)]),
    "rt_config_init": (None, [_CFG]),
    "rt_config_from_env": (None, [_CFG]),
    "rt_scene_create_ex": (_STATUS, [_DESC, _CFG, _P(_VP)]),
    "rt_scene_set_config": (_STATUS, [_VP, _CFG]),
    "rt_scene_get_config": (_STATUS, [_VP, _CFG]),
    "rt_scene_destroy": (_STATUS, [_VP]),
    "rt_scene_guard_reason": (_STR, [_VP]),
    "rt_shard_rows": (_I32, [_I32, _SHARD]),
    "rt_render": (_STATUS, [_VP, _CAM, _SHARD, _VP, *_OUT]),
    "rt_render_tile": (_STATUS, [_VP, _CAM, _I32, _I32, _I32, _I32, _VP, *_OUT]),
    "rt_last_kernel_ms": (_STATUS, [_VP, _P(C.c_float)]),
    "rt_last_timing": (_STATUS, [_VP, _TIMING]),
    "rt_render_to_host": (_STATUS, [_VP, _CAM, _SHARD, _VP, _TIMING]),
    "rt_trace_samples": (_STATUS, [_VP, _CAM, _I32] + [_VP] * 4),
    "rt_closest_hits": (_STATUS, [_VP, _I32] + [_VP] * 5),
    "rt_device_alloc": (_STATUS, [_U64, _P(_VP)]),
    "rt_device_free": (_STATUS, [_VP]),
    "rt_copy_to_host": (_STATUS, [_VP, _VP, _U64]),
    "rt_tonemap": (_STATUS, [_VP, _VP, _I64, _I32, _VP]),
    "rt_context_create": (_STATUS, [_I32, _P(_I32), _P(_VP)]),
    "rt_context_destroy": (_STATUS, [_VP]),
    "rt_context_num_devices": (_I32, [_VP]),
    "rt_context_transport": (_STR, [_VP]),
    "rt_context_scene_create": (_STATUS, [_VP, _DESC, _CFG]),
    "rt_render_sharded": (_STATUS, [_VP, _CAM, _I32, _VP, _TIMING]),
    "rt_gather": (_STATUS, [_VP, _I32, _I32, _I32, _VP]),
    "rt_get_last_error_string": (_STR, []),
    "rt_version_string": (_STR, []),
}
# the calls added since: an older build loaded through RTP_AMD_LIB for an A/B run (developer tools) lacks some and still loads
_AMD_LATER = {
    "rt_config_init_sized": (None, [_CFG, _U32]),
    "rt_render_samples": (_STATUS, [_VP, _CAM, _SHARD, _I32, _VP, *_OUT]),
    "rt_aov_buffers_init": (None, [_AOV]),
    "rt_render_aov": (_STATUS, [_VP, _CAM, _SHARD, _AOV, *_OUT]),
    "rt_render_aov_tile": (_STATUS, [_VP, _CAM, _I32, _I32, _I32, _I32, _AOV, *_OUT]),
    "rt_render_aov_samples": (_STATUS, [_VP, _CAM, _SHARD, _I32, _AOV, *_OUT]),
    "rt_denoise_params_init": (None, [_DENOISE]),
    "rt_denoise_workspace_bytes": (_U64, [_I32, _I32]),
    "rt_denoise": (_STATUS, [_VP, _AOV, _I32, _I32, _I32, _DENOISE, _VP, _U64, _VP, _VP]),
    "rt_denoise_history_bytes": (_U64, [_I32, _I32]),
    "rt_denoise_temporal": (_STATUS, [_VP, _AOV, _CAM, _DENOISE, _VP, _VP, _U64, _VP, _U64, _VP, _VP]),
    "rt_adaptive_params_init": (None, [_ADAPTIVE]),
    "rt_render_adaptive": (_STATUS, [_VP, _CAM, _SHARD, _ADAPTIVE, _VP, _VP, _VP, *_OUT]),
    "rt_tonemap_spp": (_STATUS, [_VP, _VP, _VP, _I64, _VP]),
    "rt_stop_params_init": (None, [_STOP]),
    "rt_render_adaptive_rule": (_STATUS, [_VP, _CAM, _SHARD, _ADAPTIVE, _STOP, _VP, _VP, _VP, *_OUT]),
    "rt_adaptive_judge": (_STATUS, [_I32, _I32, _SHARD, _ADAPTIVE, _STOP, _I32] + [_VP] * 4),
    "rt_denoise_spp": (_STATUS, [_VP, _VP, _VP, _AOV, _I32, _I32, _I32, _DENOISE, _VP, _U64, _VP, _VP]),
    "rt_denoise_temporal_spp": (_STATUS, [_VP, _VP, _VP, _AOV, _I32, _CAM, _DENOISE, _VP, _VP, _U64, _VP, _U64, _VP, _VP]),
    "rt_adaptive_prior": (_STATUS, [_AOV, _I32, _CAM, _VP, _U64, _VP, _VP]),
    "rt_lens_params_init": (None, [_LENS]),
    "rt_render_lens": (_STATUS, [_VP, _CAM, _CAM, _LENS, _SHARD, _I32, _VP, *_OUT]),
    "rt_render_aov_lens": (_STATUS, [_VP, _CAM, _CAM, _LENS, _SHARD, _I32, _AOV, *_OUT]),
    "rt_lens_camera_rays": (_STATUS, [_CAM, _CAM, _LENS, _I32] + [_VP] * 4),
    "rt_nee_params_init": (None, [_P(NeeParamsGlossy)]),
    "rt_render_nee": (_STATUS, [_VP, _CAM, _NEE, _SHARD, _I32, _VP, *_OUT]),
    "rt_nee_light_table": (_STATUS, [_VP, _I32, _VP, _VP, _VP, _P(_I32)]),
    "rt_nee_emitter_table": (_STATUS, [_VP, _NEE, _I32] + [_VP] * 5 + [_P(_I32)]),
    "rt_nee_light_tree": (_STATUS, [_VP, _NEE, _I32, _I32] + [_VP] * 8 + [_P(_I32)] * 2),
    "rt_trace_samples_nee": (_STATUS, [_VP, _CAM, _NEE, _I32] + [_VP] * 5),
    "rt_env_create": (_STATUS, [_VP, _I32, _P(_VP)]),
    "rt_env_destroy": (_STATUS, [_VP]),
    "rt_env_params_init": (None, [_ENV]),
    "rt_render_env": (_STATUS, [_VP, _CAM, _VP, _ENV, _SHARD, _I32, _VP, *_OUT]),
    "rt_env_table": (_STATUS, [_VP, _I32] + [_VP] * 4 + [_P(_I32)]),
    "rt_env_lookup": (_STATUS, [_VP, _I32] + [_VP] * 4),
    "rt_trace_samples_env": (_STATUS, [_VP, _CAM, _VP, _ENV, _I32] + [_VP] * 5),
    "rt_env_from_equirect": (_STATUS, [_VP, _I32, _I32, _I32, _VP]),
    "rt_lit_params_init": (None, [_LIT]),
    "rt_render_lit": (_STATUS, [_VP, _CAM, _LIT, _SHARD, _I32, _VP, *_OUT]),
    "rt_trace_samples_lit": (_STATUS, [_VP, _CAM, _LIT, _I32] + [_VP] * 6),
    "rt_render_lit_adaptive": (_STATUS, [_VP, _CAM, _LIT, _ADAPTIVE, _SHARD, _I32, _VP, _VP, _VP, *_OUT]),
    "rt_render_lit_adaptive_rule": (_STATUS, [_VP, _CAM, _LIT, _ADAPTIVE, _STOP, _SHARD, _I32, _VP, _VP, _VP, *_OUT]),
    "rt_medium_params_init": (None, [_MEDIUM]),
    "rt_render_medium": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _SHARD, _I32, _VP, *_OUT]),
    "rt_trace_samples_medium": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _I32] + [_VP] * 8),
    "rt_volume_create": (_STATUS, [_VP, _I32, _I32, _I32, _P(_VP)]),
    "rt_volume_destroy": (_STATUS, [_VP]),
    "rt_render_volume": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _SHARD, _I32, _VP, *_OUT]),
    "rt_trace_samples_volume": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _I32] + [_VP] * 9),
    "rt_render_volume_adaptive": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _ADAPTIVE, _STOP, _VP, _SHARD, _I32, _VP, _VP, _VP, *_OUT]),
    "rt_render_aov_volume": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _SHARD, _I32, _AOV, _VP, *_OUT]),
    "rt_chroma_params_init": (None, [_CHROMA]),
    "rt_render_chroma": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _CHROMA, _SHARD, _I32, _VP, *_OUT]),
    "rt_trace_samples_chroma": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _CHROMA, _I32] + [_VP] * 9),
    "rt_glow_params_init": (None, [_GLOW]),
    "rt_render_glow": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _GLOW, _VP, _SHARD, _I32, _VP, *_OUT]),
    "rt_trace_samples_glow": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _GLOW, _VP, _I32] + [_VP] * 10),
    "rt_glow_sample_params_init": (None, [_GLOW_SAMPLE]),
    "rt_glow_sampler_create": (_STATUS, [_VP, _I32, _VP, _P(_VP)]),
    "rt_glow_sampler_destroy": (_STATUS, [_VP]),
    "rt_glow_sampler_table": (_STATUS, [_VP, _I32, _I32] + [_VP] * 4 + [_P(_I32)]),
    "rt_render_glow_sampled": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _GLOW, _VP, _GLOW_SAMPLE, _VP, _SHARD, _I32, _VP, *_OUT]),
    "rt_trace_samples_glow_sampled": (_STATUS, [_VP, _CAM, _LIT, _MEDIUM, _VP, _GLOW, _VP, _GLOW_SAMPLE, _VP, _I32] + [_VP] * 11),
    "rt_fog_params_init": (None, [_FOG]),
    "rt_render_fog_adaptive": (_STATUS, [_VP, _CAM, _LIT, _FOG, _ADAPTIVE, _STOP, _VP, _SHARD, _I32, _VP, _VP, _VP, *_OUT]),
    "rt_render_lit_split": (_STATUS, [_VP, _CAM, _LIT, _SHARD, _I32, _VP, _VP, *_OUT]),
    "rt_trace_samples_lit_split": (_STATUS, [_VP, _CAM, _LIT, _I32] + [_VP] * 7),
    "rt_denoise_split_workspace_bytes": (_U64, [_I32, _I32]),
    "rt_denoise_split": (_STATUS, [_VP, _VP, _AOV, _I32, _I32, _I32, _DENOISE, _VP, _U64, _VP, _VP]),
}
# the calls that take a prior: their _rule call (the judgement: the call itself) and, last, the device address of the prior
for _base, _prior in (("rt_render_adaptive_rule", "rt_render_adaptive_prior"), ("rt_render_lit_adaptive_rule", "rt_render_lit_adaptive_prior"),
                      ("rt_adaptive_judge", "rt_adaptive_judge_prior")):
    _AMD_LATER[_prior] = (_STATUS, _AMD_LATER[_base][1] + [_VP])
AMD_ABI = {**_AMD_CORE, **_AMD_LATER}
# Every symbol include/rtp_amd.h declares (tests check that the library exports all of them).
RTP_AMD_SYMBOLS = list(AMD_ABI)

HOST_ABI = {
    "rtp_host_scene_from_config": (_VP, [_STR, _STR]),
    "rtp_host_scene_rtiow": (_VP, [_U32, _I32, _I32, _I32]),
    "rtp_host_scene_from_arrays": (_VP, [_VP, _I32, _VP, _I32, _P(Material), _I32]),
    "rtp_host_scene_free": (_INT, [_VP]),
    "rtp_host_scene_desc": (_INT, [_VP, _DESC]),
    "rtp_host_scene_config": (_INT, [_VP, _P(ConfigInfo)]),
    "rtp_host_frame_camera": (_INT, [_VP, _I32, _CAM]),
    "rtp_host_frame_camera_at": (_INT, [_VP, C.c_float, _CAM]),
    "rtp_host_make_camera": (_INT, [_I32, _I32, C.c_float, _P(C.c_float), _P(C.c_float), _P(C.c_float), _I32, _I32, _CAM]),
    "rtp_host_quantize": (_INT, [_VP, _I64, _I32, _VP]),
    "rtp_host_write_binary_image": (_INT, [_STR, _VP, _I32, _I32, _I32]),
    "rtp_host_write_png": (_INT, [_STR, _VP, _I32, _I32, _I32]),
    "rtp_host_load_hdr": (_INT, [_STR, _P(_I32), _P(_I32), _VP]),
    "rtp_host_default_config": (_STR, []),
}


def _declare(lib, abi, required):
    """Gives the functions of lib their rows of abi.  One of `required` that lib lacks fails here, at load; the others are skipped."""
    for name, (restype, argtypes) in abi.items():
        if name in required or hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = restype, argtypes
    return lib


_host = None
_amd = None


def host_lib():
    """librtp_host.so (pure host)."""
    global _host
    if _host is None:
        path = os.path.join(_HERE, "librtp_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (or make -C ray-tracing-practice_amd)")
        _host = _declare(C.CDLL(path), HOST_ABI, HOST_ABI)
    return _host


def amd_lib():
    """librtp_amd.so (HIP).  Raises if the library is not built — there is no fallback."""
    global _amd
    if _amd is None:
        # RTP_AMD_LIB: developer override used by tools/ to A/B differently compiled kernels
        path = os.environ.get("RTP_AMD_LIB") or os.path.join(_HERE, "librtp_amd.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: the HIP render library must be built (no CPU fallback exists)")
        _amd = _declare(C.CDLL(path), AMD_ABI, _AMD_CORE)
    return _amd


class RtError(RuntimeError):
    pass


def _check(status, what):
    if status != 0:
        msg = amd_lib().rt_get_last_error_string().decode()
        raise RtError(f"{what} failed with rt_status {status}: {msg}")


class HostScene:
    """Host-side scene (arrays in the reference's layouts) built by librtp_host.so."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError("host scene construction failed")
        self._h = C.c_void_p(handle)
        self.desc = SceneDesc()
        host_lib().rtp_host_scene_desc(self._h, C.byref(self.desc))
        self.info = ConfigInfo()
        host_lib().rtp_host_scene_config(self._h, C.byref(self.info))

    @classmethod
    def from_config(cls, text, texture_dir=""):
        return cls(host_lib().rtp_host_scene_from_config(text.encode(), (texture_dir or "").encode()))

    @classmethod
    def rtiow(cls, seed=12345, half_extent=11, textured_quad=False, texture_size=1024):
        return cls(host_lib().rtp_host_scene_rtiow(seed, half_extent, int(textured_quad), texture_size))

    @classmethod
    def from_arrays(cls, spheres, planes, materials):
        """spheres: [n,5] (cx,cy,cz,radius,material); planes: [n,11] (base,u,v,material,type);
        materials: list of Material."""
        sp = np.ascontiguousarray(np.asarray(spheres, dtype=np.float32).reshape(-1, 5))
        pl = np.ascontiguousarray(np.asarray(planes, dtype=np.float32).reshape(-1, 11))
        mats = (Material * max(len(materials), 1))(*materials)
        return cls(host_lib().rtp_host_scene_from_arrays(sp.ctypes.data, sp.shape[0], pl.ctypes.data, pl.shape[0], mats,
                                                         len(materials)))

    def frame_camera(self, frame=0):
        cam = CameraData()
        host_lib().rtp_host_frame_camera(self._h, frame, C.byref(cam))
        return cam

    def frame_camera_at(self, frame_time):
        """The orbit's camera at a fractional frame (rtp_host_frame_camera_at)."""
        cam = CameraData()
        host_lib().rtp_host_frame_camera_at(self._h, frame_time, C.byref(cam))
        return cam

    def nodes_array(self):
        n = self.desc.num_nodes
        return np.ctypeslib.as_array(C.cast(self.desc.nodes, C.POINTER(C.c_int32)), shape=(n, 9)).copy()

    def close(self):
        if self._h:
            host_lib().rtp_host_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_hdr_image(path):
    """rtp_main --env's loader (host/texture_io.cpp): a PFM or Radiance .hdr file → (h, w, 3) float32, top row first."""
    lib = host_lib()
    w, h = C.c_int32(), C.c_int32()
    if lib.rtp_host_load_hdr(os.fsencode(path), C.byref(w), C.byref(h), None) != 0:
        raise RtError(f"cannot load {path} as a PFM or Radiance image")
    out = np.empty((h.value, w.value, 3), dtype=np.float32)
    if lib.rtp_host_load_hdr(os.fsencode(path), C.byref(w), C.byref(h), out.ctypes.data) != 0:
        raise RtError(f"cannot load {path} as a PFM or Radiance image")
    return out


def make_camera(width, height, vfov, eye, target, background=(0, 0, 0), spp=1, max_depth=50):
    cam = CameraData()
    f3 = C.c_float * 3
    host_lib().rtp_host_make_camera(width, height, vfov, f3(*eye), f3(*target), f3(*background), spp, max_depth,
                                    C.byref(cam))
    return cam


def rtiow_camera(width, height, spp, max_depth=50):
    """Benchmark camera of SURVEY.md §8(d): from (13,3,2) at the origin, vfov 20, sky (0.7,0.8,1.0)."""
    return make_camera(width, height, 20.0, (13, 3, 2), (0, 0, 0), (0.7, 0.8, 1.0), spp, max_depth)


def quantize(fb_sum, divisor):
    fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
    out = np.empty(fb.size, dtype=np.uint8)
    host_lib().rtp_host_quantize(fb.ctypes.data, fb.size // 3, divisor, out.ctypes.data)
    return out.reshape(fb.shape)


def binary_image_bytes(fb_sum, width, height, divisor):
    """Bytes of the file BinarySaver writes (src/camera.cu:128-153)."""
    return np.array([width, height], dtype=np.int32).tobytes() + quantize(fb_sum, divisor).tobytes()


# Developer tools (tools/*.py) set HONOUR_ENV = True: handles made without an explicit honour_env then overlay the RTP_*
# variables through rt_config_from_env().  Tests and bench.py leave it off: they configure through rt_config fields only.
HONOUR_ENV = False
# rt_config fields every DeviceScene made without them starts from (a test fixture's way to say "guarded walk throughout")
DEFAULTS = {}


def denoise_params(**params):
    """rt_denoise_params with the library's defaults (rt_denoise_params_init), then the given fields (iterations, sigma_depth,
    sigma_luminance, normal_squarings)."""
    return _params(DenoiseParams, "rt_denoise_params", ("iterations", "sigma_depth", "sigma_luminance", "normal_squarings"), params,
                   unknown=lambda k: TypeError(f"rt_denoise_params has no field {k!r}"))


# rt_denoise workspaces, one per size: allocated on the device current at their first use (a caller that switches devices
# passes workspace=(address, bytes) of its own)
_denoise_workspaces = {}


def _denoise_workspace(width, height):
    """(address, bytes) of the shared rt_denoise workspace of a width x height image ((None, 0) for an empty image)."""
    lib = amd_lib()
    need = lib.rt_denoise_workspace_bytes(width, height)
    workspace = _denoise_workspaces.get(need)
    if workspace is None and need > 0:
        d = C.c_void_p()
        _check(lib.rt_device_alloc(need, C.byref(d)), "rt_device_alloc")
        workspace = _denoise_workspaces[need] = (d.value, need)
    return workspace or (None, 0)


def denoise(d_fb, aov_ptrs, width, height, spp, d_out, stream=None, workspace=None, **params):
    """rt_denoise on device addresses: d_fb (the beauty sums), aov_ptrs {"albedo", "normal", "depth", "hits"} → device address (as
    DeviceScene.render_aov takes them), d_out (width * height * 3 floats).  Only enqueues on `stream` (None = default stream).
    params: rt_denoise_params fields."""
    lib = amd_lib()
    b = _aov_struct(aov_ptrs)
    ws_ptr, ws_bytes = workspace or _denoise_workspace(width, height)
    p = denoise_params(**params)
    _check(lib.rt_denoise(C.c_void_p(d_fb), C.byref(b), width, height, spp, C.byref(p), C.c_void_p(ws_ptr), ws_bytes, C.c_void_p(d_out),
                          C.c_void_p(stream or 0)), "rt_denoise")


def denoise_split(d_direct, d_indirect, aov_ptrs, width, height, spp, d_out, stream=None, workspace=None, **params):
    """rt_denoise_split on device addresses: d_direct and d_indirect as DeviceScene.render_lit_split wrote them, the rest as denoise()
    takes it.  workspace: None (the module's shared one of that size), or (address, bytes) of at least rt_denoise_split_workspace_bytes.
    Only enqueues on `stream`.  params: rt_denoise_params fields."""
    lib = amd_lib()
    b = _aov_struct(aov_ptrs)
    p = denoise_params(**params)
    if workspace is None:
        need = lib.rt_denoise_split_workspace_bytes(width, height)
        workspace = _denoise_workspaces.get(("split", need))
        if workspace is None:
            d = C.c_void_p()
            _check(lib.rt_device_alloc(need, C.byref(d)), "rt_device_alloc")
            workspace = _denoise_workspaces[("split", need)] = (d.value, need)
    ws_ptr, ws_bytes = workspace
    _check(lib.rt_denoise_split(C.c_void_p(d_direct), C.c_void_p(d_indirect), C.byref(b), width, height, spp, C.byref(p), C.c_void_p(ws_ptr), ws_bytes,
                                C.c_void_p(d_out), C.c_void_p(stream or 0)), "rt_denoise_split")


def _aov_struct(aov_ptrs):
    b = AovBuffers()
    for key, field, _, _ in AOV_CHANNELS:
        if aov_ptrs.get(key):
            setattr(b, field, aov_ptrs[key])
    return b


def denoise_spp(d_fb, d_spp, d_moments, aov_ptrs, aov_spp, width, height, d_out, stream=None, workspace=None, **params):
    """rt_denoise_spp on device addresses: d_fb, d_spp and d_moments (or None) as DeviceScene.render_adaptive / render_lit_adaptive
    wrote them for a whole frame, aov_ptrs {"albedo", "normal", "depth", "hits"} → device address of the AOV sums at aov_spp samples
    per pixel, d_out (width * height * 3 floats).  Only enqueues on `stream` (None = default stream).  params: rt_denoise_params
    fields."""
    b = _aov_struct(aov_ptrs)
    ws_ptr, ws_bytes = workspace or _denoise_workspace(width, height)
    p = denoise_params(**params)
    _check(amd_lib().rt_denoise_spp(C.c_void_p(d_fb), C.c_void_p(d_spp), C.c_void_p(d_moments or 0), C.byref(b), aov_spp, width, height,
                                    C.byref(p), C.c_void_p(ws_ptr), ws_bytes, C.c_void_p(d_out), C.c_void_p(stream or 0)), "rt_denoise_spp")


def denoise_temporal(d_fb, aov_ptrs, cam, d_history_prev, d_history_next, history_bytes, d_out, workspace, stream=None, **params):
    """rt_denoise_temporal on device addresses: d_fb (the beauty sums of cam), aov_ptrs {"albedo", "normal", "depth", "hits",
    "prim"} → device address, d_history_prev (None: no history) and d_history_next (history_bytes each), d_out (3 floats per
    pixel), workspace = (address, bytes) of at least rt_denoise_workspace_bytes.  Only enqueues on `stream` (None = default
    stream).  params: rt_denoise_params fields."""
    b = _aov_struct(aov_ptrs)
    p = denoise_params(**params)
    ws_ptr, ws_bytes = workspace
    _check(amd_lib().rt_denoise_temporal(C.c_void_p(d_fb), C.byref(b), C.byref(cam), C.byref(p), C.c_void_p(d_history_prev or 0),
                                         C.c_void_p(d_history_next), history_bytes, C.c_void_p(ws_ptr), ws_bytes, C.c_void_p(d_out),
                                         C.c_void_p(stream or 0)), "rt_denoise_temporal")


def denoise_temporal_spp(d_fb, d_spp, d_moments, aov_ptrs, aov_spp, cam, d_history_prev, d_history_next, history_bytes, d_out, workspace,
                         stream=None, **params):
    """rt_denoise_temporal_spp on device addresses: d_fb, d_spp and d_moments (or None) as DeviceScene.render_adaptive /
    render_lit_adaptive wrote them for a whole frame of cam, aov_ptrs {"albedo", "normal", "depth", "hits", "prim"} → device address
    of the AOV sums at aov_spp samples per pixel, d_history_prev (None: no history) and d_history_next (history_bytes each), d_out
    (3 floats per pixel), workspace = (address, bytes) of at least rt_denoise_workspace_bytes.  Only enqueues on `stream` (None =
    default stream).  params: rt_denoise_params fields."""
    b = _aov_struct(aov_ptrs)
    p = denoise_params(**params)
    ws_ptr, ws_bytes = workspace
    _check(amd_lib().rt_denoise_temporal_spp(C.c_void_p(d_fb), C.c_void_p(d_spp), C.c_void_p(d_moments or 0), C.byref(b), aov_spp, C.byref(cam),
                                             C.byref(p), C.c_void_p(d_history_prev or 0), C.c_void_p(d_history_next), history_bytes,
                                             C.c_void_p(ws_ptr), ws_bytes, C.c_void_p(d_out), C.c_void_p(stream or 0)), "rt_denoise_temporal_spp")


def adaptive_prior(aov_ptrs, aov_spp, cam, d_history_prev, history_bytes, d_prior, stream=None):
    """rt_adaptive_prior on device addresses: aov_ptrs {"albedo", "normal", "depth", "hits", "prim"} → device address of the AOV sums of
    the frame about to be rendered at aov_spp samples per pixel, cam its camera, d_history_prev (None: no history) a history of
    rt_denoise_temporal_spp of history_bytes, d_prior 2 floats per pixel.  Only enqueues on `stream` (None = default stream)."""
    b = _aov_struct(aov_ptrs)
    _check(amd_lib().rt_adaptive_prior(C.byref(b), aov_spp, C.byref(cam), C.c_void_p(d_history_prev or 0), history_bytes, C.c_void_p(d_prior),
                                       C.c_void_p(stream or 0)), "rt_adaptive_prior")


_hip_rt = None


def _hip():
    """The HIP runtime librtp_amd.so itself runs on (already loaded with it: found by soname, never loaded a second time), for the
    host-to-device copies of _DeviceBuffers.upload — the C ABI has no upload call of its own."""
    global _hip_rt
    if _hip_rt is None:
        amd_lib()
        for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
            try:
                _hip_rt = C.CDLL(name, mode=os.RTLD_NOLOAD | os.RTLD_LAZY)
                break
            except OSError:
                continue
        if _hip_rt is None:
            raise RuntimeError("the HIP runtime of librtp_amd.so is not loaded")
        _hip_rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip_rt


class _DeviceBuffers:
    """The temporary device buffers of one call, as integer device addresses: `with _DeviceBuffers() as dev:` frees every one of them
    on exit, whether the call returned or raised."""

    def __enter__(self):
        self._held = []
        return self

    def __exit__(self, *exc):
        for d in self._held:
            amd_lib().rt_device_free(d)

    def alloc(self, nbytes):
        """A fresh buffer of nbytes — of 12 bytes, one pixel, for an empty request: every call gets an address to pass."""
        d = C.c_void_p()
        _check(amd_lib().rt_device_alloc(nbytes or 12, C.byref(d)), "rt_device_alloc")
        self._held.append(d)
        return d.value

    def upload(self, a):
        """A fresh buffer holding the host array a (for an empty one no copy is issued)."""
        d = self.alloc(a.nbytes)
        if a.nbytes and _hip().hipMemcpy(d, a.ctypes.data, a.nbytes, 1) != 0:       # hipMemcpyHostToDevice
            raise RtError("hipMemcpy host to device failed")
        return d

    def upload_aov(self, aov, channels=AOV_CHANNELS):
        """The arrays of render_aov_to_host's dict in fresh buffers: {key: address}, as the calls on device addresses take them."""
        return {key: self.upload(np.ascontiguousarray(aov[key], dtype=dtype)) for key, _, dtype, _ in channels}

    def download(self, d, a):
        """The buffer at d into the host array a, which it returns."""
        _check(amd_lib().rt_copy_to_host(a.ctypes.data, d, a.nbytes), "rt_copy_to_host")
        return a


def _frame_to_host(cam, shard, render):
    """The body of a render_*_to_host: the rows of rt_shard_rows, render(device address of rows x width x 3 floats) → rt_timing, the
    copy back.  Returns ((rows, width, 3) float32 sums, rt_timing)."""
    fb = np.empty((amd_lib().rt_shard_rows(cam.image_height, _ref(shard)), cam.image_width, 3), dtype=np.float32)
    with _DeviceBuffers() as dev:
        d = dev.alloc(fb.nbytes)
        t = render(d)
        dev.download(d, fb)
    return fb, t


def _adaptive_to_host(cam, shard, prior, render):
    """The body of a render_*_adaptive_to_host: render(d_fb, d_spp, d_moments, d_prior) → rt_timing, d_prior None or the address of the
    uploaded host array prior (rows, w, 2).  Returns (fb (rows, w, 3) float32, spp (rows, w) int32, moments (rows, w, 2) float32,
    rt_timing)."""
    rows, w = amd_lib().rt_shard_rows(cam.image_height, _ref(shard)), cam.image_width
    out = np.empty((rows, w, 3), dtype=np.float32), np.empty((rows, w), dtype=np.int32), np.empty((rows, w, 2), dtype=np.float32)
    with _DeviceBuffers() as dev:
        ptrs = [dev.alloc(a.nbytes) for a in out]
        d_prior = None if prior is None else dev.upload(np.ascontiguousarray(np.asarray(prior, dtype=np.float32).reshape(rows, w, 2)))
        t = render(*ptrs, d_prior)
        for d, a in zip(ptrs, out):
            dev.download(d, a)
    return (*out, t)


def _aov_to_host(rows, w, render):
    """The body of a render_aov_*_to_host: render({key: device address} of the five AOV_CHANNELS, rows x w pixels each) → rt_timing.
    Returns ({key: array}, rt_timing)."""
    pixels = max(w, 0) * max(rows, 0)
    with _DeviceBuffers() as dev:
        ptrs = {key: dev.alloc(pixels * per * 4) for key, _, _, per in AOV_CHANNELS}
        t = render(ptrs)
        out = {key: dev.download(ptrs[key], np.empty((rows, w, per) if per > 1 else (rows, w), dtype=dtype))
               for key, _, dtype, per in AOV_CHANNELS}
    return out, t


def denoise_to_host(fb_sum, aov, spp, **params):
    """rt_denoise of host arrays: fb_sum (H, W, 3) float32 as DeviceScene.render_to_host returns it, aov the dict of
    DeviceScene.render_aov_to_host (albedo, normal, depth, hits; prim is not used).  Returns the (H, W, 3) float32 output, the sum
    over samples like fb_sum.  Synchronous (default stream)."""
    fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
    height, width = fb.shape[:2]
    with _DeviceBuffers() as dev:
        d_out = dev.alloc(fb.nbytes)
        denoise(dev.upload(fb), dev.upload_aov(aov, AOV_CHANNELS[:4]), width, height, spp, d_out, **params)
        return dev.download(d_out, np.empty_like(fb))


def denoise_split_to_host(direct_sum, indirect_sum, aov, spp, **params):
    """rt_denoise_split of host arrays: direct_sum and indirect_sum (H, W, 3) float32 as DeviceScene.render_lit_split_to_host returns them,
    aov the dict of DeviceScene.render_aov_to_host.  Returns the (H, W, 3) float32 output.  Synchronous (default stream)."""
    a = np.ascontiguousarray(direct_sum, dtype=np.float32)
    b = np.ascontiguousarray(indirect_sum, dtype=np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    height, width = a.shape[:2]
    with _DeviceBuffers() as dev:
        d_out = dev.alloc(a.nbytes)
        need = amd_lib().rt_denoise_split_workspace_bytes(width, height)
        denoise_split(dev.upload(a), dev.upload(b), dev.upload_aov(aov, AOV_CHANNELS[:4]), width, height, spp, d_out, workspace=(dev.alloc(need), need), **params)
        return dev.download(d_out, np.empty_like(a))


def denoise_spp_to_host(fb_sum, spp, moments, aov, aov_spp, **params):
    """rt_denoise_spp of host arrays: fb_sum (H, W, 3) float32, spp (H, W) int32 and moments (H, W, 2) float32 or None as
    DeviceScene.render_adaptive_to_host returns them, aov the dict of DeviceScene.render_aov_to_host at aov_spp samples per pixel.
    Returns the (H, W, 3) float32 output, each pixel the sum over its own samples like fb_sum.  Synchronous (default stream)."""
    fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
    height, width = fb.shape[:2]
    with _DeviceBuffers() as dev:
        d_moments = None if moments is None else dev.upload(np.ascontiguousarray(moments, dtype=np.float32))
        d_out = dev.alloc(fb.nbytes)
        denoise_spp(dev.upload(fb), dev.upload(np.ascontiguousarray(spp, dtype=np.int32)), d_moments, dev.upload_aov(aov, AOV_CHANNELS[:4]),
                    aov_spp, width, height, d_out, **params)
        return dev.download(d_out, np.empty_like(fb))


def adaptive_judge(moments, n, going_on=None, shard=None, rule=0, prior=None, **params):
    """rt_adaptive_judge: one judgement of a stopping rule on the current device.  moments (rows, width, 2) float32 (S1, S2); going_on
    None (every pixel) or (rows, width) bool; prior None or (rows, width, 2) float32 (ch, vh): given, the call is
    rt_adaptive_judge_prior; params are rt_adaptive_params fields.  Returns goes_on (rows, width) bool."""
    mom = np.ascontiguousarray(moments, dtype=np.float32)
    rows, width = mom.shape[:2]
    out = np.empty((rows, width), dtype=np.uint8)
    p, stop = adaptive_params(**params), stop_params(rule=rule)
    with _DeviceBuffers() as dev:
        d_going_on = None if going_on is None else dev.upload(np.ascontiguousarray(np.asarray(going_on).reshape(rows, width), dtype=np.uint8))
        d_out = dev.alloc(out.nbytes)
        args = (width, rows, _ref(shard), C.byref(p), C.byref(stop), n, dev.upload(mom), d_going_on, d_out, None)
        if prior is None:
            _check(amd_lib().rt_adaptive_judge(*args), "rt_adaptive_judge")
        else:
            d_prior = dev.upload(np.ascontiguousarray(np.asarray(prior, dtype=np.float32).reshape(rows, width, 2)))
            _check(amd_lib().rt_adaptive_judge_prior(*args, d_prior), "rt_adaptive_judge_prior")
        dev.download(d_out, out)
    return out.astype(bool)


class TemporalDenoiser:
    """rt_denoise_temporal over the frames of an animation: owns the two history buffers and the workspace of a width x height
    image on the device current at construction.  step_to_host() denoises one frame and keeps its history for the next one;
    reset() forgets the history (a cut).  params: rt_denoise_params fields, the same for every frame.  step_spp() and
    step_spp_to_host() are the same for adaptively sampled frames (rt_denoise_temporal_spp); a history of the one call is empty to
    the other, so mixing them on one object restarts the history at every change."""

    def __init__(self, width, height, **params):
        lib = amd_lib()
        self.width, self.height, self.params = width, height, dict(params)
        denoise_params(**params)                              # (unknown fields fail here, not at the first frame)
        self.history_bytes = lib.rt_denoise_history_bytes(width, height)
        self.workspace_bytes = lib.rt_denoise_workspace_bytes(width, height)
        if self.history_bytes == 0:
            raise RtError(f"TemporalDenoiser: no image of {width} x {height}")
        self._dev = []
        try:
            for n in (self.history_bytes, self.history_bytes, self.workspace_bytes):
                d = C.c_void_p()
                _check(lib.rt_device_alloc(n, C.byref(d)), "rt_device_alloc")
                self._dev.append(d)
        except Exception:
            self.close()
            raise
        self._prev, self._next = self._dev[0].value, self._dev[1].value
        self._have = False

    def reset(self):
        """The next frame starts without history."""
        self._have = False

    def step(self, d_fb, aov_ptrs, cam, d_out, stream=None):
        """One frame on device addresses (denoise_temporal); only enqueues on `stream`."""
        if (cam.image_width, cam.image_height) != (self.width, self.height):
            raise RtError(f"TemporalDenoiser: a {cam.image_width} x {cam.image_height} frame for a {self.width} x {self.height} history")
        denoise_temporal(d_fb, aov_ptrs, cam, self._prev if self._have else None, self._next, self.history_bytes, d_out,
                         (self._dev[2].value, self.workspace_bytes), stream=stream, **self.params)
        self._prev, self._next = self._next, self._prev
        self._have = True

    def step_to_host(self, fb_sum, aov, cam):
        """One frame of host arrays: fb_sum (H, W, 3) float32 as DeviceScene.render_to_host returns it, aov the dict of
        DeviceScene.render_aov_to_host (prim included), cam its camera.  Returns the (H, W, 3) float32 output, the sum over samples
        like fb_sum.  Synchronous (default stream)."""
        fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
        with _DeviceBuffers() as dev:
            d_out = dev.alloc(fb.nbytes)
            self.step(dev.upload(fb), dev.upload_aov(aov), cam, d_out)
            return dev.download(d_out, np.empty_like(fb))

    def step_spp(self, d_fb, d_spp, d_moments, aov_ptrs, aov_spp, cam, d_out, stream=None):
        """One adaptively sampled frame on device addresses (denoise_temporal_spp); only enqueues on `stream`."""
        if (cam.image_width, cam.image_height) != (self.width, self.height):
            raise RtError(f"TemporalDenoiser: a {cam.image_width} x {cam.image_height} frame for a {self.width} x {self.height} history")
        denoise_temporal_spp(d_fb, d_spp, d_moments, aov_ptrs, aov_spp, cam, self._prev if self._have else None, self._next, self.history_bytes,
                             d_out, (self._dev[2].value, self.workspace_bytes), stream=stream, **self.params)
        self._prev, self._next = self._next, self._prev
        self._have = True

    def step_spp_to_host(self, fb_sum, spp, moments, aov, aov_spp, cam):
        """One frame of host arrays: fb_sum (H, W, 3) float32, spp (H, W) int32 and moments (H, W, 2) float32 or None as
        DeviceScene.render_adaptive_to_host returns them, aov the dict of DeviceScene.render_aov_to_host (prim included) at aov_spp
        samples per pixel, cam their camera.  Returns the (H, W, 3) float32 output, each pixel the sum over its own samples like
        fb_sum.  Synchronous (default stream)."""
        fb = np.ascontiguousarray(fb_sum, dtype=np.float32)
        with _DeviceBuffers() as dev:
            d_moments = None if moments is None else dev.upload(np.ascontiguousarray(moments, dtype=np.float32))
            d_out = dev.alloc(fb.nbytes)
            self.step_spp(dev.upload(fb), dev.upload(np.ascontiguousarray(spp, dtype=np.int32)), d_moments, dev.upload_aov(aov), aov_spp, cam, d_out)
            return dev.download(d_out, np.empty_like(fb))

    def prior(self, aov_ptrs, aov_spp, cam, d_prior, stream=None):
        """rt_adaptive_prior of the frame about to be rendered (its AOVs at aov_spp samples per pixel and its camera) on the history the
        next step_spp will read — none before the first step and after reset() — into d_prior (2 floats per pixel); only enqueues on
        `stream`."""
        if (cam.image_width, cam.image_height) != (self.width, self.height):
            raise RtError(f"TemporalDenoiser: a {cam.image_width} x {cam.image_height} frame for a {self.width} x {self.height} history")
        adaptive_prior(aov_ptrs, aov_spp, cam, self._prev if self._have else None, self.history_bytes, d_prior, stream=stream)

    def prior_to_host(self, aov, aov_spp, cam):
        """prior() of host arrays: aov the dict of DeviceScene.render_aov_to_host (prim included).  Returns (H, W, 2) float32 (ch, vh).
        Synchronous (default stream)."""
        out = np.empty((self.height, self.width, 2), dtype=np.float32)
        with _DeviceBuffers() as dev:
            d_prior = dev.alloc(out.nbytes)
            self.prior(dev.upload_aov(aov), aov_spp, cam, d_prior)
            return dev.download(d_prior, out)

    def history_to_host(self):
        """The history the last step wrote (uint8 array of rt_denoise_history_bytes; the header's layout)."""
        h = np.empty(self.history_bytes, np.uint8)
        _check(amd_lib().rt_copy_to_host(h.ctypes.data, C.c_void_p(self._prev), h.nbytes), "rt_copy_to_host")
        return h

    def close(self):
        for d in self._dev:
            amd_lib().rt_device_free(d)
        self._dev = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _adaptive_entry(base, rule, prior):
    """Which of the three entry points of an adaptive render call (rule, prior) ask for: (its name, its rt_stop_params argument, its
    arguments after the rt_timing).  No rule and no prior: the call `base` itself; a prior: base_prior, with rule 0 unless given; else
    base_rule.  Three symbols of the ABI, each reached."""
    if prior is not None:
        return base + "_prior", (C.byref(stop_params(rule=rule or 0)),), (C.c_void_p(prior),)
    if rule is None:
        return base, (), ()
    return base + "_rule", (C.byref(stop_params(rule=rule)),), ()


class DeviceScene:
    """rt_scene handle (device-resident repacked scene).

    Configuration: keyword arguments are rt_config fields (e.g. traversal=rb.TRAVERSAL_EXACT, pass_spp=64,
    tree_build=rb.BUILD_DEVICE_LBVH); configure(**fields) changes the render-time ones later.  With
    honour_env=True (what developer tools ask for through rb.HONOUR_ENV; the library itself never reads the
    environment) the RTP_* developer variables are overlaid through rt_config_from_env() at creation and
    before every render, so a harness can flip a knob around a single call."""

    def __init__(self, host_scene, device=None, honour_env=None, **config):
        lib = amd_lib()
        if device is not None:
            _check(lib.rt_set_device(device), "rt_set_device")
        self._h = C.c_void_p()
        self._honour_env = HONOUR_ENV if honour_env is None else honour_env
        self._explicit = dict(config)
        cfg = self._make_config()
        _check(lib.rt_scene_create_ex(C.byref(host_scene.desc), C.byref(cfg), C.byref(self._h)), "rt_scene_create_ex")
        self._keep = host_scene

    def _make_config(self):
        cfg = new_config()
        for k, v in {**DEFAULTS, **self._explicit}.items():
            setattr(cfg, k, v)
        if self._honour_env:
            amd_lib().rt_config_from_env(C.byref(cfg))
        return cfg

    def configure(self, **fields):
        """Change render-time rt_config fields of this handle."""
        self._explicit.update(fields)
        self._apply_config()

    def _apply_config(self):
        cfg = self._make_config()
        _check(amd_lib().rt_scene_set_config(self._h, C.byref(cfg)), "rt_scene_set_config")

    def config(self):
        cfg = Config()
        cfg.struct_bytes = C.sizeof(Config)
        _check(amd_lib().rt_scene_get_config(self._h, C.byref(cfg)), "rt_scene_get_config")
        return cfg

    def _call(self, name, *args, after=()):
        """The library's call `name` on this handle with the handle's configuration in force — name(handle, *args, rt_timing, *after) —
        and the rt_timing it filled."""
        t = Timing()
        self._apply_config()
        _check(getattr(amd_lib(), name)(self._h, *args, C.byref(t), *after), name)
        return t

    def render_to_host(self, cam, shard=None, sample_first=0):
        """The frame's sums as a (rows, width, 3) float32 array and the rt_timing; sample_first != 0: samples sample_first … of
        every pixel (rt_render_samples through a fresh device buffer)."""
        if sample_first:
            return _frame_to_host(cam, shard, lambda d: self.render(cam, d, shard=shard, sample_first=sample_first))
        fb = np.empty((amd_lib().rt_shard_rows(cam.image_height, _ref(shard)), cam.image_width, 3), dtype=np.float32)
        return fb, self._call("rt_render_to_host", C.byref(cam), _ref(shard), fb.ctypes.data)

    def render(self, cam, d_fb_ptr, shard=None, stream=None, sync=True, sample_first=0):
        """d_fb_ptr: integer device address (e.g. torch tensor.data_ptr()).  sample_first != 0: rt_render_samples."""
        if sample_first:
            return self._call("rt_render_samples", C.byref(cam), _ref(shard), sample_first, C.c_void_p(d_fb_ptr), *_stream_sync(stream, sync))
        return self._call("rt_render", C.byref(cam), _ref(shard), C.c_void_p(d_fb_ptr), *_stream_sync(stream, sync))

    def render_tile_to_host(self, cam, x0, y0, w, h):
        """rt_render_tile into a fresh device buffer, copied to the host: (h, w, 3) float32 sums and the rt_timing."""
        with _DeviceBuffers() as dev:          # (not _frame_to_host: the result is the tile's, made once the library has taken the tile)
            d = dev.alloc(max(w, 0) * max(h, 0) * 12)
            t = self._call("rt_render_tile", C.byref(cam), x0, y0, w, h, d, C.c_void_p(0), 1)
            return dev.download(d, np.empty((h, w, 3), dtype=np.float32)), t

    def render_aov(self, cam, ptrs, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_aov (rt_render_aov_samples for sample_first != 0).  ptrs: {"albedo", "normal", "depth", "hits", "prim"} →
        integer device address (missing / None: not written).  Returns the rt_timing."""
        b = _aov_struct(ptrs)
        if sample_first:
            return self._call("rt_render_aov_samples", C.byref(cam), _ref(shard), sample_first, C.byref(b), *_stream_sync(stream, sync))
        return self._call("rt_render_aov", C.byref(cam), _ref(shard), C.byref(b), *_stream_sync(stream, sync))

    def render_aov_to_host(self, cam, shard=None, tile=None, sample_first=0):
        """The AOVs of the frame, a shard of its rows or a tile (x0, y0, w, h) through fresh device buffers: ({"albedo": (rows, w, 3),
        "normal": (rows, w, 3), "depth": (rows, w), "hits": (rows, w) uint32, "prim": (rows, w) int32}, rt_timing).  sample_first
        != 0: samples sample_first … (rt_render_aov_samples; not for a tile)."""
        if tile is not None and sample_first:
            raise RtError("render_aov_to_host: a tile has no sample_first (rt_render_aov_samples renders rows)")
        if tile is not None:
            x0, y0, w, rows = tile
            return _aov_to_host(rows, w, lambda ptrs: self._call("rt_render_aov_tile", C.byref(cam), x0, y0, w, rows, C.byref(_aov_struct(ptrs)),
                                                                 C.c_void_p(0), 1))
        return _aov_to_host(amd_lib().rt_shard_rows(cam.image_height, _ref(shard)), cam.image_width,
                            lambda ptrs: self.render_aov(cam, ptrs, shard=shard, sample_first=sample_first))

    def render_adaptive(self, cam, d_fb_ptr, d_spp_ptr, d_moments_ptr=None, shard=None, stream=None, sync=True, prior=None, **params):
        """rt_render_adaptive: d_fb_ptr (3 floats per pixel), d_spp_ptr (1 int32 per pixel), d_moments_ptr (None, or 2 floats per pixel)
        are integer device addresses; params are rt_adaptive_params fields (min_spp, batch_spp, max_spp, threshold) and rule (0 or 1:
        given, the call goes through rt_render_adaptive_rule with that rt_stop_params.rule); prior: None, or the device address of 2
        floats per local pixel (rt_render_adaptive_prior, rule 0 unless given).  Returns the rt_timing."""
        rule = params.pop("rule", None)
        p = adaptive_params(**params)
        name, stop, after = _adaptive_entry("rt_render_adaptive", rule, prior)
        return self._call(name, C.byref(cam), _ref(shard), C.byref(p), *stop, C.c_void_p(d_fb_ptr), C.c_void_p(d_spp_ptr),
                          C.c_void_p(d_moments_ptr or 0), *_stream_sync(stream, sync), after=after)

    def render_adaptive_to_host(self, cam, shard=None, prior=None, **params):
        """rt_render_adaptive through fresh device buffers: (fb (rows, w, 3) float32 sums, spp (rows, w) int32, moments (rows, w, 2)
        float32 (S1, S2)) and the rt_timing.  prior: None or a host array (rows, w, 2) float32 (ch, vh)."""
        return _adaptive_to_host(cam, shard, prior, lambda d_fb, d_spp, d_moments, d_prior: self.render_adaptive(
            cam, d_fb, d_spp, d_moments, shard=shard, prior=d_prior, **params))

    def render_lens(self, cam_open, d_fb_ptr, cam_close=None, lens=None, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_lens: cam_close None = no motion; lens None (defaults), a LensParams or a dict of its fields.  Returns the
        rt_timing of this call."""
        return self._call("rt_render_lens", C.byref(cam_open), _ref(cam_close), _lens_struct(lens), _ref(shard), sample_first,
                          C.c_void_p(d_fb_ptr), *_stream_sync(stream, sync))

    def render_lens_to_host(self, cam_open, cam_close=None, lens=None, shard=None, sample_first=0):
        """rt_render_lens through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam_open, shard, lambda d: self.render_lens(cam_open, d, cam_close=cam_close, lens=lens, shard=shard,
                                                                          sample_first=sample_first))

    def render_aov_lens(self, cam_open, ptrs, cam_close=None, lens=None, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_aov_lens.  ptrs as render_aov takes them.  Returns the rt_timing."""
        return self._call("rt_render_aov_lens", C.byref(cam_open), _ref(cam_close), _lens_struct(lens), _ref(shard), sample_first,
                          C.byref(_aov_struct(ptrs)), *_stream_sync(stream, sync))

    def render_aov_lens_to_host(self, cam_open, cam_close=None, lens=None, shard=None, sample_first=0):
        """rt_render_aov_lens through fresh device buffers: (the dict render_aov_to_host returns, rt_timing)."""
        return _aov_to_host(amd_lib().rt_shard_rows(cam_open.image_height, _ref(shard)), cam_open.image_width,
                            lambda ptrs: self.render_aov_lens(cam_open, ptrs, cam_close=cam_close, lens=lens, shard=shard, sample_first=sample_first))

    def lens_camera_rays(self, cam_open, cam_close, lens, ijs):
        """rt_lens_camera_rays (the module function lens_camera_rays: no scene involved, the current device)."""
        return lens_camera_rays(cam_open, cam_close, lens, ijs)

    def render_nee(self, cam, d_fb_ptr, params=None, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_nee: params None (defaults: mis = 1), a NeeParams or a dict of its fields.  Returns the rt_timing of this call."""
        return self._call("rt_render_nee", C.byref(cam), _nee_struct(params), _ref(shard), sample_first, C.c_void_p(d_fb_ptr),
                          *_stream_sync(stream, sync))

    def render_nee_to_host(self, cam, params=None, shard=None, sample_first=0):
        """rt_render_nee through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_nee(cam, d, params=params, shard=shard, sample_first=sample_first))

    def nee_light_table(self):
        """rt_nee_light_table: (sphere indices int32, cdf float32, pmf float32) of the handle's emitter table."""
        lib = amd_lib()
        n = C.c_int32()
        _check(lib.rt_nee_light_table(self._h, 0, None, None, None, C.byref(n)), "rt_nee_light_table")
        idx = np.zeros(n.value, dtype=np.int32)
        cdf = np.zeros(n.value, dtype=np.float32)
        pmf = np.zeros(n.value, dtype=np.float32)
        if n.value:
            _check(lib.rt_nee_light_table(self._h, n.value, idx.ctypes.data, cdf.ctypes.data, pmf.ctypes.data, C.byref(n)),
                   "rt_nee_light_table")
        return idx, cdf, pmf

    def nee_emitter_table(self, params=None):
        """rt_nee_emitter_table: (kind int32 — 0 sphere, 1 plane —, index int32, cdf float32, pmf float32, area float32) of the emitter
        table that params (None, a NeeParams or a dict) select."""
        lib = amd_lib()
        n = C.c_int32()
        p = _nee_struct(params)
        _check(lib.rt_nee_emitter_table(self._h, p, 0, None, None, None, None, None, C.byref(n)), "rt_nee_emitter_table")
        kind, idx = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        cdf, pmf, area = (np.zeros(n.value, dtype=np.float32) for _ in range(3))
        if n.value:
            _check(lib.rt_nee_emitter_table(self._h, p, n.value, kind.ctypes.data, idx.ctypes.data, cdf.ctypes.data, pmf.ctypes.data,
                                            area.ctypes.data, C.byref(n)), "rt_nee_emitter_table")
        return kind, idx, cdf, pmf, area

    def nee_light_tree(self, params=None):
        """rt_nee_light_tree: the light tree over the emitter table that params (None, a NeeParams or a dict) select, as a dict of columns
        — per node (preorder) sphere (n, 4) float32, weight, q float32, left, right, entry int32; per table entry path uint32, depth
        int32."""
        lib = amd_lib()
        nn, ne = C.c_int32(), C.c_int32()
        p = _nee_struct(params)
        _check(lib.rt_nee_light_tree(self._h, p, 0, 0, *([None] * 8), C.byref(nn), C.byref(ne)), "rt_nee_light_tree")
        t = {"sphere": np.zeros((nn.value, 4), np.float32), "weight": np.zeros(nn.value, np.float32), "q": np.zeros(nn.value, np.float32),
             "left": np.zeros(nn.value, np.int32), "right": np.zeros(nn.value, np.int32), "entry": np.zeros(nn.value, np.int32),
             "path": np.zeros(ne.value, np.uint32), "depth": np.zeros(ne.value, np.int32)}
        if nn.value:
            _check(lib.rt_nee_light_tree(self._h, p, nn.value, ne.value, *(t[k].ctypes.data for k in ("sphere", "weight", "q", "left", "right",
                                                                                                      "entry", "path", "depth")),
                                         C.byref(nn), C.byref(ne)), "rt_nee_light_tree")
        return t

    def trace_samples_nee(self, cam, ijs, params=None):
        """rt_trace_samples_nee: ijs (n, 3) → (radiance (n, 3), rays (n,), final seeds (n,), final light-sample seeds (n,))."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _SEED, _SEED)
        _check(amd_lib().rt_trace_samples_nee(self._h, C.byref(cam), _nee_struct(params), n, ijs.ctypes.data, *(a.ctypes.data for a in out)),
               "rt_trace_samples_nee")
        return out

    def render_env(self, cam, env, d_fb_ptr, params=None, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_env: env an Env; params None (defaults: MIS, scale 1, no rotation), an EnvParams or a dict of its fields.  Returns the
        rt_timing of this call."""
        return self._call("rt_render_env", C.byref(cam), env._h, _env_struct(params), _ref(shard), sample_first, C.c_void_p(d_fb_ptr),
                          *_stream_sync(stream, sync))

    def render_env_to_host(self, cam, env, params=None, shard=None, sample_first=0):
        """rt_render_env through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_env(cam, env, d, params=params, shard=shard, sample_first=sample_first))

    def trace_samples_env(self, cam, env, ijs, params=None):
        """rt_trace_samples_env: ijs (n, 3) → (radiance (n, 3), rays (n,), final seeds (n,), final light-sample seeds (n,))."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _SEED, _SEED)
        _check(amd_lib().rt_trace_samples_env(self._h, C.byref(cam), env._h, _env_struct(params), n, ijs.ctypes.data,
                                              *(a.ctypes.data for a in out)), "rt_trace_samples_env")
        return out

    def render_lit(self, cam, d_fb_ptr, *, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None,
                   stream=None, sync=True, sample_first=0):
        """rt_render_lit: emitters, environment and lens in one frame (lit_params()'s arguments).  Returns the rt_timing of this call."""
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        return self._call("rt_render_lit", C.byref(cam), C.byref(lit), _ref(shard), sample_first, C.c_void_p(d_fb_ptr), *_stream_sync(stream, sync))

    def render_lit_to_host(self, cam, *, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None,
                           sample_first=0):
        """rt_render_lit through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_lit(cam, d, cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params, shard=shard,
                                                                    sample_first=sample_first))

    def render_lit_split(self, cam, d_direct_ptr, d_indirect_ptr, *, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None,
                         shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_lit_split: rt_render_lit's frame as its direct and its indirect light, each 3 floats per pixel at an integer device
        address (render_lit's keywords).  Returns the rt_timing of this call."""
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        return self._call("rt_render_lit_split", C.byref(cam), C.byref(lit), _ref(shard), sample_first, C.c_void_p(d_direct_ptr), C.c_void_p(d_indirect_ptr),
                          *_stream_sync(stream, sync))

    def render_lit_split_to_host(self, cam, *, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None, sample_first=0):
        """rt_render_lit_split through fresh device buffers: (direct, indirect) (rows, width, 3) float32 sums each, and the rt_timing."""
        indirect = np.empty((amd_lib().rt_shard_rows(cam.image_height, _ref(shard)), cam.image_width, 3), dtype=np.float32)
        with _DeviceBuffers() as dev:
            d2 = dev.alloc(indirect.nbytes)
            direct, t = _frame_to_host(cam, shard, lambda d: self.render_lit_split(cam, d, d2, cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env,
                                                                                   env_params=env_params, shard=shard, sample_first=sample_first))
            dev.download(d2, indirect)
        return direct, indirect, t

    def trace_samples_lit_split(self, cam, ijs, *, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None):
        """rt_trace_samples_lit_split: ijs (n, 3) → (direct (n, 3), indirect (n, 3), rays (n,), final seeds (n,), final emitter-stream seeds
        (n,), final environment-stream seeds (n,))."""
        ijs, n, out = _probe(ijs, _RGB, _RGB, _COUNT, _SEED, _SEED, _SEED)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        _check(amd_lib().rt_trace_samples_lit_split(self._h, C.byref(cam), C.byref(lit), n, ijs.ctypes.data, *(a.ctypes.data for a in out)),
               "rt_trace_samples_lit_split")
        return out

    def render_lit_adaptive(self, cam, d_fb_ptr, d_spp_ptr, d_moments_ptr=None, *, cam_close=None, lens=None, emitters=True, nee=None, env=None,
                            env_params=None, shard=None, stream=None, sync=True, sample_first=0, prior=None, **params):
        """rt_render_lit_adaptive: rt_render_adaptive's rounds on rt_render_lit's estimator.  d_fb_ptr (3 floats per pixel), d_spp_ptr
        (1 int32 per pixel), d_moments_ptr (None, or 2 floats per pixel) are integer device addresses; the keywords are lit_params()'s
        arguments; params are rt_adaptive_params fields (min_spp, batch_spp, max_spp, threshold) and rule (0 or 1: given, the call goes
        through rt_render_lit_adaptive_rule with that rt_stop_params.rule); prior: None, or the device address of 2 floats per local
        pixel (rt_render_lit_adaptive_prior, rule 0 unless given).  Returns the rt_timing of this call."""
        rule = params.pop("rule", None)
        p = adaptive_params(**params)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        name, stop, after = _adaptive_entry("rt_render_lit_adaptive", rule, prior)
        return self._call(name, C.byref(cam), C.byref(lit), C.byref(p), *stop, _ref(shard), sample_first, C.c_void_p(d_fb_ptr), C.c_void_p(d_spp_ptr),
                          C.c_void_p(d_moments_ptr or 0), *_stream_sync(stream, sync), after=after)

    def render_lit_adaptive_to_host(self, cam, *, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None,
                                    sample_first=0, prior=None, **params):
        """rt_render_lit_adaptive through fresh device buffers: (fb (rows, w, 3) float32 sums, spp (rows, w) int32, moments (rows, w, 2)
        float32 (S1, S2)) and the rt_timing.  prior: None or a host array (rows, w, 2) float32 (ch, vh)."""
        return _adaptive_to_host(cam, shard, prior, lambda d_fb, d_spp, d_moments, d_prior: self.render_lit_adaptive(
            cam, d_fb, d_spp, d_moments, cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params, shard=shard,
            sample_first=sample_first, prior=d_prior, **params))

    def trace_samples_lit(self, cam, ijs, *, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None):
        """rt_trace_samples_lit: ijs (n, 3) → (radiance (n, 3), rays (n,), final seeds (n,), final emitter-stream seeds (n,), final
        environment-stream seeds (n,))."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _SEED, _SEED, _SEED)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        _check(amd_lib().rt_trace_samples_lit(self._h, C.byref(cam), C.byref(lit), n, ijs.ctypes.data, *(a.ctypes.data for a in out)),
               "rt_trace_samples_lit")
        return out

    def render_medium(self, cam, d_fb_ptr, *, medium=None, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None,
                      stream=None, sync=True, sample_first=0):
        """rt_render_medium: rt_render_lit under a homogeneous medium (medium: None, a MediumParams or a dict of medium_params()'s
        arguments; the other keywords are lit_params()'s).  Returns the rt_timing of this call."""
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        return self._call("rt_render_medium", C.byref(cam), C.byref(lit), _medium_struct(medium), _ref(shard), sample_first, C.c_void_p(d_fb_ptr),
                          *_stream_sync(stream, sync))

    def render_medium_to_host(self, cam, *, medium=None, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None,
                              sample_first=0):
        """rt_render_medium through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_medium(cam, d, medium=medium, cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params,
                                                                       shard=shard, sample_first=sample_first))

    def trace_samples_medium(self, cam, ijs, *, medium=None, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None):
        """rt_trace_samples_medium: ijs (n, 3) → (radiance (n, 3), rays (n,), medium events (n,), final seeds (n,), final emitter-stream
        seeds (n,), final environment-stream seeds (n,), final medium-stream seeds (n,))."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _COUNT, _SEED, _SEED, _SEED, _SEED)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        _check(amd_lib().rt_trace_samples_medium(self._h, C.byref(cam), C.byref(lit), _medium_struct(medium), n, ijs.ctypes.data,
                                                 *(a.ctypes.data for a in out)), "rt_trace_samples_medium")
        return out

    def render_volume(self, cam, d_fb_ptr, *, medium=None, volume=None, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None,
                      shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_volume: rt_render_medium with a density grid in the medium's box (volume: None or a Volume; the other keywords are
        render_medium's).  Returns the rt_timing of this call."""
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        return self._call("rt_render_volume", C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _ref(shard), sample_first,
                          C.c_void_p(d_fb_ptr), *_stream_sync(stream, sync))

    def render_volume_to_host(self, cam, *, medium=None, volume=None, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None,
                              shard=None, sample_first=0):
        """rt_render_volume through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_volume(cam, d, medium=medium, volume=volume, cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params,
                                                                       shard=shard, sample_first=sample_first))

    def render_volume_adaptive(self, cam, d_fb_ptr, d_spp_ptr, d_moments_ptr=None, *, medium=None, volume=None, cam_close=None, lens=None,
                               emitters=True, nee=None, env=None, env_params=None, shard=None, stream=None, sync=True, sample_first=0, prior=None,
                               **params):
        """rt_render_volume_adaptive: render_lit_adaptive's rounds on render_volume's estimator.  The device addresses are
        render_lit_adaptive's, medium and volume render_volume's; params are rt_adaptive_params fields and rule (None: a NULL
        rt_stop_params); prior: None, or the device address of 2 floats per local pixel.  Returns the rt_timing of this call."""
        rule = params.pop("rule", None)
        p = adaptive_params(**params)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        stop = None if rule is None else C.byref(stop_params(rule=rule))
        return self._call("rt_render_volume_adaptive", C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), C.byref(p), stop,
                          C.c_void_p(prior or 0), _ref(shard), sample_first, C.c_void_p(d_fb_ptr), C.c_void_p(d_spp_ptr),
                          C.c_void_p(d_moments_ptr or 0), *_stream_sync(stream, sync))

    def render_volume_adaptive_to_host(self, cam, *, medium=None, volume=None, cam_close=None, lens=None, emitters=True, nee=None, env=None,
                                       env_params=None, shard=None, sample_first=0, prior=None, **params):
        """rt_render_volume_adaptive through fresh device buffers: (fb (rows, w, 3) float32 sums, spp (rows, w) int32, moments (rows, w, 2)
        float32 (S1, S2)) and the rt_timing.  prior: None or a host array (rows, w, 2) float32 (ch, vh)."""
        return _adaptive_to_host(cam, shard, prior, lambda d_fb, d_spp, d_moments, d_prior: self.render_volume_adaptive(
            cam, d_fb, d_spp, d_moments, medium=medium, volume=volume, cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params,
            shard=shard, sample_first=sample_first, prior=d_prior, **params))

    def render_aov_volume(self, cam, ptrs, *, medium=None, volume=None, cam_close=None, lens=None, shard=None, stream=None, sync=True, sample_first=0,
                          transmittance=None):
        """rt_render_aov_volume: render_aov_lens's buffers under render_volume's medium and volume.  ptrs as render_aov takes them;
        transmittance: None, or the device address of 1 float per pixel.  Returns the rt_timing."""
        lit = lit_params(cam_close=cam_close, lens=lens)
        return self._call("rt_render_aov_volume", C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _ref(shard), sample_first,
                          C.byref(_aov_struct(ptrs)), C.c_void_p(transmittance or 0), *_stream_sync(stream, sync))

    def render_aov_volume_to_host(self, cam, *, medium=None, volume=None, cam_close=None, lens=None, shard=None, sample_first=0):
        """rt_render_aov_volume through fresh device buffers: (render_aov_lens_to_host's dict plus "transmittance": (rows, w) float32,
        rt_timing)."""
        rows, w = amd_lib().rt_shard_rows(cam.image_height, _ref(shard)), cam.image_width
        with _DeviceBuffers() as dev:
            d_tr = dev.alloc(max(rows, 0) * max(w, 0) * 4)
            out, t = _aov_to_host(rows, w, lambda ptrs: self.render_aov_volume(cam, ptrs, medium=medium, volume=volume, cam_close=cam_close, lens=lens,
                                                                               shard=shard, sample_first=sample_first, transmittance=d_tr))
            out["transmittance"] = dev.download(d_tr, np.empty((rows, w), dtype=np.float32))
        return out, t

    def trace_samples_volume(self, cam, ijs, *, medium=None, volume=None, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None):
        """rt_trace_samples_volume: trace_samples_medium's seven columns and the grid cells visited per sample (n,)."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _COUNT, _SEED, _SEED, _SEED, _SEED, _COUNT)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        _check(amd_lib().rt_trace_samples_volume(self._h, C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), n,
                                                 ijs.ctypes.data, *(a.ctypes.data for a in out)), "rt_trace_samples_volume")
        return out

    def render_chroma(self, cam, d_fb_ptr, *, medium=None, volume=None, tint=None, cam_close=None, lens=None, emitters=True, nee=None, env=None,
                      env_params=None, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_chroma: rt_render_volume with an extinction per colour channel, sigma_t * tint[k] (tint: None, one number or three, a
        dict of chroma_params' keywords or a ChromaParams; the other keywords are render_volume's).  Returns the rt_timing of this call."""
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        return self._call("rt_render_chroma", C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _chroma_struct(tint), _ref(shard),
                          sample_first, C.c_void_p(d_fb_ptr), *_stream_sync(stream, sync))

    def render_chroma_to_host(self, cam, *, medium=None, volume=None, tint=None, cam_close=None, lens=None, emitters=True, nee=None, env=None,
                              env_params=None, shard=None, sample_first=0):
        """rt_render_chroma through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_chroma(cam, d, medium=medium, volume=volume, tint=tint, cam_close=cam_close, lens=lens,
                                                                       emitters=emitters, nee=nee, env=env, env_params=env_params, shard=shard,
                                                                       sample_first=sample_first))

    def trace_samples_chroma(self, cam, ijs, *, medium=None, volume=None, tint=None, cam_close=None, lens=None, emitters=True, nee=None, env=None,
                             env_params=None):
        """rt_trace_samples_chroma: trace_samples_volume's eight columns under the tint."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _COUNT, _SEED, _SEED, _SEED, _SEED, _COUNT)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        _check(amd_lib().rt_trace_samples_chroma(self._h, C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _chroma_struct(tint), n,
                                                 ijs.ctypes.data, *(a.ctypes.data for a in out)), "rt_trace_samples_chroma")
        return out

    def render_glow(self, cam, d_fb_ptr, *, medium=None, volume=None, glow=None, heat=None, cam_close=None, lens=None, emitters=True, nee=None,
                    env=None, env_params=None, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_glow: rt_render_volume with a medium that emits (glow: None, the radiance as one number or three, a dict of
        glow_params' keywords or a GlowParams; heat: a Volume of the volume's dimensions, source 2 only; the other keywords are
        render_volume's).  Returns the rt_timing of this call."""
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        return self._call("rt_render_glow", C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _glow_struct(glow), _volume_handle(heat),
                          _ref(shard), sample_first, C.c_void_p(d_fb_ptr), *_stream_sync(stream, sync))

    def render_glow_to_host(self, cam, *, medium=None, volume=None, glow=None, heat=None, cam_close=None, lens=None, emitters=True, nee=None, env=None,
                            env_params=None, shard=None, sample_first=0):
        """rt_render_glow through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_glow(cam, d, medium=medium, volume=volume, glow=glow, heat=heat, cam_close=cam_close, lens=lens,
                                                                     emitters=emitters, nee=nee, env=env, env_params=env_params, shard=shard,
                                                                     sample_first=sample_first))

    def trace_samples_glow(self, cam, ijs, *, medium=None, volume=None, glow=None, heat=None, cam_close=None, lens=None, emitters=True, nee=None, env=None,
                           env_params=None):
        """rt_trace_samples_glow: trace_samples_volume's eight columns and glow_length (float32) under the glow."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _COUNT, _SEED, _SEED, _SEED, _SEED, _COUNT, (np.float32, ()))
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        _check(amd_lib().rt_trace_samples_glow(self._h, C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _glow_struct(glow),
                                               _volume_handle(heat), n, ijs.ctypes.data, *(a.ctypes.data for a in out)), "rt_trace_samples_glow")
        return out

    def render_glow_sampled(self, cam, d_fb_ptr, *, medium=None, volume=None, glow=None, heat=None, sample=None, sampler=None, cam_close=None, lens=None,
                            emitters=True, nee=None, env=None, env_params=None, shard=None, stream=None, sync=True, sample_first=0):
        """rt_render_glow_sampled: rt_render_glow with light samples of the glow (sample: None, "mis", "light", a dict of
        glow_sample_params' keywords or a GlowSampleParams; sampler: the GlowSampler of the call's grids and source; the other keywords
        are render_glow's).  Returns the rt_timing of this call."""
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        return self._call("rt_render_glow_sampled", C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _glow_struct(glow),
                          _volume_handle(heat), _glow_sample_struct(sample), _sampler_handle(sampler), _ref(shard), sample_first, C.c_void_p(d_fb_ptr),
                          *_stream_sync(stream, sync))

    def render_glow_sampled_to_host(self, cam, *, medium=None, volume=None, glow=None, heat=None, sample=None, sampler=None, cam_close=None, lens=None,
                                    emitters=True, nee=None, env=None, env_params=None, shard=None, sample_first=0):
        """rt_render_glow_sampled through a fresh device buffer: (rows, width, 3) float32 sums and the rt_timing."""
        return _frame_to_host(cam, shard, lambda d: self.render_glow_sampled(cam, d, medium=medium, volume=volume, glow=glow, heat=heat, sample=sample,
                                                                             sampler=sampler, cam_close=cam_close, lens=lens, emitters=emitters, nee=nee,
                                                                             env=env, env_params=env_params, shard=shard, sample_first=sample_first))

    def trace_samples_glow_sampled(self, cam, ijs, *, medium=None, volume=None, glow=None, heat=None, sample=None, sampler=None, cam_close=None, lens=None,
                                   emitters=True, nee=None, env=None, env_params=None):
        """rt_trace_samples_glow_sampled: trace_samples_glow's nine columns and glow_samples, the glow shadow rays per sample (n,)."""
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _COUNT, _SEED, _SEED, _SEED, _SEED, _COUNT, (np.float32, ()), _COUNT)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        _check(amd_lib().rt_trace_samples_glow_sampled(self._h, C.byref(cam), C.byref(lit), _medium_struct(medium), _volume_handle(volume), _glow_struct(glow),
                                                       _volume_handle(heat), _glow_sample_struct(sample), _sampler_handle(sampler), n, ijs.ctypes.data,
                                                       *(a.ctypes.data for a in out)), "rt_trace_samples_glow_sampled")
        return out

    def render_fog_adaptive(self, cam, d_fb_ptr, d_spp_ptr, d_moments_ptr=None, *, medium=None, volume=None, tint=None, glow=None, heat=None,
                            sample=None, sampler=None, cam_close=None, lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None,
                            stream=None, sync=True, sample_first=0, prior=None, **params):
        """rt_render_fog_adaptive: render_volume_adaptive's rounds on the estimator of the fog call the keywords name — tint as
        render_chroma takes it, glow and heat as render_glow, sample and sampler as render_glow_sampled; a tint goes with neither a glow
        nor a sample.  The other keywords and the device addresses are render_volume_adaptive's.  Returns the rt_timing of this call."""
        rule = params.pop("rule", None)
        p = adaptive_params(**params)
        lit = lit_params(cam_close=cam_close, lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params)
        fog = fog_params(medium=medium, volume=volume, tint=tint, glow=glow, heat=heat, sample=sample, sampler=sampler)
        stop = None if rule is None else C.byref(stop_params(rule=rule))
        return self._call("rt_render_fog_adaptive", C.byref(cam), C.byref(lit), C.byref(fog), C.byref(p), stop, C.c_void_p(prior or 0), _ref(shard),
                          sample_first, C.c_void_p(d_fb_ptr), C.c_void_p(d_spp_ptr), C.c_void_p(d_moments_ptr or 0), *_stream_sync(stream, sync))

    def render_fog_adaptive_to_host(self, cam, *, medium=None, volume=None, tint=None, glow=None, heat=None, sample=None, sampler=None, cam_close=None,
                                    lens=None, emitters=True, nee=None, env=None, env_params=None, shard=None, sample_first=0, prior=None, **params):
        """rt_render_fog_adaptive through fresh device buffers: render_volume_adaptive_to_host's (fb, spp, moments, rt_timing)."""
        return _adaptive_to_host(cam, shard, prior, lambda d_fb, d_spp, d_moments, d_prior: self.render_fog_adaptive(
            cam, d_fb, d_spp, d_moments, medium=medium, volume=volume, tint=tint, glow=glow, heat=heat, sample=sample, sampler=sampler, cam_close=cam_close,
            lens=lens, emitters=emitters, nee=nee, env=env, env_params=env_params, shard=shard, sample_first=sample_first, prior=d_prior, **params))

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(amd_lib().rt_last_kernel_ms(self._h, C.byref(ms)), "rt_last_kernel_ms")
        return ms.value

    def last_timing(self):
        """Full rt_timing of the most recent rt_render of this scene (waits for it)."""
        t = Timing()
        _check(amd_lib().rt_last_timing(self._h, C.byref(t)), "rt_last_timing")
        return t

    def trace_kernel_name(self):
        """Name (as rocprofv3 prints it) of the dominant kernel of the most recent rt_render."""
        t = self.last_timing()
        lds = "true" if t.scene_in_lds else "false"
        # the sphere-only octant kernel behind the primary pass: render_kernel<true, false, false, false, true, true> is its build for
        # scenes without emitters (rt_timing.dark_kernel); with emitters, or rt_config.dark_kernel = -1, render_emit_kernel ran
        # (an older library loaded through RTP_AMD_LIB for an A/B run writes a shorter rt_timing and has the one kernel of that name)
        knows_dark = t.struct_bytes >= Timing.dark_kernel.offset + 4
        if knows_dark and t.guarded and t.scene_in_lds and t.sphere_only and t.primary_visibility and not t.guard_dynamic and not t.dark_kernel:
            return "rtk::render_emit_kernel(rtk::KParams)"
        return (f"void rtk::render_kernel<{lds}, {'false' if t.guarded else 'true'}, {'true' if t.guard_dynamic else 'false'}, "
                f"{'true' if t.wide_nodes else 'false'}, {'true' if t.sphere_only else 'false'}, "
                f"{'true' if t.primary_visibility else 'false'}>(rtk::KParams)")

    def trace_samples(self, cam, ijs):
        ijs, n, out = _probe(ijs, _RGB, _COUNT, _SEED)
        _check(amd_lib().rt_trace_samples(self._h, C.byref(cam), n, ijs.ctypes.data, *(a.ctypes.data for a in out)), "rt_trace_samples")
        return out

    def guard_reason(self):
        """'' when rt_render may use the guarded near-first walk, else why not."""
        return amd_lib().rt_scene_guard_reason(self._h).decode()

    def closest_hits(self, origins, directions):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        hit = np.zeros(n, dtype=np.int32)
        t = np.zeros(n, dtype=np.float32)
        prim = np.zeros(n, dtype=np.int32)
        _check(amd_lib().rt_closest_hits(self._h, n, o.ctypes.data, d.ctypes.data, hit.ctypes.data, t.ctypes.data,
                                         prim.ctypes.data), "rt_closest_hits")
        return hit, t, prim

    def close(self):
        if self._h:
            amd_lib().rt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """rt_context: one frame sharded over the GPUs of the node through the C ABI (rt_render_sharded + rt_gather)."""

    def __init__(self, num_devices=0, ordinals=None):
        self._h = C.c_void_p()
        arr = (C.c_int32 * len(ordinals))(*ordinals) if ordinals else None
        _check(amd_lib().rt_context_create(num_devices, arr, C.byref(self._h)), "rt_context_create")
        self._keep = None

    @property
    def num_devices(self):
        return amd_lib().rt_context_num_devices(self._h)

    @property
    def transport(self):
        return amd_lib().rt_context_transport(self._h).decode()

    def scene(self, host_scene, **config):
        cfg = new_config()
        for k, v in config.items():
            setattr(cfg, k, v)
        _check(amd_lib().rt_context_scene_create(self._h, C.byref(host_scene.desc), C.byref(cfg)), "rt_context_scene_create")
        self._keep = host_scene

    def render(self, cam, d_fb_ptr, band_rows=8):
        """d_fb_ptr: device address on the root device of image_height*image_width*3 floats.  Returns the per-device timings."""
        t = (Timing * self.num_devices)()
        for k in range(self.num_devices):
            t[k].struct_bytes = C.sizeof(Timing)
        _check(amd_lib().rt_render_sharded(self._h, C.byref(cam), band_rows, C.c_void_p(d_fb_ptr), t), "rt_render_sharded")
        return list(t)

    def close(self):
        if self._h:
            amd_lib().rt_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
