"""rt_render_volume / rt_trace_samples_volume (include/rtp_amd.h, "density grid"): heterogeneous fog from a density grid in
rt_render_medium's box.  The contract's restatement is tests/cpu_native/volume_ref.c (tests/volume_reference.py); the CPU tests check the
restatement and the ABI, the GPU tests the kernels against the restatement, bit for bit.  Scenes, settings and protocols are
tests/test_medium.py's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import medium_reference as mr
import rtp_bindings as rb
import volume_reference as vr
from test_lit import assert_same
from test_medium import (ABSORB_N, BACKGROUND, EQUAL_SPP, FOG_BOX, PROBE_VIEW, SETTINGS, _channel_z, _fog_ball_scene, all_ijs, dev_kw, media, rb_wang,
                         ref_kw, scenes, sun_map)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
INVALID = 1
BOX = (-4.0, -0.5, -4.0, 4.0, 3.5, 4.0)          # test_medium.py's box around the three scenes


def random_grid(shape, seed, empty=1 / 3):
    """(nz, ny, nx) densities in [0.1, 2), a share `empty` of the cells exactly 0."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.1, 2.0, shape).astype(np.float32)
    g[rng.random(shape) < empty] = 0.0
    return g


# the grids of the issue, as (nz, ny, nx) arrays: 1^3, 2 x 3 x 5, 16^3 and 1 x 1 x 64 (nx x ny x nz), zeros among the cells of the last three
GRIDS = {"1": np.full((1, 1, 1), 1.25, np.float32), "2x3x5": random_grid((5, 3, 2), 11), "16": random_grid((16, 16, 16), 12),
         "1x1x64": random_grid((64, 1, 1), 13)}


# ---- no GPU needed ---------------------------------------------------------------------------------------------------------------------

def test_abi_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_volume_create", "rt_volume_destroy", "rt_render_volume", "rt_trace_samples_volume"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert len(lib.rt_render_volume.argtypes) == 11 and len(lib.rt_trace_samples_volume.argtypes) == 15
    for name in ("render_volume", "render_volume_to_host", "trace_samples_volume"):
        assert hasattr(rb.DeviceScene, name)
    assert hasattr(rb.Volume, "__enter__") and hasattr(rb.Volume, "close")
    header = open(os.path.join(ROOT, "include", "rtp_amd.h")).read()
    assert "#define RT_VOLUME_MAX_N 256" in header
    assert lib.rt_volume_destroy(None) == 0


def test_volume_create_refusals():
    """Null pointers, a dimension below 1 or above RT_VOLUME_MAX_N, a density that is negative, NaN or infinite: refused before the device
    is looked at."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    h = C.c_void_p()
    ok = np.ones(8, np.float32)

    def refused(word, density, nx, ny, nz, out=h):
        st = lib.rt_volume_create(density.ctypes.data if density is not None else None, nx, ny, nz, C.byref(out) if out is not None else None)
        msg = lib.rt_get_last_error_string().decode()
        assert st == INVALID and word in msg and "rt_volume_create" in msg, (word, st, msg)
    refused("null", None, 2, 2, 2)
    refused("null", ok, 2, 2, 2, out=None)
    for dims in ((0, 1, 1), (1, 0, 1), (1, 1, -1), (257, 1, 1), (1, 257, 1), (1, 1, 257)):
        refused("dimension", np.ones(257, np.float32), *dims)
    for bad in (-0.5, float("nan"), float("inf")):
        d = ok.copy()
        d[5] = bad
        refused("density", d, 2, 2, 2)
    with pytest.raises(rb.RtError):
        rb.Volume(np.ones((1, 1, 257), np.float32))
    with pytest.raises(rb.RtError):
        rb.Volume(np.ones((2, 2), np.float32))


def _calls(cam, lit, medium, volume):
    """(status, message) of rt_render_volume and of rt_trace_samples_volume with a null scene."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    pl = C.byref(lit) if lit is not None else None
    pm = C.byref(medium) if medium is not None else None
    out = [lib.rt_render_volume(None, C.byref(cam), pl, pm, volume, None, 0, C.c_void_p(1 << 32), None, 1, None), lib.rt_get_last_error_string().decode()]
    out += [lib.rt_trace_samples_volume(None, C.byref(cam), pl, pm, volume, 1, ijs, f, r, r, s, s, s, s, r), lib.rt_get_last_error_string().decode()]
    return out


def test_refusals_before_the_scene_is_looked_at():
    """rt_render_medium's refusals in its order, then the volume's (a volume needs a medium with region 2), all with a null scene — nothing
    can have been enqueued, and the volume's handle is never read (it is not one).  What passes reaches the null-scene check."""
    cam = rb.rtiow_camera(8, 4, 2)
    handle = C.c_void_p(1 << 32)
    nan, inf = float("nan"), float("inf")

    def refused(word, medium, lit=None, volume=handle):
        st1, m1, st2, m2 = _calls(cam, lit, medium, volume)
        assert st1 == INVALID and word in m1, (word, m1)
        assert st2 == INVALID and word in m2 and "rt_trace_samples_volume" in m2, (word, m2)
        if volume is not None:
            assert "rt_render_volume" in m1, m1
    box = dict(box=(0, 0, 0, 1, 1, 1))
    for volume in (handle, None):
        short = rb.medium_params(sigma_t=1.0, **box)
        short.struct_bytes = 4
        refused("struct_bytes", short, volume=volume)
        for s in (-0.5, nan, inf):
            refused("sigma_t", rb.medium_params(sigma_t=s, **box), volume=volume)
        refused("albedo", rb.medium_params(sigma_t=1.0, albedo=(0.5, 1.5, 0.5), **box), volume=volume)
        refused("|g|", rb.medium_params(sigma_t=1.0, g=0.96, **box), volume=volume)
        refused("lo < hi", rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, -1, 1)), volume=volume)
        # rt_render_lit's come first, the medium's before the volume's
        refused("mis", rb.medium_params(sigma_t=-1.0), lit=rb.lit_params(nee=dict(mis=2)), volume=volume)
    refused("sigma_t", rb.medium_params(sigma_t=-1.0))
    # the volume's own: region 2 or nothing
    refused("region 2", None)
    refused("region 2", rb.medium_params(sigma_t=1.0))
    refused("region 2", rb.medium_params(sigma_t=0.0))
    refused("region 2", rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)))
    # what passes reaches the scene
    for m, volume in ((rb.medium_params(sigma_t=1.0, **box), handle), (rb.medium_params(sigma_t=0.0, **box), handle), (None, None),
                      (rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), None)):
        st1, m1, st2, m2 = _calls(cam, None, m, volume)
        assert st1 == INVALID and "null scene" in m1, m1
        assert st2 == INVALID and "region" not in m2 and "sigma_t" not in m2, m2


def _grid_file(path, dims, data, magic=b"VOL1\n"):
    with open(path, "wb") as f:
        f.write(magic + ("%d %d %d\n" % dims).encode() + np.asarray(data, "<f4").tobytes())
    return str(path)


def test_cli_refusals(test_config_text, tmp_path):
    good = _grid_file(tmp_path / "good.vol", (2, 3, 1), np.ones(6))
    fog = ["--lit", "--fog", "0.5"]
    box = ["--fog-box", "0,0,0,1,1,1"]
    cases = [(fog + ["--fog-grid", good], "--fog-box"), (["--lit", "--fog-grid", good], "need"),
             (fog + ["--fog-ball", "0,0,0,1", "--fog-grid", good], "--fog-ball"),
             (fog + box + ["--fog-grid", good, "--noise-target", "0.1"], "--noise-target"),
             (fog + box + ["--fog-grid"], "FILE"), (fog + box + ["--fog-grid", str(tmp_path / "missing.vol")], "FILE"),
             (fog + box + ["--fog-grid", _grid_file(tmp_path / "short.vol", (2, 3, 1), np.ones(5))], "FILE"),
             (fog + box + ["--fog-grid", _grid_file(tmp_path / "long.vol", (2, 3, 1), np.ones(7))], "FILE"),
             (fog + box + ["--fog-grid", _grid_file(tmp_path / "magic.vol", (2, 3, 1), np.ones(6), magic=b"VOL2\n")], "FILE"),
             (fog + box + ["--fog-grid", _grid_file(tmp_path / "zero.vol", (0, 3, 1), np.ones(6))], "FILE"),
             (fog + box + ["--fog-grid", _grid_file(tmp_path / "wide.vol", (257, 1, 1), np.ones(257))], "FILE"),
             (fog + box + ["--fog-grid", _grid_file(tmp_path / "neg.vol", (2, 3, 1), [1, 1, -1, 1, 1, 1])], "FILE"),
             (fog + box + ["--fog-grid", _grid_file(tmp_path / "nan.vol", (2, 3, 1), [1, 1, np.nan, 1, 1, 1])], "FILE")]
    with open(tmp_path / "header.vol", "wb") as f:
        f.write(b"VOL1\n2 3\n" + np.ones(6, "<f4").tobytes())
    cases.append((fog + box + ["--fog-grid", str(tmp_path / "header.vol")], "FILE"))
    for extra, word in cases:
        res = subprocess.run([EXE, "--gpu"] + extra, input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert res.returncode == 99 and word in res.stderr, (extra, res.returncode, res.stderr[-300:])


IDENTITY_VIEW = (12, 8, 2)


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_one_cell_of_density_one_is_the_homogeneous_box(scene):
    """A 1 x 1 x 1 grid of density 1.0 equals medium_reference with the same box: every probe column and whole frames, bit for bit, in every
    setting of tests/test_medium.py."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    ijs = all_ijs(w, h, spp)
    one = np.ones((1, 1, 1), np.float32)
    seen_events = seen_cells = 0
    for k, setting in enumerate(SETTINGS):
        medium = dict(sigma_t=0.25, albedo=(0.9, 0.85, 0.8), g=(-0.5, 0.0, 0.7)[k % 3], box=BOX)
        cam = camera(w, h, spp, 12)
        kw = ref_kw(scene, setting, w, h, spp, 12)
        want = mr.trace(host, cam, ijs, medium=medium, **kw)
        got = vr.trace(host, cam, ijs, medium=medium, density=one, **kw)
        for a, b, col in zip(got[:5], want, ("radiance", "rays", "events", "ends", "seeds")):
            assert_same(a, b, f"{scene} / {setting}: {col}")
        seen_events += int(got[2].sum())
        seen_cells += int(got[5].sum())
        assert_same(vr.frame(host, cam, medium=medium, density=one, **kw), mr.frame(host, cam, medium=medium, **kw), f"{scene} / {setting}: frame")
        # no grid at all is medium_reference's own path
        none = vr.trace(host, cam, ijs, medium=medium, density=None, **kw)
        assert_same(none[0], want[0], f"{scene} / {setting}: no grid")
        assert not none[5].any()
    assert seen_events > 100 and seen_cells > seen_events


def _advance(state, draws):
    for _ in range(int(draws)):
        state = rb_wang(state)
    return state


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_zero_density_grid_is_rt_render_lit(scene):
    """A grid of zeros: radiance, rays and the path, nee and env seeds are rt_render_lit's restatement's, no event, and med has advanced
    exactly one draw per non-empty path interval — counted on a 1^3 grid without light samples, where every such interval visits one cell
    and nothing else visits any."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    ijs = all_ijs(w, h, spp)
    init = [rb_wang(rb_wang(rb_wang(int(i) * w + int(j)) + int(s)) ^ 0x4D454431) for i, j, s in ijs]
    medium = dict(sigma_t=0.8, albedo=0.9, g=0.3, box=BOX)
    for setting in SETTINGS:
        cam = camera(w, h, spp, 12)
        kw = ref_kw(scene, setting, w, h, spp, 12)
        want = mr.trace(host, cam, ijs, medium=None, **kw)
        rad, rays, events, ends, seeds, cells = vr.trace(host, cam, ijs, medium=medium, density=np.zeros((5, 3, 2), np.float32), **kw)
        what = f"{scene} / {setting}"
        assert_same(rad, want[0], what + ": radiance")
        assert_same(rays, want[1], what + ": rays")
        for k in range(3):
            assert_same(seeds[:, k], want[4][:, k], what + f": seed {k}")
        assert not events.any() and cells.sum() > 0
    cam = camera(w, h, spp, 12)
    rad, rays, events, ends, seeds, cells = vr.trace(host, cam, ijs, medium=medium, density=np.zeros((1, 1, 1), np.float32), emitters=False)
    assert cells.max() >= 2 and not events.any()
    assert_same(seeds[:, 3], np.array([_advance(s, c) for s, c in zip(init, cells)], np.uint32), "med: one draw per non-empty path interval")


# ---- the walk alone ---------------------------------------------------------------------------------------------------------------------
# Boxes whose cell widths are exact in float32 (and so in float64): "along a cell plane" and "at a grid vertex" then mean the same thing in
# both statements.  (nx, ny, nz), lo, hi
WALK_GRIDS = {"1": ((1, 1, 1), (-1.0, -0.5, -2.0), (1.0, 1.5, 1.0)), "2x3x5": ((2, 3, 5), (-1.0, -0.5, -0.75), (1.0, 1.0, 0.5)),
              "16": ((16, 16, 16), (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)), "1x1x64": ((1, 1, 64), (-0.5, -0.5, -2.0), (0.5, 0.5, 2.0))}
WALK_SIGMA = 0.7
# The largest error of the float32 walk's optical depth against the float64 statement of the same walk over walk_cases(), relative to
# tau_max = sigma_t * max(rho) * |hi - lo| (the largest optical depth a ray through the box can have; a ratio to acc itself has no bound at
# grazing rays, where acc -> 0 and the two statements may disagree about an interval of rounding size).  Measured with this file's cases
# (the figure test_optical_depth_against_float64 prints); the bound is 4 x it — rounding depends on the segment count, not on the seed
WALK_MEASURED = 3.402e-07
WALK_TOL = 4 * WALK_MEASURED


# walk_rays' classes in the order it emits them: (name, rays)
WALK_CLASSES = (("outside, aimed inside", 400), ("inside, any direction", 200), ("one d_k == 0, inside", 60), ("one d_k == 0, outside", 60),
                ("two d_k == 0, inside", 60), ("two d_k == 0, outside", 60), ("at a grid vertex, from outside", 150), ("at a grid vertex, from inside", 50),
                ("from a vertex down an exact diagonal", 60), ("along a cell plane or edge, inside", 120), ("along a cell plane, from outside", 60))


def walk_rays(n, lo, hi, rng, centre=0.0, scale=1.0):
    """walk_cases' rays for any box (lo, hi) and dimensions n = (nx, ny, nz), drawn from rng: (o, d, t_end, kind), kind the index of each
    ray's class in WALK_CLASSES.  The origins "outside" lie on spheres of radius 3.5 … 6 times `scale` about `centre` (0 and 1 for the
    boxes of WALK_GRIDS, which they were written for)."""
    n, lo, hi = np.array(n), np.array(lo), np.array(hi)
    w = (hi - lo) / n
    inside = lambda k: (lo + rng.random((k, 3)) * (hi - lo)).astype(np.float32)
    vertex = lambda k: (lo + np.stack([rng.integers(0, n[a] + 1, k) for a in range(3)], 1) * w).astype(np.float32)

    def sphere(k):
        v = rng.normal(size=(k, 3))
        return (centre + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(3.5, 6.0, (k, 1)) * scale).astype(np.float32)
    o, d = [], []
    a = sphere(400)                                     # outside, aimed at points inside
    o.append(a)
    d.append(inside(400) - a)
    o.append(inside(200))                               # inside, any direction
    d.append(rng.normal(size=(200, 3)).astype(np.float32))
    for zeros in (1, 2):                                # d_k == 0, origins inside and outside
        for origin in (inside(60), (centre + (sphere(60) - np.float32(centre)) * np.float32(0.5)).astype(np.float32)):
            dd = rng.normal(size=(60, 3)).astype(np.float32)
            for r in range(60):
                dd[r, rng.choice(3, zeros, replace=False)] = 0.0
            o.append(origin)
            d.append(dd)
    a = sphere(150)                                     # aimed exactly at grid vertices (o + 1 * d is the vertex up to one rounding)
    o.append(a)
    d.append(vertex(150) - a)
    a = inside(50)
    o.append(a)
    d.append(vertex(50) - a)
    o.append(vertex(60))                                # from a vertex along an exact diagonal of the cells: through vertex after vertex
    d.append((rng.choice([-1.0, 1.0], (60, 3)) * w).astype(np.float32))
    a = inside(120)                                     # along cell planes: o_k on a plane (the box's faces included), d_k == 0
    dd = rng.normal(size=(120, 3)).astype(np.float32)
    v = vertex(120)
    for r in range(120):
        k = rng.integers(0, 3)
        a[r, k] = v[r, k]
        dd[r, k] = 0.0
        if r % 3 == 0:                                  # … and in two axes at once: along a cell edge
            k2 = (k + 1) % 3
            a[r, k2] = v[r, k2]
            dd[r, k2] = 0.0
    o.append(a)
    d.append(dd)
    a = sphere(60)                                      # along a plane from outside
    v = vertex(60)
    t = inside(60)
    for r in range(60):
        k = rng.integers(0, 3)
        a[r, k] = t[r, k] = v[r, k]
    o.append(a)
    d.append(t - a)
    assert [len(x) for x in o] == [k for _, k in WALK_CLASSES]
    kind = np.repeat(np.arange(len(WALK_CLASSES)), [k for _, k in WALK_CLASSES])
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)
    t_end = np.where(np.arange(o.shape[0]) % 2 == 0, np.float32(np.inf), rng.uniform(0.3, 1.5, o.shape[0]).astype(np.float32)).astype(np.float32)
    return o, d, t_end, kind


@functools.lru_cache(maxsize=None)
def walk_cases(name):
    """Rays (o, d, t_end) through WALK_GRIDS[name] with a random grid (a third of the cells empty): origins outside aimed into the box,
    origins inside, rays with one or two d_k == 0 (origins inside and outside), rays aimed exactly at grid vertices and leaving them along
    exact diagonals, rays along cell planes (the box's faces among them); t_end infinite for half of each kind and finite for the rest.
    The rays are walk_rays'; test_walk_cases_are_what_they_were pins the arrays' bytes."""
    n, lo, hi = WALK_GRIDS[name]
    n, lo, hi = np.array(n), np.array(lo), np.array(hi)
    rng = np.random.default_rng(sum(map(ord, name)))
    density = random_grid((n[2], n[1], n[0]), 100 + int(n.sum()))
    density.flat[0] = 1.5                               # (the 1^3 grid's only cell is not an empty one)
    o, d, t_end, _ = walk_rays(n, lo, hi, rng)
    medium = dict(sigma_t=WALK_SIGMA, box=tuple(lo) + tuple(hi))
    tau_max = WALK_SIGMA * float(density.max()) * float(np.linalg.norm(hi - lo))
    return medium, density, o, d, t_end, tau_max, float(np.linalg.norm(hi - lo))


# sha256 over the bytes of walk_cases(name)'s density, o, d and t_end, taken before walk_rays was split off it
WALK_CASES_SHA256 = {"1": "afdfb1e64b566c0157deea5b6ac04d4fe32a4e235e919c5404945e1962649e04",
                     "2x3x5": "86956aecb424f34aad121055b90b29321776441c5c752e44758d98f66fcf2667",
                     "16": "b06774428d9b01a6b8f673e55453a0cfd2637d361ba41ce25c816f5d9d2f65d9",
                     "1x1x64": "ee58d5eaf8854794b1ec8b77e6dc4168dcbdb1c1e98f1ec842cce4c03aa0eb54"}


def test_walk_cases_are_what_they_were():
    """walk_rays generalises walk_cases' generator to any box and dimensions; walk_cases itself returns the arrays it always returned."""
    import hashlib
    for name, want in WALK_CASES_SHA256.items():
        medium, density, o, d, t_end, tau_max, diag = walk_cases(name)
        assert o.shape == (1280, 3) and o.dtype == d.dtype == t_end.dtype == density.dtype == np.float32
        assert hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (density, o, d, t_end))).hexdigest() == want, name


def _walk_errors(name):
    medium, density, o, d, t_end, tau_max, diag = walk_cases(name)
    got = vr.walks(medium, density, o, d, t_end)
    hit64, acc64, len64 = vr.walks_f64(medium, density, o, d, t_end)
    return got, np.abs(got["acc"].astype(np.float64) - acc64) / tau_max, np.abs(got["seg_sum"] - got["length"]) / diag, acc64


def test_optical_depth_against_float64():
    """acc of the float32 walk against the float64 statement of the same walk, every case of walk_cases() on the four grids, none left out."""
    worst = 0.0
    for name in WALK_GRIDS:
        got, err, _, acc64 = _walk_errors(name)
        print(f"grid {name}: {len(err)} rays, {int(got['hit'].sum())} cross, {int((acc64 > 0).sum())} with acc > 0, max relative error {err.max():.3e}")
        assert got["hit"].sum() > 400 and (acc64 > 0).sum() > 300
        worst = max(worst, float(err.max()))
    print(f"largest relative error {worst:.3e}, measured {WALK_MEASURED}, bound {WALK_TOL}")
    assert worst <= WALK_TOL, worst


def test_walk_terminates_and_keeps_its_books():
    """cells <= nx + ny + nz per ray, no segment is negative, and the segments sum to (t1 - t0) * len (relative to the box's diagonal, the
    same bound); a ray that misses visits nothing."""
    for name, (n, lo, hi) in WALK_GRIDS.items():
        got, _, seg_err, _ = _walk_errors(name)
        crossed = got["hit"] == 1
        assert (got["cells"] <= sum(n)).all() and (got["cells"][crossed] >= 1).all() and not got["cells"][~crossed].any(), name
        assert (got["seg_min"][crossed] >= 0.0).all(), name
        print(f"grid {name}: most cells {int(got['cells'].max())} of {sum(n)}, segment sums within {seg_err[crossed].max():.3e}")
        assert seg_err[crossed].max() <= WALK_TOL, (name, seg_err[crossed].max())


def test_refined_grid_has_the_same_optical_depth():
    """A grid and its 2 x nearest-neighbour refinement describe the same density: the same optical depth within the bound."""
    for name in WALK_GRIDS:
        medium, density, o, d, t_end, tau_max, _ = walk_cases(name)
        if max(density.shape) * 2 > 256:
            continue
        fine = density.repeat(2, 0).repeat(2, 1).repeat(2, 2)
        a, b = vr.walks(medium, density, o, d, t_end), vr.walks(medium, fine, o, d, t_end)
        err = np.abs(a["acc"].astype(np.float64) - b["acc"]) / tau_max
        print(f"grid {name}: refinement max relative difference {err.max():.3e}")
        assert err.max() <= WALK_TOL, (name, err.max())
        assert (b["cells"] >= a["cells"]).all()


def test_free_flight_inverts_the_optical_depth():
    """The free flight's event lies where the optical depth from t0 reaches rem: acc over [0, t_event] equals rem within the bound, and
    there is no event iff rem is not below the whole optical depth (up to the bound)."""
    for name in WALK_GRIDS:
        medium, density, o, d, t_end, tau_max, _ = walk_cases(name)
        full = vr.walks(medium, density, o, d, t_end)
        rng = np.random.default_rng(5)
        rem = (full["acc"] * rng.uniform(0.05, 1.6, full["acc"].shape)).astype(np.float32)
        got = vr.walks(medium, density, o, d, t_end, rem=rem)
        ev = got["event"] == 1
        assert ev.sum() > 100 and ((full["hit"] == 1) & ~ev).sum() > 50
        part = vr.walks(medium, density, o[ev], d[ev], got["t_event"][ev])
        err = np.abs(part["acc"].astype(np.float64) - rem[ev]) / tau_max
        assert err.max() <= WALK_TOL, (name, err.max())
        clear = np.abs(rem.astype(np.float64) - full["acc"]) / tau_max > WALK_TOL
        assert (ev[clear] == (rem < full["acc"])[clear]).all()


# ---- statistics on the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r1,r2", [(1.0, 0.4), (1.5, 0.0)])
def test_two_slabs_are_beer_lambert(r1, r2):
    """albedo = 0, a 2 x 1 x 1 grid (two slabs of densities r1 != r2 across x) in front of a constant background, no emitters, pinhole: the
    share of samples that come through lies within |z| <= 4.5 of exp(-sigma_t (r1 L1 + r2 L2)) over ABSORB_N samples, L1 and L2 in float64
    from the pixel-centre ray.  Pixels: those whose rays enter by the face x = -1 and leave by x = 1 at the centre and the four corners, and
    whose optical depth varies by < 1 % over the corners."""
    host = _fog_ball_scene()
    w = h = 9
    cam = rb.make_camera(w, h, 8.0, (-9, 0.4, 0.3), (0, 0, 0), BACKGROUND, ABSORB_N, 8)
    sigma = 0.9
    medium = dict(sigma_t=sigma, albedo=0.0, box=(-1, -1, -1, 1, 1, 1))
    density = np.array([[[r1, r2]]], np.float32)
    o = np.array([cam.origin.e[k] for k in range(3)], np.float64)
    p00 = np.array([cam.pixel00_loc.e[k] for k in range(3)], np.float64)
    du = np.array([cam.pixel_delta_u.e[k] for k in range(3)], np.float64)
    dv = np.array([cam.pixel_delta_v.e[k] for k in range(3)], np.float64)

    def depth(i, j):
        """sigma_t (r1 L1 + r2 L2) of the ray through (i, j), or None unless it crosses both slabs from face to face."""
        dd = p00 + i * du + j * dv - o
        dd /= np.linalg.norm(dd)
        t = [(x - o[0]) / dd[0] for x in (-1.0, 0.0, 1.0)]
        for tt in (t[0], t[2]):
            p = o + tt * dd
            if not (abs(p[1]) < 1.0 and abs(p[2]) < 1.0):
                return None
        return sigma * (r1 * (t[1] - t[0]) + r2 * (t[2] - t[1]))
    fb, mom = vr.frame(host, cam, medium=medium, density=density, emitters=False, moments=True)
    checked = 0
    for j in range(h):
        for i in range(w):
            tau = depth(i, j)
            corners = [depth(i + a, j + b) for a in (-0.5, 0.5) for b in (-0.5, 0.5)]
            if tau is None or None in corners or (max(corners) - min(corners)) > 0.01 * tau:
                continue
            checked += 1
            p = np.exp(-tau)
            mean = mom[j, i, 0] / ABSORB_N / BACKGROUND[0]
            z = (mean - p) / np.sqrt(p * (1 - p) / ABSORB_N)
            print(f"r ({r1}, {r2}) pixel ({i}, {j}) tau {tau:.4f} share {mean:.5f} want {p:.5f} z {z:+.2f}")
            assert abs(z) <= 4.5, (i, j, z)
    assert checked >= 9


def test_uniform_grid_has_the_homogeneous_expectation():
    """A uniform 8^3 grid of density 1 in the fog box of tests/test_medium.py against the homogeneous box itself: per pixel and channel
    |z| <= 4.5 with each frame's own sample variance, at EQUAL_SPP — test_equal_expectation_under_fog's protocol and bound."""
    host, _, _ = scenes()["three balls"]
    cam = rb.make_camera(4, 4, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), EQUAL_SPP, 6)
    a = vr.frame(host, cam, medium=FOG_BOX, density=np.ones((8, 8, 8), np.float32), moments=True)[1]
    b = mr.frame(host, cam, medium=FOG_BOX, moments=True)[1]
    z = _channel_z(a, b, EQUAL_SPP)
    print("max |z|", float(np.abs(z).max()))
    assert np.abs(z).max() <= 4.5 and a[..., :3].sum() > 0
    assert (a != b).any()          # (the walks differ: eight cells' roundings against one)


@pytest.mark.parametrize("g", [0.0, 0.7])
def test_white_furnace(g):
    """albedo = 1 in a random 4^3 grid under background 1, max_depth = 200: every path that ends by a miss returns exactly 1.0f in every
    channel, and at most 0.1 % of the samples are cut by depth."""
    host = _fog_ball_scene()
    cam = rb.make_camera(16, 16, 20.0, (0, 1, 8), (0, 0, 0), (1.0, 1.0, 1.0), 8, 200)
    ijs = all_ijs(16, 16, 8)
    rad, rays, events, ends, seeds, cells = vr.trace(host, cam, ijs, medium=dict(sigma_t=1.0, albedo=1.0, g=g, box=(-1, -1, -1, 1, 1, 1)),
                                                     density=random_grid((4, 4, 4), 21), emitters=False)
    missed = ends == mr.END_MISS
    assert (rad[missed] == np.float32(1.0)).all()
    assert (~missed).mean() <= 0.001, (~missed).mean()
    assert events.max() >= 3 and (events > 0).mean() > 0.1


def test_equal_expectation_under_a_random_grid():
    """The lamp scene under a random 8^3 grid with a third of its cells empty: mis against light-only, light samples off, and select = 1
    agree per pixel and per channel, |z| <= 4.5 (test_equal_expectation_under_fog's protocol)."""
    host, _, _ = scenes()["three balls"]
    cam = rb.make_camera(4, 4, 40.0, (0, 2, 7), (0, 1, 0), (0, 0, 0), EQUAL_SPP, 6)
    density = random_grid((8, 8, 8), 31)
    assert abs((density == 0).mean() - 1 / 3) < 0.06
    medium = dict(FOG_BOX, sigma_t=0.25)
    frames = {}
    for name, kw in (("mis", dict(nee_mis=1)), ("light", dict(nee_mis=0)), ("off", dict(emitters=False)), ("select", dict(nee_mis=1, select=1))):
        frames[name] = vr.frame(host, cam, medium=medium, density=density, moments=True, **kw)[1]
    for a, b in (("mis", "light"), ("mis", "off"), ("mis", "select")):
        z = _channel_z(frames[a], frames[b], EQUAL_SPP)
        print(a, b, "max |z|", float(np.abs(z).max()))
        assert np.abs(z).max() <= 4.5, (a, b, z)
    assert frames["mis"][..., :3].sum() > 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------

def fog(g=0.0):
    return dict(sigma_t=0.5, albedo=(0.95, 0.9, 0.8), g=g, box=BOX)


def special_camera(kind, w, h, spp, depth):
    """inside: the eye inside the grid.  fan: every camera ray has d_z == 0 exactly (the camera's up is +z: no vertical extent, the pixel
    row at the eye's height z = 0.5, a cell plane of the 16^3 grid).  vertex: aimed at the grid vertex (0, 1.5, 0) of the 16^3 grid."""
    bg = (0.1, 0.2, 0.3)
    if kind == "inside":
        return rb.make_camera(w, h, 60.0, (1.0, 1.5, 2.5), (0, 1, 0), bg, spp, depth)
    if kind == "vertex":
        return rb.make_camera(w, h, 30.0, (2.0, 3.0, 9.0), (0, 1.5, 0), bg, spp, depth)
    cam = rb.make_camera(w, h, 40.0, (9.0, 1.25, 0.5), (0.0, 1.25, 0.5), bg, spp, depth)
    for k in range(3):
        cam.pixel_delta_v.e[k] = 0.0
    cam.pixel00_loc.e[2] = cam.origin.e[2]
    assert cam.pixel_delta_u.e[2] == 0.0
    return cam


def _probe_cases(scene):
    """(grid, setting, g, depth, camera): every setting on every scene with the grids, g in {0, +-0.95} and the depths {1, 2, 12} spread
    over them, then the three special cameras."""
    si = ["three balls", "night rtiow", "fuzz planes"].index(scene)
    out = []
    for k, setting in enumerate(SETTINGS):
        out.append((list(GRIDS)[(k + si) % 4], setting, (0.0, 0.95, -0.95)[(k + si) % 3], (12, 2, 1)[(k + si) % 3] if k % 2 else 12, "scene"))
    out += [("16", "mis", 0.0, 12, "inside"), ("16", "glossy", 0.95, 12, "fan"), ("16", "select", -0.95, 12, "vertex"),
            ("2x3x5", "env sun mis", 0.0, 2, "inside"), ("1x1x64", "mis", 0.0, 12, "fan")]
    return out


def _camera(scene, kind, w, h, spp, depth):
    return scenes()[scene][1](w, h, spp, depth) if kind == "scene" else special_camera(kind, w, h, spp, depth)


@functools.lru_cache(maxsize=None)
def probe_reference(scene, grid, setting, g, depth, kind):
    host = scenes()[scene][0]
    w, h, spp = PROBE_VIEW
    return vr.trace(host, _camera(scene, kind, w, h, spp, depth), all_ijs(w, h, spp), medium=fog(g), density=GRIDS[grid], **ref_kw(scene, setting, w, h, spp, depth))


def _compare_probe(got, want, what):
    rad, rays, events, seeds, ns, es, ms, cells = got
    wrad, wrays, wevents, wends, wseeds, wcells = want
    assert_same(rad, wrad, what + ": radiance")
    assert_same(rays, wrays, what + ": rays")
    assert_same(events, wevents, what + ": medium events")
    assert_same(cells, wcells, what + ": cells")
    for k, col in enumerate((seeds, ns, es, ms)):
        assert_same(col, wseeds[:, k], what + f": final seed {k}")


def test_the_fan_camera_has_parallel_rays():
    """(no GPU) the fan camera's rays have d_z == 0 exactly and the restatement walks them (the box's d_k == 0 branch, inside)."""
    host = scenes()["three balls"][0]
    w, h, spp = PROBE_VIEW
    out = mr.trace(host, special_camera("fan", w, h, spp, 1), all_ijs(w, h, spp), medium=fog(), stats=True)
    assert out[5]["box_parallel_in"] >= w * h * spp


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow", "fuzz planes"])
def test_probe_samples_equal_the_restatement(scene):
    host = scenes()[scene][0]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    seen_events = seen_cells = 0
    volumes = {name: rb.Volume(g) for name, g in GRIDS.items()}
    with rb.Env(sun_map()) as env:
        for grid, setting, g, depth, kind in _probe_cases(scene):
            want = probe_reference(scene, grid, setting, g, depth, kind)
            got = dev.trace_samples_volume(_camera(scene, kind, w, h, spp, depth), ijs, medium=fog(g), volume=volumes[grid],
                                           **dev_kw(scene, setting, env, w, h, spp, depth))
            _compare_probe(got, want, f"{scene} / grid {grid} / {setting} / g {g} / depth {depth} / camera {kind}")
            seen_events += int(want[2].sum())
            seen_cells += int(want[5].sum())
    assert seen_events > 100 and seen_cells > 10 * seen_events
    for v in volumes.values():
        v.close()
    dev.close()


@pytest.mark.gpu
def test_frames_equal_the_restatement():
    """40 x 27 x 3 spp, 7 x 5 x 1, a 3-row shard of the first, sample_first = 5, sync = 0 on a torch stream, and one small frame through
    each of the other instantiations of volume_render_kernel."""
    import torch
    scene, setting = "three balls", "glossy"
    host, camera, _ = scenes()[scene]
    medium, density = fog(0.7), GRIDS["2x3x5"]
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env, rb.Volume(density) as vol, rb.Volume(GRIDS["16"]) as vol16:
        for (w, h, spp), more in (((40, 27, 3), {}), ((7, 5, 1), {}), ((40, 27, 3), dict(shard=rb.Shard(3, 1, 4))), ((40, 27, 3), dict(sample_first=5))):
            cam = camera(w, h, spp, 12)
            want = vr.frame(host, cam, medium=medium, density=density, **more, **ref_kw(scene, setting, w, h, spp, 12))
            got, _ = dev.render_volume_to_host(cam, medium=medium, volume=vol, **more, **dev_kw(scene, setting, env, w, h, spp, 12))
            assert_same(got, want, f"frame {w}x{h}x{spp} {more}")
        # lens + motion with the light tree over the two-kind table, on a stream, without waiting inside the call
        scene2 = "fuzz planes"
        host2, camera2, _ = scenes()[scene2]
        dev2 = rb.DeviceScene(host2, device=0)
        w, h, spp = 40, 27, 3
        cam = camera2(w, h, spp, 12)
        kw_r = {**ref_kw(scene2, "lens + motion", w, h, spp, 12), "select": 1, "planes": 1}
        kw_d = dev_kw(scene2, "lens + motion", env, w, h, spp, 12)
        kw_d["nee"] = dict(select=1, sample_planes=1)
        want = vr.frame(host2, cam, medium=fog(-0.5), density=GRIDS["16"], **kw_r)
        stream = torch.cuda.Stream()
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        with torch.cuda.stream(stream):
            dev2.render_volume(cam, fb.data_ptr(), medium=fog(-0.5), volume=vol16, stream=stream.cuda_stream, sync=False, **kw_d)
        stream.synchronize()
        assert_same(fb.cpu().numpy(), want, "sync = 0 on a torch stream")
        # the other seven instantiations, each on a small frame, the 2 x 3 x 5 and the 16^3 grid in turn
        w, h, spp = 24, 13, 2
        k = 0
        for lens in (False, True):
            for select, planes in ((0, 0), (0, 1), (1, 0), (1, 1)):
                if (lens, select, planes) == (True, 1, 1):
                    continue            # (above)
                setting = "lens + motion" if lens else "mis"
                cam = camera2(w, h, spp, 12)
                kw_r = {**ref_kw(scene2, setting, w, h, spp, 12), "select": select, "planes": planes}
                kw_d = dev_kw(scene2, setting, env, w, h, spp, 12)
                kw_d["nee"] = dict(select=select, sample_planes=planes)
                want = vr.frame(host2, cam, medium=fog(0.3), density=(density, GRIDS["16"])[k % 2], **kw_r)
                got, _ = dev2.render_volume_to_host(cam, medium=fog(0.3), volume=(vol, vol16)[k % 2], **kw_d)
                assert_same(got, want, f"frame lens={lens} select={select} planes={planes}")
                k += 1
        dev2.close()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_device_identities(scene):
    """A 1^3 grid of density 1 is rt_render_medium with the box — frames and probes, each through its own kernels; volume == NULL is
    rt_render_medium (whatever the region); a grid of zeros is rt_render_lit in radiance (and rays and the three streams)."""
    host, camera, _ = scenes()[scene]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env, rb.Volume(np.ones((1, 1, 1), np.float32)) as one, rb.Volume(np.zeros((5, 3, 2), np.float32)) as zero:
        for k, setting in enumerate(SETTINGS):
            kw = dev_kw(scene, setting, env, w, h, spp, 12)
            cam = camera(w, h, spp, 12)
            medium = fog((0.0, 0.7, -0.95)[k % 3])
            what = f"{scene} / {setting}"
            hom = dev.trace_samples_medium(cam, ijs, medium=medium, **kw)
            got = dev.trace_samples_volume(cam, ijs, medium=medium, volume=one, **kw)
            for a, b, col in zip(got[:7], hom, ("radiance", "rays", "events", "seed", "nee seed", "env seed", "med seed")):
                assert_same(a, b, f"{what}: 1^3 grid, {col}")
            assert got[7].sum() > 0 and hom[2].sum() > 0
            want, _ = dev.render_medium_to_host(cam, medium=medium, **kw)
            frame, t = dev.render_volume_to_host(cam, medium=medium, volume=one, **kw)
            assert_same(frame, want, f"{what}: 1^3 grid, frame")
            # no volume: rt_render_medium itself, a ball included
            ball = media(scene)["ball g=0.7"]
            none = dev.trace_samples_volume(cam, ijs, medium=ball, volume=None, **kw)
            for a, b in zip(none[:7], dev.trace_samples_medium(cam, ijs, medium=ball, **kw)):
                assert_same(a, b, f"{what}: volume == NULL")
            assert not none[7].any()
            assert_same(dev.render_volume_to_host(cam, medium=ball, volume=None, **kw)[0], dev.render_medium_to_host(cam, medium=ball, **kw)[0],
                        f"{what}: volume == NULL, frame")
            # zeros: rt_render_lit
            lit = dev.trace_samples_lit(cam, ijs, **kw)
            z = dev.trace_samples_volume(cam, ijs, medium=medium, volume=zero, **kw)
            for a, b, col in zip((z[0], z[1], z[3], z[4], z[5]), lit, ("radiance", "rays", "seed", "nee seed", "env seed")):
                assert_same(a, b, f"{what}: zero grid, {col}")
            assert not z[2].any() and z[7].sum() > 0
            assert_same(dev.render_volume_to_host(cam, medium=medium, volume=zero, **kw)[0], dev.render_lit_to_host(cam, **kw)[0], f"{what}: zero grid, frame")
    dev.close()


@pytest.mark.gpu
def test_handle_state_is_left_alone():
    """rt_render and rt_render_lit of a handle after a volume call equal a fresh handle's."""
    host, camera, _ = scenes()["three balls"]
    cam = camera(24, 16, 2, 12)
    fresh = rb.DeviceScene(host, device=0)
    want_render, _ = fresh.render_to_host(cam)
    want_lit, _ = fresh.render_lit_to_host(cam)
    fresh.close()
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(GRIDS["16"]) as vol:
        dev.render_volume_to_host(cam, medium=fog(0.3), volume=vol)
    got_render, _ = dev.render_to_host(cam)
    got_lit, _ = dev.render_lit_to_host(cam)
    assert_same(got_render, want_render, "rt_render after rt_render_volume")
    assert_same(got_lit, want_lit, "rt_render_lit after rt_render_volume")
    dev.close()


@pytest.mark.gpu
def test_limits():
    """A 256 x 1 x 1 grid runs (and equals the restatement); a 257-wide one is refused; a ball or no medium with a volume is refused."""
    host, camera, _ = scenes()["three balls"]
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    cam = camera(w, h, spp, 12)
    density = random_grid((1, 1, 256), 41)
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(density) as vol:
        assert (vol.nx, vol.ny, vol.nz) == (256, 1, 1)
        _compare_probe(dev.trace_samples_volume(cam, ijs, medium=fog(), volume=vol), vr.trace(host, cam, ijs, medium=fog(), density=density), "256 x 1 x 1")
        for medium in (None, media("three balls")["ball g=0.7"], dict(sigma_t=0.0)):
            with pytest.raises(rb.RtError, match="region 2"):
                dev.render_volume_to_host(cam, medium=medium, volume=vol)
    with pytest.raises(rb.RtError, match="dimension"):
        rb.Volume(np.ones((1, 1, 257), np.float32))
    dev.close()
