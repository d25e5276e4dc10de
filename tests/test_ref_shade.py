"""The oracle's RNG, materials, camera, saver and path loop against the REFERENCE'S OWN CODE (oracle/ref_shade.cpp →
oracle/_ref/libref_shade.so, built from where it lies, build container only): include/random_utils.h, materials.h, camera.cuh and
src/camera.cu, compiled host-only — the vendor SDK headers those files name are alias headers of ours (oracle/shim/) that define
no behaviour.  Bit for bit (a NaN equals a NaN), on crafted inputs — a draw of exactly 1.0 against metal's `< 0.8f` and the
dielectric's `> p`, incidence in float steps across total internal reflection, draws within a few steps of `reflectance`,
absorption that overflows, cameras that look along vup — and 10^5 to 10^6 random items per routine; then whole paths
(ray_color_host seeded as render_cpu seeds it) and small frames (render_cpu) on ten scenes.

The reference's side is also recorded (tests/golden/make_ref_shade_golden.py): per-output sha256 digests of what the library
returns on the full runs (tests/golden/ref_shade_digests.json) and the outputs themselves on smaller sets
(tests/golden/ref_shade.npz).  The oracle is checked against the recordings everywhere, and item by item against the library
where it is built.  The GPU tests at the end compare the DEVICE with the recording directly, not through the oracle.

Two things of the reference are undefined and excluded: tex2D_cpu reads outside its rows when u or v lands on the
far edge (orc_tex2d wraps there; those coordinates never reach the reference, path samples that meet one are left out, and the
shares are capped: 1 % of the texture cases, 0.1 % of a textured scene's samples), and hit_bvh picks its child order from
`direction()[-1]` (the scenes have no exact ties: the oracle shows per sample that no result depends on the order).
Not covered: src/main.cu — the config parser, texture loading and the frame loop's camera path.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import ref_shade_cases as rs
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_shade.npz")
DIGESTS = os.path.join(HERE, "golden", "ref_shade_digests.json")
have_ref = os.path.exists(rs.REF_LIB)
TEXTURE_CASE_CAP = 0.01        # share of the generated texture coordinates the reference cannot be given
TEXTURED_SAMPLE_CAP = 0.001    # share of a textured scene's samples that meet such a coordinate


@pytest.fixture(scope="module")
def libs():
    return (rs.Ref() if have_ref else None), rs.Orc()


@pytest.fixture(scope="module")
def recorded():
    with open(DIGESTS) as f:
        return json.load(f), np.load(GOLDEN)


def compare(ref, orc, what, keep=None):
    for key in ref:
        a, b = ref[key], orc[key]
        sel = np.ones(a.shape[0], bool) if keep is None else keep.copy()
        if key in rs.MASKED:
            sel &= ref[rs.MASKED[key]] != 0
        a, b = a[sel], b[sel]
        d = rs.differing(a, b)
        assert not d.any(), f"{what}: '{key}' differs in {int(d.sum())} of {d.size} items, first at {int(np.argmax(d))}: {a[np.argmax(d)]} vs {b[np.argmax(d)]}"


def against_reference(topic, libs, digests):
    """Every run of a topic: the oracle's outputs against the reference's recorded digests everywhere, and item by item against the
    library's own outputs where it is built (which must also still match the recording).  Returns the oracle's outputs by run."""
    ref, orc = libs
    outs = {}
    ref_runs = rs.full_runs(topic, ref, orc) if ref else None
    for what, o, keep in rs.full_runs(topic, orc, orc):
        want = digests[what]
        if ref:
            what_r, r, _ = next(ref_runs)
            assert what_r == what
            compare(r, o, what, keep)
            assert rs.digests(r, list(want), keep) == want, f"{what}: the reference's outputs no longer match the recorded digests"
        got = rs.digests(o, list(want), keep)
        bad = [k for k in want if got[k] != want[k]]
        assert not bad, f"{what}: {bad} differ from the reference's recorded outputs"
        outs[what] = o
    return outs


def hash_steps(before, after, most=64):
    """How many wang_hash steps lead from each state to the other (-1: more than `most`)."""
    steps, s = np.full(before.shape, -1), before.copy()
    for k in range(most + 1):
        steps[(steps < 0) & (s == after)] = k
        s = rs.wang_hash(s)
    return steps


def test_struct_sizes():
    if have_ref:
        assert rs.Ref().sizes() == (76, 64)                  # CameraData, MaterialData (include/rtp_amd.h)
    assert (C.sizeof(rb.CameraData), C.sizeof(rb.Material), rs.MATERIAL_DTYPE.itemsize) == (76, 64, 64)


def test_rng_against_the_reference(libs, recorded, golden):
    """wang_hash, random_float(seed), random_float(seed, min, max) — also as random_in_unit_sphere writes it, with the double
    literals -1.0, 1.0 —, random_in_unit_sphere, random_unit_vector, random_in_hemisphere on half a million states: the survey's
    pinned states, 0, 0xFFFFFFFF, states whose hash is >= 0xFFFFFF80 (the float is exactly 1.0), states whose rejection loop takes
    at least four rounds."""
    c = rs.full_cases("rng")
    o = against_reference("rng", libs, recorded[0])["rng"]
    assert c["seeds"][:len(golden["wang_hash"])].tolist() == [int(s) for s in golden["wang_hash"]]           # the pinned states come first
    assert [int(h) for h in o["hash"][:len(golden["wang_hash"])]] == list(golden["wang_hash"].values())
    s = np.array([golden["pixel00_sample0_seed"]], np.uint32)
    for want in golden["pixel00_first_random_floats"]:                                      # the survey's chain of draws
        out = libs[1].rng({"seeds": s, "lo": np.zeros(1, np.float32), "hi": np.ones(1, np.float32), "normals": np.zeros((1, 3), np.float32)})
        assert out["random_float"][0] == np.float32(want)
        s = out["random_float_seed"]
    ones = o["random_float"] == np.float32(1.0)
    assert ones.sum() >= 3 and (o["hash"][ones] >= 0xFFFFFF80).all()
    assert o["random_pm1"][ones].tolist() == [1.0] * int(ones.sum())
    n_long = int(c["n_long"][0])
    assert n_long >= 32 and (hash_steps(c["seeds"][-n_long:], o["random_in_unit_sphere_seed"][-n_long:]) >= 15).all()     # >= 4 rejections
    assert (hash_steps(c["seeds"][:1000], o["random_in_unit_sphere_seed"][:1000]) % 3 == 0).all()


def test_reflectance_against_the_reference(libs, recorded):
    """cosine in {-0, 0, denormals, 1, 1 + one step, above 1 (negative base of powf), NaN, …} x ref_idx in {1, 1/1.5, 1.5, 0, -1
    (division by zero), 1e30, …}, then 200 000 random pairs."""
    o = against_reference("reflectance", libs, recorded[0])["reflectance"]["reflectance"]
    assert np.isnan(o).sum() > 5 and np.isinf(o).any() and ((o > 0) & (o < 1)).sum() > 100_000


def test_material_scatter_against_the_reference(libs, recorded):
    """material_scatter and material_emit on a million hits: per type, unit and non-unit normals, huge / tiny / axis-parallel /
    grazing directions; METAL with fuzz 0, 0.7, 1, 5 and first draws of 1.0 and of the floats around 0.8f; DIELECTRIC with ir 1,
    1.0001, 1.5, 2.4, both faces, incidence swept across total internal reflection in float steps, Schlick draws within a few steps
    of `reflectance`, absorption 0, 0.6, 50, -0.5, -90 (overflow to inf, then `attenuation /= p`), distance 0, p = 0, a second draw
    of exactly 1.0; DIFFUSE_LIGHT, which must leave the seed alone.  (near_zero's fallback cannot be reached from any state:
    random_in_hemisphere returns a unit vector or NaNs — it is covered as code by tests/test_ref_geom.py's near_zero.)"""
    c = rs.full_cases("scatter")
    o = against_reference("scatter", libs, recorded[0])["scatter"]
    t, steps = c["mat"]["type"], hash_steps(c["seeds"], o["seed"])
    assert (o["seed"][t == rs.DIFFUSE_LIGHT] == c["seeds"][t == rs.DIFFUSE_LIGHT]).all() and not o["ret"][t == rs.DIFFUSE_LIGHT].any()
    assert (o["ret"][t == rs.LAMBERTIAN] == 1).all()
    metal = t == rs.METAL
    first = rs.wang_hash(c["seeds"]).astype(np.float32) / np.float32(4294967296.0)
    assert ((first == np.float32(1.0)) & metal).sum() > 100 and ((first == rs.ulps(rs.P8, -1)) & metal).sum() > 100          # the draws asked for
    assert (metal & (o["ret"] == 0)).sum() > 1000 and (metal & (o["ret"] == 1) & (steps == 4)).sum() > 1000                    # below the horizon; mirror branch
    assert (metal & (first >= np.float32(rs.P8)) & (o["ret"] == 1)).sum() > 1000                                               # the 20 % branch
    glass = t == rs.DIELECTRIC
    assert (glass & (steps == 1)).sum() > 1000 and (glass & (steps == 2)).sum() > 1000        # total internal reflection: no Schlick draw
    assert (glass & (o["ret"] == 0)).sum() > 1000 and (glass & np.isnan(o["att"]).any(axis=1) & (o["ret"] == 1)).sum() > 10     # absorbed; inf / inf
    moved = np.einsum("ij,ij->i", o["sc_o"] - c["point"], c["normal"])
    assert (glass & (o["ret"] == 1) & (moved > 0)).sum() > 1000 and (glass & (o["ret"] == 1) & (moved < 0)).sum() > 1000        # both signs of the offset


def test_tex2d_against_the_reference(libs, recorded):
    """tex2D_cpu on 1x1, 4x4, 5x3 and 256x256 textures: u, v negative, above 1, -0, denormal, 1 - 2^-24 and 100 000 random pairs
    each.  Coordinates at which the reference reads outside its rows (int(px) == width or int(py) == height: any integral v) never
    reach it — they are found with its own float32 arithmetic, are at most 1 % of the cases, and on them the oracle must give
    "wrap" as numpy states it."""
    against_reference("tex", libs, recorded[0])
    for tex, u, v in rs.full_cases("tex"):
        w, h = tex.shape[1], tex.shape[0] - rs.SPARE_ROWS
        outside = rs.tex_reads_outside(u, v, w, h)
        share = outside.mean()
        print(f"tex2D {w}x{h}: {int(outside.sum())} of {outside.size} coordinates excluded ({100 * share:.3f} %)")
        assert 0 < share <= TEXTURE_CASE_CAP
        o = libs[1].tex2d(tex, u, v)
        assert ((o["wrapped"] != 0) == outside).all()
        assert rs.same_bits(o["tex"][outside], rs.tex_wrapped(tex, u[outside], v[outside]))


def test_cameras_against_the_reference(libs, recorded):
    """Camera::build_camera_data against the host mirror's — 1x1, 1920x1080, 3840x2160; vfov 1, 60, 179 and more; on the orbit of
    config.txt, straight above the target (vup parallel to w: the NaNs must agree), look-from == look-at — all 76 bytes; then
    CameraData::get_ray on 200 000 (camera, i, j, seed) with i, j at both ends."""
    outs = against_reference("cameras", libs, recorded[0])
    f = outs["cameras"]["cam_floats"]
    assert np.isnan(f[:, 3:12]).all(axis=1).sum() >= 3 * len(rs.VFOVS) * len(rs.IMAGES) and np.isfinite(f).all(axis=1).sum() >= 6 * len(rs.VFOVS) * len(rs.IMAGES)
    assert np.isfinite(outs["get_ray"]["d"]).all(axis=1).sum() > 100_000


def test_write_color_against_the_reference(libs, recorded):
    """BinarySaver::writeColor through a file, read back: sums -0, negative, 0, denormal, exactly spp, spp x 0.999^2 and the floats
    around it, around every byte threshold, NaN, inf and 100 000 random pixels at spp 1, 4, 100, 2500."""
    outs = against_reference("write_color", libs, recorded[0])
    for o in outs.values():
        assert (o["bytes"] == 255).sum() > 1000 and (o["bytes"] == 0).sum() > 1000 and len(np.unique(o["bytes"])) == 256


def test_paths_and_frames_against_the_reference(libs, recorded):
    """ray_color_host on 4 096 samples (seeded as render_cpu seeds them) at depths 1, 2 and 50, and one 48x32x4 spp frame through
    render_cpu, on ten scenes (of at most 40 primitives, but for the test config's 199): each material alone on a sphere and every plane type, glass inside glass
    with positive, zero and negative absorption, a fuzzed metal floor at a grazing view, emitters, a textured quad and sphere,
    tests/golden/test_config.txt, forty mixed primitives.  No sample's closest hits depend on the order leaves are visited in
    (brute force agrees with hit_bvh on every ray), and the samples left out for a texture fetch at the far edge stay below 0.1 %."""
    orc = libs[1]
    outs = against_reference("paths", libs, recorded[0])
    assert len(outs) == 4 * len(rs.full_cases("paths"))
    for k, sc in enumerate(rs.full_cases("paths")):
        assert sc.spheres.shape[0] + sc.planes.shape[0] <= 40 or sc.name == "test_config"         # that one is what the reference's printer makes
        wrapped = total = 0
        for depth in rs.DEPTHS:
            flags = rs.cached(("flags", k, depth), None)
            assert not (flags & 2).any(), f"{sc.name}: {int(((flags & 2) != 0).sum())} samples depend on the order of the visit"
            wrapped, total = wrapped + int((flags & 1).sum()), total + flags.size
        frame = orc.frame(sc)
        assert not frame["order"].any()
        wrapped, total = wrapped + int(frame["wrapped"].sum()) , total + frame["wrapped"].size
        if sc.textures:
            print(f"paths {sc.name}: {wrapped} of {total} samples / pixels excluded for a texture fetch at the far edge ({100 * wrapped / total:.4f} %)")
            assert wrapped / total <= TEXTURED_SAMPLE_CAP
        else:
            assert wrapped == 0
        assert np.abs(outs[f"{sc.name} depth 50"]["rad"]).sum() > 0


# ---- the recording: runs everywhere, also where the reference itself is not --------------------------------------------------------
def fixture_scene(g, name):
    pre = f"scene_{name}_"
    return rs.PathScene.from_arrays(name, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})


def scene_names(g):
    return [str(s) for s in g["scene_names"]]


def test_oracle_against_the_recorded_reference_outputs(recorded):
    """The same comparisons against outputs of the reference's own code recorded in tests/golden/ref_shade.npz: 1 024 cases per
    routine, and per scene the samples' radiance bits and final seeds and the small frame."""
    g, orc = recorded[1], rs.Orc()
    for topic in ("rng", "reflectance", "scatter", "get_ray"):
        c = {k[len(topic) + 4:]: g[k] for k in g.files if k.startswith(f"{topic}_in_")}
        if topic == "scatter":
            c["mat"] = np.ascontiguousarray(c["mat"]).view(rs.MATERIAL_DTYPE).reshape(-1)
        compare({k[len(topic) + 5:]: g[k] for k in g.files if k.startswith(f"{topic}_out_")}, getattr(orc, topic)(c), f"recorded {topic}")
    for k, (w, h) in enumerate(rs.TEX_SIZES):
        tex, u, v = rs.fixture_texture(k), g[f"tex{k}_u"], g[f"tex{k}_v"]
        assert hashlib.sha256(tex.tobytes()).hexdigest() == str(g[f"tex{k}_sha256"]), "numpy no longer makes the texture the recording was made with"
        assert not rs.tex_reads_outside(u, v, w, h).any()
        compare({"tex": g[f"tex{k}_out"]}, orc.tex2d(tex, u, v), f"recorded tex {w}x{h}")
    c = {k[11:]: g[k] for k in g.files if k.startswith("cameras_in_")}
    want = rs.split_cameras(g["cameras_out"])
    compare({k: want[k] for k in ("cam_floats", "cam_ints")}, orc.cameras(c), "recorded cameras")
    for spp in rs.SPPS:
        compare({"bytes": g[f"write_color_{spp}_out"]}, orc.write_color(g[f"write_color_{spp}_in"], spp), f"recorded write_color {spp}")
    for name in scene_names(g):
        sc = fixture_scene(g, name)
        for depth in rs.DEPTHS:
            ijs, keep = g[f"path_{name}_ijs"], g[f"path_{name}_keep_{depth}"]
            o = orc.trace(sc, depth, np.ascontiguousarray(ijs, dtype=np.int32))
            assert ((o["flags"] & 1) == 0).tolist() == keep.tolist()
            compare({"rad": g[f"path_{name}_rad_{depth}"], "seed": g[f"path_{name}_seed_{depth}"]}, o, f"recorded {name} depth {depth}", keep)
        f = orc.frame(sc)
        assert (~f["wrapped"]).tolist() == g[f"path_{name}_frame_keep"].tolist()
        compare({"frame": g[f"path_{name}_frame"].reshape(-1, 3)}, {"frame": f["frame"].reshape(-1, 3)}, f"recorded {name} frame", ~f["wrapped"].ravel())


# ---- the device against the recording ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_scenes(recorded):
    g = recorded[1]
    return g, {name: fixture_scene(g, name) for name in scene_names(g)}


@pytest.mark.gpu
@pytest.mark.parametrize("config", [{}, {"traversal": rb.TRAVERSAL_EXACT}], ids=["default", "exact"])
def test_device_paths_are_the_references(fixture_scenes, config):
    """rt_trace_samples on every recorded scene at depths 1, 2 and 50: radiance bits and final RNG state equal what the reference's
    ray_color_host gave (the samples with a texture fetch at the far edge left out, as recorded), on the default handle and on the
    reference-order walk."""
    g, scenes = fixture_scenes
    for name, sc in scenes.items():
        dev = rb.DeviceScene(sc.host(), device=0, **config)
        try:
            for depth in rs.DEPTHS:
                rad, _, seeds = dev.trace_samples(sc.camera(depth), g[f"path_{name}_ijs"])
                compare({"rad": g[f"path_{name}_rad_{depth}"], "seed": g[f"path_{name}_seed_{depth}"]}, {"rad": rad, "seed": seeds}, f"{name} depth {depth}",
                        g[f"path_{name}_keep_{depth}"])
        finally:
            dev.close()


@pytest.mark.gpu
def test_device_frames_are_the_references(fixture_scenes):
    """rt_render_to_host on the recorded 48x32x4 spp frames of render_cpu, and one of them through rt_render_tile with 13x7 tiles
    (no multiple of a block, and they do not divide the image)."""
    g, scenes = fixture_scenes
    for n, (name, sc) in enumerate(scenes.items()):
        dev = rb.DeviceScene(sc.host(), device=0)
        try:
            cam, keep = sc.camera(50), g[f"path_{name}_frame_keep"].ravel()
            want = {"frame": g[f"path_{name}_frame"].reshape(-1, 3)}
            fb, _ = dev.render_to_host(cam)
            compare(want, {"frame": fb.reshape(-1, 3)}, f"{name} frame", keep)
            if n == 2:
                tiled = np.zeros((sc.H, sc.W, 3), np.float32)
                for y0 in range(0, sc.H, 7):
                    for x0 in range(0, sc.W, 13):
                        w, h = min(13, sc.W - x0), min(7, sc.H - y0)
                        tiled[y0:y0 + h, x0:x0 + w] = dev.render_tile_to_host(cam, x0, y0, w, h)[0]
                compare(want, {"frame": tiled.reshape(-1, 3)}, f"{name} frame in tiles", keep)
        finally:
            dev.close()


@pytest.mark.gpu
def test_device_tonemap_is_the_references_write_color(recorded):
    """rt_tonemap on the recorded sums against the bytes BinarySaver::writeColor wrote for them, at spp 1, 4, 100, 2500."""
    import torch
    g, lib = recorded[1], rb.amd_lib()
    for spp in rs.SPPS:
        sums = torch.from_numpy(np.ascontiguousarray(g[f"write_color_{spp}_in"])).to("cuda:0")
        out = torch.zeros(sums.numel(), dtype=torch.uint8, device="cuda:0")
        assert lib.rt_tonemap(C.c_void_p(sums.data_ptr()), C.c_void_p(out.data_ptr()), C.c_int64(sums.numel()), spp,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        compare({"bytes": g[f"write_color_{spp}_out"]}, {"bytes": out.cpu().numpy().reshape(-1, 3)}, f"rt_tonemap at {spp}")


@pytest.mark.gpu
def test_device_camera_rays_are_the_references_get_ray(recorded):
    """rt_lens_camera_rays with no lens and no motion against the recorded CameraData::get_ray: origins, directions and the RNG
    state after the two draws, for the recorded items whose seed is the one render_cpu gives sample (i, j, s).  (The call accepts a
    pinhole camera: a null rt_lens_params means lens_radius 0, and lens_radius >= 0 is valid.)"""
    g = recorded[1]
    cams, ij, s = g["get_ray_in_cams"], g["get_ray_in_ij"], g["get_ray_in_s"]
    seeded = np.nonzero(s >= 0)[0]
    assert seeded.size >= 200
    done = 0
    for cam_bytes in np.unique(cams[seeded], axis=0):
        idx = seeded[(cams[seeded] == cam_bytes).all(axis=1)]
        cam = rb.CameraData.from_buffer_copy(cam_bytes.tobytes())
        ijs = np.ascontiguousarray(np.concatenate([ij[idx], s[idx, None]], axis=1), dtype=np.int32)
        o, d, seed = rb.lens_camera_rays(cam, None, None, ijs)
        compare({"o": g["get_ray_out_o"][idx], "d": g["get_ray_out_d"][idx], "seed": g["get_ray_out_seed"][idx]}, {"o": o, "d": d, "seed": seed},
                f"camera rays of a {cam.image_width}x{cam.image_height} camera")
        done += idx.size
    assert done == seeded.size
