"""The oracle's geometry against the REFERENCE'S OWN HEADERS (oracle/ref_geom.cpp → oracle/_ref/libref_geom.so, built from where
they lie, build container only): vec3 / ray / interval / aabb / hittable_object / sphere / plane / bvh / bvh_builder — the geometry
half of the hot path.  Bit for bit, on crafted extremes (zeros, ±inf reciprocals, NaN
planes, denormals, exact interval ends) and random values.

The reference's side is also recorded (tests/golden/make_ref_geom_golden.py): per-output sha256 digests of what the library
returns on the full runs (tests/golden/ref_geom_digests.json), and the outputs themselves on a smaller set
(tests/golden/ref_geom.npz).  The oracle is checked against the recordings everywhere, and item by item against the library
where it is built.
Not covered here: random_utils.h, materials.h, camera.cuh and src/camera.cu — the RNG, the materials, the camera, the saver and the
path loop are compared with the reference's own code by tests/test_ref_shade.py (oracle/ref_shade.cpp).
"""
import ctypes as C
import json
import os

import numpy as np

import ref_geom_cases as rg
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_geom.npz")
DIGESTS = os.path.join(HERE, "golden", "ref_geom_digests.json")
have_ref = os.path.exists(rg.REF_LIB)
SURVEY_SIZES = [12, 24, 8, 24, 44, 32, 80, 36]          # vec3 Ray Interval AABB HitRecord SphereData PlaneData BVHNode


def compare(ref, orc, what):
    for key in ref:
        a, b = ref[key], orc[key]
        if rg.hit_key(key):
            hit = ref[rg.hit_key(key)]
            a, b = a[hit != 0], b[hit != 0]           # records exist for hits only
        d = rg.differing(a, b)
        assert not d.any(), f"{what}: '{key}' differs in {int(d.sum())} of {d.size} items, first at {int(np.argmax(d))}: {a[np.argmax(d)]} vs {b[np.argmax(d)]}"


def against_reference(what, orc, keys, ref=None):
    """The oracle's outputs `orc` of run `what` against the reference's: against the recorded digests everywhere, and item by item
    against the library's own outputs `ref` where it is built (which must also still match the recording)."""
    with open(DIGESTS) as f:
        want = json.load(f)[what]
    if ref is not None:
        compare(ref if keys is None else {k: ref[k] for k in keys}, orc, what)
        assert rg.digests(ref, list(want)) == want, f"{what}: the reference's outputs no longer match the recorded digests"
    got = rg.digests(orc, list(want))
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{what}: {bad} differ from the reference's recorded outputs"


def test_struct_sizes_match_the_survey():
    if have_ref:
        assert list(rg.Ref().sizes()) == SURVEY_SIZES
    # the records the host mirror hands to the kernel and the oracle are laid out as the reference's: vec3 SphereData PlaneData BVHNode
    assert [C.sizeof(rb.Vec3), C.sizeof(rb.Sphere), C.sizeof(rb.Plane), C.sizeof(rb.BvhNode)] == [SURVEY_SIZES[i] for i in (0, 5, 6, 7)]


def test_primitives_against_the_reference_headers():
    """A million inputs through AABB::hit, operator/, unit_vector, reflect, refract, near_zero, dot, cross, len, contains, Ray::at,
    set_face_normal; a quarter of a million rays against a sphere / a plane each (hit_sphere + get_sphere_uv, the PlaneData
    constructor, hit_plane + is_interior_*): the oracle's restatements give the reference's bits."""
    ref, orc = (rg.Ref() if have_ref else None), rg.Orc()
    for what, c, keys in rg.primitive_runs():
        o = orc.primitives(c)
        if keys is None:
            # the cases do hit things
            assert o["aabb_hit"].sum() > 1000 and o["hit_sphere"].sum() > 50_000 and o["hit_plane"].sum() > 10_000
            assert o["near_zero"].sum() > 1000 and (o["contains"] == 0).sum() > 1000
        against_reference(what, o, keys, ref.primitives(c) if ref else None)


def test_bvh_build_and_traversal_against_the_reference_headers():
    """build_bvh (include/bvh_builder.h) against the host mirror's builder — node for node, boxes bit for bit — and hit_bvh
    (include/bvh.h) against the oracle's on 60 000 rays per scene: sphere scenes, mixed scenes with thin axis-aligned quads, one
    primitive, an empty scene.  (The reference's child order comes from an out-of-bounds read; it only matters on exact ties,
    which random scenes do not have: the comparison is strict.)"""
    ref, orc = (rg.Ref() if have_ref else None), rg.Orc()
    total_hits = 0
    for what, (ns, npl), (sph, pl, types, o, d) in rg.scene_runs():
        q = orc.scene(sph, pl, types, o, d)
        assert q["nodes"].shape == (2 * (ns + npl) - 1, 9)
        against_reference(what, q, None, ref.scene(sph, pl, types, o, d) if ref else None)
        total_hits += int(q["hit"].sum())
    assert total_hits > 100_000


def test_oracle_against_the_recorded_reference_outputs():
    """The same comparison against outputs of the reference's headers recorded in tests/golden/ref_geom.npz (1 024 primitive cases,
    two scenes): runs everywhere, also where the reference itself is not."""
    g = np.load(GOLDEN)
    orc = rg.Orc()
    c = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    o = orc.primitives(c)
    compare({k[4:]: g[k] for k in g.files if k.startswith("out_")}, o, "recorded primitives")
    for tag in ("s0", "s1"):
        q = orc.scene(g[f"{tag}_sph"], g[f"{tag}_pl"], g[f"{tag}_types"], g[f"{tag}_o"], g[f"{tag}_d"])
        compare({k: g[f"{tag}_{k}"] for k in ("nodes", "hit", "rec", "code")}, q, f"recorded scene {tag}")
