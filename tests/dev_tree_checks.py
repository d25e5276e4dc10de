"""Node-by-node checks of the device LBVH builder (csrc/rt_build.hip) against the host reference tests/lbvh_reference.py.
Needs the DEVELOPER build of the render library (librtp_amd_dev.so: rt_debug_build_lbvh, rt_debug_guard_leaves).  Not
collected by the normal test run (the file name does not match test_*.py): tests/test_device_tree.py runs it in one child
process with RTP_AMD_LIB pointing at the developer library.  Nothing here renders: the builder's records are only read back.

For every set of leaves: the device's root, record count and depth; every fp32 record (child codes and the 12 planes bit for
bit; a plane that is a min / max over both +0 and -0 by value, since fminf / fmaxf leave its sign open) and every binary16
record against the reference; invariants of the device's own records (each leaf code once, each internal node reached once
from the root, each child box exactly the union of the leaf boxes below it, pad words 0, binary16 planes the outward
rounding of the device's own fp32 planes, depth the longest path); and two builds giving the same bits."""
import ctypes as C

import numpy as np
import pytest

import lbvh_reference as ref
import rtp_bindings as rb

pytestmark = pytest.mark.gpu


def _lib():
    lib = rb.amd_lib()
    lib.rt_debug_build_lbvh.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.rt_debug_build_lbvh.restype = C.c_int
    lib.rt_debug_guard_leaves.argtypes = [C.POINTER(rb.SceneDesc), C.POINTER(rb.Config), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.rt_debug_guard_leaves.restype = C.c_int
    return lib


def device_build(boxes, codes):
    """(info [root, num_internal, depth, 0], fp32 records (n-1, 16) uint32, binary16 records (n-1, 8) uint32)."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    n = boxes.shape[0]
    nodes = np.full((max(n - 1, 1), 16), 0xdeadbeef, np.uint32)        # poisoned: a record the builder skips shows
    hnodes = np.full((max(n - 1, 1), 8), 0xdeadbeef, np.uint32)
    info = (C.c_int32 * 4)()
    st = _lib().rt_debug_build_lbvh(boxes.ctypes.data, codes.ctypes.data, n, nodes.ctypes.data, hnodes.ctypes.data, info)
    assert st == 0, rb.amd_lib().rt_get_last_error_string().decode()
    k = info[1]
    return list(info), nodes[:max(k, 0)], hnodes[:max(k, 0)]


def guard_leaves(host, **config):
    """The inflated leaves a RT_BUILD_DEVICE_LBVH handle of this scene and config hands to the builder."""
    lib = _lib()
    cfg = rb.new_config()
    for key, v in config.items():
        setattr(cfg, key, v)
    n = C.c_int32(0)
    assert lib.rt_debug_guard_leaves(C.byref(host.desc), C.byref(cfg), None, None, C.byref(n)) == 0, lib.rt_get_last_error_string()
    boxes = np.zeros((n.value, 6), np.float32)
    codes = np.zeros(n.value, np.int32)
    assert lib.rt_debug_guard_leaves(C.byref(host.desc), C.byref(cfg), boxes.ctypes.data, codes.ctypes.data, C.byref(n)) == 0
    assert n.value == len(codes)
    return boxes, codes


def _same_planes(got_bits, want_bits, ambiguous):
    """Bitwise equal, or both zero where the plane is a min / max over +0 and -0."""
    got, want = got_bits.view(np.float32), want_bits.view(np.float32)
    return (got_bits == want_bits) | (ambiguous & (got == 0) & (want == 0))


def _first(mask, k=6):
    return np.argwhere(mask)[:k].tolist()


def check_tree(boxes, codes, what):
    """Every check of this module on one set of leaves; returns the device's info."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    n = len(codes)
    want = ref.build(boxes, codes)
    info, nodes, hnodes = device_build(boxes, codes)
    root, num_internal, depth = info[0], info[1], info[2]
    assert num_internal == n - 1, f"{what}: {num_internal} records for {n} leaves"
    assert root == want["root"], f"{what}: root {root}, reference {want['root']}"
    assert info[3] == 0

    # ---- the device's own records, without the reference
    children = nodes[:, 12:14].view(np.int32).astype(np.int64)
    assert (nodes[:, 14:16] == 0).all(), f"{what}: pad words not 0 in records {_first(nodes[:, 14:16] != 0)}"
    leaf_seen = np.sort(np.concatenate([children[children < 0], [root] if root < 0 else []]).astype(np.int64))
    assert np.array_equal(leaf_seen, np.sort(codes.astype(np.int64))), \
        f"{what}: leaf codes are not each used once ({len(leaf_seen)} leaf children for {n} leaves)"
    planes, ambiguous, height = ref.child_planes(children, root, codes, boxes)     # also: every internal node reached once
    ok = _same_planes(nodes[:, :12], planes.view(np.uint32), ambiguous)
    assert ok.all(), f"{what}: {(~ok).sum()} planes are not the union of the leaf boxes below, first [record, plane] {_first(~ok)}"
    longest = int(height[root]) if root >= 0 else 0
    assert depth == longest, f"{what}: reported depth {depth}, longest path in the records {longest}"
    hwant = ref.half_records(nodes[:, :12].view(np.float32), children)
    ok = hnodes == hwant
    assert ok.all(), f"{what}: {(~ok).sum()} binary16 words are not the outward rounding of the record's own fp32 planes, " \
                     f"first [record, word] {_first(~ok)}"

    # ---- against the reference
    assert depth == want["depth"], f"{what}: depth {depth}, reference {want['depth']}"
    ok = children == want["children"]
    assert ok.all(), f"{what}: {(~ok.all(axis=1)).sum()} records have other children than the reference's, first " \
                     f"{_first(~ok.all(axis=1))}: device {children[~ok.all(axis=1)][:3].tolist()}, " \
                     f"reference {want['children'][~ok.all(axis=1)][:3].tolist()}"
    ok = _same_planes(nodes[:, :12], want["records"][:, :12], want["ambiguous"])
    assert ok.all(), f"{what}: {(~ok).sum()} planes differ from the reference's, first {_first(~ok)}"
    # (the sign of an ambiguous zero is the device's; everything else the reference's)
    signed = np.where(want["ambiguous"], nodes[:, :12], want["records"][:, :12]).view(np.float32)
    ok = hnodes == ref.half_records(signed, want["children"])
    assert ok.all(), f"{what}: {(~ok).sum()} binary16 words differ from the reference's, first [record, word] {_first(~ok)}"

    # ---- the same leaves again: the same bits
    info2, nodes2, hnodes2 = device_build(boxes, codes)
    assert info2 == info and np.array_equal(nodes2, nodes) and np.array_equal(hnodes2, hnodes), f"{what}: two builds differ"
    return info, want


# ---------------------------------------------------------------------------------------------------- cases
def sphere_boxes(centres, radii):
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    r = np.asarray(radii, np.float32).reshape(-1, 1)
    return np.stack([c[:, 0:1] - r, c[:, 0:1] + r, c[:, 1:2] - r, c[:, 1:2] + r, c[:, 2:3] - r, c[:, 2:3] + r], axis=1).reshape(-1, 6)


def mixed_codes(n, rng):
    """Distinct leaf codes of spheres (type 0) and planes (type 1)."""
    return np.array([ref.leaf_code(i, int(t)) for i, t in enumerate(rng.integers(0, 2, n))], np.int32)


def small_spheres(rng, n, spread=20.0):
    return sphere_boxes(rng.uniform(-spread, spread, (n, 3)), 10.0 ** rng.uniform(-2.0, -0.5, n))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 4097, 2 ** 17 + 3])
def test_random_leaves_of_every_size(n):
    """Sizes around the 256-thread blocks of the builder's kernels, up to 2^17 + 3 leaves (hundreds of workgroups in the
    refit's cross-workgroup handshake)."""
    rng = np.random.default_rng(1000 + n)
    info, want = check_tree(small_spheres(rng, n), mixed_codes(n, rng), f"{n} random leaves")
    assert want["num_large"] == 0
    print(f"{n} random leaves: depth {info[2]}")


def test_coincident_leaves():
    """600 identical boxes: every one of them is 'large', so the first 16 by index are chained and the other 584 share the key 0
    (a zero-extent Morton frame on every axis): the hierarchy comes from the positions alone."""
    boxes = np.tile(np.array([[1.0, 2.0, -1.0, 0.5, 3.0, 3.25]], np.float32), (600, 1))
    rng = np.random.default_rng(5)
    info, want = check_tree(boxes, mixed_codes(600, rng), "600 coincident leaves")
    assert want["num_large"] == 16 and (want["keys"] == 0).all()


def test_runs_of_equal_keys_across_blocks():
    """Runs of 37 leaves with one centre and different radii: equal keys whose sorted positions straddle the 256-thread
    block boundaries of the hierarchy and refit kernels."""
    rng = np.random.default_rng(6)
    centres = np.repeat(rng.uniform(-10, 10, (40, 3)).astype(np.float32), 37, axis=0)
    radii = rng.uniform(0.01, 0.2, len(centres))
    boxes = sphere_boxes(centres, radii)
    info, want = check_tree(boxes, mixed_codes(len(boxes), rng), "runs of equal keys")
    keys = want["keys"]
    assert (keys[255] == keys[256]) or (keys[511] == keys[512]) or (keys[767] == keys[768])


def test_zero_extent_axis():
    """Every centre at z = 3: the Morton frame's z scale is 0 (and then y too)."""
    rng = np.random.default_rng(7)
    n = 900
    centres = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), np.full(n, 3.0)]).astype(np.float32)
    check_tree(sphere_boxes(centres, rng.uniform(0.01, 0.1, n)), mixed_codes(n, rng), "zero extent in z")
    centres[:, 1] = -2.0
    check_tree(sphere_boxes(centres, rng.uniform(0.01, 0.1, n)), mixed_codes(n, rng), "zero extent in y and z")


def _with_large(rng, n_small, radii_large, spread=10.0):
    small = small_spheres(rng, n_small, spread)
    big = sphere_boxes(rng.integers(-2, 3, (len(radii_large), 3)), radii_large)          # c -/+ r exact: equal radii, equal extents
    boxes = np.concatenate([small, big])
    perm = rng.permutation(len(boxes))
    return boxes[perm]


@pytest.mark.parametrize("num_big,equal", [(1, False), (2, True), (16, False), (17, False), (17, True), (24, True)])
def test_large_primitives_chained_above_the_root(num_big, equal):
    """Primitives wider than a quarter of the scene: chained above the LBVH root, largest first with ties by leaf index, at
    most 16 of them."""
    rng = np.random.default_rng(100 + num_big + 50 * equal)
    radii = np.full(num_big, 6.0) if equal else rng.uniform(4.0, 8.0, num_big)
    boxes = _with_large(rng, 300, radii)
    info, want = check_tree(boxes, mixed_codes(len(boxes), rng), f"{num_big} large{' of equal extent' if equal else ''}")
    assert want["num_large"] == min(num_big, 16)


@pytest.mark.parametrize("n", [3, 5, 17])
def test_all_but_one_primitive_large(n):
    """m == 1: n - 1 large primitives and one small one: the chain starts from a leaf."""
    rng = np.random.default_rng(200 + n)
    boxes = np.concatenate([sphere_boxes(rng.uniform(-1, 1, (n - 1, 3)), rng.uniform(5, 6, n - 1)), sphere_boxes([[0.5, 0, 0]], [0.05])])
    boxes = boxes[rng.permutation(n)]
    info, want = check_tree(boxes, mixed_codes(n, rng), f"{n - 1} large, one small")
    assert want["num_large"] == n - 1 and info[2] == n - 1


def test_the_rule_for_large_primitives_at_its_edges():
    """n = 2 never chains (one large, one small); n = 3 with three equal boxes: every one is large, so none is; an extent of
    exactly a quarter of the scene's is not large, the next float above it is."""
    rng = np.random.default_rng(9)
    two = np.concatenate([sphere_boxes([[0, 0, 0]], [5.0]), sphere_boxes([[1, 0, 0]], [0.1])])
    info, want = check_tree(two, mixed_codes(2, rng), "n = 2, one large")
    assert want["num_large"] == 0
    three = sphere_boxes(np.zeros((3, 3)), [2.0, 2.0, 2.0])
    info, want = check_tree(three, mixed_codes(3, rng), "three equal large boxes")
    assert want["num_large"] == 0
    for side, large in ((1.0, False), (float(np.nextafter(np.float32(1.0), np.float32(2.0))), True)):
        boxes = np.array([[0, 4, 0, 0.1, 0, 0.1], [0, 0.1, 0, 0.1, 0, 0.1], [0, side, 1, 1.5, 0, 0.5], [3, 3.1, 3, 3.1, 3, 3.1]], np.float32)
        info, want = check_tree(boxes, mixed_codes(4, rng), f"extent {side} of 4")
        assert (2 in want["order"][:want["num_large"]]) == large


def test_deep_tree():
    """Centres whose keys are single bits (x = 2^k, y = 2^k, z = 2^k in a frame of scale 1): each split peels off one leaf,
    a tree of depth 64 — far beyond the 12-level stack of the global-memory walk."""
    rng = np.random.default_rng(11)
    pts = [(0.0, 0.0, 0.0), (2097151.0, 2097151.0, 2097151.0)]
    for k in range(21):
        pts += [(2.0 ** k, 0, 0), (0, 2.0 ** k, 0), (0, 0, 2.0 ** k)]
    boxes = sphere_boxes(pts, np.full(len(pts), 0.25))
    boxes = boxes[rng.permutation(len(boxes))]
    info, want = check_tree(boxes, mixed_codes(len(boxes), rng), "deep tree")
    assert info[2] >= 60, info
    print(f"deep tree: {len(boxes)} leaves, depth {info[2]}")


def test_planes_of_binary16_interest():
    """Leaf planes at and around the binary16 limits (65504, the rounding edge 65520, 65536, beyond), in its subnormal range,
    at exact halves and their float neighbours, and signed zeros: the binary16 records must round every one outward."""
    nxt = lambda v, d: float(np.nextafter(np.float32(v), np.float32(d)))
    vals = [0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, nxt(2.0 ** -14, 0), 2.0 ** -14 - 2.0 ** -25, 6e-8, 1e-10, 1e-45,
            1.0, 1.5, 1024.5, 2047.5, 1.0 + 2.0 ** -11, 0.1, 1.0 / 3.0, 65504.0, 65505.0, 65519.0, 65520.0, 65536.0, 70000.0, 1e6, 1e30]
    vals += [nxt(v, np.inf) for v in vals] + [nxt(v, 0.0) for v in vals if v != 0]
    vals = sorted(set(vals))
    vals = np.array(vals + [-v for v in vals] + [-0.0], np.float32)
    rng = np.random.default_rng(13)
    boxes = []
    for v in vals:
        up, down = np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))
        boxes += [[v, v, down, v, v, up], [down, up, v, v, v, v], [v, up, v, up, down, v]]
    boxes = np.array(boxes, np.float32)
    boxes = boxes[rng.permutation(len(boxes))]
    check_tree(boxes, mixed_codes(len(boxes), rng), "planes of binary16 interest")
    # +0 and -0 planes under one internal node (the first two share their key): a union whose sign fminf leaves open
    zeros = np.array([[0, 1, 0, 1, 0, 1], [-0.0, 1, -0.0, 1, -0.0, 1], [10, 11, 10, 11, 10, 11], [20, 21, 20, 21, 20, 21]], np.float32)
    info, want = check_tree(zeros, mixed_codes(4, rng), "+0 and -0 planes")
    assert want["ambiguous"].any()


@pytest.mark.parametrize("scene", ["rtiow", "rtiow_ground_in_chain", "config", "100k"])
def test_leaves_of_real_scenes(scene, test_config_text):
    """The leaves a handle would build from (rt_debug_guard_leaves): S-rtiow; S-rtiow with guard_front_primitives = -1 (the
    ground sphere is a leaf and reaches the chain); the test config scene (planes and triangles: leaf codes of type 1);
    S-100k (about 10^5 leaves)."""
    if scene == "config":
        host, cfg = rb.HostScene.from_config(test_config_text), {}
    elif scene == "100k":
        host, cfg = rb.HostScene.rtiow(half_extent=158, textured_quad=True), {}
    else:
        host, cfg = rb.HostScene.rtiow(), ({"guard_front_primitives": -1} if scene == "rtiow_ground_in_chain" else {})
    boxes, codes = guard_leaves(host, **cfg)
    info, want = check_tree(boxes, codes, scene)
    if scene == "rtiow_ground_in_chain":
        assert want["num_large"] >= 1
    if scene == "config":
        assert ((-codes.astype(np.int64) - 1) & 1).any()          # plane leaves
    if scene == "100k":
        assert len(codes) > 90000
    print(f"{scene}: {len(codes)} leaves, {want['num_large']} large, depth {info[2]}")
