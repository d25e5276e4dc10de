"""The light-sampling routines, vertex by vertex.  On the CPU: tests/light_vertex_cases.py's sets reach what they aim at —
every tally of the per-vertex restatements is met by the classes aimed at it, the tallies only count, every NaN the restatements return is
in a class DESIGN lists, no vertex is left out — and two invariants of the restatements' own numbers hold against float64: a tree's pmf
sums to 1 from every aimed point, and the light side's and the found side's MIS weights of one sample sum to 1.  On the GPU:
tests/dev_light_vertex_checks.py in one child process on the developer library — every word of every routine on every vertex against the
CPU statement, bit for bit."""
import collections
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import emit_reference as emr
import gloss_reference as glr
import light_vertex_cases as lc
import medium_reference as mr
import tree_reference as tr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T = {name: 1 << k for k, name in enumerate(glr.TALLIES)}


@pytest.fixture(scope="module", autouse=True)
def libraries():
    """The four restatements, compiled side by side."""
    with ThreadPoolExecutor(4) as pool:
        list(pool.map(lambda m: m.lib(), (emr, tr, glr, mr)))


@pytest.fixture(scope="module")
def passes():
    return lc.all_passes()


@pytest.fixture(scope="module")
def results(passes):
    """The CPU statement of every pass, computed once: (want, flags) per pass."""
    return [lc.reference(p) for p in passes]


def _classes(p):
    return p.cls if isinstance(p.cls, np.ndarray) else np.full(len(p.x), p.cls)


def test_the_sets_are_what_the_issue_lists(passes):
    assert lc.SCENES == ("lamp", "three lamps", "panel box", "night rtiow", "exact")
    kind, idx, cdf, pmf, area = emr.table(lc.scene("exact"), 1)
    d = lc.scene("exact").desc
    # the exact scene's table: three spheres, then the quad, the triangle, the ellipse and the sliver; the two planes between are skipped
    assert list(zip(kind, idx)) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (1, 4), (1, 5)]
    assert d.spheres[2].radius == 2.0 ** -10 and np.signbit(d.spheres[1].center.e[2]) and d.planes[5].v.e[1] == 2.0 ** -20
    assert area[3] == 1.0 and area[4] == 0.5 and area[6] == np.float32(2.0 ** -20)
    assert [len(lc.table_configs(s)) for s in lc.SCENES] == [2, 2, 4, 2, 4]
    assert len(emr.table(lc.scene("lamp"), 0)[0]) == 1 and tr.tree(lc.scene("lamp"))["depth"].max() == 0
    sizes = collections.defaultdict(set)
    for p in passes:
        assert len(p.x) <= lc.MAX_CALL and p.x.dtype == p.nv.dtype == p.v.dtype == p.s.dtype == np.float32 and p.seed.dtype == np.uint32
        assert np.isfinite(p.x).all() and np.isfinite(p.nv).all() and np.isfinite(p.v).all() and np.isfinite(p.s).all(), p.label
        if p.routine == 0:
            sizes[p.cls].add(len(p.x))
    assert sizes["base"] == {lc.BASE}
    for cls, s in sizes.items():
        if cls != "base":
            assert 64 <= min(s) and max(s) <= 1152, (cls, s)
    total = sum(len(p.x) for p in passes)
    print(f"{len(passes)} passes, {total} vertices; routine 0 classes: {sorted(sizes)}")
    assert 1000000 <= total <= 2000000
    rgb, params = lc.environment("two")
    assert rgb.shape == (2, 2, 3) and (rgb.sum(2) == 0).sum() == 1 and not rgb[0, 1].any()
    sun = lc.environment("sun")[0]
    assert sun.shape == (16, 16, 3) and (sun.sum(2) > 100 * np.median(sun.sum(2))).sum() == 1, "n = 16, one sun texel"
    # the seeds of the 2 x 2 map pick every neighbour of its black texel (the three others), each often, and never the black one
    for p in passes:
        if p.routine == 1 and p.env == "two" and p.pb == 0:
            want, _ = lc.reference(p)
            d = want[want[:, 0] == 1, 1:4].view(np.float32).astype(np.float64)
            q = d / np.abs(d).sum(1, keepdims=True)
            up = q[:, 1] >= 0
            u = np.where(up, q[:, 0], (1 - np.abs(q[:, 2])) * np.where(q[:, 0] >= 0, 1, -1))
            v = np.where(up, q[:, 2], (1 - np.abs(q[:, 0])) * np.where(q[:, 2] >= 0, 1, -1))
            texel = (v >= 0).astype(int) * 2 + (u >= 0).astype(int)
            counts = np.bincount(texel, minlength=4)
            print(f"{p.label}: ok samples by texel {counts}")
            assert counts[1] == 0 and (counts[[0, 2, 3]] >= 100).all(), counts
    rot = np.array(lc.environment("sun")[1]["rot"], np.float32)
    assert ((np.abs(rot) > 0.05) & (np.abs(rot) < 0.99)).all() and (rot.view(np.uint32) & 0xff != 0).all(), "all nine entries inexact: no short mantissa"


def test_tallies_only_count(passes, results):
    """Every word is the same with the tallies and without them."""
    for p, (want, flags) in zip(passes, results):
        bare, none = lc.reference(p, tallies=False)
        assert not none.any()
        assert bare.tobytes() == want.tobytes(), p.label
    assert any(flags.any() for _, flags in results)


# tally → (the classes aimed at it, the floor: vertices of those classes that reach it).  The floors are about half of what was counted
# when the sets were made (the count stands beside each; the test prints them, DESIGN.md §42 has the table), so that a change of the sets
# that loses a tally shows.
AIMED = {
    "cone refused: inside": (("sphere: x inside", "sphere: d2 == rr and neighbours"), 8000),                          # 16 704
    "om == 0": (("sphere: 2^k radii away", "tree: 1e10 sizes away", "tree: 1e20 sizes away"), 6000),                  # 11 916
    "om == 2^-24": (("sphere: 2^k radii away",), 1400),                                                               # 2 884
    "hemisphere refused": (("hemisphere: dot(dir, n) == 0 and neighbours", "hemisphere: n = -dir"), 20000),           # 28 672 and every n = -dir
    "pb == 0 refused": (("base",), 12000),                                                                            # 24 926
    "fallback taken": (("tree: 1e20 sizes away", "tree: every entry from every point"), 2800),                        # 5 728
    "triangle folded": (("base", "plane: triangle ua + ub about 1"), 2500),                                           # 4 516 and the folds of the aimed seeds
    "triangle: ua + ub == 1": (("plane: triangle ua + ub about 1",), 144),                                            # 288
    "no entry": (("table: cdf entries and every code", "tree: every entry from every point", "env: seeds"), 400),     # 817
    "pl^2 overflows": (("tree: 1e10 sizes away", "found: ok samples fed back, and every primitive"), 220),            # 446
    "plane refused: cos_l < 1e-8": (("plane: x in the plane", "plane: cos_l about 1e-8", "plane: x at a corner"), 4200),          # 8 532
    "ellipse loop >= 4 rounds": (("plane: ellipse loop >= 4 rounds",), 2000),                                         # 4 096
    "found: weighted": (("found: ok samples fed back, and every primitive", "found: ok samples of the environment fed back", "env: folds, edges and axes"), 80000),    # 167 625
    "found: pl == 0": (("found: ok samples fed back, and every primitive", "env: folds, edges and axes"), 4000),      # 8 272
    "found: not a table entry": (("found: ok samples fed back, and every primitive",), 9000),                         # 18 683
    "found: carry off": (("found: ok samples fed back, and every primitive", "found: ok samples of the environment fed back", "env: folds, edges and axes"), 26000),   # 53 246
    "basis: wn.z == +-0": (("sphere: wn.z == +-0", "sphere: w along an axis"), 24000),                                # 48 816
    "basis: wn.x == wn.y == 0": (("sphere: w along an axis",), 5500),                                                 # 11 008
    "ok": (("base",), 100000),                                                                                        # 201 658
}
UNREACHED = ("plane refused: the point is the vertex",)          # DESIGN.md §42, "what is unreachable": ua and ub would have to name x itself


def test_the_sets_reach_every_tally(passes, results):
    count = collections.defaultdict(collections.Counter)          # tally → class → vertices
    for p, (want, flags) in zip(passes, results):
        cls = _classes(p)
        for name, bit in T.items():
            hit = (flags & np.uint32(bit)) != 0
            if hit.any():
                for c, k in zip(*np.unique(cls[hit], return_counts=True)):
                    count[name][str(c)] += int(k)
    for name in glr.TALLIES:
        print(f"tally {name}: {sum(count[name].values())} vertices; " + ", ".join(f"{c}: {k}" for c, k in count[name].most_common(6)))
    for name in UNREACHED:
        assert not count[name], "a set reaches what DESIGN calls unreachable: say so there"
    assert set(AIMED) | set(UNREACHED) | {"a NaN in c"} == set(glr.TALLIES)
    for name, (classes, floor) in AIMED.items():
        got = sum(count[name][c] for c in classes)
        assert got >= floor, (name, classes, got, floor)


# the classes in which a restatement returns a NaN, and the expression that makes it
NAN_CLASSES = {
    "found: ok samples fed back, and every primitive",          # a denormal carry: pb * pb == 0 over pl == 0 is 0 / 0
    "env: folds, edges and axes",                               # the same on a miss into the texel of weight 0 (pl == 0)
}


def test_nans_are_where_design_says_and_no_vertex_is_left_out(passes, results):
    nan = collections.Counter()
    vertices = words = 0
    for p, (want, flags) in zip(passes, results):
        assert want.shape == (len(p.x), 16) and flags.shape == (len(p.x),)          # a row for every vertex: none is left out
        cols = lc.COLUMNS[p.routine]
        assert not want[:, len(cols):].any(), p.label
        vertices += len(p.x)
        words += len(p.x) * len(cols)
        f = want[:, list(lc.FLOAT_COLUMNS[p.routine])].view(np.float32)
        bad = np.isnan(f).any(1)
        if bad.any():
            for c, k in zip(*np.unique(_classes(p)[bad], return_counts=True)):
                nan[str(c)] += int(k)
    print(f"{vertices} vertices, {words} words; vertices with a NaN by class: {dict(nan)}")
    assert set(nan) <= NAN_CLASSES, set(nan) - NAN_CLASSES


def test_tree_pmf_sums_to_one():
    """Invariant 1: from every aimed point, the sum of tree_pmf over a tree's entries is 1 within 3 D 2^-24 (D: the tree's depth) — DESIGN.md
    §42 has the derivation: one rounded 1 - pl per level (exact for pl >= 1/2, within 2^-25 below) and one rounded product."""
    worst = {}
    for name in lc.SCENES:
        for planes, select in lc.table_configs(name):
            if not select:
                continue
            depth = int(tr.tree(lc.scene(name), planes)["depth"].max())
            X = np.concatenate(list(lc.tree_points(name, planes).values()) + [lc.base_set(name).x[:256]])
            pmf = tr.pmf(lc.scene(name), X, planes).astype(np.float64)
            assert np.isfinite(pmf).all() and (pmf >= 0).all()
            dev = np.abs(pmf.sum(1) - 1)
            worst[name, planes] = (float(dev.max()), depth)
            assert dev.max() <= 3 * depth * 2.0 ** -24, (name, planes, float(dev.max()), depth)
    for (name, planes), (w, depth) in worst.items():
        print(f"tree of {name}, planes={planes}: depth {depth}, largest |sum - 1| = {w:.3e} = {w * 2 ** 24:.2f} x 2^-24 (bound {3 * depth} x 2^-24)")
    assert worst["lamp", 0] == (0.0, 0)


# Invariant 2's exemption: a plane's found side takes d2 and cos_l from the hit point x + t dir, the light side from the
# sampled point y — two roundings of one geometry, not two definitions of pl.  wl + wb - 1 = pb^2 (pl^2 - pl'^2) / ((pl^2 + pb^2)
# (pl'^2 + pb^2)), at most half the relative difference of pl and pl'; that difference is the rounding of the hit point and of y (a unit
# roundoff of |x| + |point| each, against the length |w| of point - x) carried into cos_l = |n . w| / |w|, where it is divided by cos_l.
# So a plane sample is held to 8 x 2^-24 x (1 + (|x| + |point|) / (|w| cos_l)), all in float64 from the geometry.
def plane_bound(x, point, normal):
    w = point - x
    lw = np.linalg.norm(w, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_l = np.abs((w * normal).sum(1)) / lw
        bound = 8 * 2.0 ** -24 * (1 + (np.linalg.norm(x, axis=1) + np.linalg.norm(point, axis=1)) / (lw * cos_l))
    return bound          # (NaN or inf where x lies in the emitter's plane in float64 — t = 0, cos_l = 0: the test counts those)


# … and the environment: the light side takes q2 and q from the sampled octahedron point p, the found side from
# p' = d / |d|_1 of d = to_env(rot we) — the same point after two rotations (each component a 3-term dot product: 3 u of |v|, 3 sqrt(3) u
# as a vector), the L1 sum (3 u) and the division (1 u), u = 2^-24: |p'| is |p| within about 15 u.  pl goes with |p|^3, so the two pl differ
# by at most 45 u plus the roundings of q2, q and the products on either side (6 u each): 57 u, and wl + wb - 1 is at most half of that.
ENV_BOUND = 32 * 2.0 ** -24
# plane samples that are ok on the light side although x lies in the emitter's plane in float64 (its float32 cos_l is rounding noise of
# 1e-8 or more): they have no bound, and their number is pinned so that none joins them unseen
IN_PLANE = 25


def test_light_and_found_weights_sum_to_one():
    """Invariant 2: for every ok sample under the power heuristic, wl = pl^2 / (pl^2 + pb^2) from the light side's densities and
    wb = pb^2 / (pb^2 + pl'^2) from the found side's at the same (x, dir, code), both in float64 from the restatement's own float32 pl and
    pb, sum to 1 within 4 x 2^-24.  For a sphere the two pl are the same float (the descent's product is the path product bit for bit); for
    a plane they differ by the rounding of the hit point, and plane_bound holds each sample; for the environment (routine 1 against routine
    3 at the sampled direction) by the two rotations in between, and ENV_BOUND holds them."""
    worst = collections.defaultdict(float)
    n = collections.Counter()
    left_out = unbounded = one_sided = 0
    for name in lc.SCENES:
        for planes, select in lc.table_configs(name):
            for pb in (0, 1):
                for vs in lc.sample_sets(name, planes, select):
                    v, s = lc._vs_of(vs, pb, name)
                    p = lc.Pass("", name, vs.name, 0, pb, select, planes, 1, None, None, vs.x, vs.nv, v, s, vs.seed)
                    want, flags, d = lc.reference(p, densities=True)
                    ok = (want[:, 0] == 1) & np.isfinite(d).all(1)
                    left_out += int(((want[:, 0] == 1) & ~ok).sum())
                    if not ok.any():
                        continue
                    x, dirs, code = vs.x[ok], want[ok, 1:4].view(np.float32), want[ok, 7]
                    nv = np.zeros((len(x), 3), np.float32)
                    nv[:, 0] = d[ok, 1]
                    back = lc.Pass("", name, vs.name, 2, 0, select, planes, 1, None, None, x, nv, dirs, lc.closest_of(name, x, dirs, code), code)
                    _, fflags, fd = lc.reference(back, densities=True)
                    assert ((fflags & T["found: weighted"]) != 0).all(), (name, vs.name)
                    pl, pbv, pl2 = d[ok, 0].astype(np.float64), d[ok, 1].astype(np.float64), fd[:, 0].astype(np.float64)
                    # (found_hit_weight's note holds the last pass's pb, the diffuse constant: the carried one is the light side's pb itself)
                    wl = pl * pl / (pl * pl + pbv * pbv)
                    wb = pbv * pbv / (pbv * pbv + pl2 * pl2)
                    dev = np.abs(wl + wb - 1)
                    plane = (code & 1) != 0
                    for kind, sel in (("sphere", ~plane), ("plane", plane)):
                        if sel.any():
                            worst[kind] = max(worst[kind], float(dev[sel].max()))
                            n[kind] += int(sel.sum())
                    assert dev[~plane].max(initial=0) <= 4 * 2.0 ** -24, (name, planes, select, pb, vs.name, float(dev[~plane].max()))
                    if plane.any():
                        t = lc.closest_of(name, x[plane], dirs[plane], code[plane]).astype(np.float64)
                        x64 = x[plane].astype(np.float64)
                        d = lc.scene(name).desc
                        normal = np.array([d.planes[int(c) >> 1].normal.e[:] for c in code[plane]], np.float64)
                        bound = plane_bound(x64, x64 + t[:, None] * dirs[plane].astype(np.float64), normal)
                        unbounded += int((~np.isfinite(bound)).sum())
                        bound = np.where(np.isnan(bound), np.inf, bound)
                        one_sided += int((pl2[plane] == 0).sum())
                        both = plane & (pl2 != 0)
                        worst["plane, both sides sample"] = max(worst["plane, both sides sample"], float(dev[both].max(initial=0)))
                        ratio = dev[plane] / bound
                        worst["plane, of its bound"] = max(worst["plane, of its bound"], float(ratio.max()))
                        assert ratio.max() <= 1, (name, planes, select, pb, vs.name, float(ratio.max()), float(dev[plane].max()))
    for kind in ("sphere", "plane"):
        print(f"|wl + wb - 1| on {n[kind]} {kind} samples: at most {worst[kind]:.3e} = {worst[kind] * 2 ** 24:.2f} x 2^-24")
    print(f"a plane sample's deviation is at most {worst['plane, of its bound']:.3f} of its bound; {left_out} ok samples have an infinite pl and no weight in float64")
    print(f"plane samples whose found side refuses (pl' = 0, deviation 1): {one_sided}; the largest deviation where both sides sample: "
          f"{worst['plane, both sides sample']:.3e} = {worst['plane, both sides sample'] * 2 ** 24:.1f} x 2^-24; samples without a bound: {unbounded}")
    assert n["sphere"] > 50000 and n["plane"] > 10000 and left_out == 0 and unbounded == IN_PLANE
    # the environment: every ok sample of routine 1 under the power heuristic against routine 3 at the direction it returned
    for p in lc.env_passes():
        if p.routine != 1 or p.env_params["mode"] != 1 or p.pb == 2:
            continue
        want, flags, d = lc.reference(p, densities=True)
        ok = want[:, 0] == 1
        assert np.isfinite(d[ok]).all() and (d[ok] > 0).all(), p.label
        dirs = want[ok, 1:4].view(np.float32)
        m = len(dirs)
        nv = np.zeros((m, 3), np.float32)
        nv[:, 0] = d[ok, 1]
        back = lc.Pass("", "lamp", "", 3, 0, 0, 0, 1, p.env, dict(p.env_params, camera_visible=1), np.zeros((m, 3), np.float32), nv, dirs, np.zeros(m, np.float32),
                       np.zeros(m, np.uint32))
        _, fflags, fd = lc.reference(back, densities=True)
        assert ((fflags & T["found: weighted"]) != 0).all(), p.label
        pl, pbv, pl2 = d[ok, 0].astype(np.float64), d[ok, 1].astype(np.float64), fd[:, 0].astype(np.float64)
        dev = np.abs(pl * pl / (pl * pl + pbv * pbv) + pbv * pbv / (pbv * pbv + pl2 * pl2) - 1)
        rel = np.abs(pl2 - pl) / pl
        print(f"{p.label}: |wl + wb - 1| on {m} samples at most {dev.max() * 2 ** 24:.2f} x 2^-24; the two pl differ by at most {rel.max() * 2 ** 24:.1f} x 2^-24 of pl")
        assert m > 1000 and dev.max() <= ENV_BOUND and rel.max() <= 57 * 2.0 ** -24, (p.label, float(dev.max()), float(rel.max()))


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_light_routines_equal_the_restatements_vertex_by_vertex_on_gfx950():
    """tests/dev_light_vertex_checks.py in one child process that loads the developer library (rt_debug_light_vertices): every word of every
    routine on every vertex of light_vertex_cases compared as uint32 with the CPU statement.  The child's LIGHT VERTICES lines give the hook
    calls, the vertices, the words and the device time."""
    from conftest import run_child
    dev_lib = os.path.join(ROOT, "ray-tracing-practice_amd", "librtp_amd_dev.so")
    assert os.path.exists(dev_lib), "run __graft_entry__.build() (make -C ray-tracing-practice_amd dev)"
    env = dict(os.environ, RTP_AMD_LIB=dev_lib)
    res = run_child([sys.executable, "-m", "pytest", os.path.join(HERE, "dev_light_vertex_checks.py"), "-x", "-q", "-s", "-p", "no:cacheprovider"], 120, env=env)
    print(res.stdout[-6000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "3 passed" in res.stdout and "failed" not in res.stdout and "skipped" not in res.stdout
