"""rt_render_glow_sampled / rt_trace_samples_glow_sampled and rt_glow_sampler (include/rtp_amd.h, "light samples of the glow"; DESIGN.md
§36): the glowing medium as a light a vertex can aim at.  The contract's restatement is tests/cpu_native/glow_sample_ref.c
(tests/glow_sample_reference.py); the CPU tests check the restatement, the table and the ABI, the GPU tests the kernels and the table
against the restatement, bit for bit.  Scenes, settings and protocols are tests/test_medium.py's, tests/test_volume.py's and
tests/test_glow.py's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import glow_reference as gr
import glow_sample_reference as gs
import medium_reference as mr
import rtp_bindings as rb
from test_glow import FURNACE_A, FURNACE_B, GLOWS, HEATS, _grid_file
from test_lit import assert_same
from test_medium import ENV_MIS, _channel_z, _fog_ball_scene, all_ijs, scenes, sun_map
from test_nee_planes import LUM, MAT_LAMBERTIAN, QUAD, material
from test_volume import GRIDS, fog, random_grid, special_camera

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
INVALID = 1
COLUMNS = ("radiance", "rays", "events", "ends", "seeds", "cells", "glow_length", "glow_samples")
Z_BOUND = 4.5          # the project's bound on a z score
UNIT_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


# ---- no GPU needed: the ABI and the refusals -----------------------------------------------------------------------------------------------

def test_abi_and_defaults():
    lib = rb.amd_lib()
    for s in ("rt_glow_sample_params_init", "rt_glow_sampler_create", "rt_glow_sampler_destroy", "rt_glow_sampler_table", "rt_render_glow_sampled",
              "rt_trace_samples_glow_sampled"):
        assert hasattr(lib, s) and s in rb.RTP_AMD_SYMBOLS, s
    assert len(lib.rt_render_glow_sampled.argtypes) == 15 and len(lib.rt_trace_samples_glow_sampled.argtypes) == 21
    assert len(lib.rt_glow_sampler_create.argtypes) == 4 and len(lib.rt_glow_sampler_table.argtypes) == 8
    for name in ("render_glow_sampled", "render_glow_sampled_to_host", "trace_samples_glow_sampled"):
        assert hasattr(rb.DeviceScene, name)
    assert hasattr(rb, "GlowSampler")
    assert C.sizeof(rb.GlowSampleParams) == 12
    assert [rb.GlowSampleParams.__dict__[f].offset for f in ("struct_bytes", "sample", "mis")] == [0, 4, 8]
    p = rb.glow_sample_params()
    assert p.struct_bytes == 12 and p.sample == 0 and p.mis == 1
    q = rb.glow_sample_params(sample=1, mis=0)
    assert q.sample == 1 and q.mis == 0
    lib.rt_glow_sample_params_init(None)


def _calls(cam, lit, medium, volume, glow, heat, sample, sampler):
    """(status, message) of rt_render_glow_sampled and of rt_trace_samples_glow_sampled with a null scene."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    ijs = (C.c_int32 * 3)(0, 0, 0)
    f = (C.c_float * 3)()
    r = (C.c_int32 * 1)()
    s = (C.c_uint32 * 1)()
    ref = lambda x: C.byref(x) if x is not None else None          # noqa: E731
    out = [lib.rt_render_glow_sampled(None, C.byref(cam), ref(lit), ref(medium), volume, ref(glow), heat, ref(sample), sampler, None, 0, C.c_void_p(1 << 32),
                                      None, 1, None), lib.rt_get_last_error_string().decode()]
    out += [lib.rt_trace_samples_glow_sampled(None, C.byref(cam), ref(lit), ref(medium), volume, ref(glow), heat, ref(sample), sampler, 1, ijs, f, r, r, s, s, s,
                                              s, r, f, r), lib.rt_get_last_error_string().decode()]
    return out


def test_refusals_before_the_scene_is_looked_at():
    """rt_render_glow's refusals first, then the sample's in the header's order, all with a null scene and handles that are never read (the
    refusals that read the sampler are test_sampler_mismatch_and_devices' on the GPU).  Each case also breaks every LATER rule it can, so
    the word it is refused with shows the order.  What passes reaches the null-scene check.  Every message names the sampled call."""
    cam = rb.rtiow_camera(8, 4, 2)
    handle = C.c_void_p(1 << 32)
    box = dict(box=(0, 0, 0, 1, 1, 1))
    good = rb.medium_params(sigma_t=1.0, **box)

    def refused(word, medium=good, lit=None, volume=handle, glow=None, heat=None, sample=None, sampler=None):
        st1, m1, st2, m2 = _calls(cam, lit, medium, volume, glow, heat, sample, sampler)
        assert st1 == INVALID and word in m1 and "rt_render_glow_sampled" in m1, (word, m1)
        assert st2 == INVALID and word in m2 and "rt_trace_samples_glow_sampled" in m2, (word, m2)
    bad = rb.glow_sample_params(sample=2, mis=2)
    bad.struct_bytes = 4
    # rt_render_glow's come first: the lit call's, the medium's, the volume's, the glow's
    refused("mis", lit=rb.lit_params(nee=dict(mis=2)), medium=rb.medium_params(sigma_t=-1.0), glow=rb.glow_params(radiance=-1), sample=bad, volume=None)
    refused("sigma_t must", medium=rb.medium_params(sigma_t=-1.0, **box), glow=rb.glow_params(radiance=-1), sample=bad, volume=None)
    refused("region 2", medium=rb.medium_params(sigma_t=1.0), glow=rb.glow_params(radiance=-1), sample=bad)
    refused("source must", glow=rb.glow_params(radiance=-1, source=3), sample=bad, volume=None)
    refused("radiance", glow=rb.glow_params(radiance=(1, -1, 1)), sample=bad, volume=None)
    refused("needs a heat grid", glow=rb.glow_params(radiance=1, source=2), sample=bad)
    # the sample's own, in order: struct_bytes, sample, mis, the volume, the sampler
    glow = rb.glow_params(radiance=1.0)
    refused("rt_glow_sample_params", glow=glow, sample=bad, volume=None)
    for v in (-1, 2):
        refused("sample must", glow=glow, sample=rb.glow_sample_params(sample=v, mis=2), volume=None)
        refused("mis must", glow=glow, sample=rb.glow_sample_params(sample=1, mis=v), volume=None)
    st = _calls(cam, None, good, None, glow, None, rb.glow_sample_params(sample=1), None)
    refused("need a volume", glow=glow, sample=rb.glow_sample_params(sample=1), volume=None)
    assert "1 x 1 x 1" in st[1] and "1 x 1 x 1" in st[3], st
    refused("needs a sampler", glow=glow, sample=rb.glow_sample_params(sample=1, mis=0))
    # what passes reaches the scene: no sample at all, sample 0 (a sampler is not read), under any mis
    for sample, sampler in ((None, None), (rb.glow_sample_params(), None), (rb.glow_sample_params(sample=0, mis=0), handle), (None, handle)):
        for volume in (handle, None):
            st1, m1, st2, m2 = _calls(cam, None, good, volume, glow, None, sample, sampler)
            assert st1 == INVALID and "rt_render_glow_sampled: null scene" in m1, m1
            assert st2 == INVALID and "rt_trace_samples_glow_sampled: null scene" in m2, m2


def test_cli_refusals(test_config_text, tmp_path):
    """rtp_main --fog-glow-sample needs --fog-glow and --fog-grid, and takes mis or light: each refusal says why."""
    grid = _grid_file(tmp_path / "g.vol", GRIDS["2x3x5"])
    fogged = ["--lit", "--fog", "0.4", "--fog-box", "-3,-3,-3,3,3,3"]
    for extra, word in ((fogged + ["--fog-grid", grid, "--fog-glow-sample", "mis"], "needs --fog-glow R,G,B"),
                        (fogged + ["--fog-glow", "1,1,1", "--fog-glow-sample", "mis"], "needs --fog-grid FILE"),
                        (fogged + ["--fog-grid", grid, "--fog-glow", "1,1,1", "--fog-glow-sample", "both"], "mis or light"),
                        (fogged + ["--fog-grid", grid, "--fog-glow", "1,1,1", "--fog-glow-sample"], "mis or light")):
        res = subprocess.run([EXE, "--gpu"] + extra, input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert res.returncode == 99 and word in res.stderr and "--fog-glow-sample" in res.stderr, (extra, res.returncode, res.stderr[-300:])


# ---- the table -------------------------------------------------------------------------------------------------------------------------------

def _f32(x):
    return np.float32(x)


def test_table_hand_computed():
    """2 x 2 x 2 grids whose cdfs are written out by hand (float64 sums, each entry the float32 of running / total, the last 1.0f), pc the
    float32 products of the float32 differences; an empty slab and an empty row have all-zero cdfs and are skipped by their parents' cdf;
    all-zero heat is an empty sampler; source 0 is uniform."""
    h = np.array([[[1, 3], [2, 2]], [[0, 0], [4, 4]]], np.float32)          # [z][y][x]: slab sums 8 and 8, slab 1 has an empty row
    t = gs.table(np.ones_like(h), source=2, heat=h)
    assert not t["empty"]
    assert_same(t["slab_cdf"], np.float32([0.5, 1.0]), "slab cdf")
    assert_same(t["row_cdf"], np.float32([[0.5, 1.0], [0.0, 1.0]]), "row cdfs")
    assert_same(t["cell_cdf"], np.float32([[[0.25, 1.0], [0.5, 1.0]], [[0.0, 0.0], [0.5, 1.0]]]), "cell cdfs")
    assert_same(t["pc"], np.float32([[[1, 3], [2, 2]], [[0, 0], [4, 4]]]) / np.float32(16), "pc")
    # thirds do not round to themselves: every entry is the float32 of the float64 quotient, every pc the float32 products in order
    h = np.array([[[1, 2], [0, 0]], [[0, 0], [0, 0]]], np.float32)          # one row in one slab: an empty slab, an empty row
    t = gs.table(h, source=1)
    third = _f32(1.0 / 3.0)
    assert_same(t["slab_cdf"], np.float32([1.0, 1.0]), "slab cdf, an empty slab")
    assert_same(t["row_cdf"], np.float32([[1.0, 1.0], [0.0, 0.0]]), "row cdfs, an empty slab")
    assert_same(t["cell_cdf"], np.float32([[[third, 1.0], [0, 0]], [[0, 0], [0, 0]]]), "cell cdfs, empty rows")
    want = np.zeros((2, 2, 2), np.float32)
    want[0, 0] = [(_f32(1) * _f32(1)) * third, (_f32(1) * _f32(1)) * (_f32(1) - third)]
    assert_same(t["pc"], want, "pc, one row")
    assert not t["empty"] and t["pc"].sum() == 1.0
    # a first slab that is empty: the pick (the smallest e with u < cdf[e]) can never land in it
    h = np.array([[[0, 0], [0, 0]], [[5, 0], [0, 7]]], np.float32)
    t = gs.table(np.ones_like(h), source=2, heat=h)
    assert_same(t["slab_cdf"], np.float32([0.0, 1.0]), "slab cdf, the first slab empty")
    assert_same(t["row_cdf"][1], np.float32([_f32(5.0 / 12.0), 1.0]), "row cdf")
    assert_same(t["cell_cdf"][1], np.float32([[1.0, 1.0], [0.0, 1.0]]), "cell cdfs")
    assert not t["pc"][0].any() and t["pc"][1, 0, 1] == 0 and t["pc"][1, 1, 0] == 0
    # all zero: empty, everything zero
    t = gs.table(np.ones((2, 2, 2), np.float32), source=2, heat=np.zeros((2, 2, 2), np.float32))
    assert t["empty"] and not any(t[k].any() for k in ("slab_cdf", "row_cdf", "cell_cdf", "pc"))
    # source 0: uniform, whatever the density
    t = gs.table(GRIDS["2x3x5"], source=0)
    assert not t["empty"] and (t["pc"] > 0).all() and abs(float(t["pc"].astype(np.float64).sum()) - 1.0) < 1e-6
    assert_same(t["slab_cdf"], np.float32([0.2, 0.4, 0.6, 0.8, 1.0]), "uniform slabs")


PICK_DRAWS = 200000


def test_cell_pick_follows_pc():
    """On a 3 x 4 x 5 grid with a third of the cells at h == 0: the picked cells of PICK_DRAWS light samples follow pc — Pearson's chi-square
    over the cells with pc > 0, as a z score (chi2 - dof) / sqrt(2 dof) within the project's bound — and a cell with h == 0 is never picked."""
    heat = random_grid((5, 4, 3), 77)
    assert (heat == 0).sum() >= 10 and (heat > 0).sum() >= 30
    medium = dict(sigma_t=1.0, box=UNIT_BOX)
    cell, taken, dirs, pls = gs.draws(medium, np.ones_like(heat), (3.0, 0.5, 0.25), 12345, PICK_DRAWS, source=2, heat=heat)
    assert (cell >= 0).all() and taken.all()
    counts = np.zeros(heat.shape, np.int64)
    np.add.at(counts, (cell[:, 2], cell[:, 1], cell[:, 0]), 1)
    assert not counts[heat == 0].any()
    pc = gs.table(np.ones_like(heat), source=2, heat=heat)["pc"].astype(np.float64)
    hot = pc > 0
    assert (hot == (heat > 0)).all()
    expected = PICK_DRAWS * pc[hot]
    chi2 = (((counts[hot] - expected) ** 2) / expected).sum()
    dof = hot.sum() - 1
    z = (chi2 - dof) / np.sqrt(2.0 * dof)
    print(f"chi2 {chi2:.1f} dof {dof} z {z:+.2f} smallest expected count {expected.min():.0f}")
    assert expected.min() > 50 and abs(z) <= Z_BOUND, z


def _uniform_directions(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


PL_POINTS = {"outside": (2.5, 0.4, -0.3), "inside a hot cell": (0.3, 0.3, 0.3), "on a face": (1.0, 0.2, -0.4)}


@pytest.mark.parametrize("where", list(PL_POINTS))
def test_pl_integrates_to_one(where):
    """glow_pl is a density over the sphere of directions: the mean of 4 pi pl over 65 536 uniform directions is 1 within |z| <= 4.5 of its own
    standard error — from outside the box, from inside a hot cell and from a point on a face.  From inside a hot cell every direction has
    pl > 0, so the mean of 1 / pl over directions drawn BY the sample is the sphere's 4 pi."""
    heat = random_grid((4, 4, 4), 78)
    heat[2, 2, 2] = 1.5          # the cell of (0.3, 0.3, 0.3) in (-1, 1)^3
    medium = dict(sigma_t=1.0, box=UNIT_BOX)
    x = np.float32(PL_POINTS[where])
    d = _uniform_directions(65536, 5)
    pl, _ = gs.pl(medium, np.ones_like(heat), np.broadcast_to(x, d.shape), d, source=2, heat=heat)
    v = 4.0 * np.pi * pl.astype(np.float64)
    z = (v.mean() - 1.0) / (v.std(ddof=1) / np.sqrt(len(v)))
    print(f"{where}: mean 4 pi pl {v.mean():.5f} z {z:+.2f} share of directions with pl > 0 {(pl > 0).mean():.3f}")
    assert abs(z) <= Z_BOUND, z
    if where == "inside a hot cell":
        assert (pl > 0).all()
        cell, taken, dirs, pls = gs.draws(medium, np.ones_like(heat), x, 999, 65536, source=2, heat=heat)
        assert taken.all()
        w = 1.0 / pls.astype(np.float64)
        z = (w.mean() - 4.0 * np.pi) / (w.std(ddof=1) / np.sqrt(len(w)))
        print(f"mean 1 / pl {w.mean():.4f} (4 pi = {4 * np.pi:.4f}) z {z:+.2f}")
        assert abs(z) <= Z_BOUND, z
        # and the density the sample reports is glow_pl of its direction
        again, _ = gs.pl(medium, np.ones_like(heat), np.broadcast_to(x, dirs.shape), dirs, source=2, heat=heat)
        assert_same(again, pls, "pl of the sampled directions")


# the worst relative differences of the float32 quantities from their float64 sums over the same cells, measured on this restatement over
# _f64_rays of both grids and the three extinctions (printed by the test), and the tolerances: four times those
PL_MEASURED, LINE_MEASURED = 4.0e-7, 2.1e-6
PL_TOL, LINE_TOL = 4 * PL_MEASURED, 4 * LINE_MEASURED
# the share of a walk's cells on the closed-form side of the threshold that each extinction has to reach (lowest, highest)
SERIES_SHARE = {0.05: (0.0, 0.1), 1.5: (0.1, 0.9), 40.0: (0.5, 1.0)}
F64_GRIDS = {"16": (16, 16, 16), "1x1x64": (64, 1, 1)}


@functools.lru_cache(maxsize=None)
def _f64_rays(name):
    """Rays through (-1, 1)^3: origins outside aimed at points inside, origins inside with any direction, and both with one direction
    component exactly 0; t_end infinite for half and finite for the rest; directions of any length."""
    rng = np.random.default_rng(len(name))
    m = 600
    inside = rng.uniform(-0.98, 0.98, (m, 3))
    outside = rng.uniform(-4, 4, (m, 3))
    outside[np.abs(outside).max(1) < 1.05] *= 4.0
    o = np.concatenate([outside, inside])
    d = np.concatenate([rng.uniform(-0.98, 0.98, (m, 3)) - outside, rng.normal(size=(m, 3))])
    d[::7, rng.integers(0, 3)] = 0.0
    d *= rng.uniform(0.2, 3.0, (2 * m, 1))
    t_end = np.where(rng.random(2 * m) < 0.5, np.inf, rng.uniform(0.1, 3.0, 2 * m))
    return o.astype(np.float32), d.astype(np.float32), t_end.astype(np.float32)


@pytest.mark.parametrize("sigma", [0.05, 1.5, 40.0])
@pytest.mark.parametrize("name", list(F64_GRIDS))
def test_pl_and_line_against_float64(name, sigma):
    """glow_pl and glow_line in the contract's float32 order against the same sums over the same cells in float64 (glow_line's with expm1 and
    exp, no series): the relative difference stays within four times the worst one measured.  The extinctions put x = sigma_c * seg on both
    sides of the series' threshold 0.0625, counted by the restatement over the cells these walks visit: at 0.05 nearly every cell takes the
    series, at 40 most take the closed form (a third of the cells are empty, x = 0), at 1.5 both branches carry a real share."""
    shape = F64_GRIDS[name]
    density, heat = random_grid(shape, 201), random_grid(shape, 202)
    medium = dict(sigma_t=sigma, box=UNIT_BOX)
    o, d, t_end = _f64_rays(name)
    pl, pl_d = gs.pl(medium, density, o, d, source=2, heat=heat)
    G, G_d, series, closed = gs.line(medium, density, o, d, t_end, source=2, heat=heat)
    share = closed / float(series + closed)
    print(f"{name} sigma {sigma}: {series + closed} cells, {share:.3f} of them with x >= 0.0625")
    assert series + closed > 5000 and SERIES_SHARE[sigma][0] <= share <= SERIES_SHARE[sigma][1], share
    hit = pl_d > 0
    assert hit.sum() > 300 and (pl[~hit] == 0).all() and ((G_d > 0).sum() > 300) and (G[G_d == 0] == 0).all()
    rel_pl = np.abs(pl[hit] - pl_d[hit]) / pl_d[hit]
    lit = G_d > 0
    rel_G = np.abs(G[lit] - G_d[lit]) / G_d[lit]
    print(f"{name} sigma {sigma}: worst relative difference pl {rel_pl.max():.3e} line {rel_G.max():.3e}")
    assert rel_pl.max() <= PL_TOL and rel_G.max() <= LINE_TOL


# ---- the handovers and the estimator, on the restatement ----------------------------------------------------------------------------------------

def _setting(k):
    """(restatement keywords, device keywords without the env object) of combination k: glossy, emitters, environment."""
    glossy, emitters, env = k & 1, (k >> 1) & 1, (k >> 2) & 1
    ref = dict(glossy=glossy, emitters=bool(emitters))
    dev = dict(nee=dict(glossy=glossy), emitters=bool(emitters))
    if env:
        ref.update(glossy_env=glossy, rgb=sun_map(), env_params=ENV_MIS)
        dev.update(env="sun", env_params=dict(glossy=glossy, **ENV_MIS))
    return ref, dev


def test_handovers_on_the_restatement():
    """sample off, an empty table (all-zero heat) and radiance 0, 0, 0 are glow_reference's call in every column and in whole frames, with
    glow_samples 0; max_depth = 1 under mis and light is glow_reference's radiance, rays and streams, with no sample taken."""
    host, camera, _ = scenes()["fuzz planes"]
    w, h, spp = 12, 8, 2
    ijs = all_ijs(w, h, spp)
    density, heat = GRIDS["2x3x5"], HEATS["2x3x5"]
    for k in range(8):
        ref, _ = _setting(k)
        cam = camera(w, h, spp, 12)
        medium = fog((0.0, 0.7, -0.95)[k % 3])
        radiance = GLOWS[k % 3]
        for what, kw, skw in (("sample off", dict(radiance=radiance, source=2, heat=heat), dict(sample=None)),
                              ("an empty table", dict(radiance=radiance, source=2, heat=np.zeros_like(heat)), dict(sample="mis")),
                              ("no glow", dict(radiance=0.0, source=1), dict(sample="light"))):
            want = gr.trace(host, cam, ijs, medium=medium, density=density, **kw, **ref)
            got = gs.trace(host, cam, ijs, medium=medium, density=density, **kw, **skw, **ref)
            for a, b, col in zip(got, want, COLUMNS):
                assert_same(a, b, f"setting {k} / {what}: {col}")
            assert not got[7].any()
            assert_same(gs.frame(host, cam, medium=medium, density=density, **kw, **skw, **ref), gr.frame(host, cam, medium=medium, density=density, **kw, **ref),
                        f"setting {k} / {what}: frame")
        cam1 = camera(w, h, spp, 1)
        want = gr.trace(host, cam1, ijs, medium=medium, density=density, radiance=radiance, source=2, heat=heat, **ref)
        for sample in ("mis", "light"):
            got = gs.trace(host, cam1, ijs, medium=medium, density=density, radiance=radiance, source=2, heat=heat, sample=sample, **ref)
            for j in (0, 1, 2, 3, 4, 5, 6):
                assert_same(got[j], want[j], f"setting {k} / max_depth 1 / {sample}: {COLUMNS[j]}")
            assert not got[7].any() and (want[6] > 0).any()


@pytest.mark.parametrize("g", [0.0, 0.7])
def test_grey_body_furnace(g):
    """tests/test_glow.py's furnace over a 4^3 grid of density 1: a box of optical width 2, albedo (0.3, 0.6, 0.9), under a background B,
    emitting sigma_t (1 - a_k) B_k — the radiance is B everywhere.  First the unsampled estimator on this grid: at most 0.1 % of the samples
    are cut by depth, and its mean is B.  Then sample = 1 under mis and light: the same cap, and the mean is B_k within |z| <= 4.5."""
    host = _fog_ball_scene()
    cam = rb.make_camera(16, 16, 20.0, (0, 1, 8), (0, 0, 0), FURNACE_B, 16, 200)
    ijs = all_ijs(16, 16, 16)
    sigma_t = 1.0
    radiance = tuple(float(np.float32(sigma_t) * (np.float32(1.0) - np.float32(a)) * np.float32(b)) for a, b in zip(FURNACE_A, FURNACE_B))
    medium = dict(sigma_t=sigma_t, albedo=FURNACE_A, g=g, box=UNIT_BOX)
    density = np.ones((4, 4, 4), np.float32)
    for sample in (None, "mis", "light"):
        rad, rays, events, ends, seeds, cells, length, shots = gs.trace(host, cam, ijs, medium=medium, density=density, radiance=radiance, source=1, sample=sample,
                                                                        emitters=False)
        assert (ends == mr.END_DEPTH).mean() <= 0.001, (sample, (ends == mr.END_DEPTH).mean())
        assert events.max() >= 3 and (events > 0).mean() > 0.1
        assert ((shots > 0).mean() > 0.05) if sample else not shots.any()
        x = rad.astype(np.float64)
        z = (x.mean(0) - np.array(FURNACE_B)) / (x.std(0, ddof=1) / np.sqrt(len(x)))
        print(f"g {g} sample {sample}: mean {x.mean(0)} z {z} std {x.std(0)}")
        assert (np.abs(z) <= Z_BOUND).all(), (sample, z)


DARK_N = 4096
DARK_GLOW = (20.0, 12.0, 4.0)
DARK_MSE_SPP = 16


def _dark_room():
    """A black background, a diffuse floor and one wall, and a 16^3 grid of thin, purely absorbing fog (density 1, albedo 0) whose heat is one
    2^3 block: a small fire above the floor, just outside the camera's view — every pixel sees floor or wall."""
    planes = np.array([[-2.5, 0, 2.5, 5, 0, 0, 0, 0, -5, 0, QUAD], [-2.5, 0, -2.5, 5, 0, 0, 0, 4.5, 0, 1, QUAD]], np.float32)
    host = rb.HostScene.from_arrays(np.array([[0, 1000, 0, 0.5, 0]], np.float32), planes,
                                    [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_LAMBERTIAN, (0.7, 0.5, 0.4))])
    heat = np.zeros((16, 16, 16), np.float32)
    heat[3:5, 7:9, 7:9] = 1.0
    kw = dict(medium=dict(sigma_t=0.1, albedo=0.0, box=(-2, 0.25, -2, 2, 4.25, 2)), density=np.ones((16, 16, 16), np.float32), radiance=DARK_GLOW, source=2,
              heat=heat, emitters=False)
    return host, (lambda spp: rb.make_camera(8, 6, 25.0, (0, 3.2, 5.0), (0, 0.6, -0.5), (0, 0, 0), spp, 8)), kw


def test_dark_room_equal_expectation_and_the_variance_win():
    """The frame the light sample is for.  Per pixel and channel the means of rt_render_glow's estimator and of both sampled modes agree at
    4096 samples (a two-sample z with each frame's own variance, |z| <= 4.5), and at 16 samples per pixel the mis frame's luminance MSE
    against a 65 536-sample frame of other samples is below the unsampled frame's (measured ratio: DESIGN.md §36)."""
    host, camera, kw = _dark_room()
    mom = {s: gs.frame(host, camera(DARK_N), sample=s, moments=True, **kw)[1] for s in (None, "mis", "light")}
    assert (mom[None][..., :3] > 0).all()          # (every pixel is lit)
    for a, b in ((None, "mis"), (None, "light"), ("mis", "light")):
        z = _channel_z(mom[a], mom[b], DARK_N)
        print(f"{a} against {b}: max |z| {np.abs(z).max():.2f}")
        assert (np.abs(z) <= Z_BOUND).all(), (a, b, np.abs(z).max())
    ref = gs.frame(host, camera(65536), sample="mis", sample_first=1 << 20, **kw) / 65536.0
    mse = {}
    for s in (None, "mis", "light"):
        fb = gs.frame(host, camera(DARK_MSE_SPP), sample=s, **kw) / float(DARK_MSE_SPP)
        mse[s] = float((((fb - ref) @ LUM) ** 2).mean())
    print(f"luminance MSE at {DARK_MSE_SPP} spp: unsampled {mse[None]:.3e} mis {mse['mis']:.3e} light {mse['light']:.3e}; mis / unsampled {mse['mis'] / mse[None]:.4f}")
    assert mse["mis"] / mse[None] < 1.0


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------

SOURCES = (0, 1, 2)
PROBE_VIEW = (8, 5, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRIDS))
def test_sampler_table_equals_the_restatement(name):
    """rt_glow_sampler_table, row by row, against the restatement's table for the grid under the three sources; and an all-zero heat is an
    empty sampler (count 0)."""
    density, heat = GRIDS[name], HEATS[name]
    nz, ny, nx = density.shape
    rows = [(z, y) for z in range(nz) for y in range(ny)] if nz * ny <= 64 else [(0, 0), (3, 7), (15, 15), (8, 0), (0, 15), (11, 4)]
    with rb.Volume(density) as vol, rb.Volume(heat) as hv, rb.Volume(np.zeros_like(heat)) as cold:
        for source in SOURCES:
            want = gs.table(density, source, heat if source == 2 else None)
            with rb.GlowSampler(vol, source, hv if source == 2 else None) as q:
                for z, y in rows:
                    count, slab, row, cell, pc = q.table(z, y)
                    assert count == (0 if want["empty"] else nx * ny * nz)
                    assert_same(slab, want["slab_cdf"], f"{name} source {source}: slab cdf")
                    assert_same(row, want["row_cdf"][z], f"{name} source {source}: row cdf of slab {z}")
                    assert_same(cell, want["cell_cdf"][z, y], f"{name} source {source}: cell cdf of row {z}, {y}")
                    assert_same(pc, want["pc"][z, y], f"{name} source {source}: pc of row {z}, {y}")
        with rb.GlowSampler(vol, 2, cold) as q:
            count, slab, row, cell, pc = q.table(0, 0)
            assert count == 0 and not slab.any() and not row.any() and not cell.any() and not pc.any()


def _compare_probe(got, want, what):
    rad, rays, events, seeds, ns, es, ms, cells, length, shots = got
    wrad, wrays, wevents, wends, wseeds, wcells, wlength, wshots = want
    assert_same(rad, wrad, what + ": radiance")
    assert_same(rays, wrays, what + ": rays")
    assert_same(events, wevents, what + ": medium events")
    assert_same(cells, wcells, what + ": cells")
    assert_same(length, wlength, what + ": glow_length")
    assert_same(shots, wshots, what + ": glow_samples")
    for k, col in enumerate((seeds, ns, es, ms)):
        assert_same(col, wseeds[:, k], what + f": final seed {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [1, 0])
@pytest.mark.parametrize("name", list(GRIDS))
def test_probe_samples_equal_the_restatement(name, mis):
    """Every column of the probe against the restatement on the grid, for every combination of g in {0, +-0.95}, the depths 1, 2 and 12, the
    camera outside and inside the box, glossy on and off, with and without emitters and an environment; the source and the scene turn with
    the combination."""
    w, h, spp = PROBE_VIEW
    ijs = all_ijs(w, h, spp)
    names = ("fuzz planes", "three balls", "night rtiow")
    every = scenes()
    devs = {s: rb.DeviceScene(every[s][0], device=0) for s in names}
    density, heat = GRIDS[name], HEATS[name]
    sample = "mis" if mis else "light"
    seen_shots = seen_events = combos = 0
    with rb.Env(sun_map()) as env, rb.Volume(density) as vol, rb.Volume(heat) as hv:
        samplers = {s: rb.GlowSampler(vol, s, hv if s == 2 else None) for s in SOURCES}
        for g in (0.0, 0.95, -0.95):
            for depth in (1, 2, 12):
                for kind in ("scene", "inside"):
                    for k in range(8):
                        scene = names[(combos + k) % 3]
                        source = SOURCES[combos % 3]
                        ref, dkw = _setting(k)
                        if dkw.get("env") == "sun":
                            dkw["env"] = env
                        cam = every[scene][1](w, h, spp, depth) if kind == "scene" else special_camera(kind, w, h, spp, depth)
                        radiance = GLOWS[combos % 3]
                        want = gs.trace(every[scene][0], cam, ijs, medium=fog(g), density=density, radiance=radiance, source=source,
                                        heat=heat if source == 2 else None, sample=sample, **ref)
                        got = devs[scene].trace_samples_glow_sampled(cam, ijs, medium=fog(g), volume=vol, glow=dict(radiance=radiance, source=source),
                                                                     heat=hv if source == 2 else None, sample=sample, sampler=samplers[source], **dkw)
                        _compare_probe(got, want, f"{name} / {sample} / {scene} / source {source} / g {g} / depth {depth} / camera {kind} / setting {k}")
                        seen_shots += int(want[7].sum())
                        seen_events += int(want[2].sum())
                        combos += 1
        for q in samplers.values():
            q.close()
    assert combos == 144 and seen_shots > 1000 and seen_events > 100, (combos, seen_shots, seen_events)
    for d in devs.values():
        d.close()


@pytest.mark.gpu
def test_frames_equal_the_restatement():
    """40 x 27 x 3 spp, 7 x 5 x 1, a 3-row shard of the first, sample_first = 5, sync = 0 on a torch stream, and one 8 x 6 x 2 frame through
    each of the eight instantiations of glow_sample_render_kernel: pinhole / lens x the four emitter tables."""
    import torch
    scene = "three balls"
    host, camera, _ = scenes()[scene]
    ref, dkw = _setting(7)
    medium, density, heat, radiance = fog(0.7), GRIDS["2x3x5"], HEATS["2x3x5"], GLOWS[0]
    dev = rb.DeviceScene(host, device=0)
    with rb.Env(sun_map()) as env, rb.Volume(density) as vol, rb.Volume(heat) as hv, rb.Volume(GRIDS["16"]) as vol16, rb.Volume(HEATS["16"]) as heat16:
        dkw["env"] = env
        with rb.GlowSampler(vol, 2, hv) as q:
            for (w, h, spp), more in (((40, 27, 3), {}), ((7, 5, 1), {}), ((40, 27, 3), dict(shard=rb.Shard(3, 1, 4))), ((40, 27, 3), dict(sample_first=5))):
                cam = camera(w, h, spp, 12)
                want = gs.frame(host, cam, medium=medium, density=density, radiance=radiance, source=2, heat=heat, sample="mis", **more, **ref)
                got, _ = dev.render_glow_sampled_to_host(cam, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=hv, sample="mis", sampler=q,
                                                         **more, **dkw)
                assert_same(got, want, f"frame {w}x{h}x{spp} {more}")
        # lens + motion with the light tree over the two-kind table, on a stream, without waiting inside the call
        scene2 = "fuzz planes"
        host2, camera2, close2 = scenes()[scene2]
        dev2 = rb.DeviceScene(host2, device=0)
        from test_medium import LENS
        w, h, spp = 40, 27, 3
        cam = camera2(w, h, spp, 12)
        lens_r = dict(lens=LENS, cam_close=close2(w, h, spp, 12))
        lens_d = dict(lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), cam_close=close2(w, h, spp, 12))
        with rb.GlowSampler(vol16, 2, heat16) as q16:
            want = gs.frame(host2, cam, medium=fog(-0.5), density=GRIDS["16"], radiance=GLOWS[1], source=2, heat=HEATS["16"], sample="light", select=1, planes=1,
                            glossy=1, **lens_r)
            stream = torch.cuda.Stream()
            fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
            with torch.cuda.stream(stream):
                dev2.render_glow_sampled(cam, fb.data_ptr(), medium=fog(-0.5), volume=vol16, glow=dict(radiance=GLOWS[1], source=2), heat=heat16, sample="light",
                                         sampler=q16, stream=stream.cuda_stream, sync=False, nee=dict(select=1, sample_planes=1, glossy=1), **lens_d)
            stream.synchronize()
            assert_same(fb.cpu().numpy(), want, "sync = 0 on a torch stream")
        # the eight instantiations, each on an 8 x 6 x 2 frame; the three sources and the two modes in turn
        w, h, spp = 8, 6, 2
        samplers = {s: rb.GlowSampler(vol, s, hv if s == 2 else None) for s in SOURCES}
        k = 0
        for lens in (False, True):
            for select, planes in ((0, 0), (0, 1), (1, 0), (1, 1)):
                cam = camera2(w, h, spp, 12)
                source, sample = k % 3, ("mis", "light")[k % 2]
                kw_r = dict(select=select, planes=planes, glossy=k % 2, **(dict(lens=LENS, cam_close=close2(w, h, spp, 12)) if lens else {}))
                kw_d = dict(nee=dict(select=select, sample_planes=planes, glossy=k % 2),
                            **(dict(lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), cam_close=close2(w, h, spp, 12)) if lens else {}))
                want = gs.frame(host2, cam, medium=fog(0.3), density=density, radiance=GLOWS[k % 3], source=source, heat=heat if source == 2 else None, sample=sample,
                                **kw_r)
                got, t = dev2.render_glow_sampled_to_host(cam, medium=fog(0.3), volume=vol, glow=dict(radiance=GLOWS[k % 3], source=source),
                                                          heat=hv if source == 2 else None, sample=sample, sampler=samplers[source], **kw_d)
                assert_same(got, want, f"frame lens={lens} select={select} planes={planes} source={source} {sample}")
                assert t.trace_scratch_bytes == 0, (lens, select, planes, t.trace_scratch_bytes)
                k += 1
        for q in samplers.values():
            q.close()
        dev2.close()
    dev.close()


@pytest.mark.gpu
def test_device_identities():
    """Through the kernels they name: no sample (None, sample = 0), an empty sampler and radiance 0, 0, 0 are rt_render_glow — frames and
    probes, glow_samples 0; max_depth = 1 under mis and light is rt_render_glow's radiance, through the sampled kernels."""
    scene = "fuzz planes"
    host, camera, _ = scenes()[scene]
    w, h, spp = 16, 9, 3
    ijs = all_ijs(w, h, spp)
    dev = rb.DeviceScene(host, device=0)
    density, heat = GRIDS["2x3x5"], HEATS["2x3x5"]
    with rb.Env(sun_map()) as env, rb.Volume(density) as vol, rb.Volume(heat) as hv, rb.Volume(np.zeros_like(heat)) as cold:
        with rb.GlowSampler(vol, 2, hv) as q, rb.GlowSampler(vol, 2, cold) as q_cold, rb.GlowSampler(vol, 1) as q1:
            for k in range(8):
                _, dkw = _setting(k)
                if dkw.get("env") == "sun":
                    dkw["env"] = env
                cam = camera(w, h, spp, 12)
                medium = fog((0.0, 0.7, -0.95)[k % 3])
                radiance = GLOWS[k % 3]
                for what, gkw, skw in (("no sample", dict(glow=dict(radiance=radiance, source=2), heat=hv), dict(sample=None, sampler=None)),
                                       ("sample = 0", dict(glow=dict(radiance=radiance, source=2), heat=hv), dict(sample=dict(sample=0, mis=k % 2), sampler=q)),
                                       ("an empty sampler", dict(glow=dict(radiance=radiance, source=2), heat=cold), dict(sample="mis", sampler=q_cold)),
                                       ("no glow", dict(glow=dict(radiance=0.0, source=1)), dict(sample="light", sampler=q1))):
                    got = dev.trace_samples_glow_sampled(cam, ijs, medium=medium, volume=vol, **gkw, **skw, **dkw)
                    want = dev.trace_samples_glow(cam, ijs, medium=medium, volume=vol, **gkw, **dkw)
                    for j, (a, b) in enumerate(zip(got[:9], want)):
                        assert_same(a, b, f"setting {k} / {what}: column {j}")
                    assert not got[9].any()
                    assert_same(dev.render_glow_sampled_to_host(cam, medium=medium, volume=vol, **gkw, **skw, **dkw)[0],
                                dev.render_glow_to_host(cam, medium=medium, volume=vol, **gkw, **dkw)[0], f"setting {k} / {what}: frame")
                cam1 = camera(w, h, spp, 1)
                want = dev.trace_samples_glow(cam1, ijs, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=hv, **dkw)
                want_frame = dev.render_glow_to_host(cam1, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=hv, **dkw)[0]
                for sample in ("mis", "light"):
                    got = dev.trace_samples_glow_sampled(cam1, ijs, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=hv, sample=sample,
                                                         sampler=q, **dkw)
                    for j in (0, 1, 2, 3, 4, 5, 6, 8):
                        assert_same(got[j], want[j], f"setting {k} / max_depth 1 / {sample}: column {j}")
                    assert not got[9].any() and (want[8] > 0).any()
                    assert_same(dev.render_glow_sampled_to_host(cam1, medium=medium, volume=vol, glow=dict(radiance=radiance, source=2), heat=hv, sample=sample,
                                                                sampler=q, **dkw)[0], want_frame, f"setting {k} / max_depth 1 / {sample}: frame")
    dev.close()


@pytest.mark.gpu
def test_sampler_mismatch_and_devices():
    """A sampler built for another source, other dimensions or other grids than the call's is refused before the scene is looked at (a
    null scene: the sampler's word, not the scene's); the sampler of the call's own grids reaches the null-scene check.  rt_glow_sampler_create
    refuses what the header says."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    cam = rb.rtiow_camera(8, 4, 2)
    medium = rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, 1, 1))
    on = rb.glow_sample_params(sample=1)
    with rb.Volume(GRIDS["2x3x5"]) as vol, rb.Volume(GRIDS["2x3x5"].copy()) as twin, rb.Volume(HEATS["2x3x5"]) as hv, rb.Volume(GRIDS["16"]) as vol16:
        with rb.GlowSampler(vol, 1) as q1, rb.GlowSampler(vol, 2, hv) as q2, rb.GlowSampler(vol16, 1) as q16, rb.GlowSampler(twin, 1) as qt:
            for source, heat, sampler, word in ((1, None, q2, "another source"), (2, hv, q1, "another source"), (1, None, q16, "dimensions differ"),
                                                (1, None, qt, "other grids"), (2, twin, q2, "other grids"), (1, None, q1, "null scene"), (2, hv, q2, "null scene")):
                glow = rb.glow_params(radiance=1.0, source=source)
                st1, m1, st2, m2 = _calls(cam, None, medium, vol._h, glow, heat._h if heat else None, on, sampler._h)
                assert st1 == INVALID and word in m1 and "rt_render_glow_sampled" in m1, (word, m1)
                assert st2 == INVALID and word in m2 and "rt_trace_samples_glow_sampled" in m2, (word, m2)
        for args, word in (((vol, 3, None), "source must"), ((vol, 2, None), "needs a heat grid"), ((vol, 1, hv), "source 2 only"), ((vol, 2, vol16), "dimensions differ")):
            with pytest.raises(rb.RtError, match=word):
                rb.GlowSampler(*args)


@pytest.mark.gpu
def test_handle_state_is_left_alone():
    """rt_render and rt_render_lit of a handle after sampled glow calls — one of them refused with the scene in hand — equal a fresh handle's."""
    host, camera, _ = scenes()["three balls"]
    cam = camera(24, 16, 2, 12)
    fresh = rb.DeviceScene(host, device=0)
    want_render, _ = fresh.render_to_host(cam)
    want_lit, _ = fresh.render_lit_to_host(cam)
    fresh.close()
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(GRIDS["16"]) as vol, rb.Volume(HEATS["16"]) as heat, rb.GlowSampler(vol, 2, heat) as q, rb.GlowSampler(vol, 1) as q1:
        dev.render_glow_sampled_to_host(cam, medium=fog(0.3), volume=vol, glow=dict(radiance=GLOWS[0], source=2), heat=heat, sample="mis", sampler=q)
        with pytest.raises(rb.RtError, match="another source"):
            dev.render_glow_sampled_to_host(cam, medium=fog(0.3), volume=vol, glow=dict(radiance=GLOWS[0], source=2), heat=heat, sample="mis", sampler=q1)
        with pytest.raises(rb.RtError, match="needs a sampler"):
            dev.render_glow_sampled_to_host(cam, medium=fog(0.3), volume=vol, glow=dict(radiance=GLOWS[0], source=1), sample="light")
        dev.render_glow_sampled_to_host(cam, medium=fog(0.3), volume=vol, glow=dict(radiance=GLOWS[1], source=1), sample="light", sampler=q1)
    got_render, _ = dev.render_to_host(cam)
    got_lit, _ = dev.render_lit_to_host(cam)
    assert_same(got_render, want_render, "rt_render after rt_render_glow_sampled")
    assert_same(got_lit, want_lit, "rt_render_lit after rt_render_glow_sampled")
    dev.close()


@pytest.mark.gpu
def test_cli_fog_glow_sample_frames_are_the_python_path(test_config_text, tmp_path):
    """rtp_main --fog-glow … --fog-glow-sample mis|light, over the density and over a heat grid: the frame file holds the bytes of the Python path."""
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera_at(0.0)
    density, heat_grid = GRIDS["2x3x5"], HEATS["2x3x5"]
    grid_file, heat_file = _grid_file(tmp_path / "grid.vol", density), _grid_file(tmp_path / "heat.vol", heat_grid)
    box = (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0)
    medium = dict(sigma_t=0.4, albedo=0.9, g=0.3, box=box)
    with rb.Volume(density) as vol, rb.Volume(heat_grid) as heat:
        for source, sample in ((1, "mis"), (2, "light")):
            args = ["--lit", "--nee", "--light-tree", "--fog", "0.4:0.9:0.3", "--fog-box", ",".join(str(x) for x in box), "--fog-grid", grid_file,
                    "--fog-glow", "0.5,0.25,0.125" + (":density" if source == 1 else ""), "--fog-glow-sample", sample]
            args += ["--fog-heat", heat_file] if source == 2 else []
            out = subprocess.run([EXE, "--gpu", *args], input=text, capture_output=True, text=True, timeout=200)
            assert out.returncode == 0, out.stderr
            glow = dict(radiance=(0.5, 0.25, 0.125), source=source)
            with rb.GlowSampler(vol, source, heat if source == 2 else None) as q:
                fb, _ = dev.render_glow_sampled_to_host(cam, nee=dict(select=1), medium=medium, volume=vol, glow=glow, heat=heat if source == 2 else None, sample=sample,
                                                        sampler=q)
            plain, _ = dev.render_glow_to_host(cam, nee=dict(select=1), medium=medium, volume=vol, glow=glow, heat=heat if source == 2 else None)
            assert (fb != plain).any()
            assert open(tmp_path / "f_0.png", "rb").read() == rb.binary_image_bytes(fb, cam.image_width, cam.image_height, info.sqrt_spp), (source, sample)
            os.remove(tmp_path / "f_0.png")
    dev.close()
