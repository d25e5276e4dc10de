"""The fog family's ray routines, ray by ray.  On the CPU: tests/fog_ray_cases.py's sets reach what they aim at — every
tally of volume_ref.c's walk is met, the tallies only count, the restatements return no NaN on any ray, the new exports of chroma_ref.c and
glow_ref.c agree with the old ones.  On the GPU: tests/dev_fog_ray_checks.py in one child process on the developer library — every column
of every routine on every ray against the CPU statement, bit for bit.

Two things cannot be met.  The tally "left by the index": the step that would take an index out of the grid follows a cell whose tnext on
that axis is (face_k - o_k) / d_k with the box's own face (vol_plane returns a and b themselves at the ends) — the very expression, and so
the very float, med_interval took the slab's far bound from; t1 is the smallest of those bounds and t_end, so tm >= t1, tb = t1, and the
walk has left by `tb >= t1` before the index is looked at.  The index check is a guard that never fires for an interval med_interval
made; the test asserts the tally is 0 over all sets, so that a set which reaches it is noticed.  And the budget, which is replaced by the
bound that proves it: the walk's budget `left = nx + ny + nz` is never exhausted for
finite inputs.  Each step moves one index by one, monotonically (the sign of d_k never changes), inside [0, n_k - 1]; a walk therefore
takes at most (nx - 1) + (ny - 1) + (nz - 1) steps and visits at most nx + ny + nz - 2 cells, two fewer than the budget.
test_walk_never_uses_its_budget asserts that bound on every ray; it is attained on "exact 2x3x5" (8 cells) and "exact 1x1x64" (64)."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import chroma_reference as cr
import fog_ray_cases as fc
import glow_reference as gr
import glow_sample_reference as gsr
import medium_reference as mr
import test_volume as tv
import volume_reference as vr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE_SETS = 9          # walk_sets() begins with the four exact boxes and the five inexact ones


@pytest.fixture(scope="module", autouse=True)
def libraries():
    """The five restatements, compiled side by side."""
    with ThreadPoolExecutor(5) as pool:
        list(pool.map(lambda m: m.lib(), (mr, vr, cr, gr, gsr)))


def _rems(s, w):
    return {name: rem for name, rem in fc.rem_args(w["acc"]) + (("random", (w["acc"] * fc._random_args(s.name, len(s.o))).astype(np.float32)),)}


def test_the_sets_are_what_the_issue_lists():
    sets = fc.walk_sets()
    names = [s.name for s in sets]
    assert names[:BASE_SETS] == ["exact 1", "exact 2x3x5", "exact 16", "exact 1x1x64", "BOX 2x3x5", "odd box 7x1x13", "odd box 3x5x2", "odd box 1x1x256",
                                 "odd box 256x1x1"]
    for s in sets[:BASE_SETS]:
        assert len(s.o) == 1280 and s.density.shape == s.heat.shape and s.o.dtype == s.d.dtype == s.t_end.dtype == np.float32
    for base in ("exact 2x3x5", "exact 16"):
        for e in fc.SCALES:
            assert f"{base}/2^{e}" in names
        for what in ("all zero", "one cell", "1e-6 … 1e4"):
            assert f"{base}/grid {what}" in names
    by = {s.name: s for s in sets}
    assert not by["exact 16/grid all zero"].density.any() and (by["exact 16/grid one cell"].density > 0).sum() == 1
    span = by["exact 16/grid 1e-6 … 1e4"].density
    assert span.min() == np.float32(1e-6) and span.max() == np.float32(1e4)
    assert abs((by["exact 16"].density == 0).mean() - 1 / 3) < 0.05, "random_grid's third of empty cells"
    for s in sets[:BASE_SETS]:
        z = by[s.name + "/-0"]
        assert ((z.d == 0) & np.signbit(z.d)).any(1).all() and not ((z.d == 0) & ~np.signbit(z.d)).any()
        assert len(z.o) == int((s.d == 0).any(1).sum())
    for name in ("exact 2x3x5/far 1e3", "exact 2x3x5/far 1e6", "odd box 7x1x13/far 1e3", "odd box 7x1x13/far 1e6"):
        s = by[name]
        b = np.array(s.medium["box"])
        far = np.linalg.norm(s.o - (b[:3] + b[3:]) / 2, axis=1) / s.diagonal
        assert (np.abs(far / float(name.split()[-1]) - 1) < 0.01).all()
    # the widths of the inexact boxes are not float32 numbers
    for s in sets[4:BASE_SETS]:
        b = np.array(s.medium["box"], np.float32)
        w = (b[3:].astype(np.float64) - b[:3]) / np.array(s.dims)
        assert (w.astype(np.float32).astype(np.float64) != w)[np.array(s.dims) > 1].any(), s.name
    kinds = {name for name, *_ in fc.interval_sets()}
    assert {"box", "ball", "all space", "origins on a face", "tangents to the ball", "exact case 0", "exact case 26"} <= kinds


def test_tallies_only_count():
    """Every column of volume_walks is the same bytes with the tallies and without them."""
    for s in fc.walk_sets()[:BASE_SETS]:
        w = vr.walks(s.medium, s.density, s.o, s.d, s.t_end)
        rem = _rems(s, w)["random"]
        a, b = vr.walks(s.medium, s.density, s.o, s.d, s.t_end, rem=rem), vr.walks(s.medium, s.density, s.o, s.d, s.t_end, rem=rem, tallies=False)
        assert a["flags"].any() and not b["flags"].any()
        for key in a:
            if key != "flags":
                assert a[key].tobytes() == b[key].tobytes(), (s.name, key)


def test_the_sets_reach_every_tally():
    """Which set reaches which tally of vol_walk (rays per set), every tally > 0 over the sets; DESIGN.md §39 holds the table."""
    total = np.zeros(len(vr.TALLIES), np.int64)
    print("set".ljust(34) + " ".join(f"{k:>5d}" for k in range(len(vr.TALLIES))))
    for s in fc.walk_sets():
        w = vr.walks(s.medium, s.density, s.o, s.d, s.t_end)
        flags = np.zeros(len(s.o), np.int32)
        for name, rem in _rems(s, w).items():
            flags |= vr.walks(s.medium, s.density, s.o, s.d, s.t_end, rem=rem)["flags"]
        counts = np.array([int(((flags >> k) & 1).sum()) for k in range(len(vr.TALLIES))])
        total += counts
        print(s.name.ljust(34) + " ".join(f"{c:>5d}" for c in counts))
    for k, name in enumerate(vr.TALLIES):
        print(f"tally {k:2d} {name}: {total[k]} rays")
    index = vr.TALLIES.index("left by the index")
    assert (np.delete(total, index) > 0).all(), [vr.TALLIES[k] for k in np.flatnonzero(total == 0)]
    assert total[index] == 0, "the module docstring proves this exit unreachable: a set that reaches it has found a hole in the proof"
    # the classes that aim at ties reach them on the exact boxes: rays at grid vertices and down exact diagonals
    for s in fc.walk_sets()[1:3]:
        flags = vr.walks(s.medium, s.density, s.o, s.d, s.t_end)["flags"]
        names = [c for c, _ in tv.WALK_CLASSES]
        diagonal = s.kind == names.index("from a vertex down an exact diagonal")
        assert ((flags[diagonal] >> 1) & 1).sum() > 10, "three axes tie down an exact diagonal"
        assert (flags & 3 != 0).sum() > 50, s.name


def test_walk_never_uses_its_budget():
    """cells <= nx + ny + nz - 2 on every ray of every set and every flight (the module docstring has the proof); attained on two sets."""
    most = {}
    for s in fc.walk_sets():
        w = vr.walks(s.medium, s.density, s.o, s.d, s.t_end)
        f = vr.walks(s.medium, s.density, s.o, s.d, s.t_end, rem=np.inf)
        bound = max(1, sum(s.dims) - 2)
        assert (w["cells"] <= bound).all() and (f["flight_cells"] <= bound).all(), s.name
        assert (w["cells"][w["hit"] == 1] >= 1).all() and not w["cells"][w["hit"] == 0].any()
        most[s.name] = int(w["cells"].max())
    assert most["exact 2x3x5"] == 8 and most["exact 1x1x64"] == 64, most


def test_line_takes_both_branches():
    series = closed = 0
    for s in fc.walk_sets()[:BASE_SETS]:
        _, _, a, b = gsr.line(s.medium, s.density, s.o, s.d, s.t_end)
        series, closed = series + a, closed + b
    print(f"glow_line: {series} cells by the series, {closed} by the closed form")
    assert series > 1000 and closed > 1000


def test_no_restatement_returns_a_nan():
    """A condition on the inputs: the device comparison is then never about NaN payloads.  Every pass of every set, none exempt."""
    rays = columns = 0
    for passes in [fc.interval_passes()] + [fc.walk_passes(s) for s in fc.walk_sets()]:
        for p in passes:
            rays += len(p.o)
            columns += len(p.o) * len(fc.COLUMNS[p.routine])
            for name, c in fc.floats_of(p.routine, p.want).items():
                assert not np.isnan(c).any(), (p.label, name, int(np.isnan(c).sum()))
            assert not p.want[:, len(fc.COLUMNS[p.routine]):].any()
    print(f"{rays} rays, {columns} columns, no NaN")
    assert rays > 2000000


def test_scales():
    """d * 2^e with t_end / 2^e describes the same ray: at all five scales the walk, its flight, glow_pl and glow_line return no NaN and no
    infinite t_event, and as many rays cross as unscaled.  At 2^-70 the squared length is denormal."""
    by = {s.name: s for s in fc.walk_sets()}
    for base in ("exact 2x3x5", "exact 16"):
        b = by[base]
        w0 = vr.walks(b.medium, b.density, b.o, b.d, b.t_end)
        moved = 0.0
        for e in fc.SCALES:
            s = by[f"{base}/2^{e}"]
            assert (s.o == b.o).all() and np.isfinite(s.d).all() and (s.d != 0).sum() == (b.d != 0).sum(), "the scaling is exact: nothing under- or overflows"
            w = vr.walks(s.medium, s.density, s.o, s.d, s.t_end, rem=_rems(b, w0)["acc / 2"])
            assert w["hit"].sum() == w0["hit"].sum(), (s.name, int(w["hit"].sum()), int(w0["hit"].sum()))
            assert not np.isnan(w["acc"]).any() and not np.isnan(w["t_event"]).any() and np.isfinite(w["t_event"]).all() and w["event"].sum() > 300
            pl = gsr.pl(s.medium, s.density, s.o, s.d)[0]
            G = gsr.line(s.medium, s.density, s.o, s.d, s.t_end)[0]
            assert not np.isnan(pl).any() and not np.isnan(G).any(), s.name
            if e == -70:
                lensq = (s.d.astype(np.float64) ** 2).sum(1)
                assert (lensq < 2.0 ** -126).all() and (lensq > 0).all(), "the squared length is denormal"
                tau_max = tv.WALK_SIGMA * float(b.density.max()) * b.diagonal
                moved = float(np.abs(w["acc"].astype(np.float64) - w0["acc"]).max() / tau_max)
        print(f"{base}: at 2^-70 acc moves by up to {moved:.3f} of tau_max")
        # (the squared length keeps 149 - 140 or so of its 24 bits there: far more than the walk's own rounding, WALK_TOL, and far less
        # than a device that flushed the denormal to zero would show — len = 0 and acc = 0 on every ray)
        assert moved > 100 * tv.WALK_TOL, "the denormal squared length shows in acc"


def test_span_grid_reaches_one_denormals_and_zero():
    trs = np.concatenate([vr.walks(s.medium, s.density, s.o, s.d, s.t_end)["tr"][vr.walks(s.medium, s.density, s.o, s.d, s.t_end)["hit"] == 1]
                          for s in fc.walk_sets() if "1e-6" in s.name])
    denormal = (trs > 0) & (trs < np.float32(2.0 ** -126))
    print(f"tr over the span grids: {int((trs == 1).sum())} exactly 1, {int(denormal.sum())} denormal, {int((trs == 0).sum())} exactly 0")
    assert (trs == 1).any() and denormal.any() and (trs == 0).any()


def test_the_new_exports_agree_with_the_old_ones():
    """chroma_flights on the grid base with sigma_t = 1 is volume_walks' flight: event and t bit for bit, and without an event A is its
    acc bit for bit (the same sum in the same order).  glow_flights without heat keeps in E the length it flew, within the bound
    test_walk_terminates_and_keeps_its_books holds the segments' sum to: WALK_TOL x the box's diagonal, on the boxes that bound was measured
    on, and within the a-priori bound of a float32 sum on all nine."""
    worst = 0.0
    for s in fc.walk_sets()[:BASE_SETS]:
        unit = dict(s.medium, sigma_t=1.0)
        w = vr.walks(unit, s.density, s.o, s.d, s.t_end)
        for name, R in fc.rem_args(w["acc"]):
            a, b = cr.flights(unit, s.density, fc.TINT, s.o, s.d, s.t_end, R), vr.walks(unit, s.density, s.o, s.d, s.t_end, rem=R)
            assert (a["hit"] == b["hit"]).all() and (a["event"] == b["event"]).all() and a["t"].tobytes() == b["t_event"].tobytes(), (s.name, name)
            none = (a["hit"] == 1) & (a["event"] == 0)
            assert a["A"][none].tobytes() == w["acc"][none].tobytes(), (s.name, name)
            assert (a["cells"] == b["flight_cells"]).all()
        hit, t0, t1 = mr.intervals(s.medium, s.o, s.d, s.t_end)
        length = np.linalg.norm(s.d.astype(np.float64), axis=1)
        for name, u in fc.U_ARGS:
            f = gr.flights(s.medium, s.density, s.o, s.d, s.t_end, u)
            assert (f["hit"] == hit).all()
            stop = np.where(f["event"] == 1, f["t"], t1).astype(np.float64)
            flown = (stop - t0) * length
            err = np.abs(f["E"].astype(np.float64) - flown)[hit == 1] / s.diagonal
            if s.name.startswith("exact"):
                worst = max(worst, float(err.max()))
                assert err.max() <= tv.WALK_TOL, (s.name, name, float(err.max()))
            # WALK_TOL is a figure measured on walk_cases' four boxes, at most 64 segments a ray ("rounding depends on the segment count");
            # the other boxes, up to 256 segments, are held to the a-priori bound of such a sum instead: E is a float32 sum of `cells`
            # terms (cells - 1 additions, each term one product and one difference, t and t0 one rounding each), every partial sum at
            # most the length flown <= the diagonal — (cells + 4) units of roundoff
            assert (err <= (f["cells"][hit == 1] + 4) * 2.0 ** -24).all(), (s.name, name)
    print(f"E against the length flown: largest error {worst:.3e} of the diagonal, bound {tv.WALK_TOL:.3e}")


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_fog_routines_equal_the_restatements_ray_by_ray_on_gfx950():
    """tests/dev_fog_ray_checks.py in one child process that loads the developer library (rt_debug_fog_rays): medium_interval, the three
    volume_walk instantiations, chroma_flight / chroma_tr, glow_flight, glow_pl and glow_line over fog_ray_cases' rays, every column
    compared as uint32 with the CPU statement.  The child's FOG RAYS lines give the rays, the columns and the device time."""
    from conftest import run_child
    dev_lib = os.path.join(ROOT, "ray-tracing-practice_amd", "librtp_amd_dev.so")
    assert os.path.exists(dev_lib), "run __graft_entry__.build() (make -C ray-tracing-practice_amd dev)"
    env = dict(os.environ, RTP_AMD_LIB=dev_lib)
    res = run_child([sys.executable, "-m", "pytest", os.path.join(HERE, "dev_fog_ray_checks.py"), "-x", "-q", "-s", "-p", "no:cacheprovider"], 200, env=env)
    print(res.stdout[-6000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "4 passed" in res.stdout and "failed" not in res.stdout and "skipped" not in res.stdout
