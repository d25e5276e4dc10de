"""The rays on which the fog family's device routines are compared with the CPU restatements, ray by ray (TEST INFRASTRUCTURE; DESIGN.md
§39).  Deterministic: tests/test_fog_rays.py (CPU: the sets reach what they aim at) and tests/dev_fog_ray_checks.py (device: every column
of every routine on every ray, bit for bit) read the same sets.  None needs a scene, a camera or a frame.

walk_sets(): rays through density grids — test_volume.walk_cases on its four exact boxes; the same classes (test_volume.walk_rays) over
boxes whose cell widths are not exact in float32; scaled directions (d * 2^e, t_end / 2^e); far origins; d_k == -0.0 in the place of every
d_k == 0; and grids that are all empty, hold one cell, or span ten orders of magnitude.  interval_sets(): rays against the three regions —
test_lit_fuzz_gloss_medium's random rays, every ray of its test_intervals_exact_cases, origins exactly on a face, tangents to the ball.
The special arguments of the flights (rem, R, u) are rem_args() and U_ARGS."""
import functools
from typing import NamedTuple

import numpy as np

import test_lit_fuzz_gloss_medium as gm
import test_volume as tv

SCALES = (-70, -62, -40, 40, 60)          # d * 2^e, t_end / 2^e: at 2^-70 the squared length is denormal
ODD_BOX = ((-1.3, 0.1, -2.7), (0.9, 1.7, 0.2))          # corners nobody would pick: no cell width is exact
TINT = (1.0, 0.0, 2.5)          # routine 3's channels: sigma_t * tint[k], one of them exactly 0
U_ARGS = (("0", 0.0), ("2^-32", 2.0 ** -32), ("0.5", 0.5), ("1 - 2^-24", 1.0 - 2.0 ** -24), ("1", 1.0))          # routine 4's draws
INTERVAL_RAYS = 20000          # per region, of test_lit_fuzz_gloss_medium._random_rays


class RaySet(NamedTuple):
    name: str
    medium: dict          # sigma_t and the box
    density: np.ndarray          # (nz, ny, nx) float32
    heat: np.ndarray          # the same shape: source 2's h
    o: np.ndarray
    d: np.ndarray
    t_end: np.ndarray
    kind: np.ndarray          # per ray, its class: an index into tv.WALK_CLASSES
    tie_t: float = 1.0          # the parameter at which the rays aimed at a grid vertex reach it (o + tie_t * d)

    @property
    def dims(self):
        return self.density.shape[::-1]

    @property
    def diagonal(self):
        b = np.array(self.medium["box"], np.float64)
        return float(np.linalg.norm(b[3:] - b[:3]))


def _heat_of(density, seed):
    return tv.random_grid(density.shape, 5000 + seed, empty=0.25)


def _box_set(name, dims, lo, hi, density, seed):
    lo, hi = np.array(lo), np.array(hi)
    diag = float(np.linalg.norm(hi - lo))
    o, d, t_end, kind = tv.walk_rays(dims, lo, hi, np.random.default_rng([39, seed]), centre=(lo + hi) / 2, scale=max(1.0, diag / 4.0))
    return RaySet(name, dict(sigma_t=tv.WALK_SIGMA, box=tuple(lo) + tuple(hi)), density, _heat_of(density, seed), o, d, t_end, kind)


def _far(base, seed, count=200):
    """Origins 10^3 and 10^6 box diagonals away, aimed at points inside the box."""
    b = np.array(base.medium["box"], np.float64)
    lo, hi = b[:3], b[3:]
    rng = np.random.default_rng([39, 400, seed])
    out = []
    for dist in (1e3, 1e6):
        v = rng.normal(size=(count, 3))
        o = ((lo + hi) / 2 + v / np.linalg.norm(v, axis=1, keepdims=True) * dist * base.diagonal).astype(np.float32)
        d = ((lo + rng.random((count, 3)) * (hi - lo)).astype(np.float32) - o).astype(np.float32)
        d[1::2] *= rng.uniform(0.25, 4.0, (count, 1)).astype(np.float32)[1::2] / np.float32(dist * base.diagonal)          # … and of about unit length
        t_end = np.where(np.arange(count) % 2 == 0, np.float32(np.inf), np.float32(1.0)).astype(np.float32)
        out.append(base._replace(name=f"{base.name}/far 1e{int(np.log10(dist))}", o=o, d=d.astype(np.float32), t_end=t_end, kind=np.zeros(count, np.int64)))
    return out


def _minus_zero(base):
    """The rays with a d_k == 0, with -0.0 in its place."""
    sel = (base.d == 0.0).any(1)
    d = base.d[sel].copy()
    d[d == 0.0] = np.float32(-0.0)
    assert np.signbit(d[d == 0.0]).all() and sel.sum() >= 300
    return base._replace(name=base.name + "/-0", o=base.o[sel], d=d, t_end=base.t_end[sel], kind=base.kind[sel])


def _scaled(base, e):
    s = np.float32(2.0) ** np.float32(e)
    return base._replace(name=f"{base.name}/2^{e}", d=(base.d * s).astype(np.float32), t_end=(base.t_end / s).astype(np.float32), tie_t=float(1.0 / s))


def _grids(base, seed):
    """The same rays through an all-zero grid, a grid with exactly one non-empty cell, and one whose densities span 1e-6 … 1e4."""
    rng = np.random.default_rng([39, 700, seed])
    shape = base.density.shape
    zero = np.zeros(shape, np.float32)
    one = zero.copy()
    one.flat[rng.integers(0, one.size)] = 1.75
    span = (10.0 ** rng.uniform(-6.0, 4.0, shape)).astype(np.float32)
    span.flat[0], span.flat[-1] = 1e-6, 1e4
    return [base._replace(name=f"{base.name}/grid {what}", density=g) for what, g in (("all zero", zero), ("one cell", one), ("1e-6 … 1e4", span))]


@functools.lru_cache(maxsize=None)
def walk_sets():
    """Every set of rays through a grid, as a tuple of RaySet."""
    exact = []
    for k, name in enumerate(tv.WALK_GRIDS):
        medium, density, o, d, t_end, _, _ = tv.walk_cases(name)
        n, lo, hi = tv.WALK_GRIDS[name]
        kind = np.repeat(np.arange(len(tv.WALK_CLASSES)), [c for _, c in tv.WALK_CLASSES])
        exact.append(RaySet("exact " + name, dict(sigma_t=tv.WALK_SIGMA, box=tuple(lo) + tuple(hi)), density, _heat_of(density, k), o, d, t_end, kind))
    inexact = [_box_set("BOX 2x3x5", (2, 3, 5), tv.BOX[:3], tv.BOX[3:], tv.GRIDS["2x3x5"], 10)]
    for k, dims in enumerate([(7, 1, 13), (3, 5, 2), (1, 1, 256), (256, 1, 1)]):
        inexact.append(_box_set("odd box " + "x".join(map(str, dims)), dims, *ODD_BOX, tv.random_grid(dims[::-1], 3900 + k), 20 + k))
    by_name = {s.name: s for s in exact + inexact}
    sets = exact + inexact
    for name in ("exact 2x3x5", "exact 16"):
        sets += [_scaled(by_name[name], e) for e in SCALES]
    for k, name in enumerate(("exact 2x3x5", "odd box 7x1x13")):
        sets += _far(by_name[name], k)
    sets += [_minus_zero(s) for s in exact + inexact]
    for k, name in enumerate(("exact 2x3x5", "exact 16")):
        sets += _grids(by_name[name], k)
    assert len({s.name for s in sets}) == len(sets)
    return tuple(sets)


def rem_args(acc, tie=None):
    """The special rems / targets of routines 2 and 3 for rays whose whole optical depth (density length) is acc (float32): 0, the
    smallest denormal, acc / 2, acc exactly, its two neighbours, +inf.  tie: the optical depth up to the parameter tie_t, where the rays
    aimed at a grid vertex meet two or three planes at once — that depth and its two neighbours put the flight's event at the tie itself
    (the order of the steps at a tie shows nowhere else: the cell between them has a segment of length 0)."""
    acc = np.asarray(acc, np.float32)
    full = lambda v: np.full(acc.shape, v, np.float32)
    down, up = (lambda a: np.nextafter(a, np.float32(-np.inf)).astype(np.float32)), (lambda a: np.nextafter(a, np.float32(np.inf)).astype(np.float32))
    out = (("0", full(0.0)), ("2^-149", full(2.0 ** -149)), ("acc / 2", (acc * np.float32(0.5)).astype(np.float32)), ("acc", acc.copy()),
           ("acc-", down(acc)), ("acc+", up(acc)), ("+inf", full(np.inf)))
    if tie is not None:
        tie = np.asarray(tie, np.float32)
        out += (("acc(tie)", tie.copy()), ("acc(tie)-", down(tie)), ("acc(tie)+", up(tie)))
    return out


# ---- routine 0: rays against the three regions -------------------------------------------------------------------------------------------
ALL_SPACE = dict(sigma_t=1.0)


def exact_cases(one):
    """test_lit_fuzz_gloss_medium.test_intervals_exact_cases with `one` in the place of its _one: its hand-computed values asserted on
    whatever `one(medium, o, d, t_end)` returns as (hit, t0, t1)."""
    old = gm._one
    gm._one = one
    try:
        gm.test_intervals_exact_cases()
    finally:
        gm._one = old


@functools.lru_cache(maxsize=None)
def exact_case_rays():
    """Every ray test_intervals_exact_cases asks for, in its order: a tuple of (medium, o, d, t_end)."""
    seen = []

    def record(medium, o, d, t_end=gm.INF):
        seen.append((medium, tuple(o), tuple(d), float(t_end)))
        return old(medium, o, d, t_end)
    old = gm._one
    exact_cases(record)
    assert len(seen) >= 25, len(seen)
    return tuple(seen)


def _faces_and_tangents():
    rng = np.random.default_rng([39, 900])
    lo, hi = np.array(gm.BOX["box"][:3]), np.array(gm.BOX["box"][3:])
    o, d = [], []
    for k in range(3):          # origins exactly on a face: directions into the box, out of it, and along the face (d_k == 0, then -0)
        for face in (lo[k], hi[k]):
            for r in range(40):
                p = lo + rng.random(3) * (hi - lo)
                p[k] = face
                v = rng.normal(size=3)
                if r % 4 == 2:
                    v[k] = 0.0
                if r % 4 == 3:
                    v[k] = -0.0
                o.append(p)
                d.append(v)
    box = (np.array(o, np.float32), np.array(d, np.float32))
    c, R = np.array(gm.BALL["ball"][:3]), gm.BALL["ball"][3]
    o, d = [], []
    for i in range(3):          # tangents from exactly representable numbers, and their two neighbours across the tangent
        for sign in (-1.0, 1.0):
            for j in range(3):
                if j == i:
                    continue
                for along in (-1.0, 1.0):
                    for scale in (1.0, 0.5, 3.0):
                        for nudge in (0, -1, 1):
                            p = c.astype(np.float32).copy()
                            p[i] = np.float32(c[i] + sign * R)
                            if nudge:
                                p[i] = np.nextafter(p[i], np.float32(nudge * np.inf))
                            p[j] = np.float32(c[j] - along * 4.0)
                            v = np.zeros(3, np.float32)
                            v[j] = along * scale
                            o.append(p)
                            d.append(v)
    return box, (np.array(o, np.float32), np.array(d, np.float32))


@functools.lru_cache(maxsize=None)
def interval_sets():
    """Routine 0's rays: a tuple of (name, medium, o, d, t_end)."""
    sets = []
    for region in ("box", "ball", "all space"):
        rng = np.random.default_rng([26, len(region)])          # test_intervals_against_float64's generator and regions
        if region == "box":
            lo, hi = np.array(gm.BOX["box"][:3]), np.array(gm.BOX["box"][3:])
            centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo) / 2)
        else:
            centre, radius = np.array(gm.BALL["ball"][:3]), gm.BALL["ball"][3]
        o, d, t_end = gm._random_rays(rng, centre, radius, INTERVAL_RAYS)
        d[np.abs(d).sum(1) == 0] = 1.0
        sets.append((region, gm.BOX if region == "box" else gm.BALL if region == "ball" else ALL_SPACE, o, d, t_end))
    (bo, bd), (to, td) = _faces_and_tangents()
    for name, medium, o, d in (("origins on a face", gm.BOX, bo, bd), ("tangents to the ball", gm.BALL, to, td)):
        both = np.concatenate([o, o]), np.concatenate([d, d])
        t_end = np.concatenate([np.full(len(o), np.inf, np.float32), np.full(len(o), 2.0, np.float32)])
        sets.append((name, medium, both[0], both[1], t_end))
    for k, (medium, o, d, t_end) in enumerate(exact_case_rays()):
        sets.append((f"exact case {k}", medium if medium is not None else dict(sigma_t=0.0), np.array([o], np.float32), np.array([d], np.float32),
                     np.array([t_end], np.float32)))
    return tuple(sets)


# ---- the passes: one routine over one set with one argument, and the CPU statement's columns in the device hook's layout -----------------
# the columns of a routine, in the order of the hook's words (eight per ray; the rest 0)
COLUMNS = {0: ("hit", "t0", "t1"), 1: ("hit", "acc", "cells", "tr"), 2: ("hit", "event", "v", "cells"),
           3: ("hit", "event", "t", "A", "cells", "tr0", "tr1", "tr2"), 4: ("hit", "event", "t", "E", "cells"), 5: ("pl", "cells"), 6: ("hit", "G", "cells")}
INTEGER_COLUMNS = ("hit", "event", "cells")


class Pass(NamedTuple):
    label: str
    routine: int
    medium: dict
    density: object          # None: the homogeneous base (routines 0, 3 and 4)
    source: int
    heat: object
    o: np.ndarray
    d: np.ndarray
    t_end: np.ndarray
    arg: np.ndarray
    want: np.ndarray          # (m, 8) uint32: the CPU statement's columns as the hook writes them


def _words(routine, **cols):
    m = len(next(iter(cols.values())))
    out = np.zeros((m, 8), np.uint32)
    assert tuple(cols) == COLUMNS[routine], (routine, tuple(cols))
    for k, (name, c) in enumerate(cols.items()):
        c = np.ascontiguousarray(c)
        if name in INTEGER_COLUMNS:
            out[:, k] = c.astype(np.int32).view(np.uint32)
        else:
            assert c.dtype == np.float32, (name, c.dtype)
            out[:, k] = c.view(np.uint32)
    return out


def floats_of(routine, words):
    """The float columns of a routine's words, as a dict of float32 arrays."""
    return {name: np.ascontiguousarray(words[:, k]).view(np.float32) for k, name in enumerate(COLUMNS[routine]) if name not in INTEGER_COLUMNS}


def _random_args(label, m):
    return np.random.default_rng([39, sum(map(ord, label))]).uniform(0.05, 1.6, m).astype(np.float32)


def _homogeneous_passes(label, medium, o, d, t_end):
    """Routines 3 and 4 on the homogeneous base."""
    import chroma_reference as cr
    import glow_reference as gr
    zero = np.zeros(len(o), np.float32)
    A = cr.flights(medium, None, TINT, o, d, t_end, np.inf)["A"]
    for name, R in rem_args(A) + (("random", (np.where(np.isfinite(A), A, 1.0) * _random_args(label, len(o))).astype(np.float32)),):
        f = cr.flights(medium, None, TINT, o, d, t_end, R)
        yield Pass(f"{label}: chroma_flight, homogeneous, R = {name}", 3, medium, None, 0, None, o, d, t_end, R,
                   _words(3, hit=f["hit"], event=f["event"], t=f["t"], A=f["A"], cells=f["cells"], tr0=f["tr"][:, 0].copy(), tr1=f["tr"][:, 1].copy(),
                          tr2=f["tr"][:, 2].copy()))
    for name, u in tuple((n, zero + np.float32(v)) for n, v in U_ARGS) + (("random", np.minimum(_random_args(label, len(o)) / np.float32(1.6), np.float32(1.0))),):
        f = gr.flights(medium, None, o, d, t_end, u)
        yield Pass(f"{label}: glow_flight, homogeneous, u = {name}", 4, medium, None, 0, None, o, d, t_end, u,
                   _words(4, hit=f["hit"], event=f["event"], t=f["t"], E=f["E"], cells=f["cells"]))


def walk_passes(s):
    """Every pass of routines 1 … 6 over the RaySet s."""
    import chroma_reference as cr
    import glow_reference as gr
    import glow_sample_reference as gsr
    import volume_reference as vr
    m = len(s.o)
    zero = np.zeros(m, np.float32)
    inf = np.full(m, np.inf, np.float32)
    w = vr.walks(s.medium, s.density, s.o, s.d, s.t_end)
    w_inf = vr.walks(s.medium, s.density, s.o, s.d, inf)
    for name, t_end, ww in (("", s.t_end, w), (", t_end = inf", inf, w_inf)):
        yield Pass(f"{s.name}: volume_walk<false>{name}", 1, s.medium, s.density, 0, None, s.o, s.d, t_end, zero,
                   _words(1, hit=ww["hit"], acc=ww["acc"], cells=ww["cells"], tr=ww["tr"]))
    t_tie = np.minimum(s.t_end, np.float32(s.tie_t)).astype(np.float32)
    for name, rem in rem_args(w["acc"], vr.walks(s.medium, s.density, s.o, s.d, t_tie)["acc"]) + (("random", (w["acc"] * _random_args(s.name, m)).astype(np.float32)),):
        f = vr.walks(s.medium, s.density, s.o, s.d, s.t_end, rem=rem)
        v = np.where(f["event"] == 1, f["t_event"], f["rem_left"]).astype(np.float32)
        yield Pass(f"{s.name}: volume_walk<true>, rem = {name}", 2, s.medium, s.density, 0, None, s.o, s.d, s.t_end, rem,
                   _words(2, hit=f["hit"], event=f["event"], v=v, cells=f["flight_cells"]))
    A = cr.flights(s.medium, s.density, TINT, s.o, s.d, s.t_end, np.inf)["A"]
    A_tie = cr.flights(s.medium, s.density, TINT, s.o, s.d, t_tie, np.inf)["A"]
    for name, R in rem_args(A, A_tie) + (("random", (A * _random_args(s.name + "R", m)).astype(np.float32)),):
        f = cr.flights(s.medium, s.density, TINT, s.o, s.d, s.t_end, R)
        yield Pass(f"{s.name}: chroma_flight, grid, R = {name}", 3, s.medium, s.density, 0, None, s.o, s.d, s.t_end, R,
                   _words(3, hit=f["hit"], event=f["event"], t=f["t"], A=f["A"], cells=f["cells"], tr0=f["tr"][:, 0].copy(), tr1=f["tr"][:, 1].copy(),
                          tr2=f["tr"][:, 2].copy()))
    us = tuple((n, zero + np.float32(v)) for n, v in U_ARGS) + (("random", np.minimum(_random_args(s.name + "u", m) / np.float32(1.6), np.float32(1.0))),)
    for source in (0, 1, 2):
        heat = s.heat if source == 2 else None
        for name, u in us:
            f = gr.flights(s.medium, s.density, s.o, s.d, s.t_end, u, source, heat)
            yield Pass(f"{s.name}: glow_flight, grid, source {source}, u = {name}", 4, s.medium, s.density, source, heat, s.o, s.d, s.t_end, u,
                       _words(4, hit=f["hit"], event=f["event"], t=f["t"], E=f["E"], cells=f["cells"]))
        if source != 1:          # (the sampler of source 1 over a grid with nothing in it is empty: glow_pl is never called on one)
            pl = gsr.pl(s.medium, s.density, s.o, s.d, source, heat)[0]
            yield Pass(f"{s.name}: glow_pl, source {source}", 5, s.medium, s.density, source, heat, s.o, s.d, inf, zero, _words(5, pl=pl, cells=w_inf["cells"]))
        G, _, series, closed = gsr.line(s.medium, s.density, s.o, s.d, s.t_end, source, heat)
        yield Pass(f"{s.name}: glow_line, source {source} ({series} cells by the series, {closed} by the closed form)", 6, s.medium, s.density, source, heat, s.o,
                   s.d, s.t_end, zero, _words(6, hit=w["hit"], G=G, cells=w["cells"]))
    yield from _homogeneous_passes(s.name, s.medium, s.o, s.d, s.t_end)


def interval_passes():
    """Routine 0 over interval_sets(), and routines 3 and 4 on the homogeneous base over its three random sets (the ball, and all space with
    its A = +inf, among them)."""
    import medium_reference as mr
    for name, medium, o, d, t_end in interval_sets():
        hit, t0, t1 = mr.intervals(medium, o, d, t_end)
        t0, t1 = np.where(hit == 1, t0, np.float32(0.0)).astype(np.float32), np.where(hit == 1, t1, np.float32(0.0)).astype(np.float32)
        yield Pass(f"{name}: medium_interval", 0, medium, None, 0, None, o, d, t_end, np.zeros(len(o), np.float32), _words(0, hit=hit, t0=t0, t1=t1))
        if name in ("box", "ball", "all space"):
            yield from _homogeneous_passes(name, medium, o, d, t_end)
