"""The fog family's device routines against the CPU restatements, ray by ray: medium_interval, volume_walk in its three
instantiations, chroma_flight / chroma_tr, glow_flight, glow_pl and glow_line — the inline functions the render kernels call, run by the
developer library's rt_debug_fog_rays over tests/fog_ray_cases.py's rays, one ray per lane.  Every column of every routine on every ray
equals the CPU statement bit for bit, compared as uint32: no tolerance, no ray left out.  Not collected by the normal test run (the file
name does not match test_*.py): tests/test_fog_rays.py runs it in one child process with RTP_AMD_LIB pointing at the developer library."""
import collections
import ctypes as C
import time

import numpy as np
import pytest

import fog_ray_cases as fc
import medium_reference as mr
import rtp_bindings as rb
import test_volume as tv

pytestmark = pytest.mark.gpu


def _lib():
    lib = rb.amd_lib()
    lib.rt_debug_fog_rays.argtypes = [C.c_int32, C.POINTER(rb.MediumParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    lib.rt_debug_fog_rays.restype = C.c_int
    lib.rt_get_last_error_string.restype = C.c_char_p
    return lib


class Grids:
    """The device objects of a set's passes: a Volume per grid and a GlowSampler per (source, heat), made once and closed together."""

    def __init__(self):
        self.volumes, self.samplers = {}, {}

    def volume(self, grid):
        if grid is None:
            return None
        key = id(grid)
        if key not in self.volumes:
            self.volumes[key] = (rb.Volume(grid), grid)
        return self.volumes[key][0]

    def sampler(self, density, source, heat):
        key = (id(density), source, id(heat))
        if key not in self.samplers:
            self.samplers[key] = rb.GlowSampler(self.volume(density), source, self.volume(heat))
        return self.samplers[key]

    def close(self):
        for s in self.samplers.values():
            s.close()
        for v, _ in self.volumes.values():
            v.close()


def _handle(x):
    return x._h if x is not None else None


def run(lib, grids, p):
    """One pass on the device → (m, 8) uint32, and the seconds the call took."""
    medium = mr.medium_struct(p.medium)
    medium.struct_bytes = C.sizeof(rb.MediumParams)
    tint = np.array(fc.TINT, np.float32)
    out = np.empty((len(p.o), 8), np.uint32)
    volume, heat = grids.volume(p.density), grids.volume(p.heat)
    sampler = grids.sampler(p.density, p.source, p.heat) if p.routine == 5 else None
    t_end, arg = np.ascontiguousarray(p.t_end, np.float32), np.ascontiguousarray(p.arg, np.float32)
    t0 = time.perf_counter()
    st = lib.rt_debug_fog_rays(p.routine, C.byref(medium), _handle(volume), p.source, _handle(heat), _handle(sampler), tint.ctypes.data, len(p.o),
                               p.o.ctypes.data, p.d.ctypes.data, t_end.ctypes.data, arg.ctypes.data, out.ctypes.data)
    dt = time.perf_counter() - t0
    assert st == 0, (p.label, lib.rt_get_last_error_string().decode())
    return out, dt


class Tally:
    """What was compared, and where the two sides differ."""

    def __init__(self):
        self.rays = self.columns = self.calls = 0
        self.seconds = 0.0
        self.differ = collections.Counter()          # (pass, column) → rays
        self.classes = collections.Counter()          # the class of a differing ray → rays

    def compare(self, p, got, kind=None):
        self.calls += 1
        self.rays += len(p.o)
        self.columns += len(p.o) * len(fc.COLUMNS[p.routine])
        bad = got != p.want
        assert not got[:, len(fc.COLUMNS[p.routine]):].any(), p.label
        for k, name in enumerate(fc.COLUMNS[p.routine]):
            if bad[:, k].any():
                self.differ[p.label, name] += int(bad[:, k].sum())
        if kind is not None and bad.any():
            for c in kind[bad.any(1)]:
                self.classes[tv.WALK_CLASSES[c][0]] += 1

    def report(self, what):
        print(f"FOG RAYS {what}: {self.calls} calls, {self.rays} rays, {self.columns} columns compared, {sum(self.differ.values())} differ; "
              f"device calls {self.seconds:.2f} s")
        for (label, name), k in sorted(self.differ.items())[:40]:
            print(f"  differ: {label}, column {name}: {k} rays")
        for name, k in self.classes.most_common():
            print(f"  class with differing rays: {name}: {k}")
        assert not self.differ, f"{len(self.differ)} (pass, column) pairs differ from the CPU statement, e.g. {sorted(self.differ.items())[:6]}"


def test_this_is_the_developer_library_with_the_fog_hook():
    lib = rb.amd_lib()
    assert b"dev=1" in lib.rt_version_string() and hasattr(lib, "rt_debug_fog_rays")


def test_hook_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    s = fc.walk_sets()[1]
    grids = Grids()
    try:
        medium = mr.medium_struct(s.medium)
        medium.struct_bytes = C.sizeof(rb.MediumParams)
        ball = mr.medium_struct(dict(sigma_t=1.0, ball=(0, 0, 0, 1)))
        ball.struct_bytes = C.sizeof(rb.MediumParams)
        v, h = grids.volume(s.density), grids.volume(s.heat)
        other = grids.volume(np.ones((2, 2, 2), np.float32))
        tint = np.array(fc.TINT, np.float32)
        n = 4
        o, d, t, out = s.o[:n].copy(), s.d[:n].copy(), s.t_end[:n].copy(), np.zeros((n, 8), np.uint32)
        rays = (n, o.ctypes.data, d.ctypes.data, t.ctypes.data, t.ctypes.data, out.ctypes.data)

        def call(routine, m=medium, vol=v, source=0, heat=None, sampler=None, tn=tint.ctypes.data, r=rays):
            return lib.rt_debug_fog_rays(routine, C.byref(m), _handle(vol), source, _handle(heat), _handle(sampler), tn, *r)
        assert call(-1) == 1 and call(7) == 1
        assert call(1, r=(0,) + rays[1:]) == 1 and call(1, r=rays[:5] + (None,)) == 1 and call(1, r=(n, None) + rays[2:]) == 1
        assert call(1, vol=None) == 1 and call(2, vol=None) == 1 and call(5, vol=None) == 1 and call(6, vol=None) == 1
        assert call(1, m=ball) == 1, "a volume needs the box"
        assert call(4, source=3) == 1 and call(4, vol=None, source=1) == 1 and call(4, source=2) == 1 and call(4, source=0, heat=h) == 1
        assert call(4, source=2, heat=other) == 1, "the heat grid's dimensions"
        assert call(5) == 1, "glow_pl needs a sampler"
        assert call(5, sampler=grids.sampler(s.density, 2, s.heat)) == 1, "a sampler of another source"
        assert call(3, tn=None) == 1
        assert call(0, vol=None) == 0 and call(1) == 0 and call(5, sampler=grids.sampler(s.density, 0, None)) == 0
    finally:
        grids.close()


def test_intervals_on_the_device():
    """medium_interval on the three regions, and chroma_flight / glow_flight on the homogeneous base over the same rays; then
    test_intervals_exact_cases' hand-computed values on the device's own output."""
    lib, grids, tally = _lib(), Grids(), Tally()
    exact = {}
    for p in fc.interval_passes():
        got, dt = run(lib, grids, p)
        tally.seconds += dt
        tally.compare(p, got)
        if p.label.startswith("exact case"):
            exact[int(p.label.split(":")[0].split()[-1])] = got[0]
    calls = iter(range(len(fc.exact_case_rays())))

    def one(medium, o, d, t_end=float("inf")):
        k = next(calls)
        assert fc.exact_case_rays()[k] == (medium, tuple(o), tuple(d), float(t_end))
        w = exact[k]
        return int(w[0]), float(w[1:2].view(np.float32)[0]), float(w[2:3].view(np.float32)[0])
    # (an empty interval's t0 and t1 are written as 0 here; the hand-computed cases read them only where hit == 1)
    fc.exact_cases(one)
    assert next(calls, None) is None
    tally.report("intervals")


def test_every_column_of_every_walk_routine_on_every_ray():
    """Routines 1 … 6 over walk_sets().  The two hand-kept copies of the walk are also compared directly: volume_cells (under glow_pl and
    glow_line) reports volume_walk's cells on the same ray and t_end, and the three flights visit the same cells wherever none of them
    stopped at an event."""
    lib, tally = _lib(), Tally()
    copies = flights = 0
    for s in fc.walk_sets():
        grids = Grids()
        got = {}
        try:
            for p in fc.walk_passes(s):
                g, dt = run(lib, grids, p)
                tally.seconds += dt
                tally.compare(p, g, s.kind)
                got[p.label] = (p, g)
        finally:
            grids.close()
        walk = {name: g for name, (p, g) in got.items() if p.routine == 1}
        cells_end, cells_inf = walk[f"{s.name}: volume_walk<false>"][:, 2], walk[f"{s.name}: volume_walk<false>, t_end = inf"][:, 2]
        none = {}          # per flight routine on the grid: the cells of the passes' rays that had no event, by the argument +inf / u = 0
        for name, (p, g) in got.items():
            if p.routine == 5:
                assert (g[:, 1] == cells_inf).all(), name
                copies += len(g)
            if p.routine == 6:
                assert (g[:, 2] == cells_end).all() and (g[:, 0] == walk[f"{s.name}: volume_walk<false>"][:, 0]).all(), name
                copies += len(g)
            if p.density is not None and p.routine in (2, 3, 4):
                cells = g[:, {2: 3, 3: 4, 4: 4}[p.routine]]
                no_event = (g[:, 0] == 1) & (g[:, 1] == 0)
                # a flight without an event walks the whole interval: volume_walk<false>'s cells
                assert (cells[no_event] == cells_end[no_event]).all(), name
                none.setdefault(p.routine, []).append((no_event, cells))
        for a, ca in none[2]:
            for r in (3, 4):
                for b, cb in none[r]:
                    both = a & b
                    assert (ca[both] == cb[both]).all(), (s.name, r)
                    flights += int(both.sum())
    print(f"FOG RAYS the two copies of the walk: {copies} rays with the same cells; flights without an event: {flights} ray pairs with the same cells")
    assert copies > 100000 and flights > 100000
    tally.report("walks")
