"""The light-sampling device routines against the CPU restatements, vertex by vertex: light_sample on the four emitter
tables and on the environment under the three Pb kinds, light_emitted and light_miss with both carries, nee_pick / tree_pick / tree_pmf /
emit_find / nee_find, gloss_pg and PbPhase — the inline functions the render kernels call, run by the developer library's
rt_debug_light_vertices over tests/light_vertex_cases.py's vertices, one vertex per lane.  Every word of every routine on every vertex
equals the CPU statement, compared as uint32: no tolerance, no vertex left out.  Not collected by the normal test run (the file name does
not match test_*.py): tests/test_light_vertices.py runs it in one child process with RTP_AMD_LIB pointing at the developer library."""
import collections
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import emit_reference as emr
import gloss_reference as glr
import light_vertex_cases as lc
import medium_reference as mr
import rtp_bindings as rb
import tree_reference as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def libraries():
    """The four restatements, compiled side by side."""
    with ThreadPoolExecutor(4) as pool:
        list(pool.map(lambda m: m.lib(), (emr, tr, glr, mr)))


def _lib():
    lib = rb.amd_lib()
    lib.rt_debug_light_vertices.argtypes = [C.c_void_p, C.POINTER(rb.CameraData), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 7
    lib.rt_debug_light_vertices.restype = C.c_int
    lib.rt_get_last_error_string.restype = C.c_char_p
    return lib


class Objects:
    """The device objects of the passes: a DeviceScene per scene and an Env per environment, made once and closed together."""

    def __init__(self):
        self.scenes, self.envs = {}, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = rb.DeviceScene(lc.scene(name), device=0)
        return self.scenes[name]

    def env(self, which):
        if which is None:
            return None
        if which not in self.envs:
            self.envs[which] = rb.Env(lc.environment(which)[0])
        return self.envs[which]

    def close(self):
        for e in self.envs.values():
            e.close()
        for s in self.scenes.values():
            s.close()


def params_of(p):
    """(rt_nee_params, rt_env_params) of a pass: the glossy switch is on where the Pb kind needs it, and off elsewhere."""
    nee = rb.nee_params(mis=p.mis, sample_planes=p.planes, select=p.select, glossy=1 if p.pb == 1 else 0)
    ep = rb.env_params(**dict(p.env_params, glossy=1 if p.pb == 1 else 0)) if p.env_params is not None else rb.env_params()
    return nee, ep


def run(lib, objects, p, routine=None, pb=None, n=None):
    """One pass on the device → (status, (m, 16) uint32, the seconds the call took)."""
    x, nv, v, s, seed, ab = glr.vertex_arrays(p.x, p.nv, p.v, p.s, p.seed, lc.AB)
    nee, ep = params_of(p)
    env = objects.env(p.env)
    cam = lc.camera(p.scene)
    out = np.full((len(x), 16), 0xdeadbeef, np.uint32)
    t0 = time.perf_counter()
    st = lib.rt_debug_light_vertices(objects.scene(p.scene)._h, C.byref(cam), C.byref(nee), env._h if env is not None else None, C.byref(ep),
                                     p.routine if routine is None else routine, p.pb if pb is None else pb, len(x) if n is None else n, x.ctypes.data,
                                     nv.ctypes.data, v.ctypes.data, s.ctypes.data, seed.ctypes.data, ab.ctypes.data, out.ctypes.data)
    return st, out, time.perf_counter() - t0


class Tally:
    """What was compared, and where the two sides differ: routine and column, the class, and the first differing vertex of each."""

    def __init__(self):
        self.vertices = self.words = self.calls = self.nan_words = 0
        self.seconds = 0.0
        self.differ = collections.Counter()          # (routine, column) → vertices
        self.classes = collections.Counter()          # (routine, class) → vertices
        self.first = {}                               # (routine, column) → (label, vertex, device words, CPU words)
        self.tables = set()

    def compare(self, p, got, want):
        self.calls += 1
        self.vertices += len(p.x)
        cols = lc.COLUMNS[p.routine]
        self.words += len(p.x) * len(cols)
        self.tables.add((p.routine, p.pb, p.select, p.planes, p.mis, p.env))
        f = want[:, list(lc.FLOAT_COLUMNS[p.routine])].view(np.float32)
        self.nan_words += int(np.isnan(f).sum())
        bad = got != want
        if not bad.any():
            return
        cls = p.cls if isinstance(p.cls, np.ndarray) else np.full(len(p.x), p.cls)
        for c in cls[bad.any(1)]:
            self.classes[p.routine, str(c)] += 1
        for k in np.flatnonzero(bad.any(0)):
            name = cols[k] if k < len(cols) else f"word {k} (not named by the routine)"
            self.differ[p.routine, name] += int(bad[:, k].sum())
            if (p.routine, name) not in self.first:
                i = int(np.flatnonzero(bad[:, k])[0])
                self.first[p.routine, name] = (p.label, i, [hex(w) for w in got[i, :len(cols)]], [hex(w) for w in want[i, :len(cols)]])

    def report(self, what):
        print(f"LIGHT VERTICES {what}: {self.calls} hook calls, {self.vertices} vertices, {self.words} words compared, {sum(self.differ.values())} differ "
              f"({self.nan_words} of the CPU's words are NaN); {len(self.tables)} (routine, pb, select, planes, mis, env) combinations; device calls {self.seconds:.2f} s")
        for (routine, name), k in sorted(self.differ.items()):
            label, i, g, w = self.first[routine, name]
            print(f"  differ: routine {routine}, column {name}: {k} vertices; first: {label}, vertex {i}\n    device {g}\n    CPU    {w}")
        for (routine, name), k in self.classes.most_common():
            print(f"  class with differing vertices: routine {routine}, {name}: {k}")
        assert not self.differ, f"{len(self.differ)} (routine, column) pairs differ from the CPU statement, e.g. {sorted(self.differ.items())[:6]}"


def test_this_is_the_developer_library_with_the_light_hook():
    lib = rb.amd_lib()
    assert b"dev=1" in lib.rt_version_string() and hasattr(lib, "rt_debug_light_vertices")


def test_hook_refuses_bad_arguments_before_any_launch():
    """What a routine would index by is checked on the host: a code that names no primitive, an entry outside the tree's table, a vertex
    that is not finite, a Pb kind no call of these parameters runs."""
    lib, objects = _lib(), Objects()
    try:
        P = {p.routine: p for p in lc.pick_passes("panel box") if p.select == 1 and p.planes == 1 and p.cls.startswith("tree")}
        P.update({p.routine: p for p in lc.found_passes("lamp")[:1]})
        P.update({p.routine: p for p in lc.env_passes() if p.routine == 1 and p.pb == 0})
        small = {r: p._replace(x=p.x[:8], nv=p.nv[:8], v=p.v[:8], s=p.s[:8], seed=p.seed[:8]) for r, p in P.items()}
        assert run(lib, objects, small[4])[0] == 0 and run(lib, objects, small[2])[0] == 0 and run(lib, objects, small[1])[0] == 0
        assert run(lib, objects, small[4], routine=6)[0] == 1 and run(lib, objects, small[4], routine=-1)[0] == 1
        assert run(lib, objects, small[4], pb=1)[0] == 1 and run(lib, objects, small[4], pb=3)[0] == 1 and run(lib, objects, small[4], n=0)[0] == 1
        n_entries = len(emr.table(lc.scene("panel box"), 1)[0])
        for e in (-1.0, float(n_entries), 1e30):
            bad = small[4]._replace(nv=np.array([[e, 0, 0]] * 8, np.float32))
            assert run(lib, objects, bad)[0] == 1, e
        d = lc.scene("lamp").desc
        for code in (2 * d.num_spheres, 1, 0xffffffff, 0x80000000):          # one sphere too many, a plane of a scene without planes, -1, int min
            bad = small[2]._replace(seed=np.full(8, code, np.uint32))
            assert run(lib, objects, bad)[0] == 1, code
        for q in (np.inf, np.nan):
            bad = small[2]._replace(x=np.full((8, 3), q, np.float32))
            assert run(lib, objects, bad)[0] == 1
        assert run(lib, objects, small[1]._replace(env=None))[0] == 1, "the environment's routines need one"
        # pb = 1 with the light's glossy switch off: no call of these parameters runs PbGlossy
        x, nv, v, s, seed, ab = glr.vertex_arrays(small[1].x, small[1].nv, small[1].v, small[1].s, small[1].seed, lc.AB)
        nee, ep = rb.nee_params(glossy=0), rb.env_params(glossy=0)
        out = np.zeros((8, 16), np.uint32)
        cam = lc.camera("lamp")
        args = (8, x.ctypes.data, nv.ctypes.data, v.ctypes.data, s.ctypes.data, seed.ctypes.data, ab.ctypes.data, out.ctypes.data)
        assert lib.rt_debug_light_vertices(objects.scene("lamp")._h, C.byref(cam), C.byref(nee), objects.env("two")._h, C.byref(ep), 1, 1, *args) == 1
        assert lib.rt_debug_light_vertices(objects.scene("lamp")._h, C.byref(cam), C.byref(nee), None, C.byref(ep), 0, 1, *args) == 1
        assert lib.rt_debug_light_vertices(objects.scene("lamp")._h, C.byref(cam), C.byref(nee), None, C.byref(ep), 0, 0, *args) == 0
    finally:
        objects.close()


def test_every_word_of_every_routine_on_every_vertex():
    lib, objects, tally = _lib(), Objects(), Tally()
    t0 = time.perf_counter()
    passes = lc.all_passes()
    t_cases = time.perf_counter() - t0
    t_cpu = 0.0
    try:
        for p in passes:
            assert len(p.x) <= lc.MAX_CALL
            t0 = time.perf_counter()
            want, _ = lc.reference(p, tallies=False)
            t_cpu += time.perf_counter() - t0
            st, got, dt = run(lib, objects, p)
            assert st == 0, (p.label, lib.rt_get_last_error_string().decode())
            tally.seconds += dt
            tally.compare(p, got, want)
    finally:
        objects.close()
    print(f"LIGHT VERTICES the vertex sets took {t_cases:.1f} s to make, the CPU statement {t_cpu:.1f} s")
    # the four tables, both mis modes and the three Pb kinds were all run
    combos = tally.tables
    assert {(s, pl) for r, pb, s, pl, mis, env in combos if r == 0} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(pb, mis) for r, pb, s, pl, mis, env in combos if r == 0} == {(pb, mis) for pb in (0, 1, 2) for mis in (0, 1)}
    assert {r for r, *_ in combos} == {0, 1, 2, 3, 4, 5} and {pb for r, pb, *_ in combos if r == 1} == {0, 1, 2}
    assert tally.vertices >= 1000000
    tally.report("all routines")
