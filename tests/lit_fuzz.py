"""Random lit scenes for the light-sampling kernels (TEST INFRASTRUCTURE): scenes, environment maps, rotations, cameras and
lenses made deterministically from a seed and a trial index, the one large night scene, the dispatch rule of rt_capi.hip as a pure
function, and the parameter lists tests/test_lit_fuzz.py iterates over — on the CPU to show that every kernel is reached, and on the GPU to
reach them.

What a scene is made of follows the clauses of include/rtp_amd.h that no hand-made scene exercises: points inside an emissive sphere (a
dome), overlapping, concentric and touching emitters, coincident emissive planes, degenerate planes between table entries (gaps), an
emissive plane of an unsupported type, a DIFFUSE_LIGHT that emits nothing, scattering materials that emit, emit with zero channels and
weights over many decades.

DESIGN.md §27 adds, for the glossy (§23) and the medium (§25) kernels: gloss_case — a glossy twin of every trial —, fuzz_medium — one
medium per trial —, the glossy switches and the medium in the dispatch rule, and the call lists of tests/test_lit_fuzz_gloss_medium.py."""
import collections
import functools

import numpy as np

import emit_reference as emr
import rtp_bindings as rb
import tree_reference as tr

MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_LIGHT = 0, 1, 2, 3
RT_GLOSSY_MIN_FUZZ = 2.0 ** -10
QUAD, ELLIPSE, TRIANGLE, UNSUPPORTED = 0, 1, 2, 3

# material slots of a fuzz scene
(M_LAMB_A, M_LAMB_B, M_METAL, M_GLASS, M_LIGHT_A, M_LIGHT_B, M_LIGHT_GREEN, M_LAMB_GLOW, M_LIGHT_DARK, M_DOME, M_GROUND, M_FAINT) = range(12)
EMISSIVE = (M_LIGHT_A, M_LIGHT_B, M_LIGHT_GREEN, M_LAMB_GLOW)
DULL = (M_LAMB_A, M_LAMB_B, M_METAL, M_GLASS, M_LIGHT_DARK)

# eight scenes: trial = position in the list.  Trials 0, 3, 6 have the dome; 1, 4, 7 the overlapping group; even ones the ground
SEEDS = (2101, 2102, 2103, 2104, 2105, 2116, 2107, 2108)          # (2116 replaces 2106: test_lit_fuzz.py says why)
DARK_TRIAL = 5          # the trial whose dark twin (every emit zeroed: an empty table) the identity test runs
ENV_SIZES = (1, 2, 3, 5, 16, 37)


def material(kind, albedo=(0.5, 0.5, 0.5), emit=(0, 0, 0), fuzz=0.0, ir=1.5):
    m = rb.Material()
    m.type = kind
    m.fuzz = fuzz
    m.ir = ir
    for k in range(3):
        m.albedo.e[k] = albedo[k]
        m.emit.e[k] = emit[k]
    return m


def random_rot(rng):
    """A rotation matrix (rows: world → environment) from the QR of a normal matrix; det +1."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def random_env(rng, trial):
    """(n, n, 3) float32: n cycles through ENV_SIZES; for n >= 3 one whole row and every component below 0.3 are zero; for odd trials
    with n >= 5 the map is near-black but for one hot texel."""
    n = ENV_SIZES[trial % len(ENV_SIZES)]
    m = rng.uniform(0.0, 1.5, size=(n, n, 3))
    dark_row = -1
    if n >= 3:
        m[m < 0.3] = 0.0
        dark_row = int(rng.integers(0, n))
        m[dark_row] = 0.0
    if trial % 2 == 1 and n >= 5:
        m *= 0.05
        row, col = int(rng.integers(0, n)), int(rng.integers(0, n))
        m[(row + 1) % n if row == dark_row else row, col] = (300.0, 250.0, 200.0)          # (the row of weight 0 stays one)
    return m.astype(np.float32)


def random_lit_scene(rng, trial, dark=False, remat=None):
    """An rb.HostScene of 3 – 40 random spheres and 0 – 14 random planes (none on one trial in four), about a third of them emissive, plus
    what `trial` adds.  dark: the same scene with every emit zeroed — its emitter table is empty.  remat(spheres, planes, mats): called
    after the last draw from rng, it may re-material the lists in place (gloss_case's rule; it has no access to rng)."""
    u = rng.uniform
    mats = [None] * 12
    mats[M_LAMB_A] = material(MAT_LAMBERTIAN, u(0.2, 0.9, 3))
    mats[M_LAMB_B] = material(MAT_LAMBERTIAN, u(0.2, 0.9, 3))
    mats[M_METAL] = material(MAT_METAL, u(0.4, 0.9, 3), fuzz=float(u(0.0, 0.7)))
    mats[M_GLASS] = material(MAT_DIELECTRIC, ir=1.5)
    mats[M_LIGHT_A] = material(MAT_LIGHT, emit=u(0.5, 8.0, 3))
    mats[M_LIGHT_B] = material(MAT_LIGHT, emit=u(0.5, 8.0, 3))
    mats[M_LIGHT_GREEN] = material(MAT_LIGHT, emit=(0.0, float(u(0.5, 8.0)), 0.0))
    mats[M_LAMB_GLOW] = material(MAT_LAMBERTIAN, u(0.2, 0.8, 3), emit=u(0.2, 2.0, 3))
    mats[M_LIGHT_DARK] = material(MAT_LIGHT, emit=(0.0, 0.0, 0.0))
    mats[M_DOME] = material(MAT_LIGHT, emit=u(0.2, 1.0, 3))
    mats[M_GROUND] = material(MAT_LAMBERTIAN, (0.5, 0.5, 0.5))
    mats[M_FAINT] = material(MAT_LIGHT, emit=(0.5, 0.5, 0.5))

    def pick_material():
        return int(rng.choice(EMISSIVE)) if rng.random() < 1.0 / 3.0 else int(rng.choice(DULL))

    spheres = []
    for _ in range(int(rng.integers(3, 41))):
        spheres.append([*u(-5, 5, 3), 10.0 ** u(-1.3, 0.2), pick_material()])
    planes = []
    for _ in range(int(rng.integers(0, 15)) * (trial % 4 != 3)):
        mat = int(rng.choice(EMISSIVE)) if rng.random() < 0.4 else int(rng.choice(DULL))
        planes.append([*u(-5, 5, 3), *u(-3, 3, 3), *u(-3, 3, 3), mat, int(rng.integers(0, 3))])
    if trial % 2 == 0:
        spheres.append([0.0, -1006.0, 0.0, 1000.0, M_GROUND])
    if trial % 3 == 0:
        spheres.append([0.0, 0.0, 0.0, 40.0, M_DOME])
        if trial % 2 == 0:
            # weights over more than six decades: 1.5 * 0.01^2 beside the dome's >= 0.6 * 40^2, at a distance where its cone rounds away
            spheres.append([0.0, 30.0, 0.0, 0.01, M_FAINT])
    if trial % 3 == 1:
        c = u(-4, 4, 3)
        spheres.append([*c, 0.8, M_LIGHT_A])                                   # two overlapping emitters …
        spheres.append([c[0] + 0.7, c[1], c[2], 0.6, M_LIGHT_B])
        spheres.append([*c, 0.3, M_LIGHT_GREEN])                               # … a third, concentric inside the first
        d = u(-4, 4, 3)
        spheres.append([*d, 0.5, M_LAMB_A])                                    # a non-emitter and an emitter that touches it
        spheres.append([d[0], d[1] + 0.75, d[2], 0.25, M_LIGHT_A])
    if len(planes) >= 3:
        planes[1][6:9] = [2.0 * x for x in planes[1][3:6]]                     # u ∥ v: no area, so it is in no table …
        planes[1][9] = M_LIGHT_A                                               # … though it emits
        planes[0][9] = M_LIGHT_A
        planes[2] = list(planes[0])                                            # two coincident emissive planes
        planes[2][9] = M_LIGHT_B
    if len(planes) >= 5:
        planes[4][9], planes[4][10] = M_LIGHT_B, UNSUPPORTED                   # an emissive plane of a type the table does not take
    if dark:
        for m in mats:
            m.emit.e[0] = m.emit.e[1] = m.emit.e[2] = 0.0
    if remat is not None:
        remat(spheres, planes, mats)
    return rb.HostScene.from_arrays(np.array(spheres, np.float32), np.array(planes, np.float32).reshape(-1, 11), mats)


class Case:
    """One fuzz case: the scene and everything a call on it needs.  camera(w, h, spp, depth) → the open camera, close(…) → the camera at
    shutter close (None on the trials without motion); env: an (n, n, 3) map or None; rot: the 9 floats of rt_env_params.rot."""

    def __init__(self, trial, dark=False, remat=None):
        self.trial = trial
        self.seed = SEEDS[trial]
        rng = np.random.default_rng([self.seed, trial])
        self.host = random_lit_scene(rng, trial, dark, remat)
        d = rng.normal(size=3)
        d[1] = abs(d[1]) + 0.3
        self.eye = tuple(float(x) for x in 9.0 * d / np.linalg.norm(d))
        self.eye_close = tuple(float(x) for x in np.array(self.eye) + rng.uniform(-0.3, 0.3, 3))
        self.background = tuple(float(x) for x in rng.uniform(0.0, 0.3, 3))
        self.vfov = float(rng.uniform(30.0, 50.0))
        self.lens = (float(rng.uniform(0.05, 0.3)), 9.0)
        self.motion = trial % 2 == 1
        self.dome = trial % 3 == 0
        # the dome hides the sky, so the scenes under it have no environment
        self.env = None if self.dome else random_env(rng, trial)
        self.rot = tuple(float(x) for x in random_rot(rng).ravel())
        self.name = f"trial {trial} seed {self.seed}"

    def camera(self, w, h, spp, depth=50):
        return rb.make_camera(w, h, self.vfov, self.eye, (0, 0, 0), self.background, spp, depth)

    def close(self, w, h, spp, depth=50):
        return rb.make_camera(w, h, self.vfov, self.eye_close, (0, 0, 0), self.background, spp, depth) if self.motion else None

    def env_params(self, mode, scale=0.8):
        return dict(mode=mode, scale=scale, rot=self.rot)

    def lens_dict(self):
        return dict(lens_radius=self.lens[0], focus_distance=self.lens[1])

    def has_planes(self, sample_planes=1):
        """Does the table of sample_planes hold a plane?"""
        return bool(sample_planes) and bool((emr.table(self.host, 1)[0] == 1).any())

    def entries(self, sample_planes):
        return len(emr.table(self.host, sample_planes)[0])


@functools.lru_cache(maxsize=None)
def case(trial, dark=False):
    return Case(trial, dark)


TRIALS = tuple(range(len(SEEDS)))
ENV_TRIALS = tuple(t for t in TRIALS if t % 3 != 0)


def large_night_scene():
    """HostScene.rtiow(half_extent=40) with every eighth small sphere made a light, as test_light_tree.night_rtiow does it."""
    base = rb.HostScene.rtiow(half_extent=40)
    d = base.desc
    spheres, mats = [], []
    for i in range(d.num_spheres):
        s = d.spheres[i]
        m = d.materials[s.material_idx]
        if 0 < i < d.num_spheres - 3 and i % 8 == 5:
            m = material(MAT_LIGHT, emit=(6.0, 4.5, 3.0) if i % 16 == 5 else (1.5, 2.0, 3.0))
        spheres.append([s.center.e[0], s.center.e[1], s.center.e[2], s.radius, len(mats)])
        mats.append(rb.Material.from_buffer_copy(m))
    night = rb.HostScene.from_arrays(np.array(spheres, np.float32), np.zeros((0, 11), np.float32), mats)
    base.close()
    return night


@functools.lru_cache(maxsize=None)
def large():
    host = large_night_scene()
    t = tr.tree(host, 0)
    assert len(t["path"]) >= 512 and int(t["depth"].max()) >= 10, (len(t["path"]), int(t["depth"].max()))
    return host


def large_camera(w, h, spp, depth=50):
    return rb.make_camera(w, h, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), spp, depth)


FAINT_A, FAINT_B = (1e-42, 2e-42, 0.0), (3e-42, 0.0, 0.0)


def fallback_scene():
    """A crafted scene for the descent's fallback to q (no seed reaches it): a floor, a dome of weight 24 * 40^2, and two spheres whose
    weights — about 1e-42 — round to 0 in float32 next to it.  The split on x puts the two faint ones in one node, whose children's
    importances are 0 + 0."""
    mats = [material(MAT_LAMBERTIAN, (0.6, 0.6, 0.6)), material(MAT_LIGHT, emit=(8, 8, 8)), material(MAT_LIGHT, emit=FAINT_A),
            material(MAT_LIGHT, emit=FAINT_B)]
    sph = [[0, -100, 0, 100, 0], [5, 0, 0, 40, 1], [-0.6, 0.5, 0, 0.5, 2], [0.6, 0.5, 0, 0.5, 3]]
    return rb.HostScene.from_arrays(np.array(sph, np.float32), np.zeros((0, 11), np.float32), mats)


def fallback_camera(w, h, spp, depth=8):
    return rb.make_camera(w, h, 30.0, (0, 2, 6), (0, 0.5, 0), (0, 0, 0), spp, depth)


# ---- the dispatch rule of rt_capi.hip, once ---------------------------------------------------------------------------------------------
# entry points: the frame calls, their probes, and the adaptive call (which launches the frame kernel and its list variant)
NEE_FRAME, NEE_PROBE, ENV_FRAME, ENV_PROBE, LIT_FRAME, LIT_PROBE, LIT_ADAPTIVE = ("rt_render_nee", "rt_trace_samples_nee", "rt_render_env",
                                                                                 "rt_trace_samples_env", "rt_render_lit",
                                                                                 "rt_trace_samples_lit", "rt_render_lit_adaptive")


MEDIUM_FRAME, MEDIUM_PROBE = "rt_render_medium", "rt_trace_samples_medium"


def kernels_of(entry, lens=False, sample_planes=0, select=0, table_has_plane=False, table_entries=1, glossy_nee=0, glossy_env=0, medium_on=False,
               emitters=True, env=False):
    """The kernels a call launches, as a tuple of names with their template arguments: rt_capi.hip's rule.  lens: the call has a lens
    radius > 0 or a closing camera; table_has_plane: the two-kind table holds a plane; table_entries: the length of the table the
    call selects (0: the tree kernels are not used, rt_capi.hip's tree_on).  glossy_nee / glossy_env: rt_nee_params.glossy and
    rt_env_params.glossy; env: the call has an environment; emitters: rt_lit_params.sample_emitters (the lit and medium calls; off: the
    empty sphere-only table, with_emitter_table's first line); medium_on: sigma_t > 0 (the medium calls)."""
    planes = bool(sample_planes) and table_has_plane                       # emit_planes_on
    tree = select == 1 and table_entries > 0                               # tree_on
    if entry in (ENV_FRAME, ENV_PROBE):
        return (f"light_{'gloss_' if glossy_env else ''}{'render' if entry == ENV_FRAME else 'probe'}_kernel<EnvDev>",)
    table = ("TreeEmitTable" if planes else "TreeTable") if tree else ("EmitTable" if planes else "NeeTable")     # with_emitter_table
    if entry in (NEE_FRAME, NEE_PROBE):
        return (f"light_{'gloss_' if glossy_nee else ''}{'render' if entry == NEE_FRAME else 'probe'}_kernel<{table}>",)
    if not emitters:
        table = "NeeTable"
    args = f"<{'true' if lens else 'false'}, {table}>"
    gn, ge = bool(emitters and glossy_nee), bool(env and glossy_env)        # with_lit, with_medium_lit
    if entry in (MEDIUM_FRAME, MEDIUM_PROBE) and medium_on:                 # sigma_t > 0: the medium kernels whatever the switches are
        return (f"medium_{'render' if entry == MEDIUM_FRAME else 'probe'}_kernel{args}",)
    lit = "lit_gloss" if gn or ge else "lit"
    if entry in (LIT_FRAME, MEDIUM_FRAME):
        return (f"{lit}_render_kernel{args}",)
    if entry in (LIT_PROBE, MEDIUM_PROBE):
        return (f"{lit}_probe_kernel{args}",)
    assert entry == LIT_ADAPTIVE, entry
    return (f"{lit}_render_kernel{args}", f"{lit}_list_render_kernel{args}")


def all_kernels():
    """The light-sampling family: every instantiation rt_capi.hip can launch (34)."""
    tables = ("NeeTable", "EmitTable", "TreeTable", "TreeEmitTable")
    out = [f"light_{k}_kernel<{t}>" for t in tables + ("EnvDev",) for k in ("render", "probe")]
    out += [f"lit_{k}_kernel<{l}, {t}>" for k in ("render", "list_render", "probe") for l in ("true", "false") for t in tables]
    return sorted(out)


TABLES = ("NeeTable", "EmitTable", "TreeTable", "TreeEmitTable")


def all_gloss_kernels():
    """The glossy instantiations: 34."""
    out = [f"light_gloss_{k}_kernel<{t}>" for t in TABLES + ("EnvDev",) for k in ("render", "probe")]
    out += [f"lit_gloss_{k}_kernel<{l}, {t}>" for k in ("render", "list_render", "probe") for l in ("true", "false") for t in TABLES]
    return sorted(out)


def all_medium_kernels():
    """The medium instantiations: 16."""
    return sorted(f"medium_{k}_kernel<{l}, {t}>" for k in ("render", "probe") for l in ("true", "false") for t in TABLES)


# ---- the calls of the GPU tests: made here once, walked by the coverage test on the CPU and by the GPU tests ------------------------------
# test: which GPU test makes the call; lens: a lens radius and (on the trials with motion) a closing camera; env: None or the environment's
# mode; shard: None, or which of SHARDS a frame call uses
Call = collections.namedtuple("Call", "test entry trial lens planes select mis env shard")
MIS_PLANES_SELECT = tuple((mis, planes, select) for mis in (1, 0) for planes in (0, 1) for select in (0, 1))
PLANES_SELECT = tuple((planes, select) for planes in (0, 1) for select in (0, 1))
SHARDS = ((None, 0), (rb.Shard(4, 3, 2), 0), (None, 37))
ADAPTIVE_TRIALS = (1, 2, 4)


def _cells(test, trial, nee_entry, env_entry, lit_entry):
    c = case(trial)
    out = [Call(test, nee_entry, trial, False, planes, select, mis, None, None) for mis, planes, select in MIS_PLANES_SELECT]
    if c.env is not None:
        out += [Call(test, env_entry, trial, False, 0, 0, 1, mode, None) for mode in (1, 2)]
    for planes, select in PLANES_SELECT:
        for lens in (True, False):
            # the environment rides on one lens value per cell, alternating, so that every lit kernel meets it on some trial
            env = (1 if select else 2) if c.env is not None and lens == ((trial + planes + select) % 2 == 0) else None
            out.append(Call(test, lit_entry, trial, lens, planes, select, 1 if lens else 0, env, None))
    return out


def probe_calls(trial):
    return _cells("probes", trial, NEE_PROBE, ENV_PROBE, LIT_PROBE)


@functools.lru_cache(maxsize=None)
def _all_frame_calls():
    """The frame cells of every trial; each kernel's calls go through SHARDS in turn, so that every kernel meets all three."""
    turn, out = collections.Counter(), {}
    for t in TRIALS:
        out[t] = []
        for c in _cells("frames", t, NEE_FRAME, ENV_FRAME, LIT_FRAME):
            k = kernels_of_call(c)[0]
            out[t].append(c._replace(shard=turn[k] % 3))
            turn[k] += 1
    return out


def frame_calls(trial):
    return list(_all_frame_calls()[trial])


def adaptive_calls(trial):
    c = case(trial)
    return [Call("adaptive", LIT_ADAPTIVE, trial, lens, planes, select, 1, (1 if c.env is not None and lens else None), None)
            for lens in (False, True) for planes, select in PLANES_SELECT]


def large_calls():
    return [Call("large", NEE_PROBE, "large", False, 0, 1, 1, None, None), Call("large", NEE_FRAME, "large", False, 0, 0, 1, None, 0),
            Call("large", NEE_FRAME, "large", False, 0, 1, 1, None, 0), Call("large", LIT_FRAME, "large", True, 0, 1, 1, 1, 0)]


def calls():
    """Every call the GPU tests make on the light-sampling kernels."""
    out = []
    for t in TRIALS:
        out += probe_calls(t) + frame_calls(t)
    for t in ADAPTIVE_TRIALS:
        out += adaptive_calls(t)
    return out + large_calls()


def kernels_of_call(call):
    if call.trial == "large":
        return kernels_of(call.entry, call.lens, call.planes, call.select, False, len(tr.tree(large(), 0)["path"]))
    c = case(call.trial)
    has = c.has_planes(1)
    return kernels_of(call.entry, call.lens, call.planes, call.select, has, c.entries(1 if (call.planes and has) else 0))


# ---- a call's keywords, for the device and for the restatement ----------------------------------------------------------------------------
def reference_keywords(call, w, h, spp, depth):
    """tree_reference.trace / frame keywords of a lit or nee call (the camera apart)."""
    c = case(call.trial)
    kw = dict(select=call.select, nee_mis=call.mis, planes=call.planes)
    if call.lens:
        kw.update(lens=c.lens, cam_close=c.close(w, h, spp, depth))
    if call.env is not None:
        kw.update(rgb=c.env, env_params=c.env_params(call.env))
    return kw


def device_keywords(call, env, w, h, spp, depth):
    """DeviceScene.render_lit / trace_samples_lit keywords of a lit call; env: an rb.Env of the case's map (or None)."""
    c = case(call.trial)
    kw = dict(nee={"mis": call.mis, "sample_planes": call.planes, "select": call.select})
    if call.lens:
        kw.update(lens=c.lens_dict(), cam_close=c.close(w, h, spp, depth))
    if call.env is not None:
        kw.update(env=env, env_params=c.env_params(call.env))
    return kw


# ---- glossy twins and random media ---------------------------------------------------------------------------------------
# The twin of a trial: the same draws — geometry, emitter table, tree, camera, lens, map and rotation — with the non-emissive materials made
# METAL afterwards.  The fuzz values over the eight twins are exactly GLOSS_FUZZ: 0 and 2^-11 (mirrors for the switch), 2^-10 (the
# threshold itself: a glossy event), 0.05, 0.35, 1.0 (the boundary between pg's two forms) and 1.5 (the vertex inside the lobe's ball).
M_GLOSS_GROUND = 12
GLOSS_FUZZ = (0.0, 2.0 ** -11, 2.0 ** -10, 0.05, 0.35, 1.0, 1.5)
# the twins that carry the narrow lobes (fuzz < 0.3); the others have 0.35, 1.0 and 1.5 alone, so that a light-only estimator's weight
# pg / pl stays bounded by pg <= (3 + fuzz^2) / (2 pi fuzz^2) < 4.1 there (test_lit_fuzz_gloss_medium.py's light-only comparison needs that).
# 0 and 6 are the dome with the faint sphere, where light-only weights are unbounded anyway; 7 has a map, so that the threshold fuzz
# meets the environment's switch too
NARROW_TRIALS = (0, 6, 7)


def gloss_rule(seed, trial):
    """The re-materialling of a twin, a function of (seed, trial) alone; its draws (the albedos) come from a generator of its own.
    On NARROW_TRIALS: M_LAMB_A → METAL of fuzz 2^-11, M_LAMB_B → 2^-10, M_METAL → 0.05 (trial 6: fuzz 0); on the others M_LAMB_A → 1.0,
    M_LAMB_B → 1.5 and M_METAL → 0.35.  Everywhere M_GROUND and, on the odd trials, an added ground sphere (the last sphere: no index
    of the table moves) → 0.35, and M_LIGHT_DARK → 1.5 (trial 0: 1.0)."""
    g = np.random.default_rng([seed, trial, 23])
    narrow = trial in NARROW_TRIALS

    def remat(spheres, planes, mats):
        def metal(fuzz):
            return material(MAT_METAL, g.uniform(0.6, 0.95, 3), fuzz=fuzz)
        mats[M_LAMB_A] = metal(2.0 ** -11 if narrow else 1.0)
        mats[M_LAMB_B] = metal(2.0 ** -10 if narrow else 1.5)
        mats[M_METAL] = metal((0.0 if trial == 6 else 0.05) if narrow else 0.35)
        mats[M_GROUND] = metal(0.35)
        mats[M_LIGHT_DARK] = metal(1.0 if trial == 0 else 1.5)
        mats.append(metal(0.35))
        if trial % 2 == 1:
            spheres.append([0.0, -1006.0, 0.0, 1000.0, M_GLOSS_GROUND])
    return remat


@functools.lru_cache(maxsize=None)
def gloss_case(trial):
    c = Case(trial, remat=gloss_rule(SEEDS[trial], trial))
    c.name = f"twin {trial} seed {c.seed}"
    return c


def fuzz_medium(trial):
    """The medium of a trial (medium_reference / rb.medium_params keywords), a function of (SEEDS[trial], trial) alone with a generator of
    its own.  Over the eight: all space on two trials with a map (2, 5: the environment is not sampled there), balls (0: around the eye;
    4: optically thick, albedo 1 — paths end by depth inside it; 6) and boxes (1: half the scene, an albedo with a channel of exactly 0
    and one of exactly 1; 3: around the eye; 7: drawn), g over {0, 0.7, -0.5, 0.95, -0.95}, sigma_t from 0.02 to 5."""
    c = case(trial)
    g = np.random.default_rng([SEEDS[trial], trial, 25])
    eye = np.array(c.eye, np.float32)
    alb = tuple(float(np.float32(x)) for x in g.uniform(0.7, 0.98, 3))
    r = float(np.float32(g.uniform(2.0, 3.0)))
    centre = tuple(float(np.float32(x)) for x in g.uniform(-2.0, 2.0, 3))
    lo = g.uniform(-5.0, -1.0, 3)
    hi = lo + g.uniform(3.0, 6.0, 3)
    if trial == 0:
        return dict(sigma_t=0.3, albedo=alb, g=0.7, ball=(float(eye[0]), float(eye[1]), float(eye[2]), 4.0))
    if trial == 1:
        return dict(sigma_t=0.25, albedo=(1.0, 0.9, 0.0), g=-0.5, box=(-5.5, -5.5, -5.5, 0.5, 5.5, 5.5))
    if trial == 2:
        return dict(sigma_t=0.02, albedo=alb, g=0.95)
    if trial == 3:
        return dict(sigma_t=0.4, albedo=alb, g=-0.95, box=tuple(float(x) for x in np.concatenate([eye - np.float32(3.0), eye + np.float32(3.0)])))
    if trial == 4:
        return dict(sigma_t=5.0, albedo=1.0, g=0.0, ball=(0.0, 0.0, 0.0, 3.5))
    if trial == 5:
        return dict(sigma_t=0.1, albedo=alb, g=0.7)
    if trial == 6:
        return dict(sigma_t=1.0, albedo=alb, g=-0.5, ball=centre + (r,))
    return dict(sigma_t=0.6, albedo=alb, g=0.95, box=tuple(float(np.float32(x)) for x in np.concatenate([lo, hi])))


def medium_extent(m):
    """The region's largest chord (None: all space)."""
    if m.get("ball") is not None:
        return 2.0 * m["ball"][3]
    if m.get("box") is not None:
        return float(np.linalg.norm(np.array(m["box"][3:]) - np.array(m["box"][:3])))
    return None


def inside_medium(m, p):
    if m.get("ball") is not None:
        return float(np.sum((np.asarray(p, np.float64) - np.array(m["ball"][:3])) ** 2)) < m["ball"][3] ** 2
    if m.get("box") is not None:
        return all(m["box"][k] < p[k] < m["box"][3 + k] for k in range(3))
    return True


# A call on a twin.  gn, ge: rt_nee_params.glossy and rt_env_params.glossy; medium: the call goes to rt_render_medium /
# rt_trace_samples_medium under fuzz_medium(trial); the rest as in Call
GCall = collections.namedtuple("GCall", "test entry trial lens planes select mis env shard gn ge medium")


def _gloss_cells(test, trial, nee_entry, env_entry, lit_entry):
    """The glossy calls of one twin: the eight nee settings, the environment in both modes, and every (lens, planes, select) of the lit
    call with the emitters' switch alone and no environment and — where the trial has a map — with the environment's switch alone and
    with both."""
    c = gloss_case(trial)
    out = [GCall(test, nee_entry, trial, False, planes, select, mis, None, None, 1, 0, False) for mis, planes, select in MIS_PLANES_SELECT]
    if c.env is not None:
        out += [GCall(test, env_entry, trial, False, 0, 0, 1, mode, None, 0, 1, False) for mode in (1, 2)]
    for planes, select in PLANES_SELECT:
        for lens in (True, False):
            mis = 1 if lens else 0
            out.append(GCall(test, lit_entry, trial, lens, planes, select, mis, None, None, 1, 0, False))
            if c.env is not None:
                mode = 1 if select else 2
                out.append(GCall(test, lit_entry, trial, lens, planes, select, mis, mode, None, 0, 1, False))
                out.append(GCall(test, lit_entry, trial, lens, planes, select, 1, mode, None, 1, 1, False))
    return out


def gloss_probe_calls(trial):
    return _gloss_cells("gloss probes", trial, NEE_PROBE, ENV_PROBE, LIT_PROBE)


def _medium_cells(test, trial, entry):
    """The medium calls of one twin under fuzz_medium(trial): every (lens, planes, select) without an environment and, where the trial has
    a map, with it; the glossy switches alternate."""
    c = gloss_case(trial)
    out = []
    for planes, select in PLANES_SELECT:
        for lens in (True, False):
            gn = (trial + planes + int(lens)) % 2
            out.append(GCall(test, entry, trial, lens, planes, select, 1 if lens else 0, None, None, gn, 0, True))
            if c.env is not None:
                out.append(GCall(test, entry, trial, lens, planes, select, 1, 1 if select else 2, None, 1 - gn, (trial + select) % 2, True))
    return out


def medium_probe_calls(trial):
    return _medium_cells("medium probes", trial, MEDIUM_PROBE)


@functools.lru_cache(maxsize=None)
def _all_gloss_frame_calls():
    """The frame cells of every twin, glossy and medium; each kernel's calls go through SHARDS in turn."""
    turn, out = collections.Counter(), {"gloss": {}, "medium": {}}
    for t in TRIALS:
        for which, cells in (("gloss", _gloss_cells("gloss frames", t, NEE_FRAME, ENV_FRAME, LIT_FRAME)), ("medium", _medium_cells("medium frames", t, MEDIUM_FRAME))):
            out[which][t] = []
            for c in cells:
                k = kernels_of_gcall(c)[0]
                out[which][t].append(c._replace(shard=turn[k] % 3))
                turn[k] += 1
    return out


def gloss_frame_calls(trial):
    return list(_all_gloss_frame_calls()["gloss"][trial])


def medium_frame_calls(trial):
    return list(_all_gloss_frame_calls()["medium"][trial])


def gloss_adaptive_calls(trial):
    """rt_render_lit_adaptive on a twin: every (lens, planes, select) with the emitters' switch alone and no environment, the
    environment's alone, and both (the adaptive trials all have a map)."""
    c = gloss_case(trial)
    assert c.env is not None
    out = []
    for lens in (False, True):
        for planes, select in PLANES_SELECT:
            out += [GCall("gloss adaptive", LIT_ADAPTIVE, trial, lens, planes, select, 1, env, None, gn, ge, False)
                    for env, gn, ge in ((None, 1, 0), (1, 0, 1), (1, 1, 1))]
    return out


def gloss_calls():
    """Every call the GPU tests of test_lit_fuzz_gloss_medium.py make on the glossy and medium kernels."""
    out = []
    for t in TRIALS:
        out += gloss_probe_calls(t) + gloss_frame_calls(t) + medium_probe_calls(t) + medium_frame_calls(t)
    for t in ADAPTIVE_TRIALS:
        out += gloss_adaptive_calls(t)
    return out


def kernels_of_gcall(call):
    c = gloss_case(call.trial)
    has = c.has_planes(1)
    return kernels_of(call.entry, call.lens, call.planes, call.select, has, c.entries(1 if (call.planes and has) else 0), glossy_nee=call.gn,
                      glossy_env=call.ge, medium_on=call.medium and fuzz_medium(call.trial)["sigma_t"] > 0, emitters=True, env=call.env is not None)


def gloss_reference_keywords(call, w, h, spp, depth):
    """gloss_reference / medium_reference trace / frame keywords of a lit, nee or medium call on a twin (the camera apart)."""
    c = gloss_case(call.trial)
    kw = dict(select=call.select, nee_mis=call.mis, planes=call.planes, glossy=call.gn, glossy_env=call.ge)
    if call.lens:
        kw.update(lens=c.lens, cam_close=c.close(w, h, spp, depth))
    if call.env is not None:
        kw.update(rgb=c.env, env_params=c.env_params(call.env))
    if call.medium:
        kw.update(medium=fuzz_medium(call.trial))
    return kw


def gloss_device_keywords(call, env, w, h, spp, depth):
    """DeviceScene.render_lit / trace_samples_lit / render_medium / … keywords of a lit or medium call on a twin; env: an rb.Env of the
    twin's map (or None)."""
    c = gloss_case(call.trial)
    kw = dict(nee={"mis": call.mis, "sample_planes": call.planes, "select": call.select, "glossy": call.gn})
    if call.lens:
        kw.update(lens=c.lens_dict(), cam_close=c.close(w, h, spp, depth))
    if call.env is not None:
        kw.update(env=env, env_params=dict(glossy=call.ge, **c.env_params(call.env)))
    if call.medium:
        kw.update(medium=fuzz_medium(call.trial))
    return kw


# ---- random fog: a box, a density grid, a tint, a glow and a sample mode per trial, for the four fog families that came
# after §27 — volume, chroma, glow and sampled glow — and the call lists of tests/test_lit_fuzz_fog.py ----------------------------------------
FOG_DIMS = (1, 2, 3, 5, 7, 13, 16, 32, 64)
FOG_G = (0.0, 0.7, -0.5, 0.95, -0.95, 0.7, 0.0, -0.5)
FOG_SAMPLE = ("mis", "light", None, "mis", "light", None, "mis", "light")
FOG_FAMILIES = ("volume", "chroma", "glow", "glow_sampled")


def scene_bounds(host):
    """The box around every primitive of a scene but its ground and dome (spheres of radius >= 40): (lo, hi)."""
    d = host.desc
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for k in range(d.num_spheres):
        s = d.spheres[k]
        if s.radius < 40.0:
            c = np.array(s.center.e[:])
            lo, hi = np.minimum(lo, c - s.radius), np.maximum(hi, c + s.radius)
    for k in range(d.num_planes):
        p = d.planes[k]
        o, u, v = (np.array(x.e[:]) for x in (p.base, p.u, p.v))
        for a in (-1.0, 0.0, 1.0):          # (whichever way a type spans its plane from base, u and v)
            for b in (-1.0, 0.0, 1.0):
                lo, hi = np.minimum(lo, o + a * u + b * v), np.maximum(hi, o + a * u + b * v)
    return lo, hi


def _fog_grid(g, dims, empty):
    """(nz, ny, nx) densities in [0.1, 2), a share `empty` of the cells exactly 0 (test_volume.random_grid's rule, from the fog's generator)."""
    shape = (dims[2], dims[1], dims[0])
    grid = g.uniform(0.1, 2.0, shape).astype(np.float32)
    grid[g.random(shape) < empty] = 0.0
    return grid


@functools.lru_cache(maxsize=None)
def fuzz_fog(trial):
    """The fog of a trial, a pure function of (SEEDS[trial], trial) with a generator of its own: dict(medium: sigma_t, albedo, g and the
    box; density: an (nz, ny, nx) grid, each dimension drawn from FOG_DIMS; tint; radiance and source (with heat where the source is 2);
    sample: None, "mis" or "light").  The box comes from the trial's own scene bounds and eye: around the eye (0, 3), around the whole
    scene (1), a thin slab through it (2), half the scene (4), a face through the first sphere's centre (5), drawn (6, 7).  Arranged,
    like fuzz_medium's regions: a 1 x 1 x 1 grid of density 0.6 (2), a grid with a 64-long axis and the other two 1 (5), a grid with 60 %
    of its cells empty (6), equal tints (0) and a tint with a channel of exactly 0 (3), radiance 0 (5: a trial that takes no light samples); source is trial % 3."""
    c = case(trial)
    g = np.random.default_rng([SEEDS[trial], trial, 39])
    f32 = lambda x: tuple(float(np.float32(v)) for v in x)
    eye = np.array(c.eye)
    lo, hi = scene_bounds(c.host)
    dims = [int(g.choice(FOG_DIMS)) for _ in range(3)]
    half = g.uniform(2.0, 4.0, 3)
    drawn_lo = g.uniform(-5.0, -1.0, 3)
    drawn_hi = drawn_lo + g.uniform(3.0, 6.0, 3)
    margin = g.uniform(0.1, 0.5, 3)
    sigma_t = float(np.float32(10.0 ** g.uniform(-1.0, 0.2)))
    albedo = f32(g.uniform(0.7, 0.98, 3))
    tint = f32(g.uniform(0.3, 1.5, 3))
    radiance = f32(g.uniform(0.05, 0.4, 3))
    axis = int(g.integers(0, 3))
    empty = 1.0 / 3.0
    if trial in (0, 3):
        box = np.concatenate([eye - half, eye + half])
    elif trial == 1:
        box = np.concatenate([lo - margin, hi + margin])
    elif trial == 2:
        box = np.concatenate([lo - margin, hi + margin])
        mid = 0.5 * (lo[1] + hi[1])
        box[1], box[4] = mid - 0.1, mid + 0.1
        dims = [1, 1, 1]
    elif trial == 4:
        box = np.concatenate([lo - margin, hi + margin])
        box[3] = 0.5
    elif trial == 5:
        box = np.concatenate([drawn_lo, drawn_hi])
        s = c.host.desc.spheres[0]
        box[3] = s.center.e[0]
        box[0] = min(box[0], box[3] - 3.0)
        dims = [1, 1, 1]
        dims[axis] = 64
    else:
        box = np.concatenate([drawn_lo, drawn_hi])
    if trial == 6:
        empty = 0.6
    density = np.full((1, 1, 1), 0.6, np.float32) if trial == 2 else _fog_grid(g, dims, empty)
    heat = _fog_grid(g, dims, 0.25)
    if trial == 0:
        tint = (tint[0],) * 3
    if trial == 3:
        tint = (1.0, 0.0, 0.5)
    if trial == 5:
        radiance = (0.0, 0.0, 0.0)
    source = trial % 3
    density.setflags(write=False)
    heat.setflags(write=False)
    return dict(medium=dict(sigma_t=sigma_t, albedo=albedo, g=FOG_G[trial], box=f32(box)), density=density, tint=tint, radiance=radiance, source=source,
                heat=heat if source == 2 else None, sample=FOG_SAMPLE[trial])


# A fog call on a twin.  family: one of FOG_FAMILIES; grid: the call passes the fog's grid (else volume = None: the homogeneous box); the
# rest as in GCall.  The environment is the twin's map where it has one
FCall = collections.namedtuple("FCall", "test family trial lens planes select mis env shard gn ge grid")


def _fog_cells(test, trial):
    """The fog calls of one twin: per family one call for each (select, sample_planes); the lens and the grid alternate with the pair and
    the trial, so that over the eight twins every family meets lens off / on x the four pairs x grid / no grid, and per twin every family
    appears with the grid and without it.  Sampled glow keeps the grid (without one it is the glow call)."""
    c = gloss_case(trial)
    out = []
    for family in FOG_FAMILIES:
        for p, (planes, select) in enumerate(PLANES_SELECT):
            lens = (p + trial) % 2 == 1
            grid = family == "glow_sampled" or ((p >> 1) + (trial >> 1)) % 2 == 0
            env = (1 if select else 2) if c.env is not None else None
            out.append(FCall(test, family, trial, lens, planes, select, 1 if lens else 0, env, None, (trial + planes) % 2, (trial + select) % 2 if env else 0, grid))
    return out


def fog_probe_calls(trial):
    return _fog_cells("fog probes", trial)


@functools.lru_cache(maxsize=None)
def _all_fog_frame_calls():
    """The frame cells of every twin; each family's calls rotate through SHARDS."""
    turn, out = collections.Counter(), {}
    for t in TRIALS:
        out[t] = []
        for c in _fog_cells("fog frames", t):
            out[t].append(c._replace(shard=turn[c.family, c.lens] % 3))
            turn[c.family, c.lens] += 1
    return out


def fog_frame_calls(trial):
    return list(_all_fog_frame_calls()[trial])


def fog_calls(trial):
    """Per family, the probe and the frame calls of the trial: {family: (probes, frames)}."""
    return {f: ([c for c in fog_probe_calls(trial) if c.family == f], [c for c in fog_frame_calls(trial) if c.family == f]) for f in FOG_FAMILIES}


def fog_reference_keywords(call, w, h, spp, depth):
    """The keywords of volume_reference / chroma_reference / glow_reference / glow_sample_reference's trace and frame for a fog call (the
    camera apart)."""
    c, f = gloss_case(call.trial), fuzz_fog(call.trial)
    kw = dict(medium=f["medium"], density=f["density"] if call.grid else None, select=call.select, nee_mis=call.mis, planes=call.planes, glossy=call.gn,
              glossy_env=call.ge)
    if call.lens:
        kw.update(lens=c.lens, cam_close=c.close(w, h, spp, depth))
    if call.env is not None:
        kw.update(rgb=c.env, env_params=c.env_params(call.env))
    if call.family == "chroma":
        kw.update(tint=f["tint"])
    if call.family in ("glow", "glow_sampled"):
        source = f["source"] if call.grid else 0          # (source 1 and 2 follow a grid)
        kw.update(radiance=f["radiance"], source=source, heat=f["heat"] if source == 2 else None)
    if call.family == "glow_sampled":
        kw.update(sample=f["sample"])
    return kw


def fog_device_keywords(call, env, volume, heat, sampler, w, h, spp, depth):
    """DeviceScene.render_<family>_to_host / trace_samples_<family> keywords of a fog call; env: an rb.Env of the twin's map (or None);
    volume, heat: the rb.Volumes of the fog's grids (heat None unless the source is 2); sampler: the rb.GlowSampler of them."""
    c, f = gloss_case(call.trial), fuzz_fog(call.trial)
    kw = dict(nee={"mis": call.mis, "sample_planes": call.planes, "select": call.select, "glossy": call.gn}, medium=f["medium"], volume=volume if call.grid else None)
    if call.lens:
        kw.update(lens=c.lens_dict(), cam_close=c.close(w, h, spp, depth))
    if call.env is not None:
        kw.update(env=env, env_params=dict(glossy=call.ge, **c.env_params(call.env)))
    if call.family == "chroma":
        kw.update(tint=f["tint"])
    if call.family in ("glow", "glow_sampled"):
        source = f["source"] if call.grid else 0
        kw.update(glow=dict(radiance=f["radiance"], source=source), heat=heat if source == 2 else None)
    if call.family == "glow_sampled":
        kw.update(sample=f["sample"], sampler=sampler if f["sample"] is not None else None)
    return kw
