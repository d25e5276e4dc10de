"""Random fog on the random lit scenes: test_lit_fuzz_gloss_medium.py's protocol on the four fog families that came after
it — rt_render_volume, _chroma, _glow and _glow_sampled — on tests/lit_fuzz.py's glossy twins under lit_fuzz.fuzz_fog: a box nobody
placed, a grid whose dimensions were drawn, a tint, a glow and a sample mode per trial.

On the CPU: the fogs have the properties they aim at, the GPU tests' own call lists meet every family under lens off / on, the four
(select, sample_planes) pairs and grid / no grid, the restatements are finite and reach events, cells and light samples on every trial,
and they have the right expectation — sampled glow (mis) against the glow restatement, each channel of the chroma restatement against the
grey volume restatement at that channel's extinction.  On the GPU: probed samples and frames equal the restatements bit for bit.  The
`light` mode is compared for bits only: its tail is what the comment above test_lit_fuzz_gloss_medium.light_only describes."""
import functools

import numpy as np
import pytest

import chroma_reference as cr
import emit_reference as emr
import glow_reference as gr
import glow_sample_reference as gsr
import lit_fuzz as lf
import rtp_bindings as rb
import volume_reference as vr
from test_lit_fuzz import FRAME, PROBE_SIZE, _compare, probe_set
from test_lit_fuzz_gloss_medium import SPP, _bytes_of
from test_light_tree import assert_same

REFERENCE = {"volume": vr, "chroma": cr, "glow": gr, "glow_sampled": gsr}


# ---- B.1 the fogs ---------------------------------------------------------------------------------------------------------------------------
def _cuts(box, centre, radius):
    """Does a face of the box cut through the sphere?"""
    lo, hi = np.array(box[:3]), np.array(box[3:])
    for k in range(3):
        for face in (lo[k], hi[k]):
            near = np.clip(centre, lo, hi)
            near[k] = face
            if abs(centre[k] - face) < radius and np.linalg.norm(near - centre) < radius:
                return True
    return False


def test_fogs():
    """fuzz_fog over the eight trials has what it aims at, is a function of (seed, trial) alone, and making it moves neither case(trial),
    gloss_case(trial) nor fuzz_medium(trial)."""
    eye_in = partial = encloses = slab = cut = one = empty_half = long_axis = zero_tint = equal_tint = dark = 0
    sources, samples, gs = [], [], set()
    for t in lf.TRIALS:
        before, twin, medium = _bytes_of(lf.case(t).host), _bytes_of(lf.gloss_case(t).host), lf.fuzz_medium(t)
        f, again = lf.fuzz_fog(t), lf.fuzz_fog.__wrapped__(t)
        assert _bytes_of(lf.Case(t).host) == before == _bytes_of(lf.case(t).host), "case(trial) moved"
        assert _bytes_of(lf.Case(t, remat=lf.gloss_rule(lf.SEEDS[t], t)).host) == twin == _bytes_of(lf.gloss_case(t).host), "gloss_case(trial) moved"
        assert lf.fuzz_medium(t) == medium
        assert f["medium"] == again["medium"] and f["density"].tobytes() == again["density"].tobytes() and (f["tint"], f["radiance"], f["source"], f["sample"]) == (
            again["tint"], again["radiance"], again["source"], again["sample"]) and (f["heat"] is None or f["heat"].tobytes() == again["heat"].tobytes())
        c, m = lf.gloss_case(t), f["medium"]
        rb.medium_params(**m)
        box = np.array(m["box"])
        ext = box[3:] - box[:3]
        assert (ext > 0).all() and 0.05 <= m["sigma_t"] <= 2.0 and f["density"].dtype == np.float32
        assert all(n in lf.FOG_DIMS for n in f["density"].shape) and (f["heat"] is not None) == (f["source"] == 2)
        assert f["heat"] is None or f["heat"].shape == f["density"].shape
        inside = lf.inside_medium(m, c.eye)
        eye_in += inside
        d = c.host.desc
        kd, idx = emr.table(c.host, 1)[:2]
        held = [lf.inside_medium(m, d.spheres[i].center.e[:]) for k, i in zip(kd, idx) if k == 0 and d.spheres[i].radius < 40.0]
        partial += 0 < sum(held) < len(held)
        lo, hi = lf.scene_bounds(c.host)
        encloses += bool((box[:3] < lo).all() and (box[3:] > hi).all())
        slab += bool(ext.min() < 0.05 * ext.max())
        cut += any(_cuts(box, np.array(d.spheres[k].center.e[:]), d.spheres[k].radius) for k in range(d.num_spheres) if d.spheres[k].radius < 40.0)
        dims = f["density"].shape[::-1]
        one += dims == (1, 1, 1) and float(f["density"].flat[0]) != 1.0
        empty_half += bool((f["density"] == 0).mean() >= 0.5)
        long_axis += sorted(dims) == [1, 1, 64]
        zero_tint += 0.0 in f["tint"]
        equal_tint += len(set(f["tint"])) == 1
        dark += f["radiance"] == (0.0, 0.0, 0.0)
        sources.append(f["source"])
        samples.append(f["sample"])
        gs.add(m["g"])
        print(f"trial {t}: eye inside {inside}, emitting spheres inside / outside {sum(held)} / {len(held) - sum(held)}, grid {'x'.join(map(str, dims))} "
              f"({(f['density'] == 0).mean():.2f} empty), extents {np.round(ext, 2).tolist()}, tint {np.round(f['tint'], 3).tolist()}, source {f['source']}, "
              f"sample {f['sample']}")
    assert eye_in >= 2 and len(lf.TRIALS) - eye_in >= 2, eye_in
    assert partial >= 1 and encloses >= 1 and slab >= 1 and cut >= 1, (partial, encloses, slab, cut)
    assert one >= 1 and empty_half >= 1 and long_axis >= 1, (one, empty_half, long_axis)
    assert zero_tint >= 1 and equal_tint >= 1 and dark >= 1, (zero_tint, equal_tint, dark)
    assert all(sources.count(s) >= 2 for s in (0, 1, 2)) and all(samples.count(s) >= 2 for s in (None, "mis", "light")), (sources, samples)
    assert gs == {0.0, 0.7, -0.5, 0.95, -0.95}


# ---- B.2 the calls --------------------------------------------------------------------------------------------------------------------------
def test_every_family_meets_every_setting():
    """From the lists' own parameters: every family meets lens off / on x the four (select, sample_planes) pairs x grid / no grid (sampled
    glow: the grid only), as a probe and as a frame; per trial every family appears with the grid and (sampled glow apart) without it;
    sample_planes = 1 meets a twin whose table holds a plane under both lens settings; the frames rotate through lit_fuzz.SHARDS."""
    for which in (0, 1):
        met, planes_met, shards = {}, {}, {}
        for t in lf.TRIALS:
            calls = lf.fog_calls(t)
            assert sorted(calls) == sorted(lf.FOG_FAMILIES)
            for family, lists in calls.items():
                grids = {c.grid for c in lists[which]}
                assert grids == ({True} if family == "glow_sampled" else {True, False}), (t, family, grids)
                for c in lists[which]:
                    assert c.trial == t and c.family == family and (c.env is not None) == (lf.gloss_case(t).env is not None)
                    met.setdefault(family, set()).add((c.lens, c.select, c.planes, c.grid))
                    if c.planes and lf.gloss_case(t).has_planes(1):
                        planes_met.setdefault(family, set()).add(c.lens)
                    if which:
                        shards.setdefault(family, set()).add(c.shard)
                    else:
                        assert c.shard is None
        for family in lf.FOG_FAMILIES:
            want = {(lens, select, planes, grid) for lens in (False, True) for planes, select in lf.PLANES_SELECT
                    for grid in ((True,) if family == "glow_sampled" else (True, False))}
            assert met[family] == want, (family, sorted(want - met[family]))
            assert planes_met[family] == {False, True}, (family, planes_met[family])
            if which:
                assert shards[family] == {0, 1, 2}, (family, shards[family])


# ---- B.3 the restatements -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def probe_reference(call):
    c = lf.gloss_case(call.trial)
    w, h = PROBE_SIZE
    return REFERENCE[call.family].trace(c.host, c.camera(w, h, 1, 50), probe_set(), **lf.fog_reference_keywords(call, w, h, 1, 50))


def _samples(call):
    f = lf.fuzz_fog(call.trial)
    return call.family == "glow_sampled" and f["sample"] is not None and f["radiance"] != (0.0, 0.0, 0.0)


@pytest.mark.parametrize("trial", lf.TRIALS)
def test_restatements_are_finite_and_reach_the_fog(trial):
    """On probe_set() every restatement of every probe call is finite; over the trial the columns show medium events, cells where there
    is a grid, and light samples of the glow where the mode samples."""
    events = cells = shots = sampling = 0
    for call in lf.fog_probe_calls(trial):
        want = probe_reference(call)
        assert np.isfinite(want[0]).all(), call
        assert all(np.isfinite(x).all() for x in want[6:7]), call
        events += int(want[2].sum())
        if call.grid:
            assert int(want[5].sum()) > 0, call
            cells += int(want[5].sum())
        else:
            assert not want[5].any(), call
        if _samples(call):
            sampling += 1
            assert int(want[7].sum()) > 0, call
            shots += int(want[7].sum())
    print(f"trial {trial}: {events} medium events, {cells} cells, {shots} light samples of the glow on {sampling} calls")
    assert events > 0 and cells > 0
    assert sampling == (4 if lf.fuzz_fog(trial)["sample"] is not None and lf.fuzz_fog(trial)["radiance"] != (0.0, 0.0, 0.0) else 0)


def _channel(m, k):
    """The moments of channel k alone (the protocol's luminance is then that channel, up to a factor that z does not see)."""
    out = np.zeros_like(m)
    out[..., k], out[..., 3 + k] = m[..., k], m[..., 3 + k]
    return out


@pytest.mark.parametrize("trial", lf.TRIALS)
def test_unbiased_under_the_fog(trial):
    """test_unbiased_on_the_twins' protocol and bounds, unchanged, under fuzz_fog(trial) with its grid: 8 x 8 pixels, depth 6, 16384 samples
    per estimator from disjoint ranges, 2 x 2 block |z| < 5 and image |z| < 4, every comparison with a control held to the same bounds.
    Sampled glow with mis against the glow restatement (whatever mode the trial's own calls use; on the trial without radiance both are
    the volume restatement, and the comparison is a second control); each channel of the chroma restatement against the grey volume
    restatement at sigma_t * tint[k], in that channel."""
    c, f = lf.gloss_case(trial), lf.fuzz_fog(trial)
    spp = SPP
    cam = c.camera(8, 8, spp, 6)
    kw = dict(density=f["density"], select=1, planes=1, glossy=1, nee_mis=1, lens=c.lens, cam_close=c.close(8, 8, spp, 6))
    if c.env is not None:
        kw.update(glossy_env=1, rgb=c.env, env_params=c.env_params(1))
    glow = dict(radiance=f["radiance"], source=f["source"], heat=f["heat"])
    worst = []

    def check(what, x, y):
        z, za = _compare(f"{c.name} {what}", x, y, spp)
        worst.append((what, z, za))

    plain = gr.frame(c.host, cam, medium=f["medium"], sample_first=0, moments=True, **glow, **kw)[1]
    check("control glow / glow", gr.frame(c.host, cam, medium=f["medium"], sample_first=spp, moments=True, **glow, **kw)[1], plain)
    check("sampled glow (mis) / glow", gsr.frame(c.host, cam, medium=f["medium"], sample="mis", sample_first=2 * spp, moments=True, **glow, **kw)[1], plain)
    tinted = cr.frame(c.host, cam, medium=f["medium"], tint=f["tint"], sample_first=3 * spp, moments=True, **kw)[1]
    sigma = (np.float32(f["medium"]["sigma_t"]) * np.asarray(f["tint"], np.float32)).astype(np.float32)
    grey = {}
    for k in range(3):
        s = float(sigma[k])
        if s not in grey:
            m = dict(f["medium"], sigma_t=s)
            n = len(grey)
            grey[s] = (vr.frame(c.host, cam, medium=m, sample_first=(4 + 2 * n) * spp, moments=True, **kw)[1],
                       vr.frame(c.host, cam, medium=m, sample_first=(5 + 2 * n) * spp, moments=True, **kw)[1])
        a, b = grey[s]
        check(f"control grey / grey at sigma_t * tint[{k}] = {s:.4f}, channel {k}", _channel(b, k), _channel(a, k))
        check(f"chroma / grey at sigma_t * tint[{k}] = {s:.4f}, channel {k}", _channel(tinted, k), _channel(a, k))
    for what, z, za in worst:
        assert z < 5.0 and abs(za) < 4.0, (c.name, what, z, za)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------------
class Fog:
    """The device objects of a trial's fog: the scene, the map, the grids and the sampler."""

    def __init__(self, trial):
        rb.amd_lib().rt_set_device(0)
        self.c, self.f = lf.gloss_case(trial), lf.fuzz_fog(trial)
        self.dev = rb.DeviceScene(self.c.host, device=0)
        self.env = rb.Env(self.c.env) if self.c.env is not None else None
        self.volume = rb.Volume(self.f["density"])
        self.heat = rb.Volume(self.f["heat"]) if self.f["heat"] is not None else None
        self.sampler = rb.GlowSampler(self.volume, self.f["source"], self.heat)

    def keywords(self, call, w, h, spp, depth):
        return lf.fog_device_keywords(call, self.env, self.volume, self.heat, self.sampler, w, h, spp, depth)

    def close(self):
        self.sampler.close()
        if self.heat is not None:
            self.heat.close()
        self.volume.close()
        if self.env is not None:
            self.env.close()
        self.dev.close()


def _compare_probe(call, got, want, what):
    """The device's columns against the restatement's: radiance, rays, events, the four seeds, then the family's own — cells, glow_length,
    glow_samples."""
    assert len(got) == {"volume": 8, "chroma": 8, "glow": 9, "glow_sampled": 10}[call.family]
    assert_same(got[0], want[0], what + ": radiance")
    assert_same(got[1], want[1], what + ": rays")
    assert_same(got[2], want[2], what + ": medium events")
    for k in range(4):
        assert_same(got[3 + k], want[4][:, k], what + f": final seed {k}")
    assert_same(got[7], want[5], what + ": cells")
    if call.family in ("glow", "glow_sampled"):
        assert_same(got[8], want[6], what + ": glow_length")
    if call.family == "glow_sampled":
        assert_same(got[9], want[7], what + ": glow_samples")


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_fog_probes_equal_the_restatement(trial):
    """Every probe call of the trial, in all four families: every column equals the restatement's on probe_set() at PROBE_SIZE."""
    fog = Fog(trial)
    w, h = PROBE_SIZE
    cam = fog.c.camera(w, h, 1, 50)
    try:
        for call in lf.fog_probe_calls(trial):
            got = getattr(fog.dev, "trace_samples_" + call.family)(cam, probe_set(), **fog.keywords(call, w, h, 1, 50))
            _compare_probe(call, got, probe_reference(call), f"{fog.c.name} {call}")
    finally:
        fog.close()


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_fog_frames_equal_the_restatement(trial):
    """Every frame call of the trial at test_lit_fuzz.FRAME, depth 50, each with its turn of lit_fuzz.SHARDS: the frame equals the
    restatement's."""
    fog = Fog(trial)
    w, h, spp = FRAME
    cam = fog.c.camera(w, h, spp, 50)
    try:
        for call in lf.fog_frame_calls(trial):
            shard, first = lf.SHARDS[call.shard]
            got = getattr(fog.dev, f"render_{call.family}_to_host")(cam, shard=shard, sample_first=first, **fog.keywords(call, w, h, spp, 50))[0]
            want = REFERENCE[call.family].frame(fog.c.host, cam, shard=shard, sample_first=first, **lf.fog_reference_keywords(call, w, h, spp, 50))
            assert_same(got, want, f"{fog.c.name} {call}")
    finally:
        fog.close()
