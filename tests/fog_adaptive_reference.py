"""CPU reference of rt_render_fog_adaptive (TEST INFRASTRUCTURE; include/rtp_amd.h "adaptive sampling on every fog rung").
Composition only, no new arithmetic, exactly as volume_adaptive_reference.py composes volume_reference: the per-sample radiances are
chroma_reference.trace's, glow_reference.trace's or glow_sample_reference.trace's (the restatements of the three upper frame calls) through
lit_adaptive_reference.radiances; the rule, the moments and the sums are lit_adaptive_reference.from_radiances'; the other stopping rule and
the prior are adaptive_prior_reference's.  The settings of tests/test_fog_adaptive.py live here: each is a setting of
volume_adaptive_reference.py (tests/test_volume.py's scenes, BOX and GRIDS) with a tint of tests/test_chroma.py, a glow and a heat grid of
tests/test_glow.py or a sample mode of tests/test_glow_sampled.py on top, so that the CPU and the GPU tests share them."""
import contextlib
import functools

import numpy as np

import chroma_reference as cr
import env_reference as er
import glow_reference as gr
import glow_sample_reference as gs
import lit_adaptive_reference as lar
import rtp_bindings as rb
import volume_adaptive_reference as var
from test_chroma import TINTS
from test_glow import GLOWS, HEATS

F = np.float32
SPP, LEVELS, SIZE, DEPTH = var.SPP, var.LEVELS, var.SIZE, var.DEPTH
RUNGS = ("tint", "glow", "sampled")
TRACERS = {"tint": cr.trace, "glow": gr.trace, "sampled": gs.trace}
# the column of the rung's restatement that shows the rung's own effect in a sample: medium events, glow_length, glow_samples
EXTRA = {"tint": 2, "glow": 6, "sampled": 7}

# name → (the setting of volume_adaptive_reference.SETTINGS underneath, the rung, what the rung adds: the restatement's keywords; heat names
# a grid of test_glow.HEATS).  Under them (volume_adaptive_reference.py): a = night rtiow, a 2x3x5 grid, select, glossy; b = three balls, a
# 16^3 grid, select and sample_planes; c = a with the lens and the sun-and-sky map; d = three balls, a ball without a grid, the map alone
SETTINGS = {
    "tint b": ("b", "tint", dict(tint=TINTS[0])),
    "tint c": ("c", "tint", dict(tint=TINTS[2])),
    "tint d": ("d", "tint", dict(tint=TINTS[1])),
    "glow a": ("a", "glow", dict(radiance=GLOWS[0], source=1)),
    "glow c": ("c", "glow", dict(radiance=GLOWS[2], source=2, heat="2x3x5")),
    "glow d": ("d", "glow", dict(radiance=GLOWS[1], source=0)),
    "sampled b": ("b", "sampled", dict(radiance=GLOWS[0], source=1, sample="mis")),
    "sampled c": ("c", "sampled", dict(radiance=GLOWS[2], source=2, heat="2x3x5", sample="light")),
}
# The thresholds, chosen by a sweep on the restatement (tools/fog_adaptive_sweep.py) as the value whose least-populated level is fullest
# (DESIGN.md §40 has the histograms)
THRESHOLDS = {"tint b": 0.125, "tint c": 0.225, "tint d": 0.275, "glow a": 0.125, "glow c": 0.15, "glow d": 0.1, "sampled b": 0.15, "sampled c": 0.125}


def base_of(setting):
    return SETTINGS[setting][0]


def rung_of(setting):
    return SETTINGS[setting][1]


def scene_cam(setting, size=SIZE, spp=1, depth=DEPTH):
    return var.scene_cam(base_of(setting), size, spp, depth)


def heat_of(setting):
    name = SETTINGS[setting][2].get("heat")
    return None if name is None else HEATS[name]


def reference_keywords(setting):
    """The keywords of the rung's restatement (medium, density and the rung's own included)."""
    more = dict(SETTINGS[setting][2])
    if "heat" in more:
        more["heat"] = heat_of(setting)
    return dict(var.reference_keywords(base_of(setting)), **more)


@contextlib.contextmanager
def device_objects(setting):
    """(volume, heat, sampler) of a setting on the current device, each None where the setting has none; closed in reverse on exit."""
    more = SETTINGS[setting][2]
    density, heat = var.density_of(base_of(setting)), heat_of(setting)
    with contextlib.ExitStack() as stack:
        vol = stack.enter_context(rb.Volume(density)) if density is not None else None
        hv = stack.enter_context(rb.Volume(heat)) if heat is not None else None
        q = stack.enter_context(rb.GlowSampler(vol, more["source"], hv)) if "sample" in more else None
        yield vol, hv, q


def rung_keywords(setting, objects):
    """What the rung adds to a device call (the frame call's and the adaptive call's alike): tint, or glow and heat, and sample and sampler."""
    more = SETTINGS[setting][2]
    _, hv, q = objects
    if "tint" in more:
        return dict(tint=more["tint"])
    kw = dict(glow=dict(radiance=more["radiance"], source=more["source"]), heat=hv)
    if "sample" in more:
        kw.update(sample=more["sample"], sampler=q)
    return kw


def device_keywords(setting, env, objects):
    """DeviceScene.render_fog_adaptive's keywords of a setting (and, for its rung, render_chroma's, render_glow's or
    render_glow_sampled's); env: an rb.Env of lit_adaptive_reference.sky(), objects: device_objects(setting)'s."""
    return dict(var.device_keywords(base_of(setting), env, objects[0]), **rung_keywords(setting, objects))


def frame_call(dev, setting):
    """The rung's frame call of a setting, to host."""
    return {"tint": dev.render_chroma_to_host, "glow": dev.render_glow_to_host, "sampled": dev.render_glow_sampled_to_host}[rung_of(setting)]


def radiances(host, cam, samples, rung, sample_first=0, rows=None, extra_out=None, **kw):
    """lit_adaptive_reference.radiances through the rung's restatement; extra_out: a list that receives the rung's extra column per sample,
    (rows, W, samples): medium events, glow_length or glow_samples."""
    def tracer(host_, cam_, ijs, **kw_):
        out = TRACERS[rung](host_, cam_, ijs, **kw_)
        if extra_out is not None:
            extra_out.append(out[EXTRA[rung]])
        return out
    rad = lar.radiances(host, cam, samples, sample_first, rows, tracer=tracer, **kw)
    if extra_out is not None:
        extra_out[-1] = extra_out[-1].reshape(rad.shape[:3])
    return rad


def reference(host, cam, rung=None, sample_first=0, shard=None, rule=None, prior=None, **kw):
    """What render_fog_adaptive_to_host returns (without the timing); kw: rt_adaptive_params fields and the restatement's keywords.  rung
    None (no tint, no glow, no sample) is volume_adaptive_reference.reference."""
    if rung is None:
        return var.reference(host, cam, sample_first=sample_first, shard=shard, rule=rule, prior=prior, **kw)
    params = {k: kw.pop(k) for k in ("min_spp", "batch_spp", "max_spp", "threshold")}
    total = params["min_spp"] + (params["max_spp"] - params["min_spp"]) // params["batch_spp"] * params["batch_spp"]
    rad = radiances(host, cam, total, rung, sample_first, er.image_rows(cam, shard), **kw)
    return var.from_radiances(rad, shard, rule, prior, **params)


@functools.lru_cache(maxsize=None)
def setting_radiances(setting, sample_first=0, size=SIZE, samples=SPP["max_spp"]):
    """(radiances (H, W, samples, 3), the rung's extra column (H, W, samples)) of a setting's whole frame (cached and shared: do not write
    to them)."""
    host, cam = scene_cam(setting, size)
    extra = []
    rad = radiances(host, cam, samples, rung_of(setting), sample_first, extra_out=extra, **reference_keywords(setting))
    rad.setflags(write=False)
    extra[0].setflags(write=False)
    return rad, extra[0]


def setting_reference(setting, sample_first=0, shard=None, threshold=None, size=SIZE, rule=None, prior=None, **spp):
    """(fb, spp, moments) of a setting under SPP (or the given rt_adaptive_params fields) and its threshold, the rows of `shard`."""
    p = {**SPP, **spp, "threshold": THRESHOLDS[setting] if threshold is None else threshold}
    rows = er.image_rows(scene_cam(setting, size)[1], shard)
    rad = setting_radiances(setting, sample_first, size)[0][rows]
    return var.from_radiances(rad, shard, rule, prior, **p)


def level_counts(setting, threshold, size=SIZE):
    """Pixels per stop level of a setting's whole frame at a threshold, on the restatement."""
    spp = setting_reference(setting, threshold=threshold, size=size)[1]
    return [int((spp == n).sum()) for n in LEVELS]
