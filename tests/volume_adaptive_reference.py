"""CPU reference of rt_render_volume_adaptive (TEST INFRASTRUCTURE; include/rtp_amd.h "adaptive sampling under fog").
Composition only, no new arithmetic: the per-sample radiances are volume_reference.trace's (the restatement of rt_render_volume) through
lit_adaptive_reference.radiances, the rule, the moments and the sums are lit_adaptive_reference.from_radiances', and the other stopping
rule and the prior are adaptive_prior_reference's.  The settings of tests/test_volume_adaptive.py live here, on tests/test_volume.py's
scenes, BOX and GRIDS, so that the CPU and the GPU tests share them."""
import functools

import numpy as np

import adaptive_prior_reference as apr
import env_reference as er
import lit_adaptive_reference as lar
import rtp_bindings as rb
import volume_reference as vr
from test_medium import LENS, scenes
from test_volume import BOX, GRIDS

F = np.float32
SPP = dict(min_spp=4, batch_spp=4, max_spp=32)
LEVELS = list(range(4, 33, 4))
SIZE = (32, 24)
DEPTH = 50
ENV_PARAMS = dict(mode=1, scale=0.75)          # lit_adaptive_reference's: the sun-and-sky map, mis
BALL = dict(ball=(0.0, 1.0, 0.0, 3.0))         # test_medium.media's ball


def _fog(g, **more):
    return dict(sigma_t=0.5, albedo=(0.95, 0.9, 0.8), g=g, box=BOX, **more)


# name → (scene, medium, grid of GRIDS or None, the restatement's keywords ("sky": lit_adaptive_reference.sky() under ENV_PARAMS), the device
# call's keywords ("env": True marks the calls that need an rb.Env of the sky))
SETTINGS = {
    "a": ("night rtiow", _fog(0.5), "2x3x5", dict(select=1, nee_mis=1, glossy=1), dict(nee=dict(select=1, mis=1, glossy=1))),
    "b": ("three balls", _fog(-0.95), "16", dict(select=1, planes=1), dict(nee=dict(select=1, sample_planes=1))),
    "c": ("night rtiow", _fog(0.5), "2x3x5", dict(select=1, nee_mis=1, glossy=1, lens=LENS, sky=True),
          dict(nee=dict(select=1, mis=1, glossy=1), lens=dict(lens_radius=LENS[0], focus_distance=LENS[1]), env=True)),
    "d": ("three balls", dict(sigma_t=0.35, albedo=(0.95, 0.9, 0.8), g=0.7, **BALL), None, dict(emitters=False, sky=True), dict(emitters=False, env=True)),
    "e": ("three balls", dict(sigma_t=0.08, albedo=(0.9, 0.85, 0.8), g=0.0), None, dict(nee_mis=1, sky=True), dict(nee=dict(mis=1), env=True)),
}
# The thresholds of the settings, chosen on the restatement so that test_volume_adaptive.py's populated-levels condition holds
THRESHOLDS = {"a": 0.3, "b": 0.1, "c": 0.2, "d": 0.25, "e": 0.15}


def scene_cam(setting, size=SIZE, spp=1, depth=DEPTH):
    host, camera, _ = scenes()[SETTINGS[setting][0]]
    return host, camera(size[0], size[1], spp, depth)


def medium_of(setting):
    return dict(SETTINGS[setting][1])


def density_of(setting):
    grid = SETTINGS[setting][2]
    return None if grid is None else GRIDS[grid]


def reference_keywords(setting):
    """volume_reference.trace's keywords of a setting (medium and density included)."""
    kw = dict(SETTINGS[setting][3])
    if kw.pop("sky", False):
        kw.update(rgb=lar.sky(), env_params=ENV_PARAMS)
    return dict(medium=medium_of(setting), density=density_of(setting), **kw)


def device_keywords(setting, env, volume):
    """DeviceScene.render_volume[_adaptive] keywords of a setting; env: an rb.Env of lar.sky(), volume: an rb.Volume of density_of(setting)
    (each used where the setting has one)."""
    kw = dict(SETTINGS[setting][4])
    if kw.pop("env", False):
        kw.update(env=env, env_params=ENV_PARAMS)
    return dict(medium=medium_of(setting), volume=volume if density_of(setting) is not None else None, **kw)


def radiances(host, cam, samples, sample_first=0, rows=None, events_out=None, **kw):
    """lit_adaptive_reference.radiances through volume_reference.trace; events_out: a list that receives the medium events per sample,
    (rows, W, samples) int32."""
    def tracer(host_, cam_, ijs, **kw_):
        out = vr.trace(host_, cam_, ijs, **kw_)
        if events_out is not None:
            events_out.append(out[2])
        return out
    rad = lar.radiances(host, cam, samples, sample_first, rows, tracer=tracer, **kw)
    if events_out is not None:
        events_out[-1] = events_out[-1].reshape(rad.shape[:3])
    return rad


def from_radiances(rad, shard=None, rule=None, prior=None, **params):
    """(fb, spp, moments) of the buffer rows rad (rows, W, samples, 3): lit_adaptive_reference.from_radiances, or adaptive_prior_reference's
    with a rule or a prior (rows, W, 2)."""
    if rule is None and prior is None:
        return lar.from_radiances(rad, **params)
    return apr.from_radiances(rad, shard, params["min_spp"], params["batch_spp"], params["max_spp"], params["threshold"], rule or 0, prior)


def reference(host, cam, medium=None, density=None, sample_first=0, shard=None, rule=None, prior=None, **kw):
    """What render_volume_adaptive_to_host returns (without the timing); kw: rt_adaptive_params fields and volume_reference.trace's keywords.
    With the fog off (medium None or sigma_t 0) this is lit_adaptive_reference.reference."""
    params = {k: kw.pop(k) for k in ("min_spp", "batch_spp", "max_spp", "threshold")}
    if medium is None or not medium.get("sigma_t", 0.0) > 0.0:
        assert rule is None and prior is None
        return lar.reference(host, cam, sample_first=sample_first, shard=shard, **params, **kw)
    total = params["min_spp"] + (params["max_spp"] - params["min_spp"]) // params["batch_spp"] * params["batch_spp"]
    rad = radiances(host, cam, total, sample_first, er.image_rows(cam, shard), medium=medium, density=density, **kw)
    return from_radiances(rad, shard, rule, prior, **params)


@functools.lru_cache(maxsize=None)
def setting_radiances(setting, sample_first=0, size=SIZE, samples=SPP["max_spp"]):
    """(radiances (H, W, samples, 3), medium events (H, W, samples)) of a setting's whole frame (cached and shared: do not write to them)."""
    host, cam = scene_cam(setting, size)
    events = []
    rad = radiances(host, cam, samples, sample_first, events_out=events, **reference_keywords(setting))
    rad.setflags(write=False)
    events[0].setflags(write=False)
    return rad, events[0]


def setting_reference(setting, sample_first=0, shard=None, threshold=None, size=SIZE, rule=None, prior=None, **spp):
    """(fb, spp, moments) of a setting under SPP (or the given rt_adaptive_params fields) and its threshold, the rows of `shard`."""
    p = {**SPP, **spp, "threshold": THRESHOLDS[setting] if threshold is None else threshold}
    rows = er.image_rows(scene_cam(setting, size)[1], shard)
    rad = setting_radiances(setting, sample_first, size)[0][rows]
    return from_radiances(rad, shard, rule, prior, **p)


def prior_of(rows, width, seed=5):
    """A non-zero prior (rows, width, 2) float32 (ch, vh): a third of the pixels without one (ch = 0), the rest 1 … 24 samples of history
    with a small variance."""
    rng = np.random.default_rng(seed)
    ch = rng.integers(1, 25, (rows, width)).astype(F)
    ch[rng.random((rows, width)) < 1 / 3] = 0
    vh = rng.uniform(0.0, 0.02, (rows, width)).astype(F)
    return np.stack([ch, vh], axis=2).astype(F)
