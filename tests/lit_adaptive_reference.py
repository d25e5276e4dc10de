"""CPU reference of rt_render_lit_adaptive (TEST INFRASTRUCTURE; include/rtp_amd.h).  Composition, no new arithmetic:
the per-sample radiances are tree_reference.trace's (the most general restatement of rt_render_lit: select, planes, environment, lens,
motion), the rule and the moments are test_adaptive.reference's, and the sums are added in float32 in sample order up to each pixel's own
count.  The scenes, cameras and lit settings of tests/test_lit_adaptive.py live here too, so that the CPU and the GPU tests share them."""
import functools

import numpy as np

import env_reference as er
import rtp_bindings as rb
import test_adaptive as ta
import test_light_tree as tl
import tree_reference as tr

F = np.float32
LENS = tl.LENS
ENV_PARAMS = dict(mode=1, scale=0.75)
SPP = dict(min_spp=4, batch_spp=4, max_spp=32)
THRESHOLD = 0.3
SIZE = (32, 24)


@functools.lru_cache(maxsize=None)
def sky():
    return er.sun_and_sky(256)


# name → (scene of test_light_tree.py, the restatement's keywords; "sky": the environment is sky())
SETTINGS = {
    "a": ("night rtiow", dict(select=1, nee_mis=1, planes=0)),
    "b": ("panel box", dict(select=1, nee_mis=1, planes=1)),
    "c": ("panel box", dict(select=0, nee_mis=0, planes=1)),
    "d": ("panel box", dict(select=1, nee_mis=1, planes=1, lens=LENS, sky=True)),
    "e": ("lamp", dict(select=0, emitters=False, sky=True)),
}


def reference_keywords(setting):
    """tree_reference.trace / frame keywords of a setting."""
    kw = dict(SETTINGS[setting][1])
    if kw.pop("sky", False):
        kw.update(rgb=sky(), env_params=ENV_PARAMS)
    return kw


def device_keywords(setting, env):
    """DeviceScene.render_lit[_adaptive] keywords of a setting; env: an rb.Env of sky() (used where the setting has the environment)."""
    s = SETTINGS[setting][1]
    kw = dict(emitters=s.get("emitters", True))
    if kw["emitters"]:
        kw["nee"] = {"mis": s["nee_mis"], "sample_planes": s["planes"], "select": s["select"]}
    if "lens" in s:
        kw["lens"] = dict(lens_radius=s["lens"][0], focus_distance=s["lens"][1])
    if s.get("sky"):
        kw.update(env=env, env_params=ENV_PARAMS)
    return kw


def radiances(host, cam, samples, sample_first=0, rows=None, tracer=None, **kw):
    """Per-sample radiances of rt_render_lit's estimator: (len(rows), W, samples, 3) float32 for samples sample_first … + samples - 1 of every
    pixel of the image rows `rows` (default: all).  ijs rows are (column, row, sample).  tracer: the restatement whose first column is the
    radiance (default tree_reference.trace; gloss_reference.trace for the glossy switches)."""
    rows = list(range(cam.image_height)) if rows is None else list(rows)
    jj, ii, ss = np.meshgrid(np.asarray(rows), np.arange(cam.image_width), sample_first + np.arange(samples), indexing="ij")
    ijs = np.stack([ii.ravel(), jj.ravel(), ss.ravel()], axis=1).astype(np.int32)
    rad = (tracer or tr.trace)(host, cam, ijs, **kw)[0]
    return rad.reshape(len(rows), cam.image_width, samples, 3)


def from_radiances(rad, min_spp, batch_spp, max_spp, threshold):
    """rad (rows, W, samples >= min + R * batch, 3) → (fb (rows, W, 3) float32 sums, spp (rows, W) int32, moments (rows, W, 2) float32)."""
    rows, w = rad.shape[:2]
    flat = rad.reshape(rows * w, rad.shape[2], 3)
    n, s1, s2 = ta.reference(flat, min_spp, batch_spp, max_spp, threshold)
    fb = np.zeros((rows * w, 3), F)
    for s in range(int(n.max())):
        fb = np.where((s < n)[:, None], (fb + flat[:, s]).astype(F), fb)
    return fb.reshape(rows, w, 3), n.astype(np.int32).reshape(rows, w), np.stack([s1, s2], axis=1).astype(F).reshape(rows, w, 2)


def reference(host, cam, min_spp, batch_spp, max_spp, threshold, sample_first=0, shard=None, tracer=None, **kw):
    """What render_lit_adaptive_to_host returns (without the timing), from the restatement (tracer: radiances')."""
    total = min_spp + (max_spp - min_spp) // batch_spp * batch_spp
    rad = radiances(host, cam, total, sample_first, er.image_rows(cam, shard), tracer=tracer, **kw)
    return from_radiances(rad, min_spp, batch_spp, max_spp, threshold)


@functools.lru_cache(maxsize=None)
def setting_radiances(setting, sample_first=0, size=SIZE, samples=SPP["max_spp"]):
    """The whole frame's radiances of a setting at `size` (cached and shared: do not write to it)."""
    name = SETTINGS[setting][0]
    rad = radiances(tl.scene(name), tl.camera(name, size[0], size[1], 1), samples, sample_first, **reference_keywords(setting))
    rad.setflags(write=False)
    return rad


def setting_reference(setting, sample_first=0, shard=None, threshold=THRESHOLD, size=SIZE, **spp):
    """(fb, spp, moments) of a setting under SPP (or the given rt_adaptive_params fields), the rows of `shard`."""
    p = {**SPP, **spp}
    name = SETTINGS[setting][0]
    rows = er.image_rows(tl.camera(name, size[0], size[1], 1), shard)
    rad = setting_radiances(setting, sample_first, size)[rows]
    return from_radiances(rad, p["min_spp"], p["batch_spp"], p["max_spp"], threshold)
