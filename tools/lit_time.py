#!/usr/bin/env python3
"""rt_render_lit against the calls it composes: device-event times (warmed, median of --reps), closest-hit queries and shadow rays per
sample.

Scenes: the config scene (tests/golden/config.txt, frame 0; z-up, so the map is turned by the --env-up z rotation) at its own
1080 x 720 and spp, and night rtiow (every eighth small sphere an emitter) at 1920 x 1080 x 16, both under the sun-and-sky map of
tests/env_reference.py (n = 256).  Calls: rt_render_lit with both lights (pinhole, and with a 0.2 : 12 lens and an open shutter — the
kLens kernel), rt_render_lit in its two single-light identity cases, and rt_render_nee and rt_render_env, which those two equal bit
for bit.  Per call: ms per frame, Msamples/s, and from the probes on 20 000 random samples the closest-hit queries and the shadow rays
per sample (the probe's rays minus the path-alone probe's).  identity_cost: the identity cases' time over their dedicated call's.
--only NAME:SCENE renders that configuration once (for a profiler run).  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtp_bindings as rb  # noqa: E402
import env_reference as er  # noqa: E402  (the maps' formulas only: nothing is built)
from nee_time import night_rtiow, timed  # noqa: E402

LENS = dict(lens_radius=0.2, focus_distance=12.0)


def scenes():
    text = open(os.path.join(ROOT, "tests", "golden", "config.txt")).read()
    text = text.replace("../floor2.jpg", os.path.join(ROOT, "tests", "golden", "floor.jpg"))
    config = rb.HostScene.from_config(text)
    night_cam = rb.make_camera(1920, 1080, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), 16, 50)
    night_close = rb.make_camera(1920, 1080, 20.0, (12.9, 3.05, 2.1), (0, 0, 0), (0, 0, 0), 16, 50)
    return {"config": (config, config.frame_camera(0), config.frame_camera_at(0.5), er.Z_UP),
            "night_rtiow": (night_rtiow(), night_cam, night_close, None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    out = {"reps": args.reps, "scenes": {}}
    env = rb.Env(er.sun_and_sky(256))
    for sname, (host, cam, close, rot) in scenes().items():
        dev = rb.DeviceScene(host, device=0)
        px = cam.image_width * cam.image_height
        fb = torch.empty(px * 3, device="cuda:0")
        ep = dict(mode=1) if rot is None else dict(mode=1, rot=rot)
        settings = {
            "lit_both": dict(env=env, env_params=ep),
            "lit_both_lens_motion": dict(env=env, env_params=ep, cam_close=close, lens=LENS),
            "lit_emitters_only": dict(),
            "lit_env_only": dict(emitters=False, env=env, env_params=ep),
        }
        calls = {name: (lambda kw: lambda: dev.render_lit(cam, fb.data_ptr(), stream=s, sync=False, **kw))(kw) for name, kw in settings.items()}
        calls["rt_render_nee"] = lambda: dev.render_nee(cam, fb.data_ptr(), stream=s, sync=False)
        calls["rt_render_env"] = lambda: dev.render_env(cam, env, fb.data_ptr(), params=ep, stream=s, sync=False)
        if args.only:
            name, only_scene = args.only.split(":")
            if only_scene == sname:
                calls[name]()
                torch.cuda.synchronize()
            dev.close()
            continue
        rec = {"width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "calls": {}}
        for _ in range(2):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        rng = np.random.default_rng(1)
        n = 20000
        ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1)
        probes = {name: dev.trace_samples_lit(cam, ijs, **kw)[1] for name, kw in settings.items()}
        probes["rt_render_nee"] = dev.trace_samples_nee(cam, ijs)[1]
        probes["rt_render_env"] = dev.trace_samples_env(cam, env, ijs, params=ep)[1]
        # the path alone, from the same camera: the light streams do not move the path's, so the surplus is the shadow rays
        path = float(dev.trace_samples_lit(cam, ijs, emitters=False)[1].mean())
        path_lens = float(dev.trace_samples_lit(cam, ijs, emitters=False, cam_close=close, lens=LENS)[1].mean())
        for name, fn in calls.items():
            ms = timed(fn, args.reps)
            q = path_lens if name == "lit_both_lens_motion" else path
            rec["calls"][name] = {"ms": ms, "msamples_per_s": px * cam.samples_per_pixel / ms / 1e3, "queries_per_sample": q,
                                  "shadow_rays_per_sample": float(probes[name].mean()) - q}
        c = rec["calls"]
        rec["identity_cost"] = {"emitters_only_over_rt_render_nee": c["lit_emitters_only"]["ms"] / c["rt_render_nee"]["ms"],
                                "env_only_over_rt_render_env": c["lit_env_only"]["ms"] / c["rt_render_env"]["ms"]}
        # run-to-run spread of the dedicated calls: a second median of the same call over the first
        rec["spread"] = {name: timed(calls[name], args.reps) / c[name]["ms"] for name in ("rt_render_nee", "rt_render_env")}
        out["scenes"][sname] = rec
        dev.close()
    env.close()
    if not args.only:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
