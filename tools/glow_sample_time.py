#!/usr/bin/env python3
"""rt_render_glow_sampled (mis = 1) against rt_render_glow at 1920 x 1080 x 16 spp on two scenes: device-event times, warmed, median of
--reps with min and max, and the luminance MSE of both at equal GPU time.

Scenes: (a) the dark room of tests/test_glow_sampled.py — a black background, a diffuse floor and one wall, thin absorbing fog in a 16^3
grid whose heat is one 2^3 block, the fire just outside the view — where the sample should win; (b) tools/glow_time.py's night rtiow under
its 32^3 grid (source 1: the emission follows the density, all of the box glows dimly) — where it may lose.
Calls per scene: rt_render_glow, and unless --glow-only (for a build without the sampled call — RTP_AMD_LIB selects it: the parent commit's)
rt_render_glow_sampled with mis = 1.
Noise (--noise): at 480 x 270 against a --truth-spp frame of other samples (the sampled call's), the luminance MSE of the sampled call at 16
spp and of rt_render_glow at the sample count that takes the same GPU time at full size (16 * sampled ms / unsampled ms, rounded).
JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUMA = np.array([0.2126, 0.7152, 0.0722])
SPP = 16


def dark_room(rb, w, h, spp):
    """The scene, its camera, the call's keywords and the two grids."""
    quad = 0
    planes = np.array([[-2.5, 0, 2.5, 5, 0, 0, 0, 0, -5, 0, quad], [-2.5, 0, -2.5, 5, 0, 0, 0, 4.5, 0, 1, quad]], np.float32)
    mats = []
    for albedo in ((0.6, 0.6, 0.6), (0.7, 0.5, 0.4)):
        m = rb.Material()
        m.type = 0
        for k in range(3):
            m.albedo.e[k] = albedo[k]
        mats.append(m)
    host = rb.HostScene.from_arrays(np.array([[0, 1000, 0, 0.5, 0]], np.float32), planes, mats)
    cam = rb.make_camera(w, h, 25.0, (0, 3.2, 5.0), (0, 0.6, -0.5), (0, 0, 0), spp, 8)
    heat = np.zeros((16, 16, 16), np.float32)
    heat[3:5, 7:9, 7:9] = 1.0
    kw = dict(medium=dict(sigma_t=0.1, albedo=0.0, box=(-2, 0.25, -2, 2, 4.25, 2)), glow=dict(radiance=(20.0, 12.0, 4.0), source=2), emitters=False)
    return host, cam, kw, np.ones((16, 16, 16), np.float32), heat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--glow-only", action="store_true", help="rt_render_glow alone: for a build that has no rt_render_glow_sampled")
    ap.add_argument("--noise", action="store_true", help="the luminance MSE at equal GPU time as well")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import medium_time as mt
    import nee_time as nt
    import volume_time as vt

    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    night_host, night_cam = nt.scenes()["night_rtiow"]
    side, tau = 24.0, 2.0
    night_kw = dict(medium=dict(sigma_t=tau / side, albedo=0.9, g=0.5, box=(-side / 2,) * 3 + (side / 2,) * 3), glow=dict(radiance=(0.04, 0.02, 0.005), source=1),
                    nee={"mis": 1, "glossy": 1})
    room_host, room_cam, room_kw, room_density, room_heat = dark_room(rb, night_cam.image_width, night_cam.image_height, SPP)
    scenes = {"dark_room": (room_host, room_cam, room_kw, room_density, room_heat, 2), "night_rtiow": (night_host, night_cam, night_kw, vt.smooth_density(32), None, 1)}
    out = {"reps": args.reps, "width": night_cam.image_width, "height": night_cam.image_height, "spp": SPP, "scenes": {}}
    for name, (host, cam, kw, density, heat_grid, source) in scenes.items():
        dev = rb.DeviceScene(host, device=0)
        px = cam.image_width * cam.image_height
        fb = torch.empty(px * 3, device="cuda:0")
        res = {"calls": {}}
        with rb.Volume(density) as vol:
            heat = rb.Volume(heat_grid) if heat_grid is not None else None
            sampler = None if args.glow_only else rb.GlowSampler(vol, source, heat)
            calls = {"glow": lambda: dev.render_glow(cam, fb.data_ptr(), volume=vol, heat=heat, stream=s, sync=False, **kw)}
            if not args.glow_only:
                calls["glow_sampled_mis"] = lambda: dev.render_glow_sampled(cam, fb.data_ptr(), volume=vol, heat=heat, sample="mis", sampler=sampler, stream=s,
                                                                            sync=False, **kw)
            for _ in range(2):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            for call, fn in calls.items():
                r = mt.timed(fn, args.reps)
                r["msamples_per_s"] = px * SPP / r["ms"] / 1e3
                res["calls"][call] = r
            if not args.glow_only:
                ratio = res["calls"]["glow_sampled_mis"]["ms"] / res["calls"]["glow"]["ms"]
                res["calls"]["glow_sampled_mis"]["over_glow"] = ratio
                if args.noise:
                    w, h = 480, 270
                    small = lambda spp: nt.with_size(cam, w, h, spp)          # noqa: E731
                    luma = lambda frame, spp: (frame.astype(np.float64) / spp) @ LUMA          # noqa: E731
                    same = dict(volume=vol, heat=heat, **kw)
                    truth = luma(dev.render_glow_sampled_to_host(small(args.truth_spp), sample="mis", sampler=sampler, sample_first=1 << 16, **same)[0], args.truth_spp)
                    equal_spp = max(1, int(round(SPP * ratio)))
                    mse_sampled = float(np.mean((luma(dev.render_glow_sampled_to_host(small(SPP), sample="mis", sampler=sampler, **same)[0], SPP) - truth) ** 2))
                    mse_same_spp = float(np.mean((luma(dev.render_glow_to_host(small(SPP), **same)[0], SPP) - truth) ** 2))
                    mse_same_time = float(np.mean((luma(dev.render_glow_to_host(small(equal_spp), **same)[0], equal_spp) - truth) ** 2))
                    res["luminance_mse"] = dict(width=w, height=h, truth_spp=args.truth_spp, mean_luminance=float(truth.mean()), sampled_16spp=mse_sampled,
                                                glow_16spp=mse_same_spp, glow_equal_time_spp=equal_spp, glow_equal_time=mse_same_time,
                                                sampled_over_glow_equal_time=mse_sampled / mse_same_time)
            if sampler is not None:
                sampler.close()
            if heat is not None:
                heat.close()
        dev.close()
        out["scenes"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
