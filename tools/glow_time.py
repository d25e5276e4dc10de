#!/usr/bin/env python3
"""rt_render_glow against rt_render_volume on night rtiow at 1920 x 1080 x 16 spp (tools/volume_time.py's scene, setting and box fog at
optical depth 2: mis = 1, glossy = 1): device-event times, warmed, median of --reps with min and max.

Calls: (a) rt_render_volume without a grid and with the 32^3 grid of tools/volume_time.py — with --grey-only these alone, for a build that
has no rt_render_glow (RTP_AMD_LIB selects it: the parent commit's); (b) rt_render_glow under source 0 without a grid; (c) under source 1
with the grid; (d) under source 2 with the grid and a heat grid of the same size (the density mirrored: other values at every cell).
Noise (--noise): at 480 x 270 the luminance MSE of (b) at 16 spp against a --truth-spp frame of other samples, for a bright glow (the
call's radiance) and a dim one (a hundredth of it), each relative to its frame's mean luminance squared.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUMA = np.array([0.2126, 0.7152, 0.0722])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--grey-only", action="store_true", help="call (a) alone: for a build that has no rt_render_glow")
    ap.add_argument("--noise", action="store_true", help="the luminance MSE of a bright and a dim glow as well")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import medium_time as mt
    import nee_time as nt
    import volume_time as vt

    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    host, cam = nt.scenes()["night_rtiow"]
    dev = rb.DeviceScene(host, device=0)
    px = cam.image_width * cam.image_height
    fb = torch.empty(px * 3, device="cuda:0")
    nee = {"mis": 1, "glossy": 1}
    side, tau = 24.0, 2.0
    fog = dict(sigma_t=tau / side, albedo=0.9, g=0.5, box=(-side / 2,) * 3 + (side / 2,) * 3)
    radiance = (0.04, 0.02, 0.005)
    out = {"reps": args.reps, "width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "medium": fog, "radiance": radiance, "calls": {}}
    density = vt.smooth_density(32)
    with rb.Volume(density) as vol, rb.Volume(np.ascontiguousarray(density[::-1, ::-1, ::-1])) as heat:
        calls = {"volume": lambda: dev.render_volume(cam, fb.data_ptr(), medium=fog, nee=nee, stream=s, sync=False),
                 "volume_32": lambda: dev.render_volume(cam, fb.data_ptr(), medium=fog, volume=vol, nee=nee, stream=s, sync=False)}
        if not args.grey_only:
            calls["glow_source0"] = lambda: dev.render_glow(cam, fb.data_ptr(), medium=fog, glow=dict(radiance=radiance, source=0), nee=nee, stream=s, sync=False)
            calls["glow_source1_32"] = lambda: dev.render_glow(cam, fb.data_ptr(), medium=fog, volume=vol, glow=dict(radiance=radiance, source=1), nee=nee, stream=s,
                                                               sync=False)
            calls["glow_source2_32"] = lambda: dev.render_glow(cam, fb.data_ptr(), medium=fog, volume=vol, glow=dict(radiance=radiance, source=2), heat=heat, nee=nee,
                                                               stream=s, sync=False)
        for _ in range(2):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        for name, fn in calls.items():
            r = mt.timed(fn, args.reps)
            r["msamples_per_s"] = px * cam.samples_per_pixel / r["ms"] / 1e3
            out["calls"][name] = r
        if not args.grey_only:
            for name, base in (("glow_source0", "volume"), ("glow_source1_32", "volume_32"), ("glow_source2_32", "volume_32")):
                out["calls"][name]["over_volume"] = out["calls"][name]["ms"] / out["calls"][base]["ms"]
        if args.noise and not args.grey_only:
            w, h = 480, 270
            luma = lambda frame, spp: (frame.astype(np.float64) / spp) @ LUMA
            small = lambda spp: nt.with_size(cam, w, h, spp)
            mse = {}
            for name, scale in (("bright", 1.0), ("dim", 0.01)):
                glow = dict(radiance=tuple(scale * r for r in radiance), source=0)
                truth = luma(dev.render_glow_to_host(small(args.truth_spp), medium=fog, glow=glow, nee=nee, sample_first=1 << 16)[0], args.truth_spp)
                err = float(np.mean((luma(dev.render_glow_to_host(small(16), medium=fog, glow=glow, nee=nee)[0], 16) - truth) ** 2))
                mse[name] = dict(mse_16spp=err, mean_luminance=float(truth.mean()), relative=err / float(truth.mean()) ** 2)
            out["luminance_mse"] = dict(width=w, height=h, truth_spp=args.truth_spp, **mse)
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
