#!/usr/bin/env python3
"""rt_render_chroma against rt_render_volume on night rtiow at 1920 x 1080 x 16 spp (tools/volume_time.py's scene, setting and box fog at
optical depth 2: mis = 1, glossy = 1): device-event times, warmed, median of --reps with min and max.

Calls: (a) rt_render_volume without a grid and with the 32^3 grid of tools/volume_time.py — with --grey-only these alone, for a build that
has no rt_render_chroma (RTP_AMD_LIB selects it: the parent commit's); (b) rt_render_chroma at tint (1, 1, nextafter(1)): the same fog to
one ulp through the chroma kernels — their own cost — without and with the grid; (c) tint (0.5, 1, 2), without and with the grid.
Noise: at 480 x 270 the luminance MSE of (c) without a grid against a --truth-spp frame of other samples, at 16 and at 48 spp, and beside
them the MSE of a composite of three grey frames of 16 spp (channel k from rt_render_volume at sigma_t * tint[k]: 48 spp in all) — what the
channel weights cost in noise at equal samples.  JSON on stdout."""
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
    ap.add_argument("--grey-only", action="store_true", help="call (a) alone: for a build that has no rt_render_chroma")
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
    ulp = (1.0, 1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0))))
    tint = (0.5, 1.0, 2.0)
    out = {"reps": args.reps, "width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "medium": fog, "tint": tint, "calls": {}}
    with rb.Volume(vt.smooth_density(32)) as vol:
        grids = {"": None, "_32": vol}
        calls = {}
        for g, v in grids.items():
            calls["volume" + g] = lambda v=v: dev.render_volume(cam, fb.data_ptr(), medium=fog, volume=v, nee=nee, stream=s, sync=False)
            if not args.grey_only:
                calls["chroma_ulp" + g] = lambda v=v: dev.render_chroma(cam, fb.data_ptr(), medium=fog, volume=v, tint=ulp, nee=nee, stream=s, sync=False)
                calls["chroma" + g] = lambda v=v: dev.render_chroma(cam, fb.data_ptr(), medium=fog, volume=v, tint=tint, nee=nee, stream=s, sync=False)
        for _ in range(2):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        for name, fn in calls.items():
            r = mt.timed(fn, args.reps)
            r["msamples_per_s"] = px * cam.samples_per_pixel / r["ms"] / 1e3
            out["calls"][name] = r
        if not args.grey_only:
            for g in grids:
                for name in ("chroma_ulp", "chroma"):
                    out["calls"][name + g]["over_volume"] = out["calls"][name + g]["ms"] / out["calls"]["volume" + g]["ms"]
            # noise at equal samples, 480 x 270, no grid
            w, h = 480, 270
            luma = lambda frame, spp: (frame.astype(np.float64) / spp) @ LUMA
            small = lambda spp: nt.with_size(cam, w, h, spp)
            truth = luma(dev.render_chroma_to_host(small(args.truth_spp), medium=fog, tint=tint, nee=nee, sample_first=1 << 16)[0], args.truth_spp)
            mse = {}
            for spp in (16, 48):
                mse[f"chroma_{spp}spp"] = float(np.mean((luma(dev.render_chroma_to_host(small(spp), medium=fog, tint=tint, nee=nee)[0], spp) - truth) ** 2))
            grey = [dev.render_volume_to_host(small(16), medium=dict(fog, sigma_t=float(np.float32(fog["sigma_t"]) * np.float32(t))), nee=nee)[0][..., k]
                    for k, t in enumerate(tint)]
            mse["composite_3x16spp"] = float(np.mean((luma(np.stack(grey, -1), 16) - truth) ** 2))
            mse["chroma_48_over_composite"] = mse["chroma_48spp"] / mse["composite_3x16spp"]
            out["luminance_mse"] = dict(width=w, height=h, truth_spp=args.truth_spp, mean_luminance=float(truth.mean()), **mse)
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
