#!/usr/bin/env python3
"""rt_render_fog_adaptive against the frame call of its rung at the same mean sample count: device-event times, warmed,
median of --reps with min – max.  Modelled on tools/volume_adaptive_time.py.

Scenes, 1920 x 1080: tint — tools/chroma_time.py's night rtiow under the box fog at optical depth 2 and tint (0.5, 1, 2), no grid; glow —
tools/glow_sample_time.py's night rtiow under its 32^3 grid, source 1; sampled — its dark room, where a fire outside the view lights the
room (mis = 1).  Min 16, batch 16, max 256, threshold 0.05 (--spp, --threshold).  Per rung: the whole call, its mean spp and the histogram of
stop levels; the rung's frame call at the rounded mean spp and at min_spp; the min_spp frame of the adaptive call (max_spp = min_spp);
each round's time as the difference of two calls whose caps lie one round apart, the samples the round traced (from the histogram) and its
rate beside the frame call's uniform rate — what the list kernels cost.
--noise: on the dark room at 480 x 270, the luminance MSE against a --truth-spp frame of other samples of the adaptive call and of the
uniform sampled call at the sample count that takes the same GPU time.
--unchanged: rt_render_chroma, rt_render_glow and rt_render_glow_sampled at 16 spp and rt_render_volume_adaptive alone, on whatever library
RTP_AMD_LIB names (the parent commit's build, for the comparison of the kernels this change does not touch).  JSON on stdout, or into --out."""
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
    ap.add_argument("--spp", default="16:16:256")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--rungs", default="tint,glow,sampled")
    ap.add_argument("--no-rounds", action="store_true", help="leave the per-round differences out")
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import glow_sample_time as gst
    import medium_time as mt
    import nee_time as nt
    import volume_time as vt

    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    mn, batch, mx = (int(x) for x in args.spp.split(":"))
    rounds = (mx - mn) // batch
    night_host, night_cam = nt.scenes()["night_rtiow"]
    w, h = night_cam.image_width, night_cam.image_height
    side, tau = 24.0, 2.0
    box_fog = dict(sigma_t=tau / side, albedo=0.9, g=0.5, box=(-side / 2,) * 3 + (side / 2,) * 3)
    nee = {"mis": 1, "glossy": 1}
    room_host, room_cam, room_kw, room_density, room_heat = gst.dark_room(rb, w, h, 16)
    # rung → (host, camera, density, heat, the sampler's source or None, the frame method's name, the keywords without the device objects)
    scenes = {
        "tint": (night_host, night_cam, None, None, None, "render_chroma", dict(medium=box_fog, tint=(0.5, 1.0, 2.0), nee=nee)),
        "glow": (night_host, night_cam, vt.smooth_density(32), None, None, "render_glow", dict(medium=box_fog, glow=dict(radiance=(0.04, 0.02, 0.005), source=1), nee=nee)),
        "sampled": (room_host, room_cam, room_density, room_heat, 2, "render_glow_sampled", dict(sample="mis", **room_kw)),
    }
    out = {"library": os.environ.get("RTP_AMD_LIB", "this tree's"), "reps": args.reps, "width": w, "height": h, "min_spp": mn, "batch_spp": batch, "max_spp": mx,
           "threshold": args.threshold, "rungs": {}}
    px = w * h
    fb = torch.empty(px * 3, device="cuda:0")
    spp = torch.empty(px, dtype=torch.int32, device="cuda:0")
    mom = torch.empty(px * 2, device="cuda:0")

    def at(cam, n):
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = int(n)
        return c

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        return mt.timed(fn, args.reps)

    for rung in args.rungs.split(","):
        host, cam, density, heat_grid, source, method, kw = scenes[rung]
        dev = rb.DeviceScene(host, device=0)
        vol = rb.Volume(density) if density is not None else None
        heat = rb.Volume(heat_grid) if heat_grid is not None else None
        sampler = rb.GlowSampler(vol, source, heat) if source is not None else None
        kw = dict(kw, volume=vol)
        if rung != "tint":
            kw["heat"] = heat
        if sampler is not None:
            kw["sampler"] = sampler
        frame = getattr(dev, method)
        res = {}
        if args.unchanged:
            r = timed(lambda: frame(at(cam, 16), fb.data_ptr(), stream=s, sync=False, **kw))
            r["msamples_per_s"] = px * 16 / r["ms"] / 1e3
            res["frame_16spp"] = r
            if rung == "glow":
                grey = dict(medium=box_fog, volume=vol, nee=nee)
                res["volume_adaptive"] = timed(lambda: dev.render_volume_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), stream=s, sync=False, min_spp=mn,
                                                                                  batch_spp=batch, max_spp=mx, threshold=args.threshold, **grey))
        else:
            def adaptive(cap, camera=cam):
                return dev.render_fog_adaptive(camera, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), stream=s, sync=False, min_spp=mn, batch_spp=batch, max_spp=cap,
                                               threshold=args.threshold, **kw)
            whole = timed(lambda: adaptive(mx))
            counts = spp.cpu().numpy()
            levels = [mn + k * batch for k in range(rounds + 1)]
            hist = {n: int((counts == n).sum()) for n in levels}
            mean = float(counts.mean())
            whole.update(mean_spp=mean, msamples_per_s=float(counts.sum()) / whole["ms"] / 1e3)
            res.update(whole=whole, histogram=hist)
            for name, n in (("frame_at_mean_spp", int(round(mean))), ("frame_at_min_spp", mn)):
                r = timed(lambda n=n: frame(at(cam, n), fb.data_ptr(), stream=s, sync=False, **kw))
                r.update(spp=n, msamples_per_s=px * n / r["ms"] / 1e3)
                res[name] = r
            res["whole_over_frame_at_mean"] = whole["ms"] / res["frame_at_mean_spp"]["ms"]
            res["min_spp_frame"] = timed(lambda: adaptive(mn))
            res["min_spp_frame_over_frame"] = res["min_spp_frame"]["ms"] / res["frame_at_min_spp"]["ms"]
            if not args.no_rounds:
                caps = [timed(lambda c=c: adaptive(c))["ms"] for c in levels]
                per_round = []
                for r in range(1, rounds + 1):
                    going = sum(v for n, v in hist.items() if n >= levels[r])
                    ms = caps[r] - caps[r - 1]
                    per_round.append(dict(round=r, pixels=going, samples=going * batch, ms=ms, msamples_per_s=going * batch / ms / 1e3 if ms > 0 else None))
                res["rounds"] = per_round
                traced = sum(p["samples"] for p in per_round)
                spent = caps[-1] - caps[0]
                res["rounds_msamples_per_s"] = traced / spent / 1e3 if spent > 0 else None
                res["rounds_rate_over_uniform"] = res["rounds_msamples_per_s"] / res["frame_at_mean_spp"]["msamples_per_s"] if spent > 0 else None
            if args.noise and rung == "sampled":
                sw, sh = 480, 270
                small = lambda n: nt.with_size(cam, sw, sh, n)          # noqa: E731
                luma = lambda mean_rgb: mean_rgb.astype(np.float64) @ LUMA          # noqa: E731
                truth = luma(dev.render_glow_sampled_to_host(small(args.truth_spp), sample_first=1 << 16, **kw)[0] / args.truth_spp)
                t_adaptive = timed(lambda: adaptive(mx, small(1)))
                a_fb, a_spp, _, _ = dev.render_fog_adaptive_to_host(small(1), min_spp=mn, batch_spp=batch, max_spp=mx, threshold=args.threshold, **kw)
                t_uniform = timed(lambda: frame(small(mn), fb.data_ptr(), stream=s, sync=False, **kw))
                equal = max(1, int(round(mn * t_adaptive["ms"] / t_uniform["ms"])))
                t_equal = timed(lambda: frame(small(equal), fb.data_ptr(), stream=s, sync=False, **kw))
                u_fb = dev.render_glow_sampled_to_host(small(equal), **kw)[0]
                mse_a = float(np.mean((luma(a_fb / a_spp[..., None]) - truth) ** 2))
                mse_u = float(np.mean((luma(u_fb / equal) - truth) ** 2))
                res["luminance_mse"] = dict(width=sw, height=sh, truth_spp=args.truth_spp, mean_luminance=float(truth.mean()), adaptive_ms=t_adaptive["ms"],
                                            adaptive_mean_spp=float(a_spp.mean()), adaptive=mse_a, uniform_spp=equal, uniform_ms=t_equal["ms"], uniform=mse_u,
                                            adaptive_over_uniform=mse_a / mse_u)
        for obj in (sampler, heat, vol):
            if obj is not None:
                obj.close()
        dev.close()
        out["rungs"][rung] = res
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
