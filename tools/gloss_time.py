#!/usr/bin/env python3
"""The glossy switch of rt_render_nee and rt_render_lit against the same calls without it, and against rt_render: device-event times
(warmed, median of --reps, with the spread of the runs) and quality at equal GPU time.

Scenes: tools/nee_time.py's — the config scene (tests/golden/config.txt, frame 0) at its own 1080 x 720 and spp, and night rtiow at
1920 x 1080 x 16.  Calls: rt_render, rt_render_nee and rt_render_lit (pinhole, no environment: its emitters alone) with glossy 0 and 1,
all with mis = 1.  Per call: ms per frame (median, min, max), and closest-hit queries per sample from the probes on 20 000 random samples
— the surplus over rt_render's is the shadow rays.
Quality at equal time, at a quarter of the resolution in each direction: the per-sample time of each call there, the spp each affords in
the time rt_render takes for --budget-spp, and the luminance MSE of that frame against a ground truth (rt_render_nee, glossy = 1, at
--truth-spp from a disjoint sample range); the ratios against glossy = 0 and against rt_render.
--baseline: only the glossy = 0 calls, through parameters a library from before the switch understands too; with --package DIR (another
checkout's ray-tracing-practice_amd) that is the same measurement on that checkout's library.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUM = np.array([0.2126, 0.7152, 0.0722])


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs_ms": [float(x) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget-spp", type=int, default=64)
    ap.add_argument("--truth-spp", type=int, default=8192)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--package", default=os.path.join(ROOT, "ray-tracing-practice_amd"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import nee_time as nt          # (its scenes and with_size; it imports the same rtp_bindings)

    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    out = {"reps": args.reps, "package": os.path.abspath(args.package), "baseline": args.baseline, "scenes": {}}
    for sname, (host, cam) in nt.scenes().items():
        dev = rb.DeviceScene(host, device=0)
        px = cam.image_width * cam.image_height
        fb = torch.empty(px * 3, device="cuda:0")

        def nee(g):
            return {"mis": 1} if args.baseline else {"mis": 1, "glossy": g}

        def make(ptr):
            calls = {"rt_render": lambda c, first=0: dev.render(c, ptr, stream=s, sync=False, sample_first=first)}
            for g in (0,) if args.baseline else (0, 1):
                calls[f"nee_glossy{g}"] = lambda c, first=0, g=g: dev.render_nee(c, ptr, params=nee(g), stream=s, sync=False, sample_first=first)
                calls[f"lit_glossy{g}"] = lambda c, first=0, g=g: dev.render_lit(c, ptr, nee=nee(g), stream=s, sync=False, sample_first=first)
            return calls
        calls = make(fb.data_ptr())
        rec = {"width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "calls": {}}
        for _ in range(2):
            for fn in calls.values():
                fn(cam)
        torch.cuda.synchronize()
        rng = np.random.default_rng(1)
        n = 20000
        ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1)
        plain_rays = float(dev.trace_samples(cam, ijs)[1].mean())
        for name, fn in calls.items():
            r = timed(lambda: fn(cam), args.reps)
            r.update(msamples_per_s=px * cam.samples_per_pixel / r["ms"] / 1e3, queries_per_sample=plain_rays)
            if name != "rt_render":
                g = int(name[-1])
                q = float((dev.trace_samples_nee(cam, ijs, params=nee(g)) if name.startswith("nee") else dev.trace_samples_lit(cam, ijs, nee=nee(g)))[1].mean())
                r.update(queries_per_sample=q, shadow_rays_per_sample=q - plain_rays)
            rec["calls"][name] = r
        if not args.baseline:
            # ---- quality at equal GPU time, a quarter of the resolution per axis
            w, h = cam.image_width // 4, cam.image_height // 4
            fbs = torch.empty(w * h * 3, device="cuda:0")
            sm = make(fbs.data_ptr())
            truth_cam = nt.with_size(cam, w, h, args.truth_spp)
            dev.render_nee(truth_cam, fbs.data_ptr(), params=nee(1), stream=s, sync=True, sample_first=1 << 28)
            torch.cuda.synchronize()
            truth = fbs.cpu().numpy().reshape(h, w, 3).astype(np.float64) / args.truth_spp @ LUM
            per_spp = {}
            probe = nt.with_size(cam, w, h, args.budget_spp)
            for name, fn in sm.items():
                fn(probe, 0)
                per_spp[name] = timed(lambda: fn(probe, 0), args.reps)["ms"] / args.budget_spp
            budget = per_spp["rt_render"] * args.budget_spp
            q = {"width": w, "height": h, "truth_spp": args.truth_spp, "budget_ms": budget, "estimators": {}}
            for name, fn in sm.items():
                row = {"ms_per_spp": per_spp[name]}
                for label, spp in (("equal_time", max(1, int(budget / per_spp[name]))), ("equal_samples", args.budget_spp)):
                    c = nt.with_size(cam, w, h, spp)
                    fn(c, 0)
                    torch.cuda.synchronize()
                    img = fbs.cpu().numpy().reshape(h, w, 3).astype(np.float64) / spp @ LUM
                    row[label] = {"spp": spp, "mse": float(((img - truth) ** 2).mean())}
                q["estimators"][name] = row
            for label in ("equal_time", "equal_samples"):
                base = q["estimators"]["rt_render"][label]["mse"]
                for name, e in q["estimators"].items():
                    e[label]["mse_vs_rt_render"] = e[label]["mse"] / base
                    if name.endswith("glossy1"):
                        e[label]["mse_vs_glossy0"] = e[label]["mse"] / q["estimators"][name[:-1] + "0"][label]["mse"]
            rec["quality"] = q
        out["scenes"][sname] = rec
        dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
