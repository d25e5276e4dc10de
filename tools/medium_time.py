#!/usr/bin/env python3
"""rt_render_medium against rt_render_lit on night rtiow at 1920 x 1080 x 16 spp (tools/nee_time.py's scene): device-event times, warmed,
median of --reps with the spread of the runs.

Calls, all with mis = 1 and glossy = 1: (a) rt_render_lit — the closest existing kernel; (b) rt_render_medium with a ball no ray touches
— the medium kernel's extra state alone; (c) a fog ball over the scene (centre the origin, radius 12) at optical depths 0.5 and 2 across
its diameter, albedo 0.9, g = 0.5.  Per call the medium events per sample from the probe on 20 000 random samples.
Quality under fog at equal GPU time, at a quarter of the resolution per axis: light samples with mis against the path alone
(sample_emitters = 0), luminance MSE against a --truth-spp frame of the mis estimator from a disjoint sample range.  JSON on stdout."""
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
    ap.add_argument("--truth-spp", type=int, default=4096)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import nee_time as nt

    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    host, cam = nt.scenes()["night_rtiow"]
    dev = rb.DeviceScene(host, device=0)
    px = cam.image_width * cam.image_height
    fb = torch.empty(px * 3, device="cuda:0")
    nee = {"mis": 1, "glossy": 1}
    diameter = 24.0
    media = {"unreachable_ball": dict(sigma_t=1.0, albedo=0.9, g=0.5, ball=(0.0, 0.0, 1.0e4, 1.0))}
    for tau in (0.5, 2.0):
        media[f"fog_tau_{tau}"] = dict(sigma_t=tau / diameter, albedo=0.9, g=0.5, ball=(0.0, 0.0, 0.0, diameter / 2))

    def make(ptr):
        calls = {"rt_render_lit": lambda c, first=0, **kw: dev.render_lit(c, ptr, nee=nee, stream=s, sync=False, sample_first=first, **kw)}
        for name, m in media.items():
            calls[name] = lambda c, first=0, m=m, **kw: dev.render_medium(c, ptr, medium=m, nee=nee, stream=s, sync=False, sample_first=first, **kw)
        return calls
    calls = make(fb.data_ptr())
    out = {"reps": args.reps, "width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "calls": {}}
    for _ in range(2):
        for fn in calls.values():
            fn(cam)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    n = 20000
    ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1)
    for name, fn in calls.items():
        r = timed(lambda: fn(cam), args.reps)
        r["msamples_per_s"] = px * cam.samples_per_pixel / r["ms"] / 1e3
        probe = dev.trace_samples_medium(cam, ijs, medium=media.get(name), nee=nee)
        r.update(queries_per_sample=float(probe[1].mean()), medium_events_per_sample=float(probe[2].mean()))
        out["calls"][name] = r
    a = out["calls"]["rt_render_lit"]
    for name in media:
        out["calls"][name]["over_rt_render_lit"] = out["calls"][name]["ms"] / a["ms"]
    out["rt_render_lit_scatter"] = (a["max_ms"] - a["min_ms"]) / a["ms"]
    # ---- quality under fog at equal GPU time: mis against the path alone
    w, h = cam.image_width // 4, cam.image_height // 4
    fbs = torch.empty(w * h * 3, device="cuda:0")
    fog = media["fog_tau_2.0"]
    est = {"mis": lambda c, first=0: dev.render_medium(c, fbs.data_ptr(), medium=fog, nee=nee, stream=s, sync=False, sample_first=first),
           "path_only": lambda c, first=0: dev.render_medium(c, fbs.data_ptr(), medium=fog, emitters=False, stream=s, sync=False, sample_first=first)}
    est["mis"](nt.with_size(cam, w, h, args.truth_spp), 1 << 28)
    torch.cuda.synchronize()
    truth = fbs.cpu().numpy().reshape(h, w, 3).astype(np.float64) / args.truth_spp @ LUM
    probe_cam = nt.with_size(cam, w, h, args.budget_spp)
    per_spp = {}
    for name, fn in est.items():
        fn(probe_cam, 0)
        per_spp[name] = timed(lambda: fn(probe_cam, 0), args.reps)["ms"] / args.budget_spp
    budget = per_spp["path_only"] * args.budget_spp
    q = {"width": w, "height": h, "truth_spp": args.truth_spp, "budget_ms": budget, "estimators": {}}
    for name, fn in est.items():
        spp = max(1, int(budget / per_spp[name]))
        fn(nt.with_size(cam, w, h, spp), 0)
        torch.cuda.synchronize()
        img = fbs.cpu().numpy().reshape(h, w, 3).astype(np.float64) / spp @ LUM
        q["estimators"][name] = {"ms_per_spp": per_spp[name], "spp": spp, "mse": float(((img - truth) ** 2).mean())}
    q["mse_mis_over_path_only"] = q["estimators"]["mis"]["mse"] / q["estimators"]["path_only"]["mse"]
    out["quality_equal_time"] = q
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
