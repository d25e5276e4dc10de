#!/usr/bin/env python3
"""rt_render_lens on S-rtiow at 1920x1080 x 64 spp: device-event times, warmed, median of --reps.

Five configurations: default rt_render (candidate lists), rt_render with primary_visibility = -1 (every sample traced from its camera:
the yardstick of a lens frame) — and beside it the same with sphere_only_kernel = -1, the general build of the walk that lens frames
run —, lens only (R = 0.1, focus on the scene centre), motion only (two poses of an orbit-like swing) and
both.  Per configuration: ms, Msamples/s, the ratio to the yardstick, the walk that ran and the share of samples it flagged.
--only NAME renders that configuration once and exits (for a profiler run of one lens frame).  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
import rtp_bindings as rb  # noqa: E402


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(args.width, args.height, args.spp, 50)
    close = rb.make_camera(args.width, args.height, 20.0, (12.6, 3.6, 2.1), (0, 0, 0), (0.7, 0.8, 1.0), args.spp, 50)
    focus = float(np.sqrt(13.0 ** 2 + 3.0 ** 2 + 2.0 ** 2))
    lens = {"lens_radius": args.radius, "focus_distance": focus}
    default = rb.DeviceScene(host, device=0)
    no_lists = rb.DeviceScene(host, device=0, primary_visibility=-1)
    general = rb.DeviceScene(host, device=0, primary_visibility=-1, sphere_only_kernel=-1)      # the general build lens frames run
    px = args.width * args.height
    fb = torch.empty(px * 3, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    configs = {
        "rt_render": lambda: default.render(cam, fb.data_ptr(), stream=s, sync=False),
        "rt_render_pv_off": lambda: no_lists.render(cam, fb.data_ptr(), stream=s, sync=False),
        "rt_render_pv_off_general": lambda: general.render(cam, fb.data_ptr(), stream=s, sync=False),
        "lens": lambda: default.render_lens(cam, fb.data_ptr(), lens=lens, stream=s, sync=False),
        "motion": lambda: default.render_lens(cam, fb.data_ptr(), cam_close=close, stream=s, sync=False),
        "both": lambda: default.render_lens(cam, fb.data_ptr(), cam_close=close, lens=lens, stream=s, sync=False),
    }
    if args.only:
        configs[args.only]()
        torch.cuda.synchronize()
        return
    for _ in range(2):      # warm: buffers, view lists, the handle's walk decision
        for fn in configs.values():
            fn()
    torch.cuda.synchronize()
    out = {"scene": "S-rtiow", "width": args.width, "height": args.height, "spp": args.spp, "lens_radius": args.radius,
           "focus_distance": focus, "reps": args.reps, "configs": {}}
    for name, fn in configs.items():
        ms = timed(fn, args.reps)
        rec = {"ms": ms, "msamples_per_s": px * args.spp / ms / 1e3}
        # the walk that ran, and what it flagged: one synchronous call of the same configuration
        if name.startswith("rt_render"):
            d = {"rt_render": default, "rt_render_pv_off": no_lists, "rt_render_pv_off_general": general}[name]
            d.render(cam, fb.data_ptr(), stream=s, sync=True)
            t = d.last_timing()
        else:
            kw = {"lens": lens} if name in ("lens", "both") else {}
            if name in ("motion", "both"):
                kw["cam_close"] = close
            t = default.render_lens(cam, fb.data_ptr(), stream=s, sync=True, **kw)
        rec.update(guarded=int(t.guarded), flagged_share=float(t.flagged_samples) / (px * args.spp), primary_visibility=int(t.primary_visibility),
                   trace_vgprs=int(t.trace_vgprs), trace_scratch_bytes=int(t.trace_scratch_bytes))
        out["configs"][name] = rec
    yard = out["configs"]["rt_render_pv_off"]["ms"]
    for rec in out["configs"].values():
        rec["vs_pv_off"] = rec["ms"] / yard
    default.close()
    no_lists.close()
    general.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
