#!/usr/bin/env python3
"""rt_render_lit_adaptive against rt_render_lit at the same mean sample count: device-event times (warmed, median of --reps).

Scenes: night rtiow (select = 1, mis = 1) and panel box (sample_planes = 1, select = 1, mis = 1) — tools/tree_time.py's — at 1920 x 1080,
min 16, batch 16, max 256, threshold 0.05.  Per scene: the whole call's ms, the mean spp and the histogram of stop levels; each round's
time as the difference of two calls (max_spp = min + r * batch against min + (r - 1) * batch: the rule never looks at max_spp except as
the cap, so call r runs exactly the first r rounds of the full call), the samples the round traced (from the histogram) and its rate;
rt_render_lit at the rounded mean spp and at min_spp; rt_render_adaptive for the handle's other adaptive path.
--package DIR loads rtp_bindings and the libraries of another build of this project (the parent commit's): a build without
rt_render_lit_adaptive times rt_render_lit (at --lit-spp, a list of sample counts) and rt_render_adaptive alone.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tree_time import night_rtiow, panel_box, timed          # noqa: E402  (the scenes and the clock of the tree's measurements)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", default="16:16:256")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--lit-spp", default="", help="comma-separated sample counts to time rt_render_lit at, beside the ones the run finds")
    ap.add_argument("--no-rounds", action="store_true", help="skip the per-round differences")
    ap.add_argument("--package", default=os.path.join(ROOT, "ray-tracing-practice_amd"))
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import rtp_bindings as rb
    rb.amd_lib().rt_set_device(0)
    mn, batch, mx = (int(x) for x in args.spp.split(":"))
    rounds = (mx - mn) // batch
    has_call = hasattr(rb.DeviceScene, "render_lit_adaptive")
    s = torch.cuda.current_stream().cuda_stream
    scenes = {"night_rtiow": (night_rtiow(rb), rb.make_camera(1920, 1080, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), mn, 50), 0),
              "panel_box_planes": (panel_box(rb), rb.make_camera(1920, 1080, 50.0, (0, 3, 10), (0, 1.8, 0), (0, 0, 0), mn, 50), 1)}
    out = {"package": os.path.relpath(args.package, ROOT), "reps": args.reps, "lit_adaptive": has_call, "min_spp": mn, "batch_spp": batch, "max_spp": mx,
           "threshold": args.threshold, "scenes": {}}
    for sname, (host, cam, planes) in scenes.items():
        nee = {"mis": 1, "sample_planes": planes, "select": 1}
        dev = rb.DeviceScene(host, device=0)
        px = cam.image_width * cam.image_height
        fb = torch.empty(px * 3, device="cuda:0")
        spp = torch.empty(px, dtype=torch.int32, device="cuda:0")
        mom = torch.empty(px * 2, device="cuda:0")
        rec = {"width": cam.image_width, "height": cam.image_height}

        def lit(n):
            c = rb.CameraData.from_buffer_copy(cam)
            c.samples_per_pixel = n
            return lambda: dev.render_lit(c, fb.data_ptr(), nee=nee, stream=s, sync=False)

        def adaptive(cap):
            return lambda: dev.render_lit_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), nee=nee, stream=s, sync=False, min_spp=mn,
                                                   batch_spp=batch, max_spp=cap, threshold=args.threshold)
        lit_counts = {mn} | {int(x) for x in args.lit_spp.split(",") if x}
        if has_call:
            full = adaptive(mx)
            for _ in range(2):
                full()
            torch.cuda.synchronize()
            counts = spp.cpu().numpy()
            levels, pixels = np.unique(counts, return_counts=True)
            mean_spp = float(counts.mean())
            lit_counts.add(max(1, int(round(mean_spp))))
            rec["lit_adaptive"] = {"ms": None, "mean_spp": mean_spp, "levels": {int(k): int(v) for k, v in zip(levels, pixels)}}
        lit_calls = {n: lit(n) for n in sorted(lit_counts)}
        plain = lambda: dev.render_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), stream=s, sync=False, min_spp=mn, batch_spp=batch,  # noqa: E731
                                            max_spp=mx, threshold=args.threshold)
        for fn in list(lit_calls.values()) + [plain]:
            fn()
        torch.cuda.synchronize()
        # alternating: the calls whose times are compared with each other run next to each other
        rec["rt_render_lit"] = {}
        if has_call:
            rec["lit_adaptive"]["ms"] = timed(full, args.reps)
            rec["lit_adaptive"]["msamples_per_s"] = px * mean_spp / rec["lit_adaptive"]["ms"] / 1e3
        for n, fn in lit_calls.items():
            ms = timed(fn, args.reps)
            rec["rt_render_lit"][n] = {"ms": ms, "msamples_per_s": px * n / ms / 1e3}
        if has_call:
            rec["lit_adaptive"]["ms_again"] = timed(full, args.reps)          # (the run-to-run scatter of this visit)
        rec["rt_render_adaptive"] = {"ms": timed(plain, args.reps)}
        torch.cuda.synchronize()
        rec["rt_render_adaptive"]["mean_spp"] = float(spp.cpu().numpy().mean())
        if has_call and not args.no_rounds:
            prev = None
            rec["rounds"] = []
            for r in range(rounds + 1):
                fn = adaptive(mn + r * batch)
                fn()
                ms = timed(fn, args.reps)
                if r > 0:
                    going = int((counts >= mn + r * batch).sum())
                    d = ms - prev
                    rec["rounds"].append({"round": r, "pixels": going, "samples": going * batch, "ms": d,
                                          "msamples_per_s": going * batch / d / 1e3 if d > 0 and going else None})
                else:
                    rec["min_spp_frame_with_moments_and_select_ms"] = ms
                prev = ms
        out["scenes"][sname] = rec
        dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
