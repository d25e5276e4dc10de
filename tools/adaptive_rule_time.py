#!/usr/bin/env python3
"""The adaptive calls under both stopping rules: device-event times (warmed, median of --reps).

rtiow at 1920 x 1080 through rt_render_adaptive and night rtiow (select = 1, mis = 1; tools/tree_time.py's) through
rt_render_lit_adaptive, min 16, batch 16, max 256.  Rule 0 at its threshold (--threshold, --lit-threshold), timed twice with the other
calls between (the visit's run-to-run scatter).  Rule 1 at the threshold of --near-thresholds whose mean spp is nearest rule 0's: the
whole call, its mean spp and its stop levels.
--package DIR loads rtp_bindings and the libraries of another build of this project (the parent commit's): a build without
rt_render_adaptive_rule times the two unchanged calls alone.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tree_time import night_rtiow, timed          # noqa: E402  (the scene and the clock of the tree's measurements)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", default="16:16:256")
    ap.add_argument("--threshold", type=float, default=0.02, help="rule 0's threshold on rtiow (the default of rt_adaptive_params)")
    ap.add_argument("--lit-threshold", type=float, default=0.05, help="rule 0's threshold on night rtiow (§19's)")
    ap.add_argument("--near-thresholds", default="0.01,0.015,0.02,0.03,0.04,0.05,0.07,0.1")
    ap.add_argument("--package", default=os.path.join(ROOT, "ray-tracing-practice_amd"))
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import rtp_bindings as rb
    rb.amd_lib().rt_set_device(0)
    mn, batch, mx = (int(x) for x in args.spp.split(":"))
    has_rule = hasattr(rb.amd_lib(), "rt_render_adaptive_rule")
    s = torch.cuda.current_stream().cuda_stream
    near_ts = [float(x) for x in args.near_thresholds.split(",") if x]
    out = {"package": os.path.relpath(args.package, ROOT), "reps": args.reps, "rule_calls": has_rule, "min_spp": mn, "batch_spp": batch, "max_spp": mx,
           "scenes": {}}
    scenes = {"rtiow": (rb.HostScene.rtiow(), rb.rtiow_camera(1920, 1080, mn, 50), None, args.threshold),
              "night_rtiow": (night_rtiow(rb), rb.make_camera(1920, 1080, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), mn, 50), {"mis": 1, "sample_planes": 0, "select": 1},
                              args.lit_threshold)}
    for sname, (host, cam, nee, t0) in scenes.items():
        dev = rb.DeviceScene(host, device=0)
        px = cam.image_width * cam.image_height
        fb = torch.empty(px * 3, device="cuda:0")
        spp = torch.empty(px, dtype=torch.int32, device="cuda:0")
        mom = torch.empty(px * 2, device="cuda:0")

        def call(t, rule=None):
            kw = dict(stream=s, sync=False, min_spp=mn, batch_spp=batch, max_spp=mx, threshold=t)
            if rule is not None:
                kw["rule"] = rule
            if nee is None:
                return lambda: dev.render_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), **kw)
            return lambda: dev.render_lit_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), nee=nee, **kw)

        def counts(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            c = spp.cpu().numpy()
            levels, pixels = np.unique(c, return_counts=True)
            return float(c.mean()), {int(k): int(v) for k, v in zip(levels, pixels)}
        own = call(t0)
        mean0, levels0 = counts(own)
        rec = {"width": cam.image_width, "height": cam.image_height, "call": "rt_render_adaptive" if nee is None else "rt_render_lit_adaptive",
               "rule_0": {"threshold": t0, "mean_spp": mean0, "levels": levels0, "ms": timed(own, args.reps)}}
        if has_rule:
            own_new = call(t0, 0)
            counts(own_new)
            rec["rule_0_through_the_rule_call"] = {"ms": timed(own_new, args.reps)}
            means = {t: counts(call(t, 1))[0] for t in near_ts}
            t1 = min(near_ts, key=lambda t: abs(means[t] - mean0))
            near = call(t1, 1)
            mean1, levels1 = counts(near)
            rec["rule_1"] = {"threshold": t1, "mean_spp": mean1, "levels": levels1, "ms": timed(near, args.reps), "judgements": (mx - mn) // batch,
                             "mean_spp_by_threshold": {str(t): m for t, m in means.items()}}
            rec["rule_1"]["ms_again"] = timed(near, args.reps)
        rec["rule_0"]["ms_again"] = timed(own, args.reps)          # (the run-to-run scatter of this visit)
        out["scenes"][sname] = rec
        dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
