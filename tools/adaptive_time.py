#!/usr/bin/env python3
"""rt_render_adaptive on S-rtiow at 1920x1080 (min 16, batch 16, max 256): device-event times, warmed, median of --reps.

Per round k the call is timed with max_spp = min + k * batch: the difference T(k) - T(k - 1) is what round k costs (the rounds are the
same work either way, the counts decide everything).  Next to it: guarded rt_render at min_spp and at the mean count, the call with
max = min (the min_spp frame + moments + one select), and the call with a huge threshold (every round empty).  JSON on stdout."""
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
    ap.add_argument("--min", type=int, default=16)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rb.amd_lib().rt_set_device(0)
    host = rb.HostScene.rtiow()
    cam = rb.rtiow_camera(args.width, args.height, args.min, 50)
    dev = rb.DeviceScene(host, device=0)
    px = args.width * args.height
    fb = torch.empty(px * 3, device="cuda:0")
    spp = torch.empty(px, dtype=torch.int32, device="cuda:0")
    mom = torch.empty(px * 2, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream

    def adaptive(max_spp, threshold=args.threshold):
        return lambda: dev.render_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), stream=s, sync=False, min_spp=args.min,
                                           batch_spp=args.batch, max_spp=max_spp, threshold=threshold)

    def uniform(n):
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = n
        return lambda: dev.render(c, fb.data_ptr(), stream=s, sync=False)

    for _ in range(2):      # warm: buffers, view lists, the handle's walk decision
        adaptive(args.max)()
        uniform(args.min)()
    torch.cuda.synchronize()
    out = {"scene": "S-rtiow", "width": args.width, "height": args.height, "min_spp": args.min, "batch_spp": args.batch, "max_spp": args.max,
           "threshold": args.threshold, "reps": args.reps}
    out["uniform_min_ms"] = timed(uniform(args.min), args.reps)
    out["uniform_min_msamples_per_s"] = px * args.min / out["uniform_min_ms"] / 1e3
    out["guarded"] = int(dev.last_timing().guarded)
    rounds = (args.max - args.min) // args.batch
    totals, per_round = [], []
    for k in range(rounds + 1):
        totals.append(timed(adaptive(args.min + k * args.batch), args.reps))
        counts = spp.cpu().numpy()
        if k > 0:
            active = int((counts >= args.min + k * args.batch).sum())
            ms = totals[k] - totals[k - 1]
            per_round.append({"round": k, "pixels": active, "ms": ms, "msamples_per_s": active * args.batch / ms / 1e3 if ms > 0 and active else None})
    out["min_round_with_moments_ms"] = totals[0]
    out["moments_and_select_ms"] = totals[0] - out["uniform_min_ms"]
    out["total_ms"] = totals[-1]
    out["rounds"] = per_round
    counts = spp.cpu().numpy()
    out["mean_spp"] = float(counts.mean())
    out["levels"] = {int(n): int((counts == n).sum()) for n in np.unique(counts)}
    mean_n = int(round(out["mean_spp"]))
    out["uniform_mean_ms"] = timed(uniform(mean_n), args.reps)
    out["uniform_mean_spp"] = mean_n
    empty = timed(adaptive(args.max, 1e30), args.reps)
    out["empty_rounds_ms_each"] = (empty - totals[0]) / rounds if rounds else 0.0
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
