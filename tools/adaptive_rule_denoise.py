#!/usr/bin/env python3
"""DESIGN.md §20's quality table with frames of either stopping rule (§22): rtiow 320 x 180, min 4, batch 4, max 32, AOVs at 4 spp; the
MSE of the per-pixel mean clamped to [0, 1] against 1024 spp from sample 2^20 of the noisy adaptive frame, rt_denoise_spp with and
without moments, the uniform frame at the rounded mean spp and rt_denoise of it.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
import rtp_bindings as rb          # noqa: E402


def mse(fb, spp, truth):
    return float(np.mean((np.clip(fb.astype(np.float64) / np.asarray(spp, np.float64)[..., None], 0, 1) - truth) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", default="4:4:32")
    ap.add_argument("--settings", default="0:0.1,1:0.08", help="comma-separated rule:threshold pairs")
    args = ap.parse_args()
    mn, batch, mx = (int(x) for x in args.spp.split(":"))
    rb.amd_lib().rt_set_device(0)
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    cam = rb.rtiow_camera(320, 180, 1, 50)
    truth = np.clip(dev.render_to_host(rb.rtiow_camera(320, 180, 1024, 50), sample_first=1 << 20)[0].astype(np.float64) / 1024, 0, 1)
    aov, _ = dev.render_aov_to_host(rb.rtiow_camera(320, 180, mn, 50))
    rows = []
    for pair in args.settings.split(","):
        rule, t = int(pair.split(":")[0]), float(pair.split(":")[1])
        fb, spp, mom, _ = dev.render_adaptive_to_host(cam, min_spp=mn, batch_spp=batch, max_spp=mx, threshold=t, rule=rule)
        n = max(1, int(round(float(spp.mean()))))
        ucam = rb.rtiow_camera(320, 180, n, 50)
        ufb, _ = dev.render_to_host(ucam)
        uaov, _ = dev.render_aov_to_host(ucam)
        uniform = np.full(spp.shape, n, np.int32)
        levels, pixels = np.unique(spp, return_counts=True)
        rows.append({"rule": rule, "threshold": t, "mean_spp": float(spp.mean()), "levels": {int(k): int(v) for k, v in zip(levels, pixels)},
                     "noisy": mse(fb, spp, truth), "denoise_spp_with_moments": mse(rb.denoise_spp_to_host(fb, spp, mom, aov, mn), spp, truth),
                     "denoise_spp_without_moments": mse(rb.denoise_spp_to_host(fb, spp, None, aov, mn), spp, truth), "uniform_spp": n,
                     "uniform_noisy": mse(ufb, uniform, truth), "uniform_denoised": mse(rb.denoise_to_host(ufb, uaov, n), uniform, truth)})
    dev.close()
    print(json.dumps({"width": 320, "height": 180, "min_spp": mn, "batch_spp": batch, "max_spp": mx, "rows": rows}))


if __name__ == "__main__":
    main()
