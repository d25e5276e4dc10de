#!/usr/bin/env python3
"""rt_render_volume against rt_render_medium on night rtiow at 1920 x 1080 x 16 spp (tools/medium_time.py's scene and setting: mis = 1,
glossy = 1): device-event times, warmed, median of --reps with the spread of the runs.

Calls: (a) rt_render_medium with the bounding box of tools/medium_time.py's fog ball (side 24 around the origin) at optical depth 2 across
it, albedo 0.9, g = 0.5; (b) rt_render_volume with a 1 x 1 x 1 grid of density 1 in that box — the same fog, bit for bit, through the grid
kernels: their cost alone; (c) a 32^3 and (d) a 128^3 grid of one smooth density (a sum of three sines, normalised to mean 1: the same mean
extinction).  Per call the medium events, and for the grid calls the cells visited, per sample from the probe on 20 000 random samples.
JSON on stdout.  RTP_AMD_LIB selects another build of the library, e.g. the parent commit's for call (a)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def smooth_density(n):
    """(n, n, n) float32, mean 1, between about 0.1 and 1.9: cell centres of a fixed smooth function of the box's unit coordinates."""
    c = (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    f = 1.0 + 0.3 * (np.sin(2 * np.pi * x) + np.sin(4 * np.pi * y + 1.0) + np.sin(2 * np.pi * (z + x)))
    return (f / f.mean()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--medium-only", action="store_true", help="call (a) alone: for a build that has no rt_render_volume")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import medium_time as mt
    import nee_time as nt

    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    host, cam = nt.scenes()["night_rtiow"]
    dev = rb.DeviceScene(host, device=0)
    px = cam.image_width * cam.image_height
    fb = torch.empty(px * 3, device="cuda:0")
    nee = {"mis": 1, "glossy": 1}
    side, tau = 24.0, 2.0
    fog = dict(sigma_t=tau / side, albedo=0.9, g=0.5, box=(-side / 2,) * 3 + (side / 2,) * 3)
    calls = {"medium_box": lambda: dev.render_medium(cam, fb.data_ptr(), medium=fog, nee=nee, stream=s, sync=False)}
    volumes = {}
    if not args.medium_only:
        volumes = {"volume_1": rb.Volume(np.ones((1, 1, 1), np.float32)), "volume_32": rb.Volume(smooth_density(32)), "volume_128": rb.Volume(smooth_density(128))}
        for name, vol in volumes.items():
            calls[name] = lambda vol=vol: dev.render_volume(cam, fb.data_ptr(), medium=fog, volume=vol, nee=nee, stream=s, sync=False)
    out = {"reps": args.reps, "width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "medium": fog, "calls": {}}
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    n = 20000
    ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1)
    for name, fn in calls.items():
        r = mt.timed(fn, args.reps)
        r["msamples_per_s"] = px * cam.samples_per_pixel / r["ms"] / 1e3
        r["scatter"] = (r["max_ms"] - r["min_ms"]) / r["ms"]
        if name in volumes:
            probe = dev.trace_samples_volume(cam, ijs, medium=fog, volume=volumes[name], nee=nee)
            r.update(cells_per_sample=float(probe[7].mean()), most_cells=int(probe[7].max()))
        else:
            probe = dev.trace_samples_medium(cam, ijs, medium=fog, nee=nee)
        r.update(queries_per_sample=float(probe[1].mean()), medium_events_per_sample=float(probe[2].mean()))
        out["calls"][name] = r
    for name in volumes:
        out["calls"][name]["over_medium_box"] = out["calls"][name]["ms"] / out["calls"]["medium_box"]["ms"]
    for vol in volumes.values():
        vol.close()
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
