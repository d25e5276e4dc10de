#!/usr/bin/env python3
"""rt_render_aov_volume next to rt_render_aov_lens and to the frame it serves, on night rtiow at 1920 x 1080 x 16 spp under the fogs of
tools/volume_time.py: (a) the homogeneous box, (c) the 32^3 grid, (d) the 128^3 grid.  Device-event times, warmed, median of --reps with
the spread of the runs.

Per fog: the AOV call with every buffer and the transmittance, rt_render_volume's frame with the same medium and grid, and their ratio —
what the guides cost relative to the frame they are for.  Once: rt_render_aov_lens for the same camera (the fog call's resolve step is its
resolve step; the difference is the accumulation under fog), and rt_render_aov.  JSON on stdout.  RTP_AMD_LIB selects another build of
the library; --parent times only the calls a build without rt_render_aov_volume has."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", action="store_true", help="rt_render_aov, rt_render_aov_lens and rt_render_volume (c) alone")
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
    bufs = {"albedo": torch.empty(px * 3, device="cuda:0"), "normal": torch.empty(px * 3, device="cuda:0"), "depth": torch.empty(px, device="cuda:0"),
            "hits": torch.empty(px, dtype=torch.int32, device="cuda:0"), "prim": torch.empty(px, dtype=torch.int32, device="cuda:0")}
    tr = torch.empty(px, device="cuda:0")
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    nee = {"mis": 1, "glossy": 1}
    side, tau = 24.0, 2.0
    fog = dict(sigma_t=tau / side, albedo=0.9, g=0.5, box=(-side / 2,) * 3 + (side / 2,) * 3)
    volumes = {"box": None, "volume_32": rb.Volume(vt.smooth_density(32)), "volume_128": rb.Volume(vt.smooth_density(128))}
    calls = {"aov": lambda: dev.render_aov(cam, ptrs, stream=s, sync=False), "aov_lens": lambda: dev.render_aov_lens(cam, ptrs, stream=s, sync=False)}
    for name, vol in volumes.items():
        if args.parent and name != "volume_32":
            continue
        calls["frame_" + name] = lambda vol=vol: dev.render_volume(cam, fb.data_ptr(), medium=fog, volume=vol, nee=nee, stream=s, sync=False)
        if not args.parent:
            calls["aov_" + name] = lambda vol=vol: dev.render_aov_volume(cam, ptrs, medium=fog, volume=vol, transmittance=tr.data_ptr(), stream=s, sync=False)
    out = {"reps": args.reps, "width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "medium": fog, "calls": {}}
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    for name, fn in calls.items():
        r = mt.timed(fn, args.reps)
        r["scatter"] = (r["max_ms"] - r["min_ms"]) / r["ms"]
        out["calls"][name] = r
    c = out["calls"]
    for name in volumes:
        if "aov_" + name in c:
            c["aov_" + name].update(over_aov_lens=c["aov_" + name]["ms"] / c["aov_lens"]["ms"], over_its_frame=c["aov_" + name]["ms"] / c["frame_" + name]["ms"])
    if not args.parent:
        out["mean_transmittance"] = float(tr.mean().item()) / cam.samples_per_pixel          # (of the last call: the 128^3 grid)
    for vol in volumes.values():
        if vol is not None:
            vol.close()
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
