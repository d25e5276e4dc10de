#!/usr/bin/env python3
"""rt_render_lit_split against rt_render_lit on the same handle: device-event times (warmed, median of --reps) and each call's passes.

Scene: night rtiow (tools/nee_time.py's: every eighth small sphere an emitter) under the sun-and-sky map of tests/env_reference.py
(n = 256, mode 1, scale 0.75) at 1920 x 1080 x --spp (default 16), pinhole, and once more with tools/lit_time.py's lens and open shutter.
The split keeps two slabs, so a workspace budget admits half the samples per pass: the pass count of each call stands beside its time,
and a second row per camera gives both calls the same forced pass length (rt_config.pass_spp = --spp / 2), so that what is left is the
kernel's and the second accumulate's.  spread: a second median of rt_render_lit over the first.  JSON on stdout."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtp_bindings as rb  # noqa: E402
import env_reference as er  # noqa: E402  (the map's formula only: nothing is built)
from nee_time import night_rtiow, timed  # noqa: E402

LENS = dict(lens_radius=0.2, focus_distance=12.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--spp", type=int, default=16)
    args = ap.parse_args()
    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    host = night_rtiow()
    cam = rb.make_camera(1920, 1080, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), args.spp, 50)
    close = rb.make_camera(1920, 1080, 20.0, (12.9, 3.05, 2.1), (0, 0, 0), (0, 0, 0), args.spp, 50)
    px = cam.image_width * cam.image_height
    fb = torch.empty((3, px * 3), device="cuda:0")
    out = {"version": rb.amd_lib().rt_version_string().decode(), "reps": args.reps, "width": cam.image_width, "height": cam.image_height,
           "spp": args.spp, "rows": {}}
    with rb.Env(er.sun_and_sky(256)) as env:
        for cname, ckw in (("pinhole", dict()), ("lens_motion", dict(cam_close=close, lens=LENS))):
            for pname, config in (("default_passes", dict()), ("equal_passes", dict(pass_spp=max(args.spp // 2, 1)))):
                dev = rb.DeviceScene(host, device=0, **config)
                kw = dict(env=env, env_params=dict(mode=1, scale=0.75), **ckw)
                calls = {"rt_render_lit": lambda sync=False: dev.render_lit(cam, fb[0].data_ptr(), stream=s, sync=sync, **kw),
                         "rt_render_lit_split": lambda sync=False: dev.render_lit_split(cam, fb[1].data_ptr(), fb[2].data_ptr(), stream=s, sync=sync, **kw)}
                for _ in range(2):
                    for fn in calls.values():
                        fn()
                torch.cuda.synchronize()
                row = {}
                for name, fn in calls.items():
                    t = fn(sync=True)
                    row[name] = {"ms": timed(fn, args.reps), "passes": int(t.trace_launches), "vgprs": int(t.trace_vgprs), "scratch_bytes": int(t.trace_scratch_bytes)}
                row["split_over_lit"] = row["rt_render_lit_split"]["ms"] / row["rt_render_lit"]["ms"]
                row["spread"] = timed(calls["rt_render_lit"], args.reps) / row["rt_render_lit"]["ms"]
                out["rows"][f"{cname}/{pname}"] = row
                dev.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
