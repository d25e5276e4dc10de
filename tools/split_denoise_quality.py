#!/usr/bin/env python3
"""Is filtering direct and indirect light separately worth it?  rt_denoise of the beauty frame against rt_denoise_split of the two
components, at --spp (default 8) against a --truth-spp (default 1024) mean from a disjoint sample range.

Scenes: a closed box of five LAMBERTIAN quads (floor, back and side walls, ceiling) with an emissive quad in the ceiling and two
spheres, seen through the open front — indirect light matters there — and night rtiow (tools/nee_time.py's) under the sun-and-sky map
of tests/env_reference.py.  Error: MSE of the mean clamped to [0, 1], as tests/test_denoise.py's quality test has it, for the noisy frame
(direct + indirect, one float32 add), rt_denoise of that frame and rt_denoise_split; also the share of the mean luminance that is
indirect.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtp_bindings as rb  # noqa: E402
import env_reference as er  # noqa: E402  (the map's formula only: nothing is built)
from nee_time import night_rtiow  # noqa: E402

QUAD = 0
LUM = np.array([0.2126, 0.7152, 0.0722])


def material(kind, albedo=(0.5, 0.5, 0.5), emit=(0, 0, 0), fuzz=0.0, ir=1.5):
    m = rb.Material()
    m.type, m.fuzz, m.ir = kind, fuzz, ir
    for k in range(3):
        m.albedo.e[k] = albedo[k]
        m.emit.e[k] = emit[k]
    return m


def light_box():
    """The box [-2, 2] x [-2, 2] x [0, 4], open towards +y; planes are (base, u, v, material, type).  z is up, like the cameras of
    rb.make_camera: a view along their up vector has no finite image plane, and the kernels' walks are not made for rays that are not
    finite."""
    mats = [material(0, (0.73, 0.73, 0.73)), material(0, (0.65, 0.05, 0.05)), material(0, (0.12, 0.45, 0.15)), material(3, emit=(15, 15, 15)),
            material(0, (0.5, 0.5, 0.8)), material(1, (0.8, 0.8, 0.8), fuzz=0.1)]
    planes = np.array([[-2, 2, 0, 4, 0, 0, 0, -4, 0, 0, QUAD],          # floor
                       [-2, -2, 4, 4, 0, 0, 0, 4, 0, 0, QUAD],          # ceiling
                       [-2, -2, 0, 4, 0, 0, 0, 0, 4, 0, QUAD],          # back wall
                       [-2, 2, 0, 0, -4, 0, 0, 0, 4, 1, QUAD],          # left wall
                       [2, -2, 0, 0, 4, 0, 0, 0, 4, 2, QUAD],           # right wall
                       [-0.6, -0.6, 3.99, 1.2, 0, 0, 0, 1.2, 0, 3, QUAD]], np.float32)          # the lamp, just under the ceiling
    spheres = np.array([[-0.8, -0.5, 0.7, 0.7, 4], [0.9, 0.6, 0.5, 0.5, 5]], np.float32)
    return rb.HostScene.from_arrays(spheres, planes, mats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--truth-spp", type=int, default=1024)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    args = ap.parse_args()
    rb.amd_lib().rt_set_device(0)
    w, h = args.width, args.height
    out = {"version": rb.amd_lib().rt_version_string().decode(), "width": w, "height": h, "spp": args.spp, "truth_spp": args.truth_spp, "scenes": {}}
    with rb.Env(er.sun_and_sky(256)) as env:
        scenes = {"light_box": (light_box(), rb.make_camera(w, h, 40.0, (0, 9, 2), (0, 0, 2), (0, 0, 0), args.spp, 50), dict(nee=dict(sample_planes=1))),
                  "night_rtiow_sky": (night_rtiow(), rb.make_camera(w, h, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), args.spp, 50),
                                      dict(env=env, env_params=dict(mode=1, scale=0.75)))}
        for name, (host, cam, kw) in scenes.items():
            assert all(np.isfinite(list(v.e)).all() for v in (cam.origin, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v)), name
            dev = rb.DeviceScene(host, device=0)
            big = rb.CameraData.from_buffer_copy(cam)
            big.samples_per_pixel = args.truth_spp
            td, ti, _ = dev.render_lit_split_to_host(big, sample_first=1 << 20, **kw)
            truth = np.clip((td + ti) / np.float32(args.truth_spp), 0, 1)
            direct, indirect, _ = dev.render_lit_split_to_host(cam, **kw)
            aov, _ = dev.render_aov_to_host(cam)
            beauty = direct + indirect

            def mse(fb):
                return float(np.mean((np.clip(fb / np.float32(args.spp), 0, 1) - truth) ** 2))
            row = {"noisy": mse(beauty), "rt_denoise": mse(rb.denoise_to_host(beauty, aov, args.spp)),
                   "rt_denoise_split": mse(rb.denoise_split_to_host(direct, indirect, aov, args.spp)),
                   "indirect_share_of_luminance": float((ti.astype(np.float64) @ LUM).sum() / ((td.astype(np.float64) + ti) @ LUM).sum())}
            row["split_over_beauty"] = row["rt_denoise_split"] / row["rt_denoise"]
            out["scenes"][name] = row
            dev.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
