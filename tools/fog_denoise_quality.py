#!/usr/bin/env python3
"""What the fog-aware AOVs are worth to rt_denoise: night rtiow under the fogs of tools/volume_time.py — (a) the homogeneous box, (c) the
32^3 grid, (d) the 128^3 grid — at 4, 8 and 16 spp against a --truth-spp rt_render_volume reference.

Error = MSE of the sqrt-tonemapped frame (sqrt(max(sum / spp, 0)), unclamped above) against the reference, over the whole frame and over the
pixels the first-hit AOVs call sky (hit_count == 0 at that spp).  Per fog and spp: the noisy frame, rt_denoise under rt_render_aov_lens's
AOVs, rt_denoise under rt_render_aov_volume's.  Per fog one adaptive row: rt_render_volume_adaptive (threshold --threshold, 4:4:64) filtered
by rt_denoise_spp under each set of AOVs at min_spp.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--fogs", default="box,volume_32,volume_128")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import nee_time as nt
    import volume_time as vt

    rb.amd_lib().rt_set_device(0)
    host = nt.scenes()["night_rtiow"][0]
    cam = rb.make_camera(args.width, args.height, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), 16, 50)          # (tools/nee_time.py's view)
    dev = rb.DeviceScene(host, device=0)
    nee = {"mis": 1, "glossy": 1}
    side, tau = 24.0, 2.0
    fog = dict(sigma_t=tau / side, albedo=0.9, g=0.5, box=(-side / 2,) * 3 + (side / 2,) * 3)
    grids = {"box": None, "volume_32": vt.smooth_density(32), "volume_128": vt.smooth_density(128)}
    adapt = dict(min_spp=4, batch_spp=4, max_spp=64)

    def with_spp(spp):
        c = rb.CameraData.from_buffer_copy(cam)
        c.samples_per_pixel = spp
        return c

    def tonemapped(fb_sum, spp):
        """spp: a number, or the per-pixel counts of an adaptive frame."""
        mean = fb_sum.astype(np.float64) / (np.asarray(spp, np.float64)[..., None] if np.ndim(spp) else spp)
        return np.sqrt(np.clip(mean, 0.0, None))

    out = {"width": cam.image_width, "height": cam.image_height, "truth_spp": args.truth_spp, "medium": fog, "adaptive": dict(adapt, threshold=args.threshold), "fogs": {}}
    for name in args.fogs.split(","):
        vol = rb.Volume(grids[name]) if grids[name] is not None else None
        kw = dict(medium=fog, volume=vol)
        truth = tonemapped(dev.render_volume_to_host(with_spp(args.truth_spp), nee=nee, **kw)[0], args.truth_spp)
        rows = {}

        def errors(frames, sky):
            e = {}
            for k, f in frames.items():
                d = (f - truth) ** 2
                e[k] = {"all": float(d.mean()), "sky": float(d[sky].mean()) if sky.any() else None}
            for k in list(e):
                if k != "noisy":
                    e[k]["all_over_noisy"] = e[k]["all"] / e["noisy"]["all"]
                    e[k]["sky_over_noisy"] = e[k]["sky"] / e["noisy"]["sky"] if sky.any() and e["noisy"]["sky"] else None
            e["sky_share"] = float(sky.mean())
            return e
        for spp in (4, 8, 16):
            c = with_spp(spp)
            fb, _ = dev.render_volume_to_host(c, nee=nee, **kw)
            first, _ = dev.render_aov_lens_to_host(c)
            aware, _ = dev.render_aov_volume_to_host(c, **kw)
            rows[str(spp)] = errors({"noisy": tonemapped(fb, spp), "first_hit": tonemapped(rb.denoise_to_host(fb, first, spp), spp),
                                     "fog_aware": tonemapped(rb.denoise_to_host(fb, aware, spp), spp)}, first["hits"] == 0)
        c = with_spp(adapt["min_spp"])
        fb, spp, mom, _ = dev.render_volume_adaptive_to_host(c, nee=nee, threshold=args.threshold, **adapt, **kw)
        first, _ = dev.render_aov_lens_to_host(c)
        aware, _ = dev.render_aov_volume_to_host(c, **kw)
        rows["adaptive"] = errors({"noisy": tonemapped(fb, spp), "first_hit": tonemapped(rb.denoise_spp_to_host(fb, spp, mom, first, adapt["min_spp"]), spp),
                                   "fog_aware": tonemapped(rb.denoise_spp_to_host(fb, spp, mom, aware, adapt["min_spp"]), spp)}, first["hits"] == 0)
        rows["adaptive"]["mean_spp"] = float(spp.mean())
        out["fogs"][name] = rows
        if vol is not None:
            vol.close()
        torch.cuda.empty_cache()
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
