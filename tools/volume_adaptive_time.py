#!/usr/bin/env python3
"""rt_render_volume_adaptive against rt_render_volume at the same mean sample count: device-event times, warmed, median of
--reps with min – max.

Scene and fogs: tools/volume_time.py's — night rtiow at 1920 x 1080 (mis = 1, glossy = 1) under (a) the homogeneous box (no grid: the medium's
kernels) and (c) the 32^3 grid of the smooth density (the grid's kernels); min 16, batch 16, max 256, threshold 0.05.  Per fog: the whole
call, its mean spp and the histogram of stop levels; rt_render_volume at the rounded mean spp and at min_spp; the min_spp frame of the
adaptive call (max_spp = min_spp: the frame with its moments); each round's time as the difference of two calls whose caps lie one round
apart (the rule looks at max_spp only as the cap, so the call with cap min + r * batch runs exactly the first r rounds of the full call),
the samples the round traced (from the histogram) and its rate.
--unchanged: rt_render_volume, rt_render_medium and rt_render_lit_adaptive alone, on whatever library RTP_AMD_LIB names (the parent
commit's build, for the comparison of the kernels this change does not touch).  JSON on stdout, or into --out."""
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
    ap.add_argument("--spp", default="16:16:256")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rtp_bindings as rb
    import medium_time as mt
    import nee_time as nt
    from volume_time import smooth_density

    rb.amd_lib().rt_set_device(0)
    s = torch.cuda.current_stream().cuda_stream
    mn, batch, mx = (int(x) for x in args.spp.split(":"))
    rounds = (mx - mn) // batch
    host, cam16 = nt.scenes()["night_rtiow"]
    dev = rb.DeviceScene(host, device=0)
    px = cam16.image_width * cam16.image_height
    fb = torch.empty(px * 3, device="cuda:0")
    spp = torch.empty(px, dtype=torch.int32, device="cuda:0")
    mom = torch.empty(px * 2, device="cuda:0")
    nee = {"mis": 1, "glossy": 1}
    side, tau = 24.0, 2.0
    fog = dict(sigma_t=tau / side, albedo=0.9, g=0.5, box=(-side / 2,) * 3 + (side / 2,) * 3)
    vol32 = rb.Volume(smooth_density(32))
    out = {"library": os.environ.get("RTP_AMD_LIB", "this tree's"), "reps": args.reps, "width": cam16.image_width, "height": cam16.image_height,
           "min_spp": mn, "batch_spp": batch, "max_spp": mx, "threshold": args.threshold, "medium": fog}

    def cam_at(n):
        c = rb.CameraData.from_buffer_copy(cam16)
        c.samples_per_pixel = int(n)
        return c

    def uniform(volume, n):
        c = cam_at(n)
        return lambda: dev.render_volume(c, fb.data_ptr(), medium=fog, volume=volume, nee=nee, stream=s, sync=False)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        return mt.timed(fn, args.reps)

    if args.unchanged:
        c = cam_at(mn)
        lit_adaptive = lambda: dev.render_lit_adaptive(c, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), nee=nee, stream=s, sync=False, min_spp=mn,  # noqa: E731
                                                       batch_spp=batch, max_spp=4 * mn, threshold=args.threshold)
        medium = lambda: dev.render_medium(c, fb.data_ptr(), medium=fog, nee=nee, stream=s, sync=False)  # noqa: E731
        out["unchanged"] = {"rt_render_volume_32_at_min_spp": timed(uniform(vol32, mn)), "rt_render_medium_box_at_min_spp": timed(medium),
                            "rt_render_lit_adaptive_to_4x_min_spp": timed(lit_adaptive)}
    else:
        out["fogs"] = {}
        for name, volume in (("a_medium_box", None), ("c_volume_32", vol32)):
            def adaptive(cap, volume=volume):
                c = cam_at(mn)
                return lambda: dev.render_volume_adaptive(c, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), medium=fog, volume=volume, nee=nee, stream=s,
                                                          sync=False, min_spp=mn, batch_spp=batch, max_spp=cap, threshold=args.threshold)
            full = adaptive(mx)
            full()
            torch.cuda.synchronize()
            counts = spp.cpu().numpy()
            levels, pixels = np.unique(counts, return_counts=True)
            mean_spp = float(counts.mean())
            n_mean = max(1, int(round(mean_spp)))
            rec = {"mean_spp": mean_spp, "levels": {int(k): int(v) for k, v in zip(levels, pixels)}}
            # the calls whose times are compared with each other run next to each other
            rec["whole_call"] = timed(full)
            rec["rt_render_volume_at_mean_spp"] = dict(timed(uniform(volume, n_mean)), spp=n_mean)
            rec["whole_call_again"] = timed(full)
            rec["whole_call_over_uniform"] = rec["whole_call"]["ms"] / rec["rt_render_volume_at_mean_spp"]["ms"]
            rec["min_spp_frame"] = timed(adaptive(mn))
            rec["rt_render_volume_at_min_spp"] = timed(uniform(volume, mn))
            rec["min_spp_frame_over_uniform"] = rec["min_spp_frame"]["ms"] / rec["rt_render_volume_at_min_spp"]["ms"]
            rec["uniform_msamples_per_s"] = px * n_mean / rec["rt_render_volume_at_mean_spp"]["ms"] / 1e3
            prev = rec["min_spp_frame"]["ms"]
            rec["rounds"] = []
            for r in range(1, rounds + 1):
                ms = timed(adaptive(mn + r * batch))["ms"]
                going = int((counts >= mn + r * batch).sum())
                d = ms - prev
                rec["rounds"].append({"round": r, "pixels": going, "samples": going * batch, "ms": d,
                                      "msamples_per_s": going * batch / d / 1e3 if d > 0 and going else None})
                prev = ms
            out["fogs"][name] = rec
    vol32.close()
    dev.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
