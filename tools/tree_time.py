#!/usr/bin/env python3
"""rt_render_nee with select = 1 (the light tree) against select = 0 (the power table) and rt_render: device-event times (warmed,
median of --reps) and quality at equal GPU time.

Scenes: night rtiow (tests/test_light_tree.py's: every eighth small sphere of rtiow a lamp, 60 of them over a 22 x 22 field) and panel
box with sample_planes = 1 (a sphere and five plane lights), both at 1920 x 1080 x 16 with a black background.  Calls: rt_render at its
default setting, rt_render_nee (mis = 1) with select = 0 and 1.  Per call: ms per frame, Msamples/s, closest-hit queries per sample
(rt_trace_samples / rt_trace_samples_nee on 20 000 random samples; the NEE calls' surplus over rt_render's is their shadow rays).
Quality at equal time, at a quarter of the resolution in each direction: the per-sample time of each call there, the spp each affords
in the time rt_render takes for --budget-spp, and the luminance MSE of that frame against a ground truth (select = 1 at --truth-spp
from a disjoint sample range).
--package DIR loads rtp_bindings and the libraries of another build of this project (the parent commit's, as the yardstick of
select = 0); a build without select times what it has.  JSON on stdout."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUM = np.array([0.2126, 0.7152, 0.0722])
QUAD, ELLIPSE, TRIANGLE = 0, 1, 2


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


def material(rb, kind, albedo=(0.5, 0.5, 0.5), emit=(0, 0, 0), fuzz=0.0, ir=1.5):
    m = rb.Material()
    m.type, m.fuzz, m.ir = kind, fuzz, ir
    for k in range(3):
        m.albedo.e[k] = albedo[k]
        m.emit.e[k] = emit[k]
    return m


def panel_box(rb):
    planes = np.array([
        [-6, 0, 6, 12, 0, 0, 0, 0, -12, 0, QUAD], [-6, 0, -4, 12, 0, 0, 0, 4.3, 0, 1, QUAD], [-2, 5, 1.5, 4, 0, 0, 0, 0, -3, 5, QUAD],
        [1.5, 1.2, -3.9, 3, 0, 0, 0, 2.6, 0, 6, ELLIPSE], [-4.5, 0, 0.5, 1.6, 0, 1.6, 0, 2.8, 0, 7, TRIANGLE],
        [3, 4.5, -1, 2, 0, 0, 0, 0, -2, 9, QUAD], [2.5, 4.4, -0.5, 3, 0, 0, 0, 0, -3, 10, QUAD],
        [-1.2, 0.01, 5, 2.4, 0, 0, 0, 0, -1.6, 11, QUAD]], np.float32)
    spheres = np.array([[-1.6, 1, 0, 1, 2], [1.6, 1, -0.5, 1, 3], [0, 0.6, 2.2, 0.6, 4], [3.6, 0.5, 2, 0.5, 8]], np.float32)
    mats = [material(rb, 0, (0.6, 0.6, 0.6)), material(rb, 0, (0.7, 0.5, 0.4)), material(rb, 0, (0.3, 0.5, 0.8)),
            material(rb, 1, (0.8, 0.7, 0.5), fuzz=0.4), material(rb, 2, ir=1.5), material(rb, 3, emit=(6, 5, 4)), material(rb, 3, emit=(2, 3, 4)),
            material(rb, 3, emit=(4, 2, 3)), material(rb, 3, emit=(5, 5, 3)), material(rb, 3, emit=(3, 3, 3)), material(rb, 0, (0.5, 0.5, 0.5)),
            material(rb, 0, (0.5, 0.4, 0.3), emit=(0.8, 1.0, 0.6))]
    return rb.HostScene.from_arrays(spheres, planes, mats)


def night_rtiow(rb):
    base = rb.HostScene.rtiow()          # (kept alive: desc points into it)
    d = base.desc
    spheres, mats = [], []
    for i in range(d.num_spheres):
        sp = d.spheres[i]
        m = d.materials[sp.material_idx]
        if 0 < i < d.num_spheres - 3 and i % 8 == 5:
            m = material(rb, 3, emit=(6.0, 4.5, 3.0) if i % 16 == 5 else (1.5, 2.0, 3.0))
        spheres.append([sp.center.e[0], sp.center.e[1], sp.center.e[2], sp.radius, len(mats)])
        mats.append(rb.Material.from_buffer_copy(m))
    host = rb.HostScene.from_arrays(np.array(spheres, np.float32), np.zeros((0, 11), np.float32), mats)
    base.close()
    return host


def with_size(rb, cam, w, h, spp):
    """The same view at w x h: the pose kept, the pixel deltas scaled, pixel 0's centre moved to the new grid."""
    c = rb.CameraData.from_buffer_copy(cam)
    sx, sy = cam.image_width / w, cam.image_height / h
    for k in range(3):
        c.pixel_delta_u.e[k] = cam.pixel_delta_u.e[k] * sx
        c.pixel_delta_v.e[k] = cam.pixel_delta_v.e[k] * sy
        c.pixel00_loc.e[k] = cam.pixel00_loc.e[k] - 0.5 * cam.pixel_delta_u.e[k] - 0.5 * cam.pixel_delta_v.e[k] + \
            0.5 * c.pixel_delta_u.e[k] + 0.5 * c.pixel_delta_v.e[k]
    c.image_width, c.image_height, c.samples_per_pixel = w, h, spp
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget-spp", type=int, default=64)
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--package", default=os.path.join(ROOT, "ray-tracing-practice_amd"))
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import rtp_bindings as rb
    rb.amd_lib().rt_set_device(0)
    has_select = "select" in rb.NeeParams.FIELDS
    s = torch.cuda.current_stream().cuda_stream
    scenes = {"night_rtiow": (night_rtiow(rb), rb.make_camera(1920, 1080, 20.0, (13, 3, 2), (0, 0, 0), (0, 0, 0), 16, 50), 0),
              "panel_box_planes": (panel_box(rb), rb.make_camera(1920, 1080, 50.0, (0, 3, 10), (0, 1.8, 0), (0, 0, 0), 16, 50), 1)}
    out = {"package": os.path.relpath(args.package, ROOT), "reps": args.reps, "select": has_select, "scenes": {}}
    for sname, (host, cam, planes) in scenes.items():
        settings = {"select0": {"mis": 1, "sample_planes": planes}}
        if has_select:
            settings["select0"] = {"mis": 1, "sample_planes": planes, "select": 0}
            settings["select1"] = {"mis": 1, "sample_planes": planes, "select": 1}
        dev = rb.DeviceScene(host, device=0)
        px = cam.image_width * cam.image_height
        fb = torch.empty(px * 3, device="cuda:0")

        def calls_into(buf):
            c = {"rt_render": lambda cm, first=0: dev.render(cm, buf.data_ptr(), stream=s, sync=False, sample_first=first)}
            for name, p in settings.items():
                c[name] = lambda cm, first=0, p=p: dev.render_nee(cm, buf.data_ptr(), params=p, stream=s, sync=False, sample_first=first)
            return c
        calls = calls_into(fb)
        rec = {"spheres": host.desc.num_spheres, "planes": host.desc.num_planes, "width": cam.image_width, "height": cam.image_height,
               "spp": cam.samples_per_pixel, "calls": {}}
        for _ in range(2):
            for fn in calls.values():
                fn(cam)
        torch.cuda.synchronize()
        rng = np.random.default_rng(1)
        n = 20000
        ijs = np.stack([rng.integers(0, cam.image_width, n), rng.integers(0, cam.image_height, n), rng.integers(0, 1 << 20, n)], 1)
        plain_rays = float(dev.trace_samples(cam, ijs)[1].mean())
        for name, fn in calls.items():
            ms = timed(lambda: fn(cam), args.reps)
            r = {"ms": ms, "msamples_per_s": px * cam.samples_per_pixel / ms / 1e3, "queries_per_sample": plain_rays}
            if name in settings:
                q = float(dev.trace_samples_nee(cam, ijs, params=settings[name])[1].mean())
                r.update(queries_per_sample=q, shadow_rays_per_sample=q - plain_rays)
            rec["calls"][name] = r
        if has_select:
            rec["emitters"] = int(len(dev.nee_light_tree(settings["select1"])["path"]))
            # ---- quality at equal GPU time, a quarter of the resolution per axis
            w, h = cam.image_width // 4, cam.image_height // 4
            fbs = torch.empty(w * h * 3, device="cuda:0")
            sm = calls_into(fbs)
            truth_cam = with_size(rb, cam, w, h, args.truth_spp)
            dev.render_nee(truth_cam, fbs.data_ptr(), params=settings["select1"], stream=s, sync=True, sample_first=1 << 28)
            torch.cuda.synchronize()
            truth = fbs.cpu().numpy().reshape(h, w, 3).astype(np.float64) / args.truth_spp @ LUM
            per_spp = {}
            probe = with_size(rb, cam, w, h, args.budget_spp)
            for name, fn in sm.items():
                fn(probe, 0)
                per_spp[name] = timed(lambda: fn(probe, 0), args.reps) / args.budget_spp
            budget = per_spp["rt_render"] * args.budget_spp
            q = {"width": w, "height": h, "truth_spp": args.truth_spp, "budget_ms": budget, "estimators": {}}
            for name, fn in sm.items():
                spp = max(1, int(budget / per_spp[name]))
                fn(with_size(rb, cam, w, h, spp), 0)
                torch.cuda.synchronize()
                img = fbs.cpu().numpy().reshape(h, w, 3).astype(np.float64) / spp @ LUM
                q["estimators"][name] = {"ms_per_spp": per_spp[name], "spp": spp, "mse": float(((img - truth) ** 2).mean())}
            base = q["estimators"]["rt_render"]["mse"]
            for e in q["estimators"].values():
                e["mse_vs_rt_render"] = e["mse"] / base
            rec["equal_time_quality"] = q
        out["scenes"][sname] = rec
        dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
