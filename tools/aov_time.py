"""Developer tool (GPU): what the first-hit AOVs cost next to the beauty frame, on ONE handle (rt_render then rt_render_aov, the
same camera, alternating).  Warmed, then the median of --calls calls of each; every call does all of its work
(rt_config.reuse_view_lists = -1: the AOV call makes the candidate lists again, as a beauty frame of bench.py does).  Cases:
BASELINE configs[2] (1920x1080x500, S-rtiow), the same with the reference-order walk for every sample (primary_visibility = -1:
the exact-walk path), and the configs[4] geometry (S-100k + textured quad, 3840x2160) at 16 spp.
    python tools/aov_time.py [--calls 11] [--out profiles/r05/aov_time.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
import rtp_bindings as rb  # noqa: E402


def measure(name, host, cam, calls, **config):
    lib = rb.amd_lib()
    dev = rb.DeviceScene(host, device=0, honour_env=False, reuse_view_lists=-1, **config)
    pixels = cam.image_width * cam.image_height
    fb, ptrs = C.c_void_p(), {}
    rb._check(lib.rt_device_alloc(pixels * 12, C.byref(fb)), "rt_device_alloc")
    for key, _, _, per in rb.AOV_CHANNELS:
        d = C.c_void_p()
        rb._check(lib.rt_device_alloc(pixels * per * 4, C.byref(d)), "rt_device_alloc")
        ptrs[key] = d.value
    beauty, aov, last = [], [], None
    for k in range(calls + 2):              # two warm-up rounds
        tb = dev.render(cam, fb.value)
        ta = dev.render_aov(cam, ptrs)
        if k >= 2:
            beauty.append(tb.kernel_ms)
            aov.append(ta.kernel_ms)
        last = (tb, ta)
    tb, ta = last
    lib.rt_device_free(fb)
    for d in ptrs.values():
        lib.rt_device_free(C.c_void_p(d))
    dev.close()
    b, a = statistics.median(beauty), statistics.median(aov)
    row = {"case": name, "width": cam.image_width, "height": cam.image_height, "spp": cam.samples_per_pixel, "calls": calls,
           "beauty_kernel_ms_median": round(b, 3), "aov_kernel_ms_median": round(a, 3), "aov_over_beauty": round(a / b, 4),
           "beauty_kernel_ms": [round(x, 3) for x in beauty], "aov_kernel_ms": [round(x, 3) for x in aov],
           "beauty_primary_visibility": tb.primary_visibility, "beauty_guarded": tb.guarded,
           "aov_primary_visibility": ta.primary_visibility, "aov_primary_ms": round(ta.primary_ms, 3), "aov_rework_ms": round(ta.rework_ms, 3),
           "aov_walked_samples": ta.flagged_samples, "aov_traced_samples": ta.traced_samples}
    print(json.dumps({k: v for k, v in row.items() if not isinstance(v, list)}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rb.amd_lib().rt_set_device(0)
    rtiow = rb.HostScene.rtiow()
    rows = [measure("configs[2]", rtiow, rb.rtiow_camera(1920, 1080, 500, 50), args.calls),
            measure("configs[2], reference-order walk for every sample", rtiow, rb.rtiow_camera(1920, 1080, 500, 50), args.calls,
                    primary_visibility=-1),
            measure("configs[4] geometry at 16 spp", rb.HostScene.rtiow(half_extent=158, textured_quad=True, texture_size=2048),
                    rb.rtiow_camera(3840, 2160, 16, 50), args.calls)]
    result = {"version": rb.amd_lib().rt_version_string().decode(), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
