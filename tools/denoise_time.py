"""Developer tool (GPU): what rt_denoise costs.  The beauty frame and AOVs of the headline camera (S-rtiow, 1920x1080) and of a
3840x2160 frame of the same scene are rendered once at low spp (the filter's cost does not depend on the samples), then rt_denoise is
timed with device events around each call: warmed, the median of --calls calls, for 5 iterations and the other counts.  With
--rocprof the same calls run once each (no timing) for a `rocprofv3 --kernel-trace --stats` run of their own.
The bounds: bytes from shapes (the unique bytes each launch must move: its input records once and its output once) over the
measured HBM rate, and VALU instructions (the static counts of the step kernel's ISA, every tap taken, fp64 at half rate) over the
chip's VALU issue rate.
    python tools/denoise_time.py [--calls 11] [--out profiles/r07/denoise_time.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
import rtp_bindings as rb  # noqa: E402

HBM_BYTES_PER_S = 6.29e12           # MI355X float4 copy, measured (8.0e12 spec)
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9   # 256 CUs x 4 SIMD-32 x 2.4 GHz: one wave64 VALU instruction per 2 cycles per SIMD
# static VALU instructions of one interior pixel (every tap inside the image and a hit pixel), from the gfx950 ISA of
# csrc/rt_denoise.hip (hipcc --save-temps; the kernels are straight-line code apart from the normal squarings): denoise_step 1675
# of which 275 fp64 (11 per tap, exp_libm) — fp64 VALU issues at half the f32 rate, so 1675 + 275 issue slots; prepass 152;
# moments 254
VALU_STEP, VALU_PREPASS, VALU_MOMENTS = 1675 + 275, 152, 254


def bounds(pixels, iterations):
    """(bytes, VALU lane-instructions) of one call: the prepass reads 44 B and writes 48 B per pixel (12 B with 0 iterations);
    moments reads lv, nz, dg (48 B) and writes lv and dg (32 B); a step reads lv, nz, dg (48 B) and writes lv (16 B; the last one
    12 B of output, counted as 16)."""
    if iterations == 0:
        return pixels * (44 + 12), pixels * VALU_PREPASS
    b = pixels * (44 + 48) + pixels * (48 + 32) + iterations * pixels * (48 + 16)
    v = pixels * (VALU_PREPASS + VALU_MOMENTS + iterations * VALU_STEP)
    return b, v


def frame(host, cam):
    import torch
    dev = rb.DeviceScene(host, device=0)
    fb = torch.empty((cam.image_height, cam.image_width, 3), dtype=torch.float32, device="cuda:0")
    aov = {"albedo": torch.empty_like(fb), "normal": torch.empty_like(fb),
           "depth": torch.empty((cam.image_height, cam.image_width), dtype=torch.float32, device="cuda:0"),
           "hits": torch.empty((cam.image_height, cam.image_width), dtype=torch.int32, device="cuda:0")}
    dev.render(cam, fb.data_ptr())
    dev.render_aov(cam, {k: v.data_ptr() for k, v in aov.items()})
    dev.close()
    torch.cuda.synchronize()
    return fb, aov


def measure(name, fb, aov, spp, iterations, calls):
    import torch
    h, w = fb.shape[:2]
    out = torch.empty_like(fb)
    ptrs = {k: v.data_ptr() for k, v in aov.items()}
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for k in range(calls + 3):          # three warm-up calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rb.denoise(fb.data_ptr(), ptrs, w, h, spp, out.data_ptr(), stream=stream, iterations=iterations)
        e1.record()
        e1.synchronize()
        if k >= 3:
            times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    b, v = bounds(w * h, iterations)
    t_bytes, t_valu = b / HBM_BYTES_PER_S * 1e3, v / VALU_LANE_OPS_PER_S * 1e3
    row = {"case": name, "width": w, "height": h, "iterations": iterations, "calls": calls, "median_ms": round(ms, 4),
           "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "bytes": b, "bytes_bound_ms": round(t_bytes, 4),
           "valu_lane_instructions": v, "valu_bound_ms": round(t_valu, 4),
           "bound": "VALU" if t_valu >= t_bytes else "HBM", "share_of_bound": round(max(t_bytes, t_valu) / ms, 3),
           "times_ms": [round(t, 4) for t in times]}
    print(json.dumps({k: v for k, v in row.items() if k != "times_ms"}), flush=True)
    return row


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--rocprof", action="store_true", help="one untimed call per case (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rb.amd_lib().rt_set_device(0)
    torch.cuda.init()
    host = rb.HostScene.rtiow()
    rows = []
    for name, (w, h) in (("headline camera 1920x1080", (1920, 1080)), ("3840x2160", (3840, 2160))):
        fb, aov = frame(host, rb.rtiow_camera(w, h, args.spp, 50))
        for it in ((5, 0, 1, 3, 8) if w == 1920 else (5, 1, 8)):
            if args.rocprof:
                out = torch.empty_like(fb)
                rb.denoise(fb.data_ptr(), {k: v.data_ptr() for k, v in aov.items()}, w, h, args.spp, out.data_ptr(), iterations=it)
                torch.cuda.synchronize()
            else:
                rows.append(measure(name, fb, aov, args.spp, it, args.calls))
    if args.out and not args.rocprof:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"version": rb.amd_lib().rt_version_string().decode(), "spp": args.spp, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
