"""Developer tool (GPU): what rt_denoise_temporal costs.  The beauty frame and AOVs of the headline camera (S-rtiow, 1920x1080) and
of a 3840x2160 frame of the same scene are rendered once at low spp, one call fills a history, then rt_denoise_temporal is timed with
device events around each call — still camera, so every hit pixel reprojects and reads its four taps: warmed, the median of --calls
calls, prev and next swapped after every call, for 5 iterations and the other counts.  rt_denoise is timed the same way beside it.
With --rocprof the same calls run once each (no timing) for a `rocprofv3 --kernel-trace --stats` run of their own.
The bytes bound: the unique bytes each launch must move over the measured HBM rate — rt_denoise's launches (tools/denoise_time.py)
plus the temporal pass (reads lv, nz: 32 B, first_prim 4 B, four history planes 64 B; writes lv 16 B, three history planes 48 B) and
the colour plane the first step writes (16 B).
    python tools/denoise_temporal_time.py [--calls 11] [--out profiles/r08/denoise_temporal_time.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtp_bindings as rb  # noqa: E402
from denoise_time import HBM_BYTES_PER_S, bounds  # noqa: E402


def temporal_bytes(pixels, iterations):
    b, _ = bounds(pixels, max(iterations, 1))
    if iterations == 0:     # prepass without output, moments, then the temporal pass remodulates (12 B of output)
        b -= pixels * (48 + 16)
        b += pixels * 12
    return b + pixels * (32 + 4 + 64 + 16 + 48) + (pixels * 16 if iterations > 0 else 0)


class Frame:
    def __init__(self, host, cam):
        import torch
        self.cam = cam
        dev = rb.DeviceScene(host, device=0)
        h, w = cam.image_height, cam.image_width
        self.fb = torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")
        self.aov = {"albedo": torch.empty_like(self.fb), "normal": torch.empty_like(self.fb),
                    "depth": torch.empty((h, w), dtype=torch.float32, device="cuda:0"),
                    "hits": torch.empty((h, w), dtype=torch.int32, device="cuda:0"), "prim": torch.empty((h, w), dtype=torch.int32, device="cuda:0")}
        dev.render(cam, self.fb.data_ptr())
        dev.render_aov(cam, {k: v.data_ptr() for k, v in self.aov.items()})
        dev.close()
        lib = rb.amd_lib()
        self.hist_bytes = lib.rt_denoise_history_bytes(w, h)
        self.hist = [torch.zeros(self.hist_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        self.ws = torch.empty(lib.rt_denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
        self.out = torch.empty_like(self.fb)
        self.k = 0
        torch.cuda.synchronize()

    def temporal(self, iterations, stream=None):
        prev, nxt = self.hist[self.k & 1], self.hist[(self.k + 1) & 1]
        rb.denoise_temporal(self.fb.data_ptr(), {k: v.data_ptr() for k, v in self.aov.items()}, self.cam, prev.data_ptr(), nxt.data_ptr(),
                            self.hist_bytes, self.out.data_ptr(), (self.ws.data_ptr(), self.ws.numel()), stream=stream, iterations=iterations)
        self.k += 1

    def spatial(self, iterations, stream=None):
        rb.denoise(self.fb.data_ptr(), {k: v.data_ptr() for k, v in self.aov.items() if k != "prim"}, self.cam.image_width,
                   self.cam.image_height, self.cam.samples_per_pixel, self.out.data_ptr(), stream=stream,
                   workspace=(self.ws.data_ptr(), self.ws.numel()), iterations=iterations)


def measure(name, fr, which, iterations, calls):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    call = fr.temporal if which == "temporal" else fr.spatial
    times = []
    for k in range(calls + 3):          # three warm-up calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(iterations, stream)
        e1.record()
        e1.synchronize()
        if k >= 3:
            times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    pixels = fr.cam.image_width * fr.cam.image_height
    b = temporal_bytes(pixels, iterations) if which == "temporal" else bounds(pixels, iterations)[0]
    row = {"case": name, "call": which, "iterations": iterations, "calls": calls, "median_ms": round(ms, 4), "min_ms": round(min(times), 4),
           "max_ms": round(max(times), 4), "bytes": b, "bytes_bound_ms": round(b / HBM_BYTES_PER_S * 1e3, 4),
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
        fr = Frame(host, rb.rtiow_camera(w, h, args.spp, 50))
        fr.temporal(5)                      # a history for every call below
        for it in ((5, 0, 1, 8) if w == 1920 else (5,)):
            if args.rocprof:
                fr.temporal(it)
                torch.cuda.synchronize()
            else:
                rows.append(measure(name, fr, "temporal", it, args.calls))
                rows.append(measure(name, fr, "spatial", it, args.calls))
    if args.out and not args.rocprof:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"version": rb.amd_lib().rt_version_string().decode(), "spp": args.spp, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
