"""Developer tool (GPU): what rt_denoise_temporal_spp costs beside rt_denoise_temporal and rt_denoise_spp.  An adaptive frame of the
headline camera (S-rtiow, 1920x1080, rt_render_adaptive at --spp min:batch:max and --threshold) with its moments, the AOVs (first_prim
included) at min_spp, and a uniform frame at min_spp are rendered once; then rt_denoise_temporal_spp with moments, without,
rt_denoise_temporal of the uniform frame and rt_denoise_spp with moments are timed with device events around each call: warmed, the
median of --calls calls, at --iterations.  The temporal calls run as an animation does: the two histories swapped after every call, so
every timed call reprojects into a full history of a still camera.  The new call reads 4 B (counts; 12 B with moments) more per pixel
in its prepass, 4 B in its temporal pass and 4 B in its last step, and no plane more per tap; `extra_bytes_ms` is those bytes over the
measured HBM rate.
--parent-lib PATH: rt_denoise_temporal alone is timed in child processes on another build of librtp_amd.so (the parent commit's,
which has no rt_denoise_temporal_spp) between two runs of this tree's, so that the three sit in one visit to one card:
    python tools/denoise_temporal_spp_time.py --parent-lib tools/_ab/parent/librtp_amd.so --out profiles/r23/denoise_temporal_spp_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.29e12           # MI355X float4 copy, measured (tools/denoise_time.py)


def timed(call, calls):
    import torch
    times = []
    for k in range(calls + 3):          # three warm-up calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(k)
        e1.record()
        e1.synchronize()
        if k >= 3:
            times.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
            "times_ms": [round(t, 4) for t in times]}


def measure(args):
    """One process, one library (RTP_AMD_LIB, or this tree's): a dict of the timings."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-practice_amd"))
    import rtp_bindings as rb
    lib = rb.amd_lib()
    lib.rt_set_device(0)
    torch.cuda.init()
    w, h = args.width, args.height
    mn, batch, mx = (int(x) for x in args.spp.split(":"))
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0)
    f32 = dict(dtype=torch.float32, device="cuda:0")
    i32 = dict(dtype=torch.int32, device="cuda:0")
    fb, ufb, out = (torch.empty((h, w, 3), **f32) for _ in range(3))
    spp = torch.empty((h, w), **i32)
    mom = torch.empty((h, w, 2), **f32)
    aov = {"albedo": torch.empty((h, w, 3), **f32), "normal": torch.empty((h, w, 3), **f32), "depth": torch.empty((h, w), **f32),
           "hits": torch.empty((h, w), **i32), "prim": torch.empty((h, w), **i32)}
    ptrs = {k: v.data_ptr() for k, v in aov.items()}
    cam = rb.rtiow_camera(w, h, mn, 50)
    dev.render(cam, ufb.data_ptr())
    dev.render_aov(cam, ptrs)
    hist_bytes = lib.rt_denoise_history_bytes(w, h)
    hist = [torch.zeros(hist_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    ws = torch.empty(lib.rt_denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    workspace = (ws.data_ptr(), ws.numel())
    row = {"library": os.path.relpath(os.environ.get("RTP_AMD_LIB") or os.path.join(ROOT, "ray-tracing-practice_amd", "librtp_amd.so"), ROOT),
           "version": lib.rt_version_string().decode(), "width": w, "height": h, "iterations": args.iterations, "calls": args.calls}
    stream = torch.cuda.current_stream().cuda_stream
    it = args.iterations

    def temporal(k):         # (the first warm-up call reads the other call's history or zeros: an empty one)
        rb.denoise_temporal(ufb.data_ptr(), ptrs, cam, hist[(k + 1) & 1].data_ptr(), hist[k & 1].data_ptr(), hist_bytes, out.data_ptr(), workspace,
                            stream=stream, iterations=it)
    row["rt_denoise_temporal"] = timed(temporal, args.calls)
    if hasattr(lib, "rt_denoise_temporal_spp") and not args.temporal_only:
        dev.render_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), min_spp=mn, batch_spp=batch, max_spp=mx, threshold=args.threshold)
        torch.cuda.synchronize()
        levels, counts = torch.unique(spp, return_counts=True)
        row["adaptive"] = {"min_spp": mn, "batch_spp": batch, "max_spp": mx, "threshold": args.threshold, "mean_spp": round(float(spp.float().mean()), 3),
                           "pixels_per_count": dict(zip(levels.tolist(), counts.tolist()))}
        for name, m in (("rt_denoise_temporal_spp_moments", mom.data_ptr()), ("rt_denoise_temporal_spp_no_moments", None)):
            row[name] = timed(lambda k: rb.denoise_temporal_spp(fb.data_ptr(), spp.data_ptr(), m, ptrs, mn, cam, hist[(k + 1) & 1].data_ptr(),
                                                                hist[k & 1].data_ptr(), hist_bytes, out.data_ptr(), workspace, stream=stream,
                                                                iterations=it), args.calls)
        row["rt_denoise_spp_moments"] = timed(lambda k: rb.denoise_spp(fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), ptrs, mn, w, h, out.data_ptr(),
                                                                       stream=stream, workspace=workspace, iterations=it), args.calls)
        row["rt_denoise_temporal_again"] = timed(temporal, args.calls)
        px = w * h
        row["extra_bytes_ms"] = {"with_moments": round(px * 20 / HBM_BYTES_PER_S * 1e3, 5), "without_moments": round(px * 12 / HBM_BYTES_PER_S * 1e3, 5)}
    dev.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=11)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--spp", default="16:16:256")
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--temporal-only", action="store_true", help="rt_denoise_temporal alone (what --parent-lib's child processes run)")
    ap.add_argument("--parent-lib", default="", help="another build's librtp_amd.so: this tree, that build, this tree again, a process each")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not args.parent_lib:
        result = measure(args)
    else:
        own = [sys.executable, os.path.abspath(__file__), "--calls", str(args.calls), "--width", str(args.width), "--height", str(args.height),
               "--iterations", str(args.iterations), "--spp", args.spp, "--threshold", str(args.threshold)]
        runs = []
        for lib in ("", os.path.abspath(args.parent_lib), "", os.path.abspath(args.parent_lib)):
            env = {k: v for k, v in os.environ.items() if k != "RTP_AMD_LIB"}
            if lib:
                env["RTP_AMD_LIB"] = lib
            r = subprocess.run(own + (["--temporal-only"] if lib else []), env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:          # whatever ended a run: nothing more is started on the card
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode or 1)
            runs.append(json.loads(r.stdout.strip().split("\n")[-1]))
        result = {"order": ["this tree", "parent build", "this tree again", "parent build again"], "runs": runs}
    text = json.dumps(result)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
