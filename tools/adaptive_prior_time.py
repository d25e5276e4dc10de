"""Developer tool (GPU): what the history-aware stopping rule costs.  At the headline camera (S-rtiow, 1920x1080) the
AOVs (first_prim included) at min_spp and an adaptive frame at --spp and --threshold with its moments are rendered once and
rt_denoise_temporal_spp is run twice, so that a full history of a still camera exists.  Then, with device events around each call,
warmed, the median of --calls calls: rt_adaptive_prior on that history; rt_denoise_temporal_spp with moments at 0 iterations (its two
prepasses and denoise_temporal_spp, the kernel rt_adaptive_prior's is a subset of) and at --iterations; the adaptive frame through
rt_render_adaptive_rule; and the same frame through rt_render_adaptive_prior with an all-zero prior — the same counts, the prior
variants of the select and flag kernels — under both rules.
--parent-lib PATH: the frame through rt_render_adaptive_rule alone is timed in child processes on another build of librtp_amd.so (the
parent commit's, which has no rt_adaptive_prior) between two runs of this tree's, so that all sit in one visit to one card:
    python tools/adaptive_prior_time.py --parent-lib tools/_ab/parent/librtp_amd.so --out profiles/r26/adaptive_prior_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    dev = rb.DeviceScene(rb.HostScene.rtiow(), device=0)
    f32 = dict(dtype=torch.float32, device="cuda:0")
    i32 = dict(dtype=torch.int32, device="cuda:0")
    fb, out = torch.empty((h, w, 3), **f32), torch.empty((h, w, 3), **f32)
    spp = torch.empty((h, w), **i32)
    mom, prior, zero = torch.empty((h, w, 2), **f32), torch.empty((h, w, 2), **f32), torch.zeros((h, w, 2), **f32)
    cam = rb.rtiow_camera(w, h, mn, 50)
    stream = torch.cuda.current_stream().cuda_stream
    p = dict(min_spp=mn, batch_spp=batch, max_spp=mx, threshold=args.threshold)
    row = {"library": os.path.relpath(os.environ.get("RTP_AMD_LIB") or os.path.join(ROOT, "ray-tracing-practice_amd", "librtp_amd.so"), ROOT),
           "version": lib.rt_version_string().decode(), "width": w, "height": h, "iterations": args.iterations, "calls": args.calls, **p}

    def frame(rule, with_prior):
        return lambda k: dev.render_adaptive(cam, fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), stream=stream, sync=False, rule=rule,
                                             **(dict(prior=zero.data_ptr()) if with_prior else {}), **p)
    for rule in (0, 1):
        row[f"rt_render_adaptive_rule_{rule}"] = timed(frame(rule, False), args.calls)
        torch.cuda.synchronize()
        row[f"mean_spp_rule_{rule}"] = round(float(spp.float().mean()), 3)
    if hasattr(lib, "rt_adaptive_prior") and not args.rule_only:
        for rule in (0, 1):
            row[f"rt_render_adaptive_prior_zero_{rule}"] = timed(frame(rule, True), args.calls)
            torch.cuda.synchronize()
            assert round(float(spp.float().mean()), 3) == row[f"mean_spp_rule_{rule}"], "a zero prior changes no count"
        for rule in (0, 1):
            row[f"rt_render_adaptive_rule_{rule}_again"] = timed(frame(rule, False), args.calls)
        aov = {"albedo": torch.empty((h, w, 3), **f32), "normal": torch.empty((h, w, 3), **f32), "depth": torch.empty((h, w), **f32),
               "hits": torch.empty((h, w), **i32), "prim": torch.empty((h, w), **i32)}
        ptrs = {k: v.data_ptr() for k, v in aov.items()}
        dev.render_aov(cam, ptrs)
        hist_bytes = lib.rt_denoise_history_bytes(w, h)
        hist = [torch.zeros(hist_bytes, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        ws = torch.empty(lib.rt_denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
        workspace = (ws.data_ptr(), ws.numel())

        def temporal(it):
            return lambda k: rb.denoise_temporal_spp(fb.data_ptr(), spp.data_ptr(), mom.data_ptr(), ptrs, mn, cam, hist[(k + 1) & 1].data_ptr(),
                                                     hist[k & 1].data_ptr(), hist_bytes, out.data_ptr(), workspace, stream=stream, iterations=it)
        row["rt_denoise_temporal_spp_0_iterations"] = timed(temporal(0), args.calls)          # (an even number of calls: hist[1] is the newest)
        row["rt_denoise_temporal_spp"] = timed(temporal(args.iterations), args.calls)
        row["rt_adaptive_prior"] = timed(lambda k: rb.adaptive_prior(ptrs, mn, cam, hist[1].data_ptr(), hist_bytes, prior.data_ptr(), stream=stream),
                                         args.calls)
        torch.cuda.synchronize()
        row["prior_pixels_with_history"] = int((prior[..., 0] > 0).sum())
        row["rt_adaptive_prior_no_history"] = timed(lambda k: rb.adaptive_prior(ptrs, mn, cam, None, 0, prior.data_ptr(), stream=stream), args.calls)
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
    ap.add_argument("--rule-only", action="store_true", help="rt_render_adaptive_rule alone (what --parent-lib's child processes run)")
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
            r = subprocess.run(own + (["--rule-only"] if lib else []), env=env, capture_output=True, text=True, timeout=600)
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
