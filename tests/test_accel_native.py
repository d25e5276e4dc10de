"""Builds tests/cpu_native/test_accel.cpp with AddressSanitizer + UBSan against the host mirror and
the device-table packer (csrc/rt_accel.cpp) and runs it: structural invariants of the threaded /
explicit-link / child-pair tables, input validation, and a sanitizer sweep of the host code."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray-tracing-practice_amd")


def test_accel_tables_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_accel")
    srcs = [os.path.join(ROOT, "tests", "cpu_native", "test_accel.cpp"), os.path.join(PKG, "csrc", "rt_accel.cpp")]
    srcs += [os.path.join(PKG, "host", f) for f in ("bvh_builder.cpp", "scene_params.cpp", "scene_builder.cpp", "texture_io.cpp",
                                                    "jpeg_decoder.cpp", "png_writer.cpp", "camera.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-o", exe] + srcs
    subprocess.run(cmd, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout


def test_pass_sizing_keeps_the_work_index_bound(tmp_path):
    """rt_render's pass sizing (csrc/rt_accel.cpp: plan_passes, make_magic) under AddressSanitizer + UBSan: make_magic against
    integer division for every divisor up to 65536 (at 0, d - 1, d, k*d +- 1 near the top and at the largest accepted n) and
    1e6 random pairs, through both of the kernel's division forms; and over a grid of frames and row shards (1 pixel to
    2^24), spp, forced pass sizes and workspace budgets, every pass keeps pixels * pass + 64 <= 2^30 — the bound the kernel's
    div_magic, kFlagHole and kAbandonedCounter rely on, which 2^24 pixels at 64 spp and a forced pass_spp of 300 at 3840x2160
    used to break — and the passes cover the samples in order, automatic ones equally long."""
    exe = str(tmp_path / "test_pass_plan")
    srcs = [os.path.join(ROOT, "tests", "cpu_native", "test_pass_plan.cpp"), os.path.join(PKG, "csrc", "rt_accel.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-o", exe] + srcs, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and "plan_passes: 5712 cases" in out.stdout, out.stdout


def test_margin_budget_against_adversarial_rays(tmp_path):
    """The error budget behind the guarded walk's margins (gamma = 24 ulp of |oc|^2 |d|^2 in hit_sphere's discriminant,
    docs/LOG.md §3b): 400 k rays aimed at and around the silhouettes of tiny spheres from up to 2 000 units away — where
    hb^2 - a*c cancels — through the oracle's hit_sphere; every computed hit, true or phantom (a quarter of them are
    phantom hits of rays that miss), must lie within gamma |oc|^2 / (2 r) of the surface.  The largest budget these rays
    actually use is just under 8 ulp — which is why 8 (round 1's margin for big scenes) is not a bound and 24 is."""
    import re
    exe = str(tmp_path / "margin_bound")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-std=gnu11", "-w", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpu_native", "test_margin_bound.c"), "-lm", "-lpthread"], check=True)
    out = subprocess.run([exe, "400000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"computed hits (\d+)\s+phantom hits (\d+)\s+largest budget used ([0-9.]+) ulp", out.stdout)
    assert m, out.stdout
    hits, phantom, used = int(m.group(1)), int(m.group(2)), float(m.group(3))
    assert hits > 200000 and phantom > 10000          # the cancellation cases are really being produced
    assert 4.0 < used < 24.0


def test_primary_ray_candidate_lists_hold_every_hit(tmp_path):
    """csrc/rt_beam.h (the per-pixel candidate lists of the primary-visibility pass) against the oracle: for pixels of six
    frames — the headline frame, fat pixels, a camera between the spheres, the config scene (planes), distance-aware margins —
    every sphere whose hit_sphere can report a hit for any sampled camera ray of the pixel, and the oracle's closest hit, is
    on the pixel's list (or the pixel has none)."""
    exe = str(tmp_path / "test_beam")
    srcs = [os.path.join(ROOT, "tests", "cpu_native", "test_beam.cpp"), os.path.join(PKG, "csrc", "rt_accel.cpp")]
    srcs += [os.path.join(PKG, "host", f) for f in ("bvh_builder.cpp", "scene_params.cpp", "scene_builder.cpp", "texture_io.cpp",
                                                    "jpeg_decoder.cpp", "png_writer.cpp", "camera.cpp")]
    obj = str(tmp_path / "rt_oracle.o")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-std=gnu11", "-w", "-c", "-o", obj, os.path.join(ROOT, "oracle", "rt_oracle.c")], check=True)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe] + srcs + [obj, "-lpthread", "-lm"], check=True)
    out = subprocess.run([exe, "8"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout
