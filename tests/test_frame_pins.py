"""Whole production frames against oracle-made pins (tests/golden/frame_pins.json, made by tests/golden/make_frame_pins.py), the
stress frame (BASELINE configs[4]) at its own 1000 spp, and frames at the kernel's 2^30 work-index bound.

The pins are the five frames of profiles/r03/full_frame_parity*.json, compared there with the oracle pixel by pixel: per frame
the sha256 of the whole float32 frame and a digest of every band of 8 rows.  A CPU test keeps the pins tied to the oracle as it
is now (two bands of each frame re-rendered); the GPU tests require the same bits from the default path and from every other
route to the frame — passes, row shards, tiles, the exact walk (and, in tests/dev_build_checks.py, wide nodes).

The GPU tests here allocate sample slabs of up to about 13 GB (2^24 pixels at 50 samples per pass, 3840x2160 at 129)."""
import hashlib
import json
import math
import os
import sys
import time

import numpy as np
import pytest

import oracle_bindings as ob
import rtp_bindings as rb

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_frame_pins as mfp  # noqa: E402

PINS = json.load(open(os.path.join(HERE, "golden", "frame_pins.json")))
BAND = PINS["band_rows"]
THREADS = os.cpu_count() or 8
INDEX_ROOM = (1 << 30) - 64          # work indices of one pass, with the 64 behind the last, stay below 2^30 (rt_accel.h)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pinned(name):
    pin = PINS["frames"][name]
    host, cam = mfp.scene_and_camera(pin["scene"], pin["camera"])
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel) == (pin["width"], pin["height"], pin["spp"])
    return pin, host, cam


def default_handle(host, **config):
    """A fresh handle with what rt_config_init gives (plus `config`), whatever another module put in rb.DEFAULTS."""
    cfg = dict(traversal=rb.TRAVERSAL_AUTO, guard_keep=0)
    cfg.update(config)
    return rb.DeviceScene(host, device=0, honour_env=False, **cfg)


def assert_pinned(fb, pin, what):
    """The frame's band digests (and whole-frame sha256) are the pin's; on failure, which bands differ."""
    assert fb.shape == (pin["height"], pin["width"], 3), (what, fb.shape)
    got = [mfp.band_digest(fb[r:r + BAND]) for r in range(0, pin["height"], BAND)]
    bad = [k for k, (g, w) in enumerate(zip(got, pin["band_sha256_16"])) if g != w]
    assert not bad, f"{what}: {len(bad)} of {len(got)} bands of {BAND} rows differ from the pin, first rows {[k * BAND for k in bad[:12]]}"
    assert hashlib.sha256(np.ascontiguousarray(fb, dtype=np.float32).tobytes()).hexdigest() == pin["frame_sha256"], what
    print(f"PIN {pin['config']} — {what}: all {len(got)} bands match")


def test_pins_are_the_oracles_bands():
    """CPU: the oracle as it is now re-renders the first band and a middle band of every pinned frame to the pinned digests
    (and the pins are the r03 records' frames)."""
    assert set(PINS["frames"]) == {"headline", "c5", "default7", "low", "top"}
    for name in PINS["frames"]:
        pin, host, cam = pinned(name)
        rec = json.load(open(os.path.join(HERE, "..", pin["record"])))
        assert rec["frame_sha256"] == pin["frame_sha256"] and rec["pixels_differing"] == 0, name
        assert len(pin["band_sha256_16"]) == math.ceil(pin["height"] / BAND)
        mid = (len(pin["band_sha256_16"]) // 2) * BAND
        for r0 in (0, mid):
            rows = ob.render(host, cam, row0=r0, row1=min(r0 + BAND, pin["height"]), threads=THREADS)
            assert mfp.band_digest(rows) == pin["band_sha256_16"][r0 // BAND], (name, r0)
        host.close()


@pytest.mark.gpu
def test_pinned_frames_through_default_handles():
    """Each of the five pinned frames through a fresh default handle: every band is the pin's."""
    for name in PINS["frames"]:
        pin, host, cam = pinned(name)
        dev = default_handle(host)
        t0 = time.time()
        fb, t = dev.render_to_host(cam)
        assert_pinned(fb, pin, f"default handle ({t.trace_launches} trace launches, {time.time() - t0:.2f} s)")
        dev.close()


@pytest.mark.gpu
def test_headline_pins_through_passes_shards_and_tiles():
    """The headline frame (1920x1080x500) in forced passes of 64 (eight, the last short) and of 192 (192/192/116), assembled
    from a 3-way row shard with bands of 8, and from four tiles of unequal size: the same pinned bits each time."""
    import frame_parallel as fp
    pin, host, cam = pinned("headline")
    W, H = cam.image_width, cam.image_height
    dev = default_handle(host)
    for forced, launches in ((64, 8), (192, 3)):
        dev.configure(pass_spp=forced)
        fb, t = dev.render_to_host(cam)
        assert t.trace_launches == launches, (forced, t.trace_launches)
        assert_pinned(fb, pin, f"passes of {forced} spp ({launches} launches)")
    dev.configure(pass_spp=0)
    frame = np.full((H, W, 3), np.nan, dtype=np.float32)
    for r in range(3):
        part, _ = dev.render_to_host(cam, rb.Shard(8, 3, r))
        rows = fp.shard_row_indices(H, 8, 3, r)
        assert part.shape[0] == len(rows)
        frame[rows] = part
    assert_pinned(frame, pin, "3-way row shard, bands of 8")
    frame = np.full((H, W, 3), np.nan, dtype=np.float32)
    for (x0, x1), (y0, y1) in (((0, 701), (0, 389)), ((701, W), (0, 389)), ((0, 1333), (389, H)), ((1333, W), (389, H))):
        tile, _ = dev.render_tile_to_host(cam, x0, y0, x1 - x0, y1 - y0)
        frame[y0:y1, x0:x1] = tile
    assert_pinned(frame, pin, "four tiles of unequal size")
    dev.close()


@pytest.mark.gpu
def test_pins_through_the_exact_walk():
    """The "top" view (the most flagged of the five frames) through the exact walk alone: the pinned bits.  (The default-config
    frame 7 through the 4-wide node walk, an experiment of the developer build, is checked by tests/dev_build_checks.py.)"""
    pin, host, cam = pinned("top")
    dev = default_handle(host, traversal=rb.TRAVERSAL_EXACT)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 0
    assert_pinned(fb, pin, "exact walk")
    dev.close()


def _rows_match_oracle(fb, host, cam, rows, what):
    for r in rows:
        want = ob.render(host, cam, row0=r, row1=r + 1, threads=THREADS)
        assert np.array_equal(bits(fb[r:r + 1]), bits(want)), f"{what}: row {r} differs from the oracle"


@pytest.mark.gpu
def test_stress_frame_at_its_own_1000_spp():
    """BASELINE configs[4]: S-100k (99 857 spheres + a 2048^2 textured quad) at 3840x2160x1000, depth 50, through a fresh
    default handle — several passes, the guarded walk with distance-aware margins, tables read through L1 / L2.  Rows 0, 1080
    and 2159, two rows through the textured quad and two through the sphere field against the oracle.  Then forced passes of
    300 spp (clamped to the work-index bound, 129: 7 x 129 + 97) must give the same bits."""
    host = rb.HostScene.rtiow(half_extent=158, textured_quad=True, texture_size=2048)
    cam = rb.rtiow_camera(3840, 2160, 1000, 50)
    dev = default_handle(host)
    t0 = time.time()
    fb, t = dev.render_to_host(cam)
    secs = time.time() - t0
    assert t.trace_launches > 1 and t.guarded == 1 and t.guard_dynamic == 1 and t.scene_in_lds == 0, \
        (t.trace_launches, t.guarded, t.guard_dynamic, t.scene_in_lds)
    assert t.trace_launches >= math.ceil(1000 * 3840 * 2160 / INDEX_ROOM)
    print(f"REPORT configs[4] 3840x2160x1000: {t.trace_launches} trace launches, kernel {t.kernel_ms:.1f} ms, call {secs:.2f} s, "
          f"flagged {t.flagged_samples}, abandoned passes {t.abandoned_passes}")
    # (oracle statistics at 1 spp: rows 1700 and 2000 fetch the quad's texture most, 700 and 1100 test the most spheres)
    _rows_match_oracle(fb, host, cam, (0, 700, 1080, 1100, 1700, 2000, 2159), "configs[4] at 1000 spp")
    dev.configure(pass_spp=300)
    forced, tf = dev.render_to_host(cam)
    assert tf.trace_launches == 8, tf.trace_launches
    assert np.array_equal(bits(forced), bits(fb)), "forced passes of 300 spp (clamped to 129) change the frame"
    print(f"REPORT configs[4] with pass_spp=300: {tf.trace_launches} trace launches, the same bits")
    dev.close()


@pytest.mark.gpu
def test_frames_at_the_work_index_bound():
    """S-rtiow at the largest frame rt_render accepts, 4096x4096 = 2^24 pixels: at 64 spp (once a single pass of exactly 2^30
    work indices), at 200 spp, and at 100 spp with a forced pass_spp of 90 (clamped to 63).  Every pass keeps its work indices
    and the 64 behind them below 2^30, so each needs at least ceil(spp * pixels / (2^30 - 64)) trace launches; the first, middle
    and last rows are the oracle's.  (Slabs of up to about 13 GB.)"""
    host = rb.HostScene.rtiow()
    W = H = 4096
    for spp, forced in ((64, 0), (200, 0), (100, 90)):
        cam = rb.rtiow_camera(W, H, spp, 50)
        dev = default_handle(host, pass_spp=forced)
        fb, t = dev.render_to_host(cam)
        dev.close()
        need = math.ceil(spp * W * H / INDEX_ROOM)
        assert t.trace_launches >= need, (spp, forced, t.trace_launches, need)
        print(f"REPORT 4096x4096x{spp} pass_spp={forced}: {t.trace_launches} trace launches (at least {need})")
        _rows_match_oracle(fb, host, cam, (0, H // 2, H - 1), f"4096x4096x{spp} pass_spp={forced}")


@pytest.mark.gpu
def test_abandoned_pass_at_the_work_index_bound():
    """A heavily flagged 2^24-pixel frame (tools/guard_stress.py scene 4 of seed 9: 325 overlapping spheres) at 64 spp through
    the default bail-out: a guarded pass gives up in the launch and raises its work counter to 2^30 (kAbandonedCounter), which
    must lie beyond the last work index of the pass for every later reservation to find it dry.  The frame's first, middle and
    last rows are the oracle's."""
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    import guard_stress
    W = H = 4096
    for k, sph, pl, mats, cam, spread in guard_stress.scenes(9, 5, 64, W, H):
        if k == 4:
            host = rb.HostScene.from_arrays(sph, pl, mats)
            break
    assert host.desc.num_spheres == 325
    dev = default_handle(host)
    fb, t = dev.render_to_host(cam)
    dev.close()
    assert t.abandoned_passes >= 1 and t.trace_launches >= 2, (t.abandoned_passes, t.trace_launches)
    print(f"REPORT stress scene 4096x4096x64: {t.trace_launches} trace launches, {t.abandoned_passes} abandoned")
    _rows_match_oracle(fb, host, cam, (0, H // 2, H - 1), "heavily flagged 4096x4096x64")
