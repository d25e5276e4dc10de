"""rt_render_aov_volume (include/rtp_amd.h, "AOVs under fog"): the five AOV buffers and the transmittance of a fogged frame,
for rt_denoise and rt_denoise_spp.  The contract's restatement is tests/cpu_native/aov_volume_ref.c (tests/aov_volume_reference.py); the CPU
tests check the restatement, the ABI and the refusals, the GPU tests the kernels against the restatement, byte for byte.  Scenes, media,
grids and cameras are tests/test_medium.py's and tests/test_volume.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_volume_reference as avr
import denoise_reference as dnr
import denoise_spp_reference as dsr
import lens_reference as lnr
import rtp_bindings as rb
import volume_reference as vr
from test_lit import assert_same
from test_medium import ABSORB_N, BACKGROUND, FAR_BALL, _channel_z, _fog_ball_scene, dev_kw, media, ref_kw, scenes
from test_volume import BOX, GRIDS, WALK_TOL, random_grid, special_camera

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "ray-tracing-practice_amd", "rtp_main")
INVALID = 1
FAKE = 1 << 32          # a device address that is never dereferenced
FIVE = ("albedo", "normal", "depth", "hits", "prim")
LN2 = np.float32(0.693147182)


def same_aovs(got, want, what, keys=avr.KEYS):
    for k in keys:
        assert_same(got[k], want[k], f"{what}: {k}")


def camera_kw(scene, kind, w, h, spp, depth=12):
    """pinhole / lens / lens + motion → the keywords of the restatement and of the device call (cam_close, lens)."""
    if kind == "pinhole":
        return {}, {}
    r, d = dict(ref_kw(scene, "lens + motion", w, h, spp, depth)), dict(dev_kw(scene, "lens + motion", None, w, h, spp, depth))
    if kind == "lens":
        r.pop("cam_close")
        d.pop("cam_close")
    return r, d


# ---- no GPU needed ---------------------------------------------------------------------------------------------------------------------

def test_abi_and_defaults():
    lib = rb.amd_lib()
    assert hasattr(lib, "rt_render_aov_volume") and "rt_render_aov_volume" in rb.RTP_AMD_SYMBOLS
    assert len(lib.rt_render_aov_volume.argtypes) == 12
    for name in ("render_aov_volume", "render_aov_volume_to_host"):
        assert hasattr(rb.DeviceScene, name)
    header = open(os.path.join(ROOT, "include", "rtp_amd.h")).read()
    assert "#define RT_AOV_FOG_REM 0.693147182f" in header
    assert LN2 == np.float32(np.log(2.0))
    assert C.sizeof(rb.AovBuffers) == 48          # rt_aov_buffers is unchanged: the transmittance is a separate argument


def _call(cam, bufs, lit=None, medium=None, volume=None, tr=None, sample_first=0):
    """(status, message) of rt_render_aov_volume with a null scene."""
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    st = lib.rt_render_aov_volume(None, C.byref(cam), C.byref(lit) if lit is not None else None, C.byref(medium) if medium is not None else None, volume, None,
                                  sample_first, C.byref(bufs) if bufs is not None else None, tr, None, 1, None)
    return st, lib.rt_get_last_error_string().decode()


def test_refusals_before_the_scene_is_looked_at():
    """The buffers first, then rt_render_volume's refusals in its order — lit, the medium's, the volume's (a medium with region 2) — then the
    null scene: all with a null scene, so nothing can have been enqueued, and the volume's handle is never read (it is not one).  Every
    message names the call."""
    cam = rb.rtiow_camera(8, 4, 2)
    handle = C.c_void_p(FAKE)
    good = rb._aov_struct(dict(albedo=FAKE))
    box = dict(box=(0, 0, 0, 1, 1, 1))
    bad_lit, bad_medium = rb.lit_params(nee=dict(mis=2)), rb.medium_params(sigma_t=-1.0)

    def refused(word, *args, **kw):
        st, msg = _call(cam, *args, **kw)
        assert st == INVALID and word in msg and "rt_render_aov_volume" in msg, (word, st, msg)
    # the buffers: before everything else, and a transmittance pointer does not stand in for them
    short = rb._aov_struct(dict(albedo=FAKE))
    short.struct_bytes = 8
    for bufs, word in ((None, "null AOV buffers"), (short, "struct_bytes"), (rb._aov_struct({}), "every AOV buffer is NULL")):
        refused(word, bufs, lit=bad_lit, medium=bad_medium, volume=handle)
        refused(word, bufs, tr=C.c_void_p(FAKE))
    # rt_render_lit's, then the medium's, then the volume's
    refused("mis", good, lit=bad_lit, medium=bad_medium, volume=handle)
    refused("sigma_t", good, medium=bad_medium, volume=handle)
    for s in (float("nan"), float("inf")):
        refused("sigma_t", good, medium=rb.medium_params(sigma_t=s, **box))
    refused("albedo", good, medium=rb.medium_params(sigma_t=1.0, albedo=(0.5, 1.5, 0.5), **box))
    refused("|g|", good, medium=rb.medium_params(sigma_t=1.0, g=0.96, **box))
    refused("lo < hi", good, medium=rb.medium_params(sigma_t=1.0, box=(0, 0, 0, 1, -1, 1)), volume=handle)
    for medium in (None, rb.medium_params(sigma_t=1.0), rb.medium_params(sigma_t=0.0), rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1))):
        refused("region 2", good, medium=medium, volume=handle)
    # what passes reaches the scene
    for medium, volume in ((rb.medium_params(sigma_t=1.0, **box), handle), (rb.medium_params(sigma_t=0.0, **box), handle), (None, None),
                           (rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), None)):
        refused("null scene", good, medium=medium, volume=volume, tr=C.c_void_p(FAKE))


def test_cli_refusals(test_config_text, tmp_path):
    """--fog-denoise needs --fog and is refused with --denoise*, --aov, --adaptive, --devices and --shard: exit code 99, a message that names
    the flag, nothing written."""
    fog = ["--lit", "--fog", "0.5", "--fog-denoise"]
    cases = [["--lit", "--fog-denoise"], ["--fog-denoise"], ["--lit", "--fog-box", "0,0,0,1,1,1", "--fog-denoise"]]
    cases += [fog + extra for extra in (["--denoise"], ["--denoise-temporal"], ["--denoise-adaptive"], ["--denoise-adaptive-temporal"], ["--aov"],
                                        ["--adaptive", "0.1"], ["--devices", "2"], ["--shard", "2"], ["--fog-noise-target", "0.3", "--aov"])]
    for args in cases:
        res = subprocess.run([EXE, "--gpu"] + args, input=test_config_text, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert res.returncode == 99 and "--fog-denoise" in res.stderr, (args, res.returncode, res.stderr[-300:])
    assert not os.listdir(tmp_path)


IDENTITY_VIEW = (12, 8, 2)


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_restatement_identities(scene):
    """No medium is lens_reference.aov (the transmittance spp); a 1 x 1 x 1 grid of density 1 is the homogeneous box; a grid of zeros and a
    region no camera ray touches are lens_reference.aov again — for the pinhole, the lens and the lens with an open shutter."""
    host, camera, _ = scenes()[scene]
    w, h, spp = IDENTITY_VIEW
    cam = camera(w, h, spp, 12)
    box = media(scene)["box g=-0.5"]
    for kind in ("pinhole", "lens", "lens + motion"):
        kw, _ = camera_kw(scene, kind, w, h, spp)
        lens = kw.get("lens")
        want = lnr.aov(host, cam, cam_close=kw.get("cam_close"), **(dict(radius=lens[0], focus=lens[1]) if lens else {}))
        want["transmittance"] = np.full((h, w), spp, np.float32)
        for name, medium, density in (("none", None, None), ("sigma_t = 0", dict(sigma_t=0.0, ball=(0, 1, 0, 3)), None), ("far ball", FAR_BALL, None),
                                      ("zero grid", box, np.zeros((5, 3, 2), np.float32))):
            same_aovs(avr.aov(host, cam, medium=medium, density=density, **kw), want, f"{scene} / {kind} / {name}")
        hom = avr.aov(host, cam, medium=box, **kw)
        same_aovs(avr.aov(host, cam, medium=box, density=np.ones((1, 1, 1), np.float32), **kw), hom, f"{scene} / {kind} / 1^3 grid")
        assert (hom["transmittance"] < spp).any() and (hom["hits"] >= want["hits"]).all()


@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_restatement_properties(scene):
    """Every sum finite; hit_count >= rt_render_aov_lens's and <= spp; 0 <= transmittance_sum <= spp; a covered pixel whose samples all
    missed has a non-zero normal; first_prim is rt_render_aov_lens's."""
    host, camera, _ = scenes()[scene]
    w, h, spp = 24, 16, 3
    cam = camera(w, h, spp, 12)
    first = lnr.aov(host, cam)
    covered_misses = 0
    cases = [(name, m, None) for name, m in media(scene).items()] + [("grid " + g, dict(media(scene)["box g=-0.5"], box=BOX), GRIDS[g]) for g in ("2x3x5", "16")]
    for name, medium, density in cases:
        a = avr.aov(host, cam, medium=medium, density=density)
        what = f"{scene} / {name}"
        for k in ("albedo", "normal", "depth", "transmittance"):
            assert np.isfinite(a[k]).all(), (what, k)
        assert (a["hits"] >= first["hits"]).all() and (a["hits"] <= spp).all(), what
        assert (a["transmittance"] >= 0).all() and (a["transmittance"] <= spp).all(), what
        assert_same(a["prim"], first["prim"], what + ": first_prim")
        sky = (first["hits"] == 0) & (a["hits"] > 0)
        covered_misses += int(sky.sum())
        assert (np.abs(a["normal"][sky]).sum(-1) > 0).all(), what
        # (the fog's normal faces the camera: against the view direction of a sky pixel)
        assert (a["depth"][sky] > 0).all(), what
    assert covered_misses > 20


def test_refined_grid_has_the_coarse_transmittance():
    """The 2 x refined grid (every cell split in eight of its density) against the coarse one: per sample the optical depths differ by at most
    WALK_TOL * tau_max each against the exact sum (DESIGN.md §28's bound, tau_max = sigma_t * max(rho) * |hi - lo|), Tr = exp(-tau) has
    |dTr| <= |dtau|, and exp_libm adds half an ulp of a number <= 1 — summed over spp samples."""
    host, camera, _ = scenes()["three balls"]
    w, h, spp = 24, 16, 3
    cam = camera(w, h, spp, 12)
    medium = dict(sigma_t=0.5, albedo=0.9, g=0.0, box=BOX)
    coarse = GRIDS["2x3x5"]
    fine = np.repeat(np.repeat(np.repeat(coarse, 2, 0), 2, 1), 2, 2)
    a = avr.aov(host, cam, medium=medium, density=coarse)["transmittance"].astype(np.float64)
    b = avr.aov(host, cam, medium=medium, density=fine)["transmittance"].astype(np.float64)
    tau_max = medium["sigma_t"] * float(coarse.max()) * float(np.linalg.norm(np.array(BOX[3:]) - np.array(BOX[:3])))
    bound = spp * (2 * WALK_TOL * tau_max + 2 * 2.0 ** -24) + spp * 2.0 ** -23          # (+ the float32 sums themselves)
    print("max difference", float(np.abs(a - b).max()), "bound", bound)
    assert np.abs(a - b).max() <= bound and (a < spp).any()


def test_transmittance_is_the_absorption_expectation():
    """albedo = 0, nothing but the background behind a random 4^3 grid, no emitters: a sample of rt_render_volume's restatement is the
    background or 0, so its per-channel mean over ABSORB_N samples is background * transmittance_sum / spp up to sampling noise — the AOV is
    the exact expectation the Beer-Lambert tests estimate.  tests/test_medium.py's _channel_z and its bound, the exact frame with no
    variance of its own."""
    host = _fog_ball_scene()
    w = h = 9
    cam = rb.make_camera(w, h, 20.0, (0, 1, 8), (0, 0, 0), BACKGROUND, ABSORB_N, 8)
    medium = dict(sigma_t=0.9, albedo=0.0, box=(-1, -1, -1, 1, 1, 1))
    density = random_grid((4, 4, 4), 21)
    mom = vr.frame(host, cam, medium=medium, density=density, emitters=False, moments=True)[1]
    a = avr.aov(host, cam, medium=medium, density=density)
    mean = np.asarray(BACKGROUND, np.float32).astype(np.float64)[None, None, :] * (a["transmittance"].astype(np.float64) / ABSORB_N)[..., None]
    exact = np.concatenate([mean * ABSORB_N, mean * mean * ABSORB_N], -1)
    z = _channel_z(mom, exact, ABSORB_N)
    fogged = a["transmittance"] < ABSORB_N
    print("max |z|", float(np.abs(z).max()), "fogged pixels", int(fogged.sum()))
    assert np.abs(z).max() <= 4.5 and fogged.sum() >= 9
    assert (a["hits"][fogged] > 0).all() and (a["prim"] == -1).all()


def _tonemapped(fb_sum, spp):
    return np.sqrt(np.clip(fb_sum.astype(np.float64) / spp, 0.0, None))


@pytest.mark.parametrize("scene,medium", [("three balls", "box g=-0.5"), ("night rtiow", "all space g=0")])
def test_fog_aware_guides_denoise_better_than_first_hit_guides(scene, medium):
    """96 x 64 x 4 spp against 512 spp, rt_denoise at its defaults on the restatements: the sqrt-tonemapped MSE under the fog-aware guides is
    strictly smaller than under the first-hit guides.  Measured, as multiples of the noisy frame's error: three balls 0.28
    against 0.76, night rtiow 0.30 against 0.57 — an ordering with a factor of about 2 in hand."""
    host, camera, _ = scenes()[scene]
    m = media(scene)[medium]
    ref = _tonemapped(vr.frame(host, camera(96, 64, 512, 12), medium=m), 512)
    cam = camera(96, 64, 4, 12)
    noisy = vr.frame(host, cam, medium=m)
    err = {"noisy": np.mean((_tonemapped(noisy, 4) - ref) ** 2)}
    for name, aov in (("first-hit", lnr.aov(host, cam)), ("fog-aware", avr.aov(host, cam, medium=m))):
        err[name] = np.mean((_tonemapped(dnr.reference(noisy, aov, 4), 4) - ref) ** 2)
    print(scene, {k: float(v / err["noisy"]) for k, v in err.items()})
    assert err["fog-aware"] < err["first-hit"]


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------

def fog(g=0.0):
    return dict(sigma_t=0.5, albedo=(0.95, 0.9, 0.8), g=g, box=BOX)


VIEW = (16, 9, 3)
GRID_256 = random_grid((1, 1, 256), 41)


@pytest.mark.gpu
def test_frames_equal_the_restatement():
    """40 x 27 x 3 spp, 7 x 5 x 1, a 3-row shard of the first, sample_first = 5, a handle with pass_spp = 2 (the sums cross passes), and
    sync = 0 on a torch stream."""
    import torch
    scene = "three balls"
    host, camera, _ = scenes()[scene]
    medium, density = fog(0.7), GRIDS["2x3x5"]
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(density) as vol:
        for (w, h, spp), more in (((40, 27, 3), {}), ((7, 5, 1), {}), ((40, 27, 3), dict(shard=rb.Shard(3, 1, 4))), ((40, 27, 3), dict(sample_first=5))):
            cam = camera(w, h, spp, 12)
            got, _ = dev.render_aov_volume_to_host(cam, medium=medium, volume=vol, **more)
            same_aovs(got, avr.aov(host, cam, medium=medium, density=density, **more), f"frame {w}x{h}x{spp} {more}")
        w, h, spp = 40, 27, 3
        cam = camera(w, h, spp, 12)
        kw_r, kw_d = camera_kw(scene, "lens + motion", w, h, spp)
        want = avr.aov(host, cam, medium=medium, density=density, **kw_r)
        dev.configure(pass_spp=2)
        got, _ = dev.render_aov_volume_to_host(cam, medium=medium, volume=vol, **kw_d)
        same_aovs(got, want, "pass_spp = 2")
        got, _ = dev.render_aov_volume_to_host(cam, medium=medium, volume=None, **kw_d)
        same_aovs(got, avr.aov(host, cam, medium=medium, **kw_r), "pass_spp = 2, no grid")
        dev.configure(pass_spp=0)
        stream = torch.cuda.Stream()
        shapes = dict(albedo=(h, w, 3), normal=(h, w, 3), depth=(h, w), hits=(h, w), prim=(h, w), transmittance=(h, w))
        bufs = {k: torch.full(s, 7, dtype={"hits": torch.int32, "prim": torch.int32}.get(k, torch.float32), device="cuda:0") for k, s in shapes.items()}
        with torch.cuda.stream(stream):
            dev.render_aov_volume(cam, {k: bufs[k].data_ptr() for k in FIVE}, medium=medium, volume=vol, stream=stream.cuda_stream, sync=False,
                                  transmittance=bufs["transmittance"].data_ptr(), **kw_d)
        stream.synchronize()
        same_aovs({k: v.cpu().numpy().view(want[k].dtype) for k, v in bufs.items()}, want, "sync = 0 on a torch stream")
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow", "fuzz planes"])
def test_regions_grids_and_cameras_equal_the_restatement(scene):
    """The regions 0 / 1 / 2 without a grid, the grids 1^3, 2 x 3 x 5, 16^3, 1 x 1 x 64 and 256 x 1 x 1, under the pinhole, the lens and
    the lens with an open shutter in turn."""
    host, camera, _ = scenes()[scene]
    w, h, spp = VIEW
    cam = camera(w, h, spp, 12)
    si = ["three balls", "night rtiow", "fuzz planes"].index(scene)
    kinds = ("pinhole", "lens", "lens + motion")
    grids = dict(GRIDS, **{"256x1x1": GRID_256})
    dev = rb.DeviceScene(host, device=0)
    covered = 0
    for k, (name, medium) in enumerate(media(scene).items()):
        kw_r, kw_d = camera_kw(scene, kinds[(k + si) % 3], w, h, spp)
        want = avr.aov(host, cam, medium=medium, **kw_r)
        got, _ = dev.render_aov_volume_to_host(cam, medium=medium, **kw_d)
        same_aovs(got, want, f"{scene} / {name} / {kinds[(k + si) % 3]}")
        covered += int((want["transmittance"] < spp).sum())
    for k, (name, density) in enumerate(grids.items()):
        kw_r, kw_d = camera_kw(scene, kinds[(k + si + 1) % 3], w, h, spp)
        medium = fog((0.0, 0.95, -0.95)[k % 3])
        want = avr.aov(host, cam, medium=medium, density=density, **kw_r)
        with rb.Volume(density) as vol:
            got, _ = dev.render_aov_volume_to_host(cam, medium=medium, volume=vol, **kw_d)
        same_aovs(got, want, f"{scene} / grid {name} / {kinds[(k + si + 1) % 3]}")
        covered += int((want["transmittance"] < spp).sum())
    assert covered > 100
    dev.close()


@pytest.mark.gpu
def test_special_cameras_equal_the_restatement():
    """The eye inside the grid, the fan camera whose rays have d_z == 0 along a cell plane of the 16^3 grid, and the camera aimed at a grid
    vertex; the fan through the 1 x 1 x 64 grid as well."""
    host = scenes()["three balls"][0]
    w, h, spp = VIEW
    dev = rb.DeviceScene(host, device=0)
    for grid, kind in (("16", "inside"), ("16", "fan"), ("16", "vertex"), ("1x1x64", "fan"), ("2x3x5", "inside")):
        cam = special_camera(kind, w, h, spp, 12)
        want = avr.aov(host, cam, medium=fog(), density=GRIDS[grid])
        with rb.Volume(GRIDS[grid]) as vol:
            got, _ = dev.render_aov_volume_to_host(cam, medium=fog(), volume=vol)
        same_aovs(got, want, f"grid {grid} / camera {kind}")
        assert (want["transmittance"] < spp).any()
    dev.close()


@pytest.mark.gpu
def test_buffer_cases():
    """Each buffer NULL in turn, the transmittance NULL, and only the transmittance next to one buffer: what is asked for is the restatement's,
    what is not is never written."""
    import torch
    host, camera, _ = scenes()["three balls"]
    w, h, spp = VIEW
    cam = camera(w, h, spp, 12)
    medium, density = fog(0.3), GRIDS["2x3x5"]
    want, hom = avr.aov(host, cam, medium=medium, density=density), avr.aov(host, cam, medium=medium)
    shapes = dict(albedo=(h, w, 3), normal=(h, w, 3), depth=(h, w), hits=(h, w), prim=(h, w), transmittance=(h, w))
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(density) as vol:
        for asked in [tuple(k for k in avr.KEYS if k != skip) for skip in avr.KEYS] + [("depth", "transmittance"), ("prim", "transmittance")]:
            for volume, ref in ((vol, want), (None, hom)):
                bufs = {k: torch.full(s, 7, dtype={"hits": torch.int32, "prim": torch.int32}.get(k, torch.float32), device="cuda:0") for k, s in shapes.items()}
                dev.render_aov_volume(cam, {k: bufs[k].data_ptr() for k in FIVE if k in asked}, medium=medium, volume=volume,
                                      transmittance=bufs["transmittance"].data_ptr() if "transmittance" in asked else None)
                for k in avr.KEYS:
                    a = bufs[k].cpu().numpy()
                    if k in asked:
                        assert_same(a.view(ref[k].dtype), ref[k], f"asked {asked}: {k}")
                    else:
                        assert (a == 7).all(), (asked, k)
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["three balls", "night rtiow"])
def test_device_identities(scene):
    """medium == NULL and sigma_t == 0 are rt_render_aov_lens (its kernels; the transmittance spp); a 1^3 grid of density 1 through the grid
    kernel is volume == NULL with the same box through the homogeneous one; a grid of zeros and a region no camera ray touches give
    rt_render_aov_lens's buffers through the fog kernels."""
    host, camera, _ = scenes()[scene]
    w, h, spp = VIEW
    cam = camera(w, h, spp, 12)
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(np.ones((1, 1, 1), np.float32)) as one, rb.Volume(np.zeros((5, 3, 2), np.float32)) as zero:
        for kind in ("pinhole", "lens + motion"):
            _, kw = camera_kw(scene, kind, w, h, spp)
            want, _ = dev.render_aov_lens_to_host(cam, **kw)
            want["transmittance"] = np.full((h, w), spp, np.float32)
            for name, medium, volume in (("none", None, None), ("sigma_t = 0", dict(sigma_t=0.0, box=BOX), None), ("sigma_t = 0 with a grid", dict(sigma_t=0.0, box=BOX), one),
                                         ("far ball", FAR_BALL, None), ("zero grid", fog(), zero)):
                got, _ = dev.render_aov_volume_to_host(cam, medium=medium, volume=volume, **kw)
                same_aovs(got, want, f"{scene} / {kind} / {name}")
            hom, _ = dev.render_aov_volume_to_host(cam, medium=fog(), **kw)
            got, _ = dev.render_aov_volume_to_host(cam, medium=fog(), volume=one, **kw)
            same_aovs(got, hom, f"{scene} / {kind} / 1^3 grid")
            assert (hom["transmittance"] < spp).any()
    dev.close()


@pytest.mark.gpu
def test_no_samples_and_refusals_with_a_scene():
    """spp <= 0: zero sums, first_prim -1, transmittance 0.  The sample range and a volume with a ball are refused by name."""
    host, camera, _ = scenes()["three balls"]
    dev = rb.DeviceScene(host, device=0)
    cam = camera(7, 5, 0, 12)
    with rb.Volume(GRIDS["2x3x5"]) as vol:
        got, _ = dev.render_aov_volume_to_host(cam, medium=fog(), volume=vol)
        for k in avr.KEYS:
            assert (got[k] == (-1 if k == "prim" else 0)).all(), k
        with pytest.raises(rb.RtError, match="rt_render_aov_volume: sample_first"):
            dev.render_aov_volume_to_host(camera(7, 5, 1, 12), medium=fog(), volume=vol, sample_first=-1)
        with pytest.raises(rb.RtError, match="rt_render_aov_volume.*2\\^30"):
            dev.render_aov_volume_to_host(camera(7, 5, 1, 12), medium=None, sample_first=1 << 30)
        with pytest.raises(rb.RtError, match="region 2"):
            dev.render_aov_volume_to_host(camera(7, 5, 1, 12), medium=media("three balls")["ball g=0.7"], volume=vol)
    dev.close()


@pytest.mark.gpu
def test_handle_state_is_left_alone():
    """A beauty frame and rt_last_timing of a handle are the same before and after the call."""
    host, camera, _ = scenes()["three balls"]
    cam = camera(24, 16, 2, 12)
    dev = rb.DeviceScene(host, device=0)
    before, _ = dev.render_to_host(cam)
    timing = bytes(dev.last_timing())
    with rb.Volume(GRIDS["16"]) as vol:
        dev.render_aov_volume_to_host(cam, medium=fog(0.3), volume=vol)
        dev.render_aov_volume_to_host(cam, medium=fog(0.3))
    assert bytes(dev.last_timing()) == timing
    after, _ = dev.render_to_host(cam)
    assert_same(after, before, "rt_render after rt_render_aov_volume")
    fresh = rb.DeviceScene(host, device=0)
    assert_same(fresh.render_to_host(cam)[0], before, "a fresh handle")
    fresh.close()
    dev.close()


ADAPT = dict(min_spp=4, batch_spp=4, max_spp=32)


@pytest.mark.gpu
def test_the_denoisers_take_the_buffers():
    """rt_denoise and rt_denoise_spp on the device's fog-aware AOVs: the bytes of denoise_reference and denoise_spp_reference on the restated
    AOVs."""
    scene = "three balls"
    host, camera, _ = scenes()[scene]
    medium, density = fog(0.3), GRIDS["2x3x5"]
    w, h, spp = 40, 27, 4
    cam = camera(w, h, spp, 12)
    dev = rb.DeviceScene(host, device=0)
    with rb.Volume(density) as vol:
        fb, _ = dev.render_volume_to_host(cam, medium=medium, volume=vol)
        aov, _ = dev.render_aov_volume_to_host(cam, medium=medium, volume=vol)
        restated = avr.aov(host, cam, medium=medium, density=density)
        same_aovs(aov, restated, "the AOVs")
        assert_same(rb.denoise_to_host(fb, aov, spp), dnr.reference(fb, restated, spp), "rt_denoise")
        afb, aspp, amom, _ = dev.render_volume_adaptive_to_host(cam, medium=medium, volume=vol, threshold=0.3, **ADAPT)
        assert len(np.unique(aspp)) >= 2
        assert_same(rb.denoise_spp_to_host(afb, aspp, amom, aov, ADAPT["min_spp"]), dsr.reference(afb, aspp, amom, restated, ADAPT["min_spp"]), "rt_denoise_spp")
    dev.close()


@pytest.mark.gpu
def test_cli_fog_denoise_files_are_the_python_path(test_config_text, tmp_path):
    """rtp_main --fog-denoise with and without a grid file and --fog-noise-target: <frame>.denoised holds the bytes of the Python path."""
    import torch
    lines = test_config_text.split("\n")
    lines[1] = str(tmp_path / "f_%d.png")
    text = "\n".join(lines).replace("../floor2.jpg", os.path.join(HERE, "golden", "floor.jpg"))
    host = rb.HostScene.from_config(text)
    info = host.info
    dev = rb.DeviceScene(host, device=0)
    cam = host.frame_camera_at(0.0)
    density = GRIDS["2x3x5"]
    with open(tmp_path / "grid.vol", "wb") as f:
        f.write(b"VOL1\n2 3 5\n" + np.asarray(density, "<f4").tobytes())
    box = (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0)
    medium = dict(sigma_t=0.4, albedo=0.9, g=0.3, box=box)
    with rb.Volume(density) as vol:
        for grid, noise in ((True, False), (False, True), (True, True), (False, False)):
            args = ["--lit", "--nee", "--light-tree", "--fog", "0.4:0.9:0.3", "--fog-box", ",".join(str(x) for x in box), "--fog-denoise"]
            args += ["--fog-grid", str(tmp_path / "grid.vol")] if grid else []
            args += ["--fog-noise-target", "0.3:4:4:32"] if noise else []
            out = subprocess.run([EXE, "--gpu", *args], input=text, capture_output=True, text=True, timeout=200)
            assert out.returncode == 0, out.stderr
            volume = vol if grid else None
            data = open(tmp_path / "f_0.png.denoised", "rb").read()
            os.remove(tmp_path / "f_0.png.denoised")
            if not noise:
                fb, _ = dev.render_volume_to_host(cam, nee=dict(select=1), medium=medium, volume=volume)
                aov, _ = dev.render_aov_volume_to_host(cam, medium=medium, volume=volume)
                want = rb.denoise_to_host(fb, aov, cam.samples_per_pixel)
                assert data == rb.binary_image_bytes(want, cam.image_width, cam.image_height, info.sqrt_spp), (grid, noise)
                continue
            fb, spp, mom, _ = dev.render_volume_adaptive_to_host(cam, nee=dict(select=1), threshold=0.3, **ADAPT, medium=medium, volume=volume)
            cam4 = host.frame_camera_at(0.0)
            cam4.samples_per_pixel = ADAPT["min_spp"]
            aov, _ = dev.render_aov_volume_to_host(cam4, medium=medium, volume=volume)
            want = rb.denoise_spp_to_host(fb, spp, mom, aov, ADAPT["min_spp"])
            d_fb, d_spp = torch.from_numpy(np.ascontiguousarray(want)).to("cuda:0"), torch.from_numpy(spp).to("cuda:0")
            rgb = torch.zeros(want.shape, dtype=torch.uint8, device="cuda:0")
            assert rb.amd_lib().rt_tonemap_spp(C.c_void_p(d_fb.data_ptr()), C.c_void_p(d_spp.data_ptr()), C.c_void_p(rgb.data_ptr()), spp.size, None) == 0
            torch.cuda.synchronize()
            assert data == np.array([cam.image_width, cam.image_height], dtype=np.int32).tobytes() + rgb.cpu().numpy().tobytes(), (grid, noise)
    dev.close()
