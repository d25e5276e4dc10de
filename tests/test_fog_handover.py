"""The hand-overs of the fog calls: a call that has become a lower rung's refuses as that rung's call.  Refusals only —
every call here is refused before anything is enqueued, so no kernel runs: an 8 x 4 camera at 2 spp, a 1 x 1 x 1 volume, a real scene.

For each rung of the ladder and each defect (a null framebuffer, sample_first = -1, and in the probes an ijs row outside the image), the
upper call's status and full message are those of the call it hands to with the same defect; with the hand-over not taken, the message
carries the upper call's own name.  One rung is a hand-over in the probes only: rt_render_medium without a medium takes rt_render_lit's
light and stays rt_render_medium by name, while rt_trace_samples_medium calls rt_trace_samples_lit."""
import ctypes as C

import numpy as np
import pytest

import rtp_bindings as rb

INVALID = 1
BOX = (-1, -1, -1, 1, 1, 1)
# the arguments of each call between lit and the rest, and the probes' columns behind ijs (f: float32 x 3, g: float32, i: int32, u: uint32)
ARGS = {"lit": (), "medium": ("medium",), "volume": ("medium", "volume"), "chroma": ("medium", "volume", "tint"),
        "glow": ("medium", "volume", "glow", "heat"), "glow_sampled": ("medium", "volume", "glow", "heat", "sample", "sampler")}
COLUMNS = {"lit": "fiuuu", "medium": "fiiuuuu", "volume": "fiiuuuui", "chroma": "fiiuuuui", "glow": "fiiuuuuig", "glow_sampled": "fiiuuuuigi"}


@pytest.fixture(scope="module")
def world():
    """The scene, the grids and the samplers every case shares."""
    import torch
    from test_lit import MAT_LAMBERTIAN, material
    rb.amd_lib().rt_get_last_error_string.restype = C.c_char_p
    host = rb.HostScene.from_arrays(np.array([[0, 1000, 0, 0.5, 0]], np.float32), np.zeros((0, 11), np.float32), [material(MAT_LAMBERTIAN)])
    dev = rb.DeviceScene(host, device=0)
    full, empty = rb.Volume(np.ones((1, 1, 1), np.float32)), rb.Volume(np.zeros((1, 1, 1), np.float32))
    sampler, sampler_empty = rb.GlowSampler(full, source=0), rb.GlowSampler(empty, source=1)
    assert sampler.table()[0] == 1 and sampler_empty.table()[0] == 0
    w = dict(dev=dev, cam=rb.make_camera(8, 4, 40.0, (0, 0, 5), (0, 0, 0), (0.1, 0.2, 0.3), 2, 4), fb=torch.zeros((4, 8, 3), dtype=torch.float32, device="cuda:0"),
             full=full, empty=empty, sampler=sampler, sampler_empty=sampler_empty)
    yield w
    for k in ("sampler", "sampler_empty", "full", "empty", "dev"):
        w[k].close()


def _head(w, rung, given):
    """The C arguments of a rung's call up to the rung's last parameter: scene, camera, lit (NULL), then `given` by name (absent: NULL)."""
    make = {"medium": lambda v: C.byref(rb.medium_params(**v)), "volume": rb._volume_handle, "heat": rb._volume_handle, "tint": rb._chroma_struct,
            "glow": rb._glow_struct, "sample": rb._glow_sample_struct, "sampler": rb._sampler_handle}
    assert set(given) <= set(ARGS[rung]), (rung, given)
    return [w["dev"]._h, C.byref(w["cam"]), None] + [make[k](given[k]) if given.get(k) is not None else None for k in ARGS[rung]]


def frame(w, rung, given, fb=True, sample_first=0):
    """(status, message) of rt_render_<rung>."""
    lib = rb.amd_lib()
    st = getattr(lib, f"rt_render_{rung}")(*_head(w, rung, given), None, sample_first, C.c_void_p(w["fb"].data_ptr() if fb else 0), None, 1, None)
    return st, lib.rt_get_last_error_string().decode()


def probe(w, rung, given, ijs=(8, 0, 0)):
    """(status, message) of rt_trace_samples_<rung> on one sample, by default one outside the image."""
    lib = rb.amd_lib()
    ijs = (C.c_int32 * 3)(*ijs)
    kinds = {"f": C.c_float * 3, "g": C.c_float * 1, "i": C.c_int32 * 1, "u": C.c_uint32 * 1}
    st = getattr(lib, f"rt_trace_samples_{rung}")(*_head(w, rung, given), 1, ijs, *(kinds[c]() for c in COLUMNS[rung]))
    return st, lib.rt_get_last_error_string().decode()


def rungs(w):
    """name → (upper rung, its arguments, lower rung, its arguments, frames hand over by name)."""
    m1, m0, m2 = dict(sigma_t=1.0, box=BOX), dict(sigma_t=0.0, box=BOX), dict(sigma_t=2.0, box=BOX)
    lit1, lit1s1 = dict(radiance=1.0), dict(radiance=1.0, source=1)
    return {
        "sampled glow to glow: no sample": ("glow_sampled", dict(medium=m1, volume=w["full"], glow=lit1), "glow", dict(medium=m1, volume=w["full"], glow=lit1), True),
        "sampled glow to glow: an empty sampler": ("glow_sampled", dict(medium=m1, volume=w["empty"], glow=lit1s1, sample="mis", sampler=w["sampler_empty"]),
                                                   "glow", dict(medium=m1, volume=w["empty"], glow=lit1s1), True),
        "glow to volume: dark": ("glow", dict(medium=m1, volume=w["full"], glow=dict(radiance=0.0)), "volume", dict(medium=m1, volume=w["full"]), True),
        "volume to medium: no volume": ("volume", dict(medium=m1), "medium", dict(medium=m1), True),
        "medium to lit: sigma_t 0": ("medium", dict(medium=m0), "lit", {}, False),
        "chroma to volume: equal tints": ("chroma", dict(medium=m1, volume=w["full"], tint=(2.0, 2.0, 2.0)), "volume", dict(medium=m2, volume=w["full"]), True),
    }


RUNGS = ("sampled glow to glow: no sample", "sampled glow to glow: an empty sampler", "glow to volume: dark", "volume to medium: no volume",
         "medium to lit: sigma_t 0", "chroma to volume: equal tints")


@pytest.mark.gpu
@pytest.mark.parametrize("rung", RUNGS)
def test_a_handed_over_call_refuses_as_the_call_it_became(world, rung):
    upper, up_args, lower, low_args, frames_by_name = rungs(world)[rung]
    # the probes: an ijs row outside the image
    got, want = probe(world, upper, up_args), probe(world, lower, low_args)
    assert got == want and got[0] == INVALID, (got, want)
    assert got[1] == f"rt_trace_samples_{lower}: sample coordinate out of range", got
    # the frames: a null framebuffer, sample_first = -1
    for defect, word in ((dict(fb=False), "null framebuffer"), (dict(sample_first=-1), "sample_first is negative")):
        got, want = frame(world, upper, up_args, **defect), frame(world, lower, low_args, **defect)
        assert got[0] == want[0] == INVALID and word in got[1], (defect, got, want)
        if frames_by_name:
            assert got == want, (defect, got, want)
            assert "sample_first" not in defect or got[1] == f"rt_render_{lower}: {word}", got
        else:          # (the light is the lower call's, the name stays the upper's)
            assert "sample_first" not in defect or got[1] == f"rt_render_{upper}: {word}", got


@pytest.mark.gpu
def test_a_call_that_keeps_its_rung_refuses_under_its_own_name(world):
    m1 = dict(sigma_t=1.0, box=BOX)
    kept = {"glow_sampled": dict(medium=m1, volume=world["full"], glow=dict(radiance=1.0), sample="mis", sampler=world["sampler"]),
            "glow": dict(medium=m1, volume=world["full"], glow=dict(radiance=1.0)), "chroma": dict(medium=m1, volume=world["full"], tint=(1.0, 0.5, 0.25)),
            "volume": dict(medium=m1, volume=world["full"]), "medium": dict(medium=m1)}
    for rung, args in kept.items():
        assert probe(world, rung, args) == (INVALID, f"rt_trace_samples_{rung}: sample coordinate out of range"), rung
        assert frame(world, rung, args, sample_first=-1) == (INVALID, f"rt_render_{rung}: sample_first is negative"), rung
        st, msg = frame(world, rung, args, fb=False)
        assert st == INVALID and "null framebuffer" in msg, (rung, st, msg)
