"""rt_render_fog_adaptive on tests/lit_fuzz.py's glossy twins under lit_fuzz.fuzz_fog: per trial and per family — chroma,
glow, glow_sampled — the trial's first frame call of that family, at test_lit_fuzz.FRAME's size with min 3, batch 2, max 9.  On the GPU
threshold 0 is the family's frame call at 9 samples, and a mid threshold gives per-pixel parity with the frame call at each pixel's own
count; without a GPU the restatements show that the mid threshold spreads the pixels over the levels."""
import functools

import numpy as np
import pytest

import chroma_reference as cr
import glow_reference as gr
import glow_sample_reference as gs
import lit_adaptive_reference as lar
import lit_fuzz as lf
from test_lit import assert_same
from test_lit_fuzz import FRAME
from test_lit_fuzz_fog import Fog

FAMILIES = ("chroma", "glow", "glow_sampled")
REFERENCE = {"chroma": cr, "glow": gr, "glow_sampled": gs}
SPP = dict(min_spp=3, batch_spp=2, max_spp=9)
LEVELS = [3, 5, 7, 9]
# one mid threshold per family, chosen by a sweep on the restatements (tools/fog_adaptive_sweep.py --fuzz) so that the condition of
# test_mid_thresholds_spread_the_levels holds; DESIGN.md §40 has the counts
MID = {"chroma": 0.07, "glow": 0.175, "glow_sampled": 0.275}


def call_of(trial, family):
    """The trial's first frame call of the family, without its shard."""
    return next(c for c in lf.fog_frame_calls(trial) if c.family == family)._replace(shard=None)


@functools.lru_cache(maxsize=None)
def level_counts(trial, family, threshold):
    """Pixels per level of the call's frame at a threshold, on the family's restatement."""
    w, h, _ = FRAME
    c = lf.gloss_case(trial)
    call = call_of(trial, family)
    rad = lar.radiances(c.host, c.camera(w, h, 1, 50), SPP["max_spp"], tracer=REFERENCE[family].trace, **lf.fog_reference_keywords(call, w, h, 1, 50))
    spp = lar.from_radiances(rad, threshold=threshold, **SPP)[1]
    return tuple(int((spp == n).sum()) for n in LEVELS)


@pytest.mark.parametrize("family", FAMILIES)
def test_mid_thresholds_spread_the_levels(family):
    """With the family's mid threshold, in at least 5 of the 8 trials at least two levels hold at least 5 pixels each."""
    counts = {t: level_counts(t, family, MID[family]) for t in lf.TRIALS}
    print(f"{family} t={MID[family]}: pixels per level {dict(zip(LEVELS, zip(*counts.values())))} over the trials {list(counts)}")
    spread = [t for t, c in counts.items() if sum(n >= 5 for n in c) >= 2]
    assert len(spread) >= 5, counts


@pytest.mark.gpu
@pytest.mark.parametrize("trial", lf.TRIALS)
def test_threshold_zero_and_per_pixel_parity(trial):
    fog = Fog(trial)
    w, h, _ = FRAME
    cam = fog.c.camera(w, h, 1, 50)
    try:
        for family in FAMILIES:
            call = call_of(trial, family)
            kw = fog.keywords(call, w, h, 1, 50)
            frame = getattr(fog.dev, f"render_{family}_to_host")

            def uniform(n):          # (the closing camera of a shutter carries the call's own sample count)
                return frame(fog.c.camera(w, h, n, 50), **fog.keywords(call, w, h, n, 50))[0]
            fb, spp, _, t = fog.dev.render_fog_adaptive_to_host(cam, threshold=0.0, **SPP, **kw)
            assert (spp == 9).all() and t.trace_launches == 4
            assert_same(fb, uniform(9), f"{fog.c.name} {family}: threshold 0 = the frame call at 9")
            fb, spp, _, _ = fog.dev.render_fog_adaptive_to_host(cam, threshold=MID[family], **SPP, **kw)
            assert tuple(int((spp == n).sum()) for n in LEVELS) == level_counts(trial, family, MID[family]), (fog.c.name, family)
            for n in np.unique(spp).tolist():
                sel = spp == n
                assert_same(fb[sel], uniform(n)[sel], f"{fog.c.name} {family}: pixels with {n} samples")
    finally:
        fog.close()
