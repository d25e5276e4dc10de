"""CPU restatement of the stopping rules of rt_render_adaptive_rule / rt_render_lit_adaptive_rule (TEST INFRASTRUCTURE;
include/rtp_amd.h "the stopping rule of the adaptive calls").  numpy float32, one operation at a time, as
test_adaptive.reference restates rule 0 — which rule 0 here must equal exactly.  A buffer is rows x width pixels, row-major; `shard` is
None (the whole frame), an rb.Shard or a (band_rows, num_parts, part) triple, and rows are the compacted rows of that part."""
import numpy as np

import test_adaptive as ta

F = np.float32


def band_of(rows, shard):
    """Per buffer row, the index of its band in the buffer: rows r and r' are image neighbours iff |r - r'| == 1 and their bands are equal."""
    if shard is not None and not isinstance(shard, tuple):
        shard = (shard.band_rows, shard.num_parts, shard.part)
    if shard is None or shard[1] <= 1 or shard[0] <= 0:
        return np.zeros(rows, np.int64)
    return np.arange(rows) // shard[0]


def noisy(s1, s2, n, t):
    """noisy_p of rule 1; a NaN anywhere compares false."""
    t = F(t)
    with np.errstate(all="ignore"):
        mean = (s1 / F(n)).astype(F)
        var = np.fmax(F(0), ((s2 - s1 * mean).astype(F) / F(n - 1)).astype(F))
        return (var / F(n)).astype(F) > (t * t) * (mean + F(0.01)).astype(F)


def window_any(c, width, rows, shard):
    """c (rows * width) bool → per pixel: does c hold for some q of its window N(p) — p and its 8 neighbours, clipped to the buffer,
    a row above or below only within p's band."""
    c = np.asarray(c, bool).reshape(rows, width)
    band = band_of(rows, shard)
    across = c.copy()                                   # the row's own 3 columns
    across[:, 1:] |= c[:, :-1]
    across[:, :-1] |= c[:, 1:]
    out = across.copy()
    if rows > 1:
        same = band[1:] == band[:-1]                    # row r and row r + 1 are image neighbours
        out[1:] |= across[:-1] & same[:, None]
        out[:-1] |= across[1:] & same[:, None]
    return out.ravel()


def goes_on_near(s1, s2, going_on, n, width, rows, shard, batch, max_spp, t):
    """One judgement of rule 1 for flat arrays of rows * width pixels: which pixels go on to the next round."""
    going_on = np.asarray(going_on, bool).ravel()
    if n + batch > max_spp:
        return np.zeros(going_on.shape, bool)
    if F(t) == 0:
        return going_on.copy()
    c = going_on & noisy(np.asarray(s1, F).ravel(), np.asarray(s2, F).ravel(), n, t)
    return going_on & window_any(c, width, rows, shard)


def reference(rad, width, rows, shard, min_spp, batch, max_spp, t, rule):
    """rad (rows * width, samples >= min + R * batch, 3): per-sample radiances of the buffer's pixels → (counts, S1, S2) by the header's
    rounds under `rule` (0: the pixel's own relative error; 1: the neighbourhood rule)."""
    assert rule in (0, 1) and rad.shape[0] == width * rows
    y = ta.lum(rad)
    pixels = rad.shape[0]
    s1, s2 = np.zeros(pixels, F), np.zeros(pixels, F)
    for s in range(min_spp):
        s1 = (s1 + y[:, s]).astype(F)
        s2 = (s2 + (y[:, s] * y[:, s]).astype(F)).astype(F)
    n = np.full(pixels, min_spp, np.int32)
    on = np.ones(pixels, bool)
    for r in range(1, (max_spp - min_spp) // batch + 1):
        k = min_spp + (r - 1) * batch
        if rule == 0:
            on &= ta.goes_on(s1, s2, k, batch, max_spp, t)
        else:
            on = goes_on_near(s1, s2, on, k, width, rows, shard, batch, max_spp, t)
        if not on.any():
            break
        for s in range(k, k + batch):
            s1 = np.where(on, (s1 + y[:, s]).astype(F), s1)
            s2 = np.where(on, (s2 + (y[:, s] * y[:, s]).astype(F)).astype(F), s2)
        n[on] += batch
    return n, s1, s2


def from_radiances(rad, shard, min_spp, batch_spp, max_spp, threshold, rule):
    """lit_adaptive_reference.from_radiances under a rule: rad (rows, W, samples, 3) of the buffer's rows → (fb (rows, W, 3) float32
    sums, spp (rows, W) int32, moments (rows, W, 2) float32)."""
    rows, w = rad.shape[:2]
    flat = rad.reshape(rows * w, rad.shape[2], 3)
    n, s1, s2 = reference(flat, w, rows, shard, min_spp, batch_spp, max_spp, threshold, rule)
    fb = np.zeros((rows * w, 3), F)
    for s in range(int(n.max())):
        fb = np.where((s < n)[:, None], (fb + flat[:, s]).astype(F), fb)
    return fb.reshape(rows, w, 3), n.astype(np.int32).reshape(rows, w), np.stack([s1, s2], axis=1).astype(F).reshape(rows, w, 2)
