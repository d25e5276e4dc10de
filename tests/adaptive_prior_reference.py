"""CPU restatement of the history-aware stopping rule (TEST INFRASTRUCTURE; include/rtp_amd.h "a history-aware stopping rule",
DESIGN.md §26).  rt_adaptive_prior: tests/cpu_native/adaptive_prior_ref.c, the header's arithmetic with the reprojection written out
again, built into a shared library (gcc -ffp-contract=off -fno-fast-math, like denoise_temporal_spp_reference.py) the first time it is
needed, in a temporary directory.  The judgement with a prior: numpy float32, one operation at a time; reference() and
from_radiances() take a prior and otherwise mirror adaptive_rule_reference.py."""
import ctypes as C

import numpy as np

import adaptive_rule_reference as arr
import cpu_ref
import test_adaptive as ta
from denoise_temporal_reference import history_bytes

F = np.float32
MIN_ALPHA = F(0.2)


def lib():
    l = cpu_ref.build("adaptive_prior_ref.c")
    l.adaptive_prior_reference.restype = C.c_int
    l.adaptive_prior_reference.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    return l


def prior(aov, aov_spp, cam, history_prev=None):
    """What rt_adaptive_prior computes for aov {"albedo", "normal", "depth", "hits", "prim"} at aov_spp samples per pixel, cam
    (rb.CameraData) and history_prev (a uint8 array of the header's layout, or None): (H, W, 2) float32 (ch, vh)."""
    w, h = cam.image_width, cam.image_height
    arrays = [np.ascontiguousarray(aov[k], dtype=t) for k, t in (("albedo", np.float32), ("normal", np.float32), ("depth", np.float32),
                                                                  ("hits", np.uint32), ("prim", np.int32))]
    assert arrays[0].shape == arrays[1].shape == (h, w, 3) and arrays[2].shape == arrays[3].shape == arrays[4].shape == (h, w)
    prev = None if history_prev is None else np.ascontiguousarray(history_prev, dtype=np.uint8)
    assert prev is None or prev.nbytes >= history_bytes(w, h)
    out = np.full((h, w, 2), np.nan, F)
    cam_bytes = C.create_string_buffer(bytes(cam), C.sizeof(cam))
    rc = lib().adaptive_prior_reference(cam_bytes, aov_spp, *[a.ctypes.data for a in arrays], None if prev is None else prev.ctypes.data,
                                        out.ctypes.data)
    assert rc == 0
    return out


def blended_variance(vm, nf, ch, vh):
    """ve: the variance rt_denoise_temporal_spp's blend will carry; a prior that is not (ch > 0, vh >= 0) — a NaN included — is none."""
    with np.errstate(all="ignore"):
        s = (ch + nf).astype(F)
        a = (nf / s).astype(F)
        a = np.where(a >= MIN_ALPHA, a, MIN_ALPHA).astype(F)
        b = (F(1) - a).astype(F)
        ve = (((b * b).astype(F) * vh).astype(F) + ((a * a).astype(F) * vm).astype(F)).astype(F)
        return np.where((ch > 0) & (vh >= 0), ve, vm).astype(F)


def variances(s1, s2, n, pr):
    """(mean, ve) of flat pixels with n samples, moments (s1, s2) and prior pr (pixels, 2)."""
    with np.errstate(all="ignore"):
        nf = F(n)
        mean = (s1 / nf).astype(F)
        var = np.fmax(F(0), ((s2 - s1 * mean).astype(F) / F(n - 1)).astype(F))
        vm = (var / nf).astype(F)
        return mean, blended_variance(vm, np.full(vm.shape, nf, F), pr[:, 0], pr[:, 1])


def goes_on(s1, s2, pr, n, batch, max_spp, t):
    """Rule 0 with a prior."""
    if n + batch > max_spp:
        return np.zeros(s1.shape, bool)
    t = F(t)
    if t == 0:
        return np.ones(s1.shape, bool)
    mean, ve = variances(s1, s2, n, pr)
    with np.errstate(all="ignore"):
        return ve > (t * t) * ((mean * mean).astype(F) + F(1e-4))


def noisy(s1, s2, pr, n, t):
    """noisy_p of rule 1 with a prior; a NaN in the pixel's own statistics compares false."""
    t = F(t)
    mean, ve = variances(s1, s2, n, pr)
    with np.errstate(all="ignore"):
        return ve > (t * t) * (mean + F(0.01)).astype(F)


def goes_on_near(s1, s2, pr, going_on, n, width, rows, shard, batch, max_spp, t):
    """One judgement of rule 1 with a prior for flat arrays of rows * width pixels: which pixels go on to the next round."""
    going_on = np.asarray(going_on, bool).ravel()
    if n + batch > max_spp:
        return np.zeros(going_on.shape, bool)
    if F(t) == 0:
        return going_on.copy()
    c = going_on & noisy(np.asarray(s1, F).ravel(), np.asarray(s2, F).ravel(), pr, n, t)
    return going_on & arr.window_any(c, width, rows, shard)


def judge(moments, pr, n, going_on, shard, rule, batch_spp, max_spp, threshold, **_):
    """rt_adaptive_judge_prior: moments (rows, width, 2), pr (rows, width, 2), going_on (rows, width) bool or None → (rows, width) bool."""
    rows, width = moments.shape[:2]
    s1, s2 = np.ascontiguousarray(moments[..., 0], F).ravel(), np.ascontiguousarray(moments[..., 1], F).ravel()
    flat = np.ascontiguousarray(pr, F).reshape(-1, 2)
    on = np.ones(rows * width, bool) if going_on is None else np.asarray(going_on, bool).ravel()
    if rule == 0:
        out = on & goes_on(s1, s2, flat, n, batch_spp, max_spp, threshold)
    else:
        out = goes_on_near(s1, s2, flat, on, n, width, rows, shard, batch_spp, max_spp, threshold)
    return out.reshape(rows, width)


def reference(rad, width, rows, shard, min_spp, batch, max_spp, t, rule, pr=None):
    """adaptive_rule_reference.reference with a prior pr (rows * width, 2) float32 (None: all zeros — no prior)."""
    assert rule in (0, 1) and rad.shape[0] == width * rows
    pr = np.zeros((width * rows, 2), F) if pr is None else np.ascontiguousarray(pr, F).reshape(width * rows, 2)
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
            on &= goes_on(s1, s2, pr, k, batch, max_spp, t)
        else:
            on = goes_on_near(s1, s2, pr, on, k, width, rows, shard, batch, max_spp, t)
        if not on.any():
            break
        for s in range(k, k + batch):
            s1 = np.where(on, (s1 + y[:, s]).astype(F), s1)
            s2 = np.where(on, (s2 + (y[:, s] * y[:, s]).astype(F)).astype(F), s2)
        n[on] += batch
    return n, s1, s2


def from_radiances(rad, shard, min_spp, batch_spp, max_spp, threshold, rule, pr=None):
    """adaptive_rule_reference.from_radiances with a prior pr (rows, W, 2): rad (rows, W, samples, 3) of the buffer's rows → (fb (rows,
    W, 3) float32 sums, spp (rows, W) int32, moments (rows, W, 2) float32)."""
    rows, w = rad.shape[:2]
    flat = rad.reshape(rows * w, rad.shape[2], 3)
    n, s1, s2 = reference(flat, w, rows, shard, min_spp, batch_spp, max_spp, threshold, rule, pr)
    fb = np.zeros((rows * w, 3), F)
    for s in range(int(n.max())):
        fb = np.where((s < n)[:, None], (fb + flat[:, s]).astype(F), fb)
    return fb.reshape(rows, w, 3), n.astype(np.int32).reshape(rows, w), np.stack([s1, s2], axis=1).astype(F).reshape(rows, w, 2)
