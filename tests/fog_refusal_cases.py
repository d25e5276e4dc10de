"""The cases of tests/test_fog_refusals.py: every fog entry point of include/rtp_amd.h called with a NULL scene over the cross
product of its parameters' values, so that each call ends in a refusal — a parameter's, or at the latest the null scene's.  Nothing can be
enqueued, and no fake handle is read: a call looks at its handles' contents only behind the scene (the one place that compares two grids'
dimensions before it, source 2 with a volume and a heat grid, is left out, and no case has a sampler).

tests/golden/make_fog_refusals.py records (status, message) of every case from one build of the library; the test compares another build
with the record, byte for byte.  The order of `cases()` is part of the record: append, never reorder."""
import ctypes as C
import hashlib
import itertools

import rtp_bindings as rb

INVALID = 1
HANDLE = C.c_void_p(1 << 32)          # a non-null handle or device address that is never read
BOX = (0, 0, 0, 1, 1, 1)


def _short_medium():
    m = rb.medium_params(sigma_t=1.0, box=BOX)
    m.struct_bytes = 4
    return m


def values():
    """name → {label: ctypes argument} of every parameter the cases vary (built once: the structures outlive the calls)."""
    keep = {
        "lit": {"none": None, "mis2": rb.lit_params(nee=dict(mis=2))},
        "medium": {"none": None, "box1": rb.medium_params(sigma_t=1.0, box=BOX), "box0": rb.medium_params(sigma_t=0.0, box=BOX),
                   "boxneg": rb.medium_params(sigma_t=-1.0, box=BOX), "ball": rb.medium_params(sigma_t=1.0, ball=(0, 0, 0, 1)), "short": _short_medium()},
        "tint": {"none": None, "111": rb.chroma_params(tint=(1, 1, 1)), "tinted": rb.chroma_params(tint=(1, 0.5, 0.25)), "neg": rb.chroma_params(tint=(1, -1, 1))},
        "glow": {"none": None, "r0": rb.glow_params(radiance=0.0), "r1s0": rb.glow_params(radiance=1.0, source=0), "r1s1": rb.glow_params(radiance=1.0, source=1),
                 "r1s2": rb.glow_params(radiance=1.0, source=2), "r1s3": rb.glow_params(radiance=1.0, source=3), "rneg": rb.glow_params(radiance=-1.0)},
        "sample": {"none": None, "s0": rb.glow_sample_params(sample=0), "s1": rb.glow_sample_params(sample=1), "s2": rb.glow_sample_params(sample=2),
                   "mis2": rb.glow_sample_params(sample=1, mis=2)},
    }
    out = {k: {label: (C.byref(v) if v is not None else None) for label, v in d.items()} for k, d in keep.items()}
    out["volume"] = {"none": None, "handle": HANDLE}
    out["heat"] = {"none": None, "handle": HANDLE}
    out["_keep"] = keep
    return out


# the parameters of each rung's calls, in the order of the C arguments between the camera and the rest (the sampler is NULL throughout)
RUNG_PARAMS = {
    "medium": ("lit", "medium"),
    "volume": ("lit", "medium", "volume"),
    "chroma": ("lit", "medium", "volume", "tint"),
    "glow": ("lit", "medium", "volume", "glow", "heat"),
    "glow_sampled": ("lit", "medium", "volume", "glow", "heat", "sample"),
}
# the probes' columns behind n, in the order of the C arguments (ijs first)
BASE_COLUMNS = ("ijs", "radiance", "rays", "medium_events", "final_seed", "final_nee_seed", "final_env_seed", "final_medium_seed")
RUNG_COLUMNS = {"medium": BASE_COLUMNS, "volume": BASE_COLUMNS + ("cells",), "chroma": BASE_COLUMNS + ("cells",),
                "glow": BASE_COLUMNS + ("cells", "glow_length"), "glow_sampled": BASE_COLUMNS + ("cells", "glow_length", "glow_samples")}
AOV_VARIANTS = ("buffers", "null_buffers", "all_null_buffers")
ADAPTIVE_VARIANTS = ("fine", "bad_params", "bad_rule", "null_spp")


def _combos(rung):
    """The label tuples of a rung's parameters, without what would read a fake handle (source 2 with a volume and a heat grid)."""
    names = RUNG_PARAMS[rung]
    labels = {"lit": ("none", "mis2"), "medium": ("none", "box1", "box0", "boxneg", "ball", "short"), "volume": ("none", "handle"),
              "tint": ("none", "111", "tinted", "neg"), "glow": ("none", "r0", "r1s0", "r1s1", "r1s2", "r1s3", "rneg"), "heat": ("none", "handle"),
              "sample": ("none", "s0", "s1", "s2", "mis2")}
    for combo in itertools.product(*(labels[n] for n in names)):
        c = dict(zip(names, combo))
        if c.get("glow") == "r1s2" and c["volume"] == "handle" and c["heat"] == "handle":
            continue
        yield c


def cases():
    """Every case as (entry point, rung, {parameter: label}, variant), in the record's order."""
    out = []
    for rung in RUNG_PARAMS:
        for c in _combos(rung):
            out.append((f"rt_render_{rung}", rung, c, "frame"))
    for c in _combos("volume"):
        out += [("rt_render_aov_volume", "volume", c, v) for v in AOV_VARIANTS]
        out += [("rt_render_volume_adaptive", "volume", c, v) for v in ADAPTIVE_VARIANTS]
    for rung in RUNG_PARAMS:
        for c in _combos(rung):
            out += [(f"rt_trace_samples_{rung}", rung, c, v) for v in ("n=1", "n=-1") + tuple("null_" + col for col in RUNG_COLUMNS[rung])]
    return out


def case_id(case):
    entry, _, combo, variant = case
    return f"{entry}[{','.join(f'{k}={v}' for k, v in combo.items())};{variant}]"


def ids_digest(all_cases):
    """A digest of the cases' ids in order: the record is for exactly this list."""
    return hashlib.sha256("\n".join(case_id(c) for c in all_cases).encode()).hexdigest()


class Caller:
    """Calls a case on lib with a NULL scene and returns (status, message)."""

    def __init__(self, lib):
        self.lib = lib
        lib.rt_get_last_error_string.restype = C.c_char_p
        self.v = values()
        self.cam = rb.rtiow_camera(8, 4, 2)
        self.ijs = (C.c_int32 * 3)(0, 0, 0)
        self.f3, self.f1 = (C.c_float * 3)(), (C.c_float * 1)()
        self.i1 = [(C.c_int32 * 1)() for _ in range(4)]
        self.u1 = [(C.c_uint32 * 1)() for _ in range(4)]
        self.columns = {"ijs": self.ijs, "radiance": self.f3, "rays": self.i1[0], "medium_events": self.i1[1], "final_seed": self.u1[0],
                        "final_nee_seed": self.u1[1], "final_env_seed": self.u1[2], "final_medium_seed": self.u1[3], "cells": self.i1[2],
                        "glow_length": self.f1, "glow_samples": self.i1[3]}
        self.aov = rb.AovBuffers()
        self.aov.albedo_sum = self.aov.hit_count = HANDLE.value
        self.aov_all_null = rb.AovBuffers()
        self.adaptive = rb.adaptive_params()
        self.adaptive_bad = rb.adaptive_params(min_spp=1)
        self.stop_bad = rb.stop_params(rule=2)

    def __call__(self, case):
        entry, rung, combo, variant = case
        head = [None, C.byref(self.cam)] + [self.v[k][label] for k, label in combo.items()]
        if rung == "glow_sampled":
            head.append(None)          # the sampler
        if variant == "frame":
            args = head + [None, 0, HANDLE, None, 1, None]
        elif variant in AOV_VARIANTS:
            buffers = {"buffers": C.byref(self.aov), "null_buffers": None, "all_null_buffers": C.byref(self.aov_all_null)}[variant]
            args = head + [None, 0, buffers, HANDLE, None, 1, None]
        elif variant in ADAPTIVE_VARIANTS:
            params = C.byref(self.adaptive_bad if variant == "bad_params" else self.adaptive)
            stop = C.byref(self.stop_bad) if variant == "bad_rule" else None
            args = head + [params, stop, None, None, 0, HANDLE, None if variant == "null_spp" else HANDLE, None, None, 1, None]
        else:
            n = -1 if variant == "n=-1" else 1
            args = head + [n] + [None if variant == "null_" + col else self.columns[col] for col in RUNG_COLUMNS[rung]]
        status = getattr(self.lib, entry)(*args)
        return status, self.lib.rt_get_last_error_string().decode()
