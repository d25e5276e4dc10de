"""Generates tests/golden/ref_geom.npz: inputs and the outputs of the REFERENCE'S OWN HEADERS (oracle/_ref/libref_geom.so, built
from /root/reference/include by oracle/Makefile `_ref` — build container only) for 1 024 primitive cases and two small scenes;
and tests/golden/ref_geom_digests.json: sha256 digests of that library's outputs on the full runs of tests/test_ref_geom.py
(ref_geom_cases.primitive_runs / scene_runs, whose inputs are regenerated from their seeds).
Data only: the fixtures hold numbers, no source.  Run:  python tests/golden/make_ref_geom_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_geom_cases as rg  # noqa: E402

ref = rg.Ref()
rng = np.random.default_rng(77)
c = rg.primitive_cases(rng, 1024)
out = {f"in_{k}": v for k, v in c.items()}
out.update({f"out_{k}": v for k, v in ref.primitives(c).items()})
for tag, (ns, npl) in (("s0", (150, 0)), ("s1", (60, 40))):
    sph, pl, types, o, d = rg.scene_cases(rng, ns, npl, 512)
    out.update({f"{tag}_sph": sph, f"{tag}_pl": pl, f"{tag}_types": types, f"{tag}_o": o, f"{tag}_d": d})
    out.update({f"{tag}_{k}": v for k, v in ref.scene(sph, pl, types, o, d).items()})
np.savez_compressed(os.path.join(HERE, "ref_geom.npz"), **out)
print("wrote", os.path.join(HERE, "ref_geom.npz"), os.path.getsize(os.path.join(HERE, "ref_geom.npz")), "bytes")

dig = {what: rg.digests(ref.primitives(c), keys) for what, c, keys in rg.primitive_runs()}
dig.update({what: rg.digests(ref.scene(*case)) for what, _, case in rg.scene_runs()})
with open(os.path.join(HERE, "ref_geom_digests.json"), "w") as f:
    json.dump(dig, f, indent=1)
    f.write("\n")
print("wrote", os.path.join(HERE, "ref_geom_digests.json"))
