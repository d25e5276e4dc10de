"""One builder for the CPU reference libraries under tests/cpu_native/ (TEST INFRASTRUCTURE).  The flag set is a parity decision: a
reference has to round like the oracle — no contraction into fused multiply-adds, no fast-math — so every reference is built here."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-w"]


@functools.lru_cache(maxsize=None)
def build(source, *more):
    """tests/cpu_native/<source>, with `more` (paths from the repository's root, e.g. "oracle/rt_oracle.c"), as a ctypes.CDLL: built
    once per process into a fresh temporary directory.  The caller declares the argtypes of what it calls."""
    name = os.path.splitext(source)[0]
    out = os.path.join(tempfile.mkdtemp(prefix=name + "_"), f"lib{name}.so")
    subprocess.run(["gcc", *FLAGS, "-o", out, os.path.join(HERE, "cpu_native", source), *(os.path.join(ROOT, m) for m in more),
                    "-lm", "-lpthread"], check=True)
    return C.CDLL(out)
