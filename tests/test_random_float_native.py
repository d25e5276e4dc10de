"""rtd::random_float's form (csrc/rt_device_math.h: a multiplication by 2^-32) against the reference's own expression,
wang_hash(seed) / 4294967296.0f, bit for bit: tests/cpu_native/random_float_ref.cpp, built as the host code is built and once more
under AddressSanitizer + UBSan, each a program of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_native", "random_float_ref.cpp")


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["host-flags", "sanitizers"])
def test_random_float_is_the_references_division(tmp_path, flags):
    exe = str(tmp_path / "random_float_ref")
    subprocess.run(["g++", "-std=c++17", *flags, "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all ok" in out.stdout and " 0 differ" in out.stdout, out.stdout
    assert "exactly 1.0f: 128 of 128" in out.stdout, out.stdout
