"""Device sweep of log_libm (ray-tracing-practice_amd/csrc/rt_device_math.h) on gfx950: every result bit for all 2^32 floats against the
host restatement of the stated algorithm (tests/cpu_native/log_sweep_ref.cpp, log_ref.h).  Needs the DEVELOPER build
(rt_debug_math_eval's kLog routine, csrc/rt_math_check.hip).  Not collected by the normal test run (the file name does not match
test_*.py): tests/test_medium.py runs it in a child process with RTP_AMD_LIB pointing at the developer library."""
import ctypes as C
import os
import subprocess
import time

import pytest
import torch

import rtp_bindings as rb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = 10                                                    # rtm::kLog (csrc/rt_math_check.h)
THREADS = min(16, len(os.sched_getaffinity(0)))
PER = 1 << 28                                               # inputs per chunk: 1 GB of words


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = tmp_path_factory.mktemp("lsr") / "liblsr.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", str(so),
                    os.path.join(ROOT, "tests", "cpu_native", "log_sweep_ref.cpp")], check=True)
    lib = C.CDLL(str(so))
    lib.lsr_compare.restype = C.c_uint64
    lib.lsr_compare.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
    return lib


def test_this_is_the_developer_library_with_the_log_routine():
    lib = rb.amd_lib()
    assert b"dev=1" in lib.rt_version_string() and hasattr(lib, "rt_debug_math_eval")


def test_log_libm_is_the_stated_algorithm_for_every_float(ref):
    lib = rb.amd_lib()
    lib.rt_get_last_error_string.restype = C.c_char_p
    lib.rt_debug_math_eval.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.rt_debug_math_eval.restype = C.c_int
    out = torch.empty(PER * 4, dtype=torch.uint8, device="cuda:0")
    host = torch.empty(PER * 4, dtype=torch.uint8, pin_memory=True)
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    bad, examples = 0, []
    for first in range(0, 1 << 32, PER):
        st = lib.rt_debug_math_eval(LOG, first, PER, 0, out.data_ptr(), stream)
        assert st == 0, lib.rt_get_last_error_string().decode()
        host.copy_(out)
        worst = (C.c_uint32 * 8)()
        b = ref.lsr_compare(first, PER, host.data_ptr(), THREADS, worst)
        bad += b
        examples += [f"{w:08x}" for w in worst[:min(b, 8)]]
    print(f"SWEEP log_libm: 2^32 inputs, {bad} differ, {time.perf_counter() - t0:.1f} s")
    assert bad == 0, f"log_libm: {bad} inputs differ from the host restatement, e.g. {examples[:8]}"
