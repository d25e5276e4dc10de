"""Checks that need the DEVELOPER build of the render library (librtp_amd_dev.so, `make -C ray-tracing-practice_amd dev`):
the rt_debug_* entry points and the tripwire.  Not collected by the normal test run (the file name does not match test_*.py):
tests/test_gpu_parity.py::test_developer_build_checks_and_retired_experiments runs it in one child process with RTP_AMD_LIB
pointing at the developer library."""
import ctypes as C

import numpy as np
import pytest

import oracle_bindings as ob
import rtp_bindings as rb

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_frame(got, want, what):
    same = (bits(got) == bits(want)).all(axis=-1)
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} pixels differ, max abs diff {np.abs(got - want).max()}"


def test_this_is_the_developer_library():
    v = rb.amd_lib().rt_version_string()
    assert b"dev=1" in v and b"parity=1" in v


def test_retired_experiments_are_refused_here_too():
    """RT_KERNEL_WAVEFRONT and rt_config.wide_nodes = 1 were retired: the developer build refuses them as the shipped one does."""
    host = rb.HostScene.rtiow()
    for kw in (dict(kernel=rb.KERNEL_WAVEFRONT), dict(wide_nodes=1)):
        with pytest.raises(RuntimeError, match="retired"):
            rb.DeviceScene(host, device=0, honour_env=False, **kw).render_to_host(rb.rtiow_camera(32, 20, 2, 8))


def test_fast_reciprocal_and_sqrt_match_ieee_for_every_float():
    """rt_device_math.h recip() / sqrt_cr(): a hardware estimate plus one fused correction inside an exponent fence, the
    compiler's correctly rounded sequence outside it.  Proof by exhaustion on the device that renders: all 2^32 binary32
    inputs, every result bit compared with 1.0f / x and sqrtf(x) (the reference's own operations, include/vec3.h:97,105)."""
    import ctypes as C
    lib = rb.amd_lib()
    out = (C.c_uint64 * 3)()
    lib.rt_debug_check_fast_math.argtypes = [C.POINTER(C.c_uint64)]
    lib.rt_debug_check_fast_math.restype = C.c_int
    assert lib.rt_debug_check_fast_math(out) == 0
    assert out[2] == 2 ** 32
    assert out[0] == 0, "recip() differs from 1.0f / x for %d inputs" % out[0]
    assert out[1] == 0, "sqrt_cr() differs from sqrtf(x) for %d inputs" % out[1]


def test_sphere_roots_from_one_reciprocal_match_the_plain_divisions():
    """test_sphere's root selection (both fp64 quotients from one v_rcp_f64 + Newton steps, no scaling instructions) against
    the reference's form with the compiler's correctly rounded divisions, on 2^32 SAMPLED operand sets (not an exhaustive proof: four
    operands span 2^128 combinations): raw random bit patterns
    (all exponents, inf, NaN, denormals) and scene-scale operands alike — same acceptance, same accepted root, bit for bit."""
    import ctypes as C
    lib = rb.amd_lib()
    out = (C.c_uint64 * 3)()
    lib.rt_debug_check_sphere_roots.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    lib.rt_debug_check_sphere_roots.restype = C.c_int
    assert lib.rt_debug_check_sphere_roots(2 ** 32, out) == 0
    assert out[2] == 2 ** 32
    assert out[1] > 2 ** 26          # accepted roots are really being produced and compared
    assert out[0] == 0, "%d operand sets differ" % out[0]


def test_tripwire_turns_a_scheduling_fault_into_an_error():
    """The developer build checks, at every step-kind vote, that each live lane is walking, stuck at a leaf or finished, and counts
    main-loop rounds without progress (rt_kernel.hip.inc, RTP_TRIPWIRE).  rt_debug_trip_test injects the fault round 3's hang
    came from — a lane at a leaf with its park slot empty: the launch ENDS, rt_last_timing reports RT_ERR_HIP with the tripwire's
    code, and the next frame of the same handle is the oracle's again."""
    lib = rb.amd_lib()
    lib.rt_debug_trip_test.argtypes = [C.c_void_p, C.c_uint32]
    host = rb.HostScene.rtiow()
    dev = rb.DeviceScene(host, device=0, honour_env=False, traversal=rb.TRAVERSAL_GUARDED, guard_keep=1)
    cam = rb.rtiow_camera(160, 90, 8, 50)
    want = ob.render(host, cam, threads=8)
    fb, t = dev.render_to_host(cam)
    assert t.guarded == 1
    assert_same_frame(fb, want, "developer build, tripwire armed, no fault")
    assert lib.rt_debug_trip_test(dev._h, 1) == 0
    with pytest.raises(rb.RtError, match="aborted.*1414678785"):          # 0x54524901: kTripPartition
        dev.render_to_host(cam)
    assert lib.rt_debug_trip_test(dev._h, 0) == 0
    fb, t = dev.render_to_host(cam)
    assert_same_frame(fb, want, "frame after the tripped one")
