"""CPU checks of ray-tracing-practice_amd/csrc/rt_device_math.h (the kernel's arithmetic),
compiled for the host: the float shortcuts it takes are exact, and its expf/pow5 agree with the
host libm the reference calls.  The same routines compiled for gfx950 are swept on the device by
tests/dev_math_checks.py (the GPU tests at the end of this file), and a frame whose Beer-Lambert
arguments reach exp's positive range is checked against the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "%s/ray-tracing-practice_amd/csrc/rt_math_check.h"
#include <cmath>
extern "C" {
// returns number of mismatches over a strided sweep of float bit patterns
long sweep_exp(unsigned lo, unsigned hi, unsigned stride) {
    long bad = 0;
    for (unsigned long u = lo; u <= hi; u += stride) { unsigned b = (unsigned)u; float x; memcpy(&x, &b, 4);
        float a = rtd::exp_libm(x), g = expf(x); if (memcmp(&a, &g, 4)) bad++; }
    return bad;
}
static float (*volatile libm_powf5)(float, float) = powf;      // the library routine, not a compiler expansion
long sweep_pow5(unsigned stride, long *total) {
    long bad = 0, n = 0;
    for (unsigned long u = 0; u <= 0x40000000ul; u += stride) { unsigned b = (unsigned)u; float x; memcpy(&x, &b, 4);
        float a = rtd::pow5(x), g = libm_powf5(x, 5.0f); if (memcmp(&a, &g, 4)) bad++; n++; }
    *total = n; return bad;
}
// schlick_exceeds (the kernel's bracketed comparison) against reflectance with the library's powf, draws placed at and around the value
long sweep_schlick(unsigned stride, long *total) {
    long bad = 0, n = 0;
    unsigned h = 99u;
    for (int neg = 0; neg < 2; ++neg)
    for (unsigned long u = 0; u <= 0x3F800000ul; u += stride) { unsigned b = (unsigned)u | (neg ? 0x80000000u : 0u); float cosine; memcpy(&cosine, &b, 4);
        h = rtd::wang_hash(h + b);
        const float r0 = (float)(h & 0xffffu) * (0.9f / 65536.0f), x = 1.0f - cosine;
        const float ref = r0 + (1.0f - r0) * libm_powf5(x, 5.0f);
        unsigned rb; memcpy(&rb, &ref, 4);
        for (int d = -3; d <= 3; ++d) { unsigned q = rb + (unsigned)d; float rnd; memcpy(&rnd, &q, 4);
            if (rtd::schlick_exceeds(cosine, r0, rnd) != (ref > rnd)) bad++; n++; }
        const float rnd = (float)rtd::wang_hash(h) * 2.3283064365386962890625e-10f;
        if (rtd::schlick_exceeds(cosine, r0, rnd) != (ref > rnd)) bad++; n++; }
    *total = n; return bad;
}
// every result bit, NaN results included (acos_libm returns the libm's +qNaN for |x| > 1, and quietened NaN inputs)
static int same_bits(float a, float g) { return !memcmp(&a, &g, 4); }
static float (*volatile libm_acosf)(float) = acosf;
long sweep_acos(unsigned stride, long *total) {
    long bad = 0, n = 0;
    for (unsigned long u = 0; u <= 0xFFFFFFFFul; u += stride) { unsigned b = (unsigned)u; float x; memcpy(&x, &b, 4);
        if (!same_bits(rtd::acos_libm(x), libm_acosf(x))) bad++; n++; }
    *total = n; return bad;
}
long sweep_atan(unsigned stride, long *total) {
    long bad = 0, n = 0;
    for (unsigned long u = 0; u <= 0xFFFFFFFFul; u += stride) { unsigned b = (unsigned)u; float x; memcpy(&x, &b, 4);
        if (!same_bits(rtd::atan_libm(x), atanf(x))) bad++; n++; }
    *total = n; return bad;
}
long sweep_atan2(long pairs) {
    long bad = 0;
    unsigned h = 0x1234567u;
    for (long i = 0; i < pairs; ++i) { h = rtd::wang_hash(h + (unsigned)i); const unsigned a = h; h = rtd::wang_hash(h ^ 0x9e3779b9u); const unsigned b = h;
        float y, x; memcpy(&y, &a, 4); memcpy(&x, &b, 4);
        if (i & 1) { y = (float)((int)a) * 4.6566e-10f; x = (float)((int)b) * 4.6566e-10f; if (i & 2) y *= 1e-3f; if (i & 4) x *= 1e-4f; }
        if (i %% 1000 == 7) x = (i & 8) ? 1.0f : 0.0f;
        if (i %% 1000 == 9) y = (i & 8) ? -0.0f : 0.0f;
        if (!same_bits(rtd::atan2_libm(y, x), atan2f(y, x))) bad++; }
    return bad;
}
// the structured pairs of the device sweep (rt_math_check.h: specials x specials, then the unit circle), here on the host
long sweep_atan2_structured(long *total) {
    long bad = 0, n = 0;
    for (unsigned i = 0; i < rtm::kSpecialPairs + rtm::kCirclePairs; ++i) { float y, x; rtm::atan2_pair(i, y, x);
        if (!same_bits(rtd::atan2_libm(y, x), atan2f(y, x))) bad++; n++; }
    *total = n; return bad;
}
// single-operation-through-double identities the kernel relies on
long sweep_identities(unsigned stride) {
    long bad = 0;
    for (unsigned long u = 1; u < 0x7F800000ul; u += stride) { unsigned b = (unsigned)u; float x; memcpy(&x, &b, 4);
        float r1 = (float)(1.0 / (double)x), r2 = rtd::recip(x); if (memcmp(&r1, &r2, 4)) bad++;
        float y = x * 0.37f;
        float s1 = (float)(1.0 - (double)y), s2 = 1.0f - y; if (memcmp(&s1, &s2, 4)) bad++;
        float q1 = (float)((double)y / (double)x), q2 = y / x; if (memcmp(&q1, &q2, 4)) bad++;
        float h1 = (float)((double)y - 0.5), h2 = y - 0.5f; if (memcmp(&h1, &h2, 4)) bad++;
        float p1 = powf(y, 2), p2 = y * y; if (p1 == p1 && memcmp(&p1, &p2, 4)) bad++;
    }
    return bad;
}
// ELLIPSE interior test: the reference writes powf(x, 2) with a literal exponent (include/plane.h:41); the kernel
// evaluates x * x.  `literal`: the call as the reference writes it, which gcc/clang/nvcc at -O1 and above expand to
// x * x (both of the reference's build files use -O3; the oracle is built with -O2); `libm`: the library routine
// itself, reached through a volatile pointer — what an unoptimised build would call.
// Inputs: (a) every x whose exact square is a TIE between two floats (x = k * 2^e, k odd, 2^24 < k^2 < 2^25);
// (b) a strided sweep of [2^-30, 8) and its negatives.
static float (*volatile libm_powf)(float, float) = powf;
long sweep_square(unsigned stride, int use_libm, long *total) {
    long bad = 0, n = 0;
    for (int k = 4097; k <= 5791; k += 2)
        for (int e = -40; e <= 20; ++e)
            for (int sgn = 0; sgn < 2; ++sgn) {
                const float x = ldexpf((float)(sgn ? -k : k), e);
                const float p1 = use_libm ? libm_powf(x, 2) : powf(x, 2), p2 = x * x; if (memcmp(&p1, &p2, 4)) bad++; n++;
            }
    for (unsigned long u = 0x30800000ul; u < 0x41000000ul; u += stride) { unsigned b = (unsigned)u; float x; memcpy(&x, &b, 4);
        const float p2 = x * x;
        float p1 = use_libm ? libm_powf(x, 2) : powf(x, 2); if (memcmp(&p1, &p2, 4)) bad++;
        p1 = use_libm ? libm_powf(-x, 2) : powf(-x, 2); if (memcmp(&p1, &p2, 4)) bad++; n += 2; }
    *total = n; return bad;
}
unsigned dm_acos_bits(float x) { return rtm::float_to_bits(rtd::acos_libm(x)); }
unsigned dm_exp_bits(float x) { return rtm::float_to_bits(rtd::exp_libm(x)); }
// what the device hook (rt_math_check.hip, eval_kernel) writes for one routine, computed with the host build of the header:
// lets the CPU suite run the device sweeps' host reference (tests/cpu_native/math_sweep_ref.cpp) on known-good data
void dm_eval(int routine, unsigned first, unsigned long count, unsigned arg, void *out) {
    unsigned *w = (unsigned *)out;
    for (unsigned long k = 0; k < count; ++k) { const unsigned in = first + (unsigned)k; const float x = rtm::bits_to_float(in);
        switch (routine) {
        case rtm::kExp: w[k] = rtm::float_to_bits(rtd::exp_libm(x)); break;
        case rtm::kPow5: w[k] = rtm::float_to_bits(rtd::pow5(x)); break;
        case rtm::kAcos: w[k] = rtm::float_to_bits(rtd::acos_libm(x)); break;
        case rtm::kAtan: w[k] = rtm::float_to_bits(rtd::atan_libm(x)); break;
        case rtm::kAtan2: { float y2, x2; rtm::atan2_pair(in, y2, x2); w[k] = rtm::float_to_bits(rtd::atan2_libm(y2, x2)); break; }
        case rtm::kRng: { unsigned s1 = in, s2 = in; const float r = rtd::random_float(s1), pm = rtd::random_pm1(s2);
                          w[3 * k] = s1; w[3 * k + 1] = rtm::float_to_bits(r); w[3 * k + 2] = rtm::float_to_bits(pm); break; }
        case rtm::kTonemap: ((unsigned char *)out)[k] = rtd::tonemap_u8(x, rtm::bits_to_float(arg)); break;
        case rtm::kPow5Float: w[k] = rtm::float_to_bits(rtd::pow5_float(x)); break;
        }
    }
}
unsigned dm_wang(unsigned s) { return rtd::wang_hash(s); }
float dm_rand(unsigned *s) { return rtd::random_float(*s); }
unsigned char dm_tonemap(float sum, float inv) { return rtd::tonemap_u8(sum, inv); }
}
'''


@pytest.fixture(scope="module")
def dm(tmp_path_factory):
    d = tmp_path_factory.mktemp("dm")
    src = d / "dm.cpp"
    src.write_text(SRC % ROOT)
    so = d / "libdm.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.sweep_exp.restype = C.c_long
    lib.sweep_exp.argtypes = [C.c_uint, C.c_uint, C.c_uint]
    lib.sweep_pow5.restype = C.c_long
    lib.sweep_pow5.argtypes = [C.c_uint, C.POINTER(C.c_long)]
    for name in ("sweep_acos", "sweep_atan", "sweep_schlick"):
        getattr(lib, name).restype = C.c_long
        getattr(lib, name).argtypes = [C.c_uint, C.POINTER(C.c_long)]
    lib.sweep_atan2.restype = C.c_long
    lib.sweep_atan2.argtypes = [C.c_long]
    lib.sweep_atan2_structured.restype = C.c_long
    lib.sweep_atan2_structured.argtypes = [C.POINTER(C.c_long)]
    lib.dm_acos_bits.restype = lib.dm_exp_bits.restype = C.c_uint
    lib.dm_acos_bits.argtypes = lib.dm_exp_bits.argtypes = [C.c_float]
    lib.dm_eval.argtypes = [C.c_int, C.c_uint, C.c_ulong, C.c_uint, C.c_void_p]
    lib.sweep_identities.restype = C.c_long
    lib.sweep_identities.argtypes = [C.c_uint]
    lib.sweep_square.restype = C.c_long
    lib.sweep_square.argtypes = [C.c_uint, C.c_int, C.POINTER(C.c_long)]
    lib.dm_wang.restype = C.c_uint
    lib.dm_rand.restype = C.c_float
    lib.dm_rand.argtypes = [C.POINTER(C.c_uint)]
    lib.dm_tonemap.restype = C.c_ubyte
    lib.dm_tonemap.argtypes = [C.c_float, C.c_float]
    return lib


def test_expf_matches_host_libm(dm):
    """Every 61st non-positive float down to -128 and every 211th positive one up to 88: the same bits as this libm's expf
    (glibc's FMA build, which x86-64 hosts with FMA run; the restatement carries its four fusions).  The exhaustive
    sweep — tools/libm_exhaustive.cpp, profiles/r03/libm_exhaustive.txt — is 0 of 2.24e9.  Then the whole float line, NaNs
    included, every 13th float; all 94,743 floats of (88, 0x1.62e42ep6], where exp is still finite (a negative absorption
    reaches them: test_negative_absorption_frame_matches_the_oracle), and every NaN of either sign, each compared bit for bit
    (glibc returns a NaN argument as x + x: quietened).  The device build: tests/dev_math_checks.py, all 2^32 floats."""
    assert dm.sweep_exp(0x80000000, 0xC3000000, 61) == 0
    assert dm.sweep_exp(0x00000000, 0x42B00000, 211) == 0
    assert dm.sweep_exp(0x00000000, 0xFFFFFFFF, 13) == 0
    assert dm.sweep_exp(0x42B00001, 0x42B17218, 1) == 0
    assert dm.sweep_exp(0x7F800001, 0x7FFFFFFF, 1) == 0
    assert dm.sweep_exp(0xFF800001, 0xFFFFFFFF, 1) == 0
    assert dm.dm_exp_bits(88.5) != 0x7F800000 and dm.dm_exp_bits(89.0) == 0x7F800000
    assert dm.dm_exp_bits(C.c_float.from_buffer_copy(C.c_uint32(0x7F800001)).value) == 0x7FC00001


def test_pow5_is_the_host_libms_powf(dm):
    """(1 - cos)^5 of the Schlick term: rt_device_math.h pow5 restates glibc's powf for y = 5; every 37th float of [0, 2]
    here, all 1.07e9 of them in tools/libm_exhaustive.cpp: 0 differ."""
    total = C.c_long()
    assert dm.sweep_pow5(37, C.byref(total)) == 0 and total.value > 25_000_000
    # what the kernel evaluates: the comparison with the random draw, bracketed by the neighbours of the rounded x^5 — for
    # draws at, just below and just above the reflectance (the only places where the bracket is not decisive) and random ones
    assert dm.sweep_schlick(131, C.byref(total)) == 0 and total.value > 100_000_000


def test_acos_atan_atan2_are_the_host_libms(dm):
    """get_sphere_uv (include/sphere.h:16-22): the fdlibm-derived float routines glibc 2.35 carries, restated; strided
    here (every 41st float for acosf, every 157th float for atanf, 30 M pairs and the device sweep's 4.2 M structured pairs for
    atan2f), exhaustive in tools/libm_exhaustive.cpp (all of [-1, 1], all 2^32 floats, 2^31 pairs) and on the device
    (tests/dev_math_checks.py): 0 differ.  Every result bit counts, NaNs included: for |x| > 1 acos_libm returns the libm's
    +qNaN, not the x86 default NaN (sign set) of the source's (x - x) / (x - x)."""
    total = C.c_long()
    assert dm.sweep_acos(41, C.byref(total)) == 0 and total.value > 100_000_000
    assert dm.sweep_atan(157, C.byref(total)) == 0 and total.value > 25_000_000
    assert dm.sweep_atan2(30_000_000) == 0
    assert dm.sweep_atan2_structured(C.byref(total)) == 0 and total.value == 48 * 48 + (4 << 20)
    for x in (1.0000001, -1.5, float("inf"), float("-inf"), 3e38):
        assert dm.dm_acos_bits(x) == 0x7FC00000


def test_single_op_through_double_equals_float_op(dm):
    assert dm.sweep_identities(1009) == 0


def test_square_is_what_an_optimised_build_makes_of_powf_2(dm):
    """ELLIPSE interior test (include/plane.h:41: powf(x, 2); rt_kernel.hip.inc: x * x).  With the literal exponent
    every optimising compiler expands the call to x * x — checked here on the code gcc makes of it with the oracle's
    flags (-O2, no fast-math): identical on all 103 k exact-tie inputs and on every 5th float of [2^-30, 8) and the
    negatives (111 M values).  That is the parity target: both of the reference's build files compile with -O3.
    The library routine itself (what an UNoptimised build calls) is not correctly rounded: glibc 2.35's powf(x, 2)
    differs from x * x by one ulp on ~0.07 % of the sweep and on most exact ties — measured, not asserted to be zero;
    the bound below only keeps the documented figure honest."""
    total = C.c_long()
    assert dm.sweep_square(5, 0, C.byref(total)) == 0 and total.value > 100_000_000
    bad = dm.sweep_square(5, 1, C.byref(total))
    assert bad / total.value < 2e-3


def test_rng_and_tonemap_match_oracle(dm, golden):
    import oracle_bindings as ob
    for k, v in golden["wang_hash"].items():
        assert dm.dm_wang(int(k)) == v
    s1, s2 = C.c_uint(123456789), C.c_uint(123456789)
    for _ in range(1000):
        a = dm.dm_rand(C.byref(s1))
        b = ob.lib().orc_random_float(C.byref(s2))
        assert a == b and s1.value == s2.value
    rng = np.random.default_rng(3)
    sums = np.concatenate([rng.uniform(0, 40, 3000), [0.0, -1.0, 1e9, 3.996, 3.9961]]).astype(np.float32)
    want = ob.write_color_bytes(np.stack([sums, sums, sums], 1), 4)[:, 0]
    inv = np.float32(1.0 / np.float64(np.float32(4)))
    got = np.array([dm.dm_tonemap(float(x), float(inv)) for x in sums], dtype=np.uint8)
    assert np.array_equal(got, want)


def _build_sweep_reference(tmp_path_factory):
    """tests/cpu_native/math_sweep_ref.cpp: the device sweeps' host reference, built as tests/dev_math_checks.py builds it."""
    so = tmp_path_factory.mktemp("msr") / "libmsr.so"
    oracle = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", str(so),
                    os.path.join(ROOT, "tests", "cpu_native", "math_sweep_ref.cpp"), "-L" + oracle, "-lrt_oracle",
                    "-Wl,-rpath," + oracle], check=True)
    lib = C.CDLL(str(so))
    lib.msr_compare.restype = C.c_uint64
    lib.msr_compare.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
    lib.msr_sanity.restype = C.c_uint64
    lib.msr_sanity.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_double,
                               C.POINTER(C.c_uint64)]
    return lib


def test_device_sweep_reference_on_host_evaluations(dm, tmp_path_factory):
    """The comparison the device sweeps rely on, run here on what the host build of the header computes (equal to the libm
    and the oracle by the sweeps above): 0 differences for every routine; a corrupted word, an exp evaluated by the wrong
    function, or a pow5_float pushed out of its window are found, and the sanity floor passes known-good data only."""
    ref = _build_sweep_reference(tmp_path_factory)
    EXP, POW5, ACOS, ATAN, ATAN2, RNG, TONEMAP, POW5_FLOAT = range(8)
    n = 1 << 16
    buf = np.zeros(3 * n, dtype=np.uint32)
    worst = (C.c_uint32 * 8)()
    sampled = C.c_uint64()
    inv3 = int(np.float32(1.0 / 3.0).view(np.uint32))
    for routine, first, arg, carg in [(EXP, 0x42B10000, 0, 0), (EXP, 0x7FBF8000, 0, 0), (EXP, 0xC2A00000, 0, 0),
                                      (POW5, 0x3F000000, 0, 0), (POW5, 0x80000000, 0, 0), (ACOS, 0xBF7F8000, 0, 0),
                                      (ACOS, 0x3F7F8000, 0, 0), (ATAN, 0x3EE00000, 0, 0), (ATAN2, 0, 0, 0),
                                      (ATAN2, 1 << 30, 0, 0), (RNG, 0xFFFF0000, 0, 0), (TONEMAP, 0x40400000, inv3, 3),
                                      (TONEMAP, 0xFF7F8000, inv3, 3), (POW5_FLOAT, 0x3FFF0000, 0, 0)]:
        dm.dm_eval(routine, first, n, arg, buf.ctypes.data)
        assert ref.msr_compare(routine, first, n, carg, buf.ctypes.data, 4, worst) == 0, (routine, hex(first))
        if routine != POW5_FLOAT:
            ulps = 3.0 if routine == ATAN2 else 1.0
            assert ref.msr_sanity(routine, first, n, arg, buf.ctypes.data, 7, ulps, C.byref(sampled)) == 0, (routine, hex(first))
            assert sampled.value == (n + 6) // 7
    # a wrong bit is found, and reported by its input
    dm.dm_eval(ACOS, 0x3F000000, n, 0, buf.ctypes.data)
    buf[777] ^= 1
    assert ref.msr_compare(ACOS, 0x3F000000, n, 0, buf.ctypes.data, 4, worst) == 1 and worst[0] == 0x3F000000 + 777
    # exp evaluated by atan: the bit comparison and the sanity floor both object
    dm.dm_eval(ATAN, 0x3F000000, n, 0, buf.ctypes.data)
    assert ref.msr_compare(EXP, 0x3F000000, n, 0, buf.ctypes.data, 4, worst) == n
    assert ref.msr_sanity(EXP, 0x3F000000, n, 0, buf.ctypes.data, 7, 1.0, C.byref(sampled)) == sampled.value
    # pow5_float moved 13 steps: now more than kPow5Window = 6 away from the libm's powf, which was within 6 of it
    dm.dm_eval(POW5_FLOAT, 0x3F000000, n, 0, buf.ctypes.data)
    buf[:n] += 13
    assert ref.msr_compare(POW5_FLOAT, 0x3F000000, n, 0, buf.ctypes.data, 4, worst) == n


# ---------------------------------------------------------------------------------------------------- GPU
HERE = os.path.dirname(os.path.abspath(__file__))
LIBM_SWEEPS = ["test_this_is_the_developer_library_with_the_math_hook", "test_hook_refuses_bad_arguments_before_any_hip_call",
               "test_exp_libm_is_expf_for_every_float", "test_acos_libm_is_acosf_for_every_float",
               "test_atan_libm_is_atanf_for_every_float", "test_atan2_libm_is_atan2f_on_2_31_pairs",
               "test_pow5_is_powf_5_on_its_domain", "test_libm_powf_lies_in_the_schlick_window_of_pow5_float",
               "test_schlick_bracket_decides_as_the_libm_comparison_on_the_device"]
RNG_SAVER_SWEEPS = ["test_this_is_the_developer_library_with_the_math_hook", "test_rng_matches_the_oracle_for_every_state",
                    "test_tonemap_matches_the_oracles_saver_for_every_float", "test_sanity_floor_device_values_are_the_functions"]


def _run_dev_math_checks(names):
    """tests/dev_math_checks.py's named tests in one child process that loads the developer library (rt_debug_math_eval)."""
    from conftest import run_child
    dev_lib = os.path.join(ROOT, "ray-tracing-practice_amd", "librtp_amd_dev.so")
    assert os.path.exists(dev_lib), "run __graft_entry__.build() (make -C ray-tracing-practice_amd dev)"
    env = dict(os.environ, RTP_AMD_LIB=dev_lib)
    ids = [os.path.join(HERE, "dev_math_checks.py") + "::" + n for n in names]
    res = run_child([sys.executable, "-m", "pytest", *ids, "-x", "-q", "-s", "-p", "no:cacheprovider"], 200, env=env)
    print(res.stdout[-6000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert f"{len(names)} passed" in res.stdout and "failed" not in res.stdout and "skipped" not in res.stdout


@pytest.mark.gpu
def test_device_libm_routines_are_the_host_libms_on_gfx950():
    """exp_libm, acos_libm and atan_libm on all 2^32 floats, atan2_libm on 2^31 pairs, pow5 on [-0, 2.25] and the denormals,
    pow5_float's window on [0, 2], and the Schlick bracket on every cos of [-1, 1] at six r0 — compiled for gfx950 and run
    there, every result bit against glibc (tests/dev_math_checks.py).  The child's SWEEP lines give the time of each sweep;
    on an MI355X the nine tests took 12-13 s in all, 0 differences."""
    _run_dev_math_checks(LIBM_SWEEPS)


@pytest.mark.gpu
def test_device_rng_and_saver_are_the_oracles_on_gfx950():
    """wang_hash, random_float and random_pm1 for all 2^32 seeds against the oracle, rt_tonemap for all 2^32 float sums at five
    divisors against orc_write_color, and the sanity floor against double precision (tests/dev_math_checks.py).  On an MI355X:
    19-20 s in all, 0 differences."""
    _run_dev_math_checks(RNG_SAVER_SWEEPS)


@pytest.mark.gpu
def test_negative_absorption_frame_matches_the_oracle():
    """A glass sphere (radius 1, ir 1.5) with a NEGATIVE absorption: rt_material.absorption is not range-checked, and the scene
    builder makes strength * (1 - colour), negative for a colour component above 1.  Beer-Lambert evaluates
    exp(-absorption * dist) on the inside chords, whose lengths run from 2 cos(asin(1/1.5)) = 1.49 to the diameter; with
    absorption.x = -44.35 the chords longer than 88 / 44.35 = 1.984 put exp's argument in (88, 88.70], where expf is finite
    and exp_libm once returned +inf (inf / inf = NaN pixels; the oracle's are finite).  The frame must be the oracle's, bit for
    bit; y and z (-44 and -30) keep below 88."""
    import oracle_bindings as ob
    import rtp_bindings as rb
    glass = rb.Material()
    glass.type, glass.ir = 2, 1.5
    glass.absorption.e[:] = (-44.35, -44.0, -30.0)
    host = rb.HostScene.from_arrays(np.array([[0, 0, 0, 1, 0]], np.float32), np.zeros((0, 11), np.float32), [glass])
    cam = rb.make_camera(96, 96, 30.0, (5, 0, 0), (0, 0, 0), (0.7, 0.8, 1.0), spp=16, max_depth=50)      # (z is up)
    want = ob.render(host, cam, threads=8)
    assert np.isfinite(want).all()
    # paths through the glass: attenuation / p leaves red at 1 and blue at e^(-14.35 dist) per chord
    assert (want[:, :, 2] < 1e-3 * want[:, :, 0]).sum() > 1000
    dev = rb.DeviceScene(host, device=0, honour_env=False)
    fb, _ = dev.render_to_host(cam)
    dev.close()
    same = (np.ascontiguousarray(fb).view(np.uint32) == want.view(np.uint32)).all(axis=-1)
    assert same.all(), f"{(~same).sum()} of {same.size} pixels differ ({(~np.isfinite(fb)).any(axis=-1).sum()} not finite)"
