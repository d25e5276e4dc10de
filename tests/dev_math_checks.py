"""Device sweeps of ray-tracing-practice_amd/csrc/rt_device_math.h on gfx950: every result bit of the routines the kernels share,
over whole domains, against the host libm the reference calls and the oracle (tests/cpu_native/math_sweep_ref.cpp).  Needs the
DEVELOPER build (rt_debug_math_eval, csrc/rt_math_check.hip).  Not collected by the normal test run (the file name does not match
test_*.py): tests/test_device_math.py runs it in two child processes with RTP_AMD_LIB pointing at the developer library.

Each sweep evaluates chunks of at most 1 GB on the device, copies them to pinned host memory and compares them there on up to 16
threads.  NaN results are compared bit for bit like any other."""
import ctypes as C
import os
import subprocess
import time

import pytest
import torch

import rtp_bindings as rb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP, POW5, ACOS, ATAN, ATAN2, RNG, TONEMAP, POW5_FLOAT, SCHLICK = range(9)      # rtm::Routine (csrc/rt_math_check.h)
CHUNK_BYTES = 1 << 30
THREADS = min(16, len(os.sched_getaffinity(0)))
ALL = 1 << 32


def f2u(x):
    return C.c_uint32.from_buffer_copy(C.c_float(x)).value


def u2f(u):
    return C.c_float.from_buffer_copy(C.c_uint32(u)).value


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
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


class Device:
    """One device buffer and one pinned host buffer of CHUNK_BYTES, reused by every chunk; the hook on torch's stream."""

    def __init__(self):
        self.lib = rb.amd_lib()
        self.lib.rt_debug_math_eval.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        self.lib.rt_debug_math_eval.restype = C.c_int
        self.lib.rt_tonemap.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        self.lib.rt_tonemap.restype = C.c_int
        self.out = torch.empty(CHUNK_BYTES, dtype=torch.uint8, device="cuda:0")
        self.host = torch.empty(CHUNK_BYTES, dtype=torch.uint8, pin_memory=True)
        self.stream = torch.cuda.current_stream().cuda_stream

    def check(self, st):
        if st != 0:
            raise RuntimeError(f"status {st}: {self.lib.rt_get_last_error_string().decode()}")

    def eval(self, routine, first, count, arg, nbytes):
        """rt_debug_math_eval into the device buffer; its first nbytes are copied to the pinned buffer, whose address is returned."""
        assert nbytes <= CHUNK_BYTES
        self.check(self.lib.rt_debug_math_eval(routine, first, count, arg, self.out.data_ptr(), self.stream))
        self.host[:nbytes].copy_(self.out[:nbytes])
        return self.host.data_ptr()


@pytest.fixture(scope="module")
def dev():
    lib = rb.amd_lib()
    assert b"dev=1" in lib.rt_version_string()
    lib.rt_get_last_error_string.restype = C.c_char_p
    return Device()


WORD_ROUTINES = {EXP: 4, POW5: 4, ACOS: 4, ATAN: 4, ATAN2: 4, POW5_FLOAT: 4, RNG: 12, TONEMAP: 1}


def sweep(dev, ref, name, routine, lo, hi, arg=0):
    """Every input of [lo, hi) through the routine on the device, compared with the host reference.  Prints and returns the
    seconds it took."""
    t0 = time.perf_counter()
    per = min(1 << 28, CHUNK_BYTES // WORD_ROUTINES[routine])
    per = 1 << (per.bit_length() - 1)
    bad, examples = 0, []
    for first in range(lo, hi, per):
        n = min(per, hi - first)
        ptr = dev.eval(routine, first, n, arg, n * WORD_ROUTINES[routine])
        worst = (C.c_uint32 * 8)()
        b = ref.msr_compare(routine, first, n, arg, ptr, THREADS, worst)
        bad += b
        examples += [f"{w:08x}" for w in worst[:min(b, 8)]]
    dt = time.perf_counter() - t0
    print(f"SWEEP {name}: {hi - lo} inputs [{lo:#010x}, {hi:#010x}), {bad} differ, {dt:.1f} s")
    assert bad == 0, f"{name}: {bad} of {hi - lo} inputs differ from the host reference, e.g. {examples[:8]}"
    return dt


def test_this_is_the_developer_library_with_the_math_hook():
    lib = rb.amd_lib()
    assert b"dev=1" in lib.rt_version_string() and hasattr(lib, "rt_debug_math_eval")


def test_hook_refuses_bad_arguments_before_any_hip_call(dev):
    ev = dev.lib.rt_debug_math_eval
    assert ev(EXP, 0, 16, 0, None, dev.stream) == 1
    assert ev(-1, 0, 16, 0, dev.out.data_ptr(), dev.stream) == 1
    assert ev(SCHLICK + 1, 0, 16, 0, dev.out.data_ptr(), dev.stream) == 1
    assert ev(EXP, 0, 0, 0, dev.out.data_ptr(), dev.stream) == 1
    assert ev(EXP, 0xFFFFFFF0, 17, 0, dev.out.data_ptr(), dev.stream) == 1
    assert ev(EXP, 0xFFFFFFF0, 16, 0, dev.out.data_ptr(), dev.stream) == 0
    torch.cuda.synchronize()


def test_exp_libm_is_expf_for_every_float(dev, ref):
    """exp_libm against glibc's expf on all 2^32 floats, NaN bits included (Beer-Lambert, rt_kernel.hip.inc; the denoiser's
    weights).  1.1-1.2 s on an MI355X with 16 host threads."""
    sweep(dev, ref, "exp_libm", EXP, 0, ALL)


def test_acos_libm_is_acosf_for_every_float(dev, ref):
    """acos_libm against glibc's acosf on all 2^32 floats: [-1, 1], the +qNaN of |x| > 1 and the quietened NaN inputs.
    1.4-1.5 s on an MI355X."""
    sweep(dev, ref, "acos_libm", ACOS, 0, ALL)


def test_atan_libm_is_atanf_for_every_float(dev, ref):
    """atan_libm against glibc's atanf on all 2^32 floats.  1.0-1.1 s on an MI355X."""
    sweep(dev, ref, "atan_libm", ATAN, 0, ALL)


def test_atan2_libm_is_atan2f_on_2_31_pairs(dev, ref):
    """atan2_libm against glibc's atan2f on the 2^31 pairs of rtm::atan2_pair: the 48 x 48 special pairs (signed zeros,
    denormals, infinities, NaNs, +-1, the branch points), 2^22 unit-circle points, then random pairs of four kinds.
    4.5-4.8 s on an MI355X (atan2f is the slowest of the host references)."""
    sweep(dev, ref, "atan2_libm", ATAN2, 0, 1 << 31)


def test_pow5_is_powf_5_on_its_domain(dev, ref):
    """pow5 against glibc's powf(x, 5.0f) for every float of [+0, 2.25] — (1 - cos) leaves [0, 2] by rounding — and for -0 and
    the negative denormals.  0.8 s on an MI355X."""
    sweep(dev, ref, "pow5 [0, 2.25]", POW5, 0, f2u(2.25) + 1)
    sweep(dev, ref, "pow5 [-denormal, -0]", POW5, 0x80000000, 0x80800000)


def test_libm_powf_lies_in_the_schlick_window_of_pow5_float(dev, ref):
    """schlick_bracket's premise: for every x in [0, 2] the libm's powf(x, 5) is within kPow5Window float steps of the device's
    pow5_float(x).  0.7-0.8 s on an MI355X."""
    sweep(dev, ref, "pow5_float window", POW5_FLOAT, 0, f2u(2.0) + 1)


def test_schlick_bracket_decides_as_the_libm_comparison_on_the_device(dev):
    """schlick_bracket / schlick_exceeds against r0 + (1 - r0) * pow5(1 - cos) > rnd — pow5 being the libm's powf(x, 5)
    (test_pow5_is_powf_5_on_its_domain) — for every float cos in [-1, 1], at several r0 (the packer's schlick_r0sq for
    ir = 1.5, 1/1.5, 1.33, 2.4, and 0, 0.5), with draws at the reflectance, 1 … 3 float steps either side of it and two
    random_float draws, all on the device (rtm::schlick_check): 1.15e11 draws in 0.2 s on an MI355X.  Random draws the bracket
    leaves to pow5: the header says ~1e-6; measured 3.26e-7 (8 332 of 2.56e10).  The near draws are mostly undecided, by design."""
    import numpy as np
    r0s = []                                         # schlick_r0sq(ir) as the packer makes it, in float
    for ir in (1.5, 1.0 / 1.5, 1.33, 2.4):
        f = np.float32(ir)
        r = (np.float32(1.0) - f) / (np.float32(1.0) + f)
        r0s.append(float(np.float32(r * r)))
    r0s += [0.0, 0.5]
    t0 = time.perf_counter()
    ctr = (C.c_uint64 * 6)()
    total = [0] * 5
    for r0 in r0s:
        for lo, hi in ((0, f2u(1.0) + 1), (0x80000000, f2u(-1.0) + 1)):
            dev.check(dev.lib.rt_debug_math_eval(SCHLICK, lo, hi - lo, f2u(r0), dev.out.data_ptr(), dev.stream))
            dev.host[:48].copy_(dev.out[:48])
            C.memmove(ctr, dev.host.data_ptr(), 48)
            assert ctr[0] == 0, f"r0 = {r0}: {ctr[0]} draws decided differently from the libm comparison, first cos {ctr[5]:#010x}"
            for k in range(5):
                total[k] += ctr[k]
    dt = time.perf_counter() - t0
    bad, seen, near_undecided, random, random_undecided = total
    rate = random_undecided / random
    print(f"SWEEP schlick: {len(r0s)} r0 x {2 * f2u(1.0) + 2} cos, {seen} draws, {bad} differ; undecided: {near_undecided} of the "
          f"near draws, {random_undecided} of {random} random draws ({rate:.2e}), {dt:.1f} s")
    assert seen > 9 * 10 ** 10 and random == len(r0s) * 2 * (2 * f2u(1.0) + 2)
    assert near_undecided > seen // 2            # draws at the reflectance are what the bracket cannot decide
    assert 0 < rate < 1e-6


def test_rng_matches_the_oracle_for_every_state(dev, ref):
    """wang_hash and random_float against orc_wang_hash / orc_random_float, and random_pm1's fma shortcut against the reference's
    random_float(seed, -1, 1) = -1 + (1 - -1) * r in float, for all 2^32 seeds.  2.6-2.8 s on an MI355X."""
    sweep(dev, ref, "rng", RNG, 0, ALL)


def test_tonemap_matches_the_oracles_saver_for_every_float(dev, ref):
    """rt_tonemap (the public call, no hook) on all 2^32 float sums at divisors 1, 3, 500, 1000 and 65536, against
    orc_write_color: NaN, negative, denormal and infinite sums included.  14.1-14.5 s on an MI355X for the five."""
    base = torch.arange(1 << 28, dtype=torch.int32, device="cuda:0")
    sums = torch.empty_like(base)
    t0 = time.perf_counter()
    for divisor in (1, 3, 500, 1000, 65536):
        for first in range(0, ALL, 1 << 28):
            torch.add(base, first - ALL if first >= 1 << 31 else first, out=sums)
            dev.check(dev.lib.rt_tonemap(sums.data_ptr(), dev.out.data_ptr(), 1 << 28, divisor, dev.stream))
            dev.host[:1 << 28].copy_(dev.out[:1 << 28])
            worst = (C.c_uint32 * 8)()
            b = ref.msr_compare(TONEMAP, first, 1 << 28, divisor, dev.host.data_ptr(), THREADS, worst)
            assert b == 0, f"divisor {divisor}: {b} sums differ, e.g. {[f'{w:08x}' for w in worst[:min(b, 8)]]}"
    print(f"SWEEP tonemap: 5 divisors x 2^32 sums, 0 differ, {time.perf_counter() - t0:.1f} s")


def test_sanity_floor_device_values_are_the_functions(dev, ref):
    """Against the double-precision function, so that a sweep comparing a routine with itself (or with the wrong function)
    cannot pass: every 97th input of a few 2^24-input windows within 1 float step (atan2: 3 — glibc 2.35's atan2f is off by up to
    ~2.4 ulps where exhaustively equal to the device) — and the hook's tonemap_u8 at the rt_tonemap divisors within one byte
    of 256 * min(sqrt(sum / divisor), 0.999)."""
    n = 1 << 24
    cases = [(EXP, 0, [0xC2000000, 0x42A00000, 0x42B17000, 0xC2D00000]), (ACOS, 0, [0x3E000000, 0xBF000000, 0x3F7F0000]),
             (ATAN, 0, [0x3E000000, 0xBF800000, 0x4B000000]), (ATAN2, 0, [0, 1 << 24, 1 << 30]),
             (POW5, 0, [0x3E000000, 0x3F7F0000, 0x00000000]), (RNG, 0, [0, 0x9E3779B9 & ~(n - 1)])]
    for divisor in (1, 3, 500, 1000, 65536):
        cases.append((TONEMAP, f2u(1.0 / u2f(f2u(float(divisor)))), [0x3F000000, 0x44000000, 0x80000000]))
    for routine, arg, starts in cases:
        ulps = 3.0 if routine == ATAN2 else 1.0
        for first in starts:
            ptr = dev.eval(routine, first, n, arg, n * WORD_ROUTINES[routine])
            sampled = C.c_uint64()
            bad = ref.msr_sanity(routine, first, n, arg, ptr, 97, ulps, C.byref(sampled))
            assert sampled.value > 170_000
            assert bad == 0, f"routine {routine} at {first:#010x}: {bad} of {sampled.value} sampled values off the double result"
