// rt_math_check.h — what the developer build's device sweeps of rt_device_math.h evaluate (rt_math_check.hip,
// rt_debug_math_eval), shared with their host reference (tests/cpu_native/math_sweep_ref.cpp) so that both sides enumerate
// the same arguments.  Test infrastructure: the shipped library does not include it.
#pragma once
#include "rt_device_math.h"

namespace rtm {

// rt_debug_math_eval's routine numbers and what each writes per input index k (input = first + k):
enum Routine : int32_t {
    kExp = 0,        // u32: exp_libm(bits k)
    kPow5 = 1,       // u32: pow5(bits k)
    kAcos = 2,       // u32: acos_libm(bits k)
    kAtan = 3,       // u32: atan_libm(bits k)
    kAtan2 = 4,      // u32: atan2_libm(y, x) of atan2_pair(k)
    kRng = 5,        // 3 x u32: wang_hash(k), random_float's value and random_pm1's value, each from seed k
    kTonemap = 6,    // u8:  tonemap_u8(bits k, inv_divisor = bits arg)
    kPow5Float = 7,  // u32: pow5_float(bits k)
    kSchlick = 8,    // 6 x u64 in all (not per input): see schlick_check; arg = bits of r0
    kRoutines = 9,   // the routines numbered consecutively end here; 9 itself stays refused (the hook's argument test pins it as unknown)
    kLog = 10        // u32: log_libm(bits k)
};
// Is `routine` one of the above?  (Not a range test: 9 is none.  A further routine gets the next number after kLog and a line here.)
RT_HD bool is_routine(int32_t routine) { return (routine >= 0 && routine < kRoutines) || routine == kLog; }

// ---- atan2 pairs: index → (y, x) -------------------------------------------------------------------------------------
// [0, kSpecialPairs): every (y, x) of kSpecials x kSpecials — signed zeros, denormals, the normal range's ends, +-1 and its
// neighbours, the branch points of atan_libm, +-2^+-60 (atan2's |y/x| fences), infinities and NaNs of both kinds and signs.
// [kSpecialPairs, + kCirclePairs): points of the unit circle in all four quadrants, (2t, 1 - t^2) / (1 + t^2) for
// t = j 2^-20 — what a unit normal's (-z, x) gives get_sphere_uv.  Beyond: wang_hash draws, in turn raw bit patterns (every
// exponent, infinities, NaNs, denormals), [-1, 1] fixed-point pairs, pairs with x = +-1, and pairs whose exponents differ by
// -64 … 63 (both sides of the 2^60 fences).
constexpr uint32_t kNumSpecials = 48;
#if defined(__HIPCC__)
__device__ __constant__
#endif
static const uint32_t kSpecials[kNumSpecials] = {
    0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u,
    0x3f800000u, 0xbf800000u, 0x3f800001u, 0xbf800001u, 0x3f7fffffu, 0xbf7fffffu, 0x3f000000u, 0xbf000000u,
    0x40000000u, 0xc0000000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
    0x7f800001u, 0xff800001u, 0x7fc12345u, 0x7fa00000u, 0x5d800000u, 0xdd800000u, 0x21800000u, 0xa1800000u,
    0x4c000000u, 0xcc000000u, 0x31000000u, 0xb1000000u, 0x3ee00000u, 0xbee00000u, 0x3f300000u, 0xbf300000u,
    0x3f980000u, 0xbf980000u, 0x401c0000u, 0xc01c0000u, 0x3f3504f3u, 0xbf3504f3u, 0x40490fdbu, 0x3fc90fdbu,
};
constexpr uint32_t kSpecialPairs = kNumSpecials * kNumSpecials;
constexpr uint32_t kCircleBits = 20;
constexpr uint32_t kCirclePairs = 4u << kCircleBits;

RT_HD float bits_to_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
RT_HD uint32_t float_to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

RT_HD void atan2_pair(uint32_t i, float &y, float &x) {
    if (i < kSpecialPairs) {
        y = bits_to_float(kSpecials[i / kNumSpecials]);
        x = bits_to_float(kSpecials[i % kNumSpecials]);
        return;
    }
    i -= kSpecialPairs;
    if (i < kCirclePairs) {
        const float t = (float)(i >> 2) * 0x1p-20f, d = 1.0f + t * t;
        const float s = (2.0f * t) / d, c = (1.0f - t * t) / d;
        y = (i & 1u) ? -s : s;
        x = (i & 2u) ? -c : c;
        return;
    }
    uint32_t h = rtd::wang_hash(i * 0x9e3779b9u ^ 0x1234567u);
    const uint32_t a = h;
    h = rtd::wang_hash(h ^ 0x85ebca6bu);
    const uint32_t b = h;
    switch (i & 3u) {
    case 0: y = bits_to_float(a); x = bits_to_float(b); break;
    case 1: y = (float)(int32_t)a * 0x1p-31f; x = (float)(int32_t)b * 0x1p-31f; break;
    case 2: y = bits_to_float(a); x = (b & 1u) ? -1.0f : 1.0f; break;
    default: {
        const int32_t ey = (int32_t)((a >> 23) & 0xffu), ex = ey + (int32_t)(b >> 25) - 64;
        y = bits_to_float(a);
        x = bits_to_float((b & 0x807fffffu) | ((uint32_t)(ex < 0 ? 0 : ex > 254 ? 254 : ex) << 23));
    }
    }
}

// ---- Schlick: schlick_bracket / schlick_exceeds against r0 + (1 - r0) * pow5(1 - cos) > rnd ------------------------------
// For one cos in [-1, 1] (other inputs are skipped) and one r0: draws at the reflectance and 1 … 3 float steps either side of
// it (those of them that are >= 0), and two draws of random_float.  The counts are accumulated into out[] (u64):
//   [0] draws where the bracket's decided answer, or schlick_exceeds, differs from the comparison   [1] draws compared
//   [2] near draws the bracket left undecided (-1)   [3] random draws   [4] random draws left undecided
//   [5] the lowest input with a difference (all ones: none)
constexpr uint32_t kSchlickCounters = 6;
struct SchlickCounts { uint64_t bad, seen, near_undecided, random, random_undecided; };
RT_HD void schlick_check(uint32_t cos_bits, float r0, SchlickCounts &c) {
    const float cosine = bits_to_float(cos_bits);
    if (!(cosine >= -1.0f && cosine <= 1.0f)) return;
    const float ref = r0 + (1.0f - r0) * rtd::pow5(1.0f - cosine);
    const uint32_t rb = float_to_bits(ref);
    uint32_t seed = cos_bits ^ float_to_bits(r0);
    for (int d = -3; d <= 5; ++d) {
        float rnd;
        if (d <= 3) {
            if (d < 0 && rb < (uint32_t)-d) continue;
            rnd = bits_to_float(rb + (uint32_t)d);
        } else {
            rnd = rtd::random_float(seed);
        }
        const bool want = ref > rnd;
        const int b = rtd::schlick_bracket(cosine, r0, rnd);
        c.bad += ((b >= 0 && (b != 0) != want) || rtd::schlick_exceeds(cosine, r0, rnd) != want) ? 1u : 0u;
        c.seen += 1u;
        if (d <= 3) c.near_undecided += b < 0 ? 1u : 0u;
        else { c.random += 1u; c.random_undecided += b < 0 ? 1u : 0u; }
    }
}

}  // namespace rtm
