// rtd::random_float (ray-tracing-practice_amd/csrc/rt_device_math.h) against the reference's expression, bit for bit:
//     seed = wang_hash(seed);  return static_cast<float>(seed) / 4294967296.0f;          (include/random_utils.h:16-19)
// The division is a real one here (volatile divisor: the compiler cannot turn it into the multiplication under test).
// Seeds: a strided sweep of the 32-bit range, the edges 0, 1, 0x7fffffff and 0xffffff80 … 0xffffffff, and — through the inverse
// of wang_hash, which is a bijection — the seeds whose HASH is 0xffffff00 … 0xffffffff: from 0xffffff80 on (float)hash rounds up
// to 2^32 and the draw is exactly 1.0f; below it is the largest float under 1.  The state left in `seed` is compared too.
// Built by tests/test_random_float_native.py: g++ -O2 -ffp-contract=off [-fsanitize=address,undefined], a program of its own.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../ray-tracing-practice_amd/csrc/rt_device_math.h"

namespace {

volatile float kTwo32 = 4294967296.0f;

uint32_t ref_wang_hash(uint32_t seed) {
    seed = (seed ^ 61) ^ (seed >> 16);
    seed *= 9;
    seed = seed ^ (seed >> 4);
    seed *= 0x27d4eb2d;
    seed = seed ^ (seed >> 15);
    return seed;
}
float ref_random_float(uint32_t &seed) {
    seed = ref_wang_hash(seed);
    return static_cast<float>(seed) / kTwo32;
}

uint32_t inverse_odd(uint32_t a) {          // a * x = 1 mod 2^32 (Newton: each step doubles the correct low bits)
    uint32_t x = a;
    for (int k = 0; k < 5; ++k) x *= 2u - a * x;
    return x;
}
uint32_t unhash(uint32_t h) {               // the seed whose wang_hash is h
    h ^= (h >> 15) ^ (h >> 30);
    h *= inverse_odd(0x27d4eb2du);
    h ^= (h >> 4) ^ (h >> 8) ^ (h >> 12) ^ (h >> 16) ^ (h >> 20) ^ (h >> 24) ^ (h >> 28);
    h *= inverse_odd(9u);
    const uint32_t hi = h >> 16;            // (s ^ 61) ^ (s >> 16) leaves the upper half of s as it is
    return (h & 0xffff0000u) | ((h ^ 61u ^ hi) & 0xffffu);
}

uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

uint64_t checked = 0, failed = 0;
void check(uint32_t seed) {
    uint32_t a = seed, b = seed;
    const float got = rtd::random_float(a), want = ref_random_float(b);
    ++checked;
    if (bits(got) != bits(want) || a != b) {
        if (failed++ < 8) printf("seed %08x: got %08x (state %08x), reference %08x (state %08x)\n", seed, bits(got), a, bits(want), b);
    }
}

}  // namespace

int main() {
    for (uint64_t s = 0; s < (1ull << 32); s += 4099) check((uint32_t)s);
    check(0u); check(1u); check(0x7fffffffu);
    for (uint32_t s = 0xffffff80u; s != 0; ++s) check(s);
    uint32_t ones = 0, below = 0;
    for (uint32_t h = 0xffffff00u; h != 0; ++h) {
        const uint32_t s = unhash(h);
        if (ref_wang_hash(s) != h || rtd::wang_hash(s) != h) { printf("unhash(%08x) = %08x is not the inverse\n", h, s); return 2; }
        check(s);
        uint32_t t = s;
        const uint32_t r = bits(rtd::random_float(t));
        if (h >= 0xffffff80u) ones += r == 0x3f800000u;         // exactly 1.0f
        else below += r == 0x3f7fffffu;                         // the largest float below 1
    }
    printf("checked %llu seeds, %llu differ; hashes >= 0xffffff80 giving exactly 1.0f: %u of 128, the 128 below giving 0x3f7fffff: %u\n",
           (unsigned long long)checked, (unsigned long long)failed, ones, below);
    if (failed || ones != 128 || below != 128) return 1;
    printf("all ok\n");
    return 0;
}
