// Host reference of the device sweeps in tests/dev_math_checks.py: what the reference's CPU path computes for each input of
// rt_debug_math_eval (ray-tracing-practice_amd/csrc/rt_math_check.h), compared with a chunk of the device's output.
// Built by the test: g++ -O2 -ffp-contract=off -shared -fPIC -pthread, linked with oracle/librt_oracle.so.
//
// The libm routines are called through volatile function pointers, so the compiler can neither expand nor constant-fold them:
// these are glibc's own expf, powf, acosf, atanf and atan2f.  The RNG and the saver bytes are the oracle's (orc_wang_hash,
// orc_random_float, orc_write_color); random_float(seed, -1, 1) is written out as the reference writes it, in float.
#include <float.h>
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#include "../../ray-tracing-practice_amd/csrc/rt_math_check.h"

extern "C" {
uint32_t orc_wang_hash(uint32_t seed);
float orc_random_float(uint32_t *seed);
void orc_write_color(const float rgb_sum[3], int divisor, uint8_t out[3]);
}

namespace {

float (*volatile libm_expf)(float) = expf;
float (*volatile libm_acosf)(float) = acosf;
float (*volatile libm_atanf)(float) = atanf;
float (*volatile libm_atan2f)(float, float) = atan2f;
float (*volatile libm_powf)(float, float) = powf;

using rtm::bits_to_float;
using rtm::float_to_bits;

constexpr int kMaxThreads = 16, kReport = 8;

float ref_random_range(uint32_t *seed, float lo, float hi) { return lo + (hi - lo) * orc_random_float(seed); }   // random_utils.h:21-23

// Does the device's output for input index k (of the chunk starting at `first`) differ from the reference?
bool differs(int32_t routine, uint32_t in, uint32_t arg, const void *got, uint64_t k) {
    const uint32_t *w = (const uint32_t *)got;
    const float x = bits_to_float(in);
    switch (routine) {
    case rtm::kExp: return w[k] != float_to_bits(libm_expf(x));
    case rtm::kPow5: return w[k] != float_to_bits(libm_powf(x, 5.0f));
    case rtm::kAcos: return w[k] != float_to_bits(libm_acosf(x));
    case rtm::kAtan: return w[k] != float_to_bits(libm_atanf(x));
    case rtm::kAtan2: {
        float y2, x2;
        rtm::atan2_pair(in, y2, x2);
        return w[k] != float_to_bits(libm_atan2f(y2, x2));
    }
    case rtm::kRng: {
        uint32_t s1 = in, s2 = in;
        const float r = orc_random_float(&s1), pm = ref_random_range(&s2, -1.0f, 1.0f);
        return w[3 * k] != orc_wang_hash(in) || w[3 * k + 1] != float_to_bits(r) || w[3 * k + 2] != float_to_bits(pm);
    }
    case rtm::kTonemap: {            // the device's bytes of rt_tonemap at divisor `arg` (each channel is saved on its own)
        const float rgb[3] = {x, x, x};
        uint8_t want[3];
        orc_write_color(rgb, (int)arg, want);
        return ((const uint8_t *)got)[k] != want[0];
    }
    case rtm::kPow5Float: {          // the libm's powf(x, 5) within kPow5Window steps of pow5_float (x in [0, 2]: ranks)
        const uint32_t lib = float_to_bits(libm_powf(x, 5.0f)), dev = w[k];
        return (lib > dev ? lib - dev : dev - lib) > rtd::kPow5Window;
    }
    default: return true;
    }
}

struct Job {
    int32_t routine;
    uint32_t first, arg;
    const void *got;
    uint64_t lo, hi, bad;
    uint32_t worst[kReport];
    int nworst;
};

void *run(void *p) {
    Job &j = *(Job *)p;
    for (uint64_t k = j.lo; k < j.hi; ++k) {
        if (!differs(j.routine, j.first + (uint32_t)k, j.arg, j.got, k)) continue;
        if (j.nworst < kReport) j.worst[j.nworst++] = j.first + (uint32_t)k;
        ++j.bad;
    }
    return nullptr;
}

// Is the device's float within `ulps` float spacings (at the double value; subnormal spacing below 2^-126) of the
// double-precision value of the same function?  NaN only matches NaN, an infinity only an infinity of the same sign or a value
// beyond FLT_MAX.
bool within_ulps(float got, double want, double ulps) {
    if (want != want) return got != got;
    if (got != got) return false;
    if (isinf(got)) return (got > 0 ? want : -want) >= (double)FLT_MAX;
    int e;
    frexp(want, &e);
    const double ulp = ldexp(1.0, (e - 1 < -126 ? -126 : e - 1) - 23);
    return fabs((double)got - want) <= ulps * ulp;
}

}  // namespace

extern "C" {

// Compares `count` outputs of rt_debug_math_eval(routine, first, count, arg) (for kTonemap: rt_tonemap's bytes over the sums
// first … first + count - 1 at divisor `arg`) with the reference, on up to `threads` (<= 16) threads.  Returns the number of
// inputs that differ; worst[0 … min(8, that) - 1] get some of them, the lowest of each thread's share first.
uint64_t msr_compare(int32_t routine, uint32_t first, uint64_t count, uint32_t arg, const void *got, int threads, uint32_t *worst) {
    if (threads < 1) threads = 1;
    if (threads > kMaxThreads) threads = kMaxThreads;
    Job jobs[kMaxThreads];
    pthread_t tid[kMaxThreads];
    const uint64_t per = (count + threads - 1) / threads;
    for (int t = 0; t < threads; ++t) {
        Job &j = jobs[t];
        j = Job{routine, first, arg, got, per * t < count ? per * t : count, per * (t + 1) < count ? per * (t + 1) : count, 0, {}, 0};
        pthread_create(&tid[t], nullptr, run, &j);
    }
    uint64_t bad = 0;
    int n = 0;
    for (int t = 0; t < threads; ++t) {
        pthread_join(tid[t], nullptr);
        bad += jobs[t].bad;
        for (int i = 0; i < jobs[t].nworst && n < kReport; ++i) worst[n++] = jobs[t].worst[i];
    }
    return bad;
}

// The sanity floor: every stride-th output of the chunk is within `ulps` float steps of the double-precision function —
// exp, pow(x, 5), acos, atan, atan2, r = wang_hash(seed) * 2^-32 and -1 + 2 * (float)r (kRng), and for kTonemap (the kernel's
// bytes at inv_divisor = bits arg) 256 * min(sqrt(inv * sum), 0.999) in double, truncated, within one.  A comparison of a
// routine with itself, or with the wrong function, cannot pass this.  Returns the number of sampled outputs outside; *sampled
// the count.
uint64_t msr_sanity(int32_t routine, uint32_t first, uint64_t count, uint32_t arg, const void *got, uint64_t stride, double ulps,
                    uint64_t *sampled) {
    const uint32_t *w = (const uint32_t *)got;
    uint64_t bad = 0, n = 0;
    for (uint64_t k = 0; k < count; k += stride, ++n) {
        const uint32_t in = first + (uint32_t)k;
        const double x = (double)bits_to_float(in);
        bool ok = true;
        switch (routine) {
        case rtm::kExp: ok = within_ulps(bits_to_float(w[k]), exp(x), ulps); break;
        case rtm::kPow5: ok = within_ulps(bits_to_float(w[k]), pow(x, 5.0), ulps); break;
        case rtm::kAcos: ok = within_ulps(bits_to_float(w[k]), acos(x), ulps); break;
        case rtm::kAtan: ok = within_ulps(bits_to_float(w[k]), atan(x), ulps); break;
        case rtm::kAtan2: {
            float y2, x2;
            rtm::atan2_pair(in, y2, x2);
            ok = within_ulps(bits_to_float(w[k]), atan2((double)y2, (double)x2), ulps);
            break;
        }
        case rtm::kRng: {
            const double r = ldexp((double)orc_wang_hash(in), -32);
            ok = w[3 * k] == orc_wang_hash(in) && within_ulps(bits_to_float(w[3 * k + 1]), r, ulps) &&
                 within_ulps(bits_to_float(w[3 * k + 2]), -1.0 + 2.0 * (double)(float)r, ulps);
            break;
        }
        case rtm::kTonemap: {
            const double g = sqrt((double)bits_to_float(arg) * x);
            const double c = g != g ? 0.0 : g < 0.0 ? 0.0 : g > 0.999 ? 0.999 : g;
            const int want = (int)(256.0 * c), dev = ((const uint8_t *)got)[k];
            ok = dev - want <= 1 && want - dev <= 1;
            break;
        }
        default: ok = false;
        }
        bad += ok ? 0u : 1u;
    }
    *sampled = n;
    return bad;
}

}  // extern "C"
