// rt_math_check.hip — developer build only (make dev → librtp_amd_dev.so): rt_debug_math_eval, which runs one routine of
// rt_device_math.h on the device over consecutive inputs so that tests/dev_math_checks.py can compare every result bit with
// the host libm and the oracle.  A translation unit of its own, so the shipped library and its kernels are untouched.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/rtp_amd.h"
#include "rt_math_check.h"

__attribute__((visibility("hidden"))) void rt_internal_set_error(const std::string &msg);      // rt_capi.hip

namespace rtm {

constexpr unsigned kBlocks = 4096, kThreads = 256;

__global__ void __launch_bounds__(kThreads) eval_kernel(int32_t routine, uint32_t first, uint64_t count, uint32_t arg, void *out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const float farg = bits_to_float(arg);
    uint32_t *w = (uint32_t *)out;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint32_t in = first + (uint32_t)k;
        const float x = bits_to_float(in);
        switch (routine) {
        case kExp: w[k] = float_to_bits(rtd::exp_libm(x)); break;
        case kPow5: w[k] = float_to_bits(rtd::pow5(x)); break;
        case kAcos: w[k] = float_to_bits(rtd::acos_libm(x)); break;
        case kAtan: w[k] = float_to_bits(rtd::atan_libm(x)); break;
        case kAtan2: {
            float y2, x2;
            atan2_pair(in, y2, x2);
            w[k] = float_to_bits(rtd::atan2_libm(y2, x2));
            break;
        }
        case kRng: {
            uint32_t s1 = in, s2 = in;
            const float r = rtd::random_float(s1), pm = rtd::random_pm1(s2);
            w[3 * k] = s1;
            w[3 * k + 1] = float_to_bits(r);
            w[3 * k + 2] = float_to_bits(pm);
            break;
        }
        case kTonemap: ((uint8_t *)out)[k] = rtd::tonemap_u8(x, farg); break;
        case kPow5Float: w[k] = float_to_bits(rtd::pow5_float(x)); break;
        case kLog: w[k] = float_to_bits(rtd::log_libm(x)); break;
        default: break;
        }
    }
}

__global__ void __launch_bounds__(kThreads) schlick_kernel(uint32_t first, uint64_t count, float r0, unsigned long long *out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    SchlickCounts c = {0, 0, 0, 0, 0};
    unsigned long long first_bad = ~0ull;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint64_t before = c.bad;
        schlick_check(first + (uint32_t)k, r0, c);
        if (c.bad != before && first_bad == ~0ull) first_bad = first + k;
    }
    atomicAdd(&out[0], (unsigned long long)c.bad);
    atomicAdd(&out[1], (unsigned long long)c.seen);
    atomicAdd(&out[2], (unsigned long long)c.near_undecided);
    atomicAdd(&out[3], (unsigned long long)c.random);
    atomicAdd(&out[4], (unsigned long long)c.random_undecided);
    if (first_bad != ~0ull) atomicMin(&out[5], first_bad);
}

}  // namespace rtm

extern "C" {

// rt_debug_math_eval (not part of the ABI header): routine `routine` (rtm::Routine) for the inputs first … first + count - 1,
// enqueued on `hip_stream`.  d_out is device memory the caller owns: count words (count x 3 for kRng, count bytes for kTonemap),
// or for kSchlick the rtm::kSchlickCounters u64 counters, which the call resets first.  arg: the bits of kTonemap's inv_divisor
// or of kSchlick's r0.  Inputs beyond 2^32 - 1 are refused.
rt_status rt_debug_math_eval(int32_t routine, uint32_t first, uint64_t count, uint32_t arg, void *d_out, void *hip_stream) {
    if (!d_out) {
        rt_internal_set_error("rt_debug_math_eval: null d_out");
        return RT_ERR_INVALID_ARG;
    }
    if (!rtm::is_routine(routine)) {
        rt_internal_set_error("rt_debug_math_eval: unknown routine " + std::to_string(routine));
        return RT_ERR_INVALID_ARG;
    }
    if (count == 0 || count > (1ull << 32) - first) {
        rt_internal_set_error("rt_debug_math_eval: count must be 1 … 2^32 - first");
        return RT_ERR_INVALID_ARG;
    }
    const hipStream_t stream = (hipStream_t)hip_stream;
    hipError_t e;
    if (routine == rtm::kSchlick) {
        unsigned long long *ctr = (unsigned long long *)d_out;
        e = hipMemsetAsync(ctr, 0, 5 * sizeof(unsigned long long), stream);
        if (e == hipSuccess) e = hipMemsetAsync(ctr + 5, 0xff, sizeof(unsigned long long), stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(rtm::schlick_kernel, dim3(rtm::kBlocks), dim3(rtm::kThreads), 0, stream, first, count,
                               rtm::bits_to_float(arg), ctr);
            e = hipGetLastError();
        }
    } else {
        hipLaunchKernelGGL(rtm::eval_kernel, dim3(rtm::kBlocks), dim3(rtm::kThreads), 0, stream, routine, first, count, arg, d_out);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        rt_internal_set_error(std::string("rt_debug_math_eval: ") + hipGetErrorString(e));
        return RT_ERR_HIP;
    }
    return RT_OK;
}

}  // extern "C"
