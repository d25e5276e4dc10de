// rt_adaptive.hip.inc — the kernels of rt_render_adaptive (include/rtp_amd.h, "adaptive sampling"; DESIGN.md §11), included by
// rt_capi.hip after rt_kernel.hip.inc.  The samples themselves are traced by the existing kernels: the min_spp round is an ordinary
// rt_render frame, every later round the reference-order walk (render_kernel<kLds, true>) on a list of work indices, added onto the
// running sums by accumulate_kernel<true>.  These kernels keep the per-pixel luminance moments, apply the stopping rule, and turn
// the pixels that go on into that list.
namespace rtk {

constexpr int kAdaptBlock = 256;        // threads per workgroup of the moments and select kernels (one pixel per thread)

// the denoiser's lum (rtp_amd.h §denoising), of one sample's radiance
__device__ __forceinline__ float adapt_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// S1 += y, S2 += y * y for the `count` samples of one pass, in slot order, onto the moments (2 floats per local pixel: S1, S2) —
// from 0 when `first`.  kList: the pixels of a list whose length lives on the device (an adaptive round); else every local pixel
// (a pass of the min_spp round).  Pixels without a candidate leaf (primary visibility: cand[q * cand_stride] == 0) have no slab row:
// each of their samples is accumulate_kernel's sky_sample, 0 + 1 * background.  Each lane walks its own pixel's row with 16-byte
// loads, as accumulate_kernel<true> does.
template <bool kList>
__global__ void __launch_bounds__(kAdaptBlock) moments_kernel(float *mom, const float *slab, uint32_t num_pixels, uint32_t pitch, int32_t count,
                                                              int32_t first, const uint32_t *list, const uint32_t *list_count, const uint32_t *cand,
                                                              uint32_t cand_stride, float bg_r, float bg_g, float bg_b) {
    const uint32_t i = blockIdx.x * (uint32_t)kAdaptBlock + threadIdx.x;
    const uint32_t n = kList ? *list_count : num_pixels;
    if (i >= n) return;
    const uint32_t q = kList ? list[i] : i;
    float s1 = 0.0f, s2 = 0.0f;
    if (!first) { s1 = mom[2 * (size_t)q]; s2 = mom[2 * (size_t)q + 1]; }
    auto add_sample = [&](float r, float g, float b) {
        const float y = adapt_lum(r, g, b);
        s1 = s1 + y;
        s2 = s2 + y * y;
    };
    if (!kList && cand != nullptr && cand[(size_t)q * cand_stride] == 0u) {
        const f3 sky = add(mk(0.0f, 0.0f, 0.0f), mul(mk(1.0f, 1.0f, 1.0f), mk(bg_r, bg_g, bg_b)));
        for (int32_t s = 0; s < count; ++s) add_sample(sky.x, sky.y, sky.z);
    } else {
        const float *row = slab + (size_t)q * pitch * 3;
        int32_t s = 0;
        for (; s + 4 <= count; s += 4) {
            const float4 a = *reinterpret_cast<const float4 *>(row + 3 * s), b = *reinterpret_cast<const float4 *>(row + 3 * s + 4),
                         c = *reinterpret_cast<const float4 *>(row + 3 * s + 8);
            add_sample(a.x, a.y, a.z);
            add_sample(a.w, b.x, b.y);
            add_sample(b.z, b.w, c.x);
            add_sample(c.y, c.z, c.w);
        }
        for (; s < count; ++s) add_sample(row[3 * s], row[3 * s + 1], row[3 * s + 2]);
    }
    mom[2 * (size_t)q] = s1;
    mom[2 * (size_t)q + 1] = s2;
}

// The stopping rule (rtp_amd.h, rt_render_adaptive) for a pixel with n samples and moments (s1, s2): true = it goes on.
__device__ __forceinline__ bool adapt_goes_on(float s1, float s2, int32_t n, int32_t batch, int32_t max_spp, float t) {
    if (n + batch > max_spp) return false;
    if (t == 0.0f) return true;
    const float mean = s1 / (float)n;
    const float var = fmaxf(0.0f, (s2 - s1 * mean) / (float)(n - 1));
    return var / (float)n > (t * t) * (mean * mean + 1e-4f);
}

// One round's selection: the pixels of the previous round's list (kAll: every local pixel — after the min_spp round) that have
// n samples now are judged by the rule; those that go on are listed in list_out (one atomic per workgroup; the order of the list
// means nothing) and their count becomes n + batch.  kAll also writes n into the count of every pixel that stops.
template <bool kAll>
__global__ void __launch_bounds__(kAdaptBlock) adaptive_select_kernel(const float *mom, int32_t *spp, uint32_t num_pixels, const uint32_t *list_in,
                                                                      const uint32_t *count_in, uint32_t *list_out, uint32_t *count_out, int32_t n,
                                                                      int32_t batch, int32_t max_spp, float t) {
    __shared__ uint32_t wave_total[kAdaptBlock / kWave], block_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (uint32_t)kAdaptBlock + threadIdx.x;
    const uint32_t listed = kAll ? num_pixels : *count_in;
    bool on = false;
    uint32_t q = 0;
    if (i < listed) {
        q = kAll ? i : list_in[i];
        on = adapt_goes_on(mom[2 * (size_t)q], mom[2 * (size_t)q + 1], n, batch, max_spp, t);
        if (kAll || on) spp[q] = on ? n + batch : n;
    }
    const uint64_t m = __ballot(on);
    const uint32_t at = (uint32_t)lane_rank(m);
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kAdaptBlock / kWave; ++w) { const uint32_t c = wave_total[w]; wave_total[w] = sum; sum += c; }
        block_base = sum ? atomicAdd(count_out, sum) : 0u;
    }
    __syncthreads();
    if (on) list_out[block_base + wave_total[wave] + at] = q;
}

// ---- rule 1, the neighbourhood rule (rtp_amd.h, rt_render_adaptive_rule; DESIGN.md §22).  A judgement is two launches: the flag kernel
// writes c_p = "p is still going on and noisy" as one byte per pixel, the select kernel reads the up to 9 bytes of a pixel's window and
// builds the list.  No kernel both writes a pixel's byte and reads its neighbours': the launch boundary is the only ordering needed, and
// the result does not depend on how workgroups are scheduled.

// The buffer a judgement's window lives in: rows x width pixels, row-major; banded: rows r and r' are image neighbours only when
// r / band_rows == r' / band_rows (the compacted rows of a shard part: the next band of the buffer is not the next band of the image)
struct AdaptWindow {
    uint32_t width, rows, band_rows, banded;
};

// noisy_p of rule 1 for a pixel with n samples and moments (s1, s2); a NaN anywhere compares false
__device__ __forceinline__ bool adapt_noisy(float s1, float s2, int32_t n, float t) {
    const float mean = s1 / (float)n;
    const float var = fmaxf(0.0f, (s2 - s1 * mean) / (float)(n - 1));
    return var / (float)n > (t * t) * (mean + 0.01f);
}

// c of the pixels of the previous round's list (kAll: of every local pixel — after the min_spp round), which have n samples now.  A
// pixel that stopped earlier is not listed: it stopped with its whole window quiet, so its byte is 0 already and stays 0.
template <bool kAll>
__global__ void __launch_bounds__(kAdaptBlock) adaptive_flag_kernel(const float *mom, uint8_t *flag, uint32_t num_pixels, const uint32_t *list_in,
                                                                    const uint32_t *count_in, int32_t n, float t) {
    const uint32_t i = blockIdx.x * (uint32_t)kAdaptBlock + threadIdx.x;
    const uint32_t listed = kAll ? num_pixels : *count_in;
    if (i >= listed) return;
    const uint32_t q = kAll ? i : list_in[i];
    flag[q] = adapt_noisy(mom[2 * (size_t)q], mom[2 * (size_t)q + 1], n, t) ? (uint8_t)1 : (uint8_t)0;
}

// adaptive_select_kernel under rule 1: a listed pixel goes on iff the cap allows it and some byte of its window is set.  The window is
// the pixel's 3 x 3 clipped to the buffer — columns max(col - 1, 0) … min(col + 1, width - 1), and of the rows above and below those
// that exist and lie in the pixel's band — so every byte read has row < rows and column < width: an index below width x rows.
template <bool kAll>
__global__ void __launch_bounds__(kAdaptBlock) adaptive_select_near_kernel(const uint8_t *flag, int32_t *spp, uint32_t num_pixels, AdaptWindow W,
                                                                           const uint32_t *list_in, const uint32_t *count_in, uint32_t *list_out,
                                                                           uint32_t *count_out, int32_t n, int32_t batch, int32_t max_spp) {
    __shared__ uint32_t wave_total[kAdaptBlock / kWave], block_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (uint32_t)kAdaptBlock + threadIdx.x;
    const uint32_t listed = kAll ? num_pixels : *count_in;
    bool on = false;
    uint32_t q = 0;
    if (i < listed) {
        q = kAll ? i : list_in[i];
        if (n + batch <= max_spp) {
            const uint32_t row = q / W.width, col = q - row * W.width;
            const uint32_t c0 = col > 0u ? col - 1u : 0u, c1 = col + 1u < W.width ? col + 1u : col;
            const uint32_t band = W.banded ? row / W.band_rows : 0u;
            const uint32_t r0 = row > 0u && (!W.banded || (row - 1u) / W.band_rows == band) ? row - 1u : row;
            const uint32_t r1 = row + 1u < W.rows && (!W.banded || (row + 1u) / W.band_rows == band) ? row + 1u : row;
            for (uint32_t r = r0; r <= r1; ++r)
                for (uint32_t c = c0; c <= c1; ++c) on = on || flag[(size_t)r * W.width + c] != 0;
        }
        if (kAll || on) spp[q] = on ? n + batch : n;
    }
    const uint64_t m = __ballot(on);
    const uint32_t at = (uint32_t)lane_rank(m);
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kAdaptBlock / kWave; ++w) { const uint32_t c = wave_total[w]; wave_total[w] = sum; sum += c; }
        block_base = sum ? atomicAdd(count_out, sum) : 0u;
    }
    __syncthreads();
    if (on) list_out[block_base + wave_total[wave] + at] = q;
}

// ---- the rules with a prior (rtp_amd.h, rt_render_adaptive_prior; DESIGN.md §26).  prior: (ch, vh) per local pixel, the samples behind
// the pixel's reprojected history and the variance of its mean luminance (rt_adaptive_prior).  The rules compare ve, the variance
// rt_denoise_temporal_spp's blend of that history with this frame will carry, where the kernels above compare vm = var / n.  They are
// kernels of their own, not a template parameter of those above, so that those keep their arguments and their instructions.

// ve of a pixel with n samples (nf = (float)n) whose own samples give vm; a prior that is not (ch > 0, vh >= 0) — a NaN included — is none
__device__ __forceinline__ float adapt_blended_variance(float vm, float nf, float ch, float vh) {
    if (!(ch > 0.0f && vh >= 0.0f)) return vm;
    const float s = ch + nf;
    float a = nf / s;
    if (!(a >= 0.2f)) a = 0.2f;
    const float b = 1.0f - a;
    return (b * b) * vh + (a * a) * vm;
}

// mean and ve of local pixel q with n samples
__device__ __forceinline__ float adapt_prior_variance(const float *mom, const float *prior, uint32_t q, int32_t n, float &mean) {
    const float s1 = mom[2 * (size_t)q], s2 = mom[2 * (size_t)q + 1], nf = (float)n;
    mean = s1 / nf;
    const float var = fmaxf(0.0f, (s2 - s1 * mean) / (float)(n - 1));
    return adapt_blended_variance(var / nf, nf, prior[2 * (size_t)q], prior[2 * (size_t)q + 1]);
}

// adaptive_select_kernel with a prior (rule 0)
template <bool kAll>
__global__ void __launch_bounds__(kAdaptBlock) adaptive_select_prior_kernel(const float *mom, const float *prior, int32_t *spp, uint32_t num_pixels,
                                                                            const uint32_t *list_in, const uint32_t *count_in, uint32_t *list_out,
                                                                            uint32_t *count_out, int32_t n, int32_t batch, int32_t max_spp, float t) {
    __shared__ uint32_t wave_total[kAdaptBlock / kWave], block_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (uint32_t)kAdaptBlock + threadIdx.x;
    const uint32_t listed = kAll ? num_pixels : *count_in;
    bool on = false;
    uint32_t q = 0;
    if (i < listed) {
        q = kAll ? i : list_in[i];
        if (n + batch <= max_spp) {
            on = t == 0.0f;
            if (!on) {
                float mean;
                const float ve = adapt_prior_variance(mom, prior, q, n, mean);
                on = ve > (t * t) * (mean * mean + 1e-4f);
            }
        }
        if (kAll || on) spp[q] = on ? n + batch : n;
    }
    const uint64_t m = __ballot(on);
    const uint32_t at = (uint32_t)lane_rank(m);
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kAdaptBlock / kWave; ++w) { const uint32_t c = wave_total[w]; wave_total[w] = sum; sum += c; }
        block_base = sum ? atomicAdd(count_out, sum) : 0u;
    }
    __syncthreads();
    if (on) list_out[block_base + wave_total[wave] + at] = q;
}

// adaptive_flag_kernel with a prior (rule 1): noisy_p compares ve.  adaptive_select_near_kernel reads the bytes as it is.
template <bool kAll>
__global__ void __launch_bounds__(kAdaptBlock) adaptive_flag_prior_kernel(const float *mom, const float *prior, uint8_t *flag, uint32_t num_pixels,
                                                                          const uint32_t *list_in, const uint32_t *count_in, int32_t n, float t) {
    const uint32_t i = blockIdx.x * (uint32_t)kAdaptBlock + threadIdx.x;
    const uint32_t listed = kAll ? num_pixels : *count_in;
    if (i >= listed) return;
    const uint32_t q = kAll ? i : list_in[i];
    float mean;
    const float ve = adapt_prior_variance(mom, prior, q, n, mean);
    flag[q] = ve > (t * t) * (mean + 0.01f) ? (uint8_t)1 : (uint8_t)0;
}

// The list of a round → the work indices of its trace launch, q * batch + slot for slot = 0 … batch - 1 (the pass's own numbering:
// local pixel * pass_count + slot), and their number.  count * batch stays below 2^31 - 4096 (rt_render_adaptive checks
// num_pixels * batch).  Grid-stride: a round whose list is empty costs one short launch.
__global__ void __launch_bounds__(kAdaptBlock) adaptive_expand_kernel(const uint32_t *list, const uint32_t *count, uint32_t batch, uint32_t *work,
                                                                      uint32_t *work_count) {
    const uint32_t total = *count * batch;
    if (blockIdx.x == 0 && threadIdx.x == 0) *work_count = total;
    const uint32_t stride = gridDim.x * (uint32_t)kAdaptBlock;
    for (uint32_t k = blockIdx.x * (uint32_t)kAdaptBlock + threadIdx.x; k < total; k += stride) {
        const uint32_t e = k / batch;
        work[k] = list[e] * batch + (k - e * batch);
    }
}

// rt_tonemap with a divisor per pixel: float k of the frame belongs to pixel k / 3, whose divisor is spp[k / 3]
__global__ void tonemap_spp_kernel(const float *fb, const int32_t *spp, uint8_t *out, int64_t n) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < n; k += stride) {
        const float inv = (float)(1.0 / (double)(float)spp[k / 3]);
        out[k] = tonemap_u8(fb[k], inv);
    }
}

}  // namespace rtk
