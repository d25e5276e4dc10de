// rt_denoise.hip — the edge-avoiding à-trous filter behind rt_denoise (include/rtp_amd.h, "denoising").
//
// Image-space kernels over buffers the caller owns; nothing here touches a scene handle or the render kernels.  The arithmetic is
// the header's, operation for operation (-ffp-contract=off, correctly rounded division and sqrt, exp_libm for expf), so the
// output is bit-identical to the C restatement in tests/cpu_native/denoise_ref.c.
//
// One lane per pixel, 64 x 4 pixels per workgroup (a wave is 64 consecutive pixels of one row).  The workspace holds four
// 16-byte records per pixel, read with one vector load each:
//     lv[0], lv[1]  (L0, L1, L2, var)   demodulated colour and its variance, ping-ponged between passes
//     nz            (n.x, n.y, n.z, z)  unit normal and depth; n.x = +inf marks a sky pixel (never a hit pixel's value, below)
//     dg            (d0, d1, d2, gz)    demodulation divisor and depth gradient: read by the pixel itself only
// Launches: prepass (→ lv[0], nz, dg) · moments (lv[0] → lv[1] with var, gz into dg) · one step per iteration, the last of which
// remodulates into d_out.  With iterations = 0 the prepass writes d_out itself.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rtp_amd.h"
#include "rt_device_math.h"

__attribute__((visibility("hidden"))) void rt_internal_set_error(const std::string &msg);      // rt_capi.hip

namespace rtdn {

constexpr int kTileW = 64, kTileH = 4;            // pixels per workgroup: 64 x 4 = 256 lanes
constexpr uint64_t kRecordBytes = 16, kRecords = 4, kAlign = 256;

// A hit pixel's n.x is N.x / sqrtf(len2): NaN when N.x is infinite (inf / inf), 0 when another component overflows len2, and
// bounded by |N.x| / sqrtf(N.x * N.x rounded) < 2^13 when len2 is tiny — never +inf.  So +inf in nz.x is the sky marker.
__device__ __forceinline__ bool is_sky(const float4 &nz) { return nz.x == __builtin_inff(); }

struct Image {
    int32_t width, height, tiles_x;
};

// The pixel of this lane; false for the lanes of a partial tile that lie outside the image.
__device__ __forceinline__ bool pixel_of(const Image im, int32_t &x, int32_t &y) {
    const int32_t tile = (int32_t)blockIdx.x;
    const int32_t ty = tile / im.tiles_x, tx = tile - ty * im.tiles_x;
    x = tx * kTileW + (int32_t)(threadIdx.x & (kTileW - 1));
    y = ty * kTileH + (int32_t)(threadIdx.x / kTileW);
    return x < im.width && y < im.height;
}

__device__ __forceinline__ float lum(float L0, float L1, float L2) { return (0.2126f * L0 + 0.7152f * L1) + 0.0722f * L2; }

__device__ __forceinline__ void copy3(float *out, const float *in, int64_t p) {
    out[3 * p] = in[3 * p];
    out[3 * p + 1] = in[3 * p + 1];
    out[3 * p + 2] = in[3 * p + 2];
}

struct Inputs {
    const float *fb, *albedo, *normal, *depth;
    const uint32_t *hits;
};

// Per pixel: demodulate, normalise the normal, average the depth.  out != nullptr (iterations = 0): remodulate straight into it.
__global__ __launch_bounds__(256) void denoise_prepass(Image im, Inputs in, float inv, float spp, float4 *lv, float4 *nz, float4 *dg,
                                                       float *out) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const uint32_t hits = in.hits[p];
    if (hits == 0) {
        if (out) copy3(out, in.fb, p);
        else nz[p] = make_float4(__builtin_inff(), 0.0f, 0.0f, 0.0f);
        return;
    }
    float L[3], d[3];
    for (int k = 0; k < 3; ++k) {
        const float c = in.fb[3 * p + k] * inv;
        const float a = in.albedo[3 * p + k] * inv;
        d[k] = fmaxf(a, 1e-3f);
        L[k] = c / d[k];
    }
    if (out) {
        for (int k = 0; k < 3; ++k) out[3 * p + k] = (L[k] * d[k]) * spp;
        return;
    }
    const float Nx = in.normal[3 * p], Ny = in.normal[3 * p + 1], Nz = in.normal[3 * p + 2];
    const float len2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
    float4 n = make_float4(0.0f, 0.0f, 0.0f, in.depth[p] / (float)hits);
    if (len2 != 0.0f) {
        const float len = rtd::sqrt_cr(len2);
        n.x = Nx / len;
        n.y = Ny / len;
        n.z = Nz / len;
    }
    lv[p] = make_float4(L[0], L[1], L[2], 0.0f);
    nz[p] = n;
    dg[p] = make_float4(d[0], d[1], d[2], 0.0f);
}

// The second prepass: the 3x3 luminance variance (lv_in → lv_out) and the depth gradient (into dg.w).
__global__ __launch_bounds__(256) void denoise_moments(Image im, const float4 *lv_in, const float4 *nz, float4 *dg, float4 *lv_out) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const float4 np = nz[p];
    if (is_sky(np)) return;
    float m1 = 0.0f, m2 = 0.0f, k = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int32_t yy = y + dy;
        if (yy < 0 || yy >= im.height) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int32_t xx = x + dx;
            if (xx < 0 || xx >= im.width) continue;
            const int64_t q = (int64_t)yy * im.width + xx;
            if (is_sky(nz[q])) continue;
            const float4 Lq = lv_in[q];
            const float l = lum(Lq.x, Lq.y, Lq.z);
            m1 += l;
            m2 += l * l;
            k += 1.0f;
        }
    }
    const float mean = m1 / k;
    const float var = fmaxf(0.0f, m2 / k - mean * mean);
    // depth gradient: the smaller one-sided difference per axis, +inf for a missing neighbour, 0 when both are missing
    const float inf = __builtin_inff();
    const bool right = x + 1 < im.width && !is_sky(nz[p + 1]), left = x > 0 && !is_sky(nz[p - 1]);
    const float gx = (right || left) ? fminf(right ? fabsf(nz[p + 1].w - np.w) : inf, left ? fabsf(np.w - nz[p - 1].w) : inf) : 0.0f;
    const bool below = y + 1 < im.height && !is_sky(nz[p + im.width]), above = y > 0 && !is_sky(nz[p - im.width]);
    const float gy = (below || above) ? fminf(below ? fabsf(nz[p + im.width].w - np.w) : inf, above ? fabsf(np.w - nz[p - im.width].w) : inf)
                                      : 0.0f;
    const float4 lp = lv_in[p];
    lv_out[p] = make_float4(lp.x, lp.y, lp.z, var);
    float4 g = dg[p];
    g.w = gx + gy;
    dg[p] = g;
}

struct Sigmas {
    float depth, luminance;
    int32_t squarings;
};

// One à-trous pass at step s: 25 taps p + s*(dx, dy).  kFinal: remodulate into out (sky pixels copy fb) instead of writing lv_out.
template <bool kFinal>
__global__ __launch_bounds__(256) void denoise_step(Image im, int32_t s, Sigmas sg, const float4 *lv_in, const float4 *nz, const float4 *dg,
                                                    float4 *lv_out, const float *fb, float spp, float *out) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const float4 np = nz[p];
    if (is_sky(np)) {
        if (kFinal) copy3(out, fb, p);
        return;
    }
    const float4 vp = lv_in[p];
    const float gz = dg[p].w;
    const float lp = lum(vp.x, vp.y, vp.z);
    const float rl = rtd::recip(sg.luminance * rtd::sqrt_cr(vp.w) + 1e-4f);
    float rz[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) rz[m] = rtd::recip((sg.depth * gz) * (float)(s * m) + 1e-4f);
    const float kern[3] = {0.375f, 0.25f, 0.0625f};
    float W = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, SV = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int32_t yy = y + dy * s;
        if (yy < 0 || yy >= im.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int32_t xx = x + dx * s;
            if (xx < 0 || xx >= im.width) continue;
            const int64_t q = (int64_t)yy * im.width + xx;
            const float4 nq = nz[q];
            if (is_sky(nq)) continue;
            const float4 vq = lv_in[q];
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const float h = kern[ax] * kern[ay];
            float wn = fmaxf(0.0f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
            for (int k = 0; k < sg.squarings; ++k) wn = wn * wn;
            const float e = fabsf(np.w - nq.w) * rz[ax + ay] + fabsf(lp - lum(vq.x, vq.y, vq.z)) * rl;
            const float w = (h * wn) * rtd::exp_libm(-e);
            W += w;
            S0 += w * vq.x;
            S1 += w * vq.y;
            S2 += w * vq.z;
            SV += (w * w) * vq.w;
        }
    }
    float4 r = vp;
    if (W != 0.0f) r = make_float4(S0 / W, S1 / W, S2 / W, SV / (W * W));
    if (kFinal) {
        const float4 d = dg[p];
        out[3 * p] = (r.x * d.x) * spp;
        out[3 * p + 1] = (r.y * d.y) * spp;
        out[3 * p + 2] = (r.z * d.z) * spp;
    } else {
        lv_out[p] = r;
    }
}

// [a, a + na) and [b, b + nb) share a byte
bool overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

rt_status fail(rt_status st, const std::string &msg) {
    rt_internal_set_error(msg);
    return st;
}

}  // namespace rtdn

extern "C" {

void rt_denoise_params_init(rt_denoise_params *p) {
    if (!p) return;
    p->struct_bytes = (uint32_t)sizeof(rt_denoise_params);
    p->iterations = 5;
    p->sigma_depth = 1.0f;
    p->sigma_luminance = 4.0f;
    p->normal_squarings = 7;
}

uint64_t rt_denoise_workspace_bytes(int32_t width, int32_t height) {
    if (width < 1 || height < 1) return 0;
    return (uint64_t)width * (uint64_t)height * rtdn::kRecords * rtdn::kRecordBytes + rtdn::kAlign;
}

rt_status rt_denoise(const float *d_fb_sum, const rt_aov_buffers *aov, int32_t width, int32_t height, int32_t samples_per_pixel,
                     const rt_denoise_params *params, void *d_workspace, uint64_t workspace_bytes, float *d_out, void *hip_stream) {
    using rtdn::fail;
    if (!d_fb_sum || !aov || !d_workspace || !d_out) return fail(RT_ERR_INVALID_ARG, "rt_denoise: null argument");
    // rt_aov_buffers grows: fields past struct_bytes count as NULL
    rt_aov_buffers b;
    rt_aov_buffers_init(&b);
    const uint32_t ab = aov->struct_bytes < sizeof(b) ? aov->struct_bytes : (uint32_t)sizeof(b);
    memcpy(&b, aov, ab);
    if (ab < offsetof(rt_aov_buffers, hit_count) + sizeof(b.hit_count) || !b.albedo_sum || !b.normal_sum || !b.depth_sum || !b.hit_count)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise: albedo_sum, normal_sum, depth_sum and hit_count are required");
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, "rt_denoise: width and height must be at least 1");
    if (samples_per_pixel < 1 || samples_per_pixel > 65536)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise: samples_per_pixel outside 1 … 65536");
    rt_denoise_params prm;
    rt_denoise_params_init(&prm);
    if (params) {
        if (params->struct_bytes < 8) return fail(RT_ERR_INVALID_ARG, "rt_denoise: rt_denoise_params.struct_bytes is not set (rt_denoise_params_init)");
        memcpy(&prm, params, params->struct_bytes < sizeof(prm) ? params->struct_bytes : sizeof(prm));
    }
    if (prm.iterations < 0 || prm.iterations > 8) return fail(RT_ERR_INVALID_ARG, "rt_denoise: iterations outside 0 … 8");
    if (!(prm.sigma_depth > 0.0f) || !isfinite(prm.sigma_depth)) return fail(RT_ERR_INVALID_ARG, "rt_denoise: sigma_depth must be positive and finite");
    if (!(prm.sigma_luminance > 0.0f) || !isfinite(prm.sigma_luminance))
        return fail(RT_ERR_INVALID_ARG, "rt_denoise: sigma_luminance must be positive and finite");
    if (prm.normal_squarings < 0 || prm.normal_squarings > 10) return fail(RT_ERR_INVALID_ARG, "rt_denoise: normal_squarings outside 0 … 10");
    const uint64_t pixels = (uint64_t)width * (uint64_t)height;
    if (pixels > (1ull << 24)) return fail(RT_ERR_UNSUPPORTED, "rt_denoise: more than 2^24 pixels");
    const uint64_t need = rt_denoise_workspace_bytes(width, height);
    if (workspace_bytes < need)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise: workspace_bytes below rt_denoise_workspace_bytes (" + std::to_string(need) + ")");
    const struct { const void *ptr; uint64_t bytes; } inputs[] = {
        {d_fb_sum, 12 * pixels}, {b.albedo_sum, 12 * pixels}, {b.normal_sum, 12 * pixels}, {b.depth_sum, 4 * pixels}, {b.hit_count, 4 * pixels}};
    for (const auto &in : inputs) {
        if (rtdn::overlap(d_out, 12 * pixels, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise: d_out overlaps an input");
        if (rtdn::overlap(d_workspace, need, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise: the workspace overlaps an input");
    }
    if (rtdn::overlap(d_out, 12 * pixels, d_workspace, need)) return fail(RT_ERR_INVALID_ARG, "rt_denoise: d_out overlaps the workspace");

    // ---- enqueue -------------------------------------------------------------------------------------------------------------
    const hipStream_t stream = (hipStream_t)hip_stream;
    float4 *base = (float4 *)(((uintptr_t)d_workspace + rtdn::kAlign - 1) & ~(uintptr_t)(rtdn::kAlign - 1));
    float4 *lv[2] = {base, base + pixels};
    float4 *nz = base + 2 * pixels, *dg = base + 3 * pixels;
    rtdn::Image im;
    im.width = width;
    im.height = height;
    im.tiles_x = (width + rtdn::kTileW - 1) / rtdn::kTileW;
    const uint32_t blocks = (uint32_t)im.tiles_x * (uint32_t)((height + rtdn::kTileH - 1) / rtdn::kTileH);
    const rtdn::Inputs in = {d_fb_sum, b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count};
    const float inv = (float)(1.0 / (double)samples_per_pixel);
    const float spp = (float)samples_per_pixel;
    const dim3 grid(blocks), block(rtdn::kTileW * rtdn::kTileH);
    auto launched = [](const char *what) -> rt_status {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        return RT_OK;
    };
    rt_status st;
    hipLaunchKernelGGL(rtdn::denoise_prepass, grid, block, 0, stream, im, in, inv, spp, lv[0], nz, dg, prm.iterations == 0 ? d_out : nullptr);
    if ((st = launched("denoise_prepass")) != RT_OK || prm.iterations == 0) return st;
    hipLaunchKernelGGL(rtdn::denoise_moments, grid, block, 0, stream, im, lv[0], nz, dg, lv[1]);
    if ((st = launched("denoise_moments")) != RT_OK) return st;
    const rtdn::Sigmas sg = {prm.sigma_depth, prm.sigma_luminance, prm.normal_squarings};
    for (int32_t i = 0; i < prm.iterations; ++i) {
        const float4 *src = lv[(i + 1) & 1];
        float4 *dst = lv[i & 1];
        if (i + 1 < prm.iterations) hipLaunchKernelGGL(rtdn::denoise_step<false>, grid, block, 0, stream, im, 1 << i, sg, src, nz, dg, dst, d_fb_sum, spp, d_out);
        else hipLaunchKernelGGL(rtdn::denoise_step<true>, grid, block, 0, stream, im, 1 << i, sg, src, nz, dg, dst, d_fb_sum, spp, d_out);
        if ((st = launched("denoise_step")) != RT_OK) return st;
    }
    return RT_OK;
}

}  // extern "C"
