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
//
// rt_denoise_temporal (SVGF's temporal half) runs the same kernels with one more between moments and the first step: denoise_temporal
// reprojects each hit pixel into the history of the previous frame and replaces lv[1] in place with the accumulated colour and the
// variance of the accumulated moments (or keeps the spatial one while the history is short).  The first step also writes its output
// into the history (kFeedback), the colour the next frame reprojects.  The history buffer is a 256-byte header, then four planes of
// one 16-byte record per pixel:
//     colour   (L0, L1, L2, var)     iteration 0's output (the accumulated colour itself with 0 iterations)
//     moments  (M1, M2, len, prim)   accumulated luminance moments, history length (0: sky), first_prim as its int32 bits
//     position (X, 0)                mean first-hit point
//     normal   (n, 0)                unit normal of the prepass
// With an empty history every pixel is disoccluded, denoise_temporal writes back what moments wrote, and d_out is rt_denoise's.
//
// rt_denoise_spp (adaptively sampled frames: a count per pixel) runs the same launches with three kernels of its own:
// denoise_prepass_spp normalises with the pixel's count and leaves the variance of its samples in lv.w, denoise_moments_spp replaces
// the 3x3 spatial variance by the 3x3 Gaussian of that (without moments: denoise_moments as it is), and denoise_step_spp is the last
// step remodulating with the pixel's count.  The taps (rt_denoise_taps.inc) and the depth gradient are one text, expanded in rt_denoise's kernels and in these.
//
// rt_denoise_temporal_spp (the two together) runs rt_denoise_spp's prepasses, then denoise_temporal_spp: denoise_temporal
// with the history and the frame weighed by the samples behind them and the variance of that blend carried along.  Its history has a
// magic of its own, the use of moments in the header's fourth word, the accumulated count in position.w and the propagated variance
// in normal.w.  With one iteration the step is first and last at once: denoise_step_spp_feedback.  The reprojection and the tap loop
// are one text (rt_denoise_reproject.inc) expanded in denoise_temporal and in denoise_temporal_spp, which hook their sums and blend in.
//
// rt_adaptive_prior is one kernel, adaptive_prior: that text a third time, over the frame's AOVs instead of a workspace,
// keeping the reprojected count and variance of a history of rt_denoise_temporal_spp for the stopping rule of the next adaptive frame.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

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

// rt_denoise_spp's prepass: denoise_prepass with the pixel's own count n = spp[p] under the beauty sums (the AOVs keep one count, inv_aov)
// and a count below 1 making the pixel sky.  With moments the sample variance of the mean luminance, in demodulated space, goes into
// lv.w for denoise_moments_spp (0 without: denoise_moments overwrites it).
__global__ __launch_bounds__(256) void denoise_prepass_spp(Image im, Inputs in, const int32_t *spp, const float *moments, float inv_aov, float4 *lv,
                                                           float4 *nz, float4 *dg, float *out) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const uint32_t hits = in.hits[p];
    const int32_t n = spp[p];
    if (hits == 0 || n < 1) {
        if (out) copy3(out, in.fb, p);
        else nz[p] = make_float4(__builtin_inff(), 0.0f, 0.0f, 0.0f);
        return;
    }
    const float inv = (float)(1.0 / (double)n), fn = (float)n;
    float L[3], d[3];
    for (int k = 0; k < 3; ++k) {
        const float c = in.fb[3 * p + k] * inv;
        const float a = in.albedo[3 * p + k] * inv_aov;
        d[k] = fmaxf(a, 1e-3f);
        L[k] = c / d[k];
    }
    if (out) {
        for (int k = 0; k < 3; ++k) out[3 * p + k] = (L[k] * d[k]) * fn;
        return;
    }
    float v = 0.0f;
    if (moments && n >= 2) {
        const float S1 = moments[2 * p], S2 = moments[2 * p + 1];
        const float mean = S1 / fn;
        const float vs = fmaxf(0.0f, (S2 - S1 * mean) / (float)(n - 1));
        const float vm = vs / fn;
        const float dl = lum(d[0], d[1], d[2]);
        v = vm / (dl * dl);
    }
    const float Nx = in.normal[3 * p], Ny = in.normal[3 * p + 1], Nz = in.normal[3 * p + 2];
    const float len2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
    float4 nrm = make_float4(0.0f, 0.0f, 0.0f, in.depth[p] / (float)hits);
    if (len2 != 0.0f) {
        const float len = rtd::sqrt_cr(len2);
        nrm.x = Nx / len;
        nrm.y = Ny / len;
        nrm.z = Nz / len;
    }
    lv[p] = make_float4(L[0], L[1], L[2], v);
    nz[p] = nrm;
    dg[p] = make_float4(d[0], d[1], d[2], 0.0f);
}

// The depth gradient of hit pixel p = (x, y) with record np, as the statements of the kernel that uses it (a helper function moved
// denoise_moments' instructions; this text is its old one): the smaller one-sided difference per axis, +inf for a missing neighbour,
// 0 when both are missing.  Defines gx and gy.
#define RTP_DENOISE_DEPTH_GRADIENT                                                                                                        \
    const float inf = __builtin_inff();                                                                                                   \
    const bool right = x + 1 < im.width && !is_sky(nz[p + 1]), left = x > 0 && !is_sky(nz[p - 1]);                                        \
    const float gx = (right || left) ? fminf(right ? fabsf(nz[p + 1].w - np.w) : inf, left ? fabsf(np.w - nz[p - 1].w) : inf) : 0.0f;     \
    const bool below = y + 1 < im.height && !is_sky(nz[p + im.width]), above = y > 0 && !is_sky(nz[p - im.width]);                        \
    const float gy = (below || above) ? fminf(below ? fabsf(nz[p + im.width].w - np.w) : inf, above ? fabsf(np.w - nz[p - im.width].w) : inf) \
                                      : 0.0f;

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
    RTP_DENOISE_DEPTH_GRADIENT
    const float4 lp = lv_in[p];
    lv_out[p] = make_float4(lp.x, lp.y, lp.z, var);
    float4 g = dg[p];
    g.w = gx + gy;
    dg[p] = g;
}

// rt_denoise_spp's second prepass with moments: the 3x3 Gaussian of the sample variance the prepass left in lv.w, and the depth
// gradient as above.
__global__ __launch_bounds__(256) void denoise_moments_spp(Image im, const float4 *lv_in, const float4 *nz, float4 *dg, float4 *lv_out) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const float4 np = nz[p];
    if (is_sky(np)) return;
    const float kern[2] = {0.5f, 0.25f};
    float G = 0.0f, SV = 0.0f;
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
            const float g = kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy];
            G += g;
            SV += g * lv_in[q].w;
        }
    }
    RTP_DENOISE_DEPTH_GRADIENT
    const float4 lp = lv_in[p];
    lv_out[p] = make_float4(lp.x, lp.y, lp.z, SV / G);
    float4 g = dg[p];
    g.w = gx + gy;
    dg[p] = g;
}

struct Sigmas {
    float depth, luminance;
    int32_t squarings;
};

// One à-trous pass at step s: 25 taps p + s*(dx, dy).  kFinal: remodulate into out (sky pixels copy fb) instead of writing lv_out.
// kFeedback: also write the result into the colour plane of the temporal history (rt_denoise_temporal's first iteration).
template <bool kFinal, bool kFeedback = false>
__global__ __launch_bounds__(256) void denoise_step(Image im, int32_t s, Sigmas sg, const float4 *lv_in, const float4 *nz, const float4 *dg,
                                                    float4 *lv_out, const float *fb, float spp, float *out, float4 *feedback = nullptr) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const float4 np = nz[p];
    if (is_sky(np)) {
        if (kFinal) copy3(out, fb, p);
        return;
    }
#include "rt_denoise_taps.inc"
    if (kFeedback) feedback[p] = r;
    if (kFinal) {
        const float4 d = dg[p];
        out[3 * p] = (r.x * d.x) * spp;
        out[3 * p + 1] = (r.y * d.y) * spp;
        out[3 * p + 2] = (r.z * d.z) * spp;
    } else {
        lv_out[p] = r;
    }
}

// rt_denoise_spp's last pass: denoise_step<true> remodulating with the pixel's own sample count
__global__ __launch_bounds__(256) void denoise_step_spp(Image im, int32_t s, Sigmas sg, const float4 *lv_in, const float4 *nz, const float4 *dg,
                                                        const float *fb, const int32_t *spp, float *out) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const float4 np = nz[p];
    if (is_sky(np)) {
        copy3(out, fb, p);
        return;
    }
#include "rt_denoise_taps.inc"
    const float4 d = dg[p];
    const float n = (float)spp[p];
    out[3 * p] = (r.x * d.x) * n;
    out[3 * p + 1] = (r.y * d.y) * n;
    out[3 * p + 2] = (r.z * d.z) * n;
}

// rt_denoise_temporal_spp's only pass when iterations = 1: denoise_step_spp that also writes its result into the history's colour plane
__global__ __launch_bounds__(256) void denoise_step_spp_feedback(Image im, int32_t s, Sigmas sg, const float4 *lv_in, const float4 *nz, const float4 *dg,
                                                                 const float *fb, const int32_t *spp, float *out, float4 *feedback) {
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const float4 np = nz[p];
    if (is_sky(np)) {
        copy3(out, fb, p);
        return;
    }
#include "rt_denoise_taps.inc"
    feedback[p] = r;
    const float4 d = dg[p];
    const float n = (float)spp[p];
    out[3 * p] = (r.x * d.x) * n;
    out[3 * p + 1] = (r.y * d.y) * n;
    out[3 * p + 2] = (r.z * d.z) * n;
}

// ---- the temporal half (rt_denoise_temporal) ------------------------------------------------------------------------------------

constexpr uint32_t kHistMagic = 0x31485452u;          // "RTH1"
constexpr uint32_t kHistMagicSpp = 0x32485452u;       // "RTH2": rt_denoise_temporal_spp's histories
constexpr uint32_t kModeSpatial = 1, kModeMoments = 2;   // their fourth word: written without / with d_moments
constexpr uint64_t kHistHeader = 256, kHistPlanes = 4;
constexpr float kTau2 = 0.0025f, kMinWeight = 0.01f, kMaxLen = 32.0f, kMinAlpha = 0.2f, kMomentsLen = 4.0f, kMinNormalDot = 0.9f;

struct History {            // the header: written by denoise_temporal's first lane, read by all of them
    uint32_t magic;
    int32_t width, height;
    uint32_t mode;          // 0 (rt_denoise_temporal), kModeSpatial or kModeMoments (rt_denoise_temporal_spp)
    rt_camera_data cam;     // the camera the history was made with
    uint32_t zeros[(kHistHeader - 16 - sizeof(rt_camera_data)) / 4];
};
static_assert(sizeof(History) == kHistHeader, "history header");

// plane k of a history buffer (16-byte aligned: checked by the caller)
__host__ __device__ __forceinline__ float4 *plane(void *h, uint64_t pixels, int k) {
    return (float4 *)((char *)h + kHistHeader) + (uint64_t)k * pixels;
}

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Per pixel, after moments: reproject into the history of `prev`, accumulate (L, M1, M2) and write (L, var) back into lv in place;
// write the pixel's history records into `next`.  out != nullptr (iterations = 0): remodulate straight into it, and the colour plane
// of the history gets (L, var) here instead of from the first step.
__global__ __launch_bounds__(256) void denoise_temporal(Image im, rt_camera_data cam, const int32_t *first_prim, const History *prev, History *next,
                                                        float4 *lv, const float4 *nz, const float4 *dg, const float *fb, float spp, float *out) {
    const uint64_t pixels = (uint64_t)im.width * (uint64_t)im.height;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        History h;
        memset(&h, 0, sizeof(h));
        h.magic = kHistMagic;
        h.width = im.width;
        h.height = im.height;
        h.cam = cam;
        *next = h;
    }
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    float4 *const colour = plane(next, pixels, 0);
    const float4 np = nz[p];
    if (is_sky(np)) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        colour[p] = zero;
        plane(next, pixels, 1)[p] = zero;
        plane(next, pixels, 2)[p] = zero;
        plane(next, pixels, 3)[p] = zero;
        if (out) copy3(out, fb, p);
        return;
    }
    const float4 cur = lv[p];
    const int32_t prim = first_prim[p];
    const float Lc[3] = {cur.x, cur.y, cur.z};
    const float m1 = lum(cur.x, cur.y, cur.z);
#define RTP_REPROJECT_STATE float L[3] = {Lc[0], Lc[1], Lc[2]}, M1 = m1, M2 = m1 * m1, len = 1.0f;
#define RTP_REPROJECT_HISTORY_OK prev && prev->magic == kHistMagic && prev->width == im.width && prev->height == im.height
#define RTP_REPROJECT_SUMS
#define RTP_REPROJECT_TAP
#define RTP_REPROJECT_ALPHA const float a = fmaxf(kMinAlpha, 1.0f / len), b = 1.0f - a;
#define RTP_REPROJECT_VARIANCE
#include "rt_denoise_reproject.inc"
#undef RTP_REPROJECT_STATE
#undef RTP_REPROJECT_HISTORY_OK
#undef RTP_REPROJECT_SUMS
#undef RTP_REPROJECT_TAP
#undef RTP_REPROJECT_ALPHA
#undef RTP_REPROJECT_VARIANCE
    const float var = len >= kMomentsLen ? fmaxf(0.0f, M2 - M1 * M1) : cur.w;
    const float4 r = make_float4(L[0], L[1], L[2], var);
    lv[p] = r;
    plane(next, pixels, 1)[p] = make_float4(M1, M2, len, __int_as_float(prim));
    plane(next, pixels, 2)[p] = make_float4(X[0], X[1], X[2], 0.0f);
    plane(next, pixels, 3)[p] = make_float4(np.x, np.y, np.z, 0.0f);
    if (out) {
        colour[p] = r;
        const float4 d = dg[p];
        out[3 * p] = (L[0] * d.x) * spp;
        out[3 * p + 1] = (L[1] * d.y) * spp;
        out[3 * p + 2] = (L[2] * d.z) * spp;
    }
}

// rt_denoise_temporal_spp's temporal pass: denoise_temporal's reprojection (rt_denoise_reproject.inc, expanded in both) with the
// blend weighed by sample counts (n = spp[p] against the count the history carries in position.w), the variance of that blend
// propagated (normal.w) and steering the iterations when the frames come with moments (mode 2; mode 1: the accumulated moments as in
// denoise_temporal), and the pixel's count in the remodulation.
__global__ __launch_bounds__(256) void denoise_temporal_spp(Image im, rt_camera_data cam, const int32_t *first_prim, const int32_t *spp, uint32_t mode,
                                                            const History *prev, History *next, float4 *lv, const float4 *nz, const float4 *dg,
                                                            const float *fb, float *out) {
    const uint64_t pixels = (uint64_t)im.width * (uint64_t)im.height;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        History h;
        memset(&h, 0, sizeof(h));
        h.magic = kHistMagicSpp;
        h.width = im.width;
        h.height = im.height;
        h.mode = mode;
        h.cam = cam;
        *next = h;
    }
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    float4 *const colour = plane(next, pixels, 0);
    const float4 np = nz[p];
    if (is_sky(np)) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        colour[p] = zero;
        plane(next, pixels, 1)[p] = zero;
        plane(next, pixels, 2)[p] = zero;
        plane(next, pixels, 3)[p] = zero;
        if (out) copy3(out, fb, p);
        return;
    }
    const float4 cur = lv[p];
    const int32_t prim = first_prim[p];
    const float nf = (float)spp[p];
    const float Lc[3] = {cur.x, cur.y, cur.z};
    const float m1 = lum(cur.x, cur.y, cur.z);
#define RTP_REPROJECT_STATE float L[3] = {Lc[0], Lc[1], Lc[2]}, M1 = m1, M2 = m1 * m1, len = 1.0f, cnt = nf, V = cur.w;
#define RTP_REPROJECT_HISTORY_OK prev && prev->magic == kHistMagicSpp && prev->width == im.width && prev->height == im.height && prev->mode == mode
#define RTP_REPROJECT_SUMS float SC = 0.0f, SV = 0.0f;
#define RTP_REPROJECT_TAP SC += w * xq.w, SV += w * nq.w;
#define RTP_REPROJECT_ALPHA                       \
    const float ch = SC / W, s = ch + nf;         \
    float a = nf / s;                             \
    cnt = s;                                      \
    if (!(a >= kMinAlpha)) {                      \
        a = kMinAlpha;                            \
        cnt = nf / kMinAlpha;                     \
    }                                             \
    const float b = 1.0f - a;
#define RTP_REPROJECT_VARIANCE V = (b * b) * (SV / W) + (a * a) * cur.w;
#include "rt_denoise_reproject.inc"
#undef RTP_REPROJECT_STATE
#undef RTP_REPROJECT_HISTORY_OK
#undef RTP_REPROJECT_SUMS
#undef RTP_REPROJECT_TAP
#undef RTP_REPROJECT_ALPHA
#undef RTP_REPROJECT_VARIANCE
    const float var = mode == kModeMoments ? V : (len >= kMomentsLen ? fmaxf(0.0f, M2 - M1 * M1) : cur.w);
    const float4 r = make_float4(L[0], L[1], L[2], var);
    lv[p] = r;
    plane(next, pixels, 1)[p] = make_float4(M1, M2, len, __int_as_float(prim));
    plane(next, pixels, 2)[p] = make_float4(X[0], X[1], X[2], cnt);
    plane(next, pixels, 3)[p] = make_float4(np.x, np.y, np.z, V);
    if (out) {
        colour[p] = r;
        const float4 d = dg[p];
        out[3 * p] = (L[0] * d.x) * nf;
        out[3 * p + 1] = (L[1] * d.y) * nf;
        out[3 * p + 2] = (L[2] * d.z) * nf;
    }
}

// rt_adaptive_prior: what the history holds for each pixel of the frame about to be rendered — the samples behind it
// (ch) and the variance of its mean luminance in the frame's own space (vh) — for the stopping rules of the _prior calls.  The frame's
// AOVs stand in for the prepass (n, z, d as denoise_prepass_spp makes them); the reprojection is denoise_temporal_spp's
// (rt_denoise_reproject.inc) with a third set of hooks that keeps cnt and V alone: nothing is blended, so the colour plane's loads and
// the sums over it are dead and the compiler drops them.  Reads the moments, normal and position planes; writes 2 floats per pixel.
__global__ __launch_bounds__(256) void adaptive_prior(Image im, rt_camera_data cam, Inputs in, const int32_t *first_prim, float inv_aov,
                                                      const History *prev, float *prior) {
    const uint64_t pixels = (uint64_t)im.width * (uint64_t)im.height;
    int32_t x, y;
    if (!pixel_of(im, x, y)) return;
    const int64_t p = (int64_t)y * im.width + x;
    const uint32_t hits = in.hits[p];
    if (hits == 0) {
        prior[2 * p] = 0.0f;
        prior[2 * p + 1] = 0.0f;
        return;
    }
    float d[3];
    for (int k = 0; k < 3; ++k) d[k] = fmaxf(in.albedo[3 * p + k] * inv_aov, 1e-3f);
    const float dl = lum(d[0], d[1], d[2]);
    const float Nx = in.normal[3 * p], Ny = in.normal[3 * p + 1], Nz = in.normal[3 * p + 2];
    const float len2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
    float4 np = make_float4(0.0f, 0.0f, 0.0f, in.depth[p] / (float)hits);
    if (len2 != 0.0f) {
        const float nl = rtd::sqrt_cr(len2);
        np.x = Nx / nl;
        np.y = Ny / nl;
        np.z = Nz / nl;
    }
    const int32_t prim = first_prim[p];
    const float Lc[3] = {0.0f, 0.0f, 0.0f}, m1 = 0.0f;          // (no colour here: what the shared text blends is not kept)
#define RTP_REPROJECT_STATE float L[3], M1, M2, len, ch = 0.0f, vh = 0.0f;
#define RTP_REPROJECT_HISTORY_OK prev && prev->magic == kHistMagicSpp && prev->width == im.width && prev->height == im.height && prev->mode == kModeMoments
#define RTP_REPROJECT_SUMS float SC = 0.0f, SV = 0.0f;
#define RTP_REPROJECT_TAP SC += w * xq.w, SV += w * nq.w;
#define RTP_REPROJECT_ALPHA const float a = 0.0f, b = 0.0f;
#define RTP_REPROJECT_VARIANCE  \
    (void)L, (void)M1, (void)M2; \
    ch = SC / W;                 \
    vh = (SV / W) * (dl * dl);
#include "rt_denoise_reproject.inc"
#undef RTP_REPROJECT_STATE
#undef RTP_REPROJECT_HISTORY_OK
#undef RTP_REPROJECT_SUMS
#undef RTP_REPROJECT_TAP
#undef RTP_REPROJECT_ALPHA
#undef RTP_REPROJECT_VARIANCE
    (void)len;
    prior[2 * p] = ch;
    prior[2 * p + 1] = vh;
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

// params (NULL = defaults) into prm, checked; errors start with `who`
rt_status read_params(const char *who, const rt_denoise_params *params, rt_denoise_params &prm) {
    const std::string w(who);
    rt_denoise_params_init(&prm);
    if (params) {
        if (params->struct_bytes < 8) return fail(RT_ERR_INVALID_ARG, w + ": rt_denoise_params.struct_bytes is not set (rt_denoise_params_init)");
        memcpy(&prm, params, params->struct_bytes < sizeof(prm) ? params->struct_bytes : sizeof(prm));
    }
    if (prm.iterations < 0 || prm.iterations > 8) return fail(RT_ERR_INVALID_ARG, w + ": iterations outside 0 … 8");
    if (!(prm.sigma_depth > 0.0f) || !isfinite(prm.sigma_depth)) return fail(RT_ERR_INVALID_ARG, w + ": sigma_depth must be positive and finite");
    if (!(prm.sigma_luminance > 0.0f) || !isfinite(prm.sigma_luminance))
        return fail(RT_ERR_INVALID_ARG, w + ": sigma_luminance must be positive and finite");
    if (prm.normal_squarings < 0 || prm.normal_squarings > 10) return fail(RT_ERR_INVALID_ARG, w + ": normal_squarings outside 0 … 10");
    return RT_OK;
}

// The launch shape of a width x height image (one lane per pixel, kTileW x kTileH pixels per workgroup) and the workspace planes
struct Launch {
    Image im;
    dim3 grid, block;
    float4 *lv[2], *nz, *dg;
    Launch(int32_t width, int32_t height, void *workspace) {
        const uint64_t pixels = (uint64_t)width * (uint64_t)height;
        float4 *base = (float4 *)(((uintptr_t)workspace + kAlign - 1) & ~(uintptr_t)(kAlign - 1));
        lv[0] = base;
        lv[1] = base + pixels;
        nz = base + 2 * pixels;
        dg = base + 3 * pixels;
        im.width = width;
        im.height = height;
        im.tiles_x = (width + kTileW - 1) / kTileW;
        grid = dim3((uint32_t)im.tiles_x * (uint32_t)((height + kTileH - 1) / kTileH));
        block = dim3(kTileW * kTileH);
    }
};

rt_status launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return RT_OK;
}

// The iterations: lv[1] → lv[0] → lv[1] …, the last one remodulating into out; feedback != nullptr: iteration 0 also writes it;
// d_spp != nullptr (rt_denoise_spp, rt_denoise_temporal_spp): the last one remodulates with each pixel's own count instead of spp
rt_status enqueue_steps(const Launch &l, const rt_denoise_params &prm, const float *fb, float spp, float *out, float4 *feedback, hipStream_t stream,
                        const int32_t *d_spp = nullptr) {
    const Sigmas sg = {prm.sigma_depth, prm.sigma_luminance, prm.normal_squarings};
    for (int32_t i = 0; i < prm.iterations; ++i) {
        const float4 *src = l.lv[(i + 1) & 1];
        float4 *dst = l.lv[i & 1];
        const bool last = i + 1 == prm.iterations;
        if (i == 0 && feedback && last && d_spp) {
            hipLaunchKernelGGL(denoise_step_spp_feedback, l.grid, l.block, 0, stream, l.im, 1 << i, sg, src, l.nz, l.dg, fb, d_spp, out, feedback);
        } else if (i == 0 && feedback) {
            if (!last) hipLaunchKernelGGL((denoise_step<false, true>), l.grid, l.block, 0, stream, l.im, 1 << i, sg, src, l.nz, l.dg, dst, fb, spp, out, feedback);
            else hipLaunchKernelGGL((denoise_step<true, true>), l.grid, l.block, 0, stream, l.im, 1 << i, sg, src, l.nz, l.dg, dst, fb, spp, out, feedback);
        } else if (last && d_spp) {
            hipLaunchKernelGGL(denoise_step_spp, l.grid, l.block, 0, stream, l.im, 1 << i, sg, src, l.nz, l.dg, fb, d_spp, out);
        } else if (!last) {
            hipLaunchKernelGGL(denoise_step<false>, l.grid, l.block, 0, stream, l.im, 1 << i, sg, src, l.nz, l.dg, dst, fb, spp, out, nullptr);
        } else {
            hipLaunchKernelGGL(denoise_step<true>, l.grid, l.block, 0, stream, l.im, 1 << i, sg, src, l.nz, l.dg, dst, fb, spp, out, nullptr);
        }
        rt_status st;
        if ((st = launched("denoise_step")) != RT_OK) return st;
    }
    return RT_OK;
}

// d_out = a + d_out per channel (rt_denoise_split: one float32 add of the two filtered components)
__global__ __launch_bounds__(256) void denoise_add(const float *a, float *out, uint32_t floats) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < floats) out[k] = a[k] + out[k];
}

// rt_denoise's checks, in its order, for a call `who` with nfb beauty inputs and a workspace of `need` bytes → the AOV buffers and parameters
rt_status denoise_checks(const char *who, const float *const *fbs, int nfb, const rt_aov_buffers *aov, int32_t width, int32_t height, int32_t samples_per_pixel,
                         const rt_denoise_params *params, const void *d_workspace, uint64_t workspace_bytes, uint64_t need, const float *d_out,
                         rt_aov_buffers &b, rt_denoise_params &prm) {
    const std::string w(who);
    for (int k = 0; k < nfb; ++k)
        if (!fbs[k]) return fail(RT_ERR_INVALID_ARG, w + ": null argument");
    if (!aov || !d_workspace || !d_out) return fail(RT_ERR_INVALID_ARG, w + ": null argument");
    // rt_aov_buffers grows: fields past struct_bytes count as NULL
    rt_aov_buffers_init(&b);
    const uint32_t ab = aov->struct_bytes < sizeof(b) ? aov->struct_bytes : (uint32_t)sizeof(b);
    memcpy(&b, aov, ab);
    if (ab < offsetof(rt_aov_buffers, hit_count) + sizeof(b.hit_count) || !b.albedo_sum || !b.normal_sum || !b.depth_sum || !b.hit_count)
        return fail(RT_ERR_INVALID_ARG, w + ": albedo_sum, normal_sum, depth_sum and hit_count are required");
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, w + ": width and height must be at least 1");
    if (samples_per_pixel < 1 || samples_per_pixel > 65536) return fail(RT_ERR_INVALID_ARG, w + ": samples_per_pixel outside 1 … 65536");
    const rt_status st = read_params(who, params, prm);
    if (st != RT_OK) return st;
    const uint64_t pixels = (uint64_t)width * (uint64_t)height;
    if (pixels > (1ull << 24)) return fail(RT_ERR_UNSUPPORTED, w + ": more than 2^24 pixels");
    if (workspace_bytes < need) return fail(RT_ERR_INVALID_ARG, w + ": workspace_bytes below " + w + "_workspace_bytes (" + std::to_string(need) + ")");
    struct Input { const void *ptr; uint64_t bytes; };
    std::vector<Input> inputs;          // the beauty inputs first, as rt_denoise always checked them
    for (int k = 0; k < nfb; ++k) inputs.push_back({fbs[k], 12 * pixels});
    for (const Input &in : {Input{b.albedo_sum, 12 * pixels}, Input{b.normal_sum, 12 * pixels}, Input{b.depth_sum, 4 * pixels}, Input{b.hit_count, 4 * pixels}})
        inputs.push_back(in);
    for (const Input &in : inputs) {
        if (overlap(d_out, 12 * pixels, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, w + ": d_out overlaps an input");
        if (overlap(d_workspace, need, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, w + ": the workspace overlaps an input");
    }
    if (overlap(d_out, 12 * pixels, d_workspace, need)) return fail(RT_ERR_INVALID_ARG, w + ": d_out overlaps the workspace");
    return RT_OK;
}

// rt_denoise's launches on one beauty frame
rt_status denoise_enqueue(const float *d_fb_sum, const rt_aov_buffers &b, int32_t width, int32_t height, int32_t samples_per_pixel, const rt_denoise_params &prm,
                          void *d_workspace, float *d_out, hipStream_t stream) {
    const Launch l(width, height, d_workspace);
    const Inputs in = {d_fb_sum, b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count};
    const float inv = (float)(1.0 / (double)samples_per_pixel);
    const float spp = (float)samples_per_pixel;
    rt_status st;
    hipLaunchKernelGGL(denoise_prepass, l.grid, l.block, 0, stream, l.im, in, inv, spp, l.lv[0], l.nz, l.dg, prm.iterations == 0 ? d_out : nullptr);
    if ((st = launched("denoise_prepass")) != RT_OK || prm.iterations == 0) return st;
    hipLaunchKernelGGL(denoise_moments, l.grid, l.block, 0, stream, l.im, l.lv[0], l.nz, l.dg, l.lv[1]);
    if ((st = launched("denoise_moments")) != RT_OK) return st;
    return enqueue_steps(l, prm, d_fb_sum, spp, d_out, nullptr, stream);
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
    const float *fbs[1] = {d_fb_sum};
    rt_aov_buffers b;
    rt_denoise_params prm;
    const rt_status st = rtdn::denoise_checks("rt_denoise", fbs, 1, aov, width, height, samples_per_pixel, params, d_workspace, workspace_bytes,
                                              rt_denoise_workspace_bytes(width, height), d_out, b, prm);
    if (st != RT_OK) return st;
    return rtdn::denoise_enqueue(d_fb_sum, b, width, height, samples_per_pixel, prm, d_workspace, d_out, (hipStream_t)hip_stream);
}

uint64_t rt_denoise_split_workspace_bytes(int32_t width, int32_t height) {
    if (width < 1 || height < 1) return 0;
    return rt_denoise_workspace_bytes(width, height) + (uint64_t)width * (uint64_t)height * 12;
}

rt_status rt_denoise_split(const float *d_direct_sum, const float *d_indirect_sum, const rt_aov_buffers *aov, int32_t width, int32_t height,
                           int32_t samples_per_pixel, const rt_denoise_params *params, void *d_workspace, uint64_t workspace_bytes, float *d_out,
                           void *hip_stream) {
    if (!d_direct_sum || !d_indirect_sum) return rtdn::fail(RT_ERR_INVALID_ARG, "rt_denoise_split: null argument");
    const float *fbs[2] = {d_direct_sum, d_indirect_sum};
    rt_aov_buffers b;
    rt_denoise_params prm;
    rt_status st = rtdn::denoise_checks("rt_denoise_split", fbs, 2, aov, width, height, samples_per_pixel, params, d_workspace, workspace_bytes,
                                        rt_denoise_split_workspace_bytes(width, height), d_out, b, prm);
    if (st != RT_OK) return st;
    // rt_denoise's launches on each component — the direct one into the frame behind rt_denoise's planes, the indirect one into d_out — then the add
    const hipStream_t stream = (hipStream_t)hip_stream;
    const rtdn::Launch l(width, height, d_workspace);
    float *first = (float *)(l.dg + (uint64_t)width * (uint64_t)height);
    if ((st = rtdn::denoise_enqueue(d_direct_sum, b, width, height, samples_per_pixel, prm, d_workspace, first, stream)) != RT_OK) return st;
    if ((st = rtdn::denoise_enqueue(d_indirect_sum, b, width, height, samples_per_pixel, prm, d_workspace, d_out, stream)) != RT_OK) return st;
    const uint64_t floats = (uint64_t)width * (uint64_t)height * 3;
    hipLaunchKernelGGL(rtdn::denoise_add, dim3((uint32_t)((floats + 255) / 256)), dim3(256), 0, stream, (const float *)first, d_out, (uint32_t)floats);
    return rtdn::launched("denoise_add");
}

rt_status rt_denoise_spp(const float *d_fb_sum, const int32_t *d_spp, const float *d_moments, const rt_aov_buffers *aov, int32_t aov_samples,
                         int32_t width, int32_t height, const rt_denoise_params *params, void *d_workspace, uint64_t workspace_bytes, float *d_out,
                         void *hip_stream) {
    using rtdn::fail;
    if (!d_fb_sum || !d_spp || !aov || !d_workspace || !d_out) return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: null argument");
    rt_aov_buffers b;
    rt_aov_buffers_init(&b);
    const uint32_t ab = aov->struct_bytes < sizeof(b) ? aov->struct_bytes : (uint32_t)sizeof(b);
    memcpy(&b, aov, ab);
    if (ab < offsetof(rt_aov_buffers, hit_count) + sizeof(b.hit_count) || !b.albedo_sum || !b.normal_sum || !b.depth_sum || !b.hit_count)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: albedo_sum, normal_sum, depth_sum and hit_count are required");
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: width and height must be at least 1");
    if (aov_samples < 1 || aov_samples > 65536) return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: aov_samples outside 1 … 65536");
    rt_denoise_params prm;
    rt_status st = rtdn::read_params("rt_denoise_spp", params, prm);
    if (st != RT_OK) return st;
    const uint64_t pixels = (uint64_t)width * (uint64_t)height;
    if (pixels > (1ull << 24)) return fail(RT_ERR_UNSUPPORTED, "rt_denoise_spp: more than 2^24 pixels");
    const uint64_t need = rt_denoise_workspace_bytes(width, height);
    if (workspace_bytes < need)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: workspace_bytes below rt_denoise_workspace_bytes (" + std::to_string(need) + ")");
    const struct { const void *ptr; uint64_t bytes; } inputs[] = {
        {d_fb_sum, 12 * pixels}, {d_spp, 4 * pixels}, {d_moments, d_moments ? 8 * pixels : 0}, {b.albedo_sum, 12 * pixels},
        {b.normal_sum, 12 * pixels}, {b.depth_sum, 4 * pixels}, {b.hit_count, 4 * pixels}};
    for (const auto &in : inputs) {
        if (rtdn::overlap(d_out, 12 * pixels, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: d_out overlaps an input");
        if (rtdn::overlap(d_workspace, need, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: the workspace overlaps an input");
    }
    if (rtdn::overlap(d_out, 12 * pixels, d_workspace, need)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_spp: d_out overlaps the workspace");

    // ---- enqueue: the prepass with counts · the Gaussian of the sample variance (or rt_denoise's moments) · the iterations -------------
    const hipStream_t stream = (hipStream_t)hip_stream;
    const rtdn::Launch l(width, height, d_workspace);
    const rtdn::Inputs in = {d_fb_sum, b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count};
    const float inv_aov = (float)(1.0 / (double)aov_samples);
    using rtdn::launched;
    hipLaunchKernelGGL(rtdn::denoise_prepass_spp, l.grid, l.block, 0, stream, l.im, in, d_spp, d_moments, inv_aov, l.lv[0], l.nz, l.dg,
                       prm.iterations == 0 ? d_out : nullptr);
    if ((st = launched("denoise_prepass_spp")) != RT_OK || prm.iterations == 0) return st;
    if (d_moments) hipLaunchKernelGGL(rtdn::denoise_moments_spp, l.grid, l.block, 0, stream, l.im, l.lv[0], l.nz, l.dg, l.lv[1]);
    else hipLaunchKernelGGL(rtdn::denoise_moments, l.grid, l.block, 0, stream, l.im, l.lv[0], l.nz, l.dg, l.lv[1]);
    if ((st = launched("denoise_moments")) != RT_OK) return st;
    return rtdn::enqueue_steps(l, prm, d_fb_sum, 0.0f, d_out, nullptr, stream, d_spp);
}

uint64_t rt_denoise_history_bytes(int32_t width, int32_t height) {
    if (width < 1 || height < 1) return 0;
    return (uint64_t)width * (uint64_t)height * rtdn::kHistPlanes * 16 + rtdn::kHistHeader;
}

rt_status rt_denoise_temporal(const float *d_fb_sum, const rt_aov_buffers *aov, const rt_camera_data *cam, const rt_denoise_params *params,
                              const void *d_history_prev, void *d_history_next, uint64_t history_bytes, void *d_workspace, uint64_t workspace_bytes,
                              float *d_out, void *hip_stream) {
    using rtdn::fail;
    using rtdn::overlap;
    if (!d_fb_sum || !aov || !cam || !d_history_next || !d_workspace || !d_out) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: null argument");
    rt_aov_buffers b;
    rt_aov_buffers_init(&b);
    const uint32_t ab = aov->struct_bytes < sizeof(b) ? aov->struct_bytes : (uint32_t)sizeof(b);
    memcpy(&b, aov, ab);
    if (ab < offsetof(rt_aov_buffers, first_prim) + sizeof(b.first_prim) || !b.albedo_sum || !b.normal_sum || !b.depth_sum || !b.hit_count ||
        !b.first_prim)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: albedo_sum, normal_sum, depth_sum, hit_count and first_prim are required");
    const int32_t width = cam->image_width, height = cam->image_height, samples_per_pixel = cam->samples_per_pixel;
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: image width and height must be at least 1");
    if (samples_per_pixel < 1 || samples_per_pixel > 65536)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: samples_per_pixel outside 1 … 65536");
    rt_denoise_params prm;
    rt_status st = rtdn::read_params("rt_denoise_temporal", params, prm);
    if (st != RT_OK) return st;
    const uint64_t pixels = (uint64_t)width * (uint64_t)height;
    if (pixels > (1ull << 24)) return fail(RT_ERR_UNSUPPORTED, "rt_denoise_temporal: more than 2^24 pixels");
    const uint64_t need = rt_denoise_workspace_bytes(width, height), hist = rt_denoise_history_bytes(width, height);
    if (workspace_bytes < need)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: workspace_bytes below rt_denoise_workspace_bytes (" + std::to_string(need) + ")");
    if (history_bytes < hist)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: history_bytes below rt_denoise_history_bytes (" + std::to_string(hist) + ")");
    if (((uintptr_t)d_history_prev | (uintptr_t)d_history_next) & 15u)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: a history buffer is not 16-byte aligned");
    const struct { const void *ptr; uint64_t bytes; } inputs[] = {{d_fb_sum, 12 * pixels}, {b.albedo_sum, 12 * pixels}, {b.normal_sum, 12 * pixels},
                                                                   {b.depth_sum, 4 * pixels}, {b.hit_count, 4 * pixels}, {b.first_prim, 4 * pixels}};
    const uint64_t prev_bytes = d_history_prev ? hist : 0;
    for (const auto &in : inputs) {
        if (overlap(d_history_next, hist, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: history_next overlaps an input");
        if (overlap(d_out, 12 * pixels, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: d_out overlaps an input");
        if (overlap(d_workspace, need, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: the workspace overlaps an input");
    }
    if (overlap(d_history_next, hist, d_history_prev, prev_bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: history_next overlaps history_prev");
    if (overlap(d_history_next, hist, d_workspace, need)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: history_next overlaps the workspace");
    if (overlap(d_history_next, hist, d_out, 12 * pixels)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: history_next overlaps d_out");
    if (overlap(d_out, 12 * pixels, d_workspace, need)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: d_out overlaps the workspace");
    if (overlap(d_out, 12 * pixels, d_history_prev, prev_bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: d_out overlaps history_prev");
    if (overlap(d_workspace, need, d_history_prev, prev_bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal: the workspace overlaps history_prev");

    // ---- enqueue: prepass · moments · temporal · the iterations, the first of which feeds the history ----------------------------
    const hipStream_t stream = (hipStream_t)hip_stream;
    const rtdn::Launch l(width, height, d_workspace);
    const rtdn::Inputs in = {d_fb_sum, b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count};
    const float inv = (float)(1.0 / (double)samples_per_pixel);
    const float spp = (float)samples_per_pixel;
    using rtdn::launched;
    hipLaunchKernelGGL(rtdn::denoise_prepass, l.grid, l.block, 0, stream, l.im, in, inv, spp, l.lv[0], l.nz, l.dg, nullptr);
    if ((st = launched("denoise_prepass")) != RT_OK) return st;
    hipLaunchKernelGGL(rtdn::denoise_moments, l.grid, l.block, 0, stream, l.im, l.lv[0], l.nz, l.dg, l.lv[1]);
    if ((st = launched("denoise_moments")) != RT_OK) return st;
    hipLaunchKernelGGL(rtdn::denoise_temporal, l.grid, l.block, 0, stream, l.im, *cam, (const int32_t *)b.first_prim, (const rtdn::History *)d_history_prev,
                       (rtdn::History *)d_history_next, l.lv[1], l.nz, l.dg, d_fb_sum, spp, prm.iterations == 0 ? d_out : nullptr);
    if ((st = launched("denoise_temporal")) != RT_OK || prm.iterations == 0) return st;
    return rtdn::enqueue_steps(l, prm, d_fb_sum, spp, d_out, rtdn::plane(d_history_next, pixels, 0), stream);
}

rt_status rt_denoise_temporal_spp(const float *d_fb_sum, const int32_t *d_spp, const float *d_moments, const rt_aov_buffers *aov, int32_t aov_samples,
                                  const rt_camera_data *cam, const rt_denoise_params *params, const void *d_history_prev, void *d_history_next,
                                  uint64_t history_bytes, void *d_workspace, uint64_t workspace_bytes, float *d_out, void *hip_stream) {
    using rtdn::fail;
    using rtdn::overlap;
    if (!d_fb_sum || !d_spp || !aov || !cam || !d_history_next || !d_workspace || !d_out) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: null argument");
    rt_aov_buffers b;
    rt_aov_buffers_init(&b);
    const uint32_t ab = aov->struct_bytes < sizeof(b) ? aov->struct_bytes : (uint32_t)sizeof(b);
    memcpy(&b, aov, ab);
    if (ab < offsetof(rt_aov_buffers, first_prim) + sizeof(b.first_prim) || !b.albedo_sum || !b.normal_sum || !b.depth_sum || !b.hit_count ||
        !b.first_prim)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: albedo_sum, normal_sum, depth_sum, hit_count and first_prim are required");
    const int32_t width = cam->image_width, height = cam->image_height;
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: image width and height must be at least 1");
    if (aov_samples < 1 || aov_samples > 65536) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: aov_samples outside 1 … 65536");
    rt_denoise_params prm;
    rt_status st = rtdn::read_params("rt_denoise_temporal_spp", params, prm);
    if (st != RT_OK) return st;
    const uint64_t pixels = (uint64_t)width * (uint64_t)height;
    if (pixels > (1ull << 24)) return fail(RT_ERR_UNSUPPORTED, "rt_denoise_temporal_spp: more than 2^24 pixels");
    const uint64_t need = rt_denoise_workspace_bytes(width, height), hist = rt_denoise_history_bytes(width, height);
    if (workspace_bytes < need)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: workspace_bytes below rt_denoise_workspace_bytes (" + std::to_string(need) + ")");
    if (history_bytes < hist)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: history_bytes below rt_denoise_history_bytes (" + std::to_string(hist) + ")");
    if (((uintptr_t)d_history_prev | (uintptr_t)d_history_next) & 15u)
        return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: a history buffer is not 16-byte aligned");
    const struct { const void *ptr; uint64_t bytes; } inputs[] = {{d_fb_sum, 12 * pixels}, {d_spp, 4 * pixels}, {d_moments, d_moments ? 8 * pixels : 0}, {b.albedo_sum, 12 * pixels}, {b.normal_sum, 12 * pixels},
                                                                   {b.depth_sum, 4 * pixels}, {b.hit_count, 4 * pixels}, {b.first_prim, 4 * pixels}};
    const uint64_t prev_bytes = d_history_prev ? hist : 0;
    for (const auto &in : inputs) {
        if (overlap(d_history_next, hist, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: history_next overlaps an input");
        if (overlap(d_out, 12 * pixels, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: d_out overlaps an input");
        if (overlap(d_workspace, need, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: the workspace overlaps an input");
    }
    if (overlap(d_history_next, hist, d_history_prev, prev_bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: history_next overlaps history_prev");
    if (overlap(d_history_next, hist, d_workspace, need)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: history_next overlaps the workspace");
    if (overlap(d_history_next, hist, d_out, 12 * pixels)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: history_next overlaps d_out");
    if (overlap(d_out, 12 * pixels, d_workspace, need)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: d_out overlaps the workspace");
    if (overlap(d_out, 12 * pixels, d_history_prev, prev_bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: d_out overlaps history_prev");
    if (overlap(d_workspace, need, d_history_prev, prev_bytes)) return fail(RT_ERR_INVALID_ARG, "rt_denoise_temporal_spp: the workspace overlaps history_prev");

    // ---- enqueue: rt_denoise_spp's prepasses · temporal · the iterations, the first feeding the history, the last with the counts ----
    const hipStream_t stream = (hipStream_t)hip_stream;
    const rtdn::Launch l(width, height, d_workspace);
    const rtdn::Inputs in = {d_fb_sum, b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count};
    const float inv_aov = (float)(1.0 / (double)aov_samples);
    using rtdn::launched;
    hipLaunchKernelGGL(rtdn::denoise_prepass_spp, l.grid, l.block, 0, stream, l.im, in, d_spp, d_moments, inv_aov, l.lv[0], l.nz, l.dg, nullptr);
    if ((st = launched("denoise_prepass_spp")) != RT_OK) return st;
    if (d_moments) hipLaunchKernelGGL(rtdn::denoise_moments_spp, l.grid, l.block, 0, stream, l.im, l.lv[0], l.nz, l.dg, l.lv[1]);
    else hipLaunchKernelGGL(rtdn::denoise_moments, l.grid, l.block, 0, stream, l.im, l.lv[0], l.nz, l.dg, l.lv[1]);
    if ((st = launched("denoise_moments")) != RT_OK) return st;
    hipLaunchKernelGGL(rtdn::denoise_temporal_spp, l.grid, l.block, 0, stream, l.im, *cam, (const int32_t *)b.first_prim, d_spp,
                       d_moments ? rtdn::kModeMoments : rtdn::kModeSpatial, (const rtdn::History *)d_history_prev, (rtdn::History *)d_history_next, l.lv[1],
                       l.nz, l.dg, d_fb_sum, prm.iterations == 0 ? d_out : nullptr);
    if ((st = launched("denoise_temporal_spp")) != RT_OK || prm.iterations == 0) return st;
    return rtdn::enqueue_steps(l, prm, d_fb_sum, 0.0f, d_out, rtdn::plane(d_history_next, pixels, 0), stream, d_spp);
}

rt_status rt_adaptive_prior(const rt_aov_buffers *aov, int32_t aov_samples, const rt_camera_data *cam, const void *d_history_prev,
                            uint64_t history_bytes, float *d_prior, void *hip_stream) {
    using rtdn::fail;
    using rtdn::overlap;
    if (!aov || !cam || !d_prior) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: null argument");
    rt_aov_buffers b;
    rt_aov_buffers_init(&b);
    const uint32_t ab = aov->struct_bytes < sizeof(b) ? aov->struct_bytes : (uint32_t)sizeof(b);
    memcpy(&b, aov, ab);
    if (ab < offsetof(rt_aov_buffers, first_prim) + sizeof(b.first_prim) || !b.albedo_sum || !b.normal_sum || !b.depth_sum || !b.hit_count ||
        !b.first_prim)
        return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: albedo_sum, normal_sum, depth_sum, hit_count and first_prim are required");
    const int32_t width = cam->image_width, height = cam->image_height;
    if (width < 1 || height < 1) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: image width and height must be at least 1");
    if (aov_samples < 1 || aov_samples > 65536) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: aov_samples outside 1 … 65536");
    const uint64_t pixels = (uint64_t)width * (uint64_t)height;
    if (pixels > (1ull << 24)) return fail(RT_ERR_UNSUPPORTED, "rt_adaptive_prior: more than 2^24 pixels");
    const uint64_t hist = rt_denoise_history_bytes(width, height);
    if (d_history_prev && history_bytes < hist)
        return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: history_bytes below rt_denoise_history_bytes (" + std::to_string(hist) + ")");
    if ((uintptr_t)d_history_prev & 15u) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: the history buffer is not 16-byte aligned");
    if (overlap(d_prior, 8 * pixels, d_history_prev, d_history_prev ? hist : 0))
        return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: d_prior overlaps history_prev");
    const struct { const void *ptr; uint64_t bytes; } inputs[] = {{b.albedo_sum, 12 * pixels}, {b.normal_sum, 12 * pixels}, {b.depth_sum, 4 * pixels},
                                                                   {b.hit_count, 4 * pixels}, {b.first_prim, 4 * pixels}};
    for (const auto &in : inputs)
        if (overlap(d_prior, 8 * pixels, in.ptr, in.bytes)) return fail(RT_ERR_INVALID_ARG, "rt_adaptive_prior: d_prior overlaps an input");

    // ---- enqueue: one launch
    const hipStream_t stream = (hipStream_t)hip_stream;
    const rtdn::Launch l(width, height, nullptr);
    const rtdn::Inputs in = {nullptr, b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count};
    hipLaunchKernelGGL(rtdn::adaptive_prior, l.grid, l.block, 0, stream, l.im, *cam, in, (const int32_t *)b.first_prim, (float)(1.0 / (double)aov_samples),
                       (const rtdn::History *)d_history_prev, d_prior);
    return rtdn::launched("adaptive_prior");
}

}  // extern "C"
