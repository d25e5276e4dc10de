// rt_aov_fog.hip.inc — fog-aware AOVs (rt_render_aov_volume; include/rtp_amd.h, "AOVs under fog"; DESIGN.md §33).  Included by
// rt_capi.hip after rt_volume.hip.inc: the records are aov_resolve_lens_kernel's (rt_aov.hip.inc), the interval is medium_interval
// (rt_medium.hip.inc) and the cell walk volume_walk (rt_volume.hip.inc), all as they are.
//
// What is new here: the accumulation of a pass's records under a medium.  A sample whose camera ray crosses no fog adds what
// aov_accumulate_lens_kernel adds; every other sample adds its surface's albedo, normal and depth blended with the medium's by the
// transmittance Tr of the camera ray's interval, and counts as covered whether it hit a surface or not.  The contract is deterministic:
// no draw beyond the camera ray's.  Every expression is the header's, in its order.
//
// The walk runs here, a lane per pixel, and not in the per-sample resolve step: measured both ways (DESIGN.md §33), this placement wins
// without a grid, ties at 32^3 and loses 1.35 ms of a 374 ms frame at 128^3, and it needs no buffer for (Tr, t_fog).
//
// The records of a lens frame come from aov_resolve_lens_kernel alone: no candidate lists, so no sky pixel, no kPrimFlag and no
// kPrimWalk record, and this kernel neither re-walks nor counts — it has no atomic.  Its loops: the slab loop runs ceil(count / kAovSlots)
// times, the copy loop npix * seg4 / 64 times, the sample loop at most kAovSlots times, and volume_walk at most nx + ny + nz cells.
#pragma once

namespace rtk {

constexpr float kAovFogRem = RT_AOV_FOG_REM;

// the call's medium and grid (kGrid kernels only), and the transmittance sums (null: not wanted)
struct AovFog {
    MediumDev M;
    VolumeDev V;
    float *tr;          // 1 float per pixel
};

// What the medium does to the sample's camera ray (o, d) that ends at t_hit (+inf: a miss): false = clear.  Otherwise Tr of the interval,
// and t_fog, the parameter at which the optical depth along the ray reaches RT_AOV_FOG_REM (the interval's end when it never does)
template <bool kGrid>
__device__ __forceinline__ bool aov_fog_sample(const AovFog &G, f3 o, f3 d, float t_hit, float &tr, float &t_fog) {
    float t0, t1;
    if (!medium_interval(G.M, o, d, t_hit, t0, t1)) return false;
    const float len = sqrt_cr(lensq(d));
    float tau;
    int32_t cells = 0;
    if constexpr (kGrid) {
        tau = 0.0f;
        volume_walk<false>(G.M, G.V, o, d, t0, t1, len, tau, cells);
    } else {
        tau = G.M.sigma_t * ((t1 - t0) * len);
    }
    tr = exp_libm(-tau);
    if (1.0f - tr == 0.0f) return false;
    t_fog = t1;
    if constexpr (kGrid) {
        float v = kAovFogRem;
        if (volume_walk<true>(G.M, G.V, o, d, t0, t1, len, v, cells)) t_fog = v;
    } else {
        const float s = kAovFogRem / G.M.sigma_t;
        if (s < (t1 - t0) * len) t_fog = t0 + s / len;
    }
    return true;
}

// aov_accumulate_lens_kernel under fog: a wave takes 64 consecutive pixels, moves their rows through LDS (kAovSlots slots at a time), and
// each lane adds its own pixel's samples in sample order (first_pass: from zero)
template <bool kGrid>
__global__ void __launch_bounds__(kAccWaves * 64) aov_accumulate_fog_kernel(const KParams P, const LensCam C, const AovFog G, const AovOut out, int32_t first_pass) {
    __shared__ float4 tile4[kAccWaves][64 * kAovRow / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t num_pixels = P.num_pixels, pitch = P.slab_pitch;
    const int32_t count = P.pass_count;
    const uint32_t pg = (blockIdx.x * (uint32_t)kAccWaves + (uint32_t)wave) * 64u;
    if (pg >= num_pixels) return;
    const uint32_t q = pg + (uint32_t)lane;
    const bool in = q < num_pixels;
    f3 alb = mk(0.0f, 0.0f, 0.0f), nrm = mk(0.0f, 0.0f, 0.0f);
    float dep = 0.0f, trs = 0.0f;
    uint32_t hits = 0u;
    int32_t prim = -1;
    if (in && !first_pass) {
        if (out.albedo) alb = mk(out.albedo[3 * (size_t)q], out.albedo[3 * (size_t)q + 1], out.albedo[3 * (size_t)q + 2]);
        if (out.normal) nrm = mk(out.normal[3 * (size_t)q], out.normal[3 * (size_t)q + 1], out.normal[3 * (size_t)q + 2]);
        if (out.depth) dep = out.depth[q];
        if (out.hits) hits = out.hits[q];
        if (G.tr) trs = G.tr[q];
    }
    const f3 bg = mk(P.bg[0], P.bg[1], P.bg[2]);
    const f3 fog_albedo = mk(G.M.albedo[0], G.M.albedo[1], G.M.albedo[2]);
    int32_t pi = 0, pj = 0;
    if (in) aov_pixel(P, q, pi, pj);
    float *tile = reinterpret_cast<float *>(tile4[wave]);
    const uint32_t npix = num_pixels - pg < 64u ? num_pixels - pg : 64u;
    for (uint32_t s0 = 0; s0 < (uint32_t)count; s0 += kAovSlots) {
        const uint32_t ns = pitch - s0 < (uint32_t)kAovSlots ? pitch - s0 : (uint32_t)kAovSlots;      // slots of this tile (padding included: multiple of 4)
        const uint32_t seg4 = ns * 3u / 4u;
        const uint32_t total4 = npix * seg4;
        for (uint32_t k = (uint32_t)lane; k < total4; k += 64u) {
            const uint32_t pl = k / seg4, f4 = k - pl * seg4;
            const float4 v = *reinterpret_cast<const float4 *>(P.slab + ((size_t)(pg + pl) * pitch + s0) * 3 + f4 * 4u);
            *reinterpret_cast<float4 *>(tile + pl * kAovRow + f4 * 4u) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint32_t nv = (uint32_t)count - s0 < (uint32_t)kAovSlots ? (uint32_t)count - s0 : (uint32_t)kAovSlots;
        if (in) {
            const float *row = tile + lane * kAovRow;
            for (uint32_t s = 0; s < nv; ++s) {
                const float t = row[3 * s];
                const int32_t code = __float_as_int(row[3 * s + 1]);
                const uint32_t seed1 = __float_as_uint(row[3 * s + 2]);
                const bool hit = code >= 0;
                if (s0 + s == 0u) prim = hit ? code : -1;
                f3 a = bg, n = mk(0.0f, 0.0f, 0.0f);
                if (hit) aov_hit<true>(P, pi, pj, seed1, t, code, a, n, C);
                Lane L;
                f3 ray_o, ray_d;
                aov_camera_ray<true>(L, P, C, pi, pj, seed1, ray_o, ray_d);
                float tr, t_fog;
                if (!aov_fog_sample<kGrid>(G, ray_o, ray_d, hit ? t : INFINITY, tr, t_fog)) {        // clear: what rt_render_aov_lens adds
                    alb = add(alb, a);
                    if (hit) {
                        nrm = add(nrm, n);
                        dep = dep + t;
                        ++hits;
                    }
                    trs = trs + 1.0f;
                    continue;
                }
                const float f = 1.0f - tr;
                const f3 fu = scale(f, unit(ray_d));
                alb = add(alb, add(scale(tr, a), scale(f, fog_albedo)));
                if (hit) {
                    nrm = add(nrm, sub(scale(tr, n), fu));
                    dep = dep + (tr * t + f * t_fog);
                } else {
                    nrm = add(nrm, neg(fu));
                    dep = dep + t_fog;
                }
                ++hits;
                trs = trs + tr;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    if (!in) return;
    if (out.albedo) { out.albedo[3 * (size_t)q] = alb.x; out.albedo[3 * (size_t)q + 1] = alb.y; out.albedo[3 * (size_t)q + 2] = alb.z; }
    if (out.normal) { out.normal[3 * (size_t)q] = nrm.x; out.normal[3 * (size_t)q + 1] = nrm.y; out.normal[3 * (size_t)q + 2] = nrm.z; }
    if (out.depth) out.depth[q] = dep;
    if (out.hits) out.hits[q] = hits;
    if (out.prim && first_pass) out.prim[q] = prim;
    if (G.tr) G.tr[q] = trs;
}

// the transmittance of a call without a medium: every sample is clear
__global__ void __launch_bounds__(256) aov_fog_fill_kernel(float *tr, uint32_t n, float value) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q < n) tr[q] = value;
}

}  // namespace rtk
