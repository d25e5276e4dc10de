// rt_aov.hip.inc — first-hit AOVs: albedo, normal, depth, coverage and primitive id per pixel (rt_render_aov; included by
// rt_capi.hip after rt_primary.hip.inc).
//
// The buffers a denoiser and a compositor want come from the same camera samples as the beauty frame: for pixel (i, j) and
// sample s, the reference's own camera ray (get_ray with the seed quirk of sample_seed1) and its first hit, hit_scene over
// Interval(0.001, 1e30) — nothing of the path behind it.  So a pass is two steps on the handle's sample slab:
//   (1) resolve: every sample's first hit as a (distance, code, seed) record.  Where the handle takes camera rays from per-pixel
//       candidate lists (rt_primary.hip.inc) the unchanged cand_kernel and primary kernels write the records, and the pixels
//       they have no list for (kPrimWalk) are walked here in the reference's order.  Without lists every sample is walked here.
//   (2) accumulate: one lane per pixel adds the pass's samples onto the running sums in sample order, like accumulate_kernel.
//       The rare record the primary pass could not vouch for (kPrimFlag) is walked where the lane meets it: a separate launch
//       would have to scan the whole slab for them (4.2 ms of the headline frame's 12.4 GB).
// A hit is rebuilt from its record with shade()'s own arithmetic (point = o + t d, the outward normal, set_face_normal, the
// material row, tex2D_cpu for a textured one) — the same bits the beauty pass computes for that hit.
#pragma once

namespace rtk {

// device pointers of rt_aov_buffers (any may be null)
struct AovOut {
    float *albedo;       // 3 floats per pixel
    float *normal;       // 3 floats per pixel
    float *depth;        // 1 float per pixel
    uint32_t *hits;      // 1 word per pixel
    int32_t *prim;       // 1 word per pixel: code of sample 0's hit, -1 for a miss
};

constexpr int kAovSlots = 8;            // accumulate: slots per LDS tile — 28 KB per workgroup, five workgroups per CU: its loop waits on gathers (16, accumulate_kernel's: 2.3 ms slower at 1080p x 500)
constexpr int kAovRow = kAovSlots * 3 + 4;

// a sample's camera ray: the pinhole's (camera_ray), or kLens: the lens / moving camera's (lens_camera_ray, rt_render_aov_lens)
template <bool kLens>
__device__ __forceinline__ void aov_camera_ray(Lane &L, const KParams &P, const LensCam &C, int32_t pi, int32_t pj, uint32_t seed1, f3 &ray_o, f3 &ray_d) {
    if constexpr (kLens) lens_camera_ray(L, C, pi, pj, seed1, ray_o, ray_d);
    else camera_ray<false>(L, P, pi, pj, seed1, ray_o, ray_d);
}

// hit_scene for a sample's camera ray: the reference-order walk, closest_hit_kernel's loop → (t, code or kPrimMiss)
template <bool kLens = false>
__device__ __forceinline__ int32_t aov_walk(const KParams &P, int32_t pi, int32_t pj, uint32_t seed1, float &t, const LensCam &C = LensCam{}) {
    Lane L;
    f3 ray_o, ray_d;
    aov_camera_ray<kLens>(L, P, C, pi, pj, seed1, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    while (!traversal_finished<true>(L, kBlocked)) {
        if (L.sp != 0) leaf_threaded(L, P.spheres, P.planes);
        else step_threaded(L, P.tnodes, P.num_tnodes);
    }
    t = L.closest;
    return L.hit >= 0 ? L.hit : kPrimMiss;
}

// local pixel → image pixel (map_work)
__device__ __forceinline__ void aov_pixel(const KParams &P, uint32_t q, int32_t &pi, int32_t &pj) {
    const uint32_t pjl = div_magic(q, P.magic_width);
    pi = (int32_t)(q - pjl * (uint32_t)P.row_w) + P.tile_x0;
    if (P.num_parts == 1) {
        pj = (int32_t)pjl + P.tile_y0;
    } else {
        const uint32_t band = div_magic(pjl, P.magic_band);
        pj = (int32_t)((band * (uint32_t)P.num_parts + (uint32_t)P.part) * (uint32_t)P.band_rows + (pjl - band * (uint32_t)P.band_rows));
    }
}

// every sample of the pass, a lane per sample, 64 consecutive samples per wave → its (t, code, seed) record, from the lens camera's ray
// (aov_resolve_lens_kernel).  The kAll branch of aov_resolve_kernel below is the same loop for the pinhole, kept as its own text: called
// through this helper, that kernel's code changed (one instruction), and the pinhole kernels stay what they were.
template <bool kLens>
__device__ __forceinline__ void aov_resolve_all(const KParams &P, const LensCam &C, uint32_t lane, uint32_t wave, uint32_t num_waves) {
    const uint32_t batches = (P.total_work + 63u) >> 6;
    for (uint32_t b = wave; b < batches; b += num_waves) {
        const uint32_t w = b * 64u + lane;
        if (w >= P.total_work) continue;
        int32_t pi, pj;
        uint32_t k, record;
        map_work<false>(P, w, pi, pj, k, 0u, nullptr, nullptr, &record);
        const uint32_t seed1 = sample_seed1(wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj), P.pass_first + (int32_t)k);
        float t;
        const int32_t code = aov_walk<kLens>(P, pi, pj, seed1, t, C);
        float *rec = P.slab + (size_t)record * 3;
        rec[0] = t;
        rec[1] = __int_as_float(code);
        rec[2] = __uint_as_float(seed1);
    }
}

// (1) Resolve what the primary pass could not.  kAll (no candidate lists): every sample of the pass, a lane per sample, 64
// consecutive samples per wave.  Otherwise the pixels without a list (kCandNone: every record kPrimWalk) — a wave per pixel, as
// primary_pixel_kernel takes them; *walked += their samples.  (A kPrimFlag record — a tie, a hit in front of its own leaf box:
// single samples, a few in ten thousand — is walked where the accumulation meets it.)
template <bool kAll>
__global__ void __launch_bounds__(256) aov_resolve_kernel(const KParams P, uint32_t *walked) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6), num_waves = gridDim.x * 4u;
    if (kAll) {
        const uint32_t batches = (P.total_work + 63u) >> 6;
        for (uint32_t b = wave; b < batches; b += num_waves) {
            const uint32_t w = b * 64u + lane;
            if (w >= P.total_work) continue;
            int32_t pi, pj;
            uint32_t k, record;
            map_work<false>(P, w, pi, pj, k, 0u, nullptr, nullptr, &record);
            const uint32_t seed1 = sample_seed1(wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj), P.pass_first + (int32_t)k);
            float t;
            const int32_t code = aov_walk(P, pi, pj, seed1, t);
            float *rec = P.slab + (size_t)record * 3;
            rec[0] = t;
            rec[1] = __int_as_float(code);
            rec[2] = __uint_as_float(seed1);
        }
        return;
    }
    uint32_t count = 0;
    for (uint32_t q = wave; q < P.num_pixels; q += num_waves) {
        if (*(k_u32 *)(uintptr_t)(P.cand + (size_t)q * kCandWords) != kCandNone) continue;
        int32_t pi, pj;
        aov_pixel(P, q, pi, pj);
        float *row = P.slab + (size_t)q * P.slab_pitch * 3;
        for (uint32_t k = lane; k < (uint32_t)P.pass_count; k += 64u) {
            float t;
            const int32_t code = aov_walk(P, pi, pj, __float_as_uint(row[3 * k + 2]), t);
            row[3 * k] = t;
            row[3 * k + 1] = __int_as_float(code);
        }
        count += (uint32_t)P.pass_count;
    }
    if (lane == 0u && count != 0u) atomicAdd(walked, count);
}

// What one hit adds: shade()'s surface arithmetic (rt_kernel.hip.inc) on the sample's camera ray — the hit point, the outward
// normal, set_face_normal, the material row and, for a textured LAMBERTIAN or METAL material, its texel.
template <bool kLens = false>
__device__ __forceinline__ void aov_hit(const KParams &P, int32_t pi, int32_t pj, uint32_t seed1, float t, int32_t code, f3 &albedo, f3 &normal,
                                        const LensCam &C = LensCam{}) {
    Lane L;
    f3 ray_o, ray_d;
    aov_camera_ray<kLens>(L, P, C, pi, pj, seed1, ray_o, ray_d);
    const f3 point = add(ray_o, scale(t, ray_d));        // r.at(rec.t)
    const int32_t idx = code >> 1;
    const bool is_plane = (code & 1) != 0;
    f3 outward;
    int32_t mat_idx;
    if (is_plane) {
        const float4 P0 = P.planes[5 * idx + 0];
        outward = mk(P0.x, P0.y, P0.z);
        mat_idx = as_int(P.planes[5 * idx + 2].w);
    } else {
        const float4 s = P.spheres[idx];
        outward = divs(sub(point, mk(s.x, s.y, s.z)), s.w);
        mat_idx = P.sphere_mat[idx];
    }
    const bool front = dot(ray_d, outward) < 0;          // set_face_normal, include/hittable_object.h:17-20
    normal = front ? outward : neg(outward);
    const float4 MA = P.materials[3 * mat_idx + 0];      // albedo, type | texture_id << 2
    const int32_t type = as_int(MA.w) & 3;
    const int32_t tex_id = as_int(MA.w) >> 2;
    albedo = mk(1.0f, 1.0f, 1.0f);                       // DIELECTRIC, DIFFUSE_LIGHT
    if (type != RT_MAT_LAMBERTIAN && type != RT_MAT_METAL) return;
    albedo = mk(MA.x, MA.y, MA.z);
    if (tex_id == 0) return;
    float tu, tv;
    if (is_plane) {                                      // rec.u/v = alpha/beta of hit_plane
        const float4 P1 = P.planes[5 * idx + 1];
        const float4 P2 = P.planes[5 * idx + 2];
        const float4 P3 = P.planes[5 * idx + 3];
        const float4 P4 = P.planes[5 * idx + 4];
        const f3 ph = sub(point, mk(P4.x, P4.y, P4.z));
        const f3 w = mk(P1.x, P1.y, P1.z);
        tu = dot(w, cross(ph, mk(P3.x, P3.y, P3.z)));
        tv = dot(w, cross(mk(P2.x, P2.y, P2.z), ph));
    } else {                                             // get_sphere_uv, include/sphere.h:16-22
        const float theta = acos_libm(outward.y);
        const float phi = (float)((double)atan2_libm(-outward.z, outward.x) + 3.14159265358979323846);
        tu = (float)((double)phi / (2 * 3.14159265358979323846));
        tv = (float)((double)theta / 3.14159265358979323846);
    }
    albedo = mul(albedo, sample_texture(P, tex_id - 1, tu, tv));
}

// (2) Sum a pass's records onto the pixel's AOVs in sample order (first_pass: from zero).  accumulate_kernel's pattern: a wave
// takes 64 consecutive pixels, moves their rows through LDS (kAovSlots slots at a time) with 16-byte loads, and each lane then
// reads its own pixel's samples.  A kPrimFlag record is walked here (*walked counts them).  A miss adds the background to the albedo and nothing else; a sky pixel (no candidate leaf) is all
// misses and has no row, and a wave of nothing but sky reads no slab at all.
__global__ void __launch_bounds__(kAccWaves * 64) aov_accumulate_kernel(const KParams P, const AovOut out, int32_t first_pass, uint32_t *walked) {
#define RTP_AOV_WALK(...) aov_walk(__VA_ARGS__)
#define RTP_AOV_HIT(...) aov_hit(__VA_ARGS__)
#include "rt_aov_accumulate_body.inc"
#undef RTP_AOV_WALK
#undef RTP_AOV_HIT
}

// rt_render_aov_lens: the same two steps with the lens / moving camera's rays and no candidate lists — (1) every sample's first hit …
__global__ void __launch_bounds__(256) aov_resolve_lens_kernel(const KParams P, const LensCam C) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6), num_waves = gridDim.x * 4u;
    aov_resolve_all<true>(P, C, lane, wave, num_waves);
}
// … (2) added to the sums in sample order, each hit rebuilt from the sample's lens ray
__global__ void __launch_bounds__(kAccWaves * 64) aov_accumulate_lens_kernel(const KParams P, const LensCam C, const AovOut out, int32_t first_pass, uint32_t *walked) {
#define RTP_AOV_WALK(...) aov_walk<true>(__VA_ARGS__, C)
#define RTP_AOV_HIT(...) aov_hit<true>(__VA_ARGS__, C)
#include "rt_aov_accumulate_body.inc"
#undef RTP_AOV_WALK
#undef RTP_AOV_HIT
}

}  // namespace rtk
