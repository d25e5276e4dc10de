// rt_primary.hip.inc — primary visibility without a walk (included by rt_capi.hip after rt_kernel.hip.inc).
//
// A third of all rays of the headline frame are camera rays, and the 500 samples of a pixel send theirs through the same
// sliver of space.  Which leaves those rays can reach is therefore decided ONCE PER PIXEL (cand_kernel: the guarded walk's
// own tree descended with the pixel's cone, rt_beam.h — 2.5 candidates per pixel on S-rtiow), and every sample then tests just
// those primitives (primary_kernel: all 64 lanes of a wave on samples of the same pixel, same candidates, no stack, no
// votes) and leaves (hit distance, primitive code) in its own slot of the sample slab, where render_kernel<…, kPrim> picks
// it up when it starts the sample (and later overwrites the slot with the sample's radiance).
//
// Why the result is the reference's (docs/LOG.md §3b): the guarded walk's argument needs only that every primitive whose test
// can report a hit for the ray is tested, in any order — such a primitive's computed hit point lies inside its inflated leaf
// box, the ray is inside the pixel's cone, so the leaf is on the list (rt_beam.h).  Exact ties between two candidates flag
// the sample like the walk's ties do (kPrimTie); the final check of the hit against its exact leaf box and the far-origin test
// stay where they are, in the shade step and at the start of the sample.  The primitive tests are the walk's own functions.
#pragma once
#include "rt_beam.h"

namespace rtk {

constexpr int kCandWords = 16;                  // per pixel: [0] number of candidates or kCandNone, [1..15] their codes (2 index + type)
constexpr uint32_t kCandNone = 0xffffffffu;

__global__ void __launch_bounds__(256) cand_kernel(const KParams P, uint32_t *cand, double coord_max) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= P.num_pixels) return;
    const uint32_t pjl = q / (uint32_t)P.row_w;
    const int32_t pi = (int32_t)(q - pjl * (uint32_t)P.row_w) + P.tile_x0;
    int32_t pj = (int32_t)pjl + P.tile_y0;
    if (P.num_parts != 1) {           // local row → image row (map_work)
        const uint32_t band = pjl / (uint32_t)P.band_rows;
        pj = (int32_t)((band * (uint32_t)P.num_parts + (uint32_t)P.part) * (uint32_t)P.band_rows + (pjl - band * (uint32_t)P.band_rows));
    }
    const rtbeam::Beam beam = rtbeam::make_beam(P.origin, P.p00, P.du, P.dv, pi, pj, coord_max);
    uint32_t codes[kCandWords - 1];
    const float *tab = reinterpret_cast<const float *>(P.nodes);
    int n = rtbeam::beam_candidates(beam, [tab](int32_t k) { return tab + (size_t)k * 16; }, P.root, (double)P.g_dynk, codes, kCandWords - 1);
    n = rtbeam::beam_front_candidates(beam, P.num_front, P.front_code, P.front_box, (double)P.g_dynk, codes, n, kCandWords - 1);      // (not leaves of the tree)
    uint32_t *out = cand + (size_t)q * kCandWords;
    out[0] = n < 0 ? kCandNone : (uint32_t)n;
    for (int k = 0; k < kCandWords - 1; ++k) out[1 + k] = k < n ? codes[k] : 0u;
}

// ---- which pixels the trace kernel takes, and in which order -----------------------------------------------------------------
// Sky pixels (no candidate: no sample of theirs can hit anything) get no ray, no record and no row of the slab (the accumulation
// adds the background from a register) and are not in the trace kernel's index space at all: their samples used to cost a
// reservation, a record fetch and a store each, and a stretch of nothing but sky is paced by the launch's one work counter
// (an all-sky frame: 90 Gsamples/s, the counter's rate).  The other pixels are fetched through a table, expensive ones first:
//   class 0  two or more candidates (a sphere in front of the ground, or no list)   — every long path starts here
//   class 1  one candidate (the ground alone: a bounce, then mostly sky)
//   class 2  no candidate (sky) — behind the others in the table, never fetched
// stable within a class.  A launch ends with its longest paths (once the counter has run dry every wave finishes what it has
// in flight: wave exit times spread over 1.5 ms, on the whole frame and on an eighth of it alike); with the cheap pixels
// last the long paths drain while there is still work for the other waves.  What is computed per sample does not depend on
// the order (a sample is a pure function of pixel and index); the slab, the flag list and the accumulation go by pixel.
// counts[2 * num_blocks] after the scan = the number of pixels of classes 0 and 1 = the trace kernel's pixel count.
#ifndef RTP_ORDER_SPLIT
#define RTP_ORDER_SPLIT 1           /* 0: the pixels with candidates in image order */
#endif
constexpr int kOrderBlock = 256;
__device__ __forceinline__ uint32_t pixel_class(uint32_t n) { return n == 0u ? 2u : ((RTP_ORDER_SPLIT && n == 1u) ? 1u : 0u); }      // kCandNone: class 0
// (1) pixels of each class per block of 256 → counts[class * num_blocks + block]
__global__ void __launch_bounds__(kOrderBlock) order_count_kernel(const uint32_t *cand, uint32_t num_pixels, uint32_t num_blocks, uint32_t *counts) {
    __shared__ uint32_t part[3][kOrderBlock / 64];
    const uint32_t q = blockIdx.x * (uint32_t)kOrderBlock + threadIdx.x;
    const uint32_t cls = q < num_pixels ? pixel_class(cand[(size_t)q * kCandWords]) : 3u;
    const int wave = threadIdx.x >> 6;
    for (uint32_t c = 0; c < 3; ++c) {
        const uint32_t n = (uint32_t)__popcll(__ballot(cls == c));
        if ((threadIdx.x & 63) == 0) part[c][wave] = n;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t n = 0;
        for (int w = 0; w < kOrderBlock / 64; ++w) n += part[threadIdx.x][w];
        counts[threadIdx.x * num_blocks + blockIdx.x] = n;
    }
}
// (2) exclusive prefix sum over the 3 * num_blocks counts, in place (class-major: all of class 0, then 1, then 2) — one workgroup
__global__ void __launch_bounds__(1024) order_scan_kernel(uint32_t *counts, uint32_t n) {
    __shared__ uint32_t sums[1024];
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    uint32_t s = 0;
    for (uint32_t k = lo; k < hi; ++k) s += counts[k];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {          // Hillis-Steele, inclusive
        const uint32_t v = threadIdx.x >= d ? sums[threadIdx.x - d] : 0u;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = sums[threadIdx.x] - s;
    for (uint32_t k = lo; k < hi; ++k) { const uint32_t c = counts[k]; counts[k] = run; run += c; }
}
// (3) each pixel to its place: offset of its (class, block) + its rank among the block's pixels of that class.  A place is one row of
// kOrderRowWords words, everything about the pixel that the trace kernel needs where it starts a sample (map_fetch): the pixel's
// centre on the image plane — pixel_center, camera_ray's own expression on the same operands — and the local pixel.  Computed here
// once per pixel and view by a full wave, instead of once per sample by the few lanes of a wave whose paths have just ended.
__global__ void __launch_bounds__(kOrderBlock) order_scatter_kernel(const KParams P, const uint32_t *cand, uint32_t num_pixels, uint32_t num_blocks,
                                                                    const uint32_t *offsets, uint32_t *order) {
    __shared__ uint32_t part[3][kOrderBlock / 64];
    const uint32_t q = blockIdx.x * (uint32_t)kOrderBlock + threadIdx.x;
    const uint32_t cls = q < num_pixels ? pixel_class(cand[(size_t)q * kCandWords]) : 3u;
    const int wave = threadIdx.x >> 6;
    uint32_t rank = 0;
    for (uint32_t c = 0; c < 3; ++c) {
        const uint64_t m = __ballot(cls == c);
        if ((threadIdx.x & 63) == 0) part[c][wave] = (uint32_t)__popcll(m);
        if (cls == c) rank = (uint32_t)lane_rank(m);
    }
    __syncthreads();
    if (cls < 3u) {
        for (int w = 0; w < wave; ++w) rank += part[cls][w];
        int32_t pi, pj;
        local_to_image(P, q, pi, pj);
        const f3 center = pixel_center(mk(P.p00[0], P.p00[1], P.p00[2]), mk(P.du[0], P.du[1], P.du[2]), mk(P.dv[0], P.dv[1], P.dv[2]), pi, pj);
        const size_t place = (size_t)(offsets[cls * num_blocks + blockIdx.x] + rank);         // < num_pixels: the table has a row for every pixel
        *reinterpret_cast<u4v *>(order + place * kOrderRowWords) = u4v{__float_as_uint(center.x), __float_as_uint(center.y), __float_as_uint(center.z), q};
    }
}

// ---- the per-sample pass ------------------------------------------------------------------------------------------------
// For every sample of the pass: camera ray (start_sample), the pixel's candidates tested with the walk's own primitive tests,
// the hit checked against its exact leaf box (guard_final_check — the check every hit of the guarded walk gets at the start
// of its shade step; a camera ray's is done here, where all 64 lanes have one), (distance, code) into the sample's slot.
// kPlanes: the scene has planes (their candidates carry odd codes).
typedef __attribute__((address_space(4))) const uint32_t k_u32;         // constant address space: scalar loads for uniform addresses
typedef float kf4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const kf4 k_f4;

// (RayConst / ray_const, the constants of a ray that every sphere test needs: rt_kernel.hip.inc, beside test_sphere_ray)

// candidate C of a wave-uniform list: the list is read four words at a time into scalar registers (word 0 is the count, so
// a group boundary falls before candidates 3, 7 and 11), the sphere record with a scalar load too
typedef uint32_t ku4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const ku4 k_u4;
// (hs: the record of the sphere that is the closest hit so far — the final check needs it again, and a select per word here
// is cheaper than a gather with its round trip there)
template <int C, bool kPlanes>
__device__ __forceinline__ void cand_step(Lane &L, const KParams &P, const RayConst &rc, k_u4 *list4, uint32_t n, k_f4 *sph, ku4 grp, float4 &hs) {
    if constexpr (C < kCandWords - 1) {
        if ((uint32_t)C >= n) return;
        if constexpr ((C + 1) % 4 == 0) grp = list4[(C + 1) / 4];
        const uint32_t code = grp[(C + 1) % 4];
        if (kPlanes && (code & 1u)) {
            test_plane<true>(L, P.planes, (int32_t)(code >> 1), (int32_t)code);
        } else {
            const kf4 sp = sph[code >> 1];
            test_sphere_ray<true, true>(L, make_float4(sp.x, sp.y, sp.z, sp.w), (int32_t)code, rc.a, rc.da, rc.y);
            const bool took = L.hit == (int32_t)code;
            hs = make_float4(took ? sp.x : hs.x, took ? sp.y : hs.y, took ? sp.z : hs.z, took ? sp.w : hs.w);
        }
        cand_step<C + 1, kPlanes>(L, P, rc, list4, n, sph, grp, hs);
    }
}
// the whole list of local pixel q0 (wave-uniform) against the ray in L → the code to leave in the sample's record
template <bool kPlanes>
__device__ __forceinline__ int32_t test_uniform_list(Lane &L, const KParams &P, uint32_t q0, float4 &hs) {
    k_u4 *list4 = (k_u4 *)(uintptr_t)(P.cand + (size_t)q0 * kCandWords);
    const ku4 first = list4[0];
    const uint32_t n = first.x;
    if (n == kCandNone) return kPrimWalk;
    const RayConst rc = ray_const(L);
    cand_step<0, kPlanes>(L, P, rc, list4, n, (k_f4 *)(uintptr_t)P.spheres, first, hs);
    return L.hit >= 0 ? L.hit : kPrimMiss;
}
template <bool kPlanes>
__device__ __forceinline__ int32_t test_lane_list(Lane &L, const KParams &P, uint32_t q, float4 &hs) {
    const uint32_t *list = P.cand + (size_t)q * kCandWords;
    const uint32_t n = list[0];
    if (n == kCandNone) return kPrimWalk;
    const RayConst rc = ray_const(L);
    for (uint32_t c = 0; c < n; ++c) {
        const uint32_t code = list[1 + c];
        const int32_t idx = (int32_t)(code >> 1);
        if (kPlanes && (code & 1u)) test_plane<true>(L, P.planes, idx, (int32_t)code);
        else {
            const float4 sp = P.spheres[idx];
            test_sphere_ray<true, true>(L, sp, (int32_t)code, rc.a, rc.da, rc.y);
            if (L.hit == (int32_t)code) hs = sp;
        }
    }
    return L.hit >= 0 ? L.hit : kPrimMiss;
}
// (all twelve bytes of the record are written — distance, code, the RNG state camera_ray() starts from: whole cache lines leave
// the wave, and the trace kernel need not hash the pixel and the sample index again)
template <bool kPlanes>
__device__ __forceinline__ void finish_primary(Lane &L, const KParams &P, int32_t code_out, uint32_t seed1, float4 hs, float *rec) {
    // guard_final_check: the ray must enter the hit's own (exact) leaf box before the hit.  A sphere whose leaf box is
    // fl(c -/+ r) — every sphere of a scene without a leaf-box table — is checked on the record kept in hs
    if (P.leaf_boxes == nullptr) {
        float enter;
        const bool in = slab(L, hs.x - hs.w, hs.y - hs.w, hs.z - hs.w, hs.x + hs.w, hs.y + hs.w, hs.z + hs.w, 1e30f, enter);
        const bool sphere_hit = code_out >= 0 && (!kPlanes || !(code_out & 1));
        if (sphere_hit && !(in && L.closest > enter)) L.depth |= kFlagBit;
        if (kPlanes && code_out >= 0 && (code_out & 1) && !guard_final_check<false>(L, P, P.spheres)) L.depth |= kFlagBit;
    } else if (code_out >= 0 && !guard_final_check<false>(L, P, P.spheres)) {
        L.depth |= kFlagBit;
    }
    if (L.depth & kFlagBit) code_out = kPrimFlag;
    rec[0] = L.closest;
    rec[1] = __int_as_float(code_out);
    rec[2] = __uint_as_float(seed1);
}

// Any pass: a wave takes 64 consecutive work indices — samples of one pixel, or of a few neighbours when a pass has fewer
// than 64 samples per pixel or a pixel's samples end inside the batch.
template <bool kPlanes>
__global__ void __launch_bounds__(256) primary_kernel(const KParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, num_waves = gridDim.x * 4u;
    const uint32_t batches = (P.total_work + 63u) >> 6;
    for (uint32_t b = wave; b < batches; b += num_waves) {
        const uint32_t w = b * 64u + lane;
        if (w >= P.total_work) continue;
        int32_t pi, pj;
        uint32_t k, record;
        map_work<false>(P, w, pi, pj, k, 0u, nullptr, nullptr, &record);
        const uint32_t q = P.pass_count == 64 ? (w >> 6) : div_magic(w, P.magic_count);      // the local pixel (as map_work)
        if (P.cand[(size_t)q * kCandWords] == 0u) continue;         // sky: no ray, no record, no row (accumulate_kernel adds the background)
        Lane L;
        f3 ray_o, ray_d;
        const uint32_t seed1 = sample_seed1(wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj), P.pass_first + (int32_t)k);
        camera_ray<false>(L, P, pi, pj, seed1, ray_o, ray_d);
        begin_ray(L, ray_o, ray_d, 0);      // closest = 1e30, no hit; 1 / direction for the final check
        const uint32_t q0 = __builtin_amdgcn_readfirstlane(q);
        float4 hs = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const int32_t code_out = __ballot(q != q0) == 0ull ? test_uniform_list<kPlanes>(L, P, q0, hs) : test_lane_list<kPlanes>(L, P, q, hs);
        finish_primary<kPlanes>(L, P, code_out, seed1, hs, P.slab + (size_t)record * 3);
    }
}

// Passes of at least 96 samples per pixel (RTP_BY_PIXEL_MIN; the headline frame: one pass of 500): a wave takes whole PIXELS and walks a
// pixel's samples 64 at a time, so everything that belongs to the pixel — its place in the image, its seed, the centre of
// its footprint, its candidate list — is made once, in scalar registers where it is integer work.
template <bool kPlanes>
__global__ void __launch_bounds__(256) primary_pixel_kernel(const KParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6), num_waves = gridDim.x * 4u;
    for (uint32_t q = wave; q < P.num_pixels; q += num_waves) {
        const uint32_t pjl = div_magic(q, P.magic_width);
        const int32_t pi = (int32_t)(q - pjl * (uint32_t)P.row_w) + P.tile_x0;
        int32_t pj = (int32_t)pjl + P.tile_y0;
        if (P.num_parts != 1) {           // local row → image row (map_work)
            const uint32_t band = div_magic(pjl, P.magic_band);
            pj = (int32_t)((band * (uint32_t)P.num_parts + (uint32_t)P.part) * (uint32_t)P.band_rows + (pjl - band * (uint32_t)P.band_rows));
        }
        float *row = P.slab + (size_t)q * P.slab_pitch * 3;
        // a pixel no leaf of the scene can be hit through (sky: a quarter of the headline frame): its samples need no ray, no
        // record, no trace kernel and no row of the slab — accumulate_kernel adds the background count times
        if (*(k_u32 *)(uintptr_t)(P.cand + (size_t)q * kCandWords) == 0u) continue;
        const uint32_t base_seed = wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj);
        for (uint32_t k = lane; k < (uint32_t)P.pass_count; k += 64u) {
            Lane L;
            f3 ray_o, ray_d;
            const uint32_t seed1 = sample_seed1(base_seed, P.pass_first + (int32_t)k);
            camera_ray<false>(L, P, pi, pj, seed1, ray_o, ray_d);
            begin_ray(L, ray_o, ray_d, 0);
            float4 hs = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int32_t code_out = test_uniform_list<kPlanes>(L, P, q, hs);
            finish_primary<kPlanes>(L, P, code_out, seed1, hs, row + (size_t)k * 3);
        }
    }
}

}  // namespace rtk
