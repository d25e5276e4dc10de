// rt_split.hip.inc — rt_render_lit_split / rt_trace_samples_lit_split (include/rtp_amd.h, "direct and indirect light in separate
// frames"; DESIGN.md §41): rt_render_lit's sample, its radiance written as two components.  Included by rt_capi.hip right after
// rt_light.hip.inc, whose vertex (shade_lit2), fetch (RTP_LIT_POOL_FETCH) and step (lit_step) these kernels run unchanged: the split draws
// nothing and changes no branch.  Lit<Table> and GlossLit<Table> only — no fog, no list variants.
//
// Along a path every direct contribution is added before every indirect one, so the lane needs no second colour: at the crossing L.color
// goes to the sample's record of the direct slab and starts again from zero.  What the lane has to remember is its stage —
//   0  no diffuse event yet;   1  the last vertex was the path's first diffuse event;   2  crossed
// — and that lives in the two top bits of the lane's work index w, which stays below 2^30 (rt_accel.h, plan_passes).
#pragma once

namespace rtk {

constexpr uint32_t kSplitStageShift = 30u;
constexpr uint32_t kSplitWorkMask = (1u << kSplitStageShift) - 1u;

// was the vertex a diffuse event?  The carried value shade_lit2 hands out: true / RT_NEE_PB after a diffuse event; after a glossy one the
// gloss types carry -pg (or -0), after anything else 0 — so "greater than zero" and nothing that leans on the sign alone
__device__ __forceinline__ bool split_diffuse(bool carried) { return carried; }
__device__ __forceinline__ bool split_diffuse(float carried) { return carried > 0.0f; }

// the first float of work index w's record, the same in both slabs (store_sample's arithmetic)
__device__ __forceinline__ size_t split_record(const KParams &P, uint32_t w) {
    const uint32_t sq = P.pass_count == 64 ? (w >> 6) : div_magic(w, P.magic_count);
    const uint32_t sk = w - sq * (uint32_t)P.pass_count;
    return ((size_t)sq * P.slab_pitch + sk) * 3;
}
__device__ __forceinline__ void split_store(float *slab, size_t rec, f3 c) {
    slab[rec] = c.x; slab[rec + 1] = c.y; slab[rec + 2] = c.z;
}
// the end of a path: what the lane holds is the indirect component after the crossing (the direct record was written there), the direct
// one before it (the indirect record is zero).  Either way each record of the sample has been written exactly once.
__device__ __forceinline__ void split_finish(const KParams &P, float *indirect, uint32_t w, f3 color) {
    const size_t rec = split_record(P, w & kSplitWorkMask);
    if ((w >> kSplitStageShift) == 2u) {
        split_store(indirect, rec, color);
    } else {
        split_store(P.slab, rec, color);
        split_store(indirect, rec, mk(0.0f, 0.0f, 0.0f));
    }
}

// ---- probe (rt_trace_samples_lit_split): lit_probe_body without fog, radiance in two columns ------------------------------------------
template <bool kLens, class Lit>
__device__ __forceinline__ void split_probe_body(const KParams &P, const Lit &T, const LensCam &C, uint32_t *nee_seed_out, uint32_t *env_seed_out, float *indirect_out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    uint32_t nee = light_seed_of(T.N, base_seed, s), env = light_seed_of(T.E, base_seed, s);
    f3 ray_o, ray_d;
    lit_start<kLens>(L, P, C, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0;
    uint32_t stage = 0u;
    LitCarry<Lit> prev_diffuse = LitCarry<Lit>(0);
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
            LitSamples S;
            S.code = -1;
            LitCarry<Lit> diffuse;
            const bool more = shade_lit2(L, P, T, prev_diffuse, nee, env, ray_o, ray_d, S, diffuse);
            if (stage == 1u) {          // what the first diffuse event's ray found is in: the path crosses (the record is written here, as in the wave loop)
                split_store(P.probe_rad, 3 * (size_t)g, L.color);
                L.color = mk(0.0f, 0.0f, 0.0f);
                stage = 2u;
            } else if (stage == 0u && split_diffuse(diffuse)) {
                stage = 1u;
            }
            if (S.a) {
                rays++;
                begin_ray(L, ray_o, S.adir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
                if (L.hit == S.code) L.color = add(L.color, S.ac);
            }
            if (S.b) {
                rays++;
                begin_ray(L, ray_o, S.bdir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, true);
                if (L.hit < 0) L.color = add(L.color, S.bc);
            }
            if (!more) break;
            prev_diffuse = diffuse;
            begin_ray(L, ray_o, ray_d, 0);
        }
    }
    if (stage == 2u) {
        split_store(indirect_out, 3 * (size_t)g, L.color);
    } else {
        split_store(P.probe_rad, 3 * (size_t)g, L.color);
        split_store(indirect_out, 3 * (size_t)g, mk(0.0f, 0.0f, 0.0f));
    }
    P.probe_rays[g] = rays;
    P.probe_seed[g] = L.seed;
    nee_seed_out[g] = nee;
    env_seed_out[g] = env;
}

// ---- the trace kernel of rt_render_lit_split: lit_render_body's wave loop (kFog and kList false) with the stage in w -------------------
// `indirect`: the second slab, of P.slab's layout and pitch.  w is masked wherever it is used as a work index — here only in split_record;
// the fetch assigns a fresh index, whose top bits are zero: stage 0.
template <bool kLens, class Lit>
__device__ __forceinline__ void split_render_body(const KParams &P, const Lit &T, const LensCam &C, float *indirect) {
    const int lane = (int)(threadIdx.x & (kWave - 1));
    Lane L;
    L.node = kBlocked;
    L.sp = 0;
    L.hit = -1;
    L.closest = 1e30f;
    L.color = mk(0.0f, 0.0f, 0.0f);
    L.beta = mk(1.0f, 1.0f, 1.0f);
    L.depth = 0;
    L.seed = 0;
    int32_t phase = kLightIdle;
    uint32_t w = 0, nee = 0, env = 0, med = 0;
    LitCarry<Lit> prev_diffuse = LitCarry<Lit>(0);
    f3 next_d = mk(0, 0, 0);
    LitSamples S;
    S.adir = S.ac = S.bdir = S.bc = mk(0, 0, 0);
    S.code = -1;
    S.a = S.b = false;
    uint32_t pool_next = 0, pool_end = 0;  // (wave-uniform)
    bool exhausted = false;
    for (;;) {
        RTP_LIT_POOL_FETCH(P.total_work, mine)
        const bool busy = phase != kLightIdle;
        if (!__any(busy)) {
            if (exhausted) break;
            continue;
        }
        const bool walking = busy && !traversal_finished<true>(L, kBlocked);
        const bool ready = busy && !walking;
        const int n_walk = __popcll(__ballot(walking));
        const int n_ready = __popcll(__ballot(ready));
        if (n_walk == 0 || n_ready >= kLightShadeLanes) {
            if (ready) {
                if (phase == kLightPath) {
                    f3 next_o;
                    LitCarry<Lit> diffuse;
                    const uint32_t stage = w >> kSplitStageShift;
                    const bool more = shade_lit2(L, P, T, prev_diffuse, nee, env, next_o, next_d, S, diffuse);
                    prev_diffuse = diffuse;
                    if (stage == 1u) {          // what the first diffuse event's ray found is in: the path crosses
                        split_store(P.slab, split_record(P, w & kSplitWorkMask), L.color);
                        L.color = mk(0.0f, 0.0f, 0.0f);
                        w = (w & kSplitWorkMask) | (2u << kSplitStageShift);
                    } else if (stage == 0u && split_diffuse(diffuse)) {
                        w |= 1u << kSplitStageShift;
                    }
                    if (kLitGlossy<Lit> && !more && (S.a || S.b)) next_d = mk(0, 0, 0);
                    if (S.a) {
                        begin_ray(L, next_o, S.adir, 0);
                        phase = S.b ? kLitShadowAB : kLitShadowA;
                    } else if (S.b) {
                        begin_ray(L, next_o, S.bdir, 0);
                        phase = kLitShadowB;
                    } else if (more) {
                        begin_ray(L, next_o, next_d, 0);
                    } else {
                        split_finish(P, indirect, w, L.color);
                        phase = kLightIdle;
                    }
                } else if (phase == kLitShadowB) {
                    if (L.hit < 0) L.color = add(L.color, S.bc);
                    if (kLitGlossy<Lit> && no_next_ray(next_d)) {
                        split_finish(P, indirect, w, L.color);
                        phase = kLightIdle;
                    } else {
                        begin_ray(L, L.o, next_d, 0);
                        phase = kLightPath;
                    }
                } else {
                    if (L.hit == S.code) L.color = add(L.color, S.ac);
                    const bool then_env = phase == kLitShadowAB;
                    if (kLitGlossy<Lit> && !then_env && no_next_ray(next_d)) {
                        split_finish(P, indirect, w, L.color);
                        phase = kLightIdle;
                    } else {
                        begin_ray(L, L.o, then_env ? S.bdir : next_d, 0);
                        phase = then_env ? kLitShadowB : kLightPath;
                    }
                }
                if (phase == kLightIdle) {
                    L.node = kBlocked;
                    L.sp = 0;
                }
            }
        } else {
            const bool occlusion = phase == kLitShadowB;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, occlusion);
            }
        }
    }
    (void)med;
}

template <bool kLens, class Table>
__global__ void __launch_bounds__(256) lit_split_probe_kernel(const KParams P, const Lit<Table> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                                              float *indirect_out) {
    split_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out, indirect_out);
}
template <bool kLens, class Table>
__global__ void __launch_bounds__(256) lit_gloss_split_probe_kernel(const KParams P, const GlossLit<Table> T, const LensCam C, uint32_t *nee_seed_out,
                                                                    uint32_t *env_seed_out, float *indirect_out) {
    split_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out, indirect_out);
}
// (waves per SIMD: those of the kernels they restate — 4, and kLitGlossWaves for the gloss types)
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, 4) lit_split_render_kernel(const KParams P, const Lit<Table> T, const LensCam C, float *indirect) {
    split_render_body<kLens>(P, T, C, indirect);
}
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, (kLitGlossWaves<kLens, Table>)) lit_gloss_split_render_kernel(const KParams P, const GlossLit<Table> T, const LensCam C,
                                                                                                               float *indirect) {
    split_render_body<kLens>(P, T, C, indirect);
}
template <bool kLens, class Table> const void *lit_split_kernel_of(const Lit<Table> &) { return (const void *)lit_split_render_kernel<kLens, Table>; }
template <bool kLens, class Table> const void *lit_split_kernel_of(const GlossLit<Table> &) { return (const void *)lit_gloss_split_render_kernel<kLens, Table>; }

}  // namespace rtk
