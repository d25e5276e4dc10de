// rt_light.hip.inc — the path that takes light samples, written once for both kinds of light: the emissive spheres of rt_render_nee
// (NeeTable, rt_nee.hip.inc; DESIGN.md §13; with emissive planes: EmitTable, §17) and the environment of rt_render_env (EnvDev, rt_env.hip.inc; §14) — and, at the end, for
// both at once from the lens camera (rt_render_lit, Lit<Table>; §16).  Included by rt_capi.hip after both.  A light is its table type; what the two do differently is the overloads below, everything else — the lit vertex, the
// walk step, the probe and the trace kernel — is one text.
#pragma once

namespace rtk {

constexpr int kLightBlock = 256;
constexpr uint32_t kLightChunk = 128u;                       // work indices a wave reserves per atomic
constexpr int kLightShadeLanes = 32;                         // a wave shades once this many lanes are ready (or none is walking)

// ---- what a light is ---------------------------------------------------------------------------------------------------------------
// An emitter table is one of four: the sphere-only table, the two-kind one (sample_planes = 1 on a handle whose table holds a plane;
// DESIGN.md §17), or either under a light tree (select = 1; §18).  What the four share is written once, on the table inside:
__device__ __forceinline__ const NeeTable &emitter_base(const NeeTable &T) { return T; }
__device__ __forceinline__ const EmitTable &emitter_base(const EmitTable &T) { return T; }
__device__ __forceinline__ const NeeTable &emitter_base(const TreeTable &T) { return T.N; }
__device__ __forceinline__ const EmitTable &emitter_base(const TreeEmitTable &T) { return T.N; }
// pmf_e of entry e for a vertex at x: the table's own, or the tree's (tree_pmf, from x)
template <class Table> __device__ __forceinline__ float entry_pmf(const Table &T, int32_t e, f3) { return T.pmf[e]; }
__device__ __forceinline__ float entry_pmf(const TreeTable &T, int32_t e, f3 x) { return tree_pmf(T.L, e, x); }
__device__ __forceinline__ float entry_pmf(const TreeEmitTable &T, int32_t e, f3 x) { return tree_pmf(T.L, e, x); }
// Below, an overload on `const Table &` is every emitter table's — these four and no other type — and the one on EnvDev the environment's.
template <class T>
constexpr bool kEmitterTable = std::is_same_v<T, NeeTable> || std::is_same_v<T, EmitTable> || std::is_same_v<T, TreeTable> || std::is_same_v<T, TreeEmitTable>;

// the key of its RNG stream: light = wang_hash(sample_seed ^ key)
template <class Table> __device__ __forceinline__ uint32_t light_key(const Table &) { static_assert(kEmitterTable<Table>, "not an emitter table"); return kNeeStreamKey; }
__device__ __forceinline__ uint32_t light_key(const EnvDev &) { return kEnvStreamKey; }
// are light samples drawn at all?  (A tree table is never empty: the host hands an empty table to the kernels of select = 0)
template <class Table> __device__ __forceinline__ bool light_on(const Table &T) { return emitter_base(T).count > 0; }
__device__ __forceinline__ bool light_on(const EnvDev &E) { return E.sampled != 0; }
// Is its shadow ray an occlusion query?  The environment's is: it contributes when it hits nothing, an answer that does not depend on
// the visit order, and up to the first accepted hit the walk is the closest-hit search's own (closest is still 1e30) — so the walk ends
// there.  An emitter's shadow ray has to find that sphere as its closest hit: a full walk.
template <class Light> constexpr bool kLightOcclusion = false;
template <> constexpr bool kLightOcclusion<EnvDev> = true;

// miss: what the lane's ray adds when it hits nothing
// (Carry: the carried value's type — bool in the kernels without glossy events, float in those with; rt_nee.hip.inc)
template <class Table, class Carry> __device__ __forceinline__ f3 light_miss(const KParams &P, const Table &, const Lane &L, Carry) {
    static_assert(kEmitterTable<Table>, "not an emitter table");
    return mul(L.beta, mk(P.bg[0], P.bg[1], P.bg[2]));
}
template <class Carry> __device__ __forceinline__ f3 light_miss(const KParams &P, const EnvDev &E, const Lane &L, Carry prev_diffuse) {
    if (L.depth == 0 && !E.camera_visible) return mul(L.beta, mk(P.bg[0], P.bg[1], P.bg[2]));
    return env_miss(E, L.d, L.beta, prev_diffuse);
}
// emitted: beta * emitted of the hit (sphere or plane idx) — weighted when a BSDF ray from a diffuse event found a table sphere; the
// environment leaves it to the path alone.  Once per kind of table (B: T's emitter_base), with pmf_e by entry_pmf from the ray's origin
template <class Table, class Carry>
__device__ __forceinline__ f3 emitter_emitted(const KParams &P, const Table &T, const NeeTable &B, const Lane &L, int32_t idx, bool is_plane, Carry prev_diffuse, f3 emitted) {
    if (carry_on(prev_diffuse) && !is_plane) {
        const int32_t e = nee_find(B, idx);
        if (e >= 0) {
            f3 w;
            float d2, om, pl = 0.0f;
            if (nee_cone(L.o, P.spheres[idx], w, d2, om)) pl = entry_pmf(T, e, L.o) * nee_pdf_cone(om);
            const float pb = carry_pb(prev_diffuse);
            const float wb = B.mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
            emitted = scale(wb, emitted);
        }
    }
    return emitted;
}
// (the two-kind table: a table sphere as above, a table plane by step 3p from the ray's origin to the vertex's point)
template <class Table, class Carry>
__device__ __forceinline__ f3 emitter_emitted(const KParams &P, const Table &T, const EmitTable &B, const Lane &L, int32_t idx, bool is_plane, Carry prev_diffuse, f3 emitted) {
    if (carry_on(prev_diffuse)) {
        const int32_t e = emit_find(B, L.hit);
        if (e >= 0) {
            f3 w;
            float pl = 0.0f;
            if (is_plane) {
                float pa;
                if (emit_plane_pa(P, idx, B.area[e], L.o, add(L.o, scale(L.closest, L.d)), w, pa)) pl = entry_pmf(T, e, L.o) * pa;
            } else {
                float d2, om;
                if (nee_cone(L.o, P.spheres[idx], w, d2, om)) pl = entry_pmf(T, e, L.o) * nee_pdf_cone(om);
            }
            const float pb = carry_pb(prev_diffuse);
            const float wb = B.mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
            emitted = scale(wb, emitted);
        }
    }
    return emitted;
}
template <class Table, class Carry>
__device__ __forceinline__ f3 light_emitted(const KParams &P, const Table &T, const Lane &L, int32_t idx, bool is_plane, Carry prev_diffuse, f3 emitted) {
    return emitter_emitted(P, T, emitter_base(T), L, idx, is_plane, prev_diffuse, emitted);
}
template <class Carry>
__device__ __forceinline__ f3 light_emitted(const KParams &, const EnvDev &, const Lane &, int32_t, bool, Carry, f3 emitted) { return emitted; }
// sample: the light sample of a diffuse vertex at x (face-forwarded normal n, albedo a, throughput beta before the attenuation).  false:
// none; else the shadow ray's direction, what it adds when it reaches the light, and (emitters) the code of the sphere to reach.  A tree
// table picks by tree_pick, with pmf_e(x) from the descent.  PB: the BSDF strategy's density in the sampled direction (PbDiffuse, or
// PbGlossy at a glossy event)
template <class Pb>
__device__ __forceinline__ bool light_sample(const KParams &P, const NeeTable &T, uint32_t &ls, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    return nee_sample(P, T, ls, x, n, a, beta, PB, dir, c, code);
}
template <class Pb>
__device__ __forceinline__ bool light_sample(const KParams &P, const EmitTable &T, uint32_t &ls, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    return emit_sample(P, T, ls, x, n, a, beta, PB, dir, c, code);
}
template <class Pb>
__device__ __forceinline__ bool light_sample(const KParams &P, const TreeTable &T, uint32_t &ls, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    return tree_sample(P, T, ls, x, n, a, beta, PB, dir, c, code);
}
template <class Pb>
__device__ __forceinline__ bool light_sample(const KParams &P, const TreeEmitTable &T, uint32_t &ls, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    return tree_sample(P, T, ls, x, n, a, beta, PB, dir, c, code);
}
template <class Pb>
__device__ __forceinline__ bool light_sample(const KParams &, const EnvDev &E, uint32_t &ls, f3, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &) {
    return env_sample(E, ls, n, a, beta, PB, dir, c);
}
// reached: the verdict of a finished shadow walk
template <class Table> __device__ __forceinline__ bool light_reached(const Table &, const Lane &L, int32_t code) { static_assert(kEmitterTable<Table>, "not an emitter table"); return L.hit == code; }
__device__ __forceinline__ bool light_reached(const EnvDev &, const Lane &L, int32_t) { return L.hit < 0; }

// the light samples' RNG state of a sample (the path's own is start_sample's)
template <class Light>
__device__ __forceinline__ uint32_t light_seed_of(const Light &T, uint32_t base_seed, int32_t s) {
    return wang_hash(wang_hash(base_seed + (uint32_t)s) ^ light_key(T));
}

// ---- the lit vertex ----------------------------------------------------------------------------------------------------------------
// shade() of the exact walk (kGuard = false, the global material table, the general build) with light samples:
//   prev_diffuse: the ray that found this hit (or nothing) left a diffuse event at its origin L.o; diffuse_out: this vertex is one (the
//   next ray's prev_diffuse); sample: it takes a light sample — the shadow ray (out_o, sdir), which adds c when it reaches the light
//   (code).  Only an event whose next query is inside max_depth samples, and out_o — the hit point — is both rays' origin.  A diffuse
//   event that samples always has a next ray.  A glossy event (METAL's reflect branch with fuzz >= RT_GLOSSY_MIN_FUZZ, in the
//   instantiations that have them: DESIGN.md §23) samples before the absorption test, so it may sample and return false — "sample, but
//   no next ray": the caller ends the path behind the shadow verdict.
// The main stream's draws, the branches, the roulette and the next ray are shade()'s.
// The vertex is one text for both of its forms — shade_lit (one light sample) and, at the end of this file, shade_lit2 (the emitter's
// and the environment's): RTP_LIT_VERTEX, the body of a function with L, P, T, prev_diffuse, out_o, out_d and diffuse_out (set to false)
// in scope.  TAKE_SAMPLES is the statement a diffuse event runs for its light samples, with point, normal, albedo and beta_in (the
// throughput before the attenuation) at hand; GLOSSY_SAMPLES the one METAL's reflect branch runs before its absorption test, with refl
// (the mirror direction), new_d and absorbed at hand as well — empty where there are no glossy events.
#define RTP_LIT_VERTEX(TAKE_SAMPLES, GLOSSY_SAMPLES)                                                                                                 \
    if (L.hit < 0) {                                                                                                                                 \
        L.color = add(L.color, light_miss(P, T, L, prev_diffuse));                                                                                   \
        return false;                                                                                                                                \
    }                                                                                                                                                \
    const int32_t hit = L.hit;                                                                                                                       \
    const int32_t idx = hit >> 1;                                                                                                                    \
    const float t = L.closest;                                                                                                                       \
    const f3 point = add(L.o, scale(t, L.d));  /* r.at(rec.t) */                                                                                     \
    f3 normal;                                                                                                                                       \
    bool front;                                                                                                                                      \
    int32_t mat_idx;                                                                                                                                 \
    float tu = 0.0f, tv = 0.0f;                                                                                                                      \
    const bool is_plane = (hit & 1) != 0;                                                                                                            \
    f3 outward = mk(0, 0, 0);                                                                                                                        \
    if (is_plane) {                                                                                                                                  \
        const float4 P0 = P.planes[5 * idx + 0];                                                                                                     \
        const float4 P2 = P.planes[5 * idx + 2];                                                                                                     \
        outward = mk(P0.x, P0.y, P0.z);                                                                                                              \
        mat_idx = as_int(P2.w);                                                                                                                      \
    } else {                                                                                                                                         \
        const float4 s = P.spheres[idx];                                                                                                             \
        outward = divs(sub(point, mk(s.x, s.y, s.z)), s.w);                                                                                          \
        mat_idx = P.sphere_mat[idx];                                                                                                                 \
    }                                                                                                                                                \
    front = dot(L.d, outward) < 0;                                                                                                                   \
    normal = front ? outward : neg(outward);                                                                                                         \
                                                                                                                                                     \
    const float4 MA = P.materials[3 * mat_idx + 0];                                                                                                  \
    const float4 ME = P.materials[3 * mat_idx + 1];                                                                                                  \
    const int32_t type = as_int(MA.w) & 3;                                                                                                           \
    const int32_t tex_id = as_int(MA.w) >> 2;                                                                                                        \
    f3 albedo = mk(MA.x, MA.y, MA.z);                                                                                                                \
    if (tex_id != 0) {                                                                                                                               \
        if (is_plane) {                                                                                                                              \
            const float4 P1 = P.planes[5 * idx + 1];                                                                                                 \
            const float4 P2 = P.planes[5 * idx + 2];                                                                                                 \
            const float4 P3 = P.planes[5 * idx + 3];                                                                                                 \
            const float4 P4 = P.planes[5 * idx + 4];                                                                                                 \
            const f3 ph = sub(point, mk(P4.x, P4.y, P4.z));                                                                                          \
            const f3 w = mk(P1.x, P1.y, P1.z);                                                                                                       \
            tu = dot(w, cross(ph, mk(P3.x, P3.y, P3.z)));                                                                                            \
            tv = dot(w, cross(mk(P2.x, P2.y, P2.z), ph));                                                                                            \
        } else {                                                                                                                                     \
            const float theta = acos_libm(outward.y);                                                                                                \
            const float phi = (float)((double)atan2_libm(-outward.z, outward.x) + 3.14159265358979323846);                                           \
            tu = (float)((double)phi / (2 * 3.14159265358979323846));                                                                                \
            tv = (float)((double)theta / 3.14159265358979323846);                                                                                    \
        }                                                                                                                                            \
        albedo = mul(albedo, sample_texture(P, tex_id - 1, tu, tv));                                                                                 \
    }                                                                                                                                                \
    const f3 beta_in = L.beta;                                                                                                                       \
    const f3 emitted = light_emitted(P, T, L, idx, is_plane, prev_diffuse, mul(beta_in, mk(ME.x, ME.y, ME.z)));  /* final_color += beta * emitted */ \
                                                                                                                                                     \
    f3 new_o = point, new_d = normal, att = albedo;                                                                                                  \
    const bool is_lamb = type == RT_MAT_LAMBERTIAN;                                                                                                  \
    const bool is_metal = type == RT_MAT_METAL;                                                                                                      \
    const bool is_glass = type == RT_MAT_DIELECTRIC;                                                                                                 \
    if (!(is_lamb || is_metal || is_glass)) {  /* DIFFUSE_LIGHT */                                                                                   \
        L.color = add(L.color, emitted);                                                                                                             \
        return false;                                                                                                                                \
    }                                                                                                                                                \
    float4 MB = make_float4(0.0f, 0.0f, 0.0f, 1.0f);                                                                                                 \
    if (is_glass) MB = P.materials[3 * mat_idx + 2];                                                                                                 \
    bool metal_reflect = false;                                                                                                                      \
    if (is_metal) metal_reflect = random_float(L.seed) < 0.8f;                                                                                       \
    f3 in_sphere = mk(0, 0, 0);                                                                                                                      \
    if (is_lamb || is_metal) in_sphere = random_in_unit_sphere(L.seed);                                                                              \
    L.color = add(L.color, emitted);                                                                                                                 \
    f3 ud = mk(0, 0, 0);                                                                                                                             \
    if (metal_reflect || is_glass) ud = unit(L.d);                                                                                                   \
    if (is_glass) {                                                                                                                                  \
        const float ir = MB.w;                                                                                                                       \
        const float ratio = front ? ME.w : ir;                                                                                                       \
        const float cos_theta = fminf(dot(neg(ud), normal), 1.0f);                                                                                   \
        const float sin_theta = sqrt_cr(1.0f - cos_theta * cos_theta);                                                                               \
        const bool cannot_refract = ratio * sin_theta > 1.0f;                                                                                        \
        bool do_reflect = cannot_refract;                                                                                                            \
        if (!cannot_refract) {                                                                                                                       \
            const float rnd = random_float(L.seed);                                                                                                  \
            do_reflect = schlick_exceeds(cos_theta, front ? MA.x : MA.y, rnd);                                                                       \
        }                                                                                                                                            \
        new_d = do_reflect ? reflect(ud, normal) : refract(ud, normal, ratio);                                                                       \
        att = mk(1.0f, 1.0f, 1.0f);                                                                                                                  \
        if (!front) {                                                                                                                                \
            const float dist = sqrt_cr(lensq(sub(point, L.o)));                                                                                      \
            const f3 tr = mk(MB.x == 0.0f ? 1.0f : exp_libm(-MB.x * dist), MB.y == 0.0f ? 1.0f : exp_libm(-MB.y * dist),                             \
                             MB.z == 0.0f ? 1.0f : exp_libm(-MB.z * dist));                                                                          \
            att = mul(att, tr);                                                                                                                      \
        }                                                                                                                                            \
        const float p = fmaxf(att.x, fmaxf(att.y, att.z));                                                                                           \
        if (random_float(L.seed) > p) return false;  /* Russian roulette */                                                                          \
        if (p != 1.0f) att = scale(recip(p), att);                                                                                                   \
        const float side = dot(new_d, normal) > 0 ? 1.0f : -1.0f;                                                                                    \
        new_o = add(point, scale(side, scale(1e-4f, normal)));                                                                                       \
    } else if (metal_reflect) {                                                                                                                      \
        const f3 refl = reflect(ud, normal);                                                                                                         \
        new_d = add(refl, scale(ME.w, in_sphere));                                                                                                   \
        const bool absorbed = !(dot(new_d, normal) > 0);                                                                                             \
        GLOSSY_SAMPLES                                                                                                                               \
        if (absorbed) return false;                                                                                                                  \
    } else {  /* LAMBERTIAN and METAL's 20 % branch: a diffuse event */                                                                              \
        new_d = scatter_diffuse_dir(in_sphere, normal);                                                                                              \
        carry_diffuse(diffuse_out);                                                                                                                  \
        TAKE_SAMPLES                                                                                                                                 \
    }                                                                                                                                                \
    L.beta = mul(L.beta, att);                                                                                                                       \
    L.depth++;                                                                                                                                       \
    if (L.depth >= P.max_depth) return false;                                                                                                        \
    out_o = new_o;                                                                                                                                   \
    out_d = new_d;                                                                                                                                   \
    return true;
// Carry = bool: the vertex without glossy events (glossy = 0: the kernels as they were); Carry = float: with them (the light's glossy = 1)
template <class Light, class Carry>
__device__ __forceinline__ bool shade_lit(Lane &L, const KParams &P, const Light &T, Carry prev_diffuse, uint32_t &ls, f3 &out_o, f3 &out_d,
                                          f3 &sdir, f3 &c, int32_t &code, bool &sample, Carry &diffuse_out) {
    sample = false;
    diffuse_out = Carry(0);
    RTP_LIT_VERTEX(if (L.depth + 1 < P.max_depth && light_on(T)) sample = light_sample(P, T, ls, point, normal, albedo, beta_in, PbDiffuse{}, sdir, c, code);,
                   if constexpr (std::is_same_v<Carry, float>) {
                       if (ME.w >= kGlossMinFuzz && L.depth + 1 < P.max_depth && light_on(T)) {
                           sample = light_sample(P, T, ls, point, normal, albedo, beta_in, gloss_pb(refl, ME.w), sdir, c, code);
                           out_o = point;
                           if (!absorbed) diffuse_out = gloss_pg(unit(new_d), refl, ME.w);
                       }
                   })
}
// "sample, but no next ray" across a shadow walk: the pending direction is zeroed (a next ray's never is: dot(new_d, normal) > 0), so
// the glossy instantiations hold no register more than the others
__device__ __forceinline__ bool no_next_ray(f3 d) { return d.x == 0.0f && d.y == 0.0f && d.z == 0.0f; }

// one step of the lane's armed ray: reference order, through L1 / L2 (shadow: the ray is a shadow ray)
template <class Light>
__device__ __forceinline__ void light_step(Lane &L, const KParams &P, bool shadow) {
    if (L.sp != 0) {
        leaf_threaded(L, P.spheres, P.planes);
        if (kLightOcclusion<Light> && shadow && L.hit >= 0) L.node = kBlocked;
    } else {
        step_threaded(L, P.tnodes, P.num_tnodes);
    }
}

// ---- probe (rt_trace_samples_nee / _env): one lane traces one (i, j, s) sample -------------------------------------------------------
template <class Light, bool kGlossy = false>
__device__ __forceinline__ void light_probe_body(const KParams &P, const Light &T, uint32_t *light_seed_out) {
    using Carry = std::conditional_t<kGlossy, float, bool>;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    uint32_t ls = light_seed_of(T, base_seed, s);
    f3 ray_o, ray_d;
    start_sample(L, P, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0;
    Carry prev_diffuse = Carry(0);
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            while (!traversal_finished<true>(L, kBlocked)) light_step<Light>(L, P, false);
            f3 sdir, c;
            int32_t code = -1;
            bool sample;
            Carry diffuse;
            const bool more = shade_lit(L, P, T, prev_diffuse, ls, ray_o, ray_d, sdir, c, code, sample, diffuse);
            if (sample) {
                rays++;
                begin_ray(L, ray_o, sdir, 0);
                while (!traversal_finished<true>(L, kBlocked)) light_step<Light>(L, P, true);
                if (light_reached(T, L, code)) L.color = add(L.color, c);
            }
            if (!more) break;
            prev_diffuse = diffuse;
            begin_ray(L, ray_o, ray_d, 0);
        }
    }
    P.probe_rad[3 * g] = L.color.x; P.probe_rad[3 * g + 1] = L.color.y; P.probe_rad[3 * g + 2] = L.color.z;
    P.probe_rays[g] = rays;
    P.probe_seed[g] = L.seed;
    light_seed_out[g] = ls;
}

// ---- the trace kernel of rt_render_nee / rt_render_env: one pass of samples into the slab -------------------------------------------
// Persistent waves fetch work indices kLightChunk at a time (one atomic per wave) and hand them to lanes as they free up.  Each lane
// is a small state machine — walking its path ray, walking a shadow ray, or idle — and the wave either takes up to four walk steps for
// the lanes that walk or, once kLightShadeLanes lanes (or all that are busy) have finished their walk, one shade step for those: the
// path's shade (shade_lit), or the shadow ray's verdict.
// Across a shadow walk a lane holds the next ray's direction, the pending contribution and the code to reach (seven registers; the
// code is dead for the environment): the next ray's origin is the shadow ray's own (L.o), and a vertex that samples always has a next
// ray, so no flag for it either.  kGlossy (the light's glossy = 1): a glossy event may sample without a next ray — the pending
// direction is then zero, and the shadow verdict ends the path (no_next_ray); the carried value is a float.
constexpr int32_t kLightIdle = 0, kLightPath = 1, kLightShadow = 2;
// The first half of a wave loop's fetch — RTP_LIGHT_POOL_RESERVE, statements inside `if (idle != 0 && !exhausted)` with lane, idle, P, pool_next,
// pool_end and exhausted in scope: every idle lane gets the next work index of the wave's pool as `mine` (the pool refilled with one atomic per
// wave, kLightChunk indices at a time); a chunk that starts at or past TOTAL (wave-uniform) marks the wave exhausted.  `mine` may lie past
// TOTAL.  Used by light_render_body and by lit_render_body's fetch (RTP_LIT_POOL_FETCH) and, through it, rt_glow_sample.hip.inc's, which undefines it.
#define RTP_LIGHT_POOL_RESERVE(TOTAL)                                                                                 \
            const uint32_t cnt = (uint32_t)__popcll(idle);                                                            \
            const uint32_t rank = (uint32_t)lane_rank(idle);                                                          \
            const uint32_t avail = pool_end - pool_next;                                                              \
            uint32_t mine;                                                                                            \
            if (avail < cnt) {                                                                                        \
                uint32_t base = 0;                                                                                    \
                if (lane == 0) base = atomicAdd(P.queue, kLightChunk);                                                \
                base = __builtin_amdgcn_readfirstlane(base);                                                          \
                mine = rank < avail ? pool_next + rank : base + (rank - avail);                                       \
                pool_next = base + (cnt - avail);                                                                     \
                pool_end = base + kLightChunk;                                                                        \
                if (base >= (TOTAL)) exhausted = true;                                                                \
            } else {                                                                                                  \
                mine = pool_next + rank;                                                                              \
                pool_next += cnt;                                                                                     \
            }
template <class Light, bool kGlossy = false>
__device__ __forceinline__ void light_render_body(const KParams &P, const Light &T) {
    using Carry = std::conditional_t<kGlossy, float, bool>;
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
    uint32_t w = 0, ls = 0;
    Carry prev_diffuse = Carry(0);
    f3 next_d = mk(0, 0, 0), contrib = mk(0, 0, 0);
    int32_t target = -1;
    uint32_t pool_next = 0, pool_end = 0;        // (wave-uniform)
    bool exhausted = false;
    for (;;) {
        // ---- lanes without a sample take the next work indices of the wave's pool (refilled with one atomic)
        const uint64_t idle = __ballot(phase == kLightIdle);
        if (idle != 0 && !exhausted) {
            RTP_LIGHT_POOL_RESERVE(P.total_work)
            if (phase == kLightIdle && mine < P.total_work) {
                w = mine;
                int32_t pi, pj;
                uint32_t k;
                map_work(P, w, pi, pj, k);
                const int32_t s = P.pass_first + (int32_t)k;
                const uint32_t base_seed = wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj);
                ls = light_seed_of(T, base_seed, s);
                f3 o, d;
                start_sample(L, P, pi, pj, base_seed, s, o, d);
                begin_ray(L, o, d, 0);
                prev_diffuse = Carry(0);
                phase = kLightPath;
            }
        }
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
                    f3 next_o, sdir;
                    bool sample;
                    Carry diffuse;
                    const bool more = shade_lit(L, P, T, prev_diffuse, ls, next_o, next_d, sdir, contrib, target, sample, diffuse);
                    prev_diffuse = diffuse;
                    if (sample) {
                        if constexpr (kGlossy) {
                            if (!more) next_d = mk(0, 0, 0);
                        }
                        begin_ray(L, next_o, sdir, 0);
                        phase = kLightShadow;
                    } else if (more) {
                        begin_ray(L, next_o, next_d, 0);
                    } else {
                        store_sample(P, w, L.color);
                        phase = kLightIdle;
                    }
                } else {
                    if (light_reached(T, L, target)) L.color = add(L.color, contrib);
                    if (kGlossy && no_next_ray(next_d)) {
                        store_sample(P, w, L.color);
                        phase = kLightIdle;
                    } else {
                        begin_ray(L, L.o, next_d, 0);
                        phase = kLightPath;
                    }
                }
                if (phase == kLightIdle) {
                    L.node = kBlocked;
                    L.sp = 0;
                }
            }
        } else {
            const bool shadow = phase == kLightShadow;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!traversal_finished<true>(L, kBlocked)) light_step<Light>(L, P, shadow);
            }
        }
    }
}

// Light: NeeTable, EmitTable, TreeTable, TreeEmitTable or EnvDev
template <class Light>
__global__ void __launch_bounds__(256) light_probe_kernel(const KParams P, const Light T, uint32_t *light_seed_out) { light_probe_body(P, T, light_seed_out); }
template <class Light>
__global__ void __launch_bounds__(kLightBlock) light_render_kernel(const KParams P, const Light T) { light_render_body(P, T); }
// the same two with glossy events (the light's glossy = 1; DESIGN.md §23): instantiations of their own, so that glossy = 0 launches the
// kernels above as they were
template <class Light>
__global__ void __launch_bounds__(256) light_gloss_probe_kernel(const KParams P, const Light T, uint32_t *light_seed_out) { light_probe_body<Light, true>(P, T, light_seed_out); }
template <class Light>
__global__ void __launch_bounds__(kLightBlock) light_gloss_render_kernel(const KParams P, const Light T) { light_render_body<Light, true>(P, T); }

// ---- rt_render_lit: the emitter table and an environment at once, from the lens camera (DESIGN.md §16) -------------------------------
// The third light: both tables, either of which may be off (an emitter table with count 0 — sample_emitters = 0 or no emitter; env_on = 0
// — no environment: a miss adds the background).  Spheres are hits and the map is misses, so the two never weight the same radiance:
// miss and emitted are the single lights' own, and a vertex takes one sample of each light that is on, from that light's own stream.
// Table: the call's emitter table, any of the four.
template <class Table>
struct Lit {
    Table N;
    EnvDev E;
    int32_t env_on;
};
template <class Table>
__device__ __forceinline__ f3 light_miss(const KParams &P, const Lit<Table> &T, const Lane &L, bool prev_diffuse) {
    if (T.env_on) return light_miss(P, T.E, L, prev_diffuse);
    return light_miss(P, T.N, L, prev_diffuse);
}
template <class Table>
__device__ __forceinline__ f3 light_emitted(const KParams &P, const Lit<Table> &T, const Lane &L, int32_t idx, bool is_plane, bool prev_diffuse, f3 emitted) {
    return light_emitted(P, T.N, L, idx, is_plane, prev_diffuse, emitted);
}
template <class Table>
__device__ __forceinline__ bool env_sampled(const Lit<Table> &T) { return T.env_on && light_on(T.E); }
// The light of a lit call with a glossy switch on (DESIGN.md §23): a type of its own, so that a call with both off launches the kernels
// of Lit<Table> as they were.  gn, ge: the emitters' and the environment's switch.  Its carried value is a float with a sign: RT_NEE_PB
// after a diffuse event, -pg after a glossy one — a ray from a glossy event is weighted only against the lights whose switch is on
// (the switches are the call's, so "on at that vertex" is "on"), and -0 is none.
template <class Table>
struct GlossLit : Lit<Table> {
    int32_t gn, ge;
};
__device__ __forceinline__ float lit_carry(float c, int32_t on) { return c >= 0.0f ? c : (on ? -c : 0.0f); }
template <class Table>
__device__ __forceinline__ f3 light_miss(const KParams &P, const GlossLit<Table> &T, const Lane &L, float prev) {
    if (T.env_on) return light_miss(P, T.E, L, lit_carry(prev, T.ge));
    return light_miss(P, T.N, L, prev);
}
template <class Table>
__device__ __forceinline__ f3 light_emitted(const KParams &P, const GlossLit<Table> &T, const Lane &L, int32_t idx, bool is_plane, float prev, f3 emitted) {
    return light_emitted(P, T.N, L, idx, is_plane, lit_carry(prev, T.gn), emitted);
}
template <class L> constexpr bool kLitGlossy = false;
template <class Table> constexpr bool kLitGlossy<GlossLit<Table>> = true;
template <class L> using LitCarry = std::conditional_t<kLitGlossy<L>, float, bool>;

// The two light samples of a lit vertex: the emitter's (a: the shadow ray has to reach the primitive `code`) and the environment's (b: it has
// to reach nothing).  Both are drawn at shade time — the streams are independent, and the order of the adds is the caller's.
struct LitSamples {
    f3 adir, ac, bdir, bc;
    int32_t code;
    bool a, b;
};
template <class Lit>
__device__ __forceinline__ bool shade_lit2(Lane &L, const KParams &P, const Lit &T, LitCarry<Lit> prev_diffuse, uint32_t &nee, uint32_t &env, f3 &out_o,
                                           f3 &out_d, LitSamples &S, LitCarry<Lit> &diffuse_out) {
    S.a = false;
    S.b = false;
    diffuse_out = LitCarry<Lit>(0);
    RTP_LIT_VERTEX(if (L.depth + 1 < P.max_depth) {
        if (light_on(T.N)) S.a = light_sample(P, T.N, nee, point, normal, albedo, beta_in, PbDiffuse{}, S.adir, S.ac, S.code);
        if (env_sampled(T)) S.b = light_sample(P, T.E, env, point, normal, albedo, beta_in, PbDiffuse{}, S.bdir, S.bc, S.code);
    },
    if constexpr (kLitGlossy<Lit>) {
        if (ME.w >= kGlossMinFuzz && L.depth + 1 < P.max_depth) {
            const bool ga = T.gn && light_on(T.N);
            const bool gb = T.ge && env_sampled(T);
            if (ga || gb) {
                if (!absorbed) diffuse_out = -gloss_pg(unit(new_d), refl, ME.w);
                const PbGlossy pbg = gloss_pb(refl, ME.w);
                if (ga) S.a = light_sample(P, T.N, nee, point, normal, albedo, beta_in, pbg, S.adir, S.ac, S.code);
                if (gb) S.b = light_sample(P, T.E, env, point, normal, albedo, beta_in, pbg, S.bdir, S.bc, S.code);
                out_o = point;
            }
        }
    })
}
// (RTP_LIT_VERTEX stays defined for rt_glow_sample.hip.inc, whose vertex takes a third light sample; it is undefined at that file's end)
// a sample's camera ray: the pinhole's (start_sample), or kLens: the lens / moving camera's
template <bool kLens>
__device__ __forceinline__ void lit_start(Lane &L, const KParams &P, const LensCam &C, int32_t i, int32_t j, uint32_t base_seed, int32_t s, f3 &o, f3 &d) {
    if constexpr (kLens) lens_camera_ray(L, C, i, j, sample_seed1(base_seed, s), o, d);
    else start_sample(L, P, i, j, base_seed, s, o, d);
}
// one step of the lane's armed ray (occlusion: the environment's shadow ray, which ends at its first accepted hit)
__device__ __forceinline__ void lit_step(Lane &L, const KParams &P, bool occlusion) {
    if (L.sp != 0) {
        leaf_threaded(L, P.spheres, P.planes);
        if (occlusion && L.hit >= 0) L.node = kBlocked;
    } else {
        step_threaded(L, P.tnodes, P.num_tnodes);
    }
}

// ---- what fog adds to a lit light (DESIGN.md §31) --------------------------------------------------------------------------------------
// The probe and the wave loop below are written once, for a light with or without fog (Lit<Table>, GlossLit<Table>; MediumLit<Table> and
// VolumeLit<Table> of rt_medium.hip.inc and rt_volume.hip.inc; ChromaLit<Base> of rt_chroma.hip.inc and GlowLit<Base> of rt_glow.hip.inc
// over either).  What differs is four
// functions overloaded on the light's type; those of a light with fog stand in its own file and are found through the light's type where
// the bodies are instantiated:
//   fog_lit(T)                           the light that shade_lit2 and the streams see: T itself, or the GlossLit inside
//   fog_seed(T, base_seed, s)            the start of the sample's medium stream (0: there is none)
//   fog_vertex(L, P, T, …, n)            the free flight in front of the surface vertex.  false: no event — the caller runs shade_lit2, with
//                                        nothing changed but (perhaps) draws of med and, under a chromatic medium, L.beta scaled by the
//                                        channels' weights of having passed the interval and, under a medium that glows, L.color with what it
//                                        emitted over the flight.  true: the vertex was a medium vertex and is done:
//                                        `more` as shade_lit2 returns it, the light samples in S, the next ray (out_o, out_d), what it carries
//   fog_tr(T, o, d, t_end, c, n)         the contribution c of a shadow ray (o, d) that ended at t_end, times its transmittance
// n counts for the probes (FogCount); the wave loop calls the two forms without it, whose counters are their own locals and never read.
struct FogCount {
    int32_t events = 0, cells = 0;       // medium vertices; grid cells visited
};
template <class Table> __device__ __forceinline__ const Lit<Table> &fog_lit(const Lit<Table> &T) { return T; }
template <class Table> __device__ __forceinline__ const GlossLit<Table> &fog_lit(const GlossLit<Table> &T) { return T; }
template <class Table> __device__ __forceinline__ uint32_t fog_seed(const Lit<Table> &, uint32_t, int32_t) { return 0; }
template <class Table, class Carry>
__device__ __forceinline__ bool fog_vertex(Lane &, const KParams &, const Lit<Table> &, uint32_t &, uint32_t &, uint32_t &, f3 &, f3 &, LitSamples &, Carry &, bool &,
                                           FogCount &) {
    return false;
}
template <class Table> __device__ __forceinline__ f3 fog_tr(const Lit<Table> &, f3, f3, float, f3 c, FogCount &) { return c; }
template <class Light, class Carry>
__device__ __forceinline__ bool fog_vertex(Lane &L, const KParams &P, const Light &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o, f3 &out_d, LitSamples &S,
                                           Carry &carry_out, bool &more) {
    FogCount n;
    return fog_vertex(L, P, T, nee, env, med, out_o, out_d, S, carry_out, more, n);
}
template <class Light>
__device__ __forceinline__ f3 fog_tr(const Light &T, f3 o, f3 d, float t_end, f3 c) {
    FogCount n;
    return fog_tr(T, o, d, t_end, c, n);
}

// ---- probe (rt_trace_samples_lit, _medium, _volume) ------------------------------------------------------------------------------------
// med_seed_out and events_out (a light under a medium), cells_out (a density grid): null where the call has no such column
template <bool kLens, class Light>
__device__ __forceinline__ void lit_probe_body(const KParams &P, const Light &T, const LensCam &C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                               uint32_t *med_seed_out = nullptr, int32_t *events_out = nullptr, int32_t *cells_out = nullptr) {
    using Lit = std::decay_t<decltype(fog_lit(T))>;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    uint32_t nee = light_seed_of(fog_lit(T).N, base_seed, s), env = light_seed_of(fog_lit(T).E, base_seed, s), med = fog_seed(T, base_seed, s);
    f3 ray_o, ray_d;
    lit_start<kLens>(L, P, C, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0;
    FogCount n;
    LitCarry<Lit> prev_diffuse = LitCarry<Lit>(0);
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
            LitSamples S;
            S.code = -1;
            LitCarry<Lit> diffuse;
            bool more;
            if (!fog_vertex(L, P, T, nee, env, med, ray_o, ray_d, S, diffuse, more, n))
                more = shade_lit2(L, P, fog_lit(T), prev_diffuse, nee, env, ray_o, ray_d, S, diffuse);
            if (S.a) {
                rays++;
                begin_ray(L, ray_o, S.adir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
                if (L.hit == S.code) L.color = add(L.color, fog_tr(T, L.o, L.d, L.closest, S.ac, n));
            }
            if (S.b) {
                rays++;
                begin_ray(L, ray_o, S.bdir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, true);
                if (L.hit < 0) L.color = add(L.color, fog_tr(T, L.o, L.d, INFINITY, S.bc, n));
            }
            if (!more) break;
            prev_diffuse = diffuse;
            begin_ray(L, ray_o, ray_d, 0);
        }
    }
    P.probe_rad[3 * g] = L.color.x; P.probe_rad[3 * g + 1] = L.color.y; P.probe_rad[3 * g + 2] = L.color.z;
    P.probe_rays[g] = rays;
    P.probe_seed[g] = L.seed;
    nee_seed_out[g] = nee;
    env_seed_out[g] = env;
    if (med_seed_out) {
        med_seed_out[g] = med;
        events_out[g] = n.events;
    }
    if (cells_out) cells_out[g] = n.cells;
}

// ---- the trace kernel of rt_render_lit, rt_render_medium and rt_render_volume ---------------------------------------------------------
// (one wave loop for the four lights, through the hooks above: a light with fog keeps one register more across the walks, the med state,
// and nothing else — a shadow verdict's transmittance needs only the lane's own L.o, L.d and L.closest; DESIGN.md §31)
// light_render_body's wave loop with a second shadow phase: path → emitter shadow (a full closest-hit walk) → environment shadow (ends at
// its first hit) → path; a phase is skipped when its light gave no sample.  kLitShadowAB is the emitter's walk of a vertex whose
// environment sample still waits.  Across the emitter's walk a lane holds the next direction, both pending contributions, the
// environment's direction and the target (thirteen registers); across the environment's, the next direction and its contribution.
constexpr int32_t kLitShadowA = 2, kLitShadowAB = 3, kLitShadowB = 4;
// The fetch of the wave loop — RTP_LIT_POOL_FETCH, a statement with lane, L, P, T, C, phase, w, nee, env, med, prev_diffuse, pool_next,
// pool_end and exhausted in scope: RTP_LIGHT_POOL_RESERVE's index, and the start of the sample it stands for
#define RTP_LIT_POOL_FETCH(TOTAL, WORK_OF_MINE)                                                                     \
        /* ---- lanes without a sample take the next work indices of the wave's pool (refilled with one atomic) */  \
        const uint64_t idle = __ballot(phase == kLightIdle);                                                        \
        if (idle != 0 && !exhausted) {                                                                              \
            RTP_LIGHT_POOL_RESERVE(TOTAL)                                                                           \
            if (phase == kLightIdle && mine < (TOTAL)) {                                                            \
                w = (WORK_OF_MINE);                                                                                 \
                int32_t pi, pj;                                                                                     \
                uint32_t k;                                                                                         \
                map_work(P, w, pi, pj, k);                                                                          \
                const int32_t s = P.pass_first + (int32_t)k;                                                        \
                const uint32_t base_seed = wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj);              \
                nee = light_seed_of(fog_lit(T).N, base_seed, s);                                                    \
                env = light_seed_of(fog_lit(T).E, base_seed, s);                                                    \
                f3 o, d;                                                                                            \
                lit_start<kLens>(L, P, C, pi, pj, base_seed, s, o, d);                                              \
                med = fog_seed(T, base_seed, s);                                                                    \
                begin_ray(L, o, d, 0);                                                                              \
                prev_diffuse = LitCarry<Lit>(0);                                                                    \
                phase = kLightPath;                                                                                 \
            }                                                                                                       \
        }
// The wave loop is one text for both of its forms — RTP_LIT_RENDER_BODY, the body of a function with P, T and C in scope: TOTAL is the
// number of work indices (wave-uniform) and WORK_OF_MINE what the fetched index `mine` stands for.  Expanded twice rather than branched
// on inside, so that the frame kernels compile to what they compiled to before the list variants existed (DESIGN.md §19).  Lit is the type
// of fog_lit(T); the guards kLitGlossy<Lit> are constant-true under fog, whose light is always a GlossLit.  kFog (T has a medium) stands in
// front of the free flight so that without fog the front end emits `more = shade_lit2(…)` alone: with a call that returns false in its
// place, the lit kernels' instructions came out in another order (DESIGN.md §31).
#define RTP_LIT_RENDER_BODY(TOTAL, WORK_OF_MINE)                                                                    \
    const int lane = (int)(threadIdx.x & (kWave - 1));                                                              \
    Lane L;                                                                                                         \
    L.node = kBlocked;                                                                                              \
    L.sp = 0;                                                                                                       \
    L.hit = -1;                                                                                                     \
    L.closest = 1e30f;                                                                                              \
    L.color = mk(0.0f, 0.0f, 0.0f);                                                                                 \
    L.beta = mk(1.0f, 1.0f, 1.0f);                                                                                  \
    L.depth = 0;                                                                                                    \
    L.seed = 0;                                                                                                     \
    int32_t phase = kLightIdle;                                                                                     \
    uint32_t w = 0, nee = 0, env = 0, med = 0;                                                                      \
    LitCarry<Lit> prev_diffuse = LitCarry<Lit>(0);                                                                  \
    f3 next_d = mk(0, 0, 0);                                                                                        \
    LitSamples S;                                                                                                   \
    S.adir = S.ac = S.bdir = S.bc = mk(0, 0, 0);                                                                    \
    S.code = -1;                                                                                                    \
    S.a = S.b = false;                                                                                              \
    uint32_t pool_next = 0, pool_end = 0;  /* (wave-uniform) */                                                     \
    bool exhausted = false;                                                                                         \
    for (;;) {                                                                                                      \
        RTP_LIT_POOL_FETCH(TOTAL, WORK_OF_MINE)                                                                     \
        const bool busy = phase != kLightIdle;                                                                      \
        if (!__any(busy)) {                                                                                         \
            if (exhausted) break;                                                                                   \
            continue;                                                                                               \
        }                                                                                                           \
        const bool walking = busy && !traversal_finished<true>(L, kBlocked);                                        \
        const bool ready = busy && !walking;                                                                        \
        const int n_walk = __popcll(__ballot(walking));                                                             \
        const int n_ready = __popcll(__ballot(ready));                                                              \
        if (n_walk == 0 || n_ready >= kLightShadeLanes) {                                                           \
            if (ready) {                                                                                            \
                if (phase == kLightPath) {                                                                          \
                    f3 next_o;                                                                                      \
                    LitCarry<Lit> diffuse;                                                                          \
                    bool more;                                                                                      \
                    if (!kFog || !fog_vertex(L, P, T, nee, env, med, next_o, next_d, S, diffuse, more))             \
                        more = shade_lit2(L, P, fog_lit(T), prev_diffuse, nee, env, next_o, next_d, S, diffuse);    \
                    prev_diffuse = diffuse;                                                                         \
                    if (kLitGlossy<Lit> && !more && (S.a || S.b)) next_d = mk(0, 0, 0);                             \
                    if (S.a) {                                                                                      \
                        begin_ray(L, next_o, S.adir, 0);                                                            \
                        phase = S.b ? kLitShadowAB : kLitShadowA;                                                   \
                    } else if (S.b) {                                                                               \
                        begin_ray(L, next_o, S.bdir, 0);                                                            \
                        phase = kLitShadowB;                                                                        \
                    } else if (more) {                                                                              \
                        begin_ray(L, next_o, next_d, 0);                                                            \
                    } else {                                                                                        \
                        store_sample(P, w, L.color);                                                                \
                        phase = kLightIdle;                                                                         \
                    }                                                                                               \
                } else if (phase == kLitShadowB) {                                                                  \
                    if (L.hit < 0) L.color = add(L.color, fog_tr(T, L.o, L.d, INFINITY, S.bc));                     \
                    if (kLitGlossy<Lit> && no_next_ray(next_d)) {                                                   \
                        store_sample(P, w, L.color);                                                                \
                        phase = kLightIdle;                                                                         \
                    } else {                                                                                        \
                        begin_ray(L, L.o, next_d, 0);                                                               \
                        phase = kLightPath;                                                                         \
                    }                                                                                               \
                } else {                                                                                            \
                    if (L.hit == S.code) L.color = add(L.color, fog_tr(T, L.o, L.d, L.closest, S.ac));              \
                    const bool then_env = phase == kLitShadowAB;                                                    \
                    if (kLitGlossy<Lit> && !then_env && no_next_ray(next_d)) {                                      \
                        store_sample(P, w, L.color);                                                                \
                        phase = kLightIdle;                                                                         \
                    } else {                                                                                        \
                        begin_ray(L, L.o, then_env ? S.bdir : next_d, 0);                                           \
                        phase = then_env ? kLitShadowB : kLightPath;                                                \
                    }                                                                                               \
                }                                                                                                   \
                if (phase == kLightIdle) {                                                                          \
                    L.node = kBlocked;                                                                              \
                    L.sp = 0;                                                                                       \
                }                                                                                                   \
            }                                                                                                       \
        } else {                                                                                                    \
            const bool occlusion = phase == kLitShadowB;                                                            \
            _Pragma("unroll")                                                                                       \
            for (int u = 0; u < 4; ++u) {                                                                           \
                if (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, occlusion);                              \
            }                                                                                                       \
        }                                                                                                           \
    }
// With a GlossLit light a glossy event may sample without a next ray: next_d is zeroed, and the last shadow verdict ends the path.
// kList = false: the work indices are [0, P.total_work) — a pass of rt_render_lit's.
// kList = true (rt_render_lit_adaptive's rounds; DESIGN.md §19): they are the first *P.work_count entries of P.work_list — a length that lives
// on the device, read once per wave and wave-uniform; a fetched index `mine` then stands for P.work_list[mine], in map_work and in
// store_sample alike.  The fetch itself is the same: chunks of kLightChunk from P.queue until a chunk starts at or past the length, so an
// empty list leaves before the first atomic, a list shorter than a chunk is one wave's (every other wave's first chunk starts past the
// end), and the lanes of a last chunk that reaches past the end stay idle until the wave's next fetch finds the queue dry.
template <bool kLens, class Light, bool kList = false>
__device__ __forceinline__ void lit_render_body(const KParams &P, const Light &T, const LensCam &C) {
    using Lit = std::decay_t<decltype(fog_lit(T))>;
    constexpr bool kFog = !std::is_same_v<Lit, Light>;
    if constexpr (kList) {
        uint32_t listed = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)*P.work_count);
        if (listed > P.work_cap) listed = P.work_cap;          // (never more entries than the list has room for)
        if (listed == 0u) return;
        RTP_LIT_RENDER_BODY(listed, P.work_list[mine])
    } else {
        RTP_LIT_RENDER_BODY(P.total_work, mine)
    }
}
#undef RTP_LIT_RENDER_BODY
// (RTP_LIT_POOL_FETCH and RTP_LIGHT_POOL_RESERVE stay defined for the wave loop of rt_glow_sample.hip.inc, and are undefined at its end)

template <bool kLens, class Table>
__global__ void __launch_bounds__(256) lit_probe_kernel(const KParams P, const Lit<Table> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out) {
    lit_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out);
}
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, 4) lit_render_kernel(const KParams P, const Lit<Table> T, const LensCam C) { lit_render_body<kLens>(P, T, C); }
// the list variant: rt_render_lit_adaptive's rounds (DESIGN.md §19) — the same body on a list whose length lives on the device
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, 4) lit_list_render_kernel(const KParams P, const Lit<Table> T, const LensCam C) { lit_render_body<kLens, Lit<Table>, true>(P, T, C); }

// the same three with a glossy switch on (GlossLit<Table>; DESIGN.md §23)
template <bool kLens, class Table>
__global__ void __launch_bounds__(256) lit_gloss_probe_kernel(const KParams P, const GlossLit<Table> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out) {
    lit_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out);
}
// (waves per SIMD the compiler is held to: 4 like the kernels above, except from the lens camera over the sphere-only tree — that vertex
// holds the mirror direction, the fuzz and the carried value on top of lit_render_kernel<true, TreeTable>'s 128 VGPRs, and at 4 waves it
// would spill three of them to scratch; 3 waves it is, without scratch: DESIGN.md §23)
template <bool kLens, class Table> constexpr int kLitGlossWaves = (kLens && std::is_same_v<Table, TreeTable>) ? 3 : 4;
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, (kLitGlossWaves<kLens, Table>)) lit_gloss_render_kernel(const KParams P, const GlossLit<Table> T, const LensCam C) { lit_render_body<kLens>(P, T, C); }
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, (kLitGlossWaves<kLens, Table>)) lit_gloss_list_render_kernel(const KParams P, const GlossLit<Table> T, const LensCam C) {
    lit_render_body<kLens, GlossLit<Table>, true>(P, T, C);
}
// the kernels of a lit light, by its type
template <bool kLens, class Table> const void *lit_frame_kernel_of(const Lit<Table> &) { return (const void *)lit_render_kernel<kLens, Table>; }
template <bool kLens, class Table> const void *lit_list_kernel_of(const Lit<Table> &) { return (const void *)lit_list_render_kernel<kLens, Table>; }
template <bool kLens, class Table> const void *lit_frame_kernel_of(const GlossLit<Table> &) { return (const void *)lit_gloss_render_kernel<kLens, Table>; }
template <bool kLens, class Table> const void *lit_list_kernel_of(const GlossLit<Table> &) { return (const void *)lit_gloss_list_render_kernel<kLens, Table>; }

}  // namespace rtk
