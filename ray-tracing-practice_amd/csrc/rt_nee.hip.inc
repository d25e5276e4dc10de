// rt_nee.hip.inc — next-event estimation (rt_render_nee; include/rtp_amd.h, rt_nee_params; DESIGN.md §13).  Included by rt_capi.hip
// after rt_kernel.hip.inc, whose walk (step_threaded / leaf_threaded on the reference-order table) and helpers it reuses unchanged.
//
// The path draws exactly what rt_render draws; at every diffuse event (LAMBERTIAN, or METAL's hemisphere branch) whose next query is
// still inside max_depth, one light sample is taken from a second RNG stream: an emitter sphere from the handle's table (cdf, by
// bisection), a direction uniform in the cone the sphere subtends, and a shadow ray through the same walk.  The BSDF ray that leaves
// the same vertex has its hit on a table sphere weighted by the power heuristic (or by 0: light sampling alone).  Every expression is
// the header's, in its order (the project's float rules: nothing fused, correctly rounded division and sqrt).
#pragma once

namespace rtk {

constexpr uint32_t kNeeStreamKey = RT_NEE_STREAM_KEY;       // nee = wang_hash(sample_seed ^ key)
constexpr float kNeeTwoPi = RT_NEE_TWO_PI;
constexpr float kNeePb = RT_NEE_PB;                          // density of the uniform-hemisphere direction, 1 / (2 pi)
constexpr int kNeeBlock = 256;
constexpr uint32_t kNeeChunk = 128u;                         // work indices a wave reserves per atomic
constexpr int kNeeShadeLanes = 32;                           // a wave shades once this many lanes are ready (or none is walking)

// The emitter table of a handle (global memory, sphere order): sphere index, cdf (last entry 1), pmf
struct NeeTable {
    const int32_t *index;
    const float *cdf;
    const float *pmf;
    int32_t count;
    int32_t mis;          // 1: power heuristic, 0: light sampling alone
};

// smallest e with u < cdf[e]; count when there is none (u == 1.0f)
__device__ __forceinline__ int32_t nee_pick(const NeeTable &T, float u) {
    int32_t lo = 0, hi = T.count;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (u < T.cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// the table entry of a sphere, -1 when it is not an emitter of the table (the index column is increasing)
__device__ __forceinline__ int32_t nee_find(const NeeTable &T, int32_t sphere) {
    int32_t lo = 0, hi = T.count;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (T.index[mid] < sphere) lo = mid + 1;
        else hi = mid;
    }
    return (lo < T.count && T.index[lo] == sphere) ? lo : -1;
}
// step 2 of the header: the cone of sphere s seen from x.  false: no contribution (x inside or on the sphere, or a cone too narrow
// for float); else w = c - x, d2 = dot(w, w), om = 1 - cos_max
__device__ __forceinline__ bool nee_cone(f3 x, float4 s, f3 &w, float &d2, float &om) {
    w = sub(mk(s.x, s.y, s.z), x);
    d2 = dot(w, w);
    const float rr = s.w * s.w;
    if (!(d2 > rr)) return false;
    const float cos_max = sqrt_cr(1.0f - rr / d2);
    om = 1.0f - cos_max;
    return om > 0.0f;
}
__device__ __forceinline__ float nee_pdf_cone(float om) { return 1.0f / (kNeeTwoPi * om); }

// A light sample a diffuse vertex asks for: the shadow ray (o, d), the code of the sphere it has to reach (2e) and what it adds then
struct NeeReq {
    f3 o, d, c;
    int32_t code;         // -1: no light sample
};

// The light sample of a diffuse vertex at x (face-forwarded normal n, albedo a, throughput beta before the attenuation)
__device__ __forceinline__ void nee_sample(const KParams &P, const NeeTable &T, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, NeeReq &req) {
    const float u = random_float(nee);
    const int32_t e = nee_pick(T, u);
    if (e >= T.count) return;
    const int32_t sphere = T.index[e];
    f3 w;
    float d2, om;
    if (!nee_cone(x, P.spheres[sphere], w, d2, om)) return;
    const float u1 = random_float(nee);
    const float cos_t = 1.0f - u1 * om;
    const float sin_t = sqrt_cr(fmaxf(0.0f, 1.0f - cos_t * cos_t));
    float px, py, q2;
    do {                  // a point of the unit disc by rejection, x first (the lens's draw), without the centre
        px = random_pm1(nee);
        py = random_pm1(nee);
        q2 = px * px + py * py;
    } while (q2 >= 1.0f || q2 == 0.0f);
    const float q = sqrt_cr(q2);
    const float cx = px / q, cy = py / q;
    const float len = sqrt_cr(d2);
    const f3 wn = mk(w.x / len, w.y / len, w.z / len);
    // Duff et al. 2017: an orthonormal basis (t1, t2) around wn
    const float sgn = copysignf(1.0f, wn.z);
    const float ba = -1.0f / (sgn + wn.z);
    const float bb = (wn.x * wn.y) * ba;
    const f3 t1 = mk(1.0f + ((sgn * wn.x) * wn.x) * ba, sgn * bb, -sgn * wn.x);
    const f3 t2 = mk(bb, sgn + (wn.y * wn.y) * ba, -wn.y);
    const float sx = sin_t * cx, sy = sin_t * cy;
    const f3 dir = mk((t1.x * sx + t2.x * sy) + wn.x * cos_t, (t1.y * sx + t2.y * sy) + wn.y * cos_t, (t1.z * sx + t2.z * sy) + wn.z * cos_t);
    if (!(dot(dir, n) > 0.0f)) return;
    const float pl = T.pmf[e] * nee_pdf_cone(om);
    const float f = T.mis ? (kNeePb * pl) / (pl * pl + kNeePb * kNeePb) : kNeePb / pl;
    const float4 ME = P.materials[3 * P.sphere_mat[sphere] + 1];
    req.o = x;
    req.d = dir;
    req.c = scale(f, mul(mul(beta, a), mk(ME.x, ME.y, ME.z)));
    req.code = 2 * sphere;
}

// shade() of the exact walk (kGuard = false, the global material table, the general build) with next-event estimation:
//   prev_diffuse: the ray that found this hit left a diffuse event at its origin L.o — a hit on a table sphere has its emission
//   weighted; diffuse_out: this vertex is a diffuse event (the next ray's prev_diffuse); req: the light sample it takes.
// The main stream's draws, the branches, the roulette and the next ray are shade()'s.
__device__ __forceinline__ bool shade_nee(Lane &L, const KParams &P, const NeeTable &T, bool prev_diffuse, uint32_t &nee, f3 &out_o, f3 &out_d,
                                          NeeReq &req, bool &diffuse_out) {
    req.code = -1;
    diffuse_out = false;
    if (L.hit < 0) {
        L.color = add(L.color, mul(L.beta, mk(P.bg[0], P.bg[1], P.bg[2])));
        return false;
    }
    const int32_t code = L.hit;
    const int32_t idx = code >> 1;
    const float t = L.closest;
    const f3 point = add(L.o, scale(t, L.d));        // r.at(rec.t)
    f3 normal;
    bool front;
    int32_t mat_idx;
    float tu = 0.0f, tv = 0.0f;
    const bool is_plane = (code & 1) != 0;
    f3 outward = mk(0, 0, 0);
    if (is_plane) {
        const float4 P0 = P.planes[5 * idx + 0];
        const float4 P2 = P.planes[5 * idx + 2];
        outward = mk(P0.x, P0.y, P0.z);
        mat_idx = as_int(P2.w);
    } else {
        const float4 s = P.spheres[idx];
        outward = divs(sub(point, mk(s.x, s.y, s.z)), s.w);
        mat_idx = P.sphere_mat[idx];
    }
    front = dot(L.d, outward) < 0;
    normal = front ? outward : neg(outward);

    const float4 MA = P.materials[3 * mat_idx + 0];
    const float4 ME = P.materials[3 * mat_idx + 1];
    const int32_t type = as_int(MA.w) & 3;
    const int32_t tex_id = as_int(MA.w) >> 2;
    f3 albedo = mk(MA.x, MA.y, MA.z);
    if (tex_id != 0) {
        if (is_plane) {
            const float4 P1 = P.planes[5 * idx + 1];
            const float4 P2 = P.planes[5 * idx + 2];
            const float4 P3 = P.planes[5 * idx + 3];
            const float4 P4 = P.planes[5 * idx + 4];
            const f3 ph = sub(point, mk(P4.x, P4.y, P4.z));
            const f3 w = mk(P1.x, P1.y, P1.z);
            tu = dot(w, cross(ph, mk(P3.x, P3.y, P3.z)));
            tv = dot(w, cross(mk(P2.x, P2.y, P2.z), ph));
        } else {
            const float theta = acos_libm(outward.y);
            const float phi = (float)((double)atan2_libm(-outward.z, outward.x) + 3.14159265358979323846);
            tu = (float)((double)phi / (2 * 3.14159265358979323846));
            tv = (float)((double)theta / 3.14159265358979323846);
        }
        albedo = mul(albedo, sample_texture(P, tex_id - 1, tu, tv));
    }
    const f3 beta_in = L.beta;
    // final_color += beta * emitted, weighted when a BSDF ray from a diffuse event found a table sphere
    f3 emitted = mul(beta_in, mk(ME.x, ME.y, ME.z));
    if (prev_diffuse && !is_plane) {
        const int32_t e = nee_find(T, idx);
        if (e >= 0) {
            f3 w;
            float d2, om, pl = 0.0f;
            if (nee_cone(L.o, P.spheres[idx], w, d2, om)) pl = T.pmf[e] * nee_pdf_cone(om);
            const float wb = T.mis ? (kNeePb * kNeePb) / (kNeePb * kNeePb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
            emitted = scale(wb, emitted);
        }
    }

    f3 new_o = point, new_d = normal, att = albedo;
    const bool is_lamb = type == RT_MAT_LAMBERTIAN;
    const bool is_metal = type == RT_MAT_METAL;
    const bool is_glass = type == RT_MAT_DIELECTRIC;
    if (!(is_lamb || is_metal || is_glass)) {                        // DIFFUSE_LIGHT
        L.color = add(L.color, emitted);
        return false;
    }
    float4 MB = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if (is_glass) MB = P.materials[3 * mat_idx + 2];
    bool metal_reflect = false;
    if (is_metal) metal_reflect = random_float(L.seed) < 0.8f;
    f3 in_sphere = mk(0, 0, 0);
    if (is_lamb || is_metal) in_sphere = random_in_unit_sphere(L.seed);
    L.color = add(L.color, emitted);
    f3 ud = mk(0, 0, 0);
    if (metal_reflect || is_glass) ud = unit(L.d);
    if (is_glass) {
        const float ir = MB.w;
        const float ratio = front ? ME.w : ir;
        const float cos_theta = fminf(dot(neg(ud), normal), 1.0f);
        const float sin_theta = sqrt_cr(1.0f - cos_theta * cos_theta);
        const bool cannot_refract = ratio * sin_theta > 1.0f;
        bool do_reflect = cannot_refract;
        if (!cannot_refract) {
            const float rnd = random_float(L.seed);
            do_reflect = schlick_exceeds(cos_theta, front ? MA.x : MA.y, rnd);
        }
        new_d = do_reflect ? reflect(ud, normal) : refract(ud, normal, ratio);
        att = mk(1.0f, 1.0f, 1.0f);
        if (!front) {
            const float dist = sqrt_cr(lensq(sub(point, L.o)));
            const f3 tr = mk(MB.x == 0.0f ? 1.0f : exp_libm(-MB.x * dist), MB.y == 0.0f ? 1.0f : exp_libm(-MB.y * dist),
                             MB.z == 0.0f ? 1.0f : exp_libm(-MB.z * dist));
            att = mul(att, tr);
        }
        const float p = fmaxf(att.x, fmaxf(att.y, att.z));
        if (random_float(L.seed) > p) return false;                  // Russian roulette
        if (p != 1.0f) att = scale(recip(p), att);
        const float side = dot(new_d, normal) > 0 ? 1.0f : -1.0f;
        new_o = add(point, scale(side, scale(1e-4f, normal)));
    } else if (metal_reflect) {
        new_d = add(reflect(ud, normal), scale(ME.w, in_sphere));
        if (!(dot(new_d, normal) > 0)) return false;
    } else {                                                         // LAMBERTIAN and METAL's 20 % branch: a diffuse event
        new_d = scatter_diffuse_dir(in_sphere, normal);
        diffuse_out = true;
        if (L.depth + 1 < P.max_depth && T.count > 0) nee_sample(P, T, nee, point, normal, albedo, beta_in, req);
    }
    L.beta = mul(L.beta, att);
    L.depth++;
    if (L.depth >= P.max_depth) return false;
    out_o = new_o;
    out_d = new_d;
    return true;
}

// the closest hit of the lane's armed ray, reference order, through L1 / L2
__device__ __forceinline__ void nee_walk(Lane &L, const KParams &P) {
    while (!traversal_finished<true>(L, kBlocked)) {
        if (L.sp != 0) leaf_threaded(L, P.spheres, P.planes);
        else step_threaded(L, P.tnodes, P.num_tnodes);
    }
}

// the per-sample RNG states: the path's (after the camera's first hash, as start_sample takes it) and the light samples'
__device__ __forceinline__ uint32_t nee_seed_of(uint32_t base_seed, int32_t s) { return wang_hash(wang_hash(base_seed + (uint32_t)s) ^ kNeeStreamKey); }

// ---- probe (rt_trace_samples_nee): one lane traces one (i, j, s) sample -------------------------------------------------------------
__global__ void __launch_bounds__(256) nee_probe_kernel(const KParams P, const NeeTable T, uint32_t *nee_seed_out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    uint32_t nee = nee_seed_of(base_seed, s);
    f3 ray_o, ray_d;
    start_sample(L, P, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0;
    bool prev_diffuse = false;
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            nee_walk(L, P);
            NeeReq req;
            bool diffuse;
            const bool more = shade_nee(L, P, T, prev_diffuse, nee, ray_o, ray_d, req, diffuse);
            if (req.code >= 0) {
                rays++;
                begin_ray(L, req.o, req.d, 0);
                nee_walk(L, P);
                if (L.hit == req.code) L.color = add(L.color, req.c);
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
}

// ---- the trace kernel of rt_render_nee: one pass of samples into the slab -----------------------------------------------------------
// Persistent waves fetch work indices kNeeChunk at a time (one atomic per wave) and hand them to lanes as they free up.  Each lane
// is a small state machine — walking its path ray, walking a shadow ray, or idle — and the wave either takes up to four walk steps for
// the lanes that walk or, once kNeeShadeLanes lanes (or all that are busy) have finished their walk, one shade step for those: the
// path's shade (shade_nee), or the shadow ray's verdict.
constexpr int32_t kNeeIdle = 0, kNeePath = 1, kNeeShadow = 2;
__global__ void __launch_bounds__(kNeeBlock) nee_render_kernel(const KParams P, const NeeTable T) {
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
    int32_t phase = kNeeIdle;
    uint32_t w = 0, nee = 0;
    bool prev_diffuse = false, next_more = false;
    f3 next_o = mk(0, 0, 0), next_d = mk(0, 0, 0), contrib = mk(0, 0, 0);
    int32_t target = -1;
    uint32_t pool_next = 0, pool_end = 0;        // (wave-uniform)
    bool exhausted = false;
    for (;;) {
        // ---- lanes without a sample take the next work indices of the wave's pool (refilled with one atomic)
        const uint64_t idle = __ballot(phase == kNeeIdle);
        if (idle != 0 && !exhausted) {
            const uint32_t cnt = (uint32_t)__popcll(idle);
            const uint32_t rank = (uint32_t)lane_rank(idle);
            const uint32_t avail = pool_end - pool_next;
            uint32_t mine;
            if (avail < cnt) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(P.queue, kNeeChunk);
                base = __builtin_amdgcn_readfirstlane(base);
                mine = rank < avail ? pool_next + rank : base + (rank - avail);
                pool_next = base + (cnt - avail);
                pool_end = base + kNeeChunk;
                if (base >= P.total_work) exhausted = true;
            } else {
                mine = pool_next + rank;
                pool_next += cnt;
            }
            if (phase == kNeeIdle && mine < P.total_work) {
                w = mine;
                int32_t pi, pj;
                uint32_t k;
                map_work(P, w, pi, pj, k);
                const int32_t s = P.pass_first + (int32_t)k;
                const uint32_t base_seed = wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj);
                nee = nee_seed_of(base_seed, s);
                f3 o, d;
                start_sample(L, P, pi, pj, base_seed, s, o, d);
                begin_ray(L, o, d, 0);
                prev_diffuse = false;
                phase = kNeePath;
            }
        }
        const bool busy = phase != kNeeIdle;
        if (!__any(busy)) {
            if (exhausted) break;
            continue;
        }
        const bool walking = busy && !traversal_finished<true>(L, kBlocked);
        const bool ready = busy && !walking;
        const int n_walk = __popcll(__ballot(walking));
        const int n_ready = __popcll(__ballot(ready));
        if (n_walk == 0 || n_ready >= kNeeShadeLanes) {
            if (ready) {
                if (phase == kNeePath) {
                    NeeReq req;
                    bool diffuse;
                    const bool more = shade_nee(L, P, T, prev_diffuse, nee, next_o, next_d, req, diffuse);
                    prev_diffuse = diffuse;
                    if (req.code >= 0) {
                        target = req.code;
                        contrib = req.c;
                        next_more = more;
                        begin_ray(L, req.o, req.d, 0);
                        phase = kNeeShadow;
                    } else if (more) {
                        begin_ray(L, next_o, next_d, 0);
                    } else {
                        store_sample(P, w, L.color);
                        phase = kNeeIdle;
                    }
                } else {
                    if (L.hit == target) L.color = add(L.color, contrib);
                    if (next_more) {
                        begin_ray(L, next_o, next_d, 0);
                        phase = kNeePath;
                    } else {
                        store_sample(P, w, L.color);
                        phase = kNeeIdle;
                    }
                }
                if (phase == kNeeIdle) {
                    L.node = kBlocked;
                    L.sp = 0;
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!traversal_finished<true>(L, kBlocked)) {
                    if (L.sp != 0) leaf_threaded(L, P.spheres, P.planes);
                    else step_threaded(L, P.tnodes, P.num_tnodes);
                }
            }
        }
    }
}

}  // namespace rtk
