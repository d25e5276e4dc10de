// rt_env.hip.inc — image-based lighting (rt_render_env; include/rtp_amd.h, rt_env_params; DESIGN.md §14).  Included by rt_capi.hip after
// rt_nee.hip.inc; the walk (step_threaded / leaf_threaded on the reference-order table) and rt_kernel.hip.inc's helpers are reused
// unchanged.
//
// The path draws exactly what rt_render draws; a ray that hits nothing looks its direction up in an octahedral map (nearest texel, no
// trigonometry) instead of adding the background.  At every diffuse event whose next query is still inside max_depth one light
// sample is taken from a second RNG stream: a row of the map by its marginal cdf, a texel of the row by the row's conditional cdf
// (both by bisection), a uniform point inside the texel, and a shadow ray — an occlusion query: it contributes when it hits nothing,
// so its walk stops at the first accepted hit.  The miss of the BSDF ray that leaves the same vertex is weighted by the power
// heuristic (or by 0: light sampling alone).  Every expression is the header's, in its order.
#pragma once

namespace rtk {

constexpr uint32_t kEnvStreamKey = RT_ENV_STREAM_KEY;       // env = wang_hash(sample_seed ^ key)
constexpr int kEnvBlock = 256;
constexpr uint32_t kEnvChunk = 128u;                         // work indices a wave reserves per atomic
constexpr int kEnvShadeLanes = 32;                           // a wave shades once this many lanes are ready (or none is walking)

// An environment as the kernels see it (global memory): per texel (r, g, b, pj = row pmf * conditional pmf), the row marginal's cdf
// and the rows' conditional cdfs (n each), and the call's parameters
struct EnvDev {
    const float4 *texels;
    const float *row_cdf;
    const float *col_cdf;
    int32_t n;
    int32_t sampled;      // 1: light samples are drawn and misses after a diffuse event weighted (mode != 0 and a table that is not empty)
    int32_t mis;          // 1: power heuristic, 0: light sampling alone
    int32_t camera_visible;
    float scale;
    float rot[9];
    float dens;           // ((float)n * (float)n) * 0.25f
    float h;              // 2.0f / (float)n
};

__device__ __forceinline__ float env_sg(float x) { return x >= 0.0f ? 1.0f : -1.0f; }
// (u, v) of the unit square → the point of the octahedron
__device__ __forceinline__ f3 env_decode(float u, float v) {
    const float y = (1.0f - fabsf(u)) - fabsf(v);
    if (y >= 0.0f) return mk(u, y, v);
    return mk((1.0f - fabsf(v)) * env_sg(u), y, (1.0f - fabsf(u)) * env_sg(v));
}
__device__ __forceinline__ int32_t env_cell(float u, int32_t n) {
    const float t = ((u + 1.0f) * 0.5f) * (float)n;
    return t >= 0.0f ? (t < (float)n ? (int32_t)t : n - 1) : 0;
}
// direction (environment frame) → its octahedron point p and its texel iy * n + ix
__device__ __forceinline__ int32_t env_texel(f3 d, int32_t n, f3 &p) {
    const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z);
    p = mk(d.x / s, d.y / s, d.z / s);
    float u = p.x, v = p.z;
    if (!(p.y >= 0.0f)) {
        u = (1.0f - fabsf(p.z)) * env_sg(p.x);
        v = (1.0f - fabsf(p.x)) * env_sg(p.z);
    }
    return env_cell(v, n) * n + env_cell(u, n);
}
__device__ __forceinline__ float env_pl(const EnvDev &E, float pj, float q2, float q) { return (pj * E.dens) * (q2 * q); }
__device__ __forceinline__ f3 env_rotate(const EnvDev &E, f3 d) {
    return mk(dot(mk(E.rot[0], E.rot[1], E.rot[2]), d), dot(mk(E.rot[3], E.rot[4], E.rot[5]), d), dot(mk(E.rot[6], E.rot[7], E.rot[8]), d));
}
// smallest e in [0, n) with u < cdf[e]; n when there is none
__device__ __forceinline__ int32_t env_pick(const float *cdf, int32_t n, float u) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// what a ray of direction d and throughput beta that hits nothing adds: beta * sE(d), weighted when the ray left a diffuse event
__device__ __forceinline__ f3 env_miss(const EnvDev &E, f3 d, f3 beta, bool prev_diffuse) {
    f3 p;
    const int32_t t = env_texel(env_rotate(E, d), E.n, p);
    const float4 T = E.texels[t];
    f3 term = mul(beta, mk(E.scale * T.x, E.scale * T.y, E.scale * T.z));
    if (prev_diffuse && E.sampled) {
        const float q2 = dot(p, p);
        const float pl = env_pl(E, T.w, q2, sqrt_cr(q2));
        const float wb = E.mis ? (kNeePb * kNeePb) / (kNeePb * kNeePb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
        term = scale(wb, term);
    }
    return term;
}

// The light sample of a diffuse vertex with face-forwarded normal n, albedo a and throughput beta (before the attenuation): false =
// no contribution; else the shadow ray's direction and what it adds when it hits nothing
__device__ __forceinline__ bool env_sample(const EnvDev &E, uint32_t &env, f3 n, f3 a, f3 beta, f3 &dir, f3 &c) {
    const float ua = random_float(env);
    const int32_t iy = env_pick(E.row_cdf, E.n, ua);
    if (iy >= E.n) return false;
    const float ub = random_float(env);
    const int32_t ix = env_pick(E.col_cdf + (size_t)iy * (size_t)E.n, E.n, ub);
    if (ix >= E.n) return false;
    const float uc = random_float(env);
    const float ud = random_float(env);
    const float u = ((float)ix + uc) * E.h - 1.0f;
    const float v = ((float)iy + ud) * E.h - 1.0f;
    const f3 p = env_decode(u, v);
    const float q2 = dot(p, p);
    const float q = sqrt_cr(q2);
    const f3 we = mk(p.x / q, p.y / q, p.z / q);
    dir = mk((E.rot[0] * we.x + E.rot[3] * we.y) + E.rot[6] * we.z, (E.rot[1] * we.x + E.rot[4] * we.y) + E.rot[7] * we.z,
             (E.rot[2] * we.x + E.rot[5] * we.y) + E.rot[8] * we.z);
    if (!(dot(dir, n) > 0.0f)) return false;
    const float4 T = E.texels[(size_t)iy * (size_t)E.n + (size_t)ix];
    const float pl = env_pl(E, T.w, q2, q);
    const float f = E.mis ? (kNeePb * pl) / (pl * pl + kNeePb * kNeePb) : kNeePb / pl;
    c = scale(f, mul(mul(beta, a), mk(E.scale * T.x, E.scale * T.y, E.scale * T.z)));
    return true;
}

// shade() of the exact walk (kGuard = false, the global material table, the general build) lit by the environment:
//   prev_diffuse: the ray that found this hit (or nothing) left a diffuse event; diffuse_out: this vertex is one (the next ray's
//   prev_diffuse); sample: it takes a light sample — the shadow ray (out_o, sdir), which adds c when it hits nothing (a vertex that
//   samples always has a next ray: out_o is both rays' origin).
// The main stream's draws, the branches, the roulette and the next ray are shade()'s.
__device__ __forceinline__ bool shade_env(Lane &L, const KParams &P, const EnvDev &E, bool prev_diffuse, uint32_t &env, f3 &out_o, f3 &out_d,
                                          f3 &sdir, f3 &c, bool &sample, bool &diffuse_out) {
    sample = false;
    diffuse_out = false;
    if (L.hit < 0) {
        if (L.depth == 0 && !E.camera_visible) L.color = add(L.color, mul(L.beta, mk(P.bg[0], P.bg[1], P.bg[2])));
        else L.color = add(L.color, env_miss(E, L.d, L.beta, prev_diffuse));
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
    const f3 emitted = mul(beta_in, mk(ME.x, ME.y, ME.z));        // final_color += beta * emitted: found by the path alone

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
        if (L.depth + 1 < P.max_depth && E.sampled) sample = env_sample(E, env, normal, albedo, beta_in, sdir, c);
    }
    L.beta = mul(L.beta, att);
    L.depth++;
    if (L.depth >= P.max_depth) return false;
    out_o = new_o;
    out_d = new_d;
    return true;
}

// the closest hit of the lane's armed ray, reference order, through L1 / L2
__device__ __forceinline__ void env_walk(Lane &L, const KParams &P) {
    while (!traversal_finished<true>(L, kBlocked)) {
        if (L.sp != 0) leaf_threaded(L, P.spheres, P.planes);
        else step_threaded(L, P.tnodes, P.num_tnodes);
    }
}
// One step of an occlusion query: the answer "something is hit in (0.001, 1e30)" does not depend on the visit order, and up to the
// first accepted hit the walk is the closest-hit search's own (closest is still 1e30) — so the walk ends there
__device__ __forceinline__ void env_occlusion_step(Lane &L, const KParams &P) {
    if (L.sp != 0) {
        leaf_threaded(L, P.spheres, P.planes);
        if (L.hit >= 0) L.node = kBlocked;
    } else {
        step_threaded(L, P.tnodes, P.num_tnodes);
    }
}

// the light samples' RNG state of a sample
__device__ __forceinline__ uint32_t env_seed_of(uint32_t base_seed, int32_t s) { return wang_hash(wang_hash(base_seed + (uint32_t)s) ^ kEnvStreamKey); }

// ---- probes --------------------------------------------------------------------------------------------------------------------------
// rt_env_lookup: one lane looks one direction up (no rotation)
__global__ void __launch_bounds__(256) env_lookup_kernel(const EnvDev E, int32_t count, const float *dirs, int32_t *texel, float *rad, float *pl) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    f3 p;
    const int32_t t = env_texel(mk(dirs[3 * g], dirs[3 * g + 1], dirs[3 * g + 2]), E.n, p);
    const float4 T = E.texels[t];
    const float q2 = dot(p, p);
    texel[g] = t;
    rad[3 * g] = T.x; rad[3 * g + 1] = T.y; rad[3 * g + 2] = T.z;
    pl[g] = env_pl(E, T.w, q2, sqrt_cr(q2));
}

// rt_trace_samples_env: one lane traces one (i, j, s) sample
__global__ void __launch_bounds__(256) env_probe_kernel(const KParams P, const EnvDev E, uint32_t *env_seed_out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    uint32_t env = env_seed_of(base_seed, s);
    f3 ray_o, ray_d;
    start_sample(L, P, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0;
    bool prev_diffuse = false;
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            env_walk(L, P);
            f3 sdir, c;
            bool sample, diffuse;
            const bool more = shade_env(L, P, E, prev_diffuse, env, ray_o, ray_d, sdir, c, sample, diffuse);
            if (sample) {
                rays++;
                begin_ray(L, ray_o, sdir, 0);
                while (!traversal_finished<true>(L, kBlocked)) env_occlusion_step(L, P);
                if (L.hit < 0) L.color = add(L.color, c);
            }
            if (!more) break;
            prev_diffuse = diffuse;
            begin_ray(L, ray_o, ray_d, 0);
        }
    }
    P.probe_rad[3 * g] = L.color.x; P.probe_rad[3 * g + 1] = L.color.y; P.probe_rad[3 * g + 2] = L.color.z;
    P.probe_rays[g] = rays;
    P.probe_seed[g] = L.seed;
    env_seed_out[g] = env;
}

// ---- the trace kernel of rt_render_env: one pass of samples into the slab -----------------------------------------------------------
// nee_render_kernel's shape: persistent waves fetch work indices kEnvChunk at a time (one atomic per wave) and hand them to lanes as
// they free up; a lane walks its path ray, walks a shadow ray, or is idle, and the wave either takes up to four walk steps for the
// lanes that walk or, once kEnvShadeLanes lanes (or all that are busy) have finished their walk, one shade step for those.
// Across a shadow walk a lane holds the next ray's direction and the pending contribution (six registers): the next ray's origin is
// the shadow ray's own (L.o), and a vertex that samples always has a next ray, so no flag for it either.
constexpr int32_t kEnvIdle = 0, kEnvPath = 1, kEnvShadow = 2;
__global__ void __launch_bounds__(kEnvBlock) env_render_kernel(const KParams P, const EnvDev E) {
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
    int32_t phase = kEnvIdle;
    uint32_t w = 0, env = 0;
    bool prev_diffuse = false;
    f3 next_d = mk(0, 0, 0), contrib = mk(0, 0, 0);
    uint32_t pool_next = 0, pool_end = 0;        // (wave-uniform)
    bool exhausted = false;
    for (;;) {
        // ---- lanes without a sample take the next work indices of the wave's pool (refilled with one atomic)
        const uint64_t idle = __ballot(phase == kEnvIdle);
        if (idle != 0 && !exhausted) {
            const uint32_t cnt = (uint32_t)__popcll(idle);
            const uint32_t rank = (uint32_t)lane_rank(idle);
            const uint32_t avail = pool_end - pool_next;
            uint32_t mine;
            if (avail < cnt) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(P.queue, kEnvChunk);
                base = __builtin_amdgcn_readfirstlane(base);
                mine = rank < avail ? pool_next + rank : base + (rank - avail);
                pool_next = base + (cnt - avail);
                pool_end = base + kEnvChunk;
                if (base >= P.total_work) exhausted = true;
            } else {
                mine = pool_next + rank;
                pool_next += cnt;
            }
            if (phase == kEnvIdle && mine < P.total_work) {
                w = mine;
                int32_t pi, pj;
                uint32_t k;
                map_work(P, w, pi, pj, k);
                const int32_t s = P.pass_first + (int32_t)k;
                const uint32_t base_seed = wang_hash((uint32_t)pi * (uint32_t)P.width + (uint32_t)pj);
                env = env_seed_of(base_seed, s);
                f3 o, d;
                start_sample(L, P, pi, pj, base_seed, s, o, d);
                begin_ray(L, o, d, 0);
                prev_diffuse = false;
                phase = kEnvPath;
            }
        }
        const bool busy = phase != kEnvIdle;
        if (!__any(busy)) {
            if (exhausted) break;
            continue;
        }
        const bool walking = busy && !traversal_finished<true>(L, kBlocked);
        const bool ready = busy && !walking;
        const int n_walk = __popcll(__ballot(walking));
        const int n_ready = __popcll(__ballot(ready));
        if (n_walk == 0 || n_ready >= kEnvShadeLanes) {
            if (ready) {
                if (phase == kEnvPath) {
                    f3 next_o, sdir;
                    bool sample, diffuse;
                    const bool more = shade_env(L, P, E, prev_diffuse, env, next_o, next_d, sdir, contrib, sample, diffuse);
                    prev_diffuse = diffuse;
                    if (sample) {
                        begin_ray(L, next_o, sdir, 0);
                        phase = kEnvShadow;
                    } else if (more) {
                        begin_ray(L, next_o, next_d, 0);
                    } else {
                        store_sample(P, w, L.color);
                        phase = kEnvIdle;
                    }
                } else {
                    if (L.hit < 0) L.color = add(L.color, contrib);
                    begin_ray(L, L.o, next_d, 0);
                    phase = kEnvPath;
                }
                if (phase == kEnvIdle) {
                    L.node = kBlocked;
                    L.sp = 0;
                }
            }
        } else {
            const bool shadow = phase == kEnvShadow;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!traversal_finished<true>(L, kBlocked)) {
                    if (L.sp != 0) {
                        leaf_threaded(L, P.spheres, P.planes);
                        if (shadow && L.hit >= 0) L.node = kBlocked;
                    } else {
                        step_threaded(L, P.tnodes, P.num_tnodes);
                    }
                }
            }
        }
    }
}

}  // namespace rtk
