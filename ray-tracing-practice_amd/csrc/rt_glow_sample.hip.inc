// rt_glow_sample.hip.inc — light samples of a glowing medium on the lit path (rt_render_glow_sampled; include/rtp_amd.h, "light samples
// of the glow"; DESIGN.md §36).  Included by rt_capi.hip after rt_glow.hip.inc, whose light (GlowLit over a grid) and free flight
// (glow_flight) it uses as they are, with rt_medium.hip.inc's interval and medium vertex, rt_env.hip.inc's pick (env_pick) and
// rt_light.hip.inc's vertex text (RTP_LIT_VERTEX) and pool fetch (RTP_LIT_POOL_FETCH).
//
// What is new here: a third light sample at every sampling vertex — a cell of the grid by its emission, a uniform point in it, the
// direction to that point — whose density in solid angle is a sum over the cells of the whole line (glow_pl); the emission the medium
// sends along a ray to its closest hit (glow_line), which a third shadow phase adds at its verdict; and the weight of the track-length add
// of a path ray that left such a vertex.  The wave loop and the probe are this file's own: the shared ones know two shadow phases, and
// their text cannot change without moving the listings of the kernels that run on them (DESIGN.md §36).  Every expression is the
// header's, in its order.
#pragma once

namespace rtk {

// The sampler's table (rt_glow_sampler, global memory): the slabs' cdf (nz), every slab's rows' (nz * ny), every row's cells' (nz * ny * nx),
// the probability of every cell, and the call's switch
struct GlowSamplerDev {
    const float *slab_cdf, *row_cdf, *cell_cdf, *pc;
    int32_t mis;          // 1: power heuristic, 0: light sampling alone
};
template <class Table>
struct GlowSampleLit {
    GlowLit<VolumeLit<Table>> G;
    GlowSamplerDev Q;
};
// (the light and the stream that the pool fetch starts a sample with: rt_light.hip.inc, "what fog adds to a lit light")
template <class Table> __device__ __forceinline__ const GlossLit<Table> &fog_lit(const GlowSampleLit<Table> &T) { return T.G.B.G; }
template <class Table> __device__ __forceinline__ uint32_t fog_seed(const GlowSampleLit<Table> &, uint32_t base_seed, int32_t s) { return medium_seed_of(base_seed, s); }

// "density grid"'s walk over the non-empty interval [t0, t1] of the ray (o, d), cell for cell (volume_walk's cells, bounds and order),
// with what a cell does left to the caller: cell(at, ta, tb), at the cell's place in the grid, [ta, tb] the ray's stretch in it
template <class F>
__device__ __forceinline__ void volume_cells(const MediumDev &M, const VolumeDev &V, f3 o, f3 d, float t0, float t1, int32_t &cells, F &&cell) {
    const float wx = (M.b[0] - M.a[0]) / (float)V.nx, wy = (M.b[1] - M.a[1]) / (float)V.ny, wz = (M.b[2] - M.a[2]) / (float)V.nz;
    int32_t cx = volume_entry(M.a[0], wx, V.nx, o.x + t0 * d.x);
    int32_t cy = volume_entry(M.a[1], wy, V.ny, o.y + t0 * d.y);
    int32_t cz = volume_entry(M.a[2], wz, V.nz, o.z + t0 * d.z);
    float tx = volume_tnext(M.a[0], M.b[0], wx, V.nx, cx, o.x, d.x);
    float ty = volume_tnext(M.a[1], M.b[1], wy, V.ny, cy, o.y, d.y);
    float tz = volume_tnext(M.a[2], M.b[2], wz, V.nz, cz, o.z, d.z);
    float ta = t0;
    for (int32_t left = V.nx + V.ny + V.nz; left > 0; --left) {
        float tm = tx;
        int32_t axis = 0;
        if (ty < tm) {
            tm = ty;
            axis = 1;
        }
        if (tz < tm) {
            tm = tz;
            axis = 2;
        }
        float tb = tm < t1 ? tm : t1;
        if (tb < ta) tb = ta;
        cells++;
        cell(((size_t)cz * (size_t)V.ny + (size_t)cy) * (size_t)V.nx + (size_t)cx, ta, tb);
        if (tb >= t1) break;
        if (axis == 0) {
            cx += d.x > 0.0f ? 1 : -1;
            if (cx < 0 || cx >= V.nx) break;
            tx = volume_tnext(M.a[0], M.b[0], wx, V.nx, cx, o.x, d.x);
        } else if (axis == 1) {
            cy += d.y > 0.0f ? 1 : -1;
            if (cy < 0 || cy >= V.ny) break;
            ty = volume_tnext(M.a[1], M.b[1], wy, V.ny, cy, o.y, d.y);
        } else {
            cz += d.z > 0.0f ? 1 : -1;
            if (cz < 0 || cz >= V.nz) break;
            tz = volume_tnext(M.a[2], M.b[2], wz, V.nz, cz, o.z, d.z);
        }
        ta = tb;
    }
}

// glow_pl(o, d) of the header: the density in solid angle with which the light sample of a vertex at o chooses the direction d
__device__ __forceinline__ float glow_pl(const MediumDev &M, const VolumeDev &V, const float *pc, f3 o, f3 d, int32_t &cells) {
    float t0, t1;
    if (!medium_interval(M, o, d, INFINITY, t0, t1)) return 0.0f;
    const float len = sqrt_cr(lensq(d));
    float q = 0.0f;
    volume_cells(M, V, o, d, t0, t1, cells, [&](size_t at, float ta, float tb) {
        const float seg = (tb - ta) * len;
        const float ra = ta * len, rb = tb * len;
        q = q + pc[at] * (seg * ((rb * rb + rb * ra) + ra * ra));
    });
    const float wx = (M.b[0] - M.a[0]) / (float)V.nx, wy = (M.b[1] - M.a[1]) / (float)V.ny, wz = (M.b[2] - M.a[2]) / (float)V.nz;
    const float inv3v = 1.0f / (3.0f * ((wx * wy) * wz));
    return q * inv3v;
}

// glow_line(o, d, t_end) of the header: what the medium emits along the ray towards o, per unit radiance.  false: an empty interval
__device__ __forceinline__ bool glow_line(const MediumDev &M, const VolumeDev &V, const float *heat, f3 o, f3 d, float t_end, float &G, int32_t &cells) {
    float t0, t1;
    G = 0.0f;
    if (!medium_interval(M, o, d, t_end, t0, t1)) return false;
    const float len = sqrt_cr(lensq(d));
    float Tr = 1.0f;
    volume_cells(M, V, o, d, t0, t1, cells, [&](size_t at, float ta, float tb) {
        const float seg = (tb - ta) * len;
        const float sigma_c = M.sigma_t * V.rho[at];
        const float h_c = heat ? heat[at] : 1.0f;
        const float x = sigma_c * seg;
        const float e = exp_libm(-x);
        const float m = x < 0.0625f ? seg * (1.0f - x * (0.5f - x * (1.0f / 6.0f - x * (1.0f / 24.0f)))) : (1.0f - e) / sigma_c;
        G = G + Tr * (h_c * m);
        Tr = Tr * e;
    });
    return true;
}

// A light sample of the glow that waits for its shadow ray: the direction (not unit: the vector to the sampled point), the factor f and
// the throughput the vertex arrived with times its albedo
struct GlowShot {
    f3 dir, ba;
    float f;
};
// The light sample of a vertex at x (face-forwarded normal n where PB has a hemisphere, albedo a, throughput beta before the attenuation),
// six draws of med.  false: none
template <class Table, class Pb>
__device__ __forceinline__ bool glow_sample(const GlowSampleLit<Table> &T, uint32_t &med, f3 x, f3 n, f3 a, f3 beta, Pb PB, GlowShot &Q, int32_t &cells) {
    const MediumDev &M = T.G.B.M;
    const VolumeDev &V = T.G.B.V;
    const float us = random_float(med);
    const float ur = random_float(med);
    const float uc = random_float(med);
    const float ux = random_float(med);
    const float uy = random_float(med);
    const float uz = random_float(med);
    const int32_t z = env_pick(T.Q.slab_cdf, V.nz, us);
    if (z >= V.nz) return false;
    const int32_t y = env_pick(T.Q.row_cdf + (size_t)z * (size_t)V.ny, V.ny, ur);
    if (y >= V.ny) return false;
    const int32_t c = env_pick(T.Q.cell_cdf + ((size_t)z * (size_t)V.ny + (size_t)y) * (size_t)V.nx, V.nx, uc);
    if (c >= V.nx) return false;
    const float wx = (M.b[0] - M.a[0]) / (float)V.nx, wy = (M.b[1] - M.a[1]) / (float)V.ny, wz = (M.b[2] - M.a[2]) / (float)V.nz;
    const f3 p = mk(M.a[0] + ((float)c + ux) * wx, M.a[1] + ((float)y + uy) * wy, M.a[2] + ((float)z + uz) * wz);
    const f3 dir = sub(p, x);
    const float d2 = lensq(dir);
    if (d2 == 0.0f) return false;
    if (kPbHemisphere<Pb> && !(dot(dir, n) > 0.0f)) return false;
    const float l = sqrt_cr(d2);
    const float pb = PB(mk(dir.x / l, dir.y / l, dir.z / l));
    if (Pb::kGlossy && pb == 0.0f) return false;
    const float pl = glow_pl(M, V, T.Q.pc, x, dir, cells);
    if (!(pl > 0.0f)) return false;
    Q.f = T.Q.mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    Q.dir = dir;
    Q.ba = mul(beta, a);
    return true;
}
// the verdict of its shadow ray, a finished closest-hit walk of the lane
template <class Table>
__device__ __forceinline__ void glow_verdict(Lane &L, const GlowSampleLit<Table> &T, const GlowShot &Q, int32_t &cells) {
    float G;
    if (!glow_line(T.G.B.M, T.G.B.V, T.G.heat, L.o, L.d, L.hit < 0 ? INFINITY : L.closest, G, cells)) return;
    L.color = add(L.color, mk(Q.ba.x * (Q.f * (T.G.r0 * G)), Q.ba.y * (Q.f * (T.G.r1 * G)), Q.ba.z * (Q.f * (T.G.r2 * G))));
}

// glow_vertex (rt_glow.hip.inc) for a path ray that carries prev: the track-length add weighted against the light sample of the vertex
// the ray left, and after a medium vertex that goes on its own light sample (shot), drawn behind the next direction's draws
template <class Table>
__device__ __forceinline__ bool glow_sampled_vertex(Lane &L, const KParams &P, const GlowSampleLit<Table> &T, float prev, uint32_t &nee, uint32_t &env,
                                                    uint32_t &med, f3 &out_o, f3 &out_d, LitSamples &S, GlowShot &Q, bool &shot, float &carry_out, bool &more,
                                                    FogCount &n, float &length) {
    const MediumDev &M = T.G.B.M;
    shot = false;
    float t0, t1;
    if (!medium_interval(M, L.o, L.d, L.hit < 0 ? INFINITY : L.closest, t0, t1)) return false;
    const float len = sqrt_cr(lensq(L.d));
    const float u = random_float(med);
    float t, E;
    const bool event = glow_flight(T.G, L.o, L.d, t0, t1, len, u, t, E, n);
    length = length + E;
    f3 term = mk(L.beta.x * (T.G.r0 * E), L.beta.y * (T.G.r1 * E), L.beta.z * (T.G.r2 * E));
    const float pb = lit_carry(prev, T.G.B.G.gn);
    if (pb != 0.0f) {
        const float pl = glow_pl(M, T.G.B.V, T.Q.pc, L.o, L.d, n.cells);
        const float wb = T.Q.mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
        term = scale(wb, term);
    }
    L.color = add(L.color, term);
    if (!event) return false;
    const f3 x = add(L.o, scale(t, L.d));
    const f3 beta_in = L.beta;
    medium_vertex_at(L, P, T.G.B.G, M, nee, env, med, x, out_o, out_d, S, carry_out, more, n.events);
    if (more) {
        PbPhase ph;
        ph.ud = unit(L.d);
        ph.g = M.g;
        shot = glow_sample(T, med, x, ph.ud, mk(M.albedo[0], M.albedo[1], M.albedo[2]), beta_in, ph, Q, n.cells);
    }
    return true;
}

// shade_lit2 with the glow's sample behind the emitter's and the environment's: at a diffuse event, and at a glossy one under the
// emitters' glossy switch (T.gn) whether or not the table holds an emitter
template <class Table>
__device__ __forceinline__ bool shade_glow_lit(Lane &L, const KParams &P, const GlowSampleLit<Table> &TT, float prev_diffuse, uint32_t &nee, uint32_t &env,
                                               uint32_t &med, f3 &out_o, f3 &out_d, LitSamples &S, GlowShot &Q, bool &shot, float &diffuse_out, int32_t &cells) {
    const GlossLit<Table> &T = TT.G.B.G;
    S.a = false;
    S.b = false;
    shot = false;
    diffuse_out = 0.0f;
    RTP_LIT_VERTEX(if (L.depth + 1 < P.max_depth) {
        if (light_on(T.N)) S.a = light_sample(P, T.N, nee, point, normal, albedo, beta_in, PbDiffuse{}, S.adir, S.ac, S.code);
        if (env_sampled(T)) S.b = light_sample(P, T.E, env, point, normal, albedo, beta_in, PbDiffuse{}, S.bdir, S.bc, S.code);
        shot = glow_sample(TT, med, point, normal, albedo, beta_in, PbDiffuse{}, Q, cells);
    },
    if (ME.w >= kGlossMinFuzz && L.depth + 1 < P.max_depth) {
        const bool ga = T.gn && light_on(T.N);
        const bool gb = T.ge && env_sampled(T);
        const bool gg = T.gn != 0;
        if (ga || gb || gg) {
            if (!absorbed) diffuse_out = -gloss_pg(unit(new_d), refl, ME.w);
            const PbGlossy pbg = gloss_pb(refl, ME.w);
            if (ga) S.a = light_sample(P, T.N, nee, point, normal, albedo, beta_in, pbg, S.adir, S.ac, S.code);
            if (gb) S.b = light_sample(P, T.E, env, point, normal, albedo, beta_in, pbg, S.bdir, S.bc, S.code);
            if (gg) shot = glow_sample(TT, med, point, normal, albedo, beta_in, pbg, Q, cells);
            out_o = point;
        }
    })
}
#undef RTP_LIT_VERTEX

// ---- probe (rt_trace_samples_glow_sampled): lit_probe_body with the third shadow ray, the sum of the flights' E and the number of glow
// shadow rays
template <bool kLens, class Table>
__global__ void __launch_bounds__(256) glow_sample_probe_kernel(const KParams P, const GlowSampleLit<Table> T, const LensCam C, uint32_t *nee_seed_out,
                                                                uint32_t *env_seed_out, uint32_t *med_seed_out, int32_t *events_out, int32_t *cells_out,
                                                                float *length_out, int32_t *shots_out) {
    const GlossLit<Table> &G = T.G.B.G;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    uint32_t nee = light_seed_of(G.N, base_seed, s), env = light_seed_of(G.E, base_seed, s), med = medium_seed_of(base_seed, s);
    f3 ray_o, ray_d;
    lit_start<kLens>(L, P, C, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0, shots = 0;
    float length = 0.0f;
    FogCount n;
    float prev_diffuse = 0.0f;
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
            LitSamples S;
            S.code = -1;
            GlowShot Q;
            float diffuse;
            bool more, shot;
            if (!glow_sampled_vertex(L, P, T, prev_diffuse, nee, env, med, ray_o, ray_d, S, Q, shot, diffuse, more, n, length))
                more = shade_glow_lit(L, P, T, prev_diffuse, nee, env, med, ray_o, ray_d, S, Q, shot, diffuse, n.cells);
            if (S.a) {
                rays++;
                begin_ray(L, ray_o, S.adir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
                if (L.hit == S.code) L.color = add(L.color, fog_tr(T.G.B, L.o, L.d, L.closest, S.ac, n));
            }
            if (S.b) {
                rays++;
                begin_ray(L, ray_o, S.bdir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, true);
                if (L.hit < 0) L.color = add(L.color, fog_tr(T.G.B, L.o, L.d, INFINITY, S.bc, n));
            }
            if (shot) {
                rays++;
                shots++;
                begin_ray(L, ray_o, Q.dir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
                glow_verdict(L, T, Q, n.cells);
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
    med_seed_out[g] = med;
    events_out[g] = n.events;
    cells_out[g] = n.cells;
    length_out[g] = length;
    shots_out[g] = shots;
}

// ---- the trace kernel of rt_render_glow_sampled: lit_render_body's wave loop with a third shadow phase — path → emitter shadow → environment
// shadow (ends at its first hit) → glow shadow (a full closest-hit walk, like the emitter's) → path.  `pend` holds the shadow rays of the
// vertex that still wait (1 the emitter's, 2 the environment's, 4 the glow's); a vertex without a next ray zeroes next_d, and the last
// verdict ends the path (no_next_ray).  Across the walks a lane holds, beyond lit_render_body's, the glow sample's direction, f and
// throughput (seven registers) and pend.
constexpr int32_t kGlowShadow = 5;
// kList (rt_render_fog_adaptive's rounds; DESIGN.md §40) as in lit_render_body: the work indices are the first *P.work_count entries of
// P.work_list, a length read once per wave; an empty list leaves before the first atomic, and a fetched index stands for its list entry
// in map_work and in store_sample alike.
template <bool kLens, class Table, bool kList = false>
__device__ __forceinline__ void glow_sample_render_body(const KParams &P, const GlowSampleLit<Table> &T, const LensCam &C) {
    using Lit = GlossLit<Table>;
    [[maybe_unused]] uint32_t listed = 0u;          // (wave-uniform; kList only)
    if constexpr (kList) {
        listed = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)*P.work_count);
        if (listed > P.work_cap) listed = P.work_cap;          // (never more entries than the list has room for)
        if (listed == 0u) return;
    }
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
    int32_t phase = kLightIdle, pend = 0;
    uint32_t w = 0, nee = 0, env = 0, med = 0;
    float prev_diffuse = 0.0f;
    f3 next_d = mk(0, 0, 0);
    LitSamples S;
    S.adir = S.ac = S.bdir = S.bc = mk(0, 0, 0);
    S.code = -1;
    S.a = S.b = false;
    GlowShot Q;
    Q.dir = Q.ba = mk(0, 0, 0);
    Q.f = 0.0f;
    uint32_t pool_next = 0, pool_end = 0;  // (wave-uniform)
    bool exhausted = false;
    for (;;) {
        if constexpr (kList) {
            RTP_LIT_POOL_FETCH(listed, P.work_list[mine])
        } else {
            RTP_LIT_POOL_FETCH(P.total_work, mine)
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
                f3 o = L.o;          // (every shadow ray of a vertex and the next ray start where the first of them did)
                if (phase == kLightPath) {
                    float diffuse, length = 0.0f;
                    bool more, shot;
                    FogCount n;
                    if (!glow_sampled_vertex(L, P, T, prev_diffuse, nee, env, med, o, next_d, S, Q, shot, diffuse, more, n, length))
                        more = shade_glow_lit(L, P, T, prev_diffuse, nee, env, med, o, next_d, S, Q, shot, diffuse, n.cells);
                    prev_diffuse = diffuse;
                    if (!more) next_d = mk(0, 0, 0);
                    pend = (S.a ? 1 : 0) | (S.b ? 2 : 0) | (shot ? 4 : 0);
                } else if (phase == kLitShadowA) {
                    if (L.hit == S.code) L.color = add(L.color, fog_tr(T.G.B, L.o, L.d, L.closest, S.ac));
                } else if (phase == kLitShadowB) {
                    if (L.hit < 0) L.color = add(L.color, fog_tr(T.G.B, L.o, L.d, INFINITY, S.bc));
                } else {
                    int32_t cells = 0;
                    glow_verdict(L, T, Q, cells);
                }
                if (pend & 1) {
                    pend &= ~1;
                    begin_ray(L, o, S.adir, 0);
                    phase = kLitShadowA;
                } else if (pend & 2) {
                    pend &= ~2;
                    begin_ray(L, o, S.bdir, 0);
                    phase = kLitShadowB;
                } else if (pend & 4) {
                    pend = 0;
                    begin_ray(L, o, Q.dir, 0);
                    phase = kGlowShadow;
                } else if (no_next_ray(next_d)) {
                    store_sample(P, w, L.color);
                    phase = kLightIdle;
                    L.node = kBlocked;
                    L.sp = 0;
                } else {
                    begin_ray(L, o, next_d, 0);
                    phase = kLightPath;
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
}
#undef RTP_LIT_POOL_FETCH
#undef RTP_LIGHT_POOL_RESERVE

template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) glow_sample_render_kernel(const KParams P, const GlowSampleLit<Table> T, const LensCam C) {
    glow_sample_render_body<kLens>(P, T, C);
}
// the list variant: rt_render_fog_adaptive's rounds with light samples of the glow (DESIGN.md §40)
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) glow_sample_list_render_kernel(const KParams P, const GlowSampleLit<Table> T, const LensCam C) {
    glow_sample_render_body<kLens, Table, true>(P, T, C);
}
template <bool kLens, class Table> const void *lit_frame_kernel_of(const GlowSampleLit<Table> &) { return (const void *)glow_sample_render_kernel<kLens, Table>; }
template <bool kLens, class Table> const void *lit_list_kernel_of(const GlowSampleLit<Table> &) { return (const void *)glow_sample_list_render_kernel<kLens, Table>; }

}  // namespace rtk
