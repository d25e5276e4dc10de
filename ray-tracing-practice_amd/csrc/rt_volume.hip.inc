// rt_volume.hip.inc — heterogeneous fog from a density grid on the lit path (rt_render_volume; include/rtp_amd.h, "density grid";
// DESIGN.md §28).  Included by rt_capi.hip after rt_medium.hip.inc, whose interval (medium_interval), medium vertex (medium_vertex_at),
// phase function and stream it uses as they are, with rt_light.hip.inc's vertex, walk step, light samples and pool fetch.
//
// What is new here: the walk through the grid's cells along a ray's interval in the box (regular tracking: a 3-D DDA whose plane
// parameters are computed from the planes themselves, never accumulated), the free flight by inversion over that walk with ONE draw of med, and the
// optical depth of a shadow ray as the walk's sum.  The density is read from global memory, one dword per visited cell.  Every expression
// is the header's, in its order.
#pragma once

namespace rtk {

// The call's grid, by value beside its medium: nx * ny * nz densities, x fastest
struct VolumeDev {
    const float *rho;
    int32_t nx, ny, nz;
};
template <class Table>
struct VolumeLit {
    GlossLit<Table> G;
    MediumDev M;          // region 2, sigma_t > 0: the host hands every other call to the medium's or the lit kernels
    VolumeDev V;
};

// plane(m) of an axis with n cells of width w between lo and hi: the box's own faces at the ends
__device__ __forceinline__ float volume_plane(float lo, float hi, float w, int32_t n, int32_t m) { return m == 0 ? lo : (m == n ? hi : lo + (float)m * w); }
// tnext of an axis at cell c
__device__ __forceinline__ float volume_tnext(float lo, float hi, float w, int32_t n, int32_t c, float o, float d) {
    if (d == 0.0f) return INFINITY;
    return (volume_plane(lo, hi, w, n, d > 0.0f ? c + 1 : c) - o) / d;
}
// the entry cell of an axis
__device__ __forceinline__ int32_t volume_entry(float lo, float w, int32_t n, float p) {
    const int32_t c = (int32_t)floorf((p - lo) / w);
    return c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
}

// The walk of the header over the non-empty interval [t0, t1] of the ray (o, d), len = |d|.  kFlight: v is rem on entry; true = an event,
// v its parameter t.  Otherwise v is acc, the optical depth, and the result is false.  cells counts the cells visited (the probe's
// column; the render kernels drop it)
template <bool kFlight>
__device__ __forceinline__ bool volume_walk(const MediumDev &M, const VolumeDev &V, f3 o, f3 d, float t0, float t1, float len, float &v, int32_t &cells) {
    const float wx = (M.b[0] - M.a[0]) / (float)V.nx, wy = (M.b[1] - M.a[1]) / (float)V.ny, wz = (M.b[2] - M.a[2]) / (float)V.nz;
    int32_t cx = volume_entry(M.a[0], wx, V.nx, o.x + t0 * d.x);
    int32_t cy = volume_entry(M.a[1], wy, V.ny, o.y + t0 * d.y);
    int32_t cz = volume_entry(M.a[2], wz, V.nz, o.z + t0 * d.z);
    // (tnext of an axis is a function of its cell index alone: only the axis that stepped is computed again — the same values as
    // computing all three at every cell, at a third of the divisions)
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
        const float seg = (tb - ta) * len;
        const float sigma_c = M.sigma_t * V.rho[((size_t)cz * (size_t)V.ny + (size_t)cy) * (size_t)V.nx + (size_t)cx];
        cells++;
        if (kFlight) {
            if (sigma_c > 0.0f) {
                const float s = v / sigma_c;
                if (s < seg) {
                    v = ta + s / len;
                    return true;
                }
                v = v - sigma_c * seg;
            }
        } else {
            v = v + sigma_c * seg;
        }
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
    return false;
}

// Tr of a shadow ray (o, d) that ended at t_end, as a factor on its contribution c
template <class Table>
__device__ __forceinline__ f3 volume_attenuate(const VolumeLit<Table> &T, f3 o, f3 d, float t_end, f3 c, int32_t &cells) {
    float t0, t1;
    if (!medium_interval(T.M, o, d, t_end, t0, t1)) return c;
    const float len = sqrt_cr(lensq(d));
    float acc = 0.0f;
    volume_walk<false>(T.M, T.V, o, d, t0, t1, len, acc, cells);
    const float tr = exp_libm(-acc);
    return scale(tr, c);
}

// medium_vertex with the free flight through the cells: false = no event (the caller runs shade_lit2), true = a medium vertex, done
template <class Table>
__device__ __forceinline__ bool volume_vertex(Lane &L, const KParams &P, const VolumeLit<Table> &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o,
                                              f3 &out_d, LitSamples &S, float &carry_out, bool &more, int32_t &events, int32_t &cells) {
    float t0, t1;
    if (!medium_interval(T.M, L.o, L.d, L.hit < 0 ? INFINITY : L.closest, t0, t1)) return false;
    const float len = sqrt_cr(lensq(L.d));
    const float u = random_float(med);
    if (u == 0.0f) return false;
    float v = -log_libm(u);
    if (!volume_walk<true>(T.M, T.V, L.o, L.d, t0, t1, len, v, cells)) return false;
    medium_vertex_at(L, P, T.G, T.M, nee, env, med, add(L.o, scale(v, L.d)), out_o, out_d, S, carry_out, more, events);
    return true;
}

// ---- probe (rt_trace_samples_volume): medium_probe_body with the cell walk in both places ---------------------------------------------
template <bool kLens, class Table>
__device__ __forceinline__ void volume_probe_body(const KParams &P, const VolumeLit<Table> &T, const LensCam &C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                                  uint32_t *med_seed_out, int32_t *events_out, int32_t *cells_out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    uint32_t nee = light_seed_of(T.G.N, base_seed, s), env = light_seed_of(T.G.E, base_seed, s), med = medium_seed_of(base_seed, s);
    f3 ray_o, ray_d;
    lit_start<kLens>(L, P, C, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0, events = 0, cells = 0;
    float prev = 0.0f;
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
            LitSamples S;
            S.code = -1;
            float carry;
            bool more;
            if (!volume_vertex(L, P, T, nee, env, med, ray_o, ray_d, S, carry, more, events, cells)) more = shade_lit2(L, P, T.G, prev, nee, env, ray_o, ray_d, S, carry);
            if (S.a) {
                rays++;
                begin_ray(L, ray_o, S.adir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, false);
                if (L.hit == S.code) L.color = add(L.color, volume_attenuate(T, L.o, L.d, L.closest, S.ac, cells));
            }
            if (S.b) {
                rays++;
                begin_ray(L, ray_o, S.bdir, 0);
                while (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, true);
                if (L.hit < 0) L.color = add(L.color, volume_attenuate(T, L.o, L.d, INFINITY, S.bc, cells));
            }
            if (!more) break;
            prev = carry;
            begin_ray(L, ray_o, ray_d, 0);
        }
    }
    P.probe_rad[3 * g] = L.color.x; P.probe_rad[3 * g + 1] = L.color.y; P.probe_rad[3 * g + 2] = L.color.z;
    P.probe_rays[g] = rays;
    P.probe_seed[g] = L.seed;
    nee_seed_out[g] = nee;
    env_seed_out[g] = env;
    med_seed_out[g] = med;
    events_out[g] = events;
    cells_out[g] = cells;
}

// ---- the trace kernel of rt_render_volume ---------------------------------------------------------------------------------------------
// medium_render_body's wave loop, restated (a change to either loop has to be made in both, and in lit_render_body's), with the cell walk
// as the free flight and as the optical depth at the two shadow verdicts.  Nothing more lives across the tree walks than in the medium
// kernel: the walk's cell indices and plane parameters begin and end inside the shade branch.
// One text for both of its forms, like medium_render_body's (RTP_MEDIUM_RENDER_BODY): TOTAL is the number of work indices (wave-uniform)
// and WORK_OF_MINE what the fetched index `mine` stands for.
#define RTP_VOLUME_RENDER_BODY(TOTAL, WORK_OF_MINE)                                                                                                   \
    using Lit = GlossLit<Table>;                                                                                                                      \
    const int lane = (int)(threadIdx.x & (kWave - 1));                                                                                                \
    Lane L;                                                                                                                                           \
    L.node = kBlocked;                                                                                                                                \
    L.sp = 0;                                                                                                                                         \
    L.hit = -1;                                                                                                                                       \
    L.closest = 1e30f;                                                                                                                                \
    L.color = mk(0.0f, 0.0f, 0.0f);                                                                                                                   \
    L.beta = mk(1.0f, 1.0f, 1.0f);                                                                                                                    \
    L.depth = 0;                                                                                                                                      \
    L.seed = 0;                                                                                                                                       \
    int32_t phase = kLightIdle;                                                                                                                       \
    uint32_t w = 0, nee = 0, env = 0, med = 0;                                                                                                        \
    LitCarry<Lit> prev_diffuse = LitCarry<Lit>(0);                                                                                                    \
    f3 next_d = mk(0, 0, 0);                                                                                                                          \
    LitSamples S;                                                                                                                                     \
    S.adir = S.ac = S.bdir = S.bc = mk(0, 0, 0);                                                                                                      \
    S.code = -1;                                                                                                                                      \
    S.a = S.b = false;                                                                                                                                \
    uint32_t pool_next = 0, pool_end = 0;  /* (wave-uniform) */                                                                                       \
    bool exhausted = false;                                                                                                                           \
    for (;;) {                                                                                                                                        \
        RTP_LIT_POOL_FETCH(TOTAL, WORK_OF_MINE, T.G, med = medium_seed_of(base_seed, s);)                                                             \
        const bool busy = phase != kLightIdle;                                                                                                        \
        if (!__any(busy)) {                                                                                                                           \
            if (exhausted) break;                                                                                                                     \
            continue;                                                                                                                                 \
        }                                                                                                                                             \
        const bool walking = busy && !traversal_finished<true>(L, kBlocked);                                                                          \
        const bool ready = busy && !walking;                                                                                                          \
        const int n_walk = __popcll(__ballot(walking));                                                                                               \
        const int n_ready = __popcll(__ballot(ready));                                                                                                \
        if (n_walk == 0 || n_ready >= kLightShadeLanes) {                                                                                             \
            if (ready) {                                                                                                                              \
                int32_t cells = 0;          /* (never read: the probe's column) */                                                                    \
                if (phase == kLightPath) {                                                                                                            \
                    f3 next_o;                                                                                                                        \
                    float carry;                                                                                                                      \
                    bool more;                                                                                                                        \
                    int32_t events = 0;                                                                                                               \
                    if (!volume_vertex(L, P, T, nee, env, med, next_o, next_d, S, carry, more, events, cells))                                        \
                        more = shade_lit2(L, P, T.G, prev_diffuse, nee, env, next_o, next_d, S, carry);                                               \
                    prev_diffuse = carry;                                                                                                             \
                    if (!more && (S.a || S.b)) next_d = mk(0, 0, 0);                                                                                  \
                    if (S.a) {                                                                                                                        \
                        begin_ray(L, next_o, S.adir, 0);                                                                                              \
                        phase = S.b ? kLitShadowAB : kLitShadowA;                                                                                     \
                    } else if (S.b) {                                                                                                                 \
                        begin_ray(L, next_o, S.bdir, 0);                                                                                              \
                        phase = kLitShadowB;                                                                                                          \
                    } else if (more) {                                                                                                                \
                        begin_ray(L, next_o, next_d, 0);                                                                                              \
                    } else {                                                                                                                          \
                        store_sample(P, w, L.color);                                                                                                  \
                        phase = kLightIdle;                                                                                                           \
                    }                                                                                                                                 \
                } else if (phase == kLitShadowB) {                                                                                                    \
                    if (L.hit < 0) L.color = add(L.color, volume_attenuate(T, L.o, L.d, INFINITY, S.bc, cells));                                      \
                    if (no_next_ray(next_d)) {                                                                                                        \
                        store_sample(P, w, L.color);                                                                                                  \
                        phase = kLightIdle;                                                                                                           \
                    } else {                                                                                                                          \
                        begin_ray(L, L.o, next_d, 0);                                                                                                 \
                        phase = kLightPath;                                                                                                           \
                    }                                                                                                                                 \
                } else {                                                                                                                              \
                    if (L.hit == S.code) L.color = add(L.color, volume_attenuate(T, L.o, L.d, L.closest, S.ac, cells));                               \
                    const bool then_env = phase == kLitShadowAB;                                                                                      \
                    if (!then_env && no_next_ray(next_d)) {                                                                                           \
                        store_sample(P, w, L.color);                                                                                                  \
                        phase = kLightIdle;                                                                                                           \
                    } else {                                                                                                                          \
                        begin_ray(L, L.o, then_env ? S.bdir : next_d, 0);                                                                             \
                        phase = then_env ? kLitShadowB : kLightPath;                                                                                  \
                    }                                                                                                                                 \
                }                                                                                                                                     \
                if (phase == kLightIdle) {                                                                                                            \
                    L.node = kBlocked;                                                                                                                \
                    L.sp = 0;                                                                                                                         \
                }                                                                                                                                     \
            }                                                                                                                                         \
        } else {                                                                                                                                      \
            const bool occlusion = phase == kLitShadowB;                                                                                              \
            _Pragma("unroll")                                                                                                                         \
            for (int u = 0; u < 4; ++u) {                                                                                                             \
                if (!traversal_finished<true>(L, kBlocked)) lit_step(L, P, occlusion);                                                                \
            }                                                                                                                                         \
        }                                                                                                                                             \
    }
// kList = false: a pass of rt_render_volume's.  kList = true: rt_render_volume_adaptive's rounds (DESIGN.md §29), the list as
// medium_render_body takes it.
template <bool kLens, class Table, bool kList = false>
__device__ __forceinline__ void volume_render_body(const KParams &P, const VolumeLit<Table> &T, const LensCam &C) {
    if constexpr (kList) {
        uint32_t listed = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)*P.work_count);
        if (listed > P.work_cap) listed = P.work_cap;          // (never more entries than the list has room for)
        if (listed == 0u) return;
        RTP_VOLUME_RENDER_BODY(listed, P.work_list[mine])
    } else {
        RTP_VOLUME_RENDER_BODY(P.total_work, mine)
    }
}
#undef RTP_VOLUME_RENDER_BODY
#undef RTP_LIT_POOL_FETCH          // (defined in rt_light.hip.inc, which leaves it for rt_medium.hip.inc and this file: no expansion of it may follow)

template <bool kLens, class Table>
__global__ void __launch_bounds__(256) volume_probe_kernel(const KParams P, const VolumeLit<Table> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                                           uint32_t *med_seed_out, int32_t *events_out, int32_t *cells_out) {
    volume_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out, med_seed_out, events_out, cells_out);
}
// (waves per SIMD the compiler is held to, for all eight: the medium kernels' — DESIGN.md §28, profiles/r28/kernel_resource_usage.txt)
constexpr int kVolumeWaves = kMediumWaves;
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kVolumeWaves) volume_render_kernel(const KParams P, const VolumeLit<Table> T, const LensCam C) {
    volume_render_body<kLens>(P, T, C);
}
// the list variant: rt_render_volume_adaptive's rounds (DESIGN.md §29) — the same body on a list whose length lives on the device
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kVolumeWaves) volume_list_render_kernel(const KParams P, const VolumeLit<Table> T, const LensCam C) {
    volume_render_body<kLens, Table, true>(P, T, C);
}

}  // namespace rtk
