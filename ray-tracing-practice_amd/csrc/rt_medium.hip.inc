// rt_medium.hip.inc — a homogeneous participating medium on the lit path (rt_render_medium; include/rtp_amd.h, "participating medium";
// DESIGN.md §25).  Included by rt_capi.hip after rt_light.hip.inc, whose vertex (shade_lit2), camera (lit_start), walk step (lit_step),
// light samples (light_sample) and pool fetch (RTP_LIT_POOL_FETCH) it uses as they are; rt_volume.hip.inc follows and uses the same.
//
// What is new here: the region's interval on a ray, the free-flight draw in front of the surface vertex, the medium vertex — both light
// samples with the phase function as the BSDF strategy's density (PbPhase, no hemisphere) and a Henyey-Greenstein direction whose density
// the next ray carries like a glossy event's pg — and the transmittance of a shadow ray at its verdict.  The light is always a
// GlossLit<Table> (the float carry); whether METAL's reflect branch samples is its runtime gn / ge.  Every expression is the header's, in
// its order.
#pragma once

namespace rtk {

constexpr uint32_t kMediumStreamKey = RT_MEDIUM_STREAM_KEY;       // med = wang_hash(sample_seed ^ key)
constexpr float kFourPi = 2.0f * RT_NEE_TWO_PI;

// The call's medium, by value beside its light
struct MediumDev {
    int32_t region;       // 0 all space, 1 ball (a, b[0]), 2 box (a, b)
    float sigma_t;        // > 0: sigma_t == 0 never reaches these kernels (the host hands such a call to rt_render_lit's)
    float albedo[3];
    float g;
    float a[3], b[3];
};
template <class Table>
struct MediumLit {
    GlossLit<Table> G;
    MediumDev M;
};

// interval(o, d, t_end) of the header: false = empty
__device__ __forceinline__ bool medium_interval(const MediumDev &M, f3 o, f3 d, float t_end, float &t0, float &t1) {
    t0 = 0.0f;
    t1 = t_end;
    if (M.region == 1) {
        const f3 oc = sub(o, mk(M.a[0], M.a[1], M.a[2]));
        const float A = lensq(d);
        const float hb = dot(oc, d);
        const float cc = lensq(oc) - M.b[0] * M.b[0];
        const float disc = hb * hb - A * cc;
        if (!(disc > 0.0f)) return false;
        const float sq = sqrt_cr(disc);
        const float ta = (-hb - sq) / A;
        const float tb = (-hb + sq) / A;
        t0 = ta > 0.0f ? ta : 0.0f;
        t1 = tb < t_end ? tb : t_end;
    } else if (M.region == 2) {
        const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (dd[k] == 0.0f) {
                if (!(M.a[k] < oo[k] && oo[k] < M.b[k])) return false;
            } else {
                float ta = (M.a[k] - oo[k]) / dd[k];
                float tb = (M.b[k] - oo[k]) / dd[k];
                if (ta > tb) {
                    const float tt = ta;
                    ta = tb;
                    tb = tt;
                }
                if (ta > t0) t0 = ta;
                if (tb < t1) t1 = tb;
            }
        }
    }
    return t1 > t0;
}
// ph(c) of the header: Henyey-Greenstein's density in solid angle at the cosine c between the direction of travel and the new direction
__device__ __forceinline__ float medium_ph(float g, float c) {
    if (g == 0.0f) return 1.0f / kFourPi;
    const float den = (1.0f + g * g) - (2.0f * g) * c;
    return (1.0f - g * g) / (kFourPi * (den * sqrt_cr(den)));
}
// pb of a light sample at a medium vertex: ph at the sampled direction (which need not be unit).  Its 0 is "no contribution", and there
// is no hemisphere
struct PbPhase {
    static constexpr bool kGlossy = true;
    f3 ud;
    float g;
    __device__ __forceinline__ float operator()(f3 w) const { return medium_ph(g, dot(ud, w) / sqrt_cr(lensq(w))); }
};
template <> constexpr bool kPbHemisphere<PbPhase> = false;

// Tr of a shadow ray (o, d) that ended at t_end, as a factor on its contribution c
__device__ __forceinline__ f3 medium_attenuate(const MediumDev &M, f3 o, f3 d, float t_end, f3 c) {
    float t0, t1;
    if (!medium_interval(M, o, d, t_end, t0, t1)) return c;
    const float len = sqrt_cr(lensq(d));
    const float tr = exp_libm(-(M.sigma_t * ((t1 - t0) * len)));
    return scale(tr, c);
}
__device__ __forceinline__ uint32_t medium_seed_of(uint32_t base_seed, int32_t s) { return wang_hash(wang_hash(base_seed + (uint32_t)s) ^ kMediumStreamKey); }

// The medium vertex at x, the point a free flight along the lane's path ray (L.o, L.d) ended at — the homogeneous flight below, or the
// cell walk of rt_volume.hip.inc.  The vertex is done on return: `more` as shade_lit2 returns it, the light samples in S, the next ray
// (out_o, out_d) and what it carries
template <class Lit>
__device__ __forceinline__ void medium_vertex_at(Lane &L, const KParams &P, const Lit &G, const MediumDev &M, uint32_t &nee, uint32_t &env, uint32_t &med,
                                                 const f3 x, f3 &out_o, f3 &out_d, LitSamples &S, float &carry_out, bool &more, int32_t &events) {
    events++;
    S.a = false;
    S.b = false;
    carry_out = 0.0f;
    more = false;
    const f3 ud = unit(L.d);
    const f3 beta_in = L.beta;
    const f3 alb = mk(M.albedo[0], M.albedo[1], M.albedo[2]);
    L.beta = mul(L.beta, alb);
    if (L.beta.x == 0.0f && L.beta.y == 0.0f && L.beta.z == 0.0f) return;
    if (!(L.depth + 1 < P.max_depth)) return;
    PbPhase pb;
    pb.ud = ud;
    pb.g = M.g;
    if (light_on(G.N)) S.a = light_sample(P, G.N, nee, x, ud, alb, beta_in, pb, S.adir, S.ac, S.code);
    if (env_sampled(G)) S.b = light_sample(P, G.E, env, x, ud, alb, beta_in, pb, S.bdir, S.bc, S.code);
    // the next direction: Henyey-Greenstein's cosine by inversion, the azimuth by the disc loop, Duff's basis around ud
    const float u1 = random_float(med);
    float cos_t;
    if (M.g == 0.0f) {
        cos_t = 1.0f - 2.0f * u1;
    } else {
        const float q = (1.0f - M.g * M.g) / ((1.0f - M.g) + (2.0f * M.g) * u1);
        cos_t = ((1.0f + M.g * M.g) - q * q) / (2.0f * M.g);
        cos_t = cos_t < -1.0f ? -1.0f : (cos_t > 1.0f ? 1.0f : cos_t);
    }
    const float sin_t = sqrt_cr(fmaxf(0.0f, 1.0f - cos_t * cos_t));
    float px, py, q2;
    do {
        px = random_pm1(med);
        py = random_pm1(med);
        q2 = px * px + py * py;
    } while (q2 >= 1.0f || q2 == 0.0f);
    const float qq = sqrt_cr(q2);
    const float cx = px / qq, cy = py / qq;
    const float sgn = copysignf(1.0f, ud.z);
    const float ba = -1.0f / (sgn + ud.z);
    const float bb = (ud.x * ud.y) * ba;
    const f3 b1 = mk(1.0f + ((sgn * ud.x) * ud.x) * ba, sgn * bb, -sgn * ud.x);
    const f3 b2 = mk(bb, sgn + (ud.y * ud.y) * ba, -ud.y);
    const float sx = sin_t * cx, sy = sin_t * cy;
    out_d = mk((b1.x * sx + b2.x * sy) + ud.x * cos_t, (b1.y * sx + b2.y * sy) + ud.y * cos_t, (b1.z * sx + b2.z * sy) + ud.z * cos_t);
    out_o = x;
    carry_out = medium_ph(M.g, cos_t);
    L.depth++;
    more = true;
}

// ---- the medium's hooks in lit_probe_body and lit_render_body (rt_light.hip.inc, "what fog adds to a lit light"; DESIGN.md §31) ------------
template <class Table> __device__ __forceinline__ const GlossLit<Table> &fog_lit(const MediumLit<Table> &T) { return T.G; }
template <class Table> __device__ __forceinline__ uint32_t fog_seed(const MediumLit<Table> &, uint32_t base_seed, int32_t s) { return medium_seed_of(base_seed, s); }
template <class Table> __device__ __forceinline__ f3 fog_tr(const MediumLit<Table> &T, f3 o, f3 d, float t_end, f3 c, FogCount &) {
    return medium_attenuate(T.M, o, d, t_end, c);
}
// The free-flight step of a lane whose path ray has finished its closest-hit query (L.hit, L.closest), in front of the surface vertex
template <class Table>
__device__ __forceinline__ bool fog_vertex(Lane &L, const KParams &P, const MediumLit<Table> &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o, f3 &out_d,
                                           LitSamples &S, float &carry_out, bool &more, FogCount &n) {
    const MediumDev &M = T.M;
    float t0, t1;
    if (!medium_interval(M, L.o, L.d, L.hit < 0 ? INFINITY : L.closest, t0, t1)) return false;
    const float len = sqrt_cr(lensq(L.d));
    const float u = random_float(med);
    if (u == 0.0f) return false;
    const float s = -log_libm(u) / M.sigma_t;
    if (!(s < (t1 - t0) * len)) return false;
    medium_vertex_at(L, P, T.G, M, nee, env, med, add(L.o, scale(t0 + s / len, L.d)), out_o, out_d, S, carry_out, more, n.events);
    return true;
}

// ---- the kernels of rt_render_medium and rt_trace_samples_medium: lit_render_body and lit_probe_body on a MediumLit<Table> ------------
template <bool kLens, class Table>
__global__ void __launch_bounds__(256) medium_probe_kernel(const KParams P, const MediumLit<Table> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                                           uint32_t *med_seed_out, int32_t *events_out) {
    lit_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out, med_seed_out, events_out);
}
// (waves per SIMD the compiler is held to, for all eight: DESIGN.md §25, profiles/r25/kernel_resource_usage.txt)
constexpr int kMediumWaves = 3;
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) medium_render_kernel(const KParams P, const MediumLit<Table> T, const LensCam C) {
    lit_render_body<kLens>(P, T, C);
}
// the list variant: rt_render_volume_adaptive's rounds without a grid (DESIGN.md §29) — the same body on a list whose length lives on the device
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) medium_list_render_kernel(const KParams P, const MediumLit<Table> T, const LensCam C) {
    lit_render_body<kLens, MediumLit<Table>, true>(P, T, C);
}
template <bool kLens, class Table> const void *lit_frame_kernel_of(const MediumLit<Table> &) { return (const void *)medium_render_kernel<kLens, Table>; }
template <bool kLens, class Table> const void *lit_list_kernel_of(const MediumLit<Table> &) { return (const void *)medium_list_render_kernel<kLens, Table>; }

}  // namespace rtk
