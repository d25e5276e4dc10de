// rt_env.hip.inc — image-based lighting (rt_render_env; include/rtp_amd.h, rt_env_params; DESIGN.md §14): the octahedral map, what a
// miss adds and the light sample.  Included by rt_capi.hip after rt_nee.hip.inc; the vertex, the probe and the trace kernel that use it
// are rt_light.hip.inc's.
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
// (prev: the carried fact — rt_light.hip.inc, "the carried value" — whose pb is RT_NEE_PB after a diffuse event, pg after a glossy one)
template <class Carry>
__device__ __forceinline__ f3 env_miss(const EnvDev &E, f3 d, f3 beta, Carry prev) {
    f3 p;
    const int32_t t = env_texel(env_rotate(E, d), E.n, p);
    const float4 T = E.texels[t];
    f3 term = mul(beta, mk(E.scale * T.x, E.scale * T.y, E.scale * T.z));
    if (carry_on(prev) && E.sampled) {
        const float q2 = dot(p, p);
        const float pl = env_pl(E, T.w, q2, sqrt_cr(q2));
        const float pb = carry_pb(prev);
        const float wb = E.mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
        term = scale(wb, term);
    }
    return term;
}

// The light sample of a diffuse vertex with face-forwarded normal n, albedo a and throughput beta (before the attenuation): false =
// no contribution; else the shadow ray's direction and what it adds when it hits nothing
template <class Pb>
__device__ __forceinline__ bool env_sample(const EnvDev &E, uint32_t &env, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c) {
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
    if (kPbHemisphere<Pb> && !(dot(dir, n) > 0.0f)) return false;
    const float pb = PB(dir);
    if (Pb::kGlossy && pb == 0.0f) return false;
    const float4 T = E.texels[(size_t)iy * (size_t)E.n + (size_t)ix];
    const float pl = env_pl(E, T.w, q2, q);
    const float f = E.mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    c = scale(f, mul(mul(beta, a), mk(E.scale * T.x, E.scale * T.y, E.scale * T.z)));
    return true;
}

// ---- probe ---------------------------------------------------------------------------------------------------------------------------
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

}  // namespace rtk
