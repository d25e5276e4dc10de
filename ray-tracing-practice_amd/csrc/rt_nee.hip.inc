// rt_nee.hip.inc — next-event estimation (rt_render_nee; include/rtp_amd.h, rt_nee_params; DESIGN.md §13): the emitter table and its
// light sample.  Included by rt_capi.hip after rt_kernel.hip.inc; the vertex, the probe and the trace kernel that use it are
// rt_light.hip.inc's.
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

// The light sample of a diffuse vertex at x (face-forwarded normal n, albedo a, throughput beta before the attenuation): false = no
// contribution; else the shadow ray's direction (from x), the code of the sphere it has to reach and what it adds then
__device__ __forceinline__ bool nee_sample(const KParams &P, const NeeTable &T, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, f3 &dir, f3 &c, int32_t &code) {
    const float u = random_float(nee);
    const int32_t e = nee_pick(T, u);
    if (e >= T.count) return false;
    const int32_t sphere = T.index[e];
    f3 w;
    float d2, om;
    if (!nee_cone(x, P.spheres[sphere], w, d2, om)) return false;
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
    dir = mk((t1.x * sx + t2.x * sy) + wn.x * cos_t, (t1.y * sx + t2.y * sy) + wn.y * cos_t, (t1.z * sx + t2.z * sy) + wn.z * cos_t);
    if (!(dot(dir, n) > 0.0f)) return false;
    const float pl = T.pmf[e] * nee_pdf_cone(om);
    const float f = T.mis ? (kNeePb * pl) / (pl * pl + kNeePb * kNeePb) : kNeePb / pl;
    const float4 ME = P.materials[3 * P.sphere_mat[sphere] + 1];
    c = scale(f, mul(mul(beta, a), mk(ME.x, ME.y, ME.z)));
    code = 2 * sphere;
    return true;
}

}  // namespace rtk
