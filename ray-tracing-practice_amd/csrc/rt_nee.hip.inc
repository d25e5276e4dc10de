// rt_nee.hip.inc — next-event estimation (rt_render_nee; include/rtp_amd.h, rt_nee_params; DESIGN.md §13): the emitter table and its
// light sample.  Included by rt_capi.hip after rt_kernel.hip.inc; the vertex, the probe and the trace kernel that use it are
// rt_light.hip.inc's.
//
// The path draws exactly what rt_render draws; at every diffuse event (LAMBERTIAN, or METAL's hemisphere branch) whose next query is
// still inside max_depth, one light sample is taken from a second RNG stream: an emitter sphere from the handle's table (cdf, by
// bisection), a direction uniform in the cone the sphere subtends, and a shadow ray through the same walk.  The BSDF ray that leaves
// the same vertex has its hit on a table sphere weighted by the power heuristic (or by 0: light sampling alone).  With select = 1 the
// entry comes from a descent of the light tree at the end of this file instead of the cdf (DESIGN.md §18).  Every expression is
// the header's, in its order (the project's float rules: nothing fused, correctly rounded division and sqrt).
#pragma once

namespace rtk {

constexpr uint32_t kNeeStreamKey = RT_NEE_STREAM_KEY;       // nee = wang_hash(sample_seed ^ key)
constexpr float kNeeTwoPi = RT_NEE_TWO_PI;
constexpr float kNeePb = RT_NEE_PB;                          // density of the uniform-hemisphere direction, 1 / (2 pi)
constexpr float kGlossMinFuzz = RT_GLOSSY_MIN_FUZZ;          // a METAL reflect branch below this fuzz is a mirror: no light sample

// pg of the header ("glossy events"): the density in solid angle of unit(r + fuzz * B), B uniform in the unit ball, at the direction w —
// the integral of t^2 over the chord w cuts through the ball of radius fuzz about r, over the ball's volume
__device__ __forceinline__ float gloss_pg(f3 w, f3 r, float fuzz) {
    const float c = dot(w, r);
    const float ff = fuzz * fuzz;
    const float disc = (c * c - 1.0f) + ff;
    if (!(disc > 0.0f)) return 0.0f;
    const float s = sqrt_cr(disc);
    const float t2 = c + s;
    if (!(t2 > 0.0f)) return 0.0f;
    const float t1 = c - s;
    const float f3v = ff * fuzz;
    if (t1 > 0.0f) return (s * (3.0f * (c * c) + s * s)) / (kNeeTwoPi * f3v);
    return ((t2 * t2) * t2) / ((2.0f * kNeeTwoPi) * f3v);        // fuzz > 1: the vertex is inside the ball
}
// pb of a light sample in the direction w: the BSDF strategy's density there.  A diffuse event's is the constant (the expressions fold to
// what they were when kNeePb stood in them); a glossy event's is pg about its mirror direction
// The carried value: what a ray remembers of the event it left, for the weight of what it finds.  The kernels of today carry a bool
// (diffuse or not: pb is the constant); the glossy instantiations a float — 0 none, RT_NEE_PB diffuse, pg(unit(new_d)) glossy, and a pg
// that rounded to 0 is "none": weight 1, never 0 / 0
__device__ __forceinline__ bool carry_on(bool c) { return c; }
__device__ __forceinline__ bool carry_on(float c) { return c != 0.0f; }
__device__ __forceinline__ float carry_pb(bool) { return kNeePb; }
__device__ __forceinline__ float carry_pb(float c) { return c; }
__device__ __forceinline__ void carry_diffuse(bool &c) { c = true; }
__device__ __forceinline__ void carry_diffuse(float &c) { c = kNeePb; }
struct PbDiffuse {
    static constexpr bool kGlossy = false;
    __device__ __forceinline__ float operator()(f3) const { return kNeePb; }
};
struct PbGlossy {
    static constexpr bool kGlossy = true;
    f3 r;
    float fuzz;
    __device__ __forceinline__ float operator()(f3 w) const { return gloss_pg(w, r, fuzz); }
};
// Does a light sample at this kind of vertex have a hemisphere — is a direction with dot(dir, n) <= 0 refused?  Every surface vertex's has;
// a vertex in a participating medium has no normal (PbPhase, rt_medium.hip.inc)
template <class Pb> constexpr bool kPbHemisphere = true;
__device__ __forceinline__ PbGlossy gloss_pb(f3 r, float fuzz) {
    PbGlossy g;
    g.r = r;
    g.fuzz = fuzz;
    return g;
}

// The sphere-only emitter table of a handle (global memory, sphere order): sphere index, cdf (last entry 1), pmf
struct NeeTable {
    const int32_t *index;
    const float *cdf;
    const float *pmf;
    int32_t count;
    int32_t mis;          // 1: power heuristic, 0: light sampling alone
};

// The emitter table of sample_planes = 1 (DESIGN.md §17), used when it holds a plane: the table's spheres first (sphere order), then
// its planes (plane order).  code = 2 * index + kind (0 sphere, 1 plane) — what a hit on that primitive is (Lane::hit), increasing
// within each of the two ranges; area: A of a plane, 0 for a sphere
struct EmitTable {
    const int32_t *code;
    const float *cdf;
    const float *pmf;
    const float *area;
    int32_t count;
    int32_t spheres;      // entries [0, spheres) are spheres, [spheres, count) planes
    int32_t mis;
};

// smallest e with u < cdf[e]; count when there is none (u == 1.0f)
template <class Table>
__device__ __forceinline__ int32_t nee_pick(const Table &T, float u) {
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
// the table entry of a hit (code), -1 when that primitive is not in the table: a bisection of the range of its kind
__device__ __forceinline__ int32_t emit_find(const EmitTable &T, int32_t code) {
    const bool plane = (code & 1) != 0;
    int32_t lo = plane ? T.spheres : 0, hi = plane ? T.count : T.spheres;
    const int32_t end = hi;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (T.code[mid] < code) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && T.code[lo] == code) ? lo : -1;
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
// contribution; else the shadow ray's direction (from x), the code of the sphere it has to reach and what it adds then.  PB: the BSDF
// strategy's density in that direction (PbDiffuse, or at a glossy event PbGlossy — whose 0 is "no contribution" too)
// steps 2 to 4 for a picked sphere (pmf: where its entry's stands — read only by a sample that counts)
template <class Pb>
__device__ __forceinline__ bool nee_sample_sphere(const KParams &P, int32_t sphere, const float *pmf, int32_t mis, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, Pb PB,
                                                  f3 &dir, f3 &c, int32_t &code) {
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
    if (kPbHemisphere<Pb> && !(dot(dir, n) > 0.0f)) return false;
    const float pb = PB(dir);
    if (Pb::kGlossy && pb == 0.0f) return false;
    const float pl = *pmf * nee_pdf_cone(om);
    const float f = mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    const float4 ME = P.materials[3 * P.sphere_mat[sphere] + 1];
    c = scale(f, mul(mul(beta, a), mk(ME.x, ME.y, ME.z)));
    code = 2 * sphere;
    return true;
}
template <class Pb>
__device__ __forceinline__ bool nee_sample(const KParams &P, const NeeTable &T, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    const float u = random_float(nee);
    const int32_t e = nee_pick(T, u);
    if (e >= T.count) return false;
    return nee_sample_sphere(P, T.index[e], T.pmf + e, T.mis, nee, x, n, a, beta, PB, dir, c, code);
}

// ---- emissive planes (sample_planes = 1) ----------------------------------------------------------------------------------------------
// step 3p of the header: the point y of plane `plane` (area A) seen from x.  false: no contribution; else wl = (y - x) / |y - x| and
// pa, the density of y in solid angle at x
__device__ __forceinline__ bool emit_plane_pa(const KParams &P, int32_t plane, float A, f3 x, f3 y, f3 &wl, float &pa) {
    const f3 w = sub(y, x);
    const float d2 = dot(w, w);
    if (!(d2 > 0.0f)) return false;
    const float len = sqrt_cr(d2);
    wl = mk(w.x / len, w.y / len, w.z / len);
    const float4 P0 = P.planes[5 * plane + 0];
    const float cos_l = fabsf(dot(mk(P0.x, P0.y, P0.z), wl));
    if (!(cos_l >= 1e-8f)) return false;
    pa = d2 / (cos_l * A);
    return true;
}
// steps 2p to 4p for the picked entry e, a plane: a point uniform in area (QUAD: the parallelogram; TRIANGLE: its lower half, by the
// fold; ELLIPSE: the inscribed ellipse, by the disc's rejection loop), two-sided
// (one text for the table's pick and the light tree's: RTP_EMIT_PLANE_STEPS, the body of a function with P, T, e, nee, x, n, a, beta, dir,
// c and code in scope; PMF: the probability of the pick that gave e)
#define RTP_EMIT_PLANE_STEPS(PMF)                                                                                                        \
    const int32_t hit = T.code[e];                                                                                                       \
    const int32_t plane = hit >> 1;                                                                                                      \
    const float4 P1 = P.planes[5 * plane + 1];                                                                                           \
    const float4 P2 = P.planes[5 * plane + 2];                                                                                           \
    const float4 P3 = P.planes[5 * plane + 3];                                                                                           \
    const float4 P4 = P.planes[5 * plane + 4];                                                                                           \
    const int32_t type = as_int(P1.w);                                                                                                   \
    float ua, ub;                                                                                                                        \
    if (type == RT_PLANE_ELLIPSE) {                                                                                                      \
        float px, py, q2;                                                                                                                \
        do {                                                                                                                             \
            px = random_pm1(nee);                                                                                                        \
            py = random_pm1(nee);                                                                                                        \
            q2 = px * px + py * py;                                                                                                      \
        } while (q2 >= 1.0f);                                                                                                            \
        ua = 0.5f + 0.5f * px;                                                                                                           \
        ub = 0.5f + 0.5f * py;                                                                                                           \
    } else {                                                                                                                             \
        ua = random_float(nee);                                                                                                          \
        ub = random_float(nee);                                                                                                          \
        if (type == RT_PLANE_TRIANGLE && ua + ub > 1.0f) {                                                                               \
            ua = 1.0f - ua;                                                                                                              \
            ub = 1.0f - ub;                                                                                                              \
        }                                                                                                                                \
    }                                                                                                                                    \
    const f3 y = mk((P4.x + ua * P2.x) + ub * P3.x, (P4.y + ua * P2.y) + ub * P3.y, (P4.z + ua * P2.z) + ub * P3.z);                     \
    float pa;                                                                                                                            \
    if (!emit_plane_pa(P, plane, T.area[e], x, y, dir, pa)) return false;                                                                \
    if (kPbHemisphere<Pb> && !(dot(dir, n) > 0.0f)) return false;                                                                        \
    const float pb = PB(dir);                                                                                                            \
    if (Pb::kGlossy && pb == 0.0f) return false;                                                                                         \
    const float pl = PMF * pa;                                                                                                           \
    const float f = T.mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;                                                                   \
    const float4 ME = P.materials[3 * as_int(P2.w) + 1];                                                                                 \
    c = scale(f, mul(mul(beta, a), mk(ME.x, ME.y, ME.z)));                                                                               \
    code = hit;                                                                                                                          \
    return true;
template <class Pb>
__device__ __forceinline__ bool emit_sample_plane(const KParams &P, const EmitTable &T, int32_t e, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c,
                                                  int32_t &code) {
    RTP_EMIT_PLANE_STEPS(T.pmf[e])
}
// (the light tree's: pmf is the descent's product)
template <class Pb>
__device__ __forceinline__ bool tree_sample_plane(const KParams &P, const EmitTable &T, int32_t e, float pmf, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir,
                                                  f3 &c, int32_t &code) {
    RTP_EMIT_PLANE_STEPS(pmf)
}
#undef RTP_EMIT_PLANE_STEPS
// the light sample of the two-kind table: step 1, then the steps of the entry's kind
template <class Pb>
__device__ __forceinline__ bool emit_sample(const KParams &P, const EmitTable &T, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    const float u = random_float(nee);
    const int32_t e = nee_pick(T, u);
    if (e >= T.count) return false;
    if (e < T.spheres) return nee_sample_sphere(P, T.code[e] >> 1, T.pmf + e, T.mis, nee, x, n, a, beta, PB, dir, c, code);
    return emit_sample_plane(P, T, e, nee, x, n, a, beta, PB, dir, c, code);
}

// ---- the light tree (select = 1; DESIGN.md §18) ---------------------------------------------------------------------------------------
// A bounding-sphere hierarchy over a table's entries, built on the host (rt_capi.hip, TreeBuilder), in preorder: the left child of an
// interior node i is node i + 1.  Two float4 per node, read through L1 / L2: (centre, radius) and (weight, q, right, entry) — right and
// entry as int bits, right = -1 at a leaf, entry = -1 at an interior node.  Per entry: its path from the root (bit i set: step i goes
// right) and its depth.  The pick replaces step 1 of the header; the steps after it are the table's own with the descent's pmf.
struct LightTree {
    const float4 *node;
    const uint32_t *path;
    const int32_t *depth;
};
struct TreeTable {          // the sphere-only table and its tree
    NeeTable N;
    LightTree L;
};
struct TreeEmitTable {      // the two-kind table and its tree
    EmitTable N;
    LightTree L;
};
// the importance of a child (A: centre and radius, W: weight) from x
__device__ __forceinline__ float tree_importance(float4 A, float W, f3 x) {
    const f3 w = sub(mk(A.x, A.y, A.z), x);
    const float d2 = dot(w, w);
    return W / fmaxf(d2, A.w * A.w);
}
// One level below the interior node `node` (B: its second word) from x: the probability pL of its left child, and both children's second
// words.  The descent and the path product take every level through here — the same expressions in the same order
__device__ __forceinline__ float tree_level(const LightTree &L, int32_t node, float4 B, f3 x, float4 &LB, float4 &RB) {
    const int32_t l = node + 1, r = as_int(B.z);
    const float4 LA = L.node[2 * l];
    LB = L.node[2 * l + 1];
    const float4 RA = L.node[2 * r];
    RB = L.node[2 * r + 1];
    const float il = tree_importance(LA, LB.x, x);
    const float ir = tree_importance(RA, RB.x, x);
    const float s = il + ir;
    return (s > 0.0f && s < INFINITY) ? il / s : B.y;
}
// the pick: one draw per level; the entry of the leaf it ends on and p, the probability of that descent
__device__ __forceinline__ int32_t tree_pick(const LightTree &L, uint32_t &nee, f3 x, float &p) {
    int32_t node = 0;
    float4 B = L.node[1];
    p = 1.0f;
    while (as_int(B.z) >= 0) {
        float4 LB, RB;
        const float pl = tree_level(L, node, B, x, LB, RB);
        const float u = random_float(nee);
        const bool left = u < pl;
        p = p * (left ? pl : 1.0f - pl);
        node = left ? node + 1 : as_int(B.z);
        B = left ? LB : RB;
    }
    return as_int(B.w);
}
// pmf_e(x): the same product root-down along entry e's stored path
__device__ __forceinline__ float tree_pmf(const LightTree &L, int32_t e, f3 x) {
    const uint32_t path = L.path[e];
    const int32_t depth = L.depth[e];
    int32_t node = 0;
    float4 B = L.node[1];
    float p = 1.0f;
    for (int32_t i = 0; i < depth; ++i) {
        float4 LB, RB;
        const float pl = tree_level(L, node, B, x, LB, RB);
        const bool left = ((path >> i) & 1u) == 0u;
        p = p * (left ? pl : 1.0f - pl);
        node = left ? node + 1 : as_int(B.z);
        B = left ? LB : RB;
    }
    return p;
}
template <class Pb>
__device__ __forceinline__ bool tree_sample(const KParams &P, const TreeTable &T, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    float p;
    const int32_t e = tree_pick(T.L, nee, x, p);
    return nee_sample_sphere(P, T.N.index[e], &p, T.N.mis, nee, x, n, a, beta, PB, dir, c, code);
}
template <class Pb>
__device__ __forceinline__ bool tree_sample(const KParams &P, const TreeEmitTable &T, uint32_t &nee, f3 x, f3 n, f3 a, f3 beta, Pb PB, f3 &dir, f3 &c, int32_t &code) {
    float p;
    const int32_t e = tree_pick(T.L, nee, x, p);
    if (e < T.N.spheres) return nee_sample_sphere(P, T.N.code[e] >> 1, &p, T.N.mis, nee, x, n, a, beta, PB, dir, c, code);
    return tree_sample_plane(P, T.N, e, p, nee, x, n, a, beta, PB, dir, c, code);
}

}  // namespace rtk
