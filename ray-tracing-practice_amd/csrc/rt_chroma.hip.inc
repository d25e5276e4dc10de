// rt_chroma.hip.inc — fog whose extinction differs per colour channel on the lit path (rt_render_chroma; include/rtp_amd.h, "chromatic
// extinction"; DESIGN.md §34).  Included by rt_capi.hip after rt_volume.hip.inc, whose walk (volume_walk) it uses, with rt_medium.hip.inc's
// interval (medium_interval), medium vertex (medium_vertex_at), stream and light as they are; rt_light.hip.inc's probe and wave loop run
// its kernels, through the hooks at the end.
//
// What is new here: the free flight by ONE channel's extinction, that channel drawn uniformly with a second draw of med, and the weight the
// path then carries per channel — single-sample MIS over the three channels (balance heuristic), each weight in [0, 3] — and the
// transmittance of a shadow ray per channel.  The base light is held with sigma_t = 1, so its interval and its walk measure the density
// length A, and the three extinctions multiply it here.  Every expression is the header's, in its order.
#pragma once

namespace rtk {

// A light with fog (MediumLit<Table> or VolumeLit<Table>, M.sigma_t = 1) and the three channels' extinctions, sigma_k = sigma_t * tint[k]
// (the host's float products: not all equal — the host hands equal ones to the grey kernels)
template <class Base>
struct ChromaLit {
    Base B;
    float s0, s1, s2;
};

// Tr of a channel over the density length A: exactly 1 without extinction (no product: A may be infinite)
__device__ __forceinline__ float chroma_tr(float sigma_k, float A) { return sigma_k == 0.0f ? 1.0f : exp_libm(-(sigma_k * A)); }

// a channel's weight, its term e of den: (3 e) / den, at most 3 (the product's and the quotient's roundings can pass 3 by an ulp; the exact weight cannot)
__device__ __forceinline__ float chroma_weight(float e, float den) {
    const float w = (3.0f * e) / den;
    return w > 3.0f ? 3.0f : w;
}

// the density length of the non-empty interval [t0, t1]; a free flight to the target R: true = an event, t its parameter — otherwise A
template <class Table>
__device__ __forceinline__ float chroma_length(const MediumLit<Table> &, f3, f3, float t0, float t1, float len, FogCount &) { return (t1 - t0) * len; }
template <class Table>
__device__ __forceinline__ float chroma_length(const VolumeLit<Table> &B, f3 o, f3 d, float t0, float t1, float len, FogCount &n) {
    float acc = 0.0f;
    volume_walk<false>(B.M, B.V, o, d, t0, t1, len, acc, n.cells);
    return acc;
}
template <class Table>
__device__ __forceinline__ bool chroma_flight(const MediumLit<Table> &, f3, f3, float t0, float t1, float len, float R, float &t, float &A, FogCount &) {
    A = (t1 - t0) * len;
    if (!(R < A)) return false;
    t = t0 + R / len;
    return true;
}
template <class Table>
__device__ __forceinline__ bool chroma_flight(const VolumeLit<Table> &B, f3 o, f3 d, float t0, float t1, float len, float R, float &t, float &A, FogCount &n) {
    t = R;
    A = 0.0f;
    return volume_walk<true, true>(B.M, B.V, o, d, t0, t1, len, t, n.cells, A);
}

// ---- the hooks in lit_probe_body and lit_render_body (rt_light.hip.inc, "what fog adds to a lit light"): the base's light and stream
template <class Base> __device__ __forceinline__ auto fog_lit(const ChromaLit<Base> &T) -> decltype(fog_lit(T.B)) { return fog_lit(T.B); }
template <class Base> __device__ __forceinline__ uint32_t fog_seed(const ChromaLit<Base> &T, uint32_t base_seed, int32_t s) { return fog_seed(T.B, base_seed, s); }
template <class Base>
__device__ __forceinline__ f3 fog_tr(const ChromaLit<Base> &T, f3 o, f3 d, float t_end, f3 c, FogCount &n) {
    float t0, t1;
    if (!medium_interval(T.B.M, o, d, t_end, t0, t1)) return c;
    const float len = sqrt_cr(lensq(d));
    const float A = chroma_length(T.B, o, d, t0, t1, len, n);
    return mk(chroma_tr(T.s0, A) * c.x, chroma_tr(T.s1, A) * c.y, chroma_tr(T.s2, A) * c.z);
}
// The free flight of a lane whose path ray has finished its closest-hit query.  false: no event — L.beta carries the channels' weights of
// having passed the interval (unchanged where the interval is empty or the flight's draw was exactly 0)
template <class Base>
__device__ __forceinline__ bool fog_vertex(Lane &L, const KParams &P, const ChromaLit<Base> &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o, f3 &out_d,
                                           LitSamples &S, float &carry_out, bool &more, FogCount &n) {
    float t0, t1;
    if (!medium_interval(T.B.M, L.o, L.d, L.hit < 0 ? INFINITY : L.closest, t0, t1)) return false;
    const float len = sqrt_cr(lensq(L.d));
    const float u = random_float(med);
    if (u == 0.0f) return false;
    const float uc = random_float(med);
    const int32_t j = min(2, (int32_t)(uc * 3.0f));
    // (the three extinctions as vector registers before the choice: chosen among the kernel's arguments as they lie, the compiler makes
    // the choice an indexed read of them and reserves a stack frame for it — 116 to 212 bytes of scratch per lane in every render kernel)
    float s0 = T.s0, s1 = T.s1, s2 = T.s2;
    asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2));
    const float sigma_j = j == 0 ? s0 : (j == 1 ? s1 : s2);
    const float R = sigma_j == 0.0f ? INFINITY : -log_libm(u) / sigma_j;
    float t, A;
    const bool event = chroma_flight(T.B, L.o, L.d, t0, t1, len, R, t, A, n);
    if (event) A = R;
    const float tr0 = chroma_tr(T.s0, A), tr1 = chroma_tr(T.s1, A), tr2 = chroma_tr(T.s2, A);
    if (event) {
        const float e0 = T.s0 * tr0, e1 = T.s1 * tr1, e2 = T.s2 * tr2;
        const float den = (e0 + e1) + e2;
        L.beta = mk(L.beta.x * chroma_weight(e0, den), L.beta.y * chroma_weight(e1, den), L.beta.z * chroma_weight(e2, den));
        medium_vertex_at(L, P, T.B.G, T.B.M, nee, env, med, add(L.o, scale(t, L.d)), out_o, out_d, S, carry_out, more, n.events);
        return true;
    }
    const float den = (tr0 + tr1) + tr2;
    L.beta = mk(L.beta.x * chroma_weight(tr0, den), L.beta.y * chroma_weight(tr1, den), L.beta.z * chroma_weight(tr2, den));
    return false;
}

// ---- the kernels of rt_render_chroma and rt_trace_samples_chroma: lit_render_body and lit_probe_body on a ChromaLit of either base.
// Nothing more lives across the tree walks than in the base's kernel: the weights and the three exps begin and end inside the shade branch
template <bool kLens, class Base>
__global__ void __launch_bounds__(256) chroma_probe_kernel(const KParams P, const ChromaLit<Base> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                                           uint32_t *med_seed_out, int32_t *events_out, int32_t *cells_out) {
    lit_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out, med_seed_out, events_out, cells_out);
}
template <bool kLens, class Base>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) chroma_render_kernel(const KParams P, const ChromaLit<Base> T, const LensCam C) {
    lit_render_body<kLens>(P, T, C);
}
// the list variant: rt_render_fog_adaptive's rounds under a tint (DESIGN.md §40) — the same body on a list whose length lives on the device
template <bool kLens, class Base>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) chroma_list_render_kernel(const KParams P, const ChromaLit<Base> T, const LensCam C) {
    lit_render_body<kLens, ChromaLit<Base>, true>(P, T, C);
}
template <bool kLens, class Base> const void *lit_frame_kernel_of(const ChromaLit<Base> &) { return (const void *)chroma_render_kernel<kLens, Base>; }
template <bool kLens, class Base> const void *lit_list_kernel_of(const ChromaLit<Base> &) { return (const void *)chroma_list_render_kernel<kLens, Base>; }

}  // namespace rtk
