// rt_glow.hip.inc — emission in the medium on the lit path (rt_render_glow; include/rtp_amd.h, "emission in the medium"; DESIGN.md §35).
// Included by rt_capi.hip after rt_volume.hip.inc, whose walk (volume_walk) it uses, with rt_medium.hip.inc's interval (medium_interval),
// medium vertex (medium_vertex_at), stream and light as they are; rt_light.hip.inc's probe and wave loop run its kernels, through the
// hooks at the end.
//
// What is new here: the emitted radiance of a path ray as a track-length estimate — the emission coefficient summed over the stretch the
// ray's own free flight flew, E, times the call's radiance and the throughput the ray arrived with, added before the vertex adds anything.
// No draw, no exp and no shadow ray are added; shadow rays emit nothing.  Every expression is the header's, in its order.
#pragma once

namespace rtk {

// A light with fog (MediumLit<Table> or VolumeLit<Table>, as the grey kernels hold it) and the radiance per unit length at h = 1; over a
// grid also the cells' h: null = 1 everywhere (source 0), the density itself (source 1) or a heat grid of the volume's dimensions (source 2)
template <class Base>
struct GlowLit {
    Base B;
    float r0, r1, r2;
};
template <class Table>
struct GlowLit<VolumeLit<Table>> {
    VolumeLit<Table> B;
    float r0, r1, r2;
    const float *heat;
};

// The free flight of the draw u over the non-empty interval [t0, t1]: true = an event, t its parameter.  E: the emission-weighted length
// of what was flown (without a grid the length itself, D).  glow_adds: whether that length is added (D = +inf is not)
template <class Table>
__device__ __forceinline__ bool glow_flight(const GlowLit<MediumLit<Table>> &T, f3, f3, float t0, float t1, float len, float u, float &t, float &E, FogCount &) {
    const float whole = (t1 - t0) * len;
    E = whole;
    if (u == 0.0f) return false;
    const float s = -log_libm(u) / T.B.M.sigma_t;
    if (!(s < whole)) return false;
    E = s;
    t = t0 + s / len;
    return true;
}
template <class Table>
__device__ __forceinline__ bool glow_flight(const GlowLit<VolumeLit<Table>> &T, f3 o, f3 d, float t0, float t1, float len, float u, float &t, float &E, FogCount &n) {
    t = u == 0.0f ? INFINITY : -log_libm(u);
    E = 0.0f;
    float unused = 0.0f;
    return volume_walk<true, false, true>(T.B.M, T.B.V, o, d, t0, t1, len, t, n.cells, unused, T.heat, E);
}
template <class Table> __device__ __forceinline__ bool glow_adds(const GlowLit<MediumLit<Table>> &, float E) { return E < INFINITY; }
template <class Table> __device__ __forceinline__ bool glow_adds(const GlowLit<VolumeLit<Table>> &, float) { return true; }

// The free flight of a lane whose path ray has finished its closest-hit query, with what the medium emitted towards the ray's origin over
// it.  length: the probe's sum of E
template <class Base>
__device__ __forceinline__ bool glow_vertex(Lane &L, const KParams &P, const GlowLit<Base> &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o, f3 &out_d,
                                            LitSamples &S, float &carry_out, bool &more, FogCount &n, float &length) {
    float t0, t1;
    if (!medium_interval(T.B.M, L.o, L.d, L.hit < 0 ? INFINITY : L.closest, t0, t1)) return false;
    const float len = sqrt_cr(lensq(L.d));
    const float u = random_float(med);
    float t, E;
    const bool event = glow_flight(T, L.o, L.d, t0, t1, len, u, t, E, n);
    length = length + E;
    if (glow_adds(T, E)) L.color = add(L.color, mk(L.beta.x * (T.r0 * E), L.beta.y * (T.r1 * E), L.beta.z * (T.r2 * E)));
    if (!event) return false;
    medium_vertex_at(L, P, T.B.G, T.B.M, nee, env, med, add(L.o, scale(t, L.d)), out_o, out_d, S, carry_out, more, n.events);
    return true;
}

// ---- the hooks in lit_probe_body and lit_render_body (rt_light.hip.inc, "what fog adds to a lit light"): the base's light, stream and
// shadow transmittance
template <class Base> __device__ __forceinline__ auto fog_lit(const GlowLit<Base> &T) -> decltype(fog_lit(T.B)) { return fog_lit(T.B); }
template <class Base> __device__ __forceinline__ uint32_t fog_seed(const GlowLit<Base> &T, uint32_t base_seed, int32_t s) { return fog_seed(T.B, base_seed, s); }
template <class Base> __device__ __forceinline__ f3 fog_tr(const GlowLit<Base> &T, f3 o, f3 d, float t_end, f3 c, FogCount &n) { return fog_tr(T.B, o, d, t_end, c, n); }
template <class Base>
__device__ __forceinline__ bool fog_vertex(Lane &L, const KParams &P, const GlowLit<Base> &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o, f3 &out_d,
                                           LitSamples &S, float &carry_out, bool &more, FogCount &n) {
    float length = 0.0f;
    return glow_vertex(L, P, T, nee, env, med, out_o, out_d, S, carry_out, more, n, length);
}

// The probe's light: the same, with the place where the sample's glow_length is summed (lit_probe_body knows no such column: the probe
// kernel owns it)
template <class Base>
struct GlowProbeLit {
    GlowLit<Base> G;
    float *length;
};
template <class Base> __device__ __forceinline__ auto fog_lit(const GlowProbeLit<Base> &T) -> decltype(fog_lit(T.G.B)) { return fog_lit(T.G.B); }
template <class Base> __device__ __forceinline__ uint32_t fog_seed(const GlowProbeLit<Base> &T, uint32_t base_seed, int32_t s) { return fog_seed(T.G.B, base_seed, s); }
template <class Base> __device__ __forceinline__ f3 fog_tr(const GlowProbeLit<Base> &T, f3 o, f3 d, float t_end, f3 c, FogCount &n) { return fog_tr(T.G.B, o, d, t_end, c, n); }
template <class Base>
__device__ __forceinline__ bool fog_vertex(Lane &L, const KParams &P, const GlowProbeLit<Base> &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o, f3 &out_d,
                                           LitSamples &S, float &carry_out, bool &more, FogCount &n) {
    return glow_vertex(L, P, T.G, nee, env, med, out_o, out_d, S, carry_out, more, n, *T.length);
}

// ---- the kernels of rt_render_glow and rt_trace_samples_glow: lit_render_body and lit_probe_body on a GlowLit of either base.  Nothing
// more lives across the tree walks than in the base's kernel: E and the heat read begin and end inside the shade branch
template <bool kLens, class Base>
__global__ void __launch_bounds__(256) glow_probe_kernel(const KParams P, const GlowLit<Base> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                                         uint32_t *med_seed_out, int32_t *events_out, int32_t *cells_out, float *length_out) {
    float length = 0.0f;
    const GlowProbeLit<Base> TP{T, &length};
    lit_probe_body<kLens>(P, TP, C, nee_seed_out, env_seed_out, med_seed_out, events_out, cells_out);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < P.probe_n) length_out[g] = length;
}
template <bool kLens, class Base>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) glow_render_kernel(const KParams P, const GlowLit<Base> T, const LensCam C) {
    lit_render_body<kLens>(P, T, C);
}
// the list variant: rt_render_fog_adaptive's rounds under a glow (DESIGN.md §40) — the same body on a list whose length lives on the device
template <bool kLens, class Base>
__global__ void __launch_bounds__(kLightBlock, kMediumWaves) glow_list_render_kernel(const KParams P, const GlowLit<Base> T, const LensCam C) {
    lit_render_body<kLens, GlowLit<Base>, true>(P, T, C);
}
template <bool kLens, class Base> const void *lit_frame_kernel_of(const GlowLit<Base> &) { return (const void *)glow_render_kernel<kLens, Base>; }
template <bool kLens, class Base> const void *lit_list_kernel_of(const GlowLit<Base> &) { return (const void *)glow_list_render_kernel<kLens, Base>; }

}  // namespace rtk
