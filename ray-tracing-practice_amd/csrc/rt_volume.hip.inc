// rt_volume.hip.inc — heterogeneous fog from a density grid on the lit path (rt_render_volume; include/rtp_amd.h, "density grid";
// DESIGN.md §28).  Included by rt_capi.hip after rt_medium.hip.inc, whose interval (medium_interval), medium vertex (medium_vertex_at),
// phase function, stream and light it uses as they are; rt_light.hip.inc's probe and wave loop run its kernels, through the hooks at the end.
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
struct VolumeLit : MediumLit<Table> {          // (M: region 2, sigma_t > 0 — the host hands every other call to the medium's or the lit kernels)
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
// column; the render kernels drop it).  kAcc (a flight of rt_chroma.hip.inc): the flight keeps the optical depth of the cells it passed in acc as well.
// kGlow (a flight of rt_glow.hip.inc): the flight keeps E, the length it flew weighted per cell by h_c — heat's value at the cell, or 1 where heat is null
// (volume_cells of rt_glow_sample.hip.inc states the same cells, bounds and order once more, with what a cell does passed in — this text
// could not take a callback without moving the listings of the kernels on it; gs_cells of tests/cpu_native/glow_sample_ref.c restates
// that one.  A change to the entry cell, tnext, the clamp, the step or the break here is made there as well)
template <bool kFlight, bool kAcc, bool kGlow>
__device__ __forceinline__ bool volume_walk(const MediumDev &M, const VolumeDev &V, f3 o, f3 d, float t0, float t1, float len, float &v, int32_t &cells, float &acc,
                                            const float *heat, float &E) {
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
        const size_t at = ((size_t)cz * (size_t)V.ny + (size_t)cy) * (size_t)V.nx + (size_t)cx;
        const float sigma_c = M.sigma_t * V.rho[at];
        cells++;
        if (kFlight) {
            float h_c = 1.0f;
            if (kGlow && heat) h_c = heat[at];
            if (sigma_c > 0.0f) {
                const float s = v / sigma_c;
                if (s < seg) {
                    if (kGlow) E = E + h_c * s;
                    v = ta + s / len;
                    return true;
                }
                v = v - sigma_c * seg;
            }
            if (kAcc) acc = acc + sigma_c * seg;
            if (kGlow) E = E + h_c * seg;
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
template <bool kFlight, bool kAcc = false>
__device__ __forceinline__ bool volume_walk(const MediumDev &M, const VolumeDev &V, f3 o, f3 d, float t0, float t1, float len, float &v, int32_t &cells, float &acc) {
    float unused = 0.0f;
    return volume_walk<kFlight, kAcc, false>(M, V, o, d, t0, t1, len, v, cells, acc, nullptr, unused);
}
template <bool kFlight>
__device__ __forceinline__ bool volume_walk(const MediumDev &M, const VolumeDev &V, f3 o, f3 d, float t0, float t1, float len, float &v, int32_t &cells) {
    float unused = 0.0f;
    return volume_walk<kFlight, false>(M, V, o, d, t0, t1, len, v, cells, unused);
}

// ---- the grid's hooks in lit_probe_body and lit_render_body (rt_light.hip.inc, "what fog adds to a lit light"; DESIGN.md §31): the
// medium's own light and stream, the walk as the optical depth of a shadow ray and as the free flight
template <class Table>
__device__ __forceinline__ f3 fog_tr(const VolumeLit<Table> &T, f3 o, f3 d, float t_end, f3 c, FogCount &n) {
    float t0, t1;
    if (!medium_interval(T.M, o, d, t_end, t0, t1)) return c;
    const float len = sqrt_cr(lensq(d));
    float acc = 0.0f;
    volume_walk<false>(T.M, T.V, o, d, t0, t1, len, acc, n.cells);
    const float tr = exp_libm(-acc);
    return scale(tr, c);
}
template <class Table>
__device__ __forceinline__ bool fog_vertex(Lane &L, const KParams &P, const VolumeLit<Table> &T, uint32_t &nee, uint32_t &env, uint32_t &med, f3 &out_o, f3 &out_d,
                                           LitSamples &S, float &carry_out, bool &more, FogCount &n) {
    float t0, t1;
    if (!medium_interval(T.M, L.o, L.d, L.hit < 0 ? INFINITY : L.closest, t0, t1)) return false;
    const float len = sqrt_cr(lensq(L.d));
    const float u = random_float(med);
    if (u == 0.0f) return false;
    float v = -log_libm(u);
    if (!volume_walk<true>(T.M, T.V, L.o, L.d, t0, t1, len, v, n.cells)) return false;
    medium_vertex_at(L, P, T.G, T.M, nee, env, med, add(L.o, scale(v, L.d)), out_o, out_d, S, carry_out, more, n.events);
    return true;
}

// ---- the kernels of rt_render_volume and rt_trace_samples_volume: lit_render_body and lit_probe_body on a VolumeLit<Table>.  Nothing
// more lives across the tree walks than in the medium kernel: the walk's cell indices and plane parameters begin and end inside the shade branch
template <bool kLens, class Table>
__global__ void __launch_bounds__(256) volume_probe_kernel(const KParams P, const VolumeLit<Table> T, const LensCam C, uint32_t *nee_seed_out, uint32_t *env_seed_out,
                                                           uint32_t *med_seed_out, int32_t *events_out, int32_t *cells_out) {
    lit_probe_body<kLens>(P, T, C, nee_seed_out, env_seed_out, med_seed_out, events_out, cells_out);
}
// (waves per SIMD the compiler is held to, for all eight: the medium kernels' — DESIGN.md §28, profiles/r28/kernel_resource_usage.txt)
constexpr int kVolumeWaves = kMediumWaves;
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kVolumeWaves) volume_render_kernel(const KParams P, const VolumeLit<Table> T, const LensCam C) {
    lit_render_body<kLens>(P, T, C);
}
// the list variant: rt_render_volume_adaptive's rounds (DESIGN.md §29) — the same body on a list whose length lives on the device
template <bool kLens, class Table>
__global__ void __launch_bounds__(kLightBlock, kVolumeWaves) volume_list_render_kernel(const KParams P, const VolumeLit<Table> T, const LensCam C) {
    lit_render_body<kLens, VolumeLit<Table>, true>(P, T, C);
}
template <bool kLens, class Table> const void *lit_frame_kernel_of(const VolumeLit<Table> &) { return (const void *)volume_render_kernel<kLens, Table>; }
template <bool kLens, class Table> const void *lit_list_kernel_of(const VolumeLit<Table> &) { return (const void *)volume_list_render_kernel<kLens, Table>; }

}  // namespace rtk
