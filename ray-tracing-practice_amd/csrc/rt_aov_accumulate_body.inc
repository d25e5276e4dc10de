// rt_aov_accumulate_body.inc — the body of the AOV accumulate kernels (included by rt_aov.hip.inc, inside aov_accumulate_kernel and
// aov_accumulate_lens_kernel): one text, so that the pinhole kernel compiles to the code it did before lens frames existed.  Each
// kernel defines RTP_AOV_WALK and RTP_AOV_HIT (aov_walk / aov_hit with its camera) before including this file.
    __shared__ float4 tile4[kAccWaves][64 * kAovRow / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t num_pixels = P.num_pixels, pitch = P.slab_pitch;
    const int32_t count = P.pass_count;
    const uint32_t pg = (blockIdx.x * (uint32_t)kAccWaves + (uint32_t)wave) * 64u;
    if (pg >= num_pixels) return;
    const uint32_t q = pg + (uint32_t)lane;
    const bool in = q < num_pixels;
    f3 alb = mk(0.0f, 0.0f, 0.0f), nrm = mk(0.0f, 0.0f, 0.0f);
    float dep = 0.0f;
    uint32_t hits = 0u;
    int32_t prim = -1;
    if (in && !first_pass) {
        if (out.albedo) alb = mk(out.albedo[3 * (size_t)q], out.albedo[3 * (size_t)q + 1], out.albedo[3 * (size_t)q + 2]);
        if (out.normal) nrm = mk(out.normal[3 * (size_t)q], out.normal[3 * (size_t)q + 1], out.normal[3 * (size_t)q + 2]);
        if (out.depth) dep = out.depth[q];
        if (out.hits) hits = out.hits[q];
    }
    const f3 bg = mk(P.bg[0], P.bg[1], P.bg[2]);
    const bool sky = P.cand != nullptr && in && P.cand[(size_t)q * kCandWords] == 0u;
    auto store = [&]() {
        if (out.albedo) { out.albedo[3 * (size_t)q] = alb.x; out.albedo[3 * (size_t)q + 1] = alb.y; out.albedo[3 * (size_t)q + 2] = alb.z; }
        if (out.normal) { out.normal[3 * (size_t)q] = nrm.x; out.normal[3 * (size_t)q + 1] = nrm.y; out.normal[3 * (size_t)q + 2] = nrm.z; }
        if (out.depth) out.depth[q] = dep;
        if (out.hits) out.hits[q] = hits;
        if (out.prim && first_pass) out.prim[q] = prim;
    };
    if (P.cand != nullptr && __ballot(sky) == __ballot(in)) {        // a wave of nothing but sky
        if (in) {
            for (int32_t s = 0; s < count; ++s) alb = add(alb, bg);
            store();
        }
        return;
    }
    int32_t pi = 0, pj = 0;
    if (in) aov_pixel(P, q, pi, pj);
    uint32_t rewalked = 0;
    float *tile = reinterpret_cast<float *>(tile4[wave]);
    const uint32_t npix = num_pixels - pg < 64u ? num_pixels - pg : 64u;
    for (uint32_t s0 = 0; s0 < (uint32_t)count; s0 += kAovSlots) {
        const uint32_t ns = pitch - s0 < (uint32_t)kAovSlots ? pitch - s0 : (uint32_t)kAovSlots;      // slots of this tile (padding included: multiple of 4)
        const uint32_t seg4 = ns * 3u / 4u;
        const uint32_t total4 = npix * seg4;
        for (uint32_t k = (uint32_t)lane; k < total4; k += 64u) {
            const uint32_t pl = k / seg4, f4 = k - pl * seg4;
            const float4 v = *reinterpret_cast<const float4 *>(P.slab + ((size_t)(pg + pl) * pitch + s0) * 3 + f4 * 4u);
            *reinterpret_cast<float4 *>(tile + pl * kAovRow + f4 * 4u) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint32_t nv = (uint32_t)count - s0 < (uint32_t)kAovSlots ? (uint32_t)count - s0 : (uint32_t)kAovSlots;
        if (in && !sky) {
            const float *row = tile + lane * kAovRow;
            for (uint32_t s = 0; s < nv; ++s) {
                float t = row[3 * s];
                int32_t code = __float_as_int(row[3 * s + 1]);
                if (code == kPrimFlag || code == kPrimWalk) {       // (kPrimWalk: its pixel was resolved by aov_resolve_kernel — not met here)
                    code = RTP_AOV_WALK(P, pi, pj, __float_as_uint(row[3 * s + 2]), t);
                    ++rewalked;
                }
                if (s0 + s == 0u) prim = code >= 0 ? code : -1;
                if (code >= 0) {
                    f3 a, n;
                    RTP_AOV_HIT(P, pi, pj, __float_as_uint(row[3 * s + 2]), t, code, a, n);
                    alb = add(alb, a);
                    nrm = add(nrm, n);
                    dep = dep + t;
                    ++hits;
                } else {
                    alb = add(alb, bg);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    if (sky)
        for (int32_t s = 0; s < count; ++s) alb = add(alb, bg);
    if (in) store();
    if (rewalked != 0u) atomicAdd(walked, rewalked);
