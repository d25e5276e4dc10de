// rt_denoise_taps.inc — the 25 taps p + s*(dx, dy) of one à-trous pass, as the statements of the kernels that include it
// (rt_denoise.hip: denoise_step and denoise_step_spp).  One text expanded in each: a shared helper function moved the instructions of
// every denoise_step instantiation, and this text is their old one.  In scope: im, s, sg, lv_in, nz, dg, x, y, p and np, the record
// of hit pixel p.  Defines r, the filtered (L, var) — the pixel's own when no tap has weight.
    const float4 vp = lv_in[p];
    const float gz = dg[p].w;
    const float lp = lum(vp.x, vp.y, vp.z);
    const float rl = rtd::recip(sg.luminance * rtd::sqrt_cr(vp.w) + 1e-4f);
    float rz[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) rz[m] = rtd::recip((sg.depth * gz) * (float)(s * m) + 1e-4f);
    const float kern[3] = {0.375f, 0.25f, 0.0625f};
    float W = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, SV = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int32_t yy = y + dy * s;
        if (yy < 0 || yy >= im.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int32_t xx = x + dx * s;
            if (xx < 0 || xx >= im.width) continue;
            const int64_t q = (int64_t)yy * im.width + xx;
            const float4 nq = nz[q];
            if (is_sky(nq)) continue;
            const float4 vq = lv_in[q];
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const float h = kern[ax] * kern[ay];
            float wn = fmaxf(0.0f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
            for (int k = 0; k < sg.squarings; ++k) wn = wn * wn;
            const float e = fabsf(np.w - nq.w) * rz[ax + ay] + fabsf(lp - lum(vq.x, vq.y, vq.z)) * rl;
            const float w = (h * wn) * rtd::exp_libm(-e);
            W += w;
            S0 += w * vq.x;
            S1 += w * vq.y;
            S2 += w * vq.z;
            SV += (w * w) * vq.w;
        }
    }
    float4 r = vp;
    if (W != 0.0f) r = make_float4(S0 / W, S1 / W, S2 / W, SV / (W * W));
