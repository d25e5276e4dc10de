// rt_denoise_reproject.inc — the reprojection of one hit pixel into the previous frame's history, as the statements of the kernels
// that include it (rt_denoise.hip: denoise_temporal, denoise_temporal_spp and adaptive_prior).  One text expanded in each, like
// rt_denoise_taps.inc, so that the calls cannot drift apart and denoise_temporal's instructions stay what they were.  In scope: im, cam, prev, pixels, x, y,
// np (the record of hit pixel p), prim, Lc, m1.  Defines X, reach2 and what RTP_REPROJECT_STATE declares: L, M1, M2, len (and the
// including kernel's own accumulated quantities), left at their disoccluded values unless the history is taken.  The hooks, defined by
// the including kernel and undefined after it:
//     RTP_REPROJECT_STATE        the declaration of L[3], M1, M2, len, … at their disoccluded values
//     RTP_REPROJECT_HISTORY_OK   prev is a history this call takes
//     RTP_REPROJECT_SUMS         declarations of further sums over the taps (beside W, S0..2, SM1, SM2, SN)
//     RTP_REPROJECT_TAP          their accumulation for a tap that counts (w, cq, mq, nq, xq in scope)
//     RTP_REPROJECT_ALPHA        with len set: declares the blend weights a and b
//     RTP_REPROJECT_VARIANCE     after L, M1 and M2 are blended: whatever else is
    // the mean first-hit point along the pixel-centre ray
    const float O[3] = {cam.origin.e[0], cam.origin.e[1], cam.origin.e[2]};
    float X[3], OX[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float pc = (cam.pixel00_loc.e[k] + (float)x * cam.pixel_delta_u.e[k]) + (float)y * cam.pixel_delta_v.e[k];
        X[k] = O[k] + np.w * (pc - O[k]);
        OX[k] = X[k] - O[k];
    }
    const float reach2 = kTau2 * dot3(OX, OX);
    RTP_REPROJECT_STATE
    if (RTP_REPROJECT_HISTORY_OK) {
        // projection through the old viewport plane (normal du' x dv'), pixel units with integers at pixel centres
        const rt_camera_data &c = prev->cam;
        const float du[3] = {c.pixel_delta_u.e[0], c.pixel_delta_u.e[1], c.pixel_delta_u.e[2]};
        const float dv[3] = {c.pixel_delta_v.e[0], c.pixel_delta_v.e[1], c.pixel_delta_v.e[2]};
        const float N[3] = {du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]};
        float E[3], D[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            E[k] = c.pixel00_loc.e[k] - c.origin.e[k];
            D[k] = X[k] - c.origin.e[k];
        }
        const float t = dot3(E, N) / dot3(D, N);
        if (t > 0.0f && t < __builtin_inff()) {
            float R[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) R[k] = t * D[k] - E[k];
            const float u = dot3(R, du) / dot3(du, du), v = dot3(R, dv) / dot3(dv, dv);
            if (u > -1.0f && u < (float)im.width && v > -1.0f && v < (float)im.height) {
                const float fu = floorf(u), fv = floorf(v);
                const int32_t x0 = (int32_t)fu, y0 = (int32_t)fv;
                const float fx = u - fu, fy = v - fv;
                const float4 *h_colour = plane((void *)prev, pixels, 0), *h_moments = plane((void *)prev, pixels, 1);
                const float4 *h_pos = plane((void *)prev, pixels, 2), *h_normal = plane((void *)prev, pixels, 3);
                float W = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, SM1 = 0.0f, SM2 = 0.0f, SN = 0.0f;
                RTP_REPROJECT_SUMS
#pragma unroll
                for (int tap = 0; tap < 4; ++tap) {
                    const int32_t qx = x0 + (tap & 1), qy = y0 + (tap >> 1);
                    if (qx < 0 || qx >= im.width || qy < 0 || qy >= im.height) continue;
                    const int64_t q = (int64_t)qy * im.width + qx;
                    const float4 mq = h_moments[q];
                    if (!(mq.z > 0.0f) || __float_as_int(mq.w) != prim) continue;
                    const float4 nq = h_normal[q];
                    if (!((np.x * nq.x + np.y * nq.y) + np.z * nq.z >= kMinNormalDot)) continue;
                    const float4 xq = h_pos[q];
                    const float e[3] = {xq.x - X[0], xq.y - X[1], xq.z - X[2]};
                    if (!(dot3(e, e) <= reach2)) continue;
                    const float w = ((tap & 1) ? fx : 1.0f - fx) * ((tap >> 1) ? fy : 1.0f - fy);
                    const float4 cq = h_colour[q];
                    W += w;
                    S0 += w * cq.x;
                    S1 += w * cq.y;
                    S2 += w * cq.z;
                    SM1 += w * mq.x;
                    SM2 += w * mq.y;
                    SN += w * mq.z;
                    RTP_REPROJECT_TAP
                }
                if (W >= kMinWeight) {
                    len = fminf(SN / W + 1.0f, kMaxLen);
                    RTP_REPROJECT_ALPHA
                    L[0] = b * (S0 / W) + a * Lc[0];
                    L[1] = b * (S1 / W) + a * Lc[1];
                    L[2] = b * (S2 / W) + a * Lc[2];
                    M1 = b * (SM1 / W) + a * m1;
                    M2 = b * (SM2 / W) + a * (m1 * m1);
                    RTP_REPROJECT_VARIANCE
                }
            }
        }
    }
