/* adaptive_prior_ref.c — CPU restatement of rt_adaptive_prior's arithmetic as include/rtp_amd.h states it ("a history-aware stopping
 * rule"), for the bit-exact comparisons of tests/test_adaptive_prior.py (tests/adaptive_prior_reference.py builds it like
 * denoise_temporal_spp_reference.py builds its file: gcc -ffp-contract=off -fno-fast-math).  The prepass quantities (n, z, d) are the
 * header's for rt_denoise and rt_denoise_spp, the reprojection the one it states for rt_denoise_temporal, written out again here as
 * denoise_temporal_spp_ref.c does, keeping the sums of cnt and V alone.  Written from the header's contract, not from the kernel.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define HIST_MAGIC_SPP 0x32485452u
#define HIST_HEADER 256
#define MODE_MOMENTS 2u

typedef struct {
    float origin[3], p00[3], du[3], dv[3], background[3];
    int32_t width, height, spp, max_depth;
} camera; /* rt_camera_data */

static float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static float lum(const float *c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }

/* cam: rt_camera_data (76 bytes); hist_prev: NULL or a history buffer of the header's layout (W * H * 64 + 256 bytes); the AOV sums at A
 * samples per pixel; prior: 2 floats per pixel.  0 on success. */
int adaptive_prior_reference(const void *cam_bytes, int A, const float *albedo, const float *normal, const float *depth, const uint32_t *hits,
                             const int32_t *prim_of, const void *hist_prev, float *prior) {
    camera cam, hcam;
    memcpy(&cam, cam_bytes, sizeof(cam));
    const int W = cam.width, H = cam.height;
    const size_t P = (size_t)W * (size_t)H;
    const float min_weight = 0.01f, min_normal_dot = 0.9f, tau2 = 0.0025f;
    const float invA = (float)(1.0 / (double)A);
    const camera *h = NULL;
    if (hist_prev) {
        uint32_t head[4];
        memcpy(head, hist_prev, 16);
        memcpy(&hcam, (const char *)hist_prev + 16, sizeof(hcam));
        if (head[0] == HIST_MAGIC_SPP && (int32_t)head[1] == W && (int32_t)head[2] == H && head[3] == MODE_MOMENTS) h = &hcam;
    }
    const float *planes = hist_prev ? (const float *)((const char *)hist_prev + HIST_HEADER) : NULL;
    const float *hmom = planes ? planes + 4 * P : NULL, *hpos = planes ? planes + 8 * P : NULL, *hnrm = planes ? planes + 12 * P : NULL;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            float *out = prior + 2 * p;
            out[0] = 0.0f, out[1] = 0.0f;
            if (hits[p] == 0 || !h) continue;
            float d[3], n[3] = {0.0f, 0.0f, 0.0f};
            for (int k = 0; k < 3; ++k) d[k] = fmaxf(albedo[3 * p + k] * invA, 1e-3f);
            const float dl = lum(d);
            const float *N3 = normal + 3 * p;
            const float len2 = (N3[0] * N3[0] + N3[1] * N3[1]) + N3[2] * N3[2];
            if (len2 != 0.0f) {
                const float len = sqrtf(len2);
                n[0] = N3[0] / len, n[1] = N3[1] / len, n[2] = N3[2] / len;
            }
            const float z = depth[p] / (float)hits[p];
            const int32_t prim = prim_of[p];
            float X[3], OX[3];
            for (int k = 0; k < 3; ++k) {
                const float pc = (cam.p00[k] + (float)x * cam.du[k]) + (float)y * cam.dv[k];
                X[k] = cam.origin[k] + z * (pc - cam.origin[k]);
                OX[k] = X[k] - cam.origin[k];
            }
            const float reach2 = tau2 * dot3(OX, OX);
            const float N[3] = {h->du[1] * h->dv[2] - h->du[2] * h->dv[1], h->du[2] * h->dv[0] - h->du[0] * h->dv[2],
                                h->du[0] * h->dv[1] - h->du[1] * h->dv[0]};
            float E[3], D[3], R[3];
            for (int k = 0; k < 3; ++k) E[k] = h->p00[k] - h->origin[k], D[k] = X[k] - h->origin[k];
            const float tt = dot3(E, N) / dot3(D, N);
            if (!(tt > 0.0f && tt < INFINITY)) continue;
            for (int k = 0; k < 3; ++k) R[k] = tt * D[k] - E[k];
            const float u = dot3(R, h->du) / dot3(h->du, h->du), v = dot3(R, h->dv) / dot3(h->dv, h->dv);
            if (!(u > -1.0f && u < (float)W && v > -1.0f && v < (float)H)) continue;
            const float fu = floorf(u), fv = floorf(v), fx = u - fu, fy = v - fv;
            const int x0 = (int)fu, y0 = (int)fv;
            float Wt = 0.0f, SC = 0.0f, SV = 0.0f;
            for (int tap = 0; tap < 4; ++tap) {
                const int qx = x0 + (tap & 1), qy = y0 + (tap >> 1);
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                const size_t q = (size_t)qy * W + qx;
                const float *mq = hmom + 4 * q, *nq = hnrm + 4 * q, *xq = hpos + 4 * q;
                int32_t pq;
                memcpy(&pq, mq + 3, 4);
                if (!(mq[2] > 0.0f) || pq != prim) continue;
                if (!(dot3(n, nq) >= min_normal_dot)) continue;
                const float e[3] = {xq[0] - X[0], xq[1] - X[1], xq[2] - X[2]};
                if (!(dot3(e, e) <= reach2)) continue;
                const float w = ((tap & 1) ? fx : 1.0f - fx) * ((tap >> 1) ? fy : 1.0f - fy);
                Wt += w;
                SC += w * xq[3];
                SV += w * nq[3];
            }
            if (Wt >= min_weight) {
                out[0] = SC / Wt;
                out[1] = (SV / Wt) * (dl * dl);
            }
        }
    return 0;
}
