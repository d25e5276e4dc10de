/* denoise_temporal_spp_ref.c — CPU restatement of rt_denoise_temporal_spp's arithmetic as include/rtp_amd.h states it ("temporal
 * denoising of adaptively sampled frames"), for the bit-exact comparisons of tests/test_denoise_temporal_spp.py
 * (tests/denoise_temporal_spp_reference.py builds it like denoise_spp_reference.py builds denoise_spp_ref.c: gcc -ffp-contract=off
 * -fno-fast-math).  The prepass with counts, the sample variance, its 3x3 Gaussian and the remodulation with counts are
 * denoise_spp_ref.c's own passes, the second prepass and the iterations denoise_ref.c's, all included here unchanged.  The
 * reprojection is the one the header states for rt_denoise_temporal, written out again here, as denoise_temporal_ref.c does,
 * (that file cannot be included beside denoise_spp_ref.c: both bring denoise_ref.c) with the blend by counts, cnt and V of this
 * call.  Written from the header's contract, not from the kernels.
 */
#include "denoise_spp_ref.c"

#define HIST_MAGIC_FRAMES 0x31485452u /* rt_denoise_temporal's */
#define HIST_MAGIC_SPP 0x32485452u
#define HIST_HEADER 256

typedef struct {
    float origin[3], p00[3], du[3], dv[3], background[3];
    int32_t width, height, spp, max_depth;
} camera; /* rt_camera_data */

typedef struct {
    const camera *cam, *hcam;   /* hcam NULL: empty history */
    const int32_t *prim, *spp;
    int with_moments;
    const float *hcol, *hmom, *hpos, *hnrm;   /* previous history planes (4 floats per pixel) */
    float *mom, *pos, *nrm;                   /* next history planes */
} temporal;

static temporal *g_t;

static float dot3(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/* c->hits is 0 on every pixel that is not a HIT pixel (denoise_temporal_spp_reference makes it so); c->var holds var_cur */
static void pass_temporal_spp(ctx *c, int y0, int y1) {
    const temporal *t = g_t;
    const camera *cam = t->cam;
    const float min_weight = 0.01f, max_len = 32.0f, min_alpha = 0.2f, moments_len = 4.0f, min_normal_dot = 0.9f, tau2 = 0.0025f;
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            float *mom = t->mom + 4 * p, *pos = t->pos + 4 * p, *nrm = t->nrm + 4 * p;
            if (c->hits[p] == 0) {
                memset(mom, 0, 16), memset(pos, 0, 16), memset(nrm, 0, 16);
                continue;
            }
            float *L = c->L + 3 * p;
            const float Lc[3] = {L[0], L[1], L[2]};
            const float m1 = lum(Lc), var_cur = c->var[p], nf = (float)t->spp[p];
            const int32_t prim = t->prim[p];
            float X[3], OX[3];
            for (int k = 0; k < 3; ++k) {
                const float pc = (cam->p00[k] + (float)x * cam->du[k]) + (float)y * cam->dv[k];
                X[k] = cam->origin[k] + c->z[p] * (pc - cam->origin[k]);
                OX[k] = X[k] - cam->origin[k];
            }
            const float reach2 = tau2 * dot3(OX, OX);
            float M1 = m1, M2 = m1 * m1, len = 1.0f, cnt = nf, V = var_cur;
            if (t->hcam) {
                const camera *h = t->hcam;
                const float N[3] = {h->du[1] * h->dv[2] - h->du[2] * h->dv[1], h->du[2] * h->dv[0] - h->du[0] * h->dv[2],
                                    h->du[0] * h->dv[1] - h->du[1] * h->dv[0]};
                float E[3], D[3], R[3];
                for (int k = 0; k < 3; ++k) E[k] = h->p00[k] - h->origin[k], D[k] = X[k] - h->origin[k];
                const float tt = dot3(E, N) / dot3(D, N);
                if (tt > 0.0f && tt < INFINITY) {
                    for (int k = 0; k < 3; ++k) R[k] = tt * D[k] - E[k];
                    const float u = dot3(R, h->du) / dot3(h->du, h->du), v = dot3(R, h->dv) / dot3(h->dv, h->dv);
                    if (u > -1.0f && u < (float)c->W && v > -1.0f && v < (float)c->H) {
                        const float fu = floorf(u), fv = floorf(v), fx = u - fu, fy = v - fv;
                        const int x0 = (int)fu, yq0 = (int)fv;
                        float W = 0.0f, S[3] = {0.0f, 0.0f, 0.0f}, SM1 = 0.0f, SM2 = 0.0f, SN = 0.0f, SC = 0.0f, SV = 0.0f;
                        for (int tap = 0; tap < 4; ++tap) {
                            const int qx = x0 + (tap & 1), qy = yq0 + (tap >> 1);
                            if (qx < 0 || qx >= c->W || qy < 0 || qy >= c->H) continue;
                            const int64_t q = (int64_t)qy * c->W + qx;
                            const float *mq = t->hmom + 4 * q, *nq = t->hnrm + 4 * q, *xq = t->hpos + 4 * q, *cq = t->hcol + 4 * q;
                            int32_t pq;
                            memcpy(&pq, mq + 3, 4);
                            if (!(mq[2] > 0.0f) || pq != prim) continue;
                            if (!(dot3(c->n + 3 * p, nq) >= min_normal_dot)) continue;
                            const float e[3] = {xq[0] - X[0], xq[1] - X[1], xq[2] - X[2]};
                            if (!(dot3(e, e) <= reach2)) continue;
                            const float w = ((tap & 1) ? fx : 1.0f - fx) * ((tap >> 1) ? fy : 1.0f - fy);
                            W += w;
                            for (int k = 0; k < 3; ++k) S[k] += w * cq[k];
                            SM1 += w * mq[0];
                            SM2 += w * mq[1];
                            SN += w * mq[2];
                            SC += w * xq[3];
                            SV += w * nq[3];
                        }
                        if (W >= min_weight) {
                            len = fminf(SN / W + 1.0f, max_len);
                            const float ch = SC / W, s = ch + nf;
                            float a = nf / s;
                            cnt = s;
                            if (!(a >= min_alpha)) a = min_alpha, cnt = nf / min_alpha;
                            const float b = 1.0f - a;
                            for (int k = 0; k < 3; ++k) L[k] = b * (S[k] / W) + a * Lc[k];
                            M1 = b * (SM1 / W) + a * m1;
                            M2 = b * (SM2 / W) + a * (m1 * m1);
                            V = (b * b) * (SV / W) + (a * a) * var_cur;
                        }
                    }
                }
            }
            if (t->with_moments) c->var[p] = V;
            else if (len >= moments_len) c->var[p] = fmaxf(0.0f, M2 - M1 * M1);
            mom[0] = M1, mom[1] = M2, mom[2] = len;
            memcpy(mom + 3, &prim, 4);
            pos[0] = X[0], pos[1] = X[1], pos[2] = X[2], pos[3] = cnt;
            nrm[0] = c->n[3 * p], nrm[1] = c->n[3 * p + 1], nrm[2] = c->n[3 * p + 2], nrm[3] = V;
        }
}

/* cam and hist: rt_camera_data (76 bytes) and history buffers of the header's layout (W * H * 64 + 256 bytes).  hist_prev NULL or
 * not a history this call writes for this size and this use of moments: empty.  spp: 1 int per pixel; moments: NULL or 2 floats.
 * Writes out (3 floats per pixel) and the whole of hist_next.  0 on success. */
int denoise_temporal_spp_reference(const void *cam_bytes, int A, int iterations, float sigma_depth, float sigma_luminance, int squarings,
                                   const float *fb, const int32_t *spp, const float *moments, const float *albedo, const float *normal,
                                   const float *depth, const uint32_t *hits, const int32_t *prim, const void *hist_prev, void *hist_next,
                                   float *out, int threads) {
    camera cam;
    memcpy(&cam, cam_bytes, sizeof(cam));
    const int W = cam.width, H = cam.height;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    if (threads > H) threads = H;
    const size_t P = (size_t)W * (size_t)H;
    const uint32_t mode = moments ? 2u : 1u;
    uint32_t *hit_pixels = calloc(P, 4);
    if (!hit_pixels) return 1;
    for (size_t p = 0; p < P; ++p) hit_pixels[p] = spp[p] >= 1 ? hits[p] : 0;
    ctx c = {W, H, 0, iterations, squarings, sigma_depth, sigma_luminance, fb, albedo, normal, depth, hit_pixels, NULL, NULL, NULL, NULL,
             NULL, NULL, NULL, NULL, out, 0};
    c.L = calloc(3 * P, 4), c.L2 = calloc(3 * P, 4), c.d = calloc(3 * P, 4), c.n = calloc(3 * P, 4);
    c.var = calloc(P, 4), c.var2 = calloc(P, 4), c.z = calloc(P, 4), c.gz = calloc(P, 4);
    counts n = {spp, moments, A, calloc(P, 4)};
    if (!c.L || !c.L2 || !c.d || !c.n || !c.var || !c.var2 || !c.z || !c.gz || !n.v) return 1;
    g_n = &n;
    /* the history header */
    camera hcam;
    const camera *have = NULL;
    if (hist_prev) {
        uint32_t head[4];
        memcpy(head, hist_prev, 16);
        memcpy(&hcam, (const char *)hist_prev + 16, sizeof(hcam));
        if (head[0] == HIST_MAGIC_SPP && (int32_t)head[1] == W && (int32_t)head[2] == H && head[3] == mode) have = &hcam;
    }
    uint8_t *next = hist_next;
    memset(next, 0, HIST_HEADER);
    const uint32_t head[4] = {HIST_MAGIC_SPP, (uint32_t)W, (uint32_t)H, mode};
    memcpy(next, head, 16);
    memcpy(next + 16, &cam, sizeof(cam));
    float *planes = (float *)(next + HIST_HEADER);
    const float *prev = hist_prev ? (const float *)((const char *)hist_prev + HIST_HEADER) : NULL;
    temporal t = {&cam, have, prim, spp, moments != NULL, prev, prev ? prev + 4 * P : NULL, prev ? prev + 8 * P : NULL,
                  prev ? prev + 12 * P : NULL, planes + 4 * P, planes + 8 * P, planes + 12 * P};
    g_t = &t;
    parallel(&c, threads, pass_prepass_spp);
    parallel(&c, threads, pass_moments);
    if (moments) parallel(&c, threads, pass_gauss);
    parallel(&c, threads, pass_temporal_spp);
    /* the colour history: iteration 0's output (the accumulated colour itself with 0 iterations) */
    float *colour = planes;
    memset(colour, 0, 16 * P);
    for (int i = 0; i <= iterations; ++i) {
        if (i == (iterations > 0))
            for (size_t p = 0; p < P; ++p)
                if (hit_pixels[p] > 0)
                    colour[4 * p] = c.L[3 * p], colour[4 * p + 1] = c.L[3 * p + 1], colour[4 * p + 2] = c.L[3 * p + 2], colour[4 * p + 3] = c.var[p];
        if (i == iterations) break;
        c.step = 1 << i;
        parallel(&c, threads, pass_iterate);
        float *tmp = c.L; c.L = c.L2; c.L2 = tmp;
        tmp = c.var; c.var = c.var2; c.var2 = tmp;
    }
    parallel(&c, threads, pass_remodulate_spp);
    free(c.L), free(c.L2), free(c.d), free(c.n), free(c.var), free(c.var2), free(c.z), free(c.gz), free(n.v), free(hit_pixels);
    return 0;
}
