/* denoise_spp_ref.c — CPU restatement of rt_denoise_spp's arithmetic as include/rtp_amd.h states it ("denoising an adaptively
 * sampled frame"), for the bit-exact comparisons of tests/test_denoise_spp.py (tests/denoise_spp_reference.py builds it like
 * denoise_reference.py builds denoise_ref.c: gcc -ffp-contract=off -fno-fast-math).  The second prepass's depth gradient and 3x3
 * luminance variance, and the iterations, are denoise_ref.c's own passes, included here unchanged; this file adds the prepass and
 * the remodulation with each pixel's own count, the sample variance and its 3x3 Gaussian.  Written from the header's contract, not
 * from the kernels.
 */
#include "denoise_ref.c"

typedef struct {
    const int32_t *spp;     /* n per pixel */
    const float *moments;   /* NULL or (S1, S2) per pixel */
    int A;                  /* aov_samples */
    float *v;               /* the sample variance in demodulated space, per pixel */
} counts;

static counts *g_n;   /* the extra state of this file's passes (one call at a time) */

/* c->hits is the hit count of HIT pixels and 0 elsewhere (a count below 1 makes a pixel sky): denoise_spp_reference makes it so */
static void pass_prepass_spp(ctx *c, int y0, int y1) {
    const counts *t = g_n;
    const float invA = (float)(1.0 / (double)t->A);
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            if (c->hits[p] == 0) continue;
            const int32_t n = t->spp[p];
            const float inv_p = (float)(1.0 / (double)n);
            for (int k = 0; k < 3; ++k) {
                const float cc = c->fb[3 * p + k] * inv_p;
                const float a = c->albedo[3 * p + k] * invA;
                c->d[3 * p + k] = fmaxf(a, 1e-3f);
                c->L[3 * p + k] = cc / c->d[3 * p + k];
            }
            const float *N = c->normal + 3 * p;
            const float len2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
            for (int k = 0; k < 3; ++k) c->n[3 * p + k] = len2 == 0.0f ? 0.0f : N[k] / sqrtf(len2);
            c->z[p] = c->depth[p] / (float)c->hits[p];
            float v = 0.0f;
            if (t->moments && n >= 2) {
                const float S1 = t->moments[2 * p], S2 = t->moments[2 * p + 1];
                const float mean = S1 / (float)n;
                const float vs = fmaxf(0.0f, (S2 - S1 * mean) / (float)(n - 1));
                const float vm = vs / (float)n;
                const float dl = lum(c->d + 3 * p);
                v = vm / (dl * dl);
            }
            t->v[p] = v;
        }
}

/* after pass_moments (which leaves gz and the 3x3 luminance variance): var = the 3x3 Gaussian of v */
static void pass_gauss(ctx *c, int y0, int y1) {
    static const float k[2] = {1.0f / 2.0f, 1.0f / 4.0f};
    const counts *t = g_n;
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            if (c->hits[p] == 0) continue;
            float G = 0.0f, SV = 0.0f;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!hit(c, x + dx, y + dy)) continue;
                    const float g = k[abs(dx)] * k[abs(dy)];
                    G += g;
                    SV += g * t->v[(int64_t)(y + dy) * c->W + x + dx];
                }
            c->var[p] = SV / G;
        }
}

static void pass_remodulate_spp(ctx *c, int y0, int y1) {
    const counts *t = g_n;
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            for (int k = 0; k < 3; ++k)
                c->out[3 * p + k] = c->hits[p] == 0 ? c->fb[3 * p + k] : (c->L[3 * p + k] * c->d[3 * p + k]) * (float)t->spp[p];
        }
}

/* W x H pixels, row-major; fb, albedo, normal: 3 floats per pixel; depth, hits, spp: 1; moments: NULL or 2.  out: 3 floats per
 * pixel.  var_out: NULL, or 1 float per pixel that receives the second prepass's var (0 on pixels that are not hit pixels; only
 * with iterations > 0).  0 on success. */
int denoise_spp_reference(int W, int H, int A, int iterations, float sigma_depth, float sigma_luminance, int squarings, const float *fb,
                          const int32_t *spp, const float *moments, const float *albedo, const float *normal, const float *depth,
                          const uint32_t *hits, float *out, float *var_out, int threads) {
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    if (threads > H) threads = H;
    const size_t P = (size_t)W * (size_t)H;
    /* HIT pixels: hit_count > 0 and n >= 1 */
    uint32_t *hit_pixels = calloc(P, 4);
    if (!hit_pixels) return 1;
    for (size_t p = 0; p < P; ++p) hit_pixels[p] = spp[p] >= 1 ? hits[p] : 0;
    ctx c = {W, H, 0, iterations, squarings, sigma_depth, sigma_luminance, fb, albedo, normal, depth, hit_pixels, NULL, NULL, NULL, NULL,
             NULL, NULL, NULL, NULL, out, 0};
    c.L = calloc(3 * P, 4), c.L2 = calloc(3 * P, 4), c.d = calloc(3 * P, 4), c.n = calloc(3 * P, 4);
    c.var = calloc(P, 4), c.var2 = calloc(P, 4), c.z = calloc(P, 4), c.gz = calloc(P, 4);
    counts t = {spp, moments, A, calloc(P, 4)};
    if (!c.L || !c.L2 || !c.d || !c.n || !c.var || !c.var2 || !c.z || !c.gz || !t.v) return 1;
    g_n = &t;
    parallel(&c, threads, pass_prepass_spp);
    if (iterations > 0) {
        parallel(&c, threads, pass_moments);
        if (moments) parallel(&c, threads, pass_gauss);
        if (var_out) memcpy(var_out, c.var, 4 * P);
    }
    for (int i = 0; i < iterations; ++i) {
        c.step = 1 << i;
        parallel(&c, threads, pass_iterate);
        float *tmp = c.L; c.L = c.L2; c.L2 = tmp;
        tmp = c.var; c.var = c.var2; c.var2 = tmp;
    }
    parallel(&c, threads, pass_remodulate_spp);
    free(c.L), free(c.L2), free(c.d), free(c.n), free(c.var), free(c.var2), free(c.z), free(c.gz), free(t.v), free(hit_pixels);
    return 0;
}
