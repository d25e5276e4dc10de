/* denoise_ref.c — CPU restatement of rt_denoise's arithmetic as include/rtp_amd.h states it ("denoising"), for the bit-exact
 * comparisons of tests/test_denoise.py (tests/denoise_reference.py builds it: gcc -ffp-contract=off -fno-fast-math, like the
 * oracle).  Written from the header's contract, not from the kernels: plain arrays per quantity, libm's expf, every pass over
 * the whole image before the next one starts.  Threads split the rows of each pass; every pixel is computed on its own.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int W, H, S, iterations, squarings;
    float sigma_depth, sigma_luminance;
    const float *fb, *albedo, *normal, *depth;
    const uint32_t *hits;
    float *L, *var, *d, *n, *z, *gz, *L2, *var2, *out;  /* per pixel: L 3, var 1, d 3, n 3, z 1, gz 1 */
    int step;                                           /* current iteration's step (pass_iterate) */
} ctx;

typedef struct {
    ctx *c;
    int y0, y1;
    void (*pass)(ctx *, int, int);
} job;

static float lum(const float *L) { return (0.2126f * L[0] + 0.7152f * L[1]) + 0.0722f * L[2]; }
static int hit(const ctx *c, int x, int y) { return x >= 0 && x < c->W && y >= 0 && y < c->H && c->hits[(int64_t)y * c->W + x] > 0; }

static void pass_prepass(ctx *c, int y0, int y1) {
    const float inv = (float)(1.0 / (double)c->S);
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            if (c->hits[p] == 0) continue;
            for (int k = 0; k < 3; ++k) {
                const float cc = c->fb[3 * p + k] * inv;
                const float a = c->albedo[3 * p + k] * inv;
                c->d[3 * p + k] = fmaxf(a, 1e-3f);
                c->L[3 * p + k] = cc / c->d[3 * p + k];
            }
            const float *N = c->normal + 3 * p;
            const float len2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
            for (int k = 0; k < 3; ++k) c->n[3 * p + k] = len2 == 0.0f ? 0.0f : N[k] / sqrtf(len2);
            c->z[p] = c->depth[p] / (float)c->hits[p];
        }
}

static void pass_moments(ctx *c, int y0, int y1) {
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            if (c->hits[p] == 0) continue;
            float m1 = 0.0f, m2 = 0.0f, k = 0.0f;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!hit(c, x + dx, y + dy)) continue;
                    const float l = lum(c->L + 3 * ((int64_t)(y + dy) * c->W + x + dx));
                    m1 += l;
                    m2 += l * l;
                    k += 1.0f;
                }
            c->var[p] = fmaxf(0.0f, m2 / k - (m1 / k) * (m1 / k));
            float g[2];
            for (int axis = 0; axis < 2; ++axis) {
                const int ax = axis == 0, ay = axis == 1;
                const int has_next = hit(c, x + ax, y + ay), has_prev = hit(c, x - ax, y - ay);
                const float next = has_next ? fabsf(c->z[(int64_t)(y + ay) * c->W + x + ax] - c->z[p]) : INFINITY;
                const float prev = has_prev ? fabsf(c->z[p] - c->z[(int64_t)(y - ay) * c->W + x - ax]) : INFINITY;
                g[axis] = (!has_next && !has_prev) ? 0.0f : fminf(next, prev);
            }
            c->gz[p] = g[0] + g[1];
        }
}

static void pass_iterate(ctx *c, int y0, int y1) {
    static const float kern[3] = {3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const int s = c->step;
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            if (c->hits[p] == 0) continue;
            const float lp = lum(c->L + 3 * p);
            const float rl = 1.0f / (c->sigma_luminance * sqrtf(c->var[p]) + 1e-4f);
            float rz[5];
            for (int m = 0; m < 5; ++m) rz[m] = 1.0f / ((c->sigma_depth * c->gz[p]) * (float)(s * m) + 1e-4f);
            float W = 0.0f, SL[3] = {0.0f, 0.0f, 0.0f}, SV = 0.0f;
            for (int dy = -2; dy <= 2; ++dy)
                for (int dx = -2; dx <= 2; ++dx) {
                    const int qx = x + s * dx, qy = y + s * dy;
                    if (!hit(c, qx, qy)) continue;
                    const int64_t q = (int64_t)qy * c->W + qx;
                    const float h = kern[abs(dx)] * kern[abs(dy)];
                    const float *np = c->n + 3 * p, *nq = c->n + 3 * q;
                    float wn = fmaxf(0.0f, (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2]);
                    for (int k = 0; k < c->squarings; ++k) wn = wn * wn;
                    const float e = fabsf(c->z[p] - c->z[q]) * rz[abs(dx) + abs(dy)] + fabsf(lp - lum(c->L + 3 * q)) * rl;
                    const float w = (h * wn) * expf(-e);
                    W += w;
                    for (int k = 0; k < 3; ++k) SL[k] += w * c->L[3 * q + k];
                    SV += (w * w) * c->var[q];
                }
            for (int k = 0; k < 3; ++k) c->L2[3 * p + k] = W == 0.0f ? c->L[3 * p + k] : SL[k] / W;
            c->var2[p] = W == 0.0f ? c->var[p] : SV / (W * W);
        }
}

static void pass_remodulate(ctx *c, int y0, int y1) {
    for (int y = y0; y < y1; ++y)
        for (int x = 0; x < c->W; ++x) {
            const int64_t p = (int64_t)y * c->W + x;
            for (int k = 0; k < 3; ++k)
                c->out[3 * p + k] = c->hits[p] == 0 ? c->fb[3 * p + k] : (c->L[3 * p + k] * c->d[3 * p + k]) * (float)c->S;
        }
}

static void *run(void *arg) {
    job *j = (job *)arg;
    j->pass(j->c, j->y0, j->y1);
    return NULL;
}

static void parallel(ctx *c, int threads, void (*pass)(ctx *, int, int)) {
    job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        jobs[k] = (job){c, (int)((int64_t)c->H * k / threads), (int)((int64_t)c->H * (k + 1) / threads), pass};
        pthread_create(&tid[k], NULL, run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
}

/* W x H pixels, row-major; fb, albedo, normal: 3 floats per pixel; depth: 1; hits: 1.  out: 3 floats per pixel.  0 on success. */
int denoise_reference(int W, int H, int S, int iterations, float sigma_depth, float sigma_luminance, int squarings, const float *fb,
                      const float *albedo, const float *normal, const float *depth, const uint32_t *hits, float *out, int threads) {
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    if (threads > H) threads = H;
    const size_t P = (size_t)W * (size_t)H;
    ctx c = {W, H, S, iterations, squarings, sigma_depth, sigma_luminance, fb, albedo, normal, depth, hits, NULL, NULL, NULL, NULL,
             NULL, NULL, NULL, NULL, out, 0};
    c.L = calloc(3 * P, 4), c.L2 = calloc(3 * P, 4), c.d = calloc(3 * P, 4), c.n = calloc(3 * P, 4);
    c.var = calloc(P, 4), c.var2 = calloc(P, 4), c.z = calloc(P, 4), c.gz = calloc(P, 4);
    if (!c.L || !c.L2 || !c.d || !c.n || !c.var || !c.var2 || !c.z || !c.gz) return 1;
    parallel(&c, threads, pass_prepass);
    if (iterations > 0) parallel(&c, threads, pass_moments);
    for (int i = 0; i < iterations; ++i) {
        c.step = 1 << i;
        parallel(&c, threads, pass_iterate);
        float *t = c.L; c.L = c.L2; c.L2 = t;
        t = c.var; c.var = c.var2; c.var2 = t;
    }
    parallel(&c, threads, pass_remodulate);
    free(c.L), free(c.L2), free(c.d), free(c.n), free(c.var), free(c.var2), free(c.z), free(c.gz);
    return 0;
}
