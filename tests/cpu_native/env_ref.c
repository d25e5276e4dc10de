/* env_ref.c — CPU reference of rt_env / rt_render_env / rt_env_table / rt_env_lookup / rt_trace_samples_env (tests/env_reference.py
 * builds it on its own into a shared library, gcc -ffp-contract=off like the oracle).  The oracle's ray_color and hit_bvh are static:
 * this file includes oracle/rt_oracle.c to reach them.
 *
 * include/rtp_amd.h's image-based lighting contract, in its order: the path is ray_color's, draw for draw; a miss looks the
 * direction up in the octahedral map; at a diffuse event (LAMBERTIAN, METAL's hemisphere branch) with depth + 1 < max_depth one
 * light sample from the second stream, whose shadow ray contributes when the closest-hit search finds nothing; the miss of the BSDF
 * ray right after a diffuse event is weighted.
 */
#include "../../oracle/rt_oracle.c"
#include "../../include/rtp_amd.h"

#include <math.h>
#include <pthread.h>

typedef struct {
    int32_t n;
    int32_t empty;
    const float *rgb;     /* the caller's */
    float *row_cdf, *row_pmf, *col_cdf, *col_pmf;
} env_map;

static void decode_d(double u, double v, double p[3]) {
    const double y = (1.0 - fabs(u)) - fabs(v);
    p[1] = y;
    if (y >= 0.0) {
        p[0] = u;
        p[2] = v;
    } else {
        p[0] = (1.0 - fabs(v)) * (u >= 0.0 ? 1.0 : -1.0);
        p[2] = (1.0 - fabs(u)) * (v >= 0.0 ? 1.0 : -1.0);
    }
}
static float sg(float x) { return x >= 0.0f ? 1.0f : -1.0f; }
static v3 decode_f(float u, float v) {
    const float y = (1.0f - fabsf(u)) - fabsf(v);
    if (y >= 0.0f) return V(u, y, v);
    return V((1.0f - fabsf(v)) * sg(u), y, (1.0f - fabsf(u)) * sg(v));
}
static int32_t cell(float u, int32_t n) {
    const float t = ((u + 1.0f) * 0.5f) * (float)n;
    return t >= 0.0f ? (t < (float)n ? (int32_t)t : n - 1) : 0;
}
/* direction → octahedron point p and texel iy * n + ix */
static int32_t texel_of(v3 d, int32_t n, v3 *p) {
    const float s = (fabsf(d.e[0]) + fabsf(d.e[1])) + fabsf(d.e[2]);
    *p = V(d.e[0] / s, d.e[1] / s, d.e[2] / s);
    float u = p->e[0], v = p->e[2];
    if (!(p->e[1] >= 0.0f)) {
        u = (1.0f - fabsf(p->e[2])) * sg(p->e[0]);
        v = (1.0f - fabsf(p->e[0])) * sg(p->e[2]);
    }
    return cell(v, n) * n + cell(u, n);
}

/* the texel's weight: radiance x solid angle, in double */
double env_texel_weight(const float *rgb, int32_t n, int32_t ix, int32_t iy) {
    const double cellarea = (2.0 / (double)n) * (2.0 / (double)n);
    const double uc = -1.0 + (double)(2 * ix + 1) / (double)n, vc = -1.0 + (double)(2 * iy + 1) / (double)n;
    double p[3];
    decode_d(uc, vc, p);
    const double l2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
    const float *t = rgb + ((size_t)iy * n + ix) * 3;
    return (((double)t[0] + (double)t[1]) + (double)t[2]) * (cellarea / (l2 * sqrt(l2)));
}

static void cdf_of(const double *w, int32_t n, double total, float *cdf, float *pmf) {
    double run = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        run += w[k];
        cdf[k] = total > 0.0 ? (k + 1 == n ? 1.0f : (float)(run / total)) : 0.0f;
        pmf[k] = cdf[k] - (k == 0 ? 0.0f : cdf[k - 1]);
    }
}

/* The sampling table of the header into caller-made arrays (row_*: n, col_*: n * n).  Returns n, or 0 for an empty table. */
int32_t env_table(const float *rgb, int32_t n, float *row_cdf, float *row_pmf, float *col_cdf, float *col_pmf) {
    const size_t nn = (size_t)n * n;
    double *w = (double *)malloc(sizeof(double) * nn), *rw = (double *)malloc(sizeof(double) * (size_t)n);
    double total = 0.0;
    for (int32_t iy = 0; iy < n; ++iy) {
        double row = 0.0;
        for (int32_t ix = 0; ix < n; ++ix) {
            w[(size_t)iy * n + ix] = env_texel_weight(rgb, n, ix, iy);
            row += w[(size_t)iy * n + ix];
        }
        rw[iy] = row;
        total += row;
    }
    cdf_of(rw, n, total, row_cdf, row_pmf);
    for (int32_t iy = 0; iy < n; ++iy) cdf_of(w + (size_t)iy * n, n, total > 0.0 ? rw[iy] : 0.0, col_cdf + (size_t)iy * n, col_pmf + (size_t)iy * n);
    free(w);
    free(rw);
    return total > 0.0 ? n : 0;
}

static void make_map(const float *rgb, int32_t n, env_map *M) {
    const size_t nn = (size_t)n * n;
    M->n = n;
    M->rgb = rgb;
    M->row_cdf = (float *)malloc(4 * (size_t)n);
    M->row_pmf = (float *)malloc(4 * (size_t)n);
    M->col_cdf = (float *)malloc(4 * nn);
    M->col_pmf = (float *)malloc(4 * nn);
    M->empty = env_table(rgb, n, M->row_cdf, M->row_pmf, M->col_cdf, M->col_pmf) == 0;
}
static void free_map(env_map *M) { free(M->row_cdf); free(M->row_pmf); free(M->col_cdf); free(M->col_pmf); }

static float pj_of(const env_map *M, int32_t t) { return M->row_pmf[t / M->n] * M->col_pmf[t]; }
static float pl_of(const env_map *M, int32_t t, float q2, float q) {
    if (M->empty) return 0.0f;
    return (pj_of(M, t) * (((float)M->n * (float)M->n) * 0.25f)) * (q2 * q);
}

/* rt_env_lookup: count directions → texel, radiance, pl */
void env_lookup(const float *rgb, int32_t n, int64_t count, const float *dirs, int32_t *texel, float *rad, float *pl) {
    env_map M;
    make_map(rgb, n, &M);
    for (int64_t g = 0; g < count; ++g) {
        v3 p;
        const int32_t t = texel_of(V(dirs[3 * g], dirs[3 * g + 1], dirs[3 * g + 2]), n, &p);
        const float q2 = dot(p, p);
        texel[g] = t;
        memcpy(rad + 3 * g, rgb + 3 * (size_t)t, 12);
        pl[g] = pl_of(&M, t, q2, sqrtf(q2));
    }
    free_map(&M);
}
/* the unit direction of (u, v): decode, normalised (for the map tests) */
void env_decode(int64_t count, const float *uv, float *dirs) {
    for (int64_t g = 0; g < count; ++g) {
        const v3 p = decode_f(uv[2 * g], uv[2 * g + 1]);
        const float q = sqrtf(dot(p, p));
        dirs[3 * g] = p.e[0] / q; dirs[3 * g + 1] = p.e[1] / q; dirs[3 * g + 2] = p.e[2] / q;
    }
}

/* smallest e in [0, n) with u < cdf[e]; n when there is none */
static int32_t pick(const float *cdf, int32_t n, float u) {
    int32_t e = 0;
    while (e < n && !(u < cdf[e])) ++e;
    return e;
}
static int32_t pick_fast(const float *cdf, int32_t n, float u) {      /* (the cdf is monotone: the same entry by bisection) */
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

static v3 rotate(const rt_env_params *ep, v3 d) {
    return V(dot(V(ep->rot[0], ep->rot[1], ep->rot[2]), d), dot(V(ep->rot[3], ep->rot[4], ep->rot[5]), d), dot(V(ep->rot[6], ep->rot[7], ep->rot[8]), d));
}
static v3 scaled(const env_map *M, const rt_env_params *ep, int32_t t) {
    const float *c = M->rgb + 3 * (size_t)t;
    return V(ep->scale * c[0], ep->scale * c[1], ep->scale * c[2]);
}

/* one light sample at a vertex with normal n: 1 and the direction / contribution when it asks for a shadow ray */
static int env_sample(const env_map *M, const rt_env_params *ep, uint32_t *env, v3 n, v3 a, v3 beta, v3 *dir, v3 *c, int linear) {
    const float ua = orc_random_float(env);
    const int32_t iy = linear ? pick(M->row_cdf, M->n, ua) : pick_fast(M->row_cdf, M->n, ua);
    if (iy >= M->n) return 0;
    const float ub = orc_random_float(env);
    const float *cc = M->col_cdf + (size_t)iy * M->n;
    const int32_t ix = linear ? pick(cc, M->n, ub) : pick_fast(cc, M->n, ub);
    if (ix >= M->n) return 0;
    const float uc = orc_random_float(env);
    const float ud = orc_random_float(env);
    const float h = 2.0f / (float)M->n;
    const float u = ((float)ix + uc) * h - 1.0f;
    const float v = ((float)iy + ud) * h - 1.0f;
    const v3 p = decode_f(u, v);
    const float q2 = dot(p, p);
    const float q = sqrtf(q2);
    const v3 we = V(p.e[0] / q, p.e[1] / q, p.e[2] / q);
    for (int k = 0; k < 3; ++k) dir->e[k] = (ep->rot[k] * we.e[0] + ep->rot[3 + k] * we.e[1]) + ep->rot[6 + k] * we.e[2];
    if (!(dot(*dir, n) > 0.0f)) return 0;
    const int32_t t = iy * M->n + ix;
    const float pl = pl_of(M, t, q2, q);
    const float pb = RT_NEE_PB;
    const float f = ep->mode == 1 ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), scaled(M, ep, t)));
    return 1;
}

static v3 ray_color_env(ray r, uint32_t *seed, uint32_t *env, const rt_scene_desc *sc, const rt_camera_data *cam, const env_map *M,
                        const rt_env_params *ep, int32_t *rays_out, int linear) {
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0;
    int prev_diffuse = 0;
    const int sampled = ep->mode != 0 && !M->empty;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt = -1, pi = -1;
        nrays++;
        int h = sc->num_nodes > 0 ? hit_bvh(sc, &cur, 0.001f, 1e30f, &rec, &pt, &pi, NULL) : 0;
        if (!h) {
            if (depth == 0 && !ep->camera_visible) {
                final_color = add(final_color, mulv(beta, from_rt(cam->background)));
                break;
            }
            v3 p;
            const int32_t t = texel_of(rotate(ep, cur.d), M->n, &p);
            v3 term = mulv(beta, scaled(M, ep, t));
            if (prev_diffuse && sampled) {
                const float q2 = dot(p, p);
                const float pl = pl_of(M, t, q2, sqrtf(q2));
                const float pb = RT_NEE_PB;
                const float wb = ep->mode == 1 ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                term = scale(wb, term);
            }
            final_color = add(final_color, term);
            break;
        }
        const rt_material *mat = &sc->materials[rec.material_idx];
        v3 albedo = from_rt(mat->albedo);
        if (mat->texture_id != 0) {
            float tc[3];
            orc_tex2d(&sc->textures[mat->texture_id - 1], rec.u, rec.v, tc);
            albedo = mulv(albedo, V(tc[0], tc[1], tc[2]));
        }
        final_color = add(final_color, mulv(beta, from_rt(mat->emit)));
        ray scattered;
        v3 attenuation;
        int diffuse = 0, ok;
        if (mat->type == RT_MAT_LAMBERTIAN) {
            ok = scatter_diffuse(&rec, &attenuation, &scattered, seed, albedo);
            diffuse = 1;
        } else if (mat->type == RT_MAT_METAL) {
            if (orc_random_float(seed) < 0.8f) {
                v3 reflected = reflect(unit(cur.d), rec.normal);
                scattered.o = rec.point;
                scattered.d = add(reflected, scale(mat->fuzz, random_in_unit_sphere(seed)));
                attenuation = albedo;
                ok = dot(scattered.d, rec.normal) > 0;
            } else {
                ok = scatter_diffuse(&rec, &attenuation, &scattered, seed, albedo);
                diffuse = 1;
            }
        } else {
            ok = material_scatter(&cur, &rec, &attenuation, &scattered, seed, mat, albedo);
        }
        if (!ok) break;
        if (diffuse && depth + 1 < cam->max_depth && sampled) {
            ray shadow;
            v3 c;
            shadow.o = rec.point;
            if (env_sample(M, ep, env, rec.normal, albedo, beta, &shadow.d, &c, linear)) {
                nrays++;
                hitrec srec;
                int spt = -1, spi = -1;
                const int sh = sc->num_nodes > 0 ? hit_bvh(sc, &shadow, 0.001f, 1e30f, &srec, &spt, &spi, NULL) : 0;
                if (!sh) final_color = add(final_color, c);
            }
        }
        beta = mulv(beta, attenuation);
        cur = scattered;
        prev_diffuse = diffuse;
    }
    if (rays_out) *rays_out = nrays;
    return final_color;
}

/* M NULL: the oracle's ray_color (rt_render) */
static v3 sample_of(const rt_scene_desc *sc, const rt_camera_data *cam, const env_map *M, const rt_env_params *ep, int i, int j, int s,
                    int32_t *rays, uint32_t *seed_out, uint32_t *env_out, int linear) {
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    ray r = get_ray(cam, i, j, &seed);
    const v3 c = M ? ray_color_env(r, &seed, &env, sc, cam, M, ep, rays, linear) : ray_color(r, &seed, sc, cam, rays, NULL);
    if (seed_out) *seed_out = seed;
    if (env_out) *env_out = env;
    return c;
}

/* count samples (ijs: i, j, s) → radiance (3 floats), rays, final path seed and final light-sample seed.  Picks by linear scan: the
 * header's "smallest entry with u < cdf" literally (the frames below pick by bisection; tests compare the two). */
void env_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const float *rgb, int32_t n, const rt_env_params *ep, int64_t count,
               const int32_t *ijs, float *radiance, int32_t *rays, uint32_t *seeds, uint32_t *env_seeds, int32_t linear) {
    env_map M;
    make_map(rgb, n, &M);
    for (int64_t k = 0; k < count; ++k) {
        const v3 c = sample_of(sc, cam, &M, ep, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &rays[k], &seeds[k], &env_seeds[k], linear);
        memcpy(radiance + 3 * k, c.e, 12);
    }
    free_map(&M);
}

typedef struct {
    const rt_scene_desc *sc;
    const rt_camera_data *cam;
    const env_map *M;
    const rt_env_params *ep;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;          /* sums (nrows x W x 3), or NULL */
    double *mom;        /* per pixel: sum and sum of squares of each channel (6 doubles), or NULL */
} env_job;

static void *env_run(void *arg) {
    env_job *jb = (env_job *)arg;
    const int W = jb->cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double m[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + jb->cam->samples_per_pixel; ++s) {
                const v3 c = sample_of(jb->sc, jb->cam, jb->M, jb->ep, i, j, s, NULL, NULL, NULL, 0);
                pixel = add(pixel, c);
                for (int k = 0; k < 3; ++k) {
                    m[k] += c.e[k];
                    m[3 + k] += (double)c.e[k] * (double)c.e[k];
                }
            }
            if (jb->fb) memcpy(jb->fb + 3 * p, pixel.e, 12);
            if (jb->mom) memcpy(jb->mom + 6 * p, m, sizeof(m));
        }
    }
    return NULL;
}

/* The sums of samples sample_first … sample_first + spp - 1 of the listed image rows (in that order): fb (nrows x W x 3).  rgb NULL:
 * the oracle's ray_color (rt_render).  mom (may be NULL): per pixel the double sums and sums of squares of the three channels. */
void env_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const float *rgb, int32_t n, const rt_env_params *ep, const int32_t *rows,
               int nrows, int sample_first, int threads, float *fb, double *mom) {
    env_map M;
    if (rgb) make_map(rgb, n, &M);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    env_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        env_job jb = {sc, cam, rgb ? &M : NULL, ep, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, env_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    if (rgb) free_map(&M);
}
