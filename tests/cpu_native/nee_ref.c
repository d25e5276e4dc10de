/* nee_ref.c — CPU reference of rt_render_nee / rt_nee_light_table / rt_trace_samples_nee (tests/nee_reference.py builds it on its own
 * into a shared library, gcc -ffp-contract=off like the oracle).  The oracle's ray_color and hit_bvh are static: this file includes
 * oracle/rt_oracle.c to reach them.
 *
 * include/rtp_amd.h's next-event estimation contract, in its order: the path is ray_color's, draw for draw; at a diffuse event
 * (LAMBERTIAN, METAL's hemisphere branch) with depth + 1 < max_depth one light sample from the second stream; the BSDF hit of a
 * table sphere right after a diffuse event has its emission weighted.
 */
#include "../../oracle/rt_oracle.c"
#include "../../include/rtp_amd.h"

#include <math.h>
#include <pthread.h>

typedef struct {
    int32_t *index;
    float *cdf, *pmf;
    int32_t count;
    int32_t mis;
} nee_tab;

/* the emitter table of the header: spheres in order, w = (e0 + e1 + e2) r^2 in double, cdf narrowed (last 1), pmf = cdf difference */
int32_t nee_table(const rt_scene_desc *sc, int32_t *index, float *cdf, float *pmf) {
    int32_t n = 0;
    double total = 0.0;
    double *w = (double *)malloc(sizeof(double) * (size_t)(sc->num_spheres > 0 ? sc->num_spheres : 1));
    for (int32_t i = 0; i < sc->num_spheres; ++i) {
        const rt_sphere *s = &sc->spheres[i];
        const int32_t m = s->material_idx;
        if (!(s->radius > 0.0f) || m < 0 || m >= sc->num_materials) continue;
        const float *e = sc->materials[m].emit.e;
        int ok = 1, lit = 0;
        for (int c = 0; c < 3; ++c) {
            if (!(isfinite(e[c]) && e[c] >= 0.0f)) ok = 0;
            if (e[c] > 0.0f) lit = 1;
        }
        if (!ok || !lit) continue;
        index[n] = i;
        w[n] = ((double)e[0] + (double)e[1] + (double)e[2]) * ((double)s->radius * (double)s->radius);
        total += w[n];
        ++n;
    }
    double run = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        run += w[k];
        cdf[k] = k + 1 == n ? 1.0f : (float)(run / total);
        pmf[k] = cdf[k] - (k == 0 ? 0.0f : cdf[k - 1]);
    }
    free(w);
    return n;
}

static int nee_find(const nee_tab *T, int32_t sphere) {
    for (int32_t k = 0; k < T->count; ++k)
        if (T->index[k] == sphere) return k;
    return -1;
}
/* step 2: 0 = no contribution */
static int nee_cone(v3 x, const rt_sphere *s, v3 *w, float *d2, float *om) {
    *w = sub(from_rt(s->center), x);
    *d2 = dot(*w, *w);
    const float rr = s->radius * s->radius;
    if (!(*d2 > rr)) return 0;
    const float cos_max = sqrtf(1.0f - rr / *d2);
    *om = 1.0f - cos_max;
    return *om > 0.0f;
}
static float pdf_cone(float om) { return 1.0f / (RT_NEE_TWO_PI * om); }

/* one light sample at x: 1 and the sphere index / contribution when it asks for a shadow ray */
static int nee_sample(const rt_scene_desc *sc, const nee_tab *T, uint32_t *nee, v3 x, v3 n, v3 a, v3 beta, ray *shadow, int32_t *sphere_out, v3 *c) {
    const float u = orc_random_float(nee);
    int32_t e = 0;
    while (e < T->count && !(u < T->cdf[e])) ++e;
    if (e >= T->count) return 0;
    const int32_t sphere = T->index[e];
    v3 w;
    float d2, om;
    if (!nee_cone(x, &sc->spheres[sphere], &w, &d2, &om)) return 0;
    const float u1 = orc_random_float(nee);
    const float cos_t = 1.0f - u1 * om;
    const float sin_t = sqrtf(fmaxf(0.0f, 1.0f - cos_t * cos_t));
    float px, py, q2;
    do {
        px = random_range(nee, -1.0f, 1.0f);
        py = random_range(nee, -1.0f, 1.0f);
        q2 = px * px + py * py;
    } while (q2 >= 1.0f || q2 == 0.0f);
    const float q = sqrtf(q2);
    const float cx = px / q, cy = py / q;
    const float len = sqrtf(d2);
    const v3 wn = V(w.e[0] / len, w.e[1] / len, w.e[2] / len);
    const float sg = copysignf(1.0f, wn.e[2]);
    const float ba = -1.0f / (sg + wn.e[2]);
    const float bb = (wn.e[0] * wn.e[1]) * ba;
    const v3 t1 = V(1.0f + ((sg * wn.e[0]) * wn.e[0]) * ba, sg * bb, -sg * wn.e[0]);
    const v3 t2 = V(bb, sg + (wn.e[1] * wn.e[1]) * ba, -wn.e[1]);
    const float sx = sin_t * cx, sy = sin_t * cy;
    v3 dir;
    for (int k = 0; k < 3; ++k) dir.e[k] = (t1.e[k] * sx + t2.e[k] * sy) + wn.e[k] * cos_t;
    if (!(dot(dir, n) > 0.0f)) return 0;
    const float pl = T->pmf[e] * pdf_cone(om);
    const float pb = RT_NEE_PB;
    const float f = T->mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    const v3 emit = from_rt(sc->materials[sc->spheres[sphere].material_idx].emit);
    *c = scale(f, mulv(mulv(beta, a), emit));
    shadow->o = x;
    shadow->d = dir;
    *sphere_out = sphere;
    return 1;
}

static v3 ray_color_nee(ray r, uint32_t *seed, uint32_t *nee, const rt_scene_desc *sc, const rt_camera_data *cam, const nee_tab *T,
                        int32_t *rays_out) {
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0;
    int prev_diffuse = 0;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt = -1, pi = -1;
        nrays++;
        int h = sc->num_nodes > 0 ? hit_bvh(sc, &cur, 0.001f, 1e30f, &rec, &pt, &pi, NULL) : 0;
        if (!h) {
            final_color = add(final_color, mulv(beta, from_rt(cam->background)));
            break;
        }
        const rt_material *mat = &sc->materials[rec.material_idx];
        v3 albedo = from_rt(mat->albedo);
        if (mat->texture_id != 0) {
            float tc[3];
            orc_tex2d(&sc->textures[mat->texture_id - 1], rec.u, rec.v, tc);
            albedo = mulv(albedo, V(tc[0], tc[1], tc[2]));
        }
        v3 emitted = mulv(beta, from_rt(mat->emit));
        if (prev_diffuse && pt == 0) {
            const int e = nee_find(T, pi);
            if (e >= 0) {
                v3 w;
                float d2, om, pl = 0.0f;
                if (nee_cone(cur.o, &sc->spheres[pi], &w, &d2, &om)) pl = T->pmf[e] * pdf_cone(om);
                const float pb = RT_NEE_PB;
                const float wb = T->mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                emitted = scale(wb, emitted);
            }
        }
        final_color = add(final_color, emitted);
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
        if (diffuse && depth + 1 < cam->max_depth && T->count > 0) {
            ray shadow;
            int32_t sphere;
            v3 c;
            if (nee_sample(sc, T, nee, rec.point, rec.normal, albedo, beta, &shadow, &sphere, &c)) {
                nrays++;
                hitrec srec;
                int spt = -1, spi = -1;
                if (hit_bvh(sc, &shadow, 0.001f, 1e30f, &srec, &spt, &spi, NULL) && spt == 0 && spi == sphere) final_color = add(final_color, c);
            }
        }
        beta = mulv(beta, attenuation);
        cur = scattered;
        prev_diffuse = diffuse;
    }
    if (rays_out) *rays_out = nrays;
    return final_color;
}

static void make_tab(const rt_scene_desc *sc, int32_t mis, nee_tab *T) {
    const size_t n = (size_t)(sc->num_spheres > 0 ? sc->num_spheres : 1);
    T->index = (int32_t *)malloc(n * sizeof(int32_t));
    T->cdf = (float *)malloc(n * sizeof(float));
    T->pmf = (float *)malloc(n * sizeof(float));
    T->count = nee_table(sc, T->index, T->cdf, T->pmf);
    T->mis = mis;
}
static void free_tab(nee_tab *T) { free(T->index); free(T->cdf); free(T->pmf); }

/* mode: 0 / 1 = rt_render_nee with mis = mode; -1 = the oracle's ray_color (rt_render) */
static v3 sample_of(const rt_scene_desc *sc, const rt_camera_data *cam, const nee_tab *T, int mode, int i, int j, int s, int32_t *rays,
                    uint32_t *seed_out, uint32_t *nee_out) {
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    ray r = get_ray(cam, i, j, &seed);
    const v3 c = mode < 0 ? ray_color(r, &seed, sc, cam, rays, NULL) : ray_color_nee(r, &seed, &nee, sc, cam, T, rays);
    if (seed_out) *seed_out = seed;
    if (nee_out) *nee_out = nee;
    return c;
}

/* n samples (ijs: i, j, s) → radiance (3 floats), rays, final path seed and final light-sample seed */
void nee_trace(const rt_scene_desc *sc, const rt_camera_data *cam, int32_t mis, int64_t n, const int32_t *ijs, float *radiance, int32_t *rays,
               uint32_t *seeds, uint32_t *nee_seeds) {
    nee_tab T;
    make_tab(sc, mis, &T);
    for (int64_t k = 0; k < n; ++k) {
        const v3 c = sample_of(sc, cam, &T, mis, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &rays[k], &seeds[k], &nee_seeds[k]);
        memcpy(radiance + 3 * k, c.e, 12);
    }
    free_tab(&T);
}

typedef struct {
    const rt_scene_desc *sc;
    const rt_camera_data *cam;
    const nee_tab *T;
    const int32_t *rows;
    int nrows, sample_first, mode, tid, nthreads;
    float *fb;          /* sums (nrows x W x 3), or NULL */
    double *mom;        /* per pixel: sum and sum of squares of each channel (6 doubles), or NULL */
} nee_job;

static void *nee_run(void *arg) {
    nee_job *jb = (nee_job *)arg;
    const int W = jb->cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double m[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + jb->cam->samples_per_pixel; ++s) {
                const v3 c = sample_of(jb->sc, jb->cam, jb->T, jb->mode, i, j, s, NULL, NULL, NULL);
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

static void nee_run_all(nee_job proto, int threads) {
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    nee_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        jobs[k] = proto;
        jobs[k].tid = k;
        jobs[k].nthreads = threads;
        pthread_create(&tid[k], NULL, nee_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
}

/* The sums of samples sample_first … sample_first + spp - 1 of the listed image rows (in that order): fb (nrows x W x 3).  mode as
 * sample_of; mom (may be NULL): per pixel the double sums and sums of squares of the three channels. */
void nee_frame(const rt_scene_desc *sc, const rt_camera_data *cam, int32_t mode, const int32_t *rows, int nrows, int sample_first, int threads,
               float *fb, double *mom) {
    nee_tab T;
    make_tab(sc, mode < 0 ? 1 : mode, &T);
    nee_job proto = {sc, cam, &T, rows, nrows, sample_first, mode, 0, 1, fb, mom};
    nee_run_all(proto, threads);
    free_tab(&T);
}
