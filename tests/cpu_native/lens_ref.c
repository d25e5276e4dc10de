/* lens_ref.c — CPU reference of rt_render_lens / rt_render_aov_lens / rt_lens_camera_rays (tests/lens_reference.py builds it on its
 * own into a shared library, gcc -ffp-contract=off like the oracle).  The oracle's ray_color is static: this file includes
 * oracle/rt_oracle.c to reach it.
 *
 * The camera ray of include/rtp_amd.h's contract, in its order: ox, oy as get_ray draws them; tau (cam_close != NULL); (lx, ly) by
 * rejection (lens_radius > 0); the pinhole ray (O, S - O), or with a lens (L, F - L).  Frames: ray_color behind it, samples summed in
 * sample order from 0.  AOVs: aov_ref.c's sums for the first hit of the same ray.
 */
#include "../../oracle/rt_oracle.c"

#include <math.h>
#include <pthread.h>

typedef struct {
    v3 o[2], p00[2], du[2], dv[2];
    float radius, focus;
    int motion;
} lens_cam;

static void lens_from(const rt_camera_data *open, const rt_camera_data *close, float radius, float focus, lens_cam *L) {
    const rt_camera_data *ends[2] = {open, close ? close : open};
    for (int e = 0; e < 2; ++e) {
        L->o[e] = from_rt(ends[e]->origin);
        L->p00[e] = from_rt(ends[e]->pixel00_loc);
        L->du[e] = from_rt(ends[e]->pixel_delta_u);
        L->dv[e] = from_rt(ends[e]->pixel_delta_v);
    }
    L->radius = radius;
    L->focus = focus;
    L->motion = close != NULL;
}

static v3 lerp3(v3 a, v3 b, float tau) { return add(a, scale(tau, sub(b, a))); }
static v3 div3(v3 v, float t) { return V(v.e[0] / t, v.e[1] / t, v.e[2] / t); }

/* the camera ray of (i, j) from *seed (the state after the per-sample hash); *seed is left after the camera's draws.  *tau_out: the
 * drawn time (0 without motion); lens_xy: the lens sample (0, 0 without a lens) */
static ray lens_ray(const lens_cam *L, int i, int j, uint32_t *seed, float *tau_out, float lens_xy[2]) {
    const float ox = orc_random_float(seed) - 0.5f;
    const float oy = orc_random_float(seed) - 0.5f;
    float tau = 0.0f;
    v3 O = L->o[0], P00 = L->p00[0], du = L->du[0], dv = L->dv[0];
    if (L->motion) {
        tau = orc_random_float(seed);
        O = lerp3(L->o[0], L->o[1], tau);
        P00 = lerp3(L->p00[0], L->p00[1], tau);
        du = lerp3(L->du[0], L->du[1], tau);
        dv = lerp3(L->dv[0], L->dv[1], tau);
    }
    float lx = 0.0f, ly = 0.0f;
    if (L->radius > 0.0f) {
        do {
            lx = random_range(seed, -1.0f, 1.0f);
            ly = random_range(seed, -1.0f, 1.0f);
        } while (lx * lx + ly * ly >= 1.0f);
    }
    const v3 S = add(add(add(add(P00, scale((float)i, du)), scale((float)j, dv)), scale(ox, du)), scale(oy, dv));
    ray r;
    r.o = O;
    r.d = sub(S, O);
    if (L->radius > 0.0f) {
        const v3 n = cross(du, dv);
        const float dimg = fabsf(dot(sub(P00, O), n)) / sqrtf(dot(n, n));
        const float k = L->focus / dimg;
        const v3 F = add(O, scale(k, r.d));
        const v3 uh = div3(du, sqrtf(dot(du, du))), vh = div3(dv, sqrtf(dot(dv, dv)));
        const v3 Lp = add(add(O, scale(L->radius * lx, uh)), scale(L->radius * ly, vh));
        r.o = Lp;
        r.d = sub(F, Lp);
    }
    if (tau_out) *tau_out = tau;
    if (lens_xy) { lens_xy[0] = lx; lens_xy[1] = ly; }
    return r;
}

/* n samples (ijs: i, j, s) → origins, directions (3 floats each), final seeds, tau and the lens sample (lx, ly) */
void lens_rays(const rt_camera_data *open, const rt_camera_data *close, float radius, float focus, int64_t n, const int32_t *ijs,
               float *origins, float *dirs, uint32_t *seeds, float *taus, float *lens_xy) {
    lens_cam L;
    lens_from(open, close, radius, focus, &L);
    for (int64_t k = 0; k < n; ++k) {
        const int i = ijs[3 * k], j = ijs[3 * k + 1], s = ijs[3 * k + 2];
        uint32_t seed = orc_wang_hash(orc_wang_hash((uint32_t)i * (uint32_t)open->image_width + (uint32_t)j) + (uint32_t)s);
        const ray r = lens_ray(&L, i, j, &seed, taus ? &taus[k] : NULL, lens_xy ? &lens_xy[2 * k] : NULL);
        memcpy(origins + 3 * k, r.o.e, 12);
        memcpy(dirs + 3 * k, r.d.e, 12);
        seeds[k] = seed;
    }
}

typedef struct {
    const rt_scene_desc *sc;
    const rt_camera_data *cam;
    const lens_cam *L;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads, aov;
    float *fb, *albedo, *normal, *depth;
    uint32_t *hits;
    int32_t *prim;
} lens_job;

static void *lens_run(void *arg) {
    lens_job *jb = (lens_job *)arg;
    const rt_camera_data *cam = jb->cam;
    const rt_scene_desc *sc = jb->sc;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)W + (uint32_t)j);
            v3 pixel = V(0, 0, 0);
            float alb[3] = {0, 0, 0}, nrm[3] = {0, 0, 0}, dep = 0;
            uint32_t hits = 0;
            int32_t prim = -1;
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                uint32_t seed = orc_wang_hash(base + (uint32_t)s);
                const ray rr = lens_ray(jb->L, i, j, &seed, NULL, NULL);
                if (!jb->aov) {
                    pixel = add(pixel, ray_color(rr, &seed, sc, cam, NULL, NULL));
                    continue;
                }
                float rec9[9];
                int32_t hit = 0, code = 0;
                orc_geom_hit_bvh(sc, 1, rr.o.e, rr.d.e, 0.001f, 1e30f, &hit, rec9, &code);
                if (!hit) {
                    for (int c = 0; c < 3; ++c) alb[c] += cam->background.e[c];
                    continue;
                }
                const int32_t pc = code >> 1, idx = pc >> 1;
                if (s == jb->sample_first) prim = pc;
                const int32_t mi = (pc & 1) ? sc->planes[idx].material_idx : sc->spheres[idx].material_idx;
                const rt_material *m = &sc->materials[mi];
                float a[3] = {1, 1, 1};
                if (m->type == RT_MAT_LAMBERTIAN || m->type == RT_MAT_METAL) {
                    for (int c = 0; c < 3; ++c) a[c] = m->albedo.e[c];
                    if (m->texture_id != 0) {
                        float texel[3];
                        orc_tex2d(&sc->textures[m->texture_id - 1], rec9[7], rec9[8], texel);
                        for (int c = 0; c < 3; ++c) a[c] = a[c] * texel[c];
                    }
                }
                for (int c = 0; c < 3; ++c) {
                    alb[c] += a[c];
                    nrm[c] += rec9[4 + c];
                }
                dep += rec9[0];
                hits++;
            }
            if (!jb->aov) {
                memcpy(jb->fb + 3 * p, pixel.e, 12);
            } else {
                memcpy(jb->albedo + 3 * p, alb, 12);
                memcpy(jb->normal + 3 * p, nrm, 12);
                jb->depth[p] = dep;
                jb->hits[p] = hits;
                jb->prim[p] = prim;
            }
        }
    }
    return NULL;
}

static void lens_run_all(lens_job proto, int threads) {
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    lens_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        jobs[k] = proto;
        jobs[k].tid = k;
        jobs[k].nthreads = threads;
        pthread_create(&tid[k], NULL, lens_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
}

/* The sums of samples sample_first … sample_first + spp - 1 of the listed image rows (in that order): fb (nrows x W x 3) */
void lens_frame(const rt_scene_desc *sc, const rt_camera_data *open, const rt_camera_data *close, float radius, float focus,
                const int32_t *rows, int nrows, int sample_first, int threads, float *fb) {
    lens_cam L;
    lens_from(open, close, radius, focus, &L);
    lens_job proto = {sc, open, &L, rows, nrows, sample_first, 0, 1, 0, fb, NULL, NULL, NULL, NULL, NULL};
    lens_run_all(proto, threads);
}

/* … and the AOV sums of the same rays' first hits */
void lens_aov(const rt_scene_desc *sc, const rt_camera_data *open, const rt_camera_data *close, float radius, float focus,
              const int32_t *rows, int nrows, int sample_first, int threads, float *albedo, float *normal, float *depth, uint32_t *hits,
              int32_t *prim) {
    lens_cam L;
    lens_from(open, close, radius, focus, &L);
    lens_job proto = {sc, open, &L, rows, nrows, sample_first, 0, 1, 1, NULL, albedo, normal, depth, hits, prim};
    lens_run_all(proto, threads);
}
