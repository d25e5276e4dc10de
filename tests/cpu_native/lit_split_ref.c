/* lit_split_ref.c — CPU reference of rt_render_lit_split / rt_trace_samples_lit_split (tests/lit_split_reference.py builds it on its own
 * into a shared library, like lit_ref.c, which it includes for the tables, the light samples and the camera: the sample is
 * rt_render_lit's, draw for draw).
 *
 * include/rtp_amd.h's contract for direct and indirect light in separate frames, restated from its words: a path has a stage — 0 no
 * diffuse event yet, 1 the last vertex was the path's first diffuse event, 2 crossed; the vertex that the ray leaving the first diffuse
 * event finds adds its emission or miss term while still in stage 1, and immediately after that add the path crosses; what was added
 * before the crossing is direct, what is added after it — from zero — is indirect.
 */
#include "lit_ref.c"

typedef struct {
    v3 direct, indirect;
} split_rad;

/* ray_color_lit with the sum kept in two parts: `sum` is the component the path is adding to */
static split_rad ray_color_split(const lit_ctx *X, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, int32_t *rays_out) {
    const rt_scene_desc *sc = X->sc;
    const rt_camera_data *cam = X->cam;
    const rt_env_params *ep = X->cfg->ep;
    const int emitters_on = X->T->count > 0;
    const int sky_sampled = X->M && ep->mode != 0 && !X->M->empty;
    const float pb = RT_NEE_PB;
    split_rad out;
    out.direct = V(0.0f, 0.0f, 0.0f);
    out.indirect = V(0.0f, 0.0f, 0.0f);
    v3 sum = V(0.0f, 0.0f, 0.0f);
    int stage = 0;
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0;
    int prev_diffuse = 0;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt, pi;
        nrays++;
        const int hit = closest(sc, &cur, &rec, &pt, &pi);
        const rt_material *mat = NULL;
        v3 albedo = V(0.0f, 0.0f, 0.0f);
        /* the emission or miss term */
        v3 term;
        if (!hit) {
            if (!X->M || (depth == 0 && !ep->camera_visible)) {
                term = mulv(beta, from_rt(cam->background));
            } else {
                v3 p;
                const int32_t t = texel_of(to_env(ep, cur.d), X->M->n, &p);
                term = mulv(beta, scaled(X->M, ep, t));
                if (prev_diffuse && sky_sampled) {
                    const float q2 = dot(p, p);
                    const float pl = pl_of(X->M, t, q2, sqrtf(q2));
                    const float wb = ep->mode == 1 ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                    term = scale(wb, term);
                }
            }
        } else {
            mat = &sc->materials[rec.material_idx];
            albedo = from_rt(mat->albedo);
            if (mat->texture_id != 0) {
                float tc[3];
                orc_tex2d(&sc->textures[mat->texture_id - 1], rec.u, rec.v, tc);
                albedo = mulv(albedo, V(tc[0], tc[1], tc[2]));
            }
            term = mulv(beta, from_rt(mat->emit));
            if (prev_diffuse && pt == 0 && emitters_on) {
                const int e = tab_find(X->T, pi);
                if (e >= 0) {
                    v3 w;
                    float d2, om, pl = 0.0f;
                    if (cone_of(cur.o, &sc->spheres[pi], &w, &d2, &om)) pl = X->T->pmf[e] * pdf_cone(om);
                    const float wb = X->T->mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                    term = scale(wb, term);
                }
            }
        }
        sum = add(sum, term);
        /* the vertex that the first diffuse event's ray found has added its term: the path crosses */
        if (stage == 1) {
            out.direct = sum;
            sum = V(0.0f, 0.0f, 0.0f);
            stage = 2;
        }
        if (!hit) break;
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
        if (stage == 0 && diffuse) stage = 1;
        if (diffuse && depth + 1 < cam->max_depth) {
            hitrec srec;
            int spt, spi;
            ray shadow;
            v3 c;
            shadow.o = rec.point;
            int32_t sphere;
            if (emitters_on && emitter_sample(sc, X->T, nee, rec.point, rec.normal, albedo, beta, &shadow.d, &sphere, &c)) {
                nrays++;
                if (closest(sc, &shadow, &srec, &spt, &spi) && spt == 0 && spi == sphere) sum = add(sum, c);
            }
            if (sky_sampled && sky_sample(X->M, ep, env, rec.normal, albedo, beta, &shadow.d, &c, X->linear)) {
                nrays++;
                if (!closest(sc, &shadow, &srec, &spt, &spi)) sum = add(sum, c);
            }
        }
        beta = mulv(beta, attenuation);
        cur = scattered;
        prev_diffuse = diffuse;
    }
    if (stage == 2) out.indirect = sum;
    else out.direct = sum;
    if (rays_out) *rays_out = nrays;
    return out;
}

static split_rad split_sample_of(const lit_ctx *X, int i, int j, int s, int32_t *rays, uint32_t *seed_out, uint32_t *nee_out, uint32_t *env_out) {
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const split_rad c = ray_color_split(X, r, &seed, &nee, &env, rays);
    if (seed_out) *seed_out = seed;
    if (nee_out) *nee_out = nee;
    if (env_out) *env_out = env;
    return c;
}

/* lit_trace with two radiance outputs */
void lit_split_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const lit_cfg *cfg, int64_t count, const int32_t *ijs, float *direct,
                     float *indirect, int32_t *rays, uint32_t *seeds, uint32_t *nee_seeds, uint32_t *env_seeds, int32_t linear) {
    emit_tab T;
    sky_map M;
    lit_ctx X;
    make_ctx(sc, cam, cfg, &T, &M, linear, &X);
    for (int64_t k = 0; k < count; ++k) {
        const split_rad c = split_sample_of(&X, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &rays[k], &seeds[k], &nee_seeds[k], &env_seeds[k]);
        memcpy(direct + 3 * k, c.direct.e, 12);
        memcpy(indirect + 3 * k, c.indirect.e, 12);
    }
    free_ctx(cfg, &T, &M);
}

typedef struct {
    const lit_ctx *X;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *direct, *indirect;
} split_job;

static void *split_run(void *arg) {
    split_job *jb = (split_job *)arg;
    const rt_camera_data *cam = jb->X->cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 a = V(0, 0, 0), b = V(0, 0, 0);
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const split_rad c = split_sample_of(jb->X, i, j, s, NULL, NULL, NULL, NULL);
                a = add(a, c.direct);
                b = add(b, c.indirect);
            }
            memcpy(jb->direct + 3 * p, a.e, 12);
            memcpy(jb->indirect + 3 * p, b.e, 12);
        }
    }
    return NULL;
}

/* lit_frame with two outputs: each component's sum over the samples, strictly in sample order */
void lit_split_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const lit_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads,
                     float *direct, float *indirect) {
    emit_tab T;
    sky_map M;
    lit_ctx X;
    make_ctx(sc, cam, cfg, &T, &M, 0, &X);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    split_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        split_job jb = {&X, rows, nrows, sample_first, k, threads, direct, indirect};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, split_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_ctx(cfg, &T, &M);
}
