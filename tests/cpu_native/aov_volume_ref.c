/* aov_volume_ref.c — CPU reference of rt_render_aov_volume (include/rtp_amd.h, "AOVs under fog").
 * tests/aov_volume_reference.py builds it on its own into a shared library (gcc -ffp-contract=off like the oracle).  It includes
 * volume_ref.c — and through it medium_ref.c, gloss_ref.c, tree_ref.c, emit_ref.c and oracle/rt_oracle.c — and only reads them: the lens
 * camera's ray (emit_ref.c's camera_ray_of, rt_render_lens's steps as the lit restatements state them; lens_ref.c states the same ray
 * a second time, but includes the oracle itself, so both cannot stand in one translation unit — tests/test_aov_volume.py holds this file
 * against lens_reference.aov where the contract says they are equal), the first hit (orc_geom_hit_bvh), the interval (med_interval) and the
 * cell walk (vol_walk, once for acc and once for the flight: the two recurrences the header allows one loop to carry).  The sample's
 * contribution is written here from the header's words.
 */
#include "volume_ref.c"

typedef struct {
    const rt_scene_desc *sc;
    const rt_camera_data *cam;
    const volume_cfg *cfg;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *albedo, *normal, *depth, *tr;
    uint32_t *hits;
    int32_t *prim;
} aovv_job;

static void *aovv_run(void *arg) {
    aovv_job *jb = (aovv_job *)arg;
    const rt_camera_data *cam = jb->cam;
    const rt_scene_desc *sc = jb->sc;
    const lit_cfg *lc = &jb->cfg->base.base.base.base;
    const rt_medium_params *m = &jb->cfg->base.medium;
    volume_ctx Vc;
    memset(&Vc, 0, sizeof(Vc));
    Vc.Mc.m = *m;
    Vc.rho = jb->cfg->rho;
    Vc.n[0] = jb->cfg->nx;
    Vc.n[1] = jb->cfg->ny;
    Vc.n[2] = jb->cfg->nz;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)W + (uint32_t)j);
            float alb[3] = {0, 0, 0}, nrm[3] = {0, 0, 0}, dep = 0, trs = 0;
            uint32_t hits = 0;
            int32_t prim = -1;
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                uint32_t seed = orc_wang_hash(base + (uint32_t)s);
                const ray rr = camera_ray_of(cam, lc, i, j, &seed);
                /* 1. the first hit: rt_render_aov's */
                float rec9[9];
                int32_t hit = 0, code = 0;
                orc_geom_hit_bvh(sc, 1, rr.o.e, rr.d.e, 0.001f, 1e30f, &hit, rec9, &code);
                float a[3], n[3] = {0, 0, 0}, t_hit = INFINITY;
                for (int c = 0; c < 3; ++c) a[c] = cam->background.e[c];
                if (hit) {
                    const int32_t pc = code >> 1, idx = pc >> 1;
                    if (s == jb->sample_first) prim = pc;
                    const int32_t mi = (pc & 1) ? sc->planes[idx].material_idx : sc->spheres[idx].material_idx;
                    const rt_material *mt = &sc->materials[mi];
                    for (int c = 0; c < 3; ++c) a[c] = 1.0f;
                    if (mt->type == RT_MAT_LAMBERTIAN || mt->type == RT_MAT_METAL) {
                        for (int c = 0; c < 3; ++c) a[c] = mt->albedo.e[c];
                        if (mt->texture_id != 0) {
                            float texel[3];
                            orc_tex2d(&sc->textures[mt->texture_id - 1], rec9[7], rec9[8], texel);
                            for (int c = 0; c < 3; ++c) a[c] = a[c] * texel[c];
                        }
                    }
                    for (int c = 0; c < 3; ++c) n[c] = rec9[4 + c];
                    t_hit = rec9[0];
                }
                /* 2. the medium on the camera ray */
                int covered = 0;
                float Tr = 1.0f, F = 0.0f, t_fog = 0.0f;
                float t0, t1;
                if (m->sigma_t > 0.0f && med_interval(m, rr.o, rr.d, t_hit, &t0, &t1, NULL)) {
                    const float ln = sqrtf(lensq(rr.d));
                    float tau;
                    int32_t cells = 0;
                    if (Vc.rho) {
                        tau = 0.0f;
                        vol_walk(&Vc, 0, rr.o, rr.d, t0, t1, ln, &tau, &cells, NULL);
                    } else {
                        tau = m->sigma_t * ((t1 - t0) * ln);
                    }
                    Tr = expf(-tau);
                    F = 1.0f - Tr;
                    if (F != 0.0f) {
                        covered = 1;
                        t_fog = t1;
                        if (Vc.rho) {
                            float v = RT_AOV_FOG_REM;
                            if (vol_walk(&Vc, 1, rr.o, rr.d, t0, t1, ln, &v, &cells, NULL)) t_fog = v;
                        } else {
                            const float sd = RT_AOV_FOG_REM / m->sigma_t;
                            if (sd < (t1 - t0) * ln) t_fog = t0 + sd / ln;
                        }
                    }
                }
                if (!covered) { /* 3. clear: rt_render_aov_lens's sample */
                    for (int c = 0; c < 3; ++c) alb[c] += a[c];
                    if (hit) {
                        for (int c = 0; c < 3; ++c) nrm[c] += n[c];
                        dep += t_hit;
                        hits++;
                    }
                    trs += 1.0f;
                    continue;
                }
                /* 4. covered */
                const v3 ud = unit(rr.d);
                for (int c = 0; c < 3; ++c) alb[c] += Tr * a[c] + F * m->albedo[c];
                if (hit) {
                    for (int c = 0; c < 3; ++c) nrm[c] += Tr * n[c] - F * ud.e[c];
                    dep += Tr * t_hit + F * t_fog;
                } else {
                    for (int c = 0; c < 3; ++c) nrm[c] += -(F * ud.e[c]);
                    dep += t_fog;
                }
                hits++;
                trs += Tr;
            }
            memcpy(jb->albedo + 3 * p, alb, 12);
            memcpy(jb->normal + 3 * p, nrm, 12);
            jb->depth[p] = dep;
            jb->hits[p] = hits;
            jb->prim[p] = prim;
            jb->tr[p] = trs;
        }
    }
    return NULL;
}

/* The sums of samples sample_first … sample_first + spp - 1 of the listed image rows (in that order).  Of cfg only the camera (cam_close,
 * the lens), the medium and the grid are read */
void aov_volume(const rt_scene_desc *sc, const rt_camera_data *cam, const volume_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads,
                float *albedo, float *normal, float *depth, uint32_t *hits, int32_t *prim, float *tr) {
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    aovv_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        aovv_job jb = {sc, cam, cfg, rows, nrows, sample_first, k, threads, albedo, normal, depth, tr, hits, prim};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, aovv_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
}
