/* aov_ref.c — CPU reference of rt_render_aov's buffers (tests/aov_reference.py builds it together with oracle/rt_oracle.c into a
 * shared library, -ffp-contract=off like the oracle itself).
 *
 * For every listed pixel (i, j) and sample s in sample order: seed = wang_hash(wang_hash(i * W + j) + s), the reference's camera
 * ray get_ray(i, j, seed) (orc_get_ray), its first hit hit_scene over Interval(0.001, 1e30) (orc_geom_hit_bvh: rec9 = t, point,
 * normal, u, v), and the sums of include/rtp_amd.h's contract: albedo (m.albedo x tex2D_cpu(u, v) for a textured LAMBERTIAN or
 * METAL material, 1 for DIELECTRIC and DIFFUSE_LIGHT, the background on a miss), the face-forwarded normal, t, the hit count,
 * and the primitive code of sample 0.  Self-check: every ray's orc_geom_hit_bvh result is also orc_closest_hit's (hit or not,
 * t to the bit, primitive) — *mismatches counts the rays where they part.
 */
#include <pthread.h>
#include <stdint.h>
#include <string.h>

#include "../../oracle/rt_oracle.h"

typedef struct {
    const rt_scene_desc *sc;
    const rt_camera_data *cam;
    const int32_t *ij;
    int64_t first, last;
    float *albedo, *normal, *depth;
    uint32_t *hits;
    int32_t *prim;
    int64_t mismatches;
} job;

static void *run(void *arg) {
    job *jb = (job *)arg;
    const rt_scene_desc *sc = jb->sc;
    const rt_camera_data *cam = jb->cam;
    for (int64_t p = jb->first; p < jb->last; ++p) {
        const int i = jb->ij[2 * p], j = jb->ij[2 * p + 1];
        const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)cam->image_width + (uint32_t)j);
        float alb[3] = {0, 0, 0}, nrm[3] = {0, 0, 0}, dep = 0;
        uint32_t hits = 0;
        int32_t prim = -1;
        for (int s = 0; s < cam->samples_per_pixel; ++s) {
            uint32_t seed = orc_wang_hash(base + (uint32_t)s);
            float o[3], d[3], rec9[9];
            orc_get_ray(cam, i, j, &seed, o, d);
            int32_t hit = 0, code = 0;
            orc_geom_hit_bvh(sc, 1, o, d, 0.001f, 1e30f, &hit, rec9, &code);
            float t2 = 0;
            int type = -1, index = -1;
            const int hit2 = sc->num_nodes > 0 ? orc_closest_hit(sc, o, d, &t2, &type, &index) : 0;
            if (hit2 != hit || (hit && (memcmp(&t2, &rec9[0], 4) != 0 || 2 * index + type != (code >> 1)))) jb->mismatches++;
            if (!hit) {
                for (int c = 0; c < 3; ++c) alb[c] += cam->background.e[c];
                continue;
            }
            const int32_t pc = code >> 1, idx = pc >> 1;
            if (s == 0) prim = pc;
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
        memcpy(jb->albedo + 3 * p, alb, 12);
        memcpy(jb->normal + 3 * p, nrm, 12);
        jb->depth[p] = dep;
        jb->hits[p] = hits;
        jb->prim[p] = prim;
    }
    return NULL;
}

/* n pixels (ij: 2 n ints, column then row) → their AOVs.  Returns the self-check's mismatch count. */
int64_t aov_reference(const rt_scene_desc *sc, const rt_camera_data *cam, int64_t n, const int32_t *ij, int threads, float *albedo, float *normal,
                      float *depth, uint32_t *hits, int32_t *prim) {
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        jobs[k] = (job){sc, cam, ij, n * k / threads, n * (k + 1) / threads, albedo, normal, depth, hits, prim, 0};
        pthread_create(&tid[k], NULL, run, &jobs[k]);
    }
    int64_t mismatches = 0;
    for (int k = 0; k < threads; ++k) {
        pthread_join(tid[k], NULL);
        mismatches += jobs[k].mismatches;
    }
    return mismatches;
}
