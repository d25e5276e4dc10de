/* aov_samples_ref.c — CPU restatement of rt_render_aov_samples's buffers (tests/test_denoise_temporal.py builds it with
 * oracle/rt_oracle.c, -ffp-contract=off like the oracle): aov_ref.c's per-sample rules for samples first … first + spp - 1 instead
 * of 0 … spp - 1.  For pixel (i, j) and sample s: seed = wang_hash(wang_hash(i * W + j) + s), the reference's camera ray
 * (orc_get_ray) and its first hit over Interval(0.001, 1e30) (orc_geom_hit_bvh); sums from 0 in sample order; prim is the hit of
 * sample `first`.  One thread: the frames it checks are small.
 */
#include <stdint.h>
#include <string.h>

#include "../../oracle/rt_oracle.h"

void aov_samples_reference(const rt_scene_desc *sc, const rt_camera_data *cam, int32_t first, float *albedo, float *normal, float *depth,
                           uint32_t *hits, int32_t *prim) {
    const int W = cam->image_width, H = cam->image_height;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) {
            const int64_t p = (int64_t)j * W + i;
            const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)W + (uint32_t)j);
            float alb[3] = {0, 0, 0}, nrm[3] = {0, 0, 0}, dep = 0;
            uint32_t n = 0;
            int32_t pr = -1;
            for (int s = first; s < first + cam->samples_per_pixel; ++s) {
                uint32_t seed = orc_wang_hash(base + (uint32_t)s);
                float o[3], d[3], rec9[9];
                orc_get_ray(cam, i, j, &seed, o, d);
                int32_t hit = 0, code = 0;
                orc_geom_hit_bvh(sc, 1, o, d, 0.001f, 1e30f, &hit, rec9, &code);
                if (!hit) {
                    for (int c = 0; c < 3; ++c) alb[c] += cam->background.e[c];
                    continue;
                }
                const int32_t pc = code >> 1, idx = pc >> 1;
                if (s == first) pr = pc;
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
                n++;
            }
            memcpy(albedo + 3 * p, alb, 12);
            memcpy(normal + 3 * p, nrm, 12);
            depth[p] = dep;
            hits[p] = n;
            prim[p] = pr;
        }
}
