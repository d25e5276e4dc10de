/* gloss_ref.c — CPU reference of the glossy switch of rt_render_nee / rt_render_env / rt_render_lit (rt_nee_params.glossy,
 * rt_env_params.glossy; include/rtp_amd.h, "glossy = 1").  tests/gloss_reference.py builds it on its own into a shared
 * library (gcc -ffp-contract=off like the oracle).  It includes tree_ref.c — and through it emit_ref.c and oracle/rt_oracle.c — for the
 * tables, the cone, the plane point, the tree, the map and the camera; the vertex loop and the two light samples are written here from
 * the header's words, because the existing ones have pb fixed at RT_NEE_PB.
 *
 * The path is ray_color's draw for draw.  A METAL hit whose branch draw chose the reflect branch is a glossy event when its fuzz is at
 * least RT_GLOSSY_MIN_FUZZ, the next query is inside max_depth and a light is on with its switch at 1: it takes that light's sample with
 * pb = pg(wl) — whether or not the path's own direction is absorbed — and the ray that leaves it carries pg(unit(new_d)).
 */
#include "tree_ref.c"

/* what a call is made of (tests/gloss_reference.py mirrors this struct) */
typedef struct {
    tree_cfg base;
    int32_t glossy_nee, glossy_env;
} gloss_cfg;

/* per-sample tallies, in this order (gloss_trace's counters: 6 int32 per sample) */
enum {
    GC_SAMPLES,        /* glossy events: vertices that took their light samples as one */
    GC_ABSORBED,       /* those whose path direction was absorbed */
    GC_PG_ZERO,        /* light samples at glossy events whose pg was 0 */
    GC_FUZZ_GT1,       /* glossy events at fuzz > 1 */
    GC_HIT_CARRIED,    /* emitter hits weighted by a carried pg */
    GC_MISS_CARRIED,   /* misses weighted by a carried pg */
    GC_COUNT
};

/* pg of the header, in its float32 order */
static float gloss_pg(v3 w, v3 r, float fuzz) {
    const float c = dot(w, r);
    const float ff = fuzz * fuzz;
    const float disc = (c * c - 1.0f) + ff;
    if (!(disc > 0.0f)) return 0.0f;
    const float s = sqrtf(disc);
    const float t2 = c + s;
    if (!(t2 > 0.0f)) return 0.0f;
    const float t1 = c - s;
    const float f3 = ff * fuzz;
    if (t1 > 0.0f) return (s * (3.0f * (c * c) + s * s)) / (RT_NEE_TWO_PI * f3);
    return ((t2 * t2) * t2) / ((2.0f * RT_NEE_TWO_PI) * f3);
}

/* the BSDF strategy's density in a sampled direction: RT_NEE_PB at a diffuse event, pg about r at a glossy one */
typedef struct {
    int glossy;
    v3 r;
    float fuzz;
} bsdf_pb;
static float pb_of(const bsdf_pb *B, v3 w) { return B->glossy ? gloss_pg(w, B->r, B->fuzz) : RT_NEE_PB; }

/* What a light sample or a found-side weight went through, per vertex (tests/light_vertex_cases.py): the tallies below as
 * bits, and the two densities the weight was made of.  The path loops pass NULL.  A note only counts: nothing is computed from it */
enum {
    TL_INSIDE = 1 << 0,       /* cone refused: the vertex is inside or on the sphere, !(d2 > rr) */
    TL_OM_ZERO = 1 << 1,      /* cone refused: om == 0, 1 - rr / d2 rounded to 1 */
    TL_HEMISPHERE = 1 << 2,   /* hemisphere refused: !(dot(dir, n) > 0) */
    TL_PB_ZERO = 1 << 3,      /* pb == 0 refused */
    TL_FELL = 1 << 4,         /* fallback taken: a node's q stood in for the importances */
    TL_FOLDED = 1 << 5,       /* triangle folded: ua + ub > 1 */
    TL_NO_ENTRY = 1 << 6,     /* no entry: the pick returned the table's length */
    TL_PL2_INF = 1 << 7,      /* pl * pl overflows */
    TL_COS_SMALL = 1 << 8,    /* plane refused: cos_l < 1e-8 */
    TL_D2_ZERO = 1 << 9,      /* plane refused: the point drawn is the vertex */
    TL_ELLIPSE4 = 1 << 10,    /* the ellipse's rejection loop took four rounds or more */
    TL_OK = 1 << 11,          /* a shadow ray is asked for */
    TL_WEIGHTED = 1 << 12,    /* found side: the primitive is a table entry and the weight was applied */
    TL_PL_ZERO = 1 << 13,     /* found side: weighted with pl == 0 (inside the sphere, in the plane, om == 0) */
    TL_NOT_TABLE = 1 << 14,   /* found side: the primitive is no table entry */
    TL_Z_ZERO = 1 << 15,      /* Duff's basis around a wn with wn.z == +-0 */
    TL_AXIS = 1 << 16,        /* Duff's basis around a wn with wn.x == wn.y == 0 */
    TL_OM_ULP = 1 << 17,      /* the cone's om is 2^-24, the last value before 0 */
    TL_CARRY_OFF = 1 << 18,   /* found side: the carried value is "none" (0 or -0) */
    TL_C_NAN = 1 << 19,       /* the contribution or the weight holds a NaN */
    TL_SUM_ONE = 1 << 20,     /* a triangle's draw with ua + ub == 1 exactly: the last sum that is not folded */
    TL_COUNT = 21
};
typedef struct {
    uint32_t flags;
    float pl, pb;
} vtx_note;

/* steps 2 to 4 / 2p to 4p for the picked entry e (tree_ref.c's entry_sample with pb by the event): 1 = a shadow ray is asked for.
 * *pg_zero is set when the sample stopped at pb == 0; note (may be NULL) takes the tallies */
static int entry_sample_note(const rt_scene_desc *sc, const emit_tab *T, int32_t e, float pmf, uint32_t *nee, v3 x, v3 n, v3 a, v3 beta, const bsdf_pb *B,
                             v3 *dir, v3 *c, int *pg_zero, vtx_note *note) {
    float pl;
    v3 emit;
    if (T->kind[e] == 1) {
        const rt_plane *p = &sc->planes[T->index[e]];
        float ua, ub;
        if (p->type == RT_PLANE_ELLIPSE) {
            float px, py, q2;
            int rounds = 0;
            do {
                px = -1.0f + 2.0f * orc_random_float(nee);
                py = -1.0f + 2.0f * orc_random_float(nee);
                q2 = px * px + py * py;
                ++rounds;
            } while (q2 >= 1.0f);
            if (note && rounds >= 4) note->flags |= TL_ELLIPSE4;
            ua = 0.5f + 0.5f * px;
            ub = 0.5f + 0.5f * py;
        } else {
            ua = orc_random_float(nee);
            ub = orc_random_float(nee);
            if (note && p->type == RT_PLANE_TRIANGLE && ua + ub == 1.0f) note->flags |= TL_SUM_ONE;
            if (p->type == RT_PLANE_TRIANGLE && ua + ub > 1.0f) {
                ua = 1.0f - ua;
                ub = 1.0f - ub;
                if (note) note->flags |= TL_FOLDED;
            }
        }
        v3 y;
        for (int k = 0; k < 3; ++k) y.e[k] = (p->base.e[k] + ua * p->u.e[k]) + ub * p->v.e[k];
        float pa;
        if (!plane_pa(x, y, p, T->area[e], dir, &pa)) {
            const v3 xy = sub(y, x);
            if (note) note->flags |= dot(xy, xy) > 0.0f ? TL_COS_SMALL : TL_D2_ZERO;      /* (plane_pa's other refusal is d2 == 0) */
            return 0;
        }
        if (!(dot(*dir, n) > 0.0f)) {
            if (note) note->flags |= TL_HEMISPHERE;
            return 0;
        }
        pl = pmf * pa;
        emit = from_rt(sc->materials[p->material_idx].emit);
    } else {
        const rt_sphere *s = &sc->spheres[T->index[e]];
        v3 w;
        float d2, om;
        if (!cone_of(x, s, &w, &d2, &om)) {
            if (note) note->flags |= d2 > s->radius * s->radius ? TL_OM_ZERO : TL_INSIDE;
            return 0;
        }
        if (note && om == 0x1p-24f) note->flags |= TL_OM_ULP;
        const float u1 = orc_random_float(nee);
        const float cos_t = 1.0f - u1 * om;
        const float sin_t = sqrtf(fmaxf(0.0f, 1.0f - cos_t * cos_t));
        float px, py, q2;
        do {
            px = -1.0f + 2.0f * orc_random_float(nee);
            py = -1.0f + 2.0f * orc_random_float(nee);
            q2 = px * px + py * py;
        } while (q2 >= 1.0f || q2 == 0.0f);
        const float q = sqrtf(q2);
        const float cx = px / q, cy = py / q;
        const float len = sqrtf(d2);
        const v3 wn = V(w.e[0] / len, w.e[1] / len, w.e[2] / len);
        if (note && wn.e[2] == 0.0f) note->flags |= TL_Z_ZERO;
        if (note && wn.e[0] == 0.0f && wn.e[1] == 0.0f) note->flags |= TL_AXIS;
        const float sg = copysignf(1.0f, wn.e[2]);
        const float ba = -1.0f / (sg + wn.e[2]);
        const float bb = (wn.e[0] * wn.e[1]) * ba;
        const v3 t1 = V(1.0f + ((sg * wn.e[0]) * wn.e[0]) * ba, sg * bb, -sg * wn.e[0]);
        const v3 t2 = V(bb, sg + (wn.e[1] * wn.e[1]) * ba, -wn.e[1]);
        const float sx = sin_t * cx, sy = sin_t * cy;
        for (int k = 0; k < 3; ++k) dir->e[k] = (t1.e[k] * sx + t2.e[k] * sy) + wn.e[k] * cos_t;
        if (!(dot(*dir, n) > 0.0f)) {
            if (note) note->flags |= TL_HEMISPHERE;
            return 0;
        }
        pl = pmf * pdf_cone(om);
        emit = from_rt(sc->materials[s->material_idx].emit);
    }
    const float pb = pb_of(B, *dir);
    if (B->glossy && pb == 0.0f) {
        *pg_zero = 1;
        if (note) note->flags |= TL_PB_ZERO;
        return 0;
    }
    const float f = T->mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), emit));
    if (note) {
        note->flags |= TL_OK | (isinf(pl * pl) ? TL_PL2_INF : 0);
        note->pl = pl;
        note->pb = pb;
    }
    return 1;
}
static int entry_sample_pb(const rt_scene_desc *sc, const emit_tab *T, int32_t e, float pmf, uint32_t *nee, v3 x, v3 n, v3 a, v3 beta, const bsdf_pb *B,
                           v3 *dir, v3 *c, int *pg_zero) {
    return entry_sample_note(sc, T, e, pmf, nee, x, n, a, beta, B, dir, c, pg_zero, NULL);
}

/* rt_render_env's steps 1 … 4 up to the shadow ray (emit_ref.c's sky_sample with pb by the event) */
static int sky_sample_note(const sky_map *M, const rt_env_params *ep, uint32_t *env, v3 n, v3 a, v3 beta, const bsdf_pb *B, v3 *dir, v3 *c, int linear,
                           int *pg_zero, vtx_note *note) {
    const float ua = orc_random_float(env);
    const int32_t iy = pick(M->row_cdf, M->n, ua, linear);
    if (iy >= M->n) {
        if (note) note->flags |= TL_NO_ENTRY;
        return 0;
    }
    const float ub = orc_random_float(env);
    const int32_t ix = pick(M->col_cdf + (size_t)iy * M->n, M->n, ub, linear);
    if (ix >= M->n) {
        if (note) note->flags |= TL_NO_ENTRY;
        return 0;
    }
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
    if (!(dot(*dir, n) > 0.0f)) {
        if (note) note->flags |= TL_HEMISPHERE;
        return 0;
    }
    const float pb = pb_of(B, *dir);
    if (B->glossy && pb == 0.0f) {
        *pg_zero = 1;
        if (note) note->flags |= TL_PB_ZERO;
        return 0;
    }
    const int32_t t = iy * M->n + ix;
    const float pl = pl_of(M, t, q2, q);
    const float f = ep->mode == 1 ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), scaled(M, ep, t)));
    if (note) {
        note->flags |= TL_OK | (isinf(pl * pl) ? TL_PL2_INF : 0);
        note->pl = pl;
        note->pb = pb;
    }
    return 1;
}
static int sky_sample_pb(const sky_map *M, const rt_env_params *ep, uint32_t *env, v3 n, v3 a, v3 beta, const bsdf_pb *B, v3 *dir, v3 *c, int linear,
                         int *pg_zero) {
    return sky_sample_note(M, ep, env, n, a, beta, B, dir, c, linear, pg_zero, NULL);
}

/* The found side's weights, as the path below applies them.  A BSDF ray from o whose closest hit is table entry e (a sphere: pt = 0, a
 * plane: pt = 1, index pi, at `point`), left with the density pb: the weight of what it found */
static float found_hit_weight(const rt_scene_desc *sc, const emit_tab *T, const light_tree *tree, int select, int e, int pt, int pi, v3 o, v3 point, float pb,
                              vtx_note *note) {
    v3 w;
    float d2, om, pa, pl = 0.0f;
    if (pt == 1) {
        if (plane_pa(o, point, &sc->planes[pi], T->area[e], &w, &pa)) pl = (select ? tree_pmf(tree, e, o, NULL) : T->pmf[e]) * pa;
    } else if (cone_of(o, &sc->spheres[pi], &w, &d2, &om))
        pl = (select ? tree_pmf(tree, e, o, NULL) : T->pmf[e]) * pdf_cone(om);
    if (note) {
        note->flags |= TL_WEIGHTED | (pl == 0.0f ? TL_PL_ZERO : 0) | (isinf(pl * pl) ? TL_PL2_INF : 0);
        note->pl = pl;
        note->pb = pb;
    }
    return T->mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
}
/* … and of a miss into texel t of the map (p: the direction's octahedron point), left with the density pb */
static float found_miss_weight(const sky_map *M, const rt_env_params *ep, int32_t t, v3 p, float pb, vtx_note *note) {
    const float q2 = dot(p, p);
    const float pl = pl_of(M, t, q2, sqrtf(q2));
    if (note) {
        note->flags |= TL_WEIGHTED | (pl == 0.0f ? TL_PL_ZERO : 0) | (isinf(pl * pl) ? TL_PL2_INF : 0);
        note->pl = pl;
        note->pb = pb;
    }
    return ep->mode == 1 ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
}

typedef struct {
    tree_ctx Y;
    int32_t glossy_nee, glossy_env;
} gloss_ctx;

/* the path.  carried: 0 none, 1 a diffuse event (pb = RT_NEE_PB), 2 a glossy event (pb = carry_pg, against the lights whose switch is 1) */
static v3 ray_color_gloss(const gloss_ctx *G, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, int32_t *rays_out, int32_t *cnt) {
    const tree_ctx *Y = &G->Y;
    const lit_ctx *X = &Y->X;
    const rt_scene_desc *sc = X->sc;
    const rt_camera_data *cam = X->cam;
    const rt_env_params *ep = X->cfg->ep;
    const emit_tab *T = X->T;
    const int emitters_on = T->count > 0;
    const int sky_sampled = X->M && ep->mode != 0 && !X->M->empty;
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0;
    int carried = 0;
    float carry_pg = 0.0f;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt, pi;
        nrays++;
        if (!closest(sc, &cur, &rec, &pt, &pi)) {
            if (!X->M || (depth == 0 && !ep->camera_visible)) {
                final_color = add(final_color, mulv(beta, from_rt(cam->background)));
                break;
            }
            v3 p;
            const int32_t t = texel_of(to_env(ep, cur.d), X->M->n, &p);
            v3 term = mulv(beta, scaled(X->M, ep, t));
            /* weighted after a diffuse event, or after a glossy one when the environment's switch is on and pg did not round to 0 */
            const int weighted = carried == 1 || (carried == 2 && G->glossy_env && carry_pg != 0.0f);
            if (weighted && sky_sampled) {
                const float pb = carried == 1 ? RT_NEE_PB : carry_pg;
                term = scale(found_miss_weight(X->M, ep, t, p, pb, NULL), term);
                if (carried == 2 && cnt) cnt[GC_MISS_CARRIED]++;
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
        v3 emitted = mulv(beta, from_rt(mat->emit));
        const int hit_weighted = carried == 1 || (carried == 2 && G->glossy_nee && carry_pg != 0.0f);
        if (hit_weighted && (pt == 0 || pt == 1) && emitters_on) {
            const int e = tab_find(T, pt, pi);
            if (e >= 0) {
                const float pb = carried == 1 ? RT_NEE_PB : carry_pg;
                emitted = scale(found_hit_weight(sc, T, Y->tree, Y->select, e, pt, pi, cur.o, rec.point, pb, NULL), emitted);
                if (carried == 2 && cnt) cnt[GC_HIT_CARRIED]++;
            }
        }
        final_color = add(final_color, emitted);
        ray scattered;
        v3 attenuation;
        int event = 0, ok;                 /* event: 1 diffuse, 2 METAL's reflect branch */
        v3 reflected = V(0, 0, 0);
        if (mat->type == RT_MAT_LAMBERTIAN) {
            ok = scatter_diffuse(&rec, &attenuation, &scattered, seed, albedo);
            event = 1;
        } else if (mat->type == RT_MAT_METAL) {
            if (orc_random_float(seed) < 0.8f) {
                reflected = reflect(unit(cur.d), rec.normal);
                scattered.o = rec.point;
                scattered.d = add(reflected, scale(mat->fuzz, random_in_unit_sphere(seed)));
                attenuation = albedo;
                ok = dot(scattered.d, rec.normal) > 0;
                event = 2;
            } else {
                ok = scatter_diffuse(&rec, &attenuation, &scattered, seed, albedo);
                event = 1;
            }
        } else {
            ok = material_scatter(&cur, &rec, &attenuation, &scattered, seed, mat, albedo);
        }
        /* which lights sample here?  A diffuse event that goes on: each light that is on.  A reflect branch — absorbed or not — with
         * fuzz >= RT_GLOSSY_MIN_FUZZ: each light that is on with its switch at 1 */
        int take_nee = 0, take_env = 0;
        bsdf_pb B;
        B.glossy = 0;
        B.r = reflected;
        B.fuzz = mat->fuzz;
        if (depth + 1 < cam->max_depth) {
            if (event == 1 && ok) {
                take_nee = emitters_on;
                take_env = sky_sampled;
            } else if (event == 2 && mat->fuzz >= RT_GLOSSY_MIN_FUZZ) {
                take_nee = emitters_on && G->glossy_nee;
                take_env = sky_sampled && G->glossy_env;
                B.glossy = 1;
            }
        }
        const int glossy_event = B.glossy && (take_nee || take_env);
        if (glossy_event && cnt) {
            cnt[GC_SAMPLES]++;
            if (!ok) cnt[GC_ABSORBED]++;
            if (mat->fuzz > 1.0f) cnt[GC_FUZZ_GT1]++;
        }
        if (take_nee || take_env) {
            hitrec srec;
            int spt, spi;
            ray shadow;
            v3 c;
            shadow.o = rec.point;
            if (take_nee) {
                int32_t e;
                float pmf = 0.0f;
                if (Y->select) {
                    e = tree_pick(Y->tree, nee, rec.point, &pmf, NULL);
                } else {
                    const float u = orc_random_float(nee);
                    e = 0;
                    while (e < T->count && !(u < T->cdf[e])) ++e;
                    if (e < T->count) pmf = T->pmf[e];
                }
                int pg_zero = 0;
                if (e < T->count && entry_sample_pb(sc, T, e, pmf, nee, rec.point, rec.normal, albedo, beta, &B, &shadow.d, &c, &pg_zero)) {
                    nrays++;
                    const int hit = closest(sc, &shadow, &srec, &spt, &spi);
                    if (hit && spt == T->kind[e] && spi == T->index[e]) final_color = add(final_color, c);
                }
                if (pg_zero && cnt) cnt[GC_PG_ZERO]++;
            }
            if (take_env) {
                int pg_zero = 0;
                if (sky_sample_pb(X->M, ep, env, rec.normal, albedo, beta, &B, &shadow.d, &c, X->linear, &pg_zero)) {
                    nrays++;
                    if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, c);
                }
                if (pg_zero && cnt) cnt[GC_PG_ZERO]++;
            }
        }
        if (!ok) break;
        beta = mulv(beta, attenuation);
        cur = scattered;
        carried = event == 1 ? 1 : (glossy_event ? 2 : 0);
        carry_pg = glossy_event ? gloss_pg(unit(scattered.d), reflected, mat->fuzz) : 0.0f;
    }
    if (rays_out) *rays_out = nrays;
    return final_color;
}

static v3 gloss_sample_of(const gloss_ctx *G, int i, int j, int s, int32_t *rays, uint32_t *seed_out, uint32_t *nee_out, uint32_t *env_out, int32_t *cnt) {
    const lit_ctx *X = &G->Y.X;
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_gloss(G, r, &seed, &nee, &env, rays, cnt);
    if (seed_out) *seed_out = seed;
    if (nee_out) *nee_out = nee;
    if (env_out) *env_out = env;
    return c;
}

static void make_gloss_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const gloss_cfg *cfg, emit_tab *T, sky_map *M, light_tree *t, int linear,
                           gloss_ctx *G) {
    make_tree_ctx(sc, cam, &cfg->base, T, M, t, linear, &G->Y);
    G->glossy_nee = cfg->glossy_nee;
    G->glossy_env = cfg->glossy_env;
}

/* ---- what tests/gloss_reference.py calls -------------------------------------------------------------------------------------------- */
/* pg for count directions w about r (3 floats each) */
void gloss_pg_many(int64_t count, const float *w, const float *r, float fuzz, float *pg) {
    for (int64_t k = 0; k < count; ++k) pg[k] = gloss_pg(V(w[3 * k], w[3 * k + 1], w[3 * k + 2]), V(r[0], r[1], r[2]), fuzz);
}
/* count draws of the lobe about r from the stream that starts at seed: c = dot(unit(r + fuzz * in_sphere), r), in double */
void gloss_lobe_draws(int64_t count, const float *r, float fuzz, uint32_t seed, double *c) {
    const v3 R = V(r[0], r[1], r[2]);
    for (int64_t k = 0; k < count; ++k) {
        const v3 d = unit(add(R, scale(fuzz, random_in_unit_sphere(&seed))));
        c[k] = ((double)d.e[0] * R.e[0] + (double)d.e[1] * R.e[1]) + (double)d.e[2] * R.e[2];
    }
}

/* ---- per vertex (tests/light_vertex_cases.py): what the path above computes at one vertex, as the 16 words the developer
 * library's rt_debug_light_vertices writes for it ------------------------------------------------------------------------------------ */
static uint32_t word_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static void put3(uint32_t *w, v3 c, vtx_note *note) {
    for (int k = 0; k < 3; ++k) w[k] = word_of(c.e[k]);
    if (note && (isnan(c.e[0]) || isnan(c.e[1]) || isnan(c.e[2]))) note->flags |= TL_C_NAN;
}
/* step 1 of a light sample at x: by the descent (select = 1 on a table that is not empty) or by the cdf → the entry (the table's length:
 * none) and the probability of that pick */
static int32_t vertex_pick(const gloss_ctx *G, uint32_t *st, v3 x, float *pmf, vtx_note *note) {
    const emit_tab *T = G->Y.X.T;
    int32_t e = 0;
    *pmf = 0.0f;
    if (G->Y.select && T->count > 0) {
        int fell = 0;
        e = tree_pick(G->Y.tree, st, x, pmf, &fell);
        if (note && fell) note->flags |= TL_FELL;
    } else {
        const float u = orc_random_float(st);
        while (e < T->count && !(u < T->cdf[e])) ++e;
        if (e < T->count) *pmf = T->pmf[e];
    }
    if (note && !(e < T->count)) note->flags |= TL_NO_ENTRY;
    return e;
}
/* routine 0: the emitter table's light sample under pb_kind (0: RT_NEE_PB, 1: pg about r = v with fuzz = s) → ok, dir, c, the code of the
 *            primitive to reach, the stream's state after it;   1: the environment's → ok, dir, c, the state after it;
 *         2: the weighted emission of the ray (x, v) that found primitive code `seed` at closest = s, going in as beta * a — after a
 *            diffuse event, and carrying nv[0];   3: what the miss of a ray along v adds at depth 0 and 1 after a diffuse event, and at
 *            depth 1 and 0 carrying nv[0];   5: pg(w = x; r = v, fuzz = s).
 * flags (may be NULL: no tallies) takes the TL_ bits of each vertex, plpb (may be NULL) the two densities of its weight */
void gloss_vertices(const rt_scene_desc *sc, const rt_camera_data *cam, const gloss_cfg *cfg, int32_t routine, int32_t pb_kind, int64_t count, const float *x,
                    const float *nv, const float *v, const float *s, const uint32_t *seed, const float *ab, uint32_t *out, uint32_t *flags, float *plpb) {
    emit_tab T;
    sky_map M;
    light_tree t;
    gloss_ctx G;
    make_gloss_ctx(sc, cam, cfg, &T, &M, &t, 0, &G);
    const lit_ctx *X = &G.Y.X;
    const rt_env_params *ep = X->cfg->ep;
    const int sky_sampled = X->M && ep->mode != 0 && !X->M->empty;
    const v3 a = V(ab[0], ab[1], ab[2]), beta = V(ab[3], ab[4], ab[5]);
    memset(out, 0, (size_t)count * 64);
    for (int64_t k = 0; k < count; ++k) {
        const v3 xk = V(x[3 * k], x[3 * k + 1], x[3 * k + 2]), nk = V(nv[3 * k], nv[3 * k + 1], nv[3 * k + 2]), vk = V(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
        uint32_t *w = out + 16 * k;
        vtx_note note = {0u, 0.0f, 0.0f};
        vtx_note *N = (flags || plpb) ? &note : NULL;
        bsdf_pb B;
        B.glossy = pb_kind == 1;
        B.r = vk;
        B.fuzz = s[k];
        if (routine == 0 || (routine == 1 && X->M)) {
            uint32_t st = seed[k];
            v3 dir, c;
            int pg_zero = 0, ok;
            int32_t e = 0;
            if (routine == 0) {
                float pmf;
                e = vertex_pick(&G, &st, xk, &pmf, N);
                ok = e < T.count && entry_sample_note(sc, &T, e, pmf, &st, xk, nk, a, beta, &B, &dir, &c, &pg_zero, N);
            } else {
                ok = sky_sample_note(X->M, ep, &st, nk, a, beta, &B, &dir, &c, 0, &pg_zero, N);
            }
            if (ok) {
                w[0] = 1;
                put3(w + 1, dir, N);
                put3(w + 4, c, N);
                if (routine == 0) w[7] = (uint32_t)(2 * T.index[e] + T.kind[e]);
            }
            w[routine == 0 ? 8 : 7] = st;
        } else if (routine == 2) {
            const int32_t code = (int32_t)seed[k];
            const int pt = code & 1, pi = code >> 1;
            const v3 point = add(xk, scale(s[k], vk));
            for (int pass = 0; pass < 2; ++pass) {          /* the carried float first: the note keeps the diffuse event's densities */
                const float pb = pass == 0 ? nk.e[0] : RT_NEE_PB;
                v3 emitted = mulv(beta, a);
                if (pb != 0.0f && T.count > 0) {
                    const int e = tab_find(&T, pt, pi);
                    if (e >= 0) emitted = scale(found_hit_weight(sc, &T, G.Y.tree, G.Y.select, e, pt, pi, xk, point, pb, N), emitted);
                    else if (N) N->flags |= TL_NOT_TABLE;
                } else if (N) N->flags |= TL_CARRY_OFF;
                put3(w + (pass == 0 ? 3 : 0), emitted, N);
            }
        } else if (routine == 3 && X->M) {
            for (int pass = 0; pass < 4; ++pass) {          /* (depth 0, carried), (1, carried), (1, diffuse), (0, diffuse) */
                const int depth = pass == 1 || pass == 2;
                const float pb = pass < 2 ? nk.e[0] : RT_NEE_PB;
                v3 term;
                if (depth == 0 && !ep->camera_visible) {
                    term = mulv(beta, from_rt(cam->background));
                } else {
                    v3 p;
                    const int32_t tx = texel_of(to_env(ep, vk), X->M->n, &p);
                    term = mulv(beta, scaled(X->M, ep, tx));
                    if (pb != 0.0f && sky_sampled) term = scale(found_miss_weight(X->M, ep, tx, p, pb, N), term);
                    else if (N && pb == 0.0f) N->flags |= TL_CARRY_OFF;
                }
                put3(w + (pass == 0 ? 9 : (pass == 1 ? 6 : (pass == 2 ? 3 : 0))), term, N);
            }
        } else if (routine == 5) {
            w[0] = word_of(gloss_pg(xk, vk, s[k]));
        }
        if (flags) flags[k] = note.flags;
        if (plpb) {
            plpb[2 * k] = note.pl;
            plpb[2 * k + 1] = note.pb;
        }
    }
    free_tree(&t);
    free_ctx(&cfg->base.base, &T, &M);
}

/* count samples (ijs: i, j, s) → radiance, rays, the three final RNG states and the GC_COUNT tallies of each sample */
void gloss_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const gloss_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance, int32_t *rays,
                 uint32_t *seeds, uint32_t *nee_seeds, uint32_t *env_seeds, int32_t linear, int32_t *counters) {
    emit_tab T;
    sky_map M;
    light_tree t;
    gloss_ctx G;
    make_gloss_ctx(sc, cam, cfg, &T, &M, &t, linear, &G);
    memset(counters, 0, (size_t)count * GC_COUNT * sizeof(int32_t));
    for (int64_t k = 0; k < count; ++k) {
        const v3 c = gloss_sample_of(&G, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &rays[k], &seeds[k], &nee_seeds[k], &env_seeds[k],
                                     counters + GC_COUNT * k);
        memcpy(radiance + 3 * k, c.e, 12);
    }
    free_tree(&t);
    free_ctx(&cfg->base.base, &T, &M);
}

typedef struct {
    const gloss_ctx *G;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;
    double *mom;
} gloss_job;

static void *gloss_run(void *arg) {
    gloss_job *jb = (gloss_job *)arg;
    const rt_camera_data *cam = jb->G->Y.X.cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double m[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = gloss_sample_of(jb->G, i, j, s, NULL, NULL, NULL, NULL, NULL);
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

/* tree_frame's sums (and moments) with the glossy switches */
void gloss_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const gloss_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads,
                 float *fb, double *mom) {
    emit_tab T;
    sky_map M;
    light_tree t;
    gloss_ctx G;
    make_gloss_ctx(sc, cam, cfg, &T, &M, &t, 0, &G);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    gloss_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        gloss_job jb = {&G, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, gloss_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_tree(&t);
    free_ctx(&cfg->base.base, &T, &M);
}
