/* medium_ref.c — CPU reference of rt_render_medium / rt_trace_samples_medium (include/rtp_amd.h, "participating medium").
 * tests/medium_reference.py builds it on its own into a shared library (gcc -ffp-contract=off like the oracle).  It includes gloss_ref.c —
 * and through it tree_ref.c, emit_ref.c and oracle/rt_oracle.c — for the tables, the tree, the map, the camera, pg and the plane point, and
 * log_ref.h for the logarithm; it only reads them.  The vertex loop, the light samples of a medium vertex, the region's interval, the free
 * flight, the phase function and the transmittance are written here from the header's words.
 *
 * exp: the oracle's own expf — csrc/rt_device_math.h's exp_libm is that libm's for every float (tests/dev_math_checks.py).
 */
#include "gloss_ref.c"
#include "log_ref.h"

#define MED_FOUR_PI (2.0f * RT_NEE_TWO_PI)

/* what a call is made of (tests/medium_reference.py mirrors this struct) */
typedef struct {
    gloss_cfg base;
    rt_medium_params medium;
} medium_cfg;

/* the tallies of medium_trace_stats, in its order (tests/medium_reference.py names them the same way); they only count */
enum {
    MST_EVENTS,              /* medium vertices */
    MST_INTERVAL_EMPTY,      /* a path ray whose interval is empty */
    MST_ORIGIN_INSIDE,       /* a path ray whose interval starts at t0 == 0 */
    MST_BOX_PARALLEL_IN,     /* the box, a direction component of exactly 0, the origin strictly inside that slab (any ray, shadow rays included) */
    MST_BOX_PARALLEL_OUT,    /* … the origin on a face or outside: empty */
    MST_U_ZERO,              /* the free-flight draw was exactly 0 */
    MST_EVENT_AT_DEPTH_CUT,  /* a medium vertex at the last depth: no light sample, no next ray */
    MST_BLACK,               /* the throughput was black after the albedo */
    MST_TR_EMITTER,          /* Tr applied (a non-empty interval) where a shadow ray reached its emitter */
    MST_TR_ENV,              /* … where an environment shadow ray escaped */
    MST_ENV_SUPPRESSED,      /* a vertex that would have taken an environment sample, under a medium that fills all space */
    MST_CARRY_HIT,           /* a medium vertex's ph weighted a hit on a table entry */
    MST_CARRY_MISS,          /* … a miss */
    MST_GLOSSY_INSIDE,       /* a glossy event at a surface point the path ray reached inside the region */
    MST_EVENT_FIRST_RAY,     /* a medium vertex on the camera ray */
    MST_COUNT
};

typedef struct {
    gloss_ctx G;
    rt_medium_params m;
    int64_t *stats;          /* NULL, or the MST_COUNT tallies above (medium_trace_stats) */
} medium_ctx;

/* interval(o, d, t_end) of the header: 0 = empty.  st: NULL or the tallies */
static int med_interval(const rt_medium_params *m, v3 o, v3 d, float t_end, float *t0_out, float *t1_out, int64_t *st) {
    float t0 = 0.0f, t1 = t_end;
    if (m->region == 1) {
        const v3 oc = sub(o, V(m->a[0], m->a[1], m->a[2]));
        const float R = m->b[0];
        const float A = dot(d, d);
        const float hb = dot(oc, d);
        const float cc = dot(oc, oc) - R * R;
        const float disc = hb * hb - A * cc;
        if (!(disc > 0.0f)) return 0;
        const float sq = sqrtf(disc);
        const float ta = (-hb - sq) / A;
        const float tb = (-hb + sq) / A;
        t0 = ta > 0.0f ? ta : 0.0f;
        t1 = tb < t_end ? tb : t_end;
    } else if (m->region == 2) {
        for (int k = 0; k < 3; ++k) {
            if (d.e[k] == 0.0f) {
                if (!(m->a[k] < o.e[k] && o.e[k] < m->b[k])) {
                    if (st) st[MST_BOX_PARALLEL_OUT]++;
                    return 0;
                }
                if (st) st[MST_BOX_PARALLEL_IN]++;
                continue;
            }
            float ta = (m->a[k] - o.e[k]) / d.e[k];
            float tb = (m->b[k] - o.e[k]) / d.e[k];
            if (ta > tb) {
                const float t = ta;
                ta = tb;
                tb = t;
            }
            if (ta > t0) t0 = ta;
            if (tb < t1) t1 = tb;
        }
    }
    *t0_out = t0;
    *t1_out = t1;
    return t1 > t0;
}

/* ph(c) of the header */
static float med_ph(float g, float c) {
    if (g == 0.0f) return 1.0f / MED_FOUR_PI;
    const float den = (1.0f + g * g) - (2.0f * g) * c;
    return (1.0f - g * g) / (MED_FOUR_PI * (den * sqrtf(den)));
}
/* pb of a light sample at a medium vertex travelling along ud, in the sampled direction wl */
static float med_pb(float g, v3 ud, v3 wl) { return med_ph(g, dot(ud, wl) / sqrtf(dot(wl, wl))); }

/* Tr * c for the shadow ray (x, wl) that ended at t_end.  st: NULL or the tallies, which: the tally of a Tr that was applied */
static v3 med_attenuate(const rt_medium_params *m, v3 x, v3 wl, float t_end, v3 c, int64_t *st, int which) {
    float t0, t1;
    if (!(m->sigma_t > 0.0f) || !med_interval(m, x, wl, t_end, &t0, &t1, st)) return c;
    if (st) st[which]++;
    const float len = sqrtf(dot(wl, wl));
    const float L = (t1 - t0) * len;
    const float tr = expf(-(m->sigma_t * L));
    return scale(tr, c);
}

/* cos_t of the next direction from one draw */
static float med_cos(float g, float u1) {
    if (g == 0.0f) return 1.0f - 2.0f * u1;
    const float q = (1.0f - g * g) / ((1.0f - g) + (2.0f * g) * u1);
    float c = ((1.0f + g * g) - q * q) / (2.0f * g);
    if (c < -1.0f) c = -1.0f;
    if (c > 1.0f) c = 1.0f;
    return c;
}
/* the direction at cos_t from ud with the azimuth (cx, cy): Duff's basis, rt_render_nee's step 3 */
static v3 med_direction(v3 ud, float cos_t, float cx, float cy) {
    const float sin_t = sqrtf(fmaxf(0.0f, 1.0f - cos_t * cos_t));
    const float sg = copysignf(1.0f, ud.e[2]);
    const float ba = -1.0f / (sg + ud.e[2]);
    const float bb = (ud.e[0] * ud.e[1]) * ba;
    const v3 t1 = V(1.0f + ((sg * ud.e[0]) * ud.e[0]) * ba, sg * bb, -sg * ud.e[0]);
    const v3 t2 = V(bb, sg + (ud.e[1] * ud.e[1]) * ba, -ud.e[1]);
    const float sx = sin_t * cx, sy = sin_t * cy;
    v3 d;
    for (int k = 0; k < 3; ++k) d.e[k] = (t1.e[k] * sx + t2.e[k] * sy) + ud.e[k] * cos_t;
    return d;
}

/* The emitter sample of a medium vertex: rt_render_lit's step 4 (gloss_ref.c's entry_sample_pb) without the hemisphere test and with
 * pb = ph.  1 = a shadow ray is asked for */
static int med_entry_sample(const rt_scene_desc *sc, const emit_tab *T, int32_t e, float pmf, uint32_t *nee, v3 x, v3 a, v3 beta, float g, v3 ud, v3 *dir,
                            v3 *c) {
    float pl;
    v3 emit;
    if (T->kind[e] == 1) {
        const rt_plane *p = &sc->planes[T->index[e]];
        float ua, ub;
        if (p->type == RT_PLANE_ELLIPSE) {
            float px, py, q2;
            do {
                px = -1.0f + 2.0f * orc_random_float(nee);
                py = -1.0f + 2.0f * orc_random_float(nee);
                q2 = px * px + py * py;
            } while (q2 >= 1.0f);
            ua = 0.5f + 0.5f * px;
            ub = 0.5f + 0.5f * py;
        } else {
            ua = orc_random_float(nee);
            ub = orc_random_float(nee);
            if (p->type == RT_PLANE_TRIANGLE && ua + ub > 1.0f) {
                ua = 1.0f - ua;
                ub = 1.0f - ub;
            }
        }
        v3 y;
        for (int k = 0; k < 3; ++k) y.e[k] = (p->base.e[k] + ua * p->u.e[k]) + ub * p->v.e[k];
        float pa;
        if (!plane_pa(x, y, p, T->area[e], dir, &pa)) return 0;
        pl = pmf * pa;
        emit = from_rt(sc->materials[p->material_idx].emit);
    } else {
        const rt_sphere *s = &sc->spheres[T->index[e]];
        v3 w;
        float d2, om;
        if (!cone_of(x, s, &w, &d2, &om)) return 0;
        const float u1 = orc_random_float(nee);
        const float cos_t = 1.0f - u1 * om;
        float px, py, q2;
        do {
            px = -1.0f + 2.0f * orc_random_float(nee);
            py = -1.0f + 2.0f * orc_random_float(nee);
            q2 = px * px + py * py;
        } while (q2 >= 1.0f || q2 == 0.0f);
        const float q = sqrtf(q2);
        const float len = sqrtf(d2);
        *dir = med_direction(V(w.e[0] / len, w.e[1] / len, w.e[2] / len), cos_t, px / q, py / q);
        pl = pmf * pdf_cone(om);
        emit = from_rt(sc->materials[s->material_idx].emit);
    }
    const float pb = med_pb(g, ud, *dir);
    if (pb == 0.0f) return 0;
    const float f = T->mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), emit));
    return 1;
}
/* the environment sample of a medium vertex: step 5 without the hemisphere test and with pb = ph */
static int med_sky_sample(const sky_map *M, const rt_env_params *ep, uint32_t *env, v3 a, v3 beta, float g, v3 ud, v3 *dir, v3 *c, int linear) {
    const float ua = orc_random_float(env);
    const int32_t iy = pick(M->row_cdf, M->n, ua, linear);
    if (iy >= M->n) return 0;
    const float ub = orc_random_float(env);
    const int32_t ix = pick(M->col_cdf + (size_t)iy * M->n, M->n, ub, linear);
    if (ix >= M->n) return 0;
    const float uc = orc_random_float(env);
    const float ud2 = orc_random_float(env);
    const float h = 2.0f / (float)M->n;
    const float u = ((float)ix + uc) * h - 1.0f;
    const float v = ((float)iy + ud2) * h - 1.0f;
    const v3 p = decode_f(u, v);
    const float q2 = dot(p, p);
    const float q = sqrtf(q2);
    const v3 we = V(p.e[0] / q, p.e[1] / q, p.e[2] / q);
    for (int k = 0; k < 3; ++k) dir->e[k] = (ep->rot[k] * we.e[0] + ep->rot[3 + k] * we.e[1]) + ep->rot[6 + k] * we.e[2];
    const float pb = med_pb(g, ud, *dir);
    if (pb == 0.0f) return 0;
    const int32_t t = iy * M->n + ix;
    const float pl = pl_of(M, t, q2, q);
    const float f = ep->mode == 1 ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), scaled(M, ep, t)));
    return 1;
}

/* per-sample outcome beyond the radiance */
typedef struct {
    int32_t rays, events;
    int32_t end;          /* how the path ended: 0 miss, 1 depth, 2 absorbed at a surface (or an emitter), 3 beta = 0 in the medium */
} med_out;

/* The path.  carried: 0 none, 1 a diffuse event (pb = RT_NEE_PB), 2 a glossy event (pb = carry_pb against the lights whose switch is 1), 3 a
 * medium vertex (pb = carry_pb = ph against every light that is on; a ph that rounded to 0 is none) */
static v3 ray_color_medium(const medium_ctx *Mc, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, uint32_t *med, med_out *out) {
    const gloss_ctx *G = &Mc->G;
    const rt_medium_params *m = &Mc->m;
    const tree_ctx *Y = &G->Y;
    const lit_ctx *X = &Y->X;
    const rt_scene_desc *sc = X->sc;
    const rt_camera_data *cam = X->cam;
    const rt_env_params *ep = X->cfg->ep;
    const emit_tab *T = X->T;
    const int fog = m->sigma_t > 0.0f;
    const int emitters_on = T->count > 0;
    /* with region 0 and sigma_t > 0 the environment counts as not sampled for the whole call */
    const int sky_sampled = X->M && ep->mode != 0 && !X->M->empty && !(fog && m->region == 0);
    int64_t *st = Mc->stats;
    const int sky_suppressed = X->M && ep->mode != 0 && !X->M->empty && !sky_sampled;          /* (for the tallies alone) */
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0, events = 0;
    int carried = 0, end = 1;
    float carry_pb = 0.0f;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt, pi;
        int reached_inside = fog && m->region == 0;          /* (for the tallies alone) the path ray ends inside the region */
        nrays++;
        const int hit = closest(sc, &cur, &rec, &pt, &pi);
        /* ---- the segment and the free flight */
        if (fog) {
            float t0, t1;
            const int crossed = med_interval(m, cur.o, cur.d, hit ? rec.t : INFINITY, &t0, &t1, st);
            if (st && !crossed) st[MST_INTERVAL_EMPTY]++;
            reached_inside = crossed && hit && t1 == rec.t;
            if (crossed) {
                if (st && t0 == 0.0f) st[MST_ORIGIN_INSIDE]++;
                const float len = sqrtf(dot(cur.d, cur.d));
                const float u = orc_random_float(med);
                if (st && u == 0.0f) st[MST_U_ZERO]++;
                if (u != 0.0f) {
                    const float s = -log_ref(u) / m->sigma_t;
                    if (s < (t1 - t0) * len) {
                        /* ---- the medium vertex */
                        events++;
                        if (st) {
                            st[MST_EVENTS]++;
                            if (depth == 0) st[MST_EVENT_FIRST_RAY]++;
                        }
                        const v3 x = add(cur.o, scale(t0 + s / len, cur.d));
                        const v3 ud = unit(cur.d);
                        const v3 beta_in = beta;
                        const v3 a = V(m->albedo[0], m->albedo[1], m->albedo[2]);
                        beta = mulv(beta, a);
                        if (beta.e[0] == 0.0f && beta.e[1] == 0.0f && beta.e[2] == 0.0f) {
                            if (st) st[MST_BLACK]++;
                            end = 3;
                            break;
                        }
                        if (!(depth + 1 < cam->max_depth)) {
                            if (st) st[MST_EVENT_AT_DEPTH_CUT]++;
                            break;
                        }
                        if (st && sky_suppressed) st[MST_ENV_SUPPRESSED]++;
                        hitrec srec;
                        int spt, spi;
                        ray shadow;
                        v3 c;
                        shadow.o = x;
                        if (emitters_on) {
                            int32_t e;
                            float pmf = 0.0f;
                            if (Y->select) {
                                e = tree_pick(Y->tree, nee, x, &pmf, NULL);
                            } else {
                                const float ue = orc_random_float(nee);
                                e = 0;
                                while (e < T->count && !(ue < T->cdf[e])) ++e;
                                if (e < T->count) pmf = T->pmf[e];
                            }
                            if (e < T->count && med_entry_sample(sc, T, e, pmf, nee, x, a, beta_in, m->g, ud, &shadow.d, &c)) {
                                nrays++;
                                const int sh = closest(sc, &shadow, &srec, &spt, &spi);
                                if (sh && spt == T->kind[e] && spi == T->index[e]) final_color = add(final_color, med_attenuate(m, x, shadow.d, srec.t, c, st, MST_TR_EMITTER));
                            }
                        }
                        if (sky_sampled && med_sky_sample(X->M, ep, env, a, beta_in, m->g, ud, &shadow.d, &c, X->linear)) {
                            nrays++;
                            if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, med_attenuate(m, x, shadow.d, INFINITY, c, st, MST_TR_ENV));
                        }
                        const float u1 = orc_random_float(med);
                        const float cos_t = med_cos(m->g, u1);
                        float px, py, q2;
                        do {
                            px = -1.0f + 2.0f * orc_random_float(med);
                            py = -1.0f + 2.0f * orc_random_float(med);
                            q2 = px * px + py * py;
                        } while (q2 >= 1.0f || q2 == 0.0f);
                        const float q = sqrtf(q2);
                        cur.o = x;
                        cur.d = med_direction(ud, cos_t, px / q, py / q);
                        carry_pb = med_ph(m->g, cos_t);
                        carried = carry_pb != 0.0f ? 3 : 0;
                        continue;
                    }
                }
            }
        }
        /* ---- no event: rt_render_lit's vertex (gloss_ref.c's, with the medium vertex as a third kind of carried fact and Tr on the light
         * samples) */
        if (!hit) {
            end = 0;
            if (!X->M || (depth == 0 && !ep->camera_visible)) {
                final_color = add(final_color, mulv(beta, from_rt(cam->background)));
                break;
            }
            v3 p;
            const int32_t t = texel_of(to_env(ep, cur.d), X->M->n, &p);
            v3 term = mulv(beta, scaled(X->M, ep, t));
            const int weighted = carried == 1 || carried == 3 || (carried == 2 && G->glossy_env && carry_pb != 0.0f);
            if (weighted && sky_sampled) {
                if (st && carried == 3) st[MST_CARRY_MISS]++;
                const float pb = carried == 1 ? RT_NEE_PB : carry_pb;
                const float q2 = dot(p, p);
                const float pl = pl_of(X->M, t, q2, sqrtf(q2));
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
        v3 emitted = mulv(beta, from_rt(mat->emit));
        const int hit_weighted = carried == 1 || carried == 3 || (carried == 2 && G->glossy_nee && carry_pb != 0.0f);
        if (hit_weighted && (pt == 0 || pt == 1) && emitters_on) {
            const int e = tab_find(T, pt, pi);
            if (e >= 0) {
                if (st && carried == 3) st[MST_CARRY_HIT]++;
                const float pb = carried == 1 ? RT_NEE_PB : carry_pb;
                v3 w;
                float d2, om, pa, pl = 0.0f;
                if (pt == 1) {
                    if (plane_pa(cur.o, rec.point, &sc->planes[pi], T->area[e], &w, &pa)) pl = (Y->select ? tree_pmf(Y->tree, e, cur.o, NULL) : T->pmf[e]) * pa;
                } else if (cone_of(cur.o, &sc->spheres[pi], &w, &d2, &om))
                    pl = (Y->select ? tree_pmf(Y->tree, e, cur.o, NULL) : T->pmf[e]) * pdf_cone(om);
                const float wb = T->mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                emitted = scale(wb, emitted);
            }
        }
        final_color = add(final_color, emitted);
        ray scattered;
        v3 attenuation;
        int event = 0, ok;
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
        if (st) {
            if (glossy_event && reached_inside) st[MST_GLOSSY_INSIDE]++;
            /* the environment sample this vertex would have taken were the environment sampled */
            if (sky_suppressed && depth + 1 < cam->max_depth && ((event == 1 && ok) || (B.glossy && G->glossy_env))) st[MST_ENV_SUPPRESSED]++;
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
                    const int sh = closest(sc, &shadow, &srec, &spt, &spi);
                    if (sh && spt == T->kind[e] && spi == T->index[e]) final_color = add(final_color, med_attenuate(m, rec.point, shadow.d, srec.t, c, st, MST_TR_EMITTER));
                }
            }
            if (take_env) {
                int pg_zero = 0;
                if (sky_sample_pb(X->M, ep, env, rec.normal, albedo, beta, &B, &shadow.d, &c, X->linear, &pg_zero)) {
                    nrays++;
                    if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, med_attenuate(m, rec.point, shadow.d, INFINITY, c, st, MST_TR_ENV));
                }
            }
        }
        if (!ok) {
            end = 2;
            break;
        }
        beta = mulv(beta, attenuation);
        cur = scattered;
        carried = event == 1 ? 1 : (glossy_event ? 2 : 0);
        carry_pb = glossy_event ? gloss_pg(unit(scattered.d), reflected, mat->fuzz) : 0.0f;
    }
    if (out) {
        out->rays = nrays;
        out->events = events;
        out->end = end;
    }
    return final_color;
}

static v3 medium_sample_of(const medium_ctx *Mc, int i, int j, int s, med_out *out, uint32_t *seeds4) {
    const lit_ctx *X = &Mc->G.Y.X;
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    uint32_t med = orc_wang_hash(seed ^ RT_MEDIUM_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_medium(Mc, r, &seed, &nee, &env, &med, out);
    if (seeds4) {
        seeds4[0] = seed;
        seeds4[1] = nee;
        seeds4[2] = env;
        seeds4[3] = med;
    }
    return c;
}

static void make_medium_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const medium_cfg *cfg, emit_tab *T, sky_map *M, light_tree *t, int linear,
                            medium_ctx *Mc) {
    make_gloss_ctx(sc, cam, &cfg->base, T, M, t, linear, &Mc->G);
    Mc->m = cfg->medium;
    Mc->stats = NULL;
}

/* ---- what tests/medium_reference.py calls -------------------------------------------------------------------------------------------- */
/* ph(c) for count cosines, in the header's float32 order */
void medium_ph_many(int64_t count, float g, const float *c, float *ph) {
    for (int64_t k = 0; k < count; ++k) ph[k] = med_ph(g, c[k]);
}
/* count draws of cos_t from the stream that starts at seed (one draw each, consecutive) */
void medium_cos_draws(int64_t count, float g, uint32_t seed, float *c) {
    for (int64_t k = 0; k < count; ++k) c[k] = med_cos(g, orc_random_float(&seed));
}
/* the region's interval on count rays (o, d: 3 floats each) over [0, t_end]: hit 1/0, t0, t1 */
void medium_intervals(const rt_medium_params *m, int64_t count, const float *o, const float *d, const float *t_end, int32_t *hit, float *t0, float *t1) {
    for (int64_t k = 0; k < count; ++k) {
        t0[k] = t1[k] = 0.0f;
        hit[k] = med_interval(m, V(o[3 * k], o[3 * k + 1], o[3 * k + 2]), V(d[3 * k], d[3 * k + 1], d[3 * k + 2]), t_end[k], &t0[k], &t1[k], NULL);
    }
}

/* per vertex (tests/light_vertex_cases.py): gloss_vertices' words for a medium vertex — the light sample under pb = ph about
 * ud = nv with g = s, without a hemisphere.  routine 0: the emitter table's, 1: the environment's, 5: ph itself in the direction w = x
 * (word 1: word 0 is gloss_vertices').  flags (may be NULL) takes TL_OK, TL_NO_ENTRY and TL_FELL: the sample functions here keep no note */
void medium_vertices(const rt_scene_desc *sc, const rt_camera_data *cam, const gloss_cfg *cfg, int32_t routine, int64_t count, const float *x, const float *nv,
                     const float *s, const uint32_t *seed, const float *ab, uint32_t *out, uint32_t *flags) {
    emit_tab T;
    sky_map M;
    light_tree t;
    gloss_ctx G;
    make_gloss_ctx(sc, cam, cfg, &T, &M, &t, 0, &G);
    const lit_ctx *X = &G.Y.X;
    const v3 a = V(ab[0], ab[1], ab[2]), beta = V(ab[3], ab[4], ab[5]);
    memset(out, 0, (size_t)count * 64);
    for (int64_t k = 0; k < count; ++k) {
        const v3 xk = V(x[3 * k], x[3 * k + 1], x[3 * k + 2]), ud = V(nv[3 * k], nv[3 * k + 1], nv[3 * k + 2]);
        uint32_t *w = out + 16 * k;
        vtx_note note = {0u, 0.0f, 0.0f};
        vtx_note *N = flags ? &note : NULL;
        if (routine == 0 || (routine == 1 && X->M)) {
            uint32_t st = seed[k];
            v3 dir, c;
            int ok;
            int32_t e = 0;
            if (routine == 0) {
                float pmf;
                e = vertex_pick(&G, &st, xk, &pmf, N);
                ok = e < T.count && med_entry_sample(sc, &T, e, pmf, &st, xk, a, beta, s[k], ud, &dir, &c);
            } else {
                ok = med_sky_sample(X->M, X->cfg->ep, &st, a, beta, s[k], ud, &dir, &c, 0);
            }
            if (ok) {
                w[0] = 1;
                put3(w + 1, dir, N);
                put3(w + 4, c, N);
                if (routine == 0) w[7] = (uint32_t)(2 * T.index[e] + T.kind[e]);
                if (N) N->flags |= TL_OK;
            }
            w[routine == 0 ? 8 : 7] = st;
        } else if (routine == 5) {
            w[1] = word_of(med_pb(s[k], ud, xk));
        }
        if (flags) flags[k] = note.flags;
    }
    free_tree(&t);
    free_ctx(&cfg->base.base, &T, &M);
}

/* count samples (ijs: i, j, s) → radiance, rays, medium events, how each path ended, and the four final RNG states (seed, nee, env, med);
 * stats (MST_COUNT words, may be NULL): the tallies named above, summed over the samples */
void medium_trace_stats(const rt_scene_desc *sc, const rt_camera_data *cam, const medium_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance,
                        int32_t *rays, int32_t *events, int32_t *ends, uint32_t *seeds4, int32_t linear, int64_t *stats) {
    emit_tab T;
    sky_map M;
    light_tree t;
    medium_ctx Mc;
    make_medium_ctx(sc, cam, cfg, &T, &M, &t, linear, &Mc);
    if (stats) memset(stats, 0, MST_COUNT * sizeof(int64_t));
    Mc.stats = stats;
    for (int64_t k = 0; k < count; ++k) {
        med_out o;
        const v3 c = medium_sample_of(&Mc, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &o, seeds4 + 4 * k);
        memcpy(radiance + 3 * k, c.e, 12);
        rays[k] = o.rays;
        events[k] = o.events;
        ends[k] = o.end;
    }
    free_tree(&t);
    free_ctx(&cfg->base.base.base, &T, &M);
}

void medium_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const medium_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance, int32_t *rays,
                  int32_t *events, int32_t *ends, uint32_t *seeds4, int32_t linear) {
    medium_trace_stats(sc, cam, cfg, count, ijs, radiance, rays, events, ends, seeds4, linear, NULL);
}

typedef struct {
    const medium_ctx *Mc;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;
    double *mom;
} medium_job;

static void *medium_run(void *arg) {
    medium_job *jb = (medium_job *)arg;
    const rt_camera_data *cam = jb->Mc->G.Y.X.cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double mm[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = medium_sample_of(jb->Mc, i, j, s, NULL, NULL);
                pixel = add(pixel, c);
                for (int k = 0; k < 3; ++k) {
                    mm[k] += c.e[k];
                    mm[3 + k] += (double)c.e[k] * (double)c.e[k];
                }
            }
            if (jb->fb) memcpy(jb->fb + 3 * p, pixel.e, 12);
            if (jb->mom) memcpy(jb->mom + 6 * p, mm, sizeof(mm));
        }
    }
    return NULL;
}

/* gloss_frame's sums (and moments) under the medium */
void medium_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const medium_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads,
                  float *fb, double *mom) {
    emit_tab T;
    sky_map M;
    light_tree t;
    medium_ctx Mc;
    make_medium_ctx(sc, cam, cfg, &T, &M, &t, 0, &Mc);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    medium_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        medium_job jb = {&Mc, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, medium_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_tree(&t);
    free_ctx(&cfg->base.base.base, &T, &M);
}
