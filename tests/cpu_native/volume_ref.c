/* volume_ref.c — CPU reference of rt_render_volume / rt_trace_samples_volume (include/rtp_amd.h, "density grid").
 * tests/volume_reference.py builds it on its own into a shared library (gcc -ffp-contract=off like the oracle).  It includes medium_ref.c —
 * and through it gloss_ref.c, tree_ref.c, emit_ref.c, oracle/rt_oracle.c and log_ref.h — for the interval, the medium vertex's light
 * samples, the phase function and everything of the lit path; it only reads them.  The walk through the cells, the free flight over it and
 * the optical depth are written here from the header's words, and the vertex loop is medium_ref.c's with those two in the places of the
 * homogeneous flight and transmittance.  vol_walk_d states the same walk in float64 (interval included), for the tests of the rounding.
 */
#include "medium_ref.c"

/* what a call is made of (tests/volume_reference.py mirrors this struct) */
typedef struct {
    medium_cfg base;
    const float *rho;        /* NULL: no grid — medium_ref.c's path */
    int32_t nx, ny, nz;
} volume_cfg;

typedef struct {
    medium_ctx Mc;
    const float *rho;
    int32_t n[3];
} volume_ctx;

/* plane(m) of axis k */
static float vol_plane(const rt_medium_params *m, const int32_t *n, int k, int32_t i) {
    if (i == 0) return m->a[k];
    if (i == n[k]) return m->b[k];
    const float w = (m->b[k] - m->a[k]) / (float)n[k];
    return m->a[k] + (float)i * w;
}

/* Tallies of one walk, a bit each (tests/volume_reference.py's TALLIES names them in this order).  They only count: vol_tally is NULL except
 * inside volume_walks, which runs on one thread, and no value of the walk depends on them */
enum { VT_TIE2, VT_TIE3, VT_CLAMP, VT_ENTRY_CLAMPED, VT_LEFT_T1, VT_LEFT_INDEX, VT_D_ZERO, VT_FL_EMPTY, VT_FL_FIRST, VT_FL_AFTER_EMPTY, VT_FL_NONE };
static int32_t *vol_tally = NULL;
#define VOL_TALLY(bit) do { if (vol_tally) *vol_tally |= 1 << (bit); } while (0)

/* The walk of the header over the non-empty interval [t0, t1] of (o, d), len = |d|.  flight 1: *v is rem on entry; 1 = an event, *v its
 * parameter t.  flight 0: *v is acc (0 on entry), the result 0.  cells: the visited cells are added.  segs: NULL, or 3 doubles — the sum of
 * the segments (each a float, summed in double), the smallest segment, the number of cells of this walk */
static int vol_walk(const volume_ctx *Vc, int flight, v3 o, v3 d, float t0, float t1, float len, float *v, int32_t *cells, double *segs) {
    const rt_medium_params *m = &Vc->Mc.m;
    const int32_t *n = Vc->n;
    int32_t c[3];
    for (int k = 0; k < 3; ++k) {
        const float w = (m->b[k] - m->a[k]) / (float)n[k];
        const float p = o.e[k] + t0 * d.e[k];
        c[k] = (int32_t)floorf((p - m->a[k]) / w);
        if (c[k] < 0 || c[k] > n[k] - 1) VOL_TALLY(VT_ENTRY_CLAMPED);
        if (d.e[k] == 0.0f) VOL_TALLY(VT_D_ZERO);
        if (c[k] < 0) c[k] = 0;
        if (c[k] > n[k] - 1) c[k] = n[k] - 1;
    }
    float ta = t0;
    int first = 1, passed_empty = 0;          /* (for the tallies alone) */
    for (int32_t left = n[0] + n[1] + n[2]; left > 0; --left) {
        float tn[3];
        for (int k = 0; k < 3; ++k) {
            if (d.e[k] > 0.0f) tn[k] = (vol_plane(m, n, k, c[k] + 1) - o.e[k]) / d.e[k];
            else if (d.e[k] < 0.0f) tn[k] = (vol_plane(m, n, k, c[k]) - o.e[k]) / d.e[k];
            else tn[k] = INFINITY;
        }
        float tm = tn[0];
        int axis = 0;
        if (tn[1] < tm) {
            tm = tn[1];
            axis = 1;
        }
        if (tn[2] < tm) {
            tm = tn[2];
            axis = 2;
        }
        if (vol_tally && tm < INFINITY) {
            const int ties = (tn[0] == tm) + (tn[1] == tm) + (tn[2] == tm);
            if (ties == 2) VOL_TALLY(VT_TIE2);
            if (ties == 3) VOL_TALLY(VT_TIE3);
        }
        float tb = tm < t1 ? tm : t1;
        if (tb < ta) VOL_TALLY(VT_CLAMP);
        if (tb < ta) tb = ta;
        const float seg = (tb - ta) * len;
        const float sigma_c = m->sigma_t * Vc->rho[((size_t)c[2] * (size_t)n[1] + (size_t)c[1]) * (size_t)n[0] + (size_t)c[0]];
        (*cells)++;
        if (segs) {
            segs[0] += (double)seg;
            if ((double)seg < segs[1]) segs[1] = (double)seg;
            segs[2] += 1.0;
        }
        if (flight) {
            if (sigma_c > 0.0f) {
                const float s = *v / sigma_c;
                if (s < seg) {
                    if (first) VOL_TALLY(VT_FL_FIRST);
                    if (passed_empty) VOL_TALLY(VT_FL_AFTER_EMPTY);
                    *v = ta + s / len;
                    return 1;
                }
                *v = *v - sigma_c * seg;
            } else {
                VOL_TALLY(VT_FL_EMPTY);
                passed_empty = 1;
            }
            first = 0;
        } else {
            *v = *v + sigma_c * seg;
        }
        if (tb >= t1) VOL_TALLY(VT_LEFT_T1);
        if (tb >= t1) break;
        c[axis] += d.e[axis] > 0.0f ? 1 : -1;
        if (c[axis] < 0 || c[axis] >= n[axis]) VOL_TALLY(VT_LEFT_INDEX);
        if (c[axis] < 0 || c[axis] >= n[axis]) break;
        ta = tb;
    }
    if (flight) VOL_TALLY(VT_FL_NONE);
    return 0;
}

/* Tr * c for the shadow ray (x, wl) that ended at t_end.  st: NULL or the tallies, which: the tally of a Tr that was applied */
static v3 vol_attenuate(const volume_ctx *Vc, v3 x, v3 wl, float t_end, v3 c, int32_t *cells, int64_t *st, int which) {
    const rt_medium_params *m = &Vc->Mc.m;
    float t0, t1;
    if (!(m->sigma_t > 0.0f) || !med_interval(m, x, wl, t_end, &t0, &t1, st)) return c;
    if (st) st[which]++;
    const float len = sqrtf(dot(wl, wl));
    float acc = 0.0f;
    vol_walk(Vc, 0, x, wl, t0, t1, len, &acc, cells, NULL);
    const float tr = expf(-acc);
    return scale(tr, c);
}

/* The path: medium_ref.c's ray_color_medium, restated, with the walk as the free flight and as the optical depth */
static v3 ray_color_volume(const volume_ctx *Vc, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, uint32_t *med, med_out *out, int32_t *cells_out) {
    const medium_ctx *Mc = &Vc->Mc;
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
    const int sky_sampled = X->M && ep->mode != 0 && !X->M->empty && !(fog && m->region == 0);
    int64_t *st = Mc->stats;
    const int sky_suppressed = X->M && ep->mode != 0 && !X->M->empty && !sky_sampled;          /* (for the tallies alone) */
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0, events = 0, cells = 0;
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
                    float v = -log_ref(u);
                    if (vol_walk(Vc, 1, cur.o, cur.d, t0, t1, len, &v, &cells, NULL)) {
                        /* ---- the medium vertex */
                        events++;
                        if (st) {
                            st[MST_EVENTS]++;
                            if (depth == 0) st[MST_EVENT_FIRST_RAY]++;
                        }
                        const v3 x = add(cur.o, scale(v, cur.d));
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
                                if (sh && spt == T->kind[e] && spi == T->index[e])
                                    final_color = add(final_color, vol_attenuate(Vc, x, shadow.d, srec.t, c, &cells, st, MST_TR_EMITTER));
                            }
                        }
                        if (sky_sampled && med_sky_sample(X->M, ep, env, a, beta_in, m->g, ud, &shadow.d, &c, X->linear)) {
                            nrays++;
                            if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, vol_attenuate(Vc, x, shadow.d, INFINITY, c, &cells, st, MST_TR_ENV));
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
        /* ---- no event: rt_render_lit's vertex, as in medium_ref.c */
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
                    if (sh && spt == T->kind[e] && spi == T->index[e])
                        final_color = add(final_color, vol_attenuate(Vc, rec.point, shadow.d, srec.t, c, &cells, st, MST_TR_EMITTER));
                }
            }
            if (take_env) {
                int pg_zero = 0;
                if (sky_sample_pb(X->M, ep, env, rec.normal, albedo, beta, &B, &shadow.d, &c, X->linear, &pg_zero)) {
                    nrays++;
                    if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, vol_attenuate(Vc, rec.point, shadow.d, INFINITY, c, &cells, st, MST_TR_ENV));
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
    if (cells_out) *cells_out = cells;
    return final_color;
}

/* one sample: without a grid medium_ref.c's own path (volume == NULL is rt_render_medium itself) */
static v3 volume_sample_of(const volume_ctx *Vc, int i, int j, int s, med_out *out, uint32_t *seeds4, int32_t *cells_out) {
    if (!Vc->rho) {
        if (cells_out) *cells_out = 0;
        return medium_sample_of(&Vc->Mc, i, j, s, out, seeds4);
    }
    const lit_ctx *X = &Vc->Mc.G.Y.X;
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    uint32_t med = orc_wang_hash(seed ^ RT_MEDIUM_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_volume(Vc, r, &seed, &nee, &env, &med, out, cells_out);
    if (seeds4) {
        seeds4[0] = seed;
        seeds4[1] = nee;
        seeds4[2] = env;
        seeds4[3] = med;
    }
    return c;
}

static void make_volume_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const volume_cfg *cfg, emit_tab *T, sky_map *M, light_tree *t, int linear,
                            volume_ctx *Vc) {
    make_medium_ctx(sc, cam, &cfg->base, T, M, t, linear, &Vc->Mc);
    Vc->rho = cfg->rho;
    Vc->n[0] = cfg->nx;
    Vc->n[1] = cfg->ny;
    Vc->n[2] = cfg->nz;
}

/* ---- what tests/volume_reference.py calls -------------------------------------------------------------------------------------------- */
/* The walk alone on count rays (o, d: 3 floats each) over [0, t_end] through the grid rho (n: nx, ny, nz) in the box of m: hit 1/0 (the
 * interval), acc = the optical depth (float32, the header's sum), cells, and per ray three doubles: the sum of the segments, the smallest
 * segment, (t1 - t0) * len as the walk's float32 computes it.  rem (may be NULL): per ray a remaining optical depth for a free flight over
 * the same interval → event 1/0, its t (0 without an event), rem_left, the rem the flight ended with (0 with an event), and the cells the
 * flight visited.  tr: expf(-acc) as
 * vol_attenuate takes it (0, like every column, where the interval is empty).  flags (may be NULL): per ray the tallies of its walks, a bit each (VT_*) */
void volume_walks(const rt_medium_params *m, const float *rho, const int32_t *n, int64_t count, const float *o, const float *d, const float *t_end, int32_t *hit,
                  float *acc, int32_t *cells, double *segs, const float *rem, int32_t *event, float *t_event, float *tr, float *rem_left, int32_t *flight_cells, int32_t *flags) {
    volume_ctx Vc;
    memset(&Vc, 0, sizeof(Vc));
    Vc.Mc.m = *m;
    Vc.rho = rho;
    for (int k = 0; k < 3; ++k) Vc.n[k] = n[k];
    for (int64_t r = 0; r < count; ++r) {
        const v3 oo = V(o[3 * r], o[3 * r + 1], o[3 * r + 2]), dd = V(d[3 * r], d[3 * r + 1], d[3 * r + 2]);
        float t0, t1;
        acc[r] = 0.0f;
        cells[r] = 0;
        segs[3 * r] = segs[3 * r + 2] = 0.0;
        segs[3 * r + 1] = INFINITY;
        if (rem) {
            event[r] = 0;
            t_event[r] = 0.0f;
            rem_left[r] = 0.0f;
            flight_cells[r] = 0;
        }
        tr[r] = 0.0f;
        if (flags) flags[r] = 0;
        hit[r] = med_interval(m, oo, dd, t_end[r], &t0, &t1, NULL);
        if (!hit[r]) continue;
        const float len = sqrtf(dot(dd, dd));
        double sg[3] = {0.0, INFINITY, 0.0};
        vol_tally = flags ? &flags[r] : NULL;
        vol_walk(&Vc, 0, oo, dd, t0, t1, len, &acc[r], &cells[r], sg);
        tr[r] = expf(-acc[r]);
        segs[3 * r] = sg[0];
        segs[3 * r + 1] = sg[1];
        segs[3 * r + 2] = (double)((t1 - t0) * len);
        if (rem) {
            float v = rem[r];
            event[r] = vol_walk(&Vc, 1, oo, dd, t0, t1, len, &v, &flight_cells[r], NULL);
            if (event[r]) t_event[r] = v;
            else rem_left[r] = v;
        }
        vol_tally = NULL;
    }
}

/* The same walk in float64 — the interval, the planes, the entry cell, tnext, the segments and the sum — from the same float32 inputs:
 * hit, acc and (t1 - t0) * len per ray */
void volume_walks_f64(const rt_medium_params *m, const float *rho, const int32_t *n, int64_t count, const float *o, const float *d, const float *t_end,
                      int32_t *hit, double *acc, double *length) {
    for (int64_t r = 0; r < count; ++r) {
        double oo[3], dd[3], lo[3], hi[3], w[3];
        for (int k = 0; k < 3; ++k) {
            oo[k] = o[3 * r + k];
            dd[k] = d[3 * r + k];
            lo[k] = m->a[k];
            hi[k] = m->b[k];
            w[k] = (hi[k] - lo[k]) / (double)n[k];
        }
        double t0 = 0.0, t1 = t_end[r];
        int empty = 0;
        for (int k = 0; k < 3 && !empty; ++k) {
            if (dd[k] == 0.0) {
                if (!(lo[k] < oo[k] && oo[k] < hi[k])) empty = 1;
                continue;
            }
            double ta = (lo[k] - oo[k]) / dd[k], tb = (hi[k] - oo[k]) / dd[k];
            if (ta > tb) {
                const double t = ta;
                ta = tb;
                tb = t;
            }
            if (ta > t0) t0 = ta;
            if (tb < t1) t1 = tb;
        }
        hit[r] = !empty && t1 > t0;
        acc[r] = 0.0;
        length[r] = 0.0;
        if (!hit[r]) continue;
        const double len = sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]);
        length[r] = (t1 - t0) * len;
        int32_t c[3];
        for (int k = 0; k < 3; ++k) {
            c[k] = (int32_t)floor(((oo[k] + t0 * dd[k]) - lo[k]) / w[k]);
            if (c[k] < 0) c[k] = 0;
            if (c[k] > n[k] - 1) c[k] = n[k] - 1;
        }
        double ta = t0, sum = 0.0;
        for (int32_t left = n[0] + n[1] + n[2]; left > 0; --left) {
            double tn[3];
            for (int k = 0; k < 3; ++k) {
                const int32_t i = dd[k] > 0.0 ? c[k] + 1 : c[k];
                const double plane = i == 0 ? lo[k] : (i == n[k] ? hi[k] : lo[k] + (double)i * w[k]);
                tn[k] = dd[k] == 0.0 ? INFINITY : (plane - oo[k]) / dd[k];
            }
            double tm = tn[0];
            int axis = 0;
            if (tn[1] < tm) {
                tm = tn[1];
                axis = 1;
            }
            if (tn[2] < tm) {
                tm = tn[2];
                axis = 2;
            }
            double tb = tm < t1 ? tm : t1;
            if (tb < ta) tb = ta;
            sum += ((double)m->sigma_t * (double)rho[((size_t)c[2] * (size_t)n[1] + (size_t)c[1]) * (size_t)n[0] + (size_t)c[0]]) * ((tb - ta) * len);
            if (tb >= t1) break;
            c[axis] += dd[axis] > 0.0 ? 1 : -1;
            if (c[axis] < 0 || c[axis] >= n[axis]) break;
            ta = tb;
        }
        acc[r] = sum;
    }
}

/* count samples (ijs: i, j, s) → medium_trace's columns and the cells visited per sample */
void volume_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const volume_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance, int32_t *rays,
                  int32_t *events, int32_t *ends, uint32_t *seeds4, int32_t *cells, int32_t linear) {
    emit_tab T;
    sky_map M;
    light_tree t;
    volume_ctx Vc;
    make_volume_ctx(sc, cam, cfg, &T, &M, &t, linear, &Vc);
    for (int64_t k = 0; k < count; ++k) {
        med_out o;
        const v3 c = volume_sample_of(&Vc, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &o, seeds4 + 4 * k, &cells[k]);
        memcpy(radiance + 3 * k, c.e, 12);
        rays[k] = o.rays;
        events[k] = o.events;
        ends[k] = o.end;
    }
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base, &T, &M);
}

typedef struct {
    const volume_ctx *Vc;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;
    double *mom;
} volume_job;

static void *volume_run(void *arg) {
    volume_job *jb = (volume_job *)arg;
    const rt_camera_data *cam = jb->Vc->Mc.G.Y.X.cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double mm[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = volume_sample_of(jb->Vc, i, j, s, NULL, NULL, NULL);
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

/* medium_frame's sums (and moments) under the grid */
void volume_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const volume_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads,
                  float *fb, double *mom) {
    emit_tab T;
    sky_map M;
    light_tree t;
    volume_ctx Vc;
    make_volume_ctx(sc, cam, cfg, &T, &M, &t, 0, &Vc);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    volume_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        volume_job jb = {&Vc, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, volume_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base, &T, &M);
}
