/* chroma_ref.c — CPU reference of rt_render_chroma / rt_trace_samples_chroma (include/rtp_amd.h, "chromatic extinction").
 * tests/chroma_reference.py builds it on its own into a shared library (gcc -ffp-contract=off like the oracle).  It includes volume_ref.c —
 * and through it medium_ref.c and everything of the lit path — for the interval, the walk, the medium vertex's light samples and the phase
 * function; it only reads them.  The channel draw, the target, the density length, the per-channel transmittance and the weights are
 * written here from the header's words, and the vertex loop is volume_ref.c's with those in the places of the grey flight and
 * transmittance.  Equal tints (and no medium) are handed to volume_ref.c's own entry points, as the library hands them to rt_render_volume.
 */
#include "volume_ref.c"

/* what a call is made of (tests/chroma_reference.py mirrors this struct) */
typedef struct {
    volume_cfg base;
    float tint[3];
} chroma_cfg;

typedef struct {
    volume_ctx V;          /* its medium's sigma_t is 1: the walk sums rho_c * seg.  V.rho == NULL: no grid */
    float sigma[3];        /* sigma_t * tint[k] */
} chroma_ctx;

/* Tr of a channel over the density length A */
static float chr_tr(float sigma_k, float A) { return sigma_k == 0.0f ? 1.0f : expf(-(sigma_k * A)); }

/* a channel's weight, its term e of den: (3 e) / den, at most 3 */
static float chr_weight(float e, float den) {
    const float w = (3.0f * e) / den;
    return w > 3.0f ? 3.0f : w;
}

/* the density length of the non-empty interval [t0, t1] */
static float chr_length(const volume_ctx *Vc, v3 o, v3 d, float t0, float t1, float len, int32_t *cells) {
    if (!Vc->rho) return (t1 - t0) * len;
    float acc = 0.0f;
    vol_walk(Vc, 0, o, d, t0, t1, len, &acc, cells, NULL);
    return acc;
}
/* the flight to the target R over the non-empty interval: 1 = an event at *t; 0: *A is the interval's density length (the sum a flight
 * walk keeps is the transmittance walk's: the same products added in the same order, and a cell of density 0 adds +0) */
static int chr_flight(const volume_ctx *Vc, v3 o, v3 d, float t0, float t1, float len, float R, float *t, float *A, int32_t *cells) {
    if (!Vc->rho) {
        *A = (t1 - t0) * len;
        if (!(R < *A)) return 0;
        *t = t0 + R / len;
        return 1;
    }
    float v = R;
    if (vol_walk(Vc, 1, o, d, t0, t1, len, &v, cells, NULL)) {
        *t = v;
        return 1;
    }
    int32_t again = 0;
    *A = chr_length(Vc, o, d, t0, t1, len, &again);
    return 0;
}

/* Tr_k * c_k for the shadow ray (x, wl) that ended at t_end */
static v3 chr_attenuate(const chroma_ctx *Cc, v3 x, v3 wl, float t_end, v3 c, int32_t *cells, int64_t *st, int which) {
    const volume_ctx *Vc = &Cc->V;
    float t0, t1;
    if (!med_interval(&Vc->Mc.m, x, wl, t_end, &t0, &t1, st)) return c;
    if (st) st[which]++;
    const float len = sqrtf(dot(wl, wl));
    const float A = chr_length(Vc, x, wl, t0, t1, len, cells);
    return V(chr_tr(Cc->sigma[0], A) * c.e[0], chr_tr(Cc->sigma[1], A) * c.e[1], chr_tr(Cc->sigma[2], A) * c.e[2]);
}

/* The path: volume_ref.c's ray_color_volume, restated, with the flight by one channel's extinction, the channels' weights on beta and the
 * per-channel transmittance of the shadow rays */
static v3 ray_color_chroma(const chroma_ctx *Cc, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, uint32_t *med, med_out *out, int32_t *cells_out) {
    const volume_ctx *Vc = &Cc->V;
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
                    /* ---- the channel, the target and the flight */
                    const float uc = orc_random_float(med);
                    int j = (int)(uc * 3.0f);
                    if (j > 2) j = 2;
                    const float sigma_j = Cc->sigma[j];
                    const float R = sigma_j == 0.0f ? INFINITY : -log_ref(u) / sigma_j;
                    float A, t;
                    const int flown = chr_flight(Vc, cur.o, cur.d, t0, t1, len, R, &t, &A, &cells);
                    if (flown) A = R;
                    const float tr0 = chr_tr(Cc->sigma[0], A), tr1 = chr_tr(Cc->sigma[1], A), tr2 = chr_tr(Cc->sigma[2], A);
                    if (flown) {
                        const float e0 = Cc->sigma[0] * tr0, e1 = Cc->sigma[1] * tr1, e2 = Cc->sigma[2] * tr2;
                        const float den = (e0 + e1) + e2;
                        beta = V(beta.e[0] * chr_weight(e0, den), beta.e[1] * chr_weight(e1, den), beta.e[2] * chr_weight(e2, den));
                    /* ---- the medium vertex */
                    events++;
                    if (st) {
                        st[MST_EVENTS]++;
                        if (depth == 0) st[MST_EVENT_FIRST_RAY]++;
                    }
                    const v3 x = add(cur.o, scale(t, cur.d));
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
                                final_color = add(final_color, chr_attenuate(Cc, x, shadow.d, srec.t, c, &cells, st, MST_TR_EMITTER));
                        }
                    }
                    if (sky_sampled && med_sky_sample(X->M, ep, env, a, beta_in, m->g, ud, &shadow.d, &c, X->linear)) {
                        nrays++;
                        if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, chr_attenuate(Cc, x, shadow.d, INFINITY, c, &cells, st, MST_TR_ENV));
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
                    const float den = (tr0 + tr1) + tr2;
                    beta = V(beta.e[0] * chr_weight(tr0, den), beta.e[1] * chr_weight(tr1, den), beta.e[2] * chr_weight(tr2, den));
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
                        final_color = add(final_color, chr_attenuate(Cc, rec.point, shadow.d, srec.t, c, &cells, st, MST_TR_EMITTER));
                }
            }
            if (take_env) {
                int pg_zero = 0;
                if (sky_sample_pb(X->M, ep, env, rec.normal, albedo, beta, &B, &shadow.d, &c, X->linear, &pg_zero)) {
                    nrays++;
                    if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, chr_attenuate(Cc, rec.point, shadow.d, INFINITY, c, &cells, st, MST_TR_ENV));
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

static v3 chroma_sample_of(const chroma_ctx *Cc, int i, int j, int s, med_out *out, uint32_t *seeds4, int32_t *cells_out) {
    const lit_ctx *X = &Cc->V.Mc.G.Y.X;
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    uint32_t med = orc_wang_hash(seed ^ RT_MEDIUM_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_chroma(Cc, r, &seed, &nee, &env, &med, out, cells_out);
    if (seeds4) {
        seeds4[0] = seed;
        seeds4[1] = nee;
        seeds4[2] = env;
        seeds4[3] = med;
    }
    return c;
}

/* the handover: 1 = the call is grey — *grey is the volume call that stands for it (sigma_t * e) */
static int chroma_is_grey(const chroma_cfg *cfg, volume_cfg *grey) {
    const float sigma_t = cfg->base.base.medium.sigma_t;
    if (!((cfg->tint[0] == cfg->tint[1] && cfg->tint[1] == cfg->tint[2]) || !(sigma_t > 0.0f))) return 0;
    *grey = cfg->base;
    grey->base.medium.sigma_t = sigma_t * cfg->tint[0];
    return 1;
}

static void make_chroma_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const chroma_cfg *cfg, emit_tab *T, sky_map *M, light_tree *t, int linear,
                            chroma_ctx *Cc) {
    make_volume_ctx(sc, cam, &cfg->base, T, M, t, linear, &Cc->V);
    for (int k = 0; k < 3; ++k) Cc->sigma[k] = Cc->V.Mc.m.sigma_t * cfg->tint[k];
    Cc->V.Mc.m.sigma_t = 1.0f;
}

/* ---- what tests/chroma_reference.py calls -------------------------------------------------------------------------------------------- */
/* The weights alone, on count draws over a homogeneous interval of density length A (sigma: 3 floats each): event 1/0, the three factors
 * on beta, den, and Tr of the sampled channel */
void chroma_weights(int64_t count, const float *u, const float *uc, const float *A, const float *sigma, int32_t *event, float *w, float *den_out, float *trj) {
    for (int64_t r = 0; r < count; ++r) {
        const float *s = sigma + 3 * r;
        int j = (int)(uc[r] * 3.0f);
        if (j > 2) j = 2;
        const float R = s[j] == 0.0f ? INFINITY : -log_ref(u[r]) / s[j];
        event[r] = R < A[r];
        const float a = event[r] ? R : A[r];
        const float tr[3] = {chr_tr(s[0], a), chr_tr(s[1], a), chr_tr(s[2], a)};
        trj[r] = tr[j];
        if (event[r]) {
            const float e0 = s[0] * tr[0], e1 = s[1] * tr[1], e2 = s[2] * tr[2];
            const float den = (e0 + e1) + e2;
            den_out[r] = den;
            w[3 * r] = chr_weight(e0, den);
            w[3 * r + 1] = chr_weight(e1, den);
            w[3 * r + 2] = chr_weight(e2, den);
        } else {
            const float den = (tr[0] + tr[1]) + tr[2];
            den_out[r] = den;
            w[3 * r] = chr_weight(tr[0], den);
            w[3 * r + 1] = chr_weight(tr[1], den);
            w[3 * r + 2] = chr_weight(tr[2], den);
        }
    }
}

/* chr_flight and chr_tr alone on count rays (o, d: 3 floats each) over [0, t_end] to the targets R, as the vertex loop uses them: the base
 * (rho NULL: the homogeneous one; else the grid rho of n: nx, ny, nz, in the box of m) holds sigma_t = 1, sigma is the three channels'
 * sigma_t * tint[k].  hit 1/0 (the interval), event 1/0, its t (0 without one), A (R at an event, the interval's density length otherwise),
 * cells, and tr: chr_tr(sigma[k], A), 3 floats per ray.  An empty interval leaves zeros */
void chroma_flights(const rt_medium_params *m, const float *rho, const int32_t *n, const float *sigma, int64_t count, const float *o, const float *d,
                    const float *t_end, const float *R, int32_t *hit, int32_t *event, float *t, float *A, int32_t *cells, float *tr) {
    volume_ctx Vc;
    memset(&Vc, 0, sizeof(Vc));
    Vc.Mc.m = *m;
    Vc.Mc.m.sigma_t = 1.0f;
    Vc.rho = rho;
    for (int k = 0; k < 3; ++k) Vc.n[k] = rho ? n[k] : 0;
    for (int64_t r = 0; r < count; ++r) {
        const v3 oo = V(o[3 * r], o[3 * r + 1], o[3 * r + 2]), dd = V(d[3 * r], d[3 * r + 1], d[3 * r + 2]);
        float t0, t1;
        event[r] = cells[r] = 0;
        t[r] = A[r] = tr[3 * r] = tr[3 * r + 1] = tr[3 * r + 2] = 0.0f;
        hit[r] = med_interval(&Vc.Mc.m, oo, dd, t_end[r], &t0, &t1, NULL);
        if (!hit[r]) continue;
        const float len = sqrtf(dot(dd, dd));
        float tt = 0.0f, AA = 0.0f;
        event[r] = chr_flight(&Vc, oo, dd, t0, t1, len, R[r], &tt, &AA, &cells[r]);
        if (event[r]) AA = R[r];
        t[r] = event[r] ? tt : 0.0f;
        A[r] = AA;
        for (int k = 0; k < 3; ++k) tr[3 * r + k] = chr_tr(sigma[k], AA);
    }
}

/* count samples (ijs: i, j, s) → volume_trace's columns */
void chroma_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const chroma_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance, int32_t *rays,
                  int32_t *events, int32_t *ends, uint32_t *seeds4, int32_t *cells, int32_t linear) {
    volume_cfg grey;
    if (chroma_is_grey(cfg, &grey)) {
        volume_trace(sc, cam, &grey, count, ijs, radiance, rays, events, ends, seeds4, cells, linear);
        return;
    }
    emit_tab T;
    sky_map M;
    light_tree t;
    chroma_ctx Cc;
    make_chroma_ctx(sc, cam, cfg, &T, &M, &t, linear, &Cc);
    for (int64_t k = 0; k < count; ++k) {
        med_out o;
        const v3 c = chroma_sample_of(&Cc, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &o, seeds4 + 4 * k, &cells[k]);
        memcpy(radiance + 3 * k, c.e, 12);
        rays[k] = o.rays;
        events[k] = o.events;
        ends[k] = o.end;
    }
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base.base, &T, &M);
}

typedef struct {
    const chroma_ctx *Cc;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;
    double *mom;
} chroma_job;

static void *chroma_run(void *arg) {
    chroma_job *jb = (chroma_job *)arg;
    const rt_camera_data *cam = jb->Cc->V.Mc.G.Y.X.cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double mm[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = chroma_sample_of(jb->Cc, i, j, s, NULL, NULL, NULL);
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

/* volume_frame's sums (and moments) under the tint */
void chroma_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const chroma_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads,
                  float *fb, double *mom) {
    volume_cfg grey;
    if (chroma_is_grey(cfg, &grey)) {
        volume_frame(sc, cam, &grey, rows, nrows, sample_first, threads, fb, mom);
        return;
    }
    emit_tab T;
    sky_map M;
    light_tree t;
    chroma_ctx Cc;
    make_chroma_ctx(sc, cam, cfg, &T, &M, &t, 0, &Cc);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    chroma_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        chroma_job jb = {&Cc, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, chroma_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base.base, &T, &M);
}
