/* glow_ref.c — CPU reference of rt_render_glow / rt_trace_samples_glow (include/rtp_amd.h, "emission in the medium").
 * tests/glow_reference.py builds it on its own into a shared library (gcc -ffp-contract=off like the oracle).  It includes volume_ref.c —
 * and through it medium_ref.c and everything of the lit path — for the interval, the medium vertex's light samples, the phase function and
 * the shadow rays' transmittance; it only reads them.  The flight that keeps the emission-weighted length it flew, and the radiance a path
 * ray adds from it, are written here from the header's words, and the vertex loop is volume_ref.c's with those in the place of the grey
 * flight.  No glow (radiance 0, 0, 0) is handed to volume_ref.c's own entry points, as the library hands it to rt_render_volume.
 */
#include "volume_ref.c"

/* what a call is made of (tests/glow_reference.py mirrors this struct) */
typedef struct {
    volume_cfg base;
    int32_t source;          /* 0: h = 1; 1: h_c = rho_c; 2: h_c = heat_c */
    float radiance[3];
    const float *heat;       /* source 2: the volume's dimensions */
} glow_cfg;

typedef struct {
    volume_ctx V;            /* V.rho == NULL: no grid */
    float radiance[3];
    const float *h;          /* NULL: 1 everywhere */
} glow_ctx;

/* The free-flight walk of "density grid" over the non-empty interval [t0, t1] that also keeps E: 1 = an event at *t */
static int glow_walk(const glow_ctx *Gc, v3 o, v3 d, float t0, float t1, float len, float rem, float *t, float *E, int32_t *cells) {
    const volume_ctx *Vc = &Gc->V;
    const rt_medium_params *m = &Vc->Mc.m;
    const int32_t *n = Vc->n;
    int32_t c[3];
    for (int k = 0; k < 3; ++k) {
        const float w = (m->b[k] - m->a[k]) / (float)n[k];
        const float p = o.e[k] + t0 * d.e[k];
        c[k] = (int32_t)floorf((p - m->a[k]) / w);
        if (c[k] < 0) c[k] = 0;
        if (c[k] > n[k] - 1) c[k] = n[k] - 1;
    }
    float ta = t0;
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
        float tb = tm < t1 ? tm : t1;
        if (tb < ta) tb = ta;
        const float seg = (tb - ta) * len;
        const size_t at = ((size_t)c[2] * (size_t)n[1] + (size_t)c[1]) * (size_t)n[0] + (size_t)c[0];
        const float sigma_c = m->sigma_t * Vc->rho[at];
        const float h_c = Gc->h ? Gc->h[at] : 1.0f;
        (*cells)++;
        if (sigma_c > 0.0f) {
            const float s = rem / sigma_c;
            if (s < seg) {
                *E = *E + h_c * s;
                *t = ta + s / len;
                return 1;
            }
            rem = rem - sigma_c * seg;
        }
        *E = *E + h_c * seg;
        if (tb >= t1) break;
        c[axis] += d.e[axis] > 0.0f ? 1 : -1;
        if (c[axis] < 0 || c[axis] >= n[axis]) break;
        ta = tb;
    }
    return 0;
}

/* The free flight of the draw u: 1 = an event at *t.  *E: D without a grid, E with one */
static int glow_flight(const glow_ctx *Gc, v3 o, v3 d, float t0, float t1, float len, float u, float *t, float *E, int32_t *cells) {
    const volume_ctx *Vc = &Gc->V;
    if (!Vc->rho) {
        const float whole = (t1 - t0) * len;
        *E = whole;
        if (u == 0.0f) return 0;
        const float s = -log_ref(u) / Vc->Mc.m.sigma_t;
        if (!(s < whole)) return 0;
        *E = s;
        *t = t0 + s / len;
        return 1;
    }
    *E = 0.0f;
    return glow_walk(Gc, o, d, t0, t1, len, u == 0.0f ? INFINITY : -log_ref(u), t, E, cells);
}

/* Tr * c for a shadow ray: the grey one, with or without the grid */
static v3 glow_attenuate(const glow_ctx *Gc, v3 x, v3 wl, float t_end, v3 c, int32_t *cells, int64_t *st, int which) {
    const volume_ctx *Vc = &Gc->V;
    if (Vc->rho) return vol_attenuate(Vc, x, wl, t_end, c, cells, st, which);
    return med_attenuate(&Vc->Mc.m, x, wl, t_end, c, st, which);
}

/* The path: volume_ref.c's ray_color_volume, restated, with the flight that keeps E and the radiance the medium emitted over it */
static v3 ray_color_glow(const glow_ctx *Gc, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, uint32_t *med, med_out *out, int32_t *cells_out,
                         float *length_out) {
    const volume_ctx *Vc = &Gc->V;
    const medium_ctx *Mc = &Vc->Mc;
    const gloss_ctx *G = &Mc->G;
    const rt_medium_params *m = &Mc->m;
    const tree_ctx *Y = &G->Y;
    const lit_ctx *X = &Y->X;
    const rt_scene_desc *sc = X->sc;
    const rt_camera_data *cam = X->cam;
    const rt_env_params *ep = X->cfg->ep;
    const emit_tab *T = X->T;
    const int emitters_on = T->count > 0;
    const int sky_sampled = X->M && ep->mode != 0 && !X->M->empty && m->region != 0;
    int64_t *st = Mc->stats;
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0, events = 0, cells = 0;
    int carried = 0, end = 1;
    float carry_pb = 0.0f, length = 0.0f;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt, pi;
        nrays++;
        const int hit = closest(sc, &cur, &rec, &pt, &pi);
        /* ---- the segment, the free flight and what the medium emitted over it */
        float t0, t1;
        if (med_interval(m, cur.o, cur.d, hit ? rec.t : INFINITY, &t0, &t1, st)) {
            const float len = sqrtf(dot(cur.d, cur.d));
            const float u = orc_random_float(med);
            float t = 0.0f, E;
            const int flown = glow_flight(Gc, cur.o, cur.d, t0, t1, len, u, &t, &E, &cells);
            length = length + E;
            if (Vc->rho || E < INFINITY)
                final_color = add(final_color, V(beta.e[0] * (Gc->radiance[0] * E), beta.e[1] * (Gc->radiance[1] * E), beta.e[2] * (Gc->radiance[2] * E)));
            if (flown) {
                /* ---- the medium vertex */
                events++;
                const v3 x = add(cur.o, scale(t, cur.d));
                const v3 ud = unit(cur.d);
                const v3 beta_in = beta;
                const v3 a = V(m->albedo[0], m->albedo[1], m->albedo[2]);
                beta = mulv(beta, a);
                if (beta.e[0] == 0.0f && beta.e[1] == 0.0f && beta.e[2] == 0.0f) {
                    end = 3;
                    break;
                }
                if (!(depth + 1 < cam->max_depth)) break;
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
                            final_color = add(final_color, glow_attenuate(Gc, x, shadow.d, srec.t, c, &cells, st, MST_TR_EMITTER));
                    }
                }
                if (sky_sampled && med_sky_sample(X->M, ep, env, a, beta_in, m->g, ud, &shadow.d, &c, X->linear)) {
                    nrays++;
                    if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, glow_attenuate(Gc, x, shadow.d, INFINITY, c, &cells, st, MST_TR_ENV));
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
        /* ---- no event: rt_render_lit's vertex, as in medium_ref.c */
        if (!hit) {
            end = 0;
            if (!X->M || (depth == 0 && !ep->camera_visible)) {
                final_color = add(final_color, mulv(beta, from_rt(cam->background)));
                break;
            }
            v3 p;
            const int32_t tx = texel_of(to_env(ep, cur.d), X->M->n, &p);
            v3 term = mulv(beta, scaled(X->M, ep, tx));
            const int weighted = carried == 1 || carried == 3 || (carried == 2 && G->glossy_env && carry_pb != 0.0f);
            if (weighted && sky_sampled) {
                const float pb = carried == 1 ? RT_NEE_PB : carry_pb;
                const float q2 = dot(p, p);
                const float pl = pl_of(X->M, tx, q2, sqrtf(q2));
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
                    const float ue = orc_random_float(nee);
                    e = 0;
                    while (e < T->count && !(ue < T->cdf[e])) ++e;
                    if (e < T->count) pmf = T->pmf[e];
                }
                int pg_zero = 0;
                if (e < T->count && entry_sample_pb(sc, T, e, pmf, nee, rec.point, rec.normal, albedo, beta, &B, &shadow.d, &c, &pg_zero)) {
                    nrays++;
                    const int sh = closest(sc, &shadow, &srec, &spt, &spi);
                    if (sh && spt == T->kind[e] && spi == T->index[e])
                        final_color = add(final_color, glow_attenuate(Gc, rec.point, shadow.d, srec.t, c, &cells, st, MST_TR_EMITTER));
                }
            }
            if (take_env) {
                int pg_zero = 0;
                if (sky_sample_pb(X->M, ep, env, rec.normal, albedo, beta, &B, &shadow.d, &c, X->linear, &pg_zero)) {
                    nrays++;
                    if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, glow_attenuate(Gc, rec.point, shadow.d, INFINITY, c, &cells, st, MST_TR_ENV));
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
    if (length_out) *length_out = length;
    return final_color;
}

static v3 glow_sample_of(const glow_ctx *Gc, int i, int j, int s, med_out *out, uint32_t *seeds4, int32_t *cells_out, float *length_out) {
    const lit_ctx *X = &Gc->V.Mc.G.Y.X;
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    uint32_t med = orc_wang_hash(seed ^ RT_MEDIUM_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_glow(Gc, r, &seed, &nee, &env, &med, out, cells_out, length_out);
    if (seeds4) {
        seeds4[0] = seed;
        seeds4[1] = nee;
        seeds4[2] = env;
        seeds4[3] = med;
    }
    return c;
}

/* the handover: 1 = no glow — the call is the volume call with the same arguments */
static int glow_is_dark(const glow_cfg *cfg) { return cfg->radiance[0] == 0.0f && cfg->radiance[1] == 0.0f && cfg->radiance[2] == 0.0f; }

static void make_glow_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const glow_cfg *cfg, emit_tab *T, sky_map *M, light_tree *t, int linear, glow_ctx *Gc) {
    make_volume_ctx(sc, cam, &cfg->base, T, M, t, linear, &Gc->V);
    for (int k = 0; k < 3; ++k) Gc->radiance[k] = cfg->radiance[k];
    Gc->h = cfg->source == 0 ? NULL : (cfg->source == 1 ? cfg->base.rho : cfg->heat);
}

/* ---- what tests/glow_reference.py calls ---------------------------------------------------------------------------------------------- */
/* glow_flight alone on count rays (o, d: 3 floats each) over [0, t_end] with the draws u: the base is the homogeneous one (rho NULL) or the
 * grid rho of n (nx, ny, nz) in the box of m, h the cells' emission (NULL: 1).  hit 1/0 (the interval), event 1/0, its t (0 without one), E
 * and cells.  An empty interval leaves zeros */
void glow_flights(const rt_medium_params *m, const float *rho, const float *h, const int32_t *n, int64_t count, const float *o, const float *d, const float *t_end,
                  const float *u, int32_t *hit, int32_t *event, float *t, float *E, int32_t *cells) {
    glow_ctx Gc;
    memset(&Gc, 0, sizeof(Gc));
    Gc.V.Mc.m = *m;
    Gc.V.rho = rho;
    Gc.h = h;
    for (int k = 0; k < 3; ++k) Gc.V.n[k] = rho ? n[k] : 0;
    for (int64_t r = 0; r < count; ++r) {
        const v3 oo = V(o[3 * r], o[3 * r + 1], o[3 * r + 2]), dd = V(d[3 * r], d[3 * r + 1], d[3 * r + 2]);
        float t0, t1;
        event[r] = cells[r] = 0;
        t[r] = E[r] = 0.0f;
        hit[r] = med_interval(m, oo, dd, t_end[r], &t0, &t1, NULL);
        if (!hit[r]) continue;
        const float len = sqrtf(dot(dd, dd));
        float tt = 0.0f, EE = 0.0f;
        event[r] = glow_flight(&Gc, oo, dd, t0, t1, len, u[r], &tt, &EE, &cells[r]);
        t[r] = event[r] ? tt : 0.0f;
        E[r] = EE;
    }
}

/* count samples (ijs: i, j, s) → volume_trace's columns and glow_length per sample */
void glow_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const glow_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance, int32_t *rays,
                int32_t *events, int32_t *ends, uint32_t *seeds4, int32_t *cells, float *glow_length, int32_t linear) {
    if (glow_is_dark(cfg)) {
        volume_trace(sc, cam, &cfg->base, count, ijs, radiance, rays, events, ends, seeds4, cells, linear);
        for (int64_t k = 0; k < count; ++k) glow_length[k] = 0.0f;
        return;
    }
    emit_tab T;
    sky_map M;
    light_tree t;
    glow_ctx Gc;
    make_glow_ctx(sc, cam, cfg, &T, &M, &t, linear, &Gc);
    for (int64_t k = 0; k < count; ++k) {
        med_out o;
        const v3 c = glow_sample_of(&Gc, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &o, seeds4 + 4 * k, &cells[k], &glow_length[k]);
        memcpy(radiance + 3 * k, c.e, 12);
        rays[k] = o.rays;
        events[k] = o.events;
        ends[k] = o.end;
    }
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base.base, &T, &M);
}

typedef struct {
    const glow_ctx *Gc;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;
    double *mom;
} glow_job;

static void *glow_run(void *arg) {
    glow_job *jb = (glow_job *)arg;
    const rt_camera_data *cam = jb->Gc->V.Mc.G.Y.X.cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double mm[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = glow_sample_of(jb->Gc, i, j, s, NULL, NULL, NULL, NULL);
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

/* volume_frame's sums (and moments) under the glow */
void glow_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const glow_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads, float *fb,
                double *mom) {
    if (glow_is_dark(cfg)) {
        volume_frame(sc, cam, &cfg->base, rows, nrows, sample_first, threads, fb, mom);
        return;
    }
    emit_tab T;
    sky_map M;
    light_tree t;
    glow_ctx Gc;
    make_glow_ctx(sc, cam, cfg, &T, &M, &t, 0, &Gc);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    glow_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        glow_job jb = {&Gc, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, glow_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base.base, &T, &M);
}
