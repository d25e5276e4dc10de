/* glow_sample_ref.c — CPU reference of rt_render_glow_sampled / rt_trace_samples_glow_sampled and of rt_glow_sampler's table
 * (include/rtp_amd.h, "light samples of the glow").  tests/glow_sample_reference.py builds it on its own into a shared
 * library (gcc -ffp-contract=off like the oracle).  It includes glow_ref.c — and through it everything of the fog path — for the flight that
 * keeps E, the medium vertex's pieces and the shadow rays' transmittance; it only reads them.  The table, the pick, the two walk quantities
 * (glow_pl, glow_line), the light sample, the path ray's weight and the third shadow ray are written here from the header's words, and the
 * vertex loop is glow_ref.c's with those added.  What the library hands over to rt_render_glow is handed to glow_ref.c's entry points.
 * gs_pl_d and gs_line_d state the two sums in float64 over the cells of the same float32 walk, for the tests of the rounding.
 */
#include "glow_ref.c"

/* what a call is made of (tests/glow_sample_reference.py mirrors this struct) */
typedef struct {
    glow_cfg base;
    int32_t sample, mis;
} glow_sample_cfg;

/* ---- the table, by the header's contract ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n[3];
    float *slab_cdf, *row_cdf, *cell_cdf, *pc;
    int empty;
} gs_table;

static void gs_cdf(const double *value, size_t stride, int32_t n, double sum, float *cdf) {
    double run = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        run += value[(size_t)k * stride];
        cdf[k] = sum > 0.0 ? (float)(run / sum) : 0.0f;
    }
    if (sum > 0.0) cdf[n - 1] = 1.0f;
}
static float gs_pmf(const float *cdf, int32_t k) { return cdf[k] - (k == 0 ? 0.0f : cdf[k - 1]); }

/* h: NULL = 1 everywhere (source 0), else nx * ny * nz values */
static void gs_make_table(const float *h, int32_t nx, int32_t ny, int32_t nz, gs_table *T) {
    const size_t rows = (size_t)nz * (size_t)ny, count = rows * (size_t)nx;
    T->n[0] = nx;
    T->n[1] = ny;
    T->n[2] = nz;
    T->slab_cdf = (float *)malloc((size_t)nz * 4);
    T->row_cdf = (float *)malloc(rows * 4);
    T->cell_cdf = (float *)malloc(count * 4);
    T->pc = (float *)malloc(count * 4);
    double *hd = (double *)malloc(count * 8), *row_sum = (double *)calloc(rows, 8), *slab_sum = (double *)calloc((size_t)nz, 8);
    double total = 0.0;
    for (size_t c = 0; c < count; ++c) hd[c] = h ? (double)h[c] : 1.0;
    for (size_t r = 0; r < rows; ++r)
        for (int32_t x = 0; x < nx; ++x) row_sum[r] += hd[r * (size_t)nx + (size_t)x];
    for (int32_t z = 0; z < nz; ++z) {
        for (int32_t y = 0; y < ny; ++y) slab_sum[z] += row_sum[(size_t)z * (size_t)ny + (size_t)y];
        total += slab_sum[z];
    }
    gs_cdf(slab_sum, 1, nz, total, T->slab_cdf);
    for (int32_t z = 0; z < nz; ++z) gs_cdf(row_sum + (size_t)z * (size_t)ny, 1, ny, slab_sum[z], T->row_cdf + (size_t)z * (size_t)ny);
    for (size_t r = 0; r < rows; ++r) gs_cdf(hd + r * (size_t)nx, 1, nx, row_sum[r], T->cell_cdf + r * (size_t)nx);
    for (int32_t z = 0; z < nz; ++z)
        for (int32_t y = 0; y < ny; ++y) {
            const size_t r = (size_t)z * (size_t)ny + (size_t)y;
            const float sr = gs_pmf(T->slab_cdf, z) * gs_pmf(T->row_cdf + (size_t)z * (size_t)ny, y);
            for (int32_t x = 0; x < nx; ++x) T->pc[r * (size_t)nx + (size_t)x] = sr * gs_pmf(T->cell_cdf + r * (size_t)nx, x);
        }
    T->empty = !(total > 0.0);
    free(hd);
    free(row_sum);
    free(slab_sum);
}
static void gs_free_table(gs_table *T) {
    free(T->slab_cdf);
    free(T->row_cdf);
    free(T->cell_cdf);
    free(T->pc);
}
/* the smallest e in [0, n) with u < cdf[e]; n when there is none */
static int32_t gs_pick(const float *cdf, int32_t n, float u) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

/* ---- the walk, cell for cell, with what a cell does left to the caller ------------------------------------------------------------------- */
typedef void (*gs_cell_fn)(void *ctx, size_t at, float ta, float tb);
static void gs_cells(const rt_medium_params *m, const int32_t *n, v3 o, v3 d, float t0, float t1, int32_t *cells, gs_cell_fn fn, void *ctx) {
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
        (*cells)++;
        fn(ctx, ((size_t)c[2] * (size_t)n[1] + (size_t)c[1]) * (size_t)n[0] + (size_t)c[0], ta, tb);
        if (tb >= t1) break;
        c[axis] += d.e[axis] > 0.0f ? 1 : -1;
        if (c[axis] < 0 || c[axis] >= n[axis]) break;
        ta = tb;
    }
}

/* what the two quantities read: the medium, the grid, h (NULL: 1) and the table's pc */
typedef struct {
    const rt_medium_params *m;
    const int32_t *n;
    const float *rho, *h, *pc;
} gs_grid;

typedef struct {
    const gs_grid *g;
    float len, q, Tr, G;
    double lend, qd, Trd, Gd;
    int32_t series, closed;          /* cells of a glow_line walk that took the series (x < 0.0625) and the closed form */
} gs_acc;
static void gs_pl_cell(void *ctx, size_t at, float ta, float tb) {
    gs_acc *A = (gs_acc *)ctx;
    const float seg = (tb - ta) * A->len;
    const float ra = ta * A->len, rb = tb * A->len;
    A->q = A->q + A->g->pc[at] * (seg * ((rb * rb + rb * ra) + ra * ra));
}
static void gs_pl_cell_d(void *ctx, size_t at, float ta, float tb) {
    gs_acc *A = (gs_acc *)ctx;
    const double ra = (double)ta * A->lend, rb = (double)tb * A->lend;
    A->qd += (double)A->g->pc[at] * (rb * rb * rb - ra * ra * ra);
}
static void gs_line_cell(void *ctx, size_t at, float ta, float tb) {
    gs_acc *A = (gs_acc *)ctx;
    const float seg = (tb - ta) * A->len;
    const float sigma_c = A->g->m->sigma_t * A->g->rho[at];
    const float h_c = A->g->h ? A->g->h[at] : 1.0f;
    const float x = sigma_c * seg;
    const float e = expf(-x);
    const float m = x < 0.0625f ? seg * (1.0f - x * (0.5f - x * (1.0f / 6.0f - x * (1.0f / 24.0f)))) : (1.0f - e) / sigma_c;
    if (x < 0.0625f) A->series++;
    else A->closed++;
    A->G = A->G + A->Tr * (h_c * m);
    A->Tr = A->Tr * e;
}
static void gs_line_cell_d(void *ctx, size_t at, float ta, float tb) {
    gs_acc *A = (gs_acc *)ctx;
    const double seg = ((double)tb - (double)ta) * A->lend;
    const double sigma_c = (double)A->g->m->sigma_t * (double)A->g->rho[at];
    const double h_c = A->g->h ? (double)A->g->h[at] : 1.0;
    const double x = sigma_c * seg;
    const double m = sigma_c > 0.0 ? -expm1(-x) / sigma_c : seg;
    A->Gd += A->Trd * (h_c * m);
    A->Trd *= exp(-x);
}
static float gs_inv3v(const gs_grid *g) {
    const float wx = (g->m->b[0] - g->m->a[0]) / (float)g->n[0], wy = (g->m->b[1] - g->m->a[1]) / (float)g->n[1], wz = (g->m->b[2] - g->m->a[2]) / (float)g->n[2];
    return 1.0f / (3.0f * ((wx * wy) * wz));
}
/* glow_pl(o, d) of the header */
static float gs_pl(const gs_grid *g, v3 o, v3 d, int32_t *cells) {
    float t0, t1;
    if (!med_interval(g->m, o, d, INFINITY, &t0, &t1, NULL)) return 0.0f;
    gs_acc A;
    A.g = g;
    A.len = sqrtf(dot(d, d));
    A.q = 0.0f;
    gs_cells(g->m, g->n, o, d, t0, t1, cells, gs_pl_cell, &A);
    return A.q * gs_inv3v(g);
}
/* the same sum in float64 over the same cells (the cells' widths in float64 too) */
static double gs_pl_d(const gs_grid *g, v3 o, v3 d) {
    float t0, t1;
    int32_t cells = 0;
    if (!med_interval(g->m, o, d, INFINITY, &t0, &t1, NULL)) return 0.0;
    gs_acc A;
    A.g = g;
    A.lend = sqrt((double)d.e[0] * d.e[0] + (double)d.e[1] * d.e[1] + (double)d.e[2] * d.e[2]);
    A.qd = 0.0;
    gs_cells(g->m, g->n, o, d, t0, t1, &cells, gs_pl_cell_d, &A);
    double v = 1.0;
    for (int k = 0; k < 3; ++k) v *= ((double)g->m->b[k] - (double)g->m->a[k]) / (double)g->n[k];
    return A.qd / (3.0 * v);
}
/* glow_line(o, d, t_end) of the header: 0 = an empty interval.  branches: NULL, or two counts that the walk's cells are added to — those
 * with x < 0.0625 (the series) and the others (the closed form) */
static int gs_line(const gs_grid *g, v3 o, v3 d, float t_end, float *G, int32_t *cells, int32_t *branches) {
    float t0, t1;
    *G = 0.0f;
    if (!med_interval(g->m, o, d, t_end, &t0, &t1, NULL)) return 0;
    gs_acc A;
    A.g = g;
    A.len = sqrtf(dot(d, d));
    A.Tr = 1.0f;
    A.G = 0.0f;
    A.series = A.closed = 0;
    gs_cells(g->m, g->n, o, d, t0, t1, cells, gs_line_cell, &A);
    *G = A.G;
    if (branches) {
        branches[0] += A.series;
        branches[1] += A.closed;
    }
    return 1;
}
static double gs_line_d(const gs_grid *g, v3 o, v3 d, float t_end) {
    float t0, t1;
    int32_t cells = 0;
    if (!med_interval(g->m, o, d, t_end, &t0, &t1, NULL)) return 0.0;
    gs_acc A;
    A.g = g;
    A.lend = sqrt((double)d.e[0] * d.e[0] + (double)d.e[1] * d.e[1] + (double)d.e[2] * d.e[2]);
    A.Trd = 1.0;
    A.Gd = 0.0;
    gs_cells(g->m, g->n, o, d, t0, t1, &cells, gs_line_cell_d, &A);
    return A.Gd;
}

/* ---- the light sample --------------------------------------------------------------------------------------------------------------------- */
/* the BSDF strategy's density at a vertex: kind 0 a diffuse event (the constant), 1 a glossy one (pg about B's mirror direction), 2 a medium
 * vertex (ph about ud) */
typedef struct {
    int kind;
    const bsdf_pb *B;
    float g;
    v3 ud;
} gs_pb;
/* six draws of med: the cell (its coordinates in cell[3], when not NULL), the point, the direction.  0: no sample.  normal: read at kinds 0 and 1 */
static int gs_sample(const gs_grid *g, const gs_table *T, int mis, uint32_t *med, v3 x, v3 normal, const gs_pb *PB, v3 *dir_out, float *f, float *pl_out,
                     int32_t *cell, int32_t *cells) {
    const rt_medium_params *m = g->m;
    const int32_t *n = g->n;
    const float us = orc_random_float(med);
    const float ur = orc_random_float(med);
    const float uc = orc_random_float(med);
    const float ux = orc_random_float(med);
    const float uy = orc_random_float(med);
    const float uz = orc_random_float(med);
    if (cell) cell[0] = cell[1] = cell[2] = -1;
    const int32_t z = gs_pick(T->slab_cdf, n[2], us);
    if (z >= n[2]) return 0;
    const int32_t y = gs_pick(T->row_cdf + (size_t)z * (size_t)n[1], n[1], ur);
    if (y >= n[1]) return 0;
    const int32_t c = gs_pick(T->cell_cdf + ((size_t)z * (size_t)n[1] + (size_t)y) * (size_t)n[0], n[0], uc);
    if (c >= n[0]) return 0;
    if (cell) {
        cell[0] = c;
        cell[1] = y;
        cell[2] = z;
    }
    const float wx = (m->b[0] - m->a[0]) / (float)n[0], wy = (m->b[1] - m->a[1]) / (float)n[1], wz = (m->b[2] - m->a[2]) / (float)n[2];
    const v3 p = V(m->a[0] + ((float)c + ux) * wx, m->a[1] + ((float)y + uy) * wy, m->a[2] + ((float)z + uz) * wz);
    const v3 dir = sub(p, x);
    const float d2 = dot(dir, dir);
    if (d2 == 0.0f) return 0;
    if (PB->kind != 2 && !(dot(dir, normal) > 0.0f)) return 0;
    const float l = sqrtf(d2);
    const v3 wl = V(dir.e[0] / l, dir.e[1] / l, dir.e[2] / l);
    const float pb = PB->kind == 0 ? RT_NEE_PB : (PB->kind == 1 ? pb_of(PB->B, wl) : med_pb(PB->g, PB->ud, wl));
    if (PB->kind != 0 && pb == 0.0f) return 0;
    const float pl = gs_pl(g, x, dir, cells);
    if (pl_out) *pl_out = pl;
    if (!(pl > 0.0f)) return 0;
    *f = mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *dir_out = dir;
    return 1;
}

typedef struct {
    glow_ctx Gc;
    gs_grid g;
    gs_table T;
    int mis;
} gs_ctx;

/* the sample's shadow ray, a full closest-hit query, and what it adds: 1 = a ray was traced */
static void gs_shadow(const gs_ctx *Sc, v3 x, v3 dir, float f, v3 ba, v3 *final_color, int32_t *cells) {
    const rt_scene_desc *sc = Sc->Gc.V.Mc.G.Y.X.sc;
    hitrec srec;
    int spt, spi;
    ray shadow;
    shadow.o = x;
    shadow.d = dir;
    const int sh = closest(sc, &shadow, &srec, &spt, &spi);
    float G;
    if (!gs_line(&Sc->g, x, dir, sh ? srec.t : INFINITY, &G, cells, NULL)) return;
    const float *r = Sc->Gc.radiance;
    *final_color = add(*final_color, V(ba.e[0] * (f * (r[0] * G)), ba.e[1] * (f * (r[1] * G)), ba.e[2] * (f * (r[2] * G))));
}

/* The path: glow_ref.c's ray_color_glow, restated, with the glow's light sample, its shadow ray and the path ray's weight */
static v3 ray_color_glow_sampled(const gs_ctx *Sc, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, uint32_t *med, med_out *out, int32_t *cells_out,
                                 float *length_out, int32_t *shots_out) {
    const glow_ctx *Gc = &Sc->Gc;
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
    const int glossy_glow = G->glossy_nee && X->cfg->sample_emitters;          /* the emitters' glossy switch, with or without an emitter */
    int64_t *st = Mc->stats;
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0, events = 0, cells = 0, shots = 0;
    int carried = 0, end = 1;
    float carry_pb = 0.0f, length = 0.0f;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt, pi;
        nrays++;
        const int hit = closest(sc, &cur, &rec, &pt, &pi);
        /* ---- the segment, the free flight and what the medium emitted over it, weighted against the light sample of the vertex behind */
        float t0, t1;
        if (med_interval(m, cur.o, cur.d, hit ? rec.t : INFINITY, &t0, &t1, st)) {
            const float len = sqrtf(dot(cur.d, cur.d));
            const float u = orc_random_float(med);
            float t = 0.0f, E;
            const int flown = glow_flight(Gc, cur.o, cur.d, t0, t1, len, u, &t, &E, &cells);
            length = length + E;
            v3 term = V(beta.e[0] * (Gc->radiance[0] * E), beta.e[1] * (Gc->radiance[1] * E), beta.e[2] * (Gc->radiance[2] * E));
            const float pbw = carried == 1 ? RT_NEE_PB : (carried == 3 || (carried == 2 && glossy_glow) ? carry_pb : 0.0f);
            if (pbw != 0.0f) {
                const float pl = gs_pl(&Sc->g, cur.o, cur.d, &cells);
                const float wb = Sc->mis ? (pbw * pbw) / (pbw * pbw + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                term = scale(wb, term);
            }
            final_color = add(final_color, term);
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
                /* the glow's sample, behind the next direction's draws */
                gs_pb PB;
                PB.kind = 2;
                PB.B = NULL;
                PB.g = m->g;
                PB.ud = ud;
                v3 gdir;
                float gf;
                if (gs_sample(&Sc->g, &Sc->T, Sc->mis, med, x, ud, &PB, &gdir, &gf, NULL, NULL, &cells)) {
                    nrays++;
                    shots++;
                    gs_shadow(Sc, x, gdir, gf, mulv(beta_in, a), &final_color, &cells);
                }
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
        int take_nee = 0, take_env = 0, take_glow = 0;
        bsdf_pb B;
        B.glossy = 0;
        B.r = reflected;
        B.fuzz = mat->fuzz;
        if (depth + 1 < cam->max_depth) {
            if (event == 1 && ok) {
                take_nee = emitters_on;
                take_env = sky_sampled;
                take_glow = 1;
            } else if (event == 2 && mat->fuzz >= RT_GLOSSY_MIN_FUZZ) {
                take_nee = emitters_on && G->glossy_nee;
                take_env = sky_sampled && G->glossy_env;
                take_glow = glossy_glow;
                B.glossy = 1;
            }
        }
        const int glossy_event = B.glossy && (take_nee || take_env || take_glow);
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
        if (take_glow) {
            gs_pb PB;
            PB.kind = B.glossy ? 1 : 0;
            PB.B = &B;
            PB.g = 0.0f;
            PB.ud = V(0, 0, 0);
            v3 gdir;
            float gf;
            if (gs_sample(&Sc->g, &Sc->T, Sc->mis, med, rec.point, rec.normal, &PB, &gdir, &gf, NULL, NULL, &cells)) {
                nrays++;
                shots++;
                gs_shadow(Sc, rec.point, gdir, gf, mulv(beta, albedo), &final_color, &cells);
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
    if (shots_out) *shots_out = shots;
    return final_color;
}

static v3 gs_sample_of(const gs_ctx *Sc, int i, int j, int s, med_out *out, uint32_t *seeds4, int32_t *cells_out, float *length_out, int32_t *shots_out) {
    const lit_ctx *X = &Sc->Gc.V.Mc.G.Y.X;
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    uint32_t med = orc_wang_hash(seed ^ RT_MEDIUM_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_glow_sampled(Sc, r, &seed, &nee, &env, &med, out, cells_out, length_out, shots_out);
    if (seeds4) {
        seeds4[0] = seed;
        seeds4[1] = nee;
        seeds4[2] = env;
        seeds4[3] = med;
    }
    return c;
}

/* the table of a call's grids */
static void gs_table_of(const glow_cfg *cfg, gs_table *T) {
    const float *h = cfg->source == 0 ? NULL : (cfg->source == 1 ? cfg->base.rho : cfg->heat);
    gs_make_table(h, cfg->base.nx, cfg->base.ny, cfg->base.nz, T);
}
/* the handover: 1 = the call is the glow call with the same arguments (T is made either way, for a grid) */
static int gs_hands_over(const glow_sample_cfg *cfg, gs_table *T) {
    T->slab_cdf = T->row_cdf = T->cell_cdf = T->pc = NULL;
    T->empty = 1;
    if (cfg->sample == 0 || !cfg->base.base.rho) return 1;
    gs_table_of(&cfg->base, T);
    return T->empty || glow_is_dark(&cfg->base);
}
static void gs_make_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const glow_sample_cfg *cfg, emit_tab *T, sky_map *M, light_tree *t, int linear,
                        gs_ctx *Sc) {
    make_glow_ctx(sc, cam, &cfg->base, T, M, t, linear, &Sc->Gc);
    Sc->g.m = &Sc->Gc.V.Mc.m;
    Sc->g.n = Sc->Gc.V.n;
    Sc->g.rho = Sc->Gc.V.rho;
    Sc->g.h = Sc->Gc.h;
    Sc->g.pc = Sc->T.pc;
    Sc->mis = cfg->mis;
}

/* ---- what tests/glow_sample_reference.py calls ------------------------------------------------------------------------------------------- */
/* the whole table of a grid's h (NULL: 1 everywhere): slab_cdf (nz), row_cdf (nz * ny), cell_cdf and pc (nz * ny * nx); returns empty */
int32_t glow_sample_table(const float *h, int32_t nx, int32_t ny, int32_t nz, float *slab_cdf, float *row_cdf, float *cell_cdf, float *pc) {
    gs_table T;
    gs_make_table(h, nx, ny, nz, &T);
    const size_t rows = (size_t)nz * (size_t)ny;
    memcpy(slab_cdf, T.slab_cdf, (size_t)nz * 4);
    memcpy(row_cdf, T.row_cdf, rows * 4);
    memcpy(cell_cdf, T.cell_cdf, rows * (size_t)nx * 4);
    memcpy(pc, T.pc, rows * (size_t)nx * 4);
    const int32_t empty = T.empty;
    gs_free_table(&T);
    return empty;
}

/* glow_pl (float32 and the float64 sum over the same cells) of count rays (o, d) */
void glow_sample_pl(const rt_medium_params *m, const float *rho, const float *h, const int32_t *n3, int64_t count, const float *o, const float *d, float *pl,
                    double *pl_d) {
    gs_table T;
    gs_make_table(h, n3[0], n3[1], n3[2], &T);
    const gs_grid g = {m, n3, rho, h, T.pc};
    for (int64_t k = 0; k < count; ++k) {
        int32_t cells = 0;
        const v3 oo = V(o[3 * k], o[3 * k + 1], o[3 * k + 2]), dd = V(d[3 * k], d[3 * k + 1], d[3 * k + 2]);
        pl[k] = gs_pl(&g, oo, dd, &cells);
        if (pl_d) pl_d[k] = gs_pl_d(&g, oo, dd);
    }
    gs_free_table(&T);
}

/* glow_line (float32 and float64 over the same cells) of count rays (o, d) up to t_end; branches: two counts over all the rays' cells,
 * those whose x = sigma_c * seg took the series and those that took the closed form */
void glow_sample_line(const rt_medium_params *m, const float *rho, const float *h, const int32_t *n3, int64_t count, const float *o, const float *d,
                      const float *t_end, float *G, double *G_d, int32_t *branches) {
    const gs_grid g = {m, n3, rho, h, NULL};
    branches[0] = branches[1] = 0;
    for (int64_t k = 0; k < count; ++k) {
        int32_t cells = 0;
        const v3 oo = V(o[3 * k], o[3 * k + 1], o[3 * k + 2]), dd = V(d[3 * k], d[3 * k + 1], d[3 * k + 2]);
        gs_line(&g, oo, dd, t_end[k], &G[k], &cells, branches);
        G_d[k] = gs_line_d(&g, oo, dd, t_end[k]);
    }
}

/* count light samples of a vertex at x without a hemisphere and with a constant pb (a medium vertex under g = 0), from the oracle's generator
 * started at seed: the picked cell (x, y, z; -1: the pick found nothing), whether a sample came of it, its direction and pl */
void glow_sample_draws(const rt_medium_params *m, const float *rho, const float *h, const int32_t *n3, const float *x, uint32_t seed, int64_t count,
                       int32_t *cell, int32_t *taken, float *dir, float *pl) {
    gs_table T;
    gs_make_table(h, n3[0], n3[1], n3[2], &T);
    const gs_grid g = {m, n3, rho, h, T.pc};
    gs_pb PB;
    PB.kind = 2;
    PB.B = NULL;
    PB.g = 0.0f;
    PB.ud = V(0.0f, 0.0f, 1.0f);
    uint32_t med = seed;
    for (int64_t k = 0; k < count; ++k) {
        int32_t cells = 0;
        v3 dd = V(0, 0, 0);
        float f = 0.0f;
        pl[k] = 0.0f;
        taken[k] = gs_sample(&g, &T, 1, &med, V(x[0], x[1], x[2]), V(0, 0, 0), &PB, &dd, &f, &pl[k], cell + 3 * k, &cells);
        memcpy(dir + 3 * k, dd.e, 12);
    }
    gs_free_table(&T);
}

/* count samples (ijs: i, j, s) → glow_trace's columns and glow_samples per sample */
void glow_sample_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const glow_sample_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance,
                       int32_t *rays, int32_t *events, int32_t *ends, uint32_t *seeds4, int32_t *cells, float *glow_length, int32_t *glow_samples,
                       int32_t linear) {
    gs_ctx Sc;
    if (gs_hands_over(cfg, &Sc.T)) {
        glow_trace(sc, cam, &cfg->base, count, ijs, radiance, rays, events, ends, seeds4, cells, glow_length, linear);
        for (int64_t k = 0; k < count; ++k) glow_samples[k] = 0;
        gs_free_table(&Sc.T);
        return;
    }
    emit_tab T;
    sky_map M;
    light_tree t;
    gs_make_ctx(sc, cam, cfg, &T, &M, &t, linear, &Sc);
    for (int64_t k = 0; k < count; ++k) {
        med_out o;
        const v3 c = gs_sample_of(&Sc, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &o, seeds4 + 4 * k, &cells[k], &glow_length[k], &glow_samples[k]);
        memcpy(radiance + 3 * k, c.e, 12);
        rays[k] = o.rays;
        events[k] = o.events;
        ends[k] = o.end;
    }
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base.base.base, &T, &M);
    gs_free_table(&Sc.T);
}

typedef struct {
    const gs_ctx *Sc;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;
    double *mom;
} gs_job;

static void *gs_run(void *arg) {
    gs_job *jb = (gs_job *)arg;
    const rt_camera_data *cam = jb->Sc->Gc.V.Mc.G.Y.X.cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double mm[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = gs_sample_of(jb->Sc, i, j, s, NULL, NULL, NULL, NULL, NULL);
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

/* glow_frame's sums (and moments) with the light samples */
void glow_sample_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const glow_sample_cfg *cfg, const int32_t *rows, int nrows, int sample_first,
                       int threads, float *fb, double *mom) {
    gs_ctx Sc;
    if (gs_hands_over(cfg, &Sc.T)) {
        glow_frame(sc, cam, &cfg->base, rows, nrows, sample_first, threads, fb, mom);
        gs_free_table(&Sc.T);
        return;
    }
    emit_tab T;
    sky_map M;
    light_tree t;
    gs_make_ctx(sc, cam, cfg, &T, &M, &t, 0, &Sc);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    gs_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        gs_job jb = {&Sc, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, gs_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_tree(&t);
    free_ctx(&cfg->base.base.base.base.base.base, &T, &M);
    gs_free_table(&Sc.T);
}
