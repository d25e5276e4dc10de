/* emit_ref.c — CPU reference of rt_render_lit / rt_trace_samples_lit with rt_nee_params.sample_planes (DESIGN.md §17;
 * tests/emit_reference.py builds it on its own into a shared library, gcc -ffp-contract=off like the oracle); rt_render_nee is its pinhole
 * case without an environment.  The oracle's ray_color and hit_bvh are static: this file includes oracle/rt_oracle.c to reach them.
 *
 * The emitter table has a kind column: the spheres, then — sample_planes = 1 — the emissive QUAD, ELLIPSE and TRIANGLE planes, which are
 * sampled uniformly in area (steps 2p … 4p) and weighted when a BSDF ray from a diffuse event finds them.
 *
 * include/rtp_amd.h's contract for emitters, environment and lens in one frame, restated from its words: the camera ray of
 * rt_render_lens (ox, oy, tau, the lens point); the path is ray_color's, draw for draw, from the state the camera leaves; two light
 * streams that start as in the single calls; at a vertex the emission or miss term first (a table sphere after a diffuse event
 * weighted, a miss looked up in the map and weighted after a diffuse event), then the emitter's light sample, then the environment's.
 */
#include "../../oracle/rt_oracle.c"
#include "../../include/rtp_amd.h"

#include <math.h>
#include <pthread.h>

/* what a call is made of (tests/emit_reference.py mirrors this struct) */
typedef struct {
    const rt_camera_data *cam_close;   /* NULL: no motion */
    float lens_radius, focus_distance;
    int32_t sample_emitters, nee_mis, sample_planes;
    const float *rgb;                  /* NULL: no environment */
    int32_t n;
    const rt_env_params *ep;           /* read when rgb != NULL */
} lit_cfg;

/* ---- the emitter table: a kind column (0 sphere, 1 plane), spheres first, then planes ------------------------------------------ */
typedef struct {
    int32_t *kind, *index;
    float *cdf, *pmf, *area;
    int32_t count, mis;
} emit_tab;

/* the sum of a material's emit components in double, or -1 when it is no light's (a component negative or not finite, or all 0) */
static double emit_sum(const rt_scene_desc *sc, int32_t m) {
    if (m < 0 || m >= sc->num_materials) return -1.0;
    const float *e = sc->materials[m].emit.e;
    int lit = 0;
    for (int c = 0; c < 3; ++c) {
        if (!(isfinite(e[c]) && e[c] >= 0.0f)) return -1.0;
        if (e[c] > 0.0f) lit = 1;
    }
    return lit ? ((double)e[0] + (double)e[1]) + (double)e[2] : -1.0;
}
static float plane_area(const rt_plane *p) {
    const double u[3] = {p->u.e[0], p->u.e[1], p->u.e[2]}, v[3] = {p->v.e[0], p->v.e[1], p->v.e[2]};
    const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double k = p->type == RT_PLANE_QUAD ? 1.0 : (p->type == RT_PLANE_ELLIPSE ? M_PI / 4.0 : 0.5);
    return (float)(k * sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]));
}
static void make_tab(const rt_scene_desc *sc, int on, int32_t mis, int32_t planes, emit_tab *T) {
    const size_t cap = (size_t)(sc->num_spheres + sc->num_planes + 1);
    T->kind = (int32_t *)malloc(cap * sizeof(int32_t));
    T->index = (int32_t *)malloc(cap * sizeof(int32_t));
    T->cdf = (float *)malloc(cap * sizeof(float));
    T->pmf = (float *)malloc(cap * sizeof(float));
    T->area = (float *)malloc(cap * sizeof(float));
    T->count = 0;
    T->mis = mis;
    if (!on) return;
    double *w = (double *)malloc(cap * sizeof(double)), total = 0.0, run = 0.0;
    int32_t n = 0;
    for (int32_t i = 0; i < sc->num_spheres; ++i) {
        const rt_sphere *s = &sc->spheres[i];
        const double e = emit_sum(sc, s->material_idx);
        if (!(s->radius > 0.0f) || e < 0.0) continue;
        T->kind[n] = 0;
        T->index[n] = i;
        T->area[n] = 0.0f;
        w[n++] = e * ((double)s->radius * (double)s->radius);
    }
    for (int32_t i = 0; planes && i < sc->num_planes; ++i) {
        const rt_plane *p = &sc->planes[i];
        if (p->type != RT_PLANE_QUAD && p->type != RT_PLANE_ELLIPSE && p->type != RT_PLANE_TRIANGLE) continue;
        const double e = emit_sum(sc, p->material_idx);
        if (e < 0.0) continue;
        const float A = plane_area(p);
        if (!(isfinite(A) && A > 0.0f)) continue;
        T->kind[n] = 1;
        T->index[n] = i;
        T->area[n] = A;
        w[n++] = e * (double)A / M_PI;
    }
    for (int32_t k = 0; k < n; ++k) total += w[k];
    for (int32_t k = 0; k < n; ++k) {
        run += w[k];
        T->cdf[k] = k + 1 == n ? 1.0f : (float)(run / total);
        T->pmf[k] = T->cdf[k] - (k == 0 ? 0.0f : T->cdf[k - 1]);
    }
    free(w);
    T->count = n;
}
static void free_tab(emit_tab *T) { free(T->kind); free(T->index); free(T->cdf); free(T->pmf); free(T->area); }
static int tab_find(const emit_tab *T, int32_t kind, int32_t index) {
    for (int32_t k = 0; k < T->count; ++k)
        if (T->kind[k] == kind && T->index[k] == index) return k;
    return -1;
}
/* the cone of a sphere seen from x: 0 = no contribution */
static int cone_of(v3 x, const rt_sphere *s, v3 *w, float *d2, float *om) {
    *w = sub(from_rt(s->center), x);
    *d2 = dot(*w, *w);
    const float rr = s->radius * s->radius;
    if (!(*d2 > rr)) return 0;
    const float cos_max = sqrtf(1.0f - rr / *d2);
    *om = 1.0f - cos_max;
    return *om > 0.0f;
}
static float pdf_cone(float om) { return 1.0f / (RT_NEE_TWO_PI * om); }
/* step 3p: the point y of plane p (area A) seen from x: 0 = no contribution, else the unit direction and the solid-angle density */
static int plane_pa(v3 x, v3 y, const rt_plane *p, float A, v3 *wl, float *pa) {
    const v3 w = sub(y, x);
    const float d2 = dot(w, w);
    if (!(d2 > 0.0f)) return 0;
    const float len = sqrtf(d2);
    *wl = V(w.e[0] / len, w.e[1] / len, w.e[2] / len);
    const float cos_l = fabsf(dot(from_rt(p->normal), *wl));
    if (!(cos_l >= 1e-8f)) return 0;
    *pa = d2 / (cos_l * A);
    return 1;
}

/* the light sample up to the shadow ray: 1 = it asks for one (direction, kind and index of the primitive to reach, contribution) */
static int emitter_sample(const rt_scene_desc *sc, const emit_tab *T, uint32_t *nee, v3 x, v3 n, v3 a, v3 beta, v3 *dir, int32_t *kind_out,
                          int32_t *index_out, v3 *c) {
    const float u = orc_random_float(nee);
    int32_t e = 0;
    while (e < T->count && !(u < T->cdf[e])) ++e;
    if (e >= T->count) return 0;
    const float pb = RT_NEE_PB;
    float pl;
    v3 emit;
    if (T->kind[e] == 1) {
        const rt_plane *p = &sc->planes[T->index[e]];
        float ua, ub;
        if (p->type == RT_PLANE_ELLIPSE) {
            float px, py, q2;
            do {
                px = random_range(nee, -1.0f, 1.0f);
                py = random_range(nee, -1.0f, 1.0f);
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
        if (!(dot(*dir, n) > 0.0f)) return 0;
        pl = T->pmf[e] * pa;
        emit = from_rt(sc->materials[p->material_idx].emit);
    } else {
        const int32_t sphere = T->index[e];
        v3 w;
        float d2, om;
        if (!cone_of(x, &sc->spheres[sphere], &w, &d2, &om)) return 0;
        const float u1 = orc_random_float(nee);
        const float cos_t = 1.0f - u1 * om;
        const float sin_t = sqrtf(fmaxf(0.0f, 1.0f - cos_t * cos_t));
        float px, py, q2;
        do {
            px = random_range(nee, -1.0f, 1.0f);
            py = random_range(nee, -1.0f, 1.0f);
            q2 = px * px + py * py;
        } while (q2 >= 1.0f || q2 == 0.0f);
        const float q = sqrtf(q2);
        const float cx = px / q, cy = py / q;
        const float len = sqrtf(d2);
        const v3 wn = V(w.e[0] / len, w.e[1] / len, w.e[2] / len);
        const float sg = copysignf(1.0f, wn.e[2]);
        const float ba = -1.0f / (sg + wn.e[2]);
        const float bb = (wn.e[0] * wn.e[1]) * ba;
        const v3 t1 = V(1.0f + ((sg * wn.e[0]) * wn.e[0]) * ba, sg * bb, -sg * wn.e[0]);
        const v3 t2 = V(bb, sg + (wn.e[1] * wn.e[1]) * ba, -wn.e[1]);
        const float sx = sin_t * cx, sy = sin_t * cy;
        for (int k = 0; k < 3; ++k) dir->e[k] = (t1.e[k] * sx + t2.e[k] * sy) + wn.e[k] * cos_t;
        if (!(dot(*dir, n) > 0.0f)) return 0;
        pl = T->pmf[e] * pdf_cone(om);
        emit = from_rt(sc->materials[sc->spheres[sphere].material_idx].emit);
    }
    const float f = T->mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), emit));
    *kind_out = T->kind[e];
    *index_out = T->index[e];
    return 1;
}

/* ---- the environment (rt_render_env's) --------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, empty;
    const float *rgb;
    float *row_cdf, *row_pmf, *col_cdf, *col_pmf;
} sky_map;

static float sgn1(float x) { return x >= 0.0f ? 1.0f : -1.0f; }
static void decode_d(double u, double v, double p[3]) {
    const double y = (1.0 - fabs(u)) - fabs(v);
    p[1] = y;
    if (y >= 0.0) {
        p[0] = u;
        p[2] = v;
    } else {
        p[0] = (1.0 - fabs(v)) * (u >= 0.0 ? 1.0 : -1.0);
        p[2] = (1.0 - fabs(u)) * (v >= 0.0 ? 1.0 : -1.0);
    }
}
static v3 decode_f(float u, float v) {
    const float y = (1.0f - fabsf(u)) - fabsf(v);
    if (y >= 0.0f) return V(u, y, v);
    return V((1.0f - fabsf(v)) * sgn1(u), y, (1.0f - fabsf(u)) * sgn1(v));
}
static int32_t cell_of(float u, int32_t n) {
    const float t = ((u + 1.0f) * 0.5f) * (float)n;
    return t >= 0.0f ? (t < (float)n ? (int32_t)t : n - 1) : 0;
}
static int32_t texel_of(v3 d, int32_t n, v3 *p) {
    const float s = (fabsf(d.e[0]) + fabsf(d.e[1])) + fabsf(d.e[2]);
    *p = V(d.e[0] / s, d.e[1] / s, d.e[2] / s);
    float u = p->e[0], v = p->e[2];
    if (!(p->e[1] >= 0.0f)) {
        u = (1.0f - fabsf(p->e[2])) * sgn1(p->e[0]);
        v = (1.0f - fabsf(p->e[0])) * sgn1(p->e[2]);
    }
    return cell_of(v, n) * n + cell_of(u, n);
}
static void cdf_of(const double *w, int32_t n, double total, float *cdf, float *pmf) {
    double run = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        run += w[k];
        cdf[k] = total > 0.0 ? (k + 1 == n ? 1.0f : (float)(run / total)) : 0.0f;
        pmf[k] = cdf[k] - (k == 0 ? 0.0f : cdf[k - 1]);
    }
}
static void make_map(const float *rgb, int32_t n, sky_map *M) {
    const size_t nn = (size_t)n * n;
    M->n = n;
    M->rgb = rgb;
    M->row_cdf = (float *)malloc(4 * (size_t)n);
    M->row_pmf = (float *)malloc(4 * (size_t)n);
    M->col_cdf = (float *)malloc(4 * nn);
    M->col_pmf = (float *)malloc(4 * nn);
    double *w = (double *)malloc(sizeof(double) * nn), *rw = (double *)malloc(sizeof(double) * (size_t)n), total = 0.0;
    const double cellarea = (2.0 / (double)n) * (2.0 / (double)n);
    for (int32_t iy = 0; iy < n; ++iy) {
        double row = 0.0;
        for (int32_t ix = 0; ix < n; ++ix) {
            const double uc = -1.0 + (double)(2 * ix + 1) / (double)n, vc = -1.0 + (double)(2 * iy + 1) / (double)n;
            double p[3];
            decode_d(uc, vc, p);
            const double l2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
            const float *t = rgb + ((size_t)iy * n + ix) * 3;
            w[(size_t)iy * n + ix] = (((double)t[0] + (double)t[1]) + (double)t[2]) * (cellarea / (l2 * sqrt(l2)));
            row += w[(size_t)iy * n + ix];
        }
        rw[iy] = row;
        total += row;
    }
    cdf_of(rw, n, total, M->row_cdf, M->row_pmf);
    for (int32_t iy = 0; iy < n; ++iy) cdf_of(w + (size_t)iy * n, n, total > 0.0 ? rw[iy] : 0.0, M->col_cdf + (size_t)iy * n, M->col_pmf + (size_t)iy * n);
    M->empty = !(total > 0.0);
    free(w);
    free(rw);
}
static void free_map(sky_map *M) { free(M->row_cdf); free(M->row_pmf); free(M->col_cdf); free(M->col_pmf); }
static float pl_of(const sky_map *M, int32_t t, float q2, float q) {
    if (M->empty) return 0.0f;
    return ((M->row_pmf[t / M->n] * M->col_pmf[t]) * (((float)M->n * (float)M->n) * 0.25f)) * (q2 * q);
}
/* smallest e in [0, n) with u < cdf[e]; n when there is none — by scan (the header's words) or by bisection (the cdf is monotone) */
static int32_t pick(const float *cdf, int32_t n, float u, int linear) {
    if (linear) {
        int32_t e = 0;
        while (e < n && !(u < cdf[e])) ++e;
        return e;
    }
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (u < cdf[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
static v3 to_env(const rt_env_params *ep, v3 d) {
    return V(dot(V(ep->rot[0], ep->rot[1], ep->rot[2]), d), dot(V(ep->rot[3], ep->rot[4], ep->rot[5]), d), dot(V(ep->rot[6], ep->rot[7], ep->rot[8]), d));
}
static v3 scaled(const sky_map *M, const rt_env_params *ep, int32_t t) {
    const float *c = M->rgb + 3 * (size_t)t;
    return V(ep->scale * c[0], ep->scale * c[1], ep->scale * c[2]);
}
/* rt_render_env's steps 1 … 4 up to the shadow ray */
static int sky_sample(const sky_map *M, const rt_env_params *ep, uint32_t *env, v3 n, v3 a, v3 beta, v3 *dir, v3 *c, int linear) {
    const float ua = orc_random_float(env);
    const int32_t iy = pick(M->row_cdf, M->n, ua, linear);
    if (iy >= M->n) return 0;
    const float ub = orc_random_float(env);
    const int32_t ix = pick(M->col_cdf + (size_t)iy * M->n, M->n, ub, linear);
    if (ix >= M->n) return 0;
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
    if (!(dot(*dir, n) > 0.0f)) return 0;
    const int32_t t = iy * M->n + ix;
    const float pl = pl_of(M, t, q2, q);
    const float pb = RT_NEE_PB;
    const float f = ep->mode == 1 ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), scaled(M, ep, t)));
    return 1;
}

/* ---- the camera (rt_render_lens's steps 1 … 5) ---------------------------------------------------------------------------------- */
static v3 lerp3(v3 a, v3 b, float tau) { return add(a, scale(tau, sub(b, a))); }
static v3 div3(v3 v, float t) { return V(v.e[0] / t, v.e[1] / t, v.e[2] / t); }
static ray camera_ray_of(const rt_camera_data *open, const lit_cfg *cfg, int i, int j, uint32_t *seed) {
    const float ox = orc_random_float(seed) - 0.5f;
    const float oy = orc_random_float(seed) - 0.5f;
    v3 O = from_rt(open->origin), P00 = from_rt(open->pixel00_loc), du = from_rt(open->pixel_delta_u), dv = from_rt(open->pixel_delta_v);
    if (cfg->cam_close) {
        const rt_camera_data *cl = cfg->cam_close;
        const float tau = orc_random_float(seed);
        O = lerp3(O, from_rt(cl->origin), tau);
        P00 = lerp3(P00, from_rt(cl->pixel00_loc), tau);
        du = lerp3(du, from_rt(cl->pixel_delta_u), tau);
        dv = lerp3(dv, from_rt(cl->pixel_delta_v), tau);
    }
    float lx = 0.0f, ly = 0.0f;
    const float R = cfg->lens_radius;
    if (R > 0.0f) {
        do {
            lx = random_range(seed, -1.0f, 1.0f);
            ly = random_range(seed, -1.0f, 1.0f);
        } while (lx * lx + ly * ly >= 1.0f);
    }
    const v3 S = add(add(add(add(P00, scale((float)i, du)), scale((float)j, dv)), scale(ox, du)), scale(oy, dv));
    ray r;
    r.o = O;
    r.d = sub(S, O);
    if (R > 0.0f) {
        const v3 n = cross(du, dv);
        const float dimg = fabsf(dot(sub(P00, O), n)) / sqrtf(dot(n, n));
        const float k = cfg->focus_distance / dimg;
        const v3 F = add(O, scale(k, r.d));
        const v3 uh = div3(du, sqrtf(dot(du, du))), vh = div3(dv, sqrtf(dot(dv, dv)));
        const v3 Lp = add(add(O, scale(R * lx, uh)), scale(R * ly, vh));
        r.o = Lp;
        r.d = sub(F, Lp);
    }
    return r;
}

/* ---- the path ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    const rt_scene_desc *sc;
    const rt_camera_data *cam;
    const lit_cfg *cfg;
    const emit_tab *T;
    const sky_map *M;              /* NULL: no environment */
    int linear;
} lit_ctx;

static int closest(const rt_scene_desc *sc, const ray *r, hitrec *rec, int *pt, int *pi) {
    *pt = -1;
    *pi = -1;
    return sc->num_nodes > 0 ? hit_bvh(sc, r, 0.001f, 1e30f, rec, pt, pi, NULL) : 0;
}

static v3 ray_color_lit(const lit_ctx *X, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, int32_t *rays_out) {
    const rt_scene_desc *sc = X->sc;
    const rt_camera_data *cam = X->cam;
    const rt_env_params *ep = X->cfg->ep;
    const int emitters_on = X->T->count > 0;
    const int sky_sampled = X->M && ep->mode != 0 && !X->M->empty;
    const float pb = RT_NEE_PB;
    v3 final_color = V(0.0f, 0.0f, 0.0f);
    v3 beta = V(1.0f, 1.0f, 1.0f);
    ray cur = r;
    int32_t nrays = 0;
    int prev_diffuse = 0;
    for (int depth = 0; depth < cam->max_depth; depth++) {
        hitrec rec;
        int pt, pi;
        nrays++;
        if (!closest(sc, &cur, &rec, &pt, &pi)) {
            /* 2. the miss term */
            if (!X->M || (depth == 0 && !ep->camera_visible)) {
                final_color = add(final_color, mulv(beta, from_rt(cam->background)));
                break;
            }
            v3 p;
            const int32_t t = texel_of(to_env(ep, cur.d), X->M->n, &p);
            v3 term = mulv(beta, scaled(X->M, ep, t));
            if (prev_diffuse && sky_sampled) {
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
        /* 1. / 3. the emission term: a table sphere found from a diffuse event is weighted, everything else keeps weight 1 */
        v3 emitted = mulv(beta, from_rt(mat->emit));
        if (prev_diffuse && (pt == 0 || pt == 1) && emitters_on) {
            const int e = tab_find(X->T, pt, pi);
            if (e >= 0) {
                v3 w;
                float d2, om, pa, pl = 0.0f;
                if (pt == 1) {
                    if (plane_pa(cur.o, rec.point, &sc->planes[pi], X->T->area[e], &w, &pa)) pl = X->T->pmf[e] * pa;
                } else if (cone_of(cur.o, &sc->spheres[pi], &w, &d2, &om)) pl = X->T->pmf[e] * pdf_cone(om);
                const float wb = X->T->mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                emitted = scale(wb, emitted);
            }
        }
        final_color = add(final_color, emitted);
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
        if (diffuse && depth + 1 < cam->max_depth) {
            hitrec srec;
            int spt, spi;
            ray shadow;
            v3 c;
            shadow.o = rec.point;
            /* 4. the emitter sample: its shadow ray's closest hit must be the picked entry's primitive */
            int32_t lkind, lindex;
            if (emitters_on && emitter_sample(sc, X->T, nee, rec.point, rec.normal, albedo, beta, &shadow.d, &lkind, &lindex, &c)) {
                nrays++;
                if (closest(sc, &shadow, &srec, &spt, &spi) && spt == lkind && spi == lindex) final_color = add(final_color, c);
            }
            /* 5. the environment sample: an occlusion query from the same point */
            if (sky_sampled && sky_sample(X->M, ep, env, rec.normal, albedo, beta, &shadow.d, &c, X->linear)) {
                nrays++;
                if (!closest(sc, &shadow, &srec, &spt, &spi)) final_color = add(final_color, c);
            }
        }
        beta = mulv(beta, attenuation);
        cur = scattered;
        prev_diffuse = diffuse;
    }
    if (rays_out) *rays_out = nrays;
    return final_color;
}

static v3 sample_of(const lit_ctx *X, int i, int j, int s, int32_t *rays, uint32_t *seed_out, uint32_t *nee_out, uint32_t *env_out) {
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_lit(X, r, &seed, &nee, &env, rays);
    if (seed_out) *seed_out = seed;
    if (nee_out) *nee_out = nee;
    if (env_out) *env_out = env;
    return c;
}

static void make_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const lit_cfg *cfg, emit_tab *T, sky_map *M, int linear, lit_ctx *X) {
    make_tab(sc, cfg->sample_emitters != 0, cfg->nee_mis, cfg->sample_planes, T);
    if (cfg->rgb) make_map(cfg->rgb, cfg->n, M);
    X->sc = sc;
    X->cam = cam;
    X->cfg = cfg;
    X->T = T;
    X->M = cfg->rgb ? M : NULL;
    X->linear = linear;
}
static void free_ctx(const lit_cfg *cfg, emit_tab *T, sky_map *M) {
    free_tab(T);
    if (cfg->rgb) free_map(M);
}

/* the emitter table of (sample_planes): kind, index, cdf, pmf, area (room for num_spheres + num_planes entries each) → its length */
int32_t emit_table(const rt_scene_desc *sc, int32_t sample_planes, int32_t *kind, int32_t *index, float *cdf, float *pmf, float *area) {
    emit_tab T;
    make_tab(sc, 1, 1, sample_planes, &T);
    memcpy(kind, T.kind, sizeof(int32_t) * (size_t)T.count);
    memcpy(index, T.index, sizeof(int32_t) * (size_t)T.count);
    memcpy(cdf, T.cdf, sizeof(float) * (size_t)T.count);
    memcpy(pmf, T.pmf, sizeof(float) * (size_t)T.count);
    memcpy(area, T.area, sizeof(float) * (size_t)T.count);
    const int32_t n = T.count;
    free_tab(&T);
    return n;
}

/* per vertex (tests/light_vertex_cases.py): the table's pick at u[k] — the smallest e with u < cdf[e], the table's length when there is
 * none — and the entry of primitive code[k], -1 when the table does not hold it.  two_kind: code is 2 * index + kind (the two-kind table's
 * emit_find); else it is a sphere's index (the sphere-only table's nee_find) */
void emit_vertex_picks(const rt_scene_desc *sc, int32_t sample_planes, int32_t two_kind, int64_t count, const float *u, const int32_t *code, int32_t *entry,
                       int32_t *found) {
    emit_tab T;
    make_tab(sc, 1, 1, sample_planes, &T);
    for (int64_t k = 0; k < count; ++k) {
        int32_t e = 0;
        while (e < T.count && !(u[k] < T.cdf[e])) ++e;
        entry[k] = e;
        found[k] = two_kind ? tab_find(&T, code[k] & 1, code[k] >> 1) : tab_find(&T, 0, code[k]);
    }
    free_tab(&T);
}

/* where the pinhole camera ray of count samples first lands: the primitive's kind (0 sphere, 1 plane, -1 nothing), its index and the point */
void emit_first_hit(const rt_scene_desc *sc, const rt_camera_data *cam, int64_t count, const int32_t *ijs, int32_t *kind, int32_t *index, float *point) {
    for (int64_t k = 0; k < count; ++k) {
        const uint32_t base = orc_wang_hash((uint32_t)ijs[3 * k] * (uint32_t)cam->image_width + (uint32_t)ijs[3 * k + 1]);
        uint32_t seed = orc_wang_hash(base + (uint32_t)ijs[3 * k + 2]);
        const ray r = get_ray(cam, ijs[3 * k], ijs[3 * k + 1], &seed);
        hitrec rec;
        int pt, pi;
        memset(&rec, 0, sizeof(rec));
        if (!closest(sc, &r, &rec, &pt, &pi)) pt = pi = -1;
        kind[k] = pt;
        index[k] = pi;
        memcpy(point + 3 * k, rec.point.e, 12);
    }
}

/* count samples (ijs: i, j, s) → radiance (3 floats), rays, the path's final seed and both light streams' final states */
void emit_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const lit_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance,
               int32_t *rays, uint32_t *seeds, uint32_t *nee_seeds, uint32_t *env_seeds, int32_t linear) {
    emit_tab T;
    sky_map M;
    lit_ctx X;
    make_ctx(sc, cam, cfg, &T, &M, linear, &X);
    for (int64_t k = 0; k < count; ++k) {
        const v3 c = sample_of(&X, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &rays[k], &seeds[k], &nee_seeds[k], &env_seeds[k]);
        memcpy(radiance + 3 * k, c.e, 12);
    }
    free_ctx(cfg, &T, &M);
}

typedef struct {
    const lit_ctx *X;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;          /* sums (nrows x W x 3), or NULL */
    double *mom;        /* per pixel: sum and sum of squares of each channel (6 doubles), or NULL */
} lit_job;

static void *lit_run(void *arg) {
    lit_job *jb = (lit_job *)arg;
    const rt_camera_data *cam = jb->X->cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double m[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = sample_of(jb->X, i, j, s, NULL, NULL, NULL, NULL);
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

/* The sums of samples sample_first … sample_first + spp - 1 of the listed image rows (in that order): fb (nrows x W x 3).  mom (may be
 * NULL): per pixel the double sums and sums of squares of the three channels.  Threads split the rows. */
void emit_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const lit_cfg *cfg, const int32_t *rows, int nrows, int sample_first,
               int threads, float *fb, double *mom) {
    emit_tab T;
    sky_map M;
    lit_ctx X;
    make_ctx(sc, cam, cfg, &T, &M, 0, &X);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    lit_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        lit_job jb = {&X, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, lit_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_ctx(cfg, &T, &M);
}
