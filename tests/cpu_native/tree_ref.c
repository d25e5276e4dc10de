/* tree_ref.c — CPU reference of rt_nee_params.select (tests/tree_reference.py builds it on its own into a shared library,
 * gcc -ffp-contract=off like the oracle): emit_ref.c's rt_render_lit with the light tree's build and pick, restated from the words of
 * include/rtp_amd.h.  This file includes emit_ref.c (and through it the oracle) for everything the tree leaves alone: the emitter table,
 * the cone and the plane density, the environment, the camera, the closest-hit query.
 *
 * select = 0 picks by the table's cdf and then takes the steps written here, so that frame compared with emit_ref.c's checks those steps;
 * select = 1 picks by the descent, and a BSDF hit on a table entry is weighted with the product along the entry's stored path.
 */
#include "emit_ref.c"

typedef struct {
    lit_cfg base;
    int32_t select;
} tree_cfg;

/* ---- the tree: columns per node (preorder) and per entry ----------------------------------------------------------------------- */
typedef struct {
    int32_t nodes, entries;
    float *sphere, *weight, *q;        /* sphere: 4 per node */
    int32_t *left, *right, *entry;
    uint32_t *path;
    int32_t *depth;
    double *geom, total;               /* per entry: c0 c1 c2 rho w */
} light_tree;

static double len3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
static void entry_bound(const rt_scene_desc *sc, const emit_tab *T, int32_t e, double *g) {
    if (T->kind[e] == 0) {
        const rt_sphere *s = &sc->spheres[T->index[e]];
        for (int k = 0; k < 3; ++k) g[k] = s->center.e[k];
        g[3] = s->radius;
        g[4] = emit_sum(sc, s->material_idx) * ((double)s->radius * (double)s->radius);
        return;
    }
    const rt_plane *p = &sc->planes[T->index[e]];
    double b[3], u[3], v[3];
    for (int k = 0; k < 3; ++k) {
        b[k] = p->base.e[k];
        u[k] = p->u.e[k];
        v[k] = p->v.e[k];
    }
    if (p->type == RT_PLANE_TRIANGLE) {
        for (int k = 0; k < 3; ++k) g[k] = b[k] + (u[k] + v[k]) / 3.0;
        const double d0 = len3(b[0] - g[0], b[1] - g[1], b[2] - g[2]);
        const double d1 = len3((b[0] + u[0]) - g[0], (b[1] + u[1]) - g[1], (b[2] + u[2]) - g[2]);
        const double d2 = len3((b[0] + v[0]) - g[0], (b[1] + v[1]) - g[1], (b[2] + v[2]) - g[2]);
        g[3] = fmax(d0, fmax(d1, d2));
    } else {
        for (int k = 0; k < 3; ++k) g[k] = (b[k] + 0.5 * u[k]) + 0.5 * v[k];
        g[3] = 0.5 * fmax(len3(u[0] + v[0], u[1] + v[1], u[2] + v[2]), len3(u[0] - v[0], u[1] - v[1], u[2] - v[2]));
    }
    g[4] = emit_sum(sc, p->material_idx) * (double)T->area[e] / M_PI;
}
/* the node over the n entries of list S, reached by `bits` in `level` steps → its index; *wsum: the sum of its weights in list order */
static int32_t tree_node(light_tree *t, int32_t *S, int32_t n, uint32_t bits, int32_t level, double *wsum) {
    const int32_t id = t->nodes++;
    double lo[3], hi[3], clo[3], chi[3], W = 0.0, m[3], R = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        const double *g = t->geom + 5 * (size_t)S[k];
        for (int a = 0; a < 3; ++a) {
            if (k == 0 || g[a] - g[3] < lo[a]) lo[a] = g[a] - g[3];
            if (k == 0 || g[a] + g[3] > hi[a]) hi[a] = g[a] + g[3];
            if (k == 0 || g[a] < clo[a]) clo[a] = g[a];
            if (k == 0 || g[a] > chi[a]) chi[a] = g[a];
        }
        W += g[4];
    }
    for (int a = 0; a < 3; ++a) m[a] = 0.5 * (lo[a] + hi[a]);
    for (int32_t k = 0; k < n; ++k) {
        const double *g = t->geom + 5 * (size_t)S[k];
        const double r = len3(g[0] - m[0], g[1] - m[1], g[2] - m[2]) + g[3];
        if (r > R) R = r;
    }
    for (int a = 0; a < 3; ++a) t->sphere[4 * id + a] = (float)m[a];
    t->sphere[4 * id + 3] = nextafterf((float)R, INFINITY);
    t->weight[id] = (float)(W / t->total);
    t->q[id] = 0.0f;
    t->left[id] = t->right[id] = t->entry[id] = -1;
    if (n == 1) {
        t->entry[id] = S[0];
        t->path[S[0]] = bits;
        t->depth[S[0]] = level;
    } else {
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
        /* a stable sort: insertion */
        for (int32_t i = 1; i < n; ++i) {
            const int32_t e = S[i];
            int32_t j = i;
            while (j > 0 && t->geom[5 * (size_t)S[j - 1] + axis] > t->geom[5 * (size_t)e + axis]) {
                S[j] = S[j - 1];
                --j;
            }
            S[j] = e;
        }
        const int32_t nl = (n + 1) / 2;
        double wl, wr;
        t->left[id] = tree_node(t, S, nl, bits, level + 1, &wl);
        t->right[id] = tree_node(t, S + nl, n - nl, bits | (1u << level), level + 1, &wr);
        t->q[id] = (float)(wl / (wl + wr));
    }
    *wsum = W;
    return id;
}
static void make_tree(const rt_scene_desc *sc, const emit_tab *T, light_tree *t) {
    const int32_t n = T->count;
    const size_t cap = (size_t)(2 * n + 1);
    memset(t, 0, sizeof(*t));
    t->entries = n;
    t->sphere = (float *)malloc(cap * 16);
    t->weight = (float *)malloc(cap * 4);
    t->q = (float *)malloc(cap * 4);
    t->left = (int32_t *)malloc(cap * 4);
    t->right = (int32_t *)malloc(cap * 4);
    t->entry = (int32_t *)malloc(cap * 4);
    t->path = (uint32_t *)malloc(cap * 4);
    t->depth = (int32_t *)malloc(cap * 4);
    t->geom = (double *)malloc(cap * 5 * sizeof(double));
    if (n == 0) return;
    int32_t *S = (int32_t *)malloc((size_t)n * 4);
    for (int32_t e = 0; e < n; ++e) {
        entry_bound(sc, T, e, t->geom + 5 * (size_t)e);
        t->total += t->geom[5 * (size_t)e + 4];
        S[e] = e;
    }
    double w;
    tree_node(t, S, n, 0u, 0, &w);
    free(S);
}
static void free_tree(light_tree *t) {
    free(t->sphere); free(t->weight); free(t->q); free(t->left); free(t->right); free(t->entry); free(t->path); free(t->depth); free(t->geom);
}

/* ---- the pick and the path product ---------------------------------------------------------------------------------------------- */
static float importance(const light_tree *t, int32_t c, v3 x) {
    const v3 w = sub(V(t->sphere[4 * c], t->sphere[4 * c + 1], t->sphere[4 * c + 2]), x);
    const float d2 = dot(w, w);
    const float rho = t->sphere[4 * c + 3];
    return t->weight[c] / fmaxf(d2, rho * rho);
}
/* *fell (may be NULL) is set when the node's q stood in for the importances; it is never cleared here */
static float left_probability(const light_tree *t, int32_t node, v3 x, int *fell) {
    const float il = importance(t, t->left[node], x), ir = importance(t, t->right[node], x);
    const float s = il + ir;
    if (s > 0.0f && s < INFINITY) return il / s;
    if (fell) *fell = 1;
    return t->q[node];
}
static int32_t tree_pick(const light_tree *t, uint32_t *nee, v3 x, float *p_out, int *fell) {
    int32_t node = 0;
    float p = 1.0f;
    while (t->entry[node] < 0) {
        const float pl = left_probability(t, node, x, fell);
        const float u = orc_random_float(nee);
        if (u < pl) {
            p = p * pl;
            node = t->left[node];
        } else {
            p = p * (1.0f - pl);
            node = t->right[node];
        }
    }
    *p_out = p;
    return t->entry[node];
}
static float tree_pmf(const light_tree *t, int32_t e, v3 x, int *fell) {
    int32_t node = 0;
    float p = 1.0f;
    for (int32_t i = 0; i < t->depth[e]; ++i) {
        const float pl = left_probability(t, node, x, fell);
        if ((t->path[e] >> i) & 1u) {
            p = p * (1.0f - pl);
            node = t->right[node];
        } else {
            p = p * pl;
            node = t->left[node];
        }
    }
    return p;
}

/* the tallies of tree_trace's stats, in its order (tests/tree_reference.py names them the same way) */
enum {
    ST_INSIDE_PARENT = 0,   /* sampling vertices inside the sphere of their picked leaf's parent */
    ST_WEIGHTED,            /* BSDF hits on table entries that were weighted */
    ST_DROP_INSIDE,         /* light samples dropped at step 2: the point is not outside the sphere (!(d2 > rr)) */
    ST_DROP_OMEGA,          /* light samples dropped at step 2: om <= 0 */
    ST_DROP_COS,            /* light samples dropped at 3p: cos_l < 1e-8 */
    ST_SHADOW_OTHER_ENTRY,  /* shadow rays whose closest hit is another table entry */
    ST_SHADOW_NON_TABLE,    /* shadow rays whose closest hit is a primitive outside the table */
    ST_HIT_PL_ZERO,         /* weighted BSDF hits with pl == 0 */
    ST_Q_FALLBACK,          /* descents and path products in which a node's q stood in for the importances */
    ST_PICK_NONE,           /* picks that returned no entry */
    ST_COUNT
};

/* steps 2 to 4 / 2p to 4p for the picked entry e with the probability pmf of that pick: 1 = a shadow ray is asked for.  stats (may be NULL)
 * counts why a sample was dropped; it changes nothing else */
static int entry_sample(const rt_scene_desc *sc, const emit_tab *T, int32_t e, float pmf, uint32_t *nee, v3 x, v3 n, v3 a, v3 beta, v3 *dir, v3 *c,
                        int64_t *stats) {
    const float pb = RT_NEE_PB;
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
        if (!plane_pa(x, y, p, T->area[e], dir, &pa)) {
            const v3 xy = sub(y, x);
            if (stats && dot(xy, xy) > 0.0f) stats[ST_DROP_COS]++;      /* (plane_pa's other refusal is d2 == 0) */
            return 0;
        }
        if (!(dot(*dir, n) > 0.0f)) return 0;
        pl = pmf * pa;
        emit = from_rt(sc->materials[p->material_idx].emit);
    } else {
        const rt_sphere *s = &sc->spheres[T->index[e]];
        v3 w;
        float d2, om;
        if (!cone_of(x, s, &w, &d2, &om)) {
            if (stats) stats[d2 > s->radius * s->radius ? ST_DROP_OMEGA : ST_DROP_INSIDE]++;
            return 0;
        }
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
        const float sg = copysignf(1.0f, wn.e[2]);
        const float ba = -1.0f / (sg + wn.e[2]);
        const float bb = (wn.e[0] * wn.e[1]) * ba;
        const v3 t1 = V(1.0f + ((sg * wn.e[0]) * wn.e[0]) * ba, sg * bb, -sg * wn.e[0]);
        const v3 t2 = V(bb, sg + (wn.e[1] * wn.e[1]) * ba, -wn.e[1]);
        const float sx = sin_t * cx, sy = sin_t * cy;
        for (int k = 0; k < 3; ++k) dir->e[k] = (t1.e[k] * sx + t2.e[k] * sy) + wn.e[k] * cos_t;
        if (!(dot(*dir, n) > 0.0f)) return 0;
        pl = pmf * pdf_cone(om);
        emit = from_rt(sc->materials[s->material_idx].emit);
    }
    const float f = T->mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;
    *c = scale(f, mulv(mulv(beta, a), emit));
    return 1;
}

/* ---- the path: emit_ref.c's ray_color_lit with the pick by `select` ------------------------------------------------------------------ */
typedef struct {
    lit_ctx X;
    const light_tree *tree;
    int32_t select;
    int64_t *stats;        /* NULL, or the ST_COUNT tallies above (tree_trace) */
} tree_ctx;

static v3 ray_color_tree(const tree_ctx *Y, ray r, uint32_t *seed, uint32_t *nee, uint32_t *env, int32_t *rays_out) {
    const lit_ctx *X = &Y->X;
    const rt_scene_desc *sc = X->sc;
    const rt_camera_data *cam = X->cam;
    const rt_env_params *ep = X->cfg->ep;
    const emit_tab *T = X->T;
    const int emitters_on = T->count > 0;
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
        v3 emitted = mulv(beta, from_rt(mat->emit));
        if (prev_diffuse && (pt == 0 || pt == 1) && emitters_on) {
            const int e = tab_find(T, pt, pi);
            if (e >= 0) {
                v3 w;
                float d2, om, pa, pl = 0.0f;
                int fell = 0;
                if (pt == 1) {
                    if (plane_pa(cur.o, rec.point, &sc->planes[pi], T->area[e], &w, &pa))
                        pl = (Y->select ? tree_pmf(Y->tree, e, cur.o, &fell) : T->pmf[e]) * pa;
                } else if (cone_of(cur.o, &sc->spheres[pi], &w, &d2, &om))
                    pl = (Y->select ? tree_pmf(Y->tree, e, cur.o, &fell) : T->pmf[e]) * pdf_cone(om);
                const float wb = T->mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0.0f ? 0.0f : 1.0f);
                emitted = scale(wb, emitted);
                if (Y->stats) {
                    Y->stats[ST_WEIGHTED]++;
                    if (pl == 0.0f) Y->stats[ST_HIT_PL_ZERO]++;
                    if (fell) Y->stats[ST_Q_FALLBACK]++;
                }
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
            if (emitters_on) {
                int32_t e;
                float pmf = 0.0f;
                if (Y->select) {
                    int fell = 0;
                    e = tree_pick(Y->tree, nee, rec.point, &pmf, &fell);
                    if (Y->stats && fell) Y->stats[ST_Q_FALLBACK]++;
                    if (Y->stats && Y->tree->nodes > 1) {
                        /* is the vertex inside the sphere of the picked leaf's parent?  (the importance's clamp is at work there) */
                        int32_t node = 0, parent = 0;
                        for (int32_t i = 0; i < Y->tree->depth[e]; ++i) {
                            parent = node;
                            node = ((Y->tree->path[e] >> i) & 1u) ? Y->tree->right[node] : Y->tree->left[node];
                        }
                        const float *s = Y->tree->sphere + 4 * parent;
                        const v3 w = sub(V(s[0], s[1], s[2]), rec.point);
                        if (dot(w, w) < s[3] * s[3]) Y->stats[ST_INSIDE_PARENT]++;
                    }
                } else {
                    const float u = orc_random_float(nee);
                    e = 0;
                    while (e < T->count && !(u < T->cdf[e])) ++e;
                    if (e < T->count) pmf = T->pmf[e];
                }
                if (Y->stats && !(e < T->count)) Y->stats[ST_PICK_NONE]++;
                if (e < T->count && entry_sample(sc, T, e, pmf, nee, rec.point, rec.normal, albedo, beta, &shadow.d, &c, Y->stats)) {
                    nrays++;
                    const int hit = closest(sc, &shadow, &srec, &spt, &spi);
                    if (hit && spt == T->kind[e] && spi == T->index[e]) final_color = add(final_color, c);
                    else if (hit && Y->stats) Y->stats[tab_find(T, spt, spi) >= 0 ? ST_SHADOW_OTHER_ENTRY : ST_SHADOW_NON_TABLE]++;
                }
            }
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

static v3 tree_sample_of(const tree_ctx *Y, int i, int j, int s, int32_t *rays, uint32_t *seed_out, uint32_t *nee_out, uint32_t *env_out) {
    const lit_ctx *X = &Y->X;
    const uint32_t base = orc_wang_hash((uint32_t)i * (uint32_t)X->cam->image_width + (uint32_t)j);
    uint32_t seed = orc_wang_hash(base + (uint32_t)s);
    uint32_t nee = orc_wang_hash(seed ^ RT_NEE_STREAM_KEY);
    uint32_t env = orc_wang_hash(seed ^ RT_ENV_STREAM_KEY);
    const ray r = camera_ray_of(X->cam, X->cfg, i, j, &seed);
    const v3 c = ray_color_tree(Y, r, &seed, &nee, &env, rays);
    if (seed_out) *seed_out = seed;
    if (nee_out) *nee_out = nee;
    if (env_out) *env_out = env;
    return c;
}

/* ---- what tests/tree_reference.py calls ------------------------------------------------------------------------------------------- */
/* the tree over the table of sample_planes: its columns (room for 2 (num_spheres + num_planes) nodes) → node count; *entries: N */
int32_t tree_columns(const rt_scene_desc *sc, int32_t sample_planes, float *sphere, float *weight, float *q, int32_t *left, int32_t *right, int32_t *entry,
                     uint32_t *path, int32_t *depth, int32_t *entries) {
    emit_tab T;
    light_tree t;
    make_tab(sc, 1, 1, sample_planes, &T);
    make_tree(sc, &T, &t);
    memcpy(sphere, t.sphere, 16 * (size_t)t.nodes);
    memcpy(weight, t.weight, 4 * (size_t)t.nodes);
    memcpy(q, t.q, 4 * (size_t)t.nodes);
    memcpy(left, t.left, 4 * (size_t)t.nodes);
    memcpy(right, t.right, 4 * (size_t)t.nodes);
    memcpy(entry, t.entry, 4 * (size_t)t.nodes);
    memcpy(path, t.path, 4 * (size_t)t.entries);
    memcpy(depth, t.depth, 4 * (size_t)t.entries);
    *entries = t.entries;
    const int32_t n = t.nodes;
    free_tree(&t);
    free_tab(&T);
    return n;
}
/* pmf_e(x) by the path product for count points (3 floats each) → pmf (count x N) */
void tree_pmf_points(const rt_scene_desc *sc, int32_t sample_planes, int64_t count, const float *points, float *pmf) {
    emit_tab T;
    light_tree t;
    make_tab(sc, 1, 1, sample_planes, &T);
    make_tree(sc, &T, &t);
    for (int64_t k = 0; k < count; ++k)
        for (int32_t e = 0; e < t.entries; ++e) pmf[k * t.entries + e] = tree_pmf(&t, e, V(points[3 * k], points[3 * k + 1], points[3 * k + 2]), NULL);
    free_tree(&t);
    free_tab(&T);
}
/* `draws` picks from one point, from the stream that starts at seed → how often each entry came (N counts); every pick's p must be the
 * path product of its entry, bit for bit: → the number of picks for which it was not */
int64_t tree_pick_counts(const rt_scene_desc *sc, int32_t sample_planes, const float *point, int64_t draws, uint32_t seed, int64_t *counts) {
    emit_tab T;
    light_tree t;
    make_tab(sc, 1, 1, sample_planes, &T);
    make_tree(sc, &T, &t);
    const v3 x = V(point[0], point[1], point[2]);
    int64_t bad = 0;
    for (int32_t e = 0; e < t.entries; ++e) counts[e] = 0;
    for (int64_t k = 0; k < draws && t.entries > 0; ++k) {
        float p;
        const int32_t e = tree_pick(&t, &seed, x, &p, NULL);
        counts[e]++;
        if (p != tree_pmf(&t, e, x, NULL)) bad++;
    }
    free_tree(&t);
    free_tab(&T);
    return bad;
}

/* per vertex (tests/light_vertex_cases.py): tree_pick from x[k] on the stream that starts at seed[k] → its entry, its p and the stream's
 * state after it; tree_pmf of entry e_in[k] from the same x; fell[k] (may be NULL): bit 0 the descent, bit 1 the path product took a
 * node's q for the importances; pl_root[k] (may be NULL): the root's left probability from x, 1 for a tree of one leaf — what the
 * descent's first draw is compared with */
void tree_vertex_picks(const rt_scene_desc *sc, int32_t sample_planes, int64_t count, const float *x, const uint32_t *seed, const int32_t *e_in,
                       int32_t *entry, float *p, uint32_t *seed_after, float *pmf, int32_t *fell, float *pl_root) {
    emit_tab T;
    light_tree t;
    make_tab(sc, 1, 1, sample_planes, &T);
    make_tree(sc, &T, &t);
    for (int64_t k = 0; k < count && t.entries > 0; ++k) {
        const v3 X = V(x[3 * k], x[3 * k + 1], x[3 * k + 2]);
        uint32_t st = seed[k];
        int fa = 0, fb = 0;
        entry[k] = tree_pick(&t, &st, X, &p[k], fell ? &fa : NULL);
        seed_after[k] = st;
        pmf[k] = tree_pmf(&t, e_in[k], X, fell ? &fb : NULL);
        if (fell) fell[k] = fa | (fb << 1);
        if (pl_root) pl_root[k] = t.entry[0] < 0 ? left_probability(&t, 0, X, NULL) : 1.0f;
    }
    free_tree(&t);
    free_tab(&T);
}

static void make_tree_ctx(const rt_scene_desc *sc, const rt_camera_data *cam, const tree_cfg *cfg, emit_tab *T, sky_map *M, light_tree *t, int linear, tree_ctx *Y) {
    make_ctx(sc, cam, &cfg->base, T, M, linear, &Y->X);
    make_tree(sc, T, t);
    Y->tree = t;
    Y->select = cfg->select;
    Y->stats = NULL;
}

/* count samples (ijs: i, j, s) → radiance, rays, the three final RNG states; stats (ST_COUNT words, may be NULL): the tallies named above —
 * the first two are how many sampling vertices lay inside the sphere of their picked leaf's parent, and how many BSDF hits on table entries
 * were weighted */
void tree_trace(const rt_scene_desc *sc, const rt_camera_data *cam, const tree_cfg *cfg, int64_t count, const int32_t *ijs, float *radiance, int32_t *rays,
                uint32_t *seeds, uint32_t *nee_seeds, uint32_t *env_seeds, int32_t linear, int64_t *stats) {
    emit_tab T;
    sky_map M;
    light_tree t;
    tree_ctx Y;
    make_tree_ctx(sc, cam, cfg, &T, &M, &t, linear, &Y);
    if (stats) memset(stats, 0, ST_COUNT * sizeof(int64_t));
    Y.stats = stats;
    for (int64_t k = 0; k < count; ++k) {
        const v3 c = tree_sample_of(&Y, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], &rays[k], &seeds[k], &nee_seeds[k], &env_seeds[k]);
        memcpy(radiance + 3 * k, c.e, 12);
    }
    free_tree(&t);
    free_ctx(&cfg->base, &T, &M);
}

typedef struct {
    const tree_ctx *Y;
    const int32_t *rows;
    int nrows, sample_first, tid, nthreads;
    float *fb;
    double *mom;
} tree_job;

static void *tree_run(void *arg) {
    tree_job *jb = (tree_job *)arg;
    const rt_camera_data *cam = jb->Y->X.cam;
    const int W = cam->image_width;
    for (int r = jb->tid; r < jb->nrows; r += jb->nthreads) {
        const int j = jb->rows[r];
        for (int i = 0; i < W; ++i) {
            const size_t p = (size_t)r * W + i;
            v3 pixel = V(0, 0, 0);
            double m[6] = {0, 0, 0, 0, 0, 0};
            for (int s = jb->sample_first; s < jb->sample_first + cam->samples_per_pixel; ++s) {
                const v3 c = tree_sample_of(jb->Y, i, j, s, NULL, NULL, NULL, NULL);
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

/* emit_frame's sums (and moments) with the pick by cfg->select */
void tree_frame(const rt_scene_desc *sc, const rt_camera_data *cam, const tree_cfg *cfg, const int32_t *rows, int nrows, int sample_first, int threads,
                float *fb, double *mom) {
    emit_tab T;
    sky_map M;
    light_tree t;
    tree_ctx Y;
    make_tree_ctx(sc, cam, cfg, &T, &M, &t, 0, &Y);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    tree_job jobs[64];
    pthread_t tid[64];
    for (int k = 0; k < threads; ++k) {
        tree_job jb = {&Y, rows, nrows, sample_first, k, threads, fb, mom};
        jobs[k] = jb;
        pthread_create(&tid[k], NULL, tree_run, &jobs[k]);
    }
    for (int k = 0; k < threads; ++k) pthread_join(tid[k], NULL);
    free_tree(&t);
    free_ctx(&cfg->base, &T, &M);
}
