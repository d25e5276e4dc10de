/*
 * rtp_amd.h — C ABI of the MI355X-native path-tracing render library (librtp_amd.so).
 *
 * Drop-in boundary: this library replaces the reference's device side of
 *     void Camera::render(color *d_fb) const        (reference include/camera.cuh:122, src/camera.cu:198-216)
 * i.e. the launch of render_kernel (src/camera.cu:17-34) and everything it calls
 * (ray_color src/camera.cu:218-252, hit_scene include/scene.h:23, hit_bvh include/bvh.h:19,
 * hit_sphere include/sphere.h:24, hit_plane include/plane.h:57, material_scatter
 * include/materials.h:70, the RNG of include/random_utils.h:7-42).
 *
 * The reference passes its inputs through two __constant__ symbols
 * (d_cam_data_const / d_scene_data_const, src/camera.cu:14-15, written at :291 and :325) whose
 * scene pointers were cudaMalloc'd by create_scene (src/main.cu:429-474).  Here the same data are
 * passed explicitly: rt_scene_create() takes the host arrays create_scene builds, in the reference's
 * own struct layouts, and rt_render() takes the 76-byte CameraData the reference uploads per frame.
 *
 * Plain C types only; caller owns every buffer; no function exits the process
 * (the reference's checkCudaErrors calls exit(99), include/camera.cuh:20-29 — the host-side
 * mirror in ray-tracing-practice_amd/host reproduces that behaviour on top of these status codes).
 */
#ifndef RTP_AMD_H
#define RTP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = 1,   /* null pointer, negative count, index out of range in the scene */
    RT_ERR_NO_DEVICE = 2,     /* no HIP device / device ordinal out of range */
    RT_ERR_HIP = 3,           /* a HIP runtime call failed; see rt_get_last_error_string() */
    RT_ERR_UNSUPPORTED = 4,   /* scene exceeds a documented limit of this build */
    RT_ERR_OUT_OF_MEMORY = 5
} rt_status;

/* ---- reference data layouts (sizes/offsets measured on the reference's headers, x86-64) --- */

/* vec3 / point3 / color: include/vec3.h:18 — three packed floats, 12 bytes. */
typedef struct rt_vec3 { float e[3]; } rt_vec3;

/* SphereData: include/sphere.h:8-14 — __align__(16), 32 bytes. */
typedef struct rt_sphere {
    rt_vec3 center;        /* +0  */
    float   radius;        /* +12 */
    int32_t material_idx;  /* +16 */
    int32_t _pad[3];       /* +20 (alignment tail of the reference struct) */
} rt_sphere;

/* PlaneType: include/plane.h:7. */
enum { RT_PLANE_QUAD = 0, RT_PLANE_ELLIPSE = 1, RT_PLANE_TRIANGLE = 2 };

/* PlaneData: include/plane.h:9-17 — __align__(16), 80 bytes.  normal, D and w are the values
 * the reference's host-only constructor precomputes (include/plane.h:19-28). */
typedef struct rt_plane {
    int32_t type;          /* +0  */
    float   D;             /* +4  dot(normal, base) */
    int32_t material_idx;  /* +8  */
    rt_vec3 w;             /* +12 n / dot(n,n), n = cross(u,v) */
    rt_vec3 u;             /* +24 */
    rt_vec3 v;             /* +36 */
    rt_vec3 base;          /* +48 */
    rt_vec3 normal;        /* +60 unit_vector(n) */
    int32_t _pad[2];       /* +72 */
} rt_plane;

/* MaterialType: include/materials.h:12. */
enum { RT_MAT_LAMBERTIAN = 0, RT_MAT_METAL = 1, RT_MAT_DIELECTRIC = 2, RT_MAT_DIFFUSE_LIGHT = 3 };

/* MaterialData: include/materials.h:53-62 — 64 bytes.  The reference's two trailing handles
 * (cudaTextureObject_t tex_obj at +48, CpuTexture* cpu_tex at +56) are process-local; here +48
 * holds a 1-based index into rt_scene_desc.textures (0 = untextured) and +56 is reserved (0). */
typedef struct rt_material {
    int32_t  type;         /* +0  */
    float    fuzz;         /* +4  */
    float    ir;           /* +8  */
    rt_vec3  absorption;   /* +12 */
    rt_vec3  albedo;       /* +24 */
    rt_vec3  emit;         /* +36 */
    uint64_t texture_id;   /* +48 */
    uint64_t reserved;     /* +56 */
} rt_material;

/* BVHNode: include/bvh.h:7-12 — 36 bytes: AABB as x.min,x.max,y.min,y.max,z.min,z.max
 * (include/aabb.h:8, include/interval.h:7-8) then left,right,type.  Leaf <=> left < 0, then
 * right = primitive index and type = 0 sphere / 1 plane; internal nodes carry type = -1
 * (include/bvh_builder.h:61-64,92-94).  Pre-order array, root = node 0. */
typedef struct rt_bvh_node {
    float   box[6];
    int32_t left, right, type;
} rt_bvh_node;

/* CameraData: include/camera.cuh:86-95 — 76 bytes. */
typedef struct rt_camera_data {
    rt_vec3 origin;
    rt_vec3 pixel00_loc;
    rt_vec3 pixel_delta_u;
    rt_vec3 pixel_delta_v;
    rt_vec3 background;
    int32_t image_width;
    int32_t image_height;
    int32_t samples_per_pixel;
    int32_t max_depth;
} rt_camera_data;

/* CpuTexture: include/materials.h:14-18 — float RGBA rows, top row first (stbi_loadf(...,4),
 * src/main.cu:52-60).  Sampling follows tex2D_cpu (include/materials.h:20-51): gfx950 has no
 * texture units, so the device does the same software bilinear fetch from a linear buffer. */
typedef struct rt_texture {
    const float *rgba;
    int32_t width, height;
} rt_texture;

/* What the reference keeps in SceneData + BVHTree (include/scene.h:9-21, include/bvh.h:14-17). */
typedef struct rt_scene_desc {
    const rt_sphere   *spheres;   int32_t num_spheres;
    const rt_plane    *planes;    int32_t num_planes;
    const rt_material *materials; int32_t num_materials;
    const rt_bvh_node *nodes;     int32_t num_nodes;     /* the one BVH tree of the scene */
    const rt_texture  *textures;  int32_t num_textures;
} rt_scene_desc;

/* Which rows of the image one call renders.  Rows are grouped into bands of band_rows rows;
 * band b belongs to part (b % num_parts).  The call renders the rows of `part` and writes them
 * compacted, in increasing row order, into the output buffer (rt_shard_rows() rows of width
 * image_width).  {0,1,0} or a null pointer = the whole image. */
typedef struct rt_shard {
    int32_t band_rows;
    int32_t num_parts;
    int32_t part;
} rt_shard;

/* What a render call did and what it cost.  An OUT structure that grows with the library: the caller sets struct_bytes to the
 * sizeof(rt_timing) it was compiled with (rt_timing_init does) and the library writes at most that many bytes — a caller built
 * against an older, shorter header keeps working.  struct_bytes smaller than the first two fields is RT_ERR_INVALID_ARG. */
typedef struct rt_timing {
    uint32_t struct_bytes;    /* in: sizeof(rt_timing) as the caller compiled it */
    float    kernel_ms;       /* hipEvent time from the first to after the last kernel of the call, on the given stream */
    uint32_t num_workgroups;
    uint32_t workgroup_size;
    uint32_t lds_bytes;
    uint32_t scene_in_lds;    /* 1 when the whole traversal structure is LDS-resident */
    uint32_t trace_launches;  /* passes: launches of the path-tracing kernel (one per pass of samples per pixel) */
    float    trace_ms;        /* sum of the trace launches' hipEvent durations (the dominant kernel) */
    uint32_t guarded;         /* 1: guarded near-first walk + exact re-walk of flagged samples; 0: exact walk only */
    uint64_t flagged_samples; /* samples the guarded walk handed to the exact walk (0 when not guarded) */
    float    rework_ms;       /* sum of the exact re-walk launches' durations (0 when not guarded) */
    uint32_t guard_unproven;  /* 1: the guarded walk ran with rt_config.guard_gamma_ulps below the proven bound */
    uint32_t kernel;          /* RT_KERNEL_* actually used */
    uint32_t guard_dynamic;   /* 1: the guarded walk ran with distance-aware margins (rt_config.guard_dynamic_margins) */
    uint32_t wide_nodes;      /* 1: the guarded walk ran on 4-wide nodes */
    uint32_t sphere_only;     /* 1: the sphere-only build of the guarded kernel ran (rt_config.sphere_only_kernel) */
    uint32_t primary_visibility; /* 1: camera rays were resolved by the per-pixel candidate pass (rt_config.primary_visibility) */
    float    primary_ms;      /* … its launches' hipEvent durations (candidate lists + one pass per trace launch) */
    uint32_t trace_vgprs;     /* vector registers per lane of the trace kernel that ran, as the loaded code object reports them */
    uint32_t trace_scratch_bytes; /* … and its scratch (spill) bytes per lane */
    uint32_t abandoned_passes; /* guarded passes that gave up part-way because too many of their samples were being flagged
                                  (rt_config.guard_bail_share): the exact walk rendered those passes whole */
    uint64_t traced_samples;  /* samples the trace kernel worked on: all of them, or with the primary-visibility pass those of the pixels
                                  some leaf can be hit through (the others got the background without any per-sample work) */
    uint32_t guard_paused;    /* 1: this handle has stepped aside to the exact walk for its next frames (a frame abandoned a pass or
                                  flagged more than the bail share of its samples; rt_config.guard_keep = 1 prevents it) */
    uint32_t front_primitives; /* primitives the guarded walk tested at the start of every ray instead of keeping them in its tree
                                  (rt_config.guard_front_primitives); 0 when the exact walk ran */
    uint32_t dark_kernel;     /* 1: the sphere-only kernel behind the primary-visibility pass ran in its build for scenes without emitters
                                  (rt_config.dark_kernel): no radiance carried, each ray's sphere-test constants instead (2: a developer
                                  build of it without those constants, RTP_DARK_CARRY=0); 0 with sphere_only, primary_visibility and
                                  scene_in_lds all 1: the build that carries radiance ran (render_emit_kernel) */
} rt_timing;
/* *t = zeros with struct_bytes = sizeof(rt_timing). */
void rt_timing_init(rt_timing *t);

typedef struct rt_scene rt_scene;   /* opaque: device-resident repacked scene */

/* Library configuration.  The reference has no equivalent (its launch shape is hard-coded,
 * src/camera.cu:200-204); everything that changes how THIS library renders travels through this struct,
 * never through the environment.  rt_config_init() fills the defaults; 0 in a field marked "0 = auto"
 * means the library decides.  Results are the same bits for every setting except where a field says
 * otherwise. */
enum { RT_TRAVERSAL_AUTO = 0, RT_TRAVERSAL_EXACT = 1, RT_TRAVERSAL_GUARDED = 2 };
enum { RT_BUILD_HOST_SAH = 0, RT_BUILD_DEVICE_LBVH = 1 };
enum { RT_KERNEL_AUTO = 0, RT_KERNEL_MEGA = 1, RT_KERNEL_WAVEFRONT = 2 /* retired experiment: rendering answers RT_ERR_UNSUPPORTED */ };
typedef struct rt_config {
    uint32_t struct_bytes;        /* sizeof(rt_config) as the caller compiled it */
    /* --- fixed at rt_scene_create_ex ------------------------------------------------------------ */
    int32_t  tree_build;          /* RT_BUILD_*: who builds the guarded walk's own tree */
    float    guard_gamma_ulps;    /* rounding budget of hit_sphere's discriminant, in units of 2^-24 |oc|^2 |d|^2, that
                                     the guarded walk's leaf margins cover.  0 = the proven bound (24).  A smaller
                                     positive value is an UNPROVEN margin: opt-in, reported in rt_timing.guard_unproven */
    int32_t  guard_exact_leaf_table; /* 1: always upload the exact leaf boxes as a table (developer) */
    /* --- may be changed between frames with rt_scene_set_config ----------------------------------- */
    int32_t  traversal;           /* RT_TRAVERSAL_*: AUTO = guarded near-first walk where the scene is eligible and
                                     has at least guard_min_primitives primitives, else the reference-order walk.  AUTO also
                                     MEASURES: a guarded frame that flagged more than 0.4 % of its samples is followed by one
                                     frame on the exact walk, and the handle keeps whichever cost less per sample (same bits
                                     either way).  GUARDED / EXACT: that walk, no measuring */
    int32_t  guard_min_primitives;/* default 64: below that the exact walk's tree is a few levels deep and the second launch the
                                     guarded walk needs costs more than it saves (random scenes of 20-60 spheres: 1.3-1.4 x slower) */
    int32_t  guard_keep;          /* 1: keep the guarded walk even after a frame that flagged more than the bail share of its samples */
    int32_t  guard_repack;        /* 1 (default): re-pack the guarded tree for a camera outside the reach it was sized for */
    int32_t  kernel;              /* RT_KERNEL_*: AUTO picks per scene */
    uint64_t workspace_bytes;     /* budget of the per-pass sample workspace the scene handle owns (12 bytes per sample of a
                                     pass, allocated on demand).  0 = default: a sixteenth of the device's memory.  A smaller
                                     budget means more, shorter passes: 4 GiB costs 1.9 % at 1920x1080x500 spp.  Footprint: rows are
                                     padded to 32 samples (128-byte lines; to 4 samples for passes shorter than 32), so a pass of S
                                     samples per pixel takes pixels x round_up(S, 32) x 12 bytes */
    int32_t  pass_spp;            /* samples per pixel per pass (0 = auto: what the workspace admits) */
    int32_t  stack_levels;        /* cap on the guarded walk's per-lane stack entries (0 = auto) */
    uint32_t flag_capacity;       /* cap on the flagged-sample list (0 = auto; overflow = "re-walk everything") */
    int32_t  scene_in_lds;        /* 1 (default): stage tables in LDS when they fit; 0: read them through L1/L2 */
    int32_t  lds_treelet;         /* 1 (default): scenes too big for LDS keep the top of their tree there */
    int32_t  workgroups_per_cu;   /* 0 = auto */
    int32_t  k_inner, k_shade;    /* wave scheduling thresholds in lanes (0 = defaults: 24 / 48; 32 / 52 for the LDS-resident guarded walk, 48 / 52 for big scenes with distance-aware margins) */
    int32_t  reserve_chunk;       /* work indices per queue reservation in units of 64 (0 = auto) */
    int32_t  reserve_taper;       /* 1 (default): reservations shrink towards the end of a pass */
    int32_t  wavefront_paths;     /* (RT_KERNEL_WAVEFRONT, retired: ignored) */
    int32_t  wavefront_exchange;  /* (RT_KERNEL_WAVEFRONT, retired: ignored) */
    int32_t  wide_nodes;          /* 0 (default): scenes with distance-aware margins (guard_dynamic_margins) walk the 4-wide form of their tree —
                                     half the dependent record loads per ray, and with the growth of the boxes in parametric form fewer
                                     instructions as well (BASELINE configs[4] +1.7 %) —, every other scene child-pair nodes; -1: pair nodes
                                     always; 1: 4-wide nodes for every guarded walk — a retired experiment, 6 % slower than the octant
                                     pair walk on S-rtiow: rendering answers RT_ERR_UNSUPPORTED */
    int32_t  guard_dynamic_margins; /* (fixed at create) margins of the guarded walk's small spheres: 0 = auto (distance-aware
                                     where one margin per sphere would exceed a quarter of the smallest radius), 1 = always one
                                     margin per sphere, 2 = always distance-aware */
    int32_t  sphere_only_kernel;  /* 0 (default): scenes without planes, textures and absorbing dielectrics are rendered by the sphere-only
                                     build of the guarded kernel (64 registers per lane, 8 waves per SIMD instead of 6; the same frame bit
                                     for bit) — the LDS-resident octant walk where the tables fit, the pair walk through L1 / L2 with
                                     distance-aware margins beyond; -1: always the general kernel */
    int32_t  overlap_rework;      /* 0 (default): the exact re-walk of flagged samples and the accumulation of their pixels run on a
                                     second stream of the handle beside the accumulation of all other pixels; -1: one after the other */
    int32_t  primary_visibility;  /* 0 (default): where the guarded walk's tables are LDS-resident, the first hit of every camera ray
                                     comes from a per-pixel candidate list (the leaves the pixel's cone of rays can reach, made once per
                                     frame; 80 bytes per pixel of device memory, taken on demand — without it the frame is rendered the
                                     other way) instead of a walk per sample; pixels no leaf can be hit through get the background
                                     without any per-sample work, the others are traced expensive ones first — the same frame bit for
                                     bit; -1: camera rays walk the tree */
    int32_t  guard_bail_share;    /* what the guarded walk may cost before it steps aside, as the share of flagged samples in 1/256ths
                                     (0 = default: 64, i.e. 25 % — measured break-even is 21-26 % of a frame's samples; -1: never).
                                     Inside a pass: once the flagged share of the samples handed out so far exceeds it AND 9.4 % of the
                                     whole pass is on the list AND the pass is still in its first quarter, the waves stop fetching and
                                     the exact walk renders the WHOLE pass (bounded loss: what the guarded launch had done).  Between frames: a frame that abandoned a
                                     pass, or flagged more than this share overall, makes the handle use the exact walk from then on —
                                     found at the next render call from what the previous one left in host memory, no rt_last_timing
                                     needed.  Below it RT_TRAVERSAL_AUTO decides by measurement (see traversal) */
    int32_t  guard_front_primitives; /* (fixed at create) 0 (default): up to four primitives that span the scene — a leaf box of at least half
                                     the surface of everything that is left: a ground sphere, a floor quad — are not leaves of the guarded
                                     walk's tree; every ray tests them when it is armed, all lanes of a wave together, and walks with their
                                     hit as its closest so far (the same frame bit for bit: the guarded walk's result does not depend on
                                     the order of its tests); -1: every primitive is a leaf of the tree */
    int32_t  reuse_view_lists;    /* 0 (default): the per-pixel candidate lists of the primary-visibility pass and the fetch order made from
                                     them are kept with the handle, and a call with the same camera, image, shard and tree on the same
                                     stream (the next batch of a progressive render, the next frame of a still) does not make them again
                                     (0.4 ms at 1920x1080); -1: every call makes them (bench.py: every timed frame does all of a frame's work) */
    int32_t  resume_flagged;      /* 0 (default): the exact re-walk of a sample the guarded walk flagged goes on from the ray that was flagged —
                                     the path's state at that point is left in a 17 MB table of the handle (a sample whose slot is taken, or
                                     that was flagged inside a shade step, is redone from its camera ray as before); -1: every flagged
                                     sample is redone from the camera.  The same frame bit for bit: up to the flagged ray both walks agree */
    int32_t  dark_kernel;         /* 0 (default): a scene in which nothing emits — every material's emit is +0.0f bit for bit, no albedo component
                                     beyond 1 in magnitude — that rt_render gives to the sphere-only kernel behind the primary-visibility pass is
                                     traced by that kernel's variant without a radiance accumulator (the radiance of such a path is +0 until it
                                     leaves the scene), which keeps each ray's |d|^2 and fp64 reciprocal for all its sphere tests in the freed
                                     registers; the same frame bit for bit; -1: never */
} rt_config;

/* ---- entry points -------------------------------------------------------------------------- */

/* Select the HIP device this thread's subsequent calls use (hipSetDevice). */
rt_status rt_set_device(int32_t device_ordinal);

/* Replaces create_scene's upload block (src/main.cu:429-474) and gpu_render's
 * cudaMemcpyToSymbol(d_scene_data_const) (src/camera.cu:291): validates the arrays, repacks them
 * to the device layout and uploads them once. */
rt_status rt_scene_create(const rt_scene_desc *desc, rt_scene **out_scene);

/* Defaults into *cfg.  rt_config grows with the library, like rt_timing: the macro hands over the size the CALLER was compiled
 * with and the library writes at most that many bytes (struct_bytes = that size) — a caller built against an older, shorter
 * header keeps working.  A binding that calls the exported function rt_config_init itself (ctypes, cgo: no macro) gets the
 * library's own sizeof(rt_config) and has to mirror the struct of the library it loads. */
void rt_config_init_sized(rt_config *cfg, uint32_t struct_bytes);
void rt_config_init(rt_config *cfg);
#define rt_config_init(cfg) rt_config_init_sized((cfg), (uint32_t)sizeof(rt_config))
/* Developer convenience for test harnesses and tools: overlays the RTP_* environment variables (RTP_TRAVERSAL,
 * RTP_BUILD, RTP_SLAB_GIB, RTP_PASS_SPP, …; list in INTEGRATION.md) onto *cfg.  The library itself never reads
 * the environment: a host that wants this behaviour calls it explicitly. */
void rt_config_from_env(rt_config *cfg);
/* rt_scene_create with a configuration (NULL = defaults). */
rt_status rt_scene_create_ex(const rt_scene_desc *desc, const rt_config *cfg, rt_scene **out_scene);
/* Replace the render-time fields of the scene's configuration (the create-time fields are ignored). */
rt_status rt_scene_set_config(rt_scene *scene, const rt_config *cfg);
/* The scene's configuration into *cfg: at most cfg->struct_bytes bytes (set by rt_config_init; below 8: RT_ERR_INVALID_ARG). */
rt_status rt_scene_get_config(const rt_scene *scene, rt_config *cfg);

/* Replaces destroy_scene_arrays / destroy_texture_resources (src/main.cu:235-246,322-344). */
rt_status rt_scene_destroy(rt_scene *scene);

/* Which closest-hit walk rt_render uses for this scene.  "" = the guarded near-first walk with an
 * exact re-walk of flagged samples (sphere-only scenes whose tables fit LDS); otherwise the reason
 * the scene only gets the reference-order walk (e.g. "scene has planes").  Results are the same
 * bits either way; this is a diagnostic.  The string lives as long as the scene. */
const char *rt_scene_guard_reason(const rt_scene *scene);

/* Number of rows rt_render writes for (image_height, shard). */
int32_t rt_shard_rows(int32_t image_height, const rt_shard *shard);

/* Replaces cudaMemcpyToSymbol(d_cam_data_const) + render_kernel<<<>>> + cudaDeviceSynchronize
 * (src/camera.cu:325,204-206).  d_fb_sum is DEVICE memory, rt_shard_rows()*image_width*3 floats,
 * row-major; like the reference's framebuffer it receives the SUM over samples_per_pixel of the
 * per-sample radiance, added in sample order (src/camera.cu:27-33).  hip_stream is a hipStream_t
 * (NULL = default stream).  With sync != 0 the call waits for the kernel and fills `timing`
 * (may be NULL); with sync == 0 it only enqueues (timing->kernel_ms is then read later with
 * rt_last_kernel_ms()).
 * Limits: at most 2^24 pixels per call (rt_shard_rows() x image_width; 4K = 2^23) and samples_per_pixel <= 65536 —
 * RT_ERR_UNSUPPORTED beyond.  The scene must have been created on the calling thread's current device
 * (RT_ERR_INVALID_ARG otherwise).  One handle renders one frame at a time: calls on the same handle must be
 * issued to the same stream or separated by a synchronisation.  (With rt_config.overlap_rework the handle runs part of a
 * pass on a second, non-blocking stream of its own; that stream is forked from and joined to hip_stream with events inside the
 * call, so to the caller everything still happens in hip_stream's order.) */
rt_status rt_render(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard,
                    float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);

/* The same for a RECTANGLE of the image (tile_x0, tile_y0, w, h): d_fb_sum is tile_h rows of tile_w pixels, row-major;
 * pixel (x, y) of the tile is pixel (tile_x0 + x, tile_y0 + y) of the image — the same seeds, the same camera rays, the same
 * sums, so tiles of any shape assemble to the bits of the whole frame.  RT_ERR_INVALID_ARG for a tile that leaves the image. */
rt_status rt_render_tile(rt_scene *scene, const rt_camera_data *cam, int32_t tile_x0, int32_t tile_y0, int32_t tile_w, int32_t tile_h,
                         float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);

/* rt_render for samples sample_first … sample_first + samples_per_pixel - 1 of every pixel instead of 0 … samples_per_pixel - 1: the
 * seeds of those samples (pixel (i, j), sample s: wang_hash(wang_hash(base(i, j) + s)), as always), added in sample order into sums
 * that start from 0 — d_fb_sum is overwritten, not added onto.  Successive calls with sample_first = 0, S, 2S, … are fresh samples
 * of the same image (what a temporal filter needs from a still camera).  rt_render is this call with sample_first = 0.
 * RT_ERR_INVALID_ARG: sample_first < 0.  RT_ERR_UNSUPPORTED: sample_first + samples_per_pixel above 2^30 (the kernels carry sample
 * indices as int32).  Both before anything is enqueued.  Rows of a shard only: tiles and rt_context have no such call. */
rt_status rt_render_samples(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard, int32_t sample_first,
                            float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);

/* ---- first-hit AOVs: the per-pixel buffers a denoiser and a compositor want, from the beauty frame's own camera samples -----
 * For pixel (i, j) and sample s = 0 … samples_per_pixel-1, in sample order: the reference's camera ray (get_ray with the seed of
 * the beauty pass) and its first hit, hit_scene over Interval(0.001, 1e30) as in ray_color.  A hit adds
 *     albedo_sum += m.albedo (times the texel tex2D_cpu gives at the hit, for a textured material) for LAMBERTIAN and METAL,
 *                   (1, 1, 1) for DIELECTRIC and DIFFUSE_LIGHT;
 *     normal_sum += rec.normal, the face-forwarded normal set_face_normal leaves;
 *     depth_sum  += rec.t, the RAY PARAMETER — camera directions are not unit length, so this is not a distance;
 *     hit_count  += 1;
 * a miss adds the camera's background to albedo_sum and nothing else.  first_prim is the code 2 * index + type (type 0 sphere /
 * 1 plane) of sample 0's hit, -1 if sample 0 misses.  Sums are float32, start at 0 and are added one sample at a time in sample
 * order.  max_depth plays no part.  Buffers are compacted like d_fb_sum (rt_shard_rows() x image_width pixels, or tile_h x tile_w),
 * so rows, shards and tiles assemble to the bits of the whole frame.
 * An IN structure that grows with the library: the caller sets struct_bytes to the sizeof(rt_aov_buffers) it was compiled with
 * (rt_aov_buffers_init does) and the library reads at most that many bytes; fields past them count as NULL.  All pointers are
 * DEVICE memory and each may be NULL (that buffer is not written); all of them NULL, or struct_bytes below 16, is
 * RT_ERR_INVALID_ARG. */
typedef struct rt_aov_buffers {
    uint32_t struct_bytes;    /* in: sizeof(rt_aov_buffers) as the caller compiled it */
    uint32_t reserved;        /* 0 */
    float    *albedo_sum;     /* 3 floats per pixel */
    float    *normal_sum;     /* 3 floats per pixel */
    float    *depth_sum;      /* 1 float per pixel */
    uint32_t *hit_count;      /* 1 per pixel */
    int32_t  *first_prim;     /* 1 per pixel */
} rt_aov_buffers;
/* *b = all NULL with struct_bytes = sizeof(rt_aov_buffers). */
void rt_aov_buffers_init(rt_aov_buffers *b);

/* The AOVs of a frame, a shard of its rows or a tile: the argument checks, limits, stream contract and pass planning of rt_render
 * and rt_render_tile.  Where the handle takes camera rays from per-pixel candidate lists (rt_config.primary_visibility) those
 * lists and the primary pass resolve the samples, sharing the handle's lists with its beauty frames (rt_config.reuse_view_lists);
 * the samples they cannot vouch for, and every sample elsewhere, get the reference-order walk.  The call leaves the handle's own
 * decisions — its choice of walk, a pause of the guarded walk, the re-pack of its tree for a far camera — as a sequence of
 * rt_render calls alone would leave them, and rt_last_timing keeps describing the last rt_render.
 * timing (may be NULL) with sync != 0: kernel_ms, primary_visibility, primary_ms (candidate lists and primary passes),
 * traced_samples (the samples of pixels some leaf can be hit through, or all of them), flagged_samples (the samples the
 * reference-order walk resolved) and rework_ms (the launches that walk whole pixels, or every sample: the few single samples the
 * candidate lists leave undecided are walked inside the accumulation); every other field 0.  With sync == 0 only
 * primary_visibility is filled. */
rt_status rt_render_aov(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard, const rt_aov_buffers *buffers,
                        void *hip_stream, int32_t sync, rt_timing *timing);
rt_status rt_render_aov_tile(rt_scene *scene, const rt_camera_data *cam, int32_t tile_x0, int32_t tile_y0, int32_t tile_w, int32_t tile_h,
                             const rt_aov_buffers *buffers, void *hip_stream, int32_t sync, rt_timing *timing);
/* rt_render_aov for samples sample_first … sample_first + samples_per_pixel - 1, with the checks of rt_render_samples: the sums start
 * from 0 and first_prim is the hit of sample sample_first.  rt_render_aov is this call with sample_first = 0. */
rt_status rt_render_aov_samples(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard, int32_t sample_first,
                                const rt_aov_buffers *buffers, void *hip_stream, int32_t sync, rt_timing *timing);

/* ---- denoising: an edge-avoiding à-trous wavelet filter guided by the first-hit AOVs ----------------------------------------
 * The spatial filter of SVGF (Dammertz et al. 2010, Schied et al. 2017; no temporal part) over a whole image: a beauty frame as
 * rt_render writes it (the sum over samples) and the AOV sums rt_render_aov wrote for the same camera.  W x H buffers of a frame
 * rendered without a shard, or of one tile treated as an image of its own.
 *
 * The arithmetic is part of the contract: float32, evaluated in the order written, nothing fused, divisions and sqrtf correctly
 * rounded, exp = the host libm's expf (the library's exp_libm restates it bit for bit for every float).  S = samples_per_pixel,
 * inv = (float)(1.0 / (double)S) as rt_tonemap computes it.  A pixel is a HIT pixel when hit_count > 0.
 *   Sky pixels (hit_count == 0): out = fb_sum bit for bit; a sky pixel is never a tap of another pixel.
 *   Prepass, per hit pixel:  c_k = fb_sum_k * inv,  a_k = albedo_sum_k * inv,  d_k = fmaxf(a_k, 1e-3f),  L_k = c_k / d_k;
 *     len2 = (N.x*N.x + N.y*N.y) + N.z*N.z with N = normal_sum,  n_k = N_k / sqrtf(len2)  (n = 0 when len2 == 0);
 *     z = depth_sum / (float)hit_count;   lum(L) = (0.2126f*L0 + 0.7152f*L1) + 0.0722f*L2.
 *   Second prepass, per hit pixel p:
 *     var_p: over the 3x3 window (dy = -1..1 outer, dx = -1..1 inner), hit pixels inside the image only, l = lum(L):
 *       m1 += l, m2 += l*l, k += 1 (float, from 0);  var = fmaxf(0, m2/k - (m1/k)*(m1/k)).
 *     gz_p = gx + gy,  gx = fminf(|z(x+1) - z_p|, |z_p - z(x-1)|) where a neighbour outside the image or not a hit pixel gives
 *       +inf for its term; gx = 0 when both are missing.  gy the same along y.
 *   Iteration i = 0 … iterations-1, step s = 2^i, per hit pixel p:
 *     rl = 1 / (sigma_luminance * sqrtf(var_p) + 1e-4f);   rz[m] = 1 / ((sigma_depth * gz_p) * (float)(s*m) + 1e-4f), m = 0…4;
 *     taps q = p + s*(dx, dy), dy = -2..2 outer, dx = -2..2 inner, skipping taps outside the image or not hit pixels; W, ΣL_k,
 *     ΣV start at 0;  per tap:
 *       h  = kern[|dx|] * kern[|dy|],  kern = {3/8, 1/4, 1/16};
 *       wn = fmaxf(0, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z), then wn = wn*wn, normal_squarings times;
 *       e  = |z_p - z_q| * rz[|dx|+|dy|] + |l_p - l_q| * rl;       w = (h * wn) * exp(-e);
 *       W += w;  ΣL_k += w * L_q,k;  ΣV += (w*w) * var_q;
 *     L'_p = ΣL / W, var'_p = ΣV / (W*W); W == 0 keeps L and var.  The next iteration reads L' and var' (and l = lum(L')).
 *   Remodulation, per hit pixel: out_k = (L_k * d_k) * (float)S  (with iterations = 0: the prepass's L).
 * d_out has d_fb_sum's convention (the sum over samples), so rt_tonemap with the caller's divisor and the savers take it as they
 * take a beauty frame. */
typedef struct rt_denoise_params {   /* IN, grows like rt_aov_buffers: the library reads at most struct_bytes; later fields keep
                                        their defaults.  struct_bytes below 8 is RT_ERR_INVALID_ARG */
    uint32_t struct_bytes;           /* sizeof(rt_denoise_params) as the caller compiled it */
    int32_t  iterations;             /* 5; 0 … 8 (the last step is 2^7 = 128 pixels) */
    float    sigma_depth;            /* 1.0 (> 0, finite) */
    float    sigma_luminance;        /* 4.0 (> 0, finite) */
    int32_t  normal_squarings;       /* 7: the normal weight is max(0, n_p·n_q)^(2^7); 0 … 10 */
} rt_denoise_params;
/* Defaults into *p, struct_bytes = sizeof(rt_denoise_params). */
void rt_denoise_params_init(rt_denoise_params *p);
/* Bytes of device workspace rt_denoise needs for a width x height image (64 per pixel and 256 for alignment; 0 when width or
 * height is below 1).  Any alignment of d_workspace is accepted. */
uint64_t rt_denoise_workspace_bytes(int32_t width, int32_t height);
/* Enqueues the filter on hip_stream (NULL = default stream): no allocation, no synchronisation.  All pointers are DEVICE memory;
 * aov->albedo_sum, normal_sum, depth_sum and hit_count are required (first_prim is not used).  params NULL = defaults.
 * RT_ERR_INVALID_ARG: a required pointer NULL, width or height below 1, samples_per_pixel outside 1 … 65536, a parameter outside
 * its range, workspace_bytes below rt_denoise_workspace_bytes, d_out overlapping an input or the workspace, or the workspace
 * overlapping an input.  RT_ERR_UNSUPPORTED: width x height above 2^24 (rt_render's limit).  Every check comes before any HIP
 * call. */
rt_status rt_denoise(const float *d_fb_sum, const rt_aov_buffers *aov, int32_t width, int32_t height, int32_t samples_per_pixel,
                     const rt_denoise_params *params, void *d_workspace, uint64_t workspace_bytes, float *d_out, void *hip_stream);
/* rt_denoise of the two frames rt_render_lit_split writes, filtered separately with the same guides and parameters and added:
 * d_out = rt_denoise(d_direct_sum) + rt_denoise(d_indirect_sum) per channel, bit for bit (float32, one add).  rt_denoise's launches run
 * once per component, then one kernel adds.  The workspace holds rt_denoise's and one frame behind it:
 * rt_denoise_split_workspace_bytes = rt_denoise_workspace_bytes + 12 bytes per pixel (0 when width or height is below 1).
 * Checks: RT_ERR_INVALID_ARG for a NULL d_direct_sum or d_indirect_sum, then rt_denoise's own in its order — each input, d_out and the
 * workspace of the larger size stand where rt_denoise's stand.  The two inputs may be the same buffer.  Every check comes before any HIP call. */
uint64_t rt_denoise_split_workspace_bytes(int32_t width, int32_t height);
rt_status rt_denoise_split(const float *d_direct_sum, const float *d_indirect_sum, const rt_aov_buffers *aov, int32_t width, int32_t height,
                           int32_t samples_per_pixel, const rt_denoise_params *params, void *d_workspace, uint64_t workspace_bytes, float *d_out,
                           void *hip_stream);

/* ---- temporal denoising: SVGF's reprojected history across the frames of an animation ----------------------------------------
 * rt_denoise's filter fed with colour and luminance moments accumulated over earlier frames (Schied et al. 2017, §4.1-4.2): each hit
 * pixel is reprojected into the history the previous call wrote, blended with it, and the variance that steers the à-trous weights
 * comes from the accumulated moments once the history is long enough.  The image size and S come from cam (HOST memory); the
 * other inputs are rt_denoise's plus first_prim (all five AOV buffers required).
 *
 * The arithmetic extends rt_denoise's contract (same rules: float32 in the order written, nothing fused, correctly rounded division
 * and sqrtf, exp = expf).  Fixed constants: tau2 = 0.0025f (a tap's hit point within 0.05 of the pixel's distance from the camera),
 * min_weight = 0.01f, max_len = 32.0f, min_alpha = 0.2f, moments_len = 4.0f, min_normal_dot = 0.9f.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2.
 *   Prepass and second prepass: rt_denoise's, giving per hit pixel L_cur, d, n, z, gz and the 3x3 spatial variance var_sp.
 *   Temporal pass, per hit pixel p = (x, y), with prim = first_prim_p and m1 = lum(L_cur):
 *     pc_k = (P00_k + (float)x * du_k) + (float)y * dv_k,  X_k = O_k + z * (pc_k - O_k)  (the camera cam: O origin, P00 pixel00_loc,
 *       du, dv pixel_delta_u / v);  OX = X - O,  reach2 = tau2 * dot(OX, OX).
 *     The history is EMPTY when history_prev is NULL or its header is not one this call writes for this width and height (an
 *       all-zero buffer is empty).  Otherwise, with the history's camera (O', P00', du', dv'):
 *       N = cross(du', dv') = (du'1*dv'2 - du'2*dv'1, du'2*dv'0 - du'0*dv'2, du'0*dv'1 - du'1*dv'0);  E = P00' - O',  D = X - O';
 *       t = dot(E, N) / dot(D, N); the pixel reprojects only when 0 < t < +inf (in front of the old camera, not on its plane);
 *       R_k = t * D_k - E_k,  u = dot(R, du') / dot(du', du'),  v = dot(R, dv') / dot(dv', dv');  and only when -1 < u < W, -1 < v < H.
 *       x0 = floorf(u), y0 = floorf(v), fx = u - x0, fy = v - y0.  Taps q = (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) in that
 *       order, bilinear weights w = (fx or 1 - fx) * (fy or 1 - fy); a tap counts when it lies inside the image, its history length
 *       len_q > 0 (it was a hit pixel), first_prim_q == prim, dot(n_p, n_q) >= min_normal_dot and dot(X_q - X, X_q - X) <= reach2
 *       (X_q - X per component).  Over the taps that count, from 0: W += w, S_k += w * Lh_q,k, SM1 += w * M1_q, SM2 += w * M2_q,
 *       SN += w * len_q.
 *     With W >= min_weight: len = fminf(SN / W + 1, max_len), a = fmaxf(min_alpha, 1 / len), b = 1 - a;
 *       L_k = b * (S_k / W) + a * L_cur,k,  M1 = b * (SM1 / W) + a * m1,  M2 = b * (SM2 / W) + a * (m1 * m1).
 *     Otherwise (empty history, no reprojection, W < min_weight) the pixel is disoccluded: L = L_cur, M1 = m1, M2 = m1 * m1, len = 1.
 *     var = len >= moments_len ? fmaxf(0, M2 - M1 * M1) : var_sp.
 *   Iterations: rt_denoise's, on (L, var).  Remodulation: rt_denoise's (with iterations = 0: of L).  Sky pixels: out = fb_sum bit for bit.
 * With an empty history d_out is rt_denoise's output bit for bit.
 *
 * History buffer (rt_denoise_history_bytes, 16-byte aligned): a 256-byte header — uint32 magic 0x31485452, int32 width, int32 height,
 * uint32 0, the 76-byte rt_camera_data the history was made with, zeros — then four planes of W x H records of four floats:
 *   colour  (L'_0, L'_1, L'_2, var')  iteration 0's output, the colour the next frame reprojects (with 0 iterations: (L, var))
 *   moments (M1, M2, len, prim)       prim as its int32 bits
 *   position (X_0, X_1, X_2, 0)   normal (n_0, n_1, n_2, 0)
 * A sky pixel's four records are all zero (len = 0).  The call's kernels write the whole of history_next; the caller swaps prev and
 * next between frames and may hipMemset a fresh buffer to 0 (or pass NULL) for a first frame or a cut.  Because the two buffers are
 * distinct, a call can be replayed. */
/* Bytes of one history buffer for a width x height image (64 per pixel and the 256-byte header; 0 when width or height is below 1). */
uint64_t rt_denoise_history_bytes(int32_t width, int32_t height);
/* Enqueues the temporal filter on hip_stream (NULL = default stream): no allocation, no synchronisation.  The workspace is rt_denoise's
 * (rt_denoise_workspace_bytes).  params NULL = defaults.
 * RT_ERR_INVALID_ARG: a required pointer NULL, the image width or height below 1, samples_per_pixel outside 1 … 65536, a parameter
 * outside its range, workspace_bytes or history_bytes below their size functions, a history buffer not 16-byte aligned,
 * history_next overlapping history_prev, an input, the workspace or d_out, d_out overlapping an input, the workspace or
 * history_prev, or the workspace overlapping an input or history_prev.  RT_ERR_UNSUPPORTED: more than 2^24 pixels.  Every check
 * comes before any HIP call. */
rt_status rt_denoise_temporal(const float *d_fb_sum, const rt_aov_buffers *aov, const rt_camera_data *cam, const rt_denoise_params *params,
                              const void *d_history_prev, void *d_history_next, uint64_t history_bytes,
                              void *d_workspace, uint64_t workspace_bytes, float *d_out, void *hip_stream);

/* ---- adaptive sampling: per pixel, samples until a noise target or a cap -----------------------------------------------------
 * Instead of samples_per_pixel for every pixel, each pixel gets samples in rounds until the standard error of its mean luminance is
 * small enough or max_spp is reached.
 *
 * Per-pixel parity (the central promise).  Pixel p receives n_p samples, namely samples 0 … n_p - 1, and d_fb_sum[p] equals, bit for
 * bit, pixel p of rt_render with samples_per_pixel = n_p: the sum added in sample order, starting from 0.  d_spp[p] = n_p, and n_p is
 * min_spp + k * batch_spp for some k >= 0 with n_p <= max_spp.  cam->samples_per_pixel is ignored.
 *
 * Statistics.  Per sample, with (r, g, b) the radiance rt_render adds for it: y = (0.2126f*r + 0.7152f*g) + 0.0722f*b (rt_denoise's lum);
 * S1 += y and S2 += y*y, float32, from 0, in sample order, nothing fused.  When d_moments is not NULL it receives (S1, S2) per pixel
 * (2 floats per pixel, compacted like d_fb_sum).  A pixel no leaf can be hit through (primary visibility) adds the background's y once
 * per sample, like every other pixel's miss.
 *
 * Rule.  With R = (max_spp - min_spp) / batch_spp (integer division) rounds after the min_spp samples, the rule is evaluated after the
 * min_spp samples and after every round but the last.  For a pixel with n samples (float32, in this order, nothing fused, division
 * correctly rounded; t = threshold):
 *     mean = S1 / (float)n;   var = fmaxf(0, (S2 - S1 * mean) / (float)(n - 1));
 *     goes_on = n + batch_spp <= max_spp && (t == 0 || var / (float)n > (t * t) * (mean * mean + 1e-4f))
 * A pixel goes on to the next round iff it went on in every earlier judgement and goes_on holds now; a pixel that stops never
 * resumes.  So every pixel of round r (1 … R) has min_spp + (r - 1) * batch_spp samples as it starts and gets the next batch_spp.
 * In C:
 *     int n = min_spp; for (int r = 1; r <= R; ++r) { if (!goes_on(S1, S2, n)) break; add samples n … n + batch_spp - 1; n += batch_spp; }
 *     n_p = n;
 * threshold = 0 never stops early: n_p = min_spp + R * batch_spp everywhere.  A NaN radiance makes var NaN and stops the pixel.
 *
 * Limits and checks: rt_render's (at most 2^24 pixels, its stream contract, a shard's rows or the whole frame; no tiles, no
 * rt_context).  Before anything is enqueued: RT_ERR_INVALID_ARG for params NULL or struct_bytes below 8, min_spp < 2, batch_spp < 1,
 * max_spp < min_spp, a threshold that is negative, NaN or infinite, d_fb_sum or d_spp NULL (and rt_render's own checks);
 * RT_ERR_UNSUPPORTED for max_spp above 65536, or pixels x batch_spp at or above 2^31 - 4096 when there is a round.
 *
 * Work.  All R rounds are enqueued up front; which pixels go on, and how many, lives on the device only, and a round whose list is
 * empty costs a few empty launches.  With sync == 0 the call only enqueues (it may wait for the stream once, when it grows the
 * handle's buffers, as rt_render does for its slab).  The rounds walk the scene in the reference's order (the exact walk) with
 * every sample traced from the camera.
 * Handle state: the min_spp samples are an ordinary rt_render frame — its walk, its feedback and RT_TRAVERSAL_AUTO's decisions count
 * like an rt_render's, and rt_last_timing then describes that frame alone.  The rounds leave the handle's decisions alone, as
 * rt_render_aov does.  timing (may be NULL) with sync != 0: what rt_last_timing reports for the min_spp frame, except kernel_ms (from
 * the first to the last kernel of the whole call) and trace_launches (+ R). */
typedef struct rt_adaptive_params {   /* IN, grows like rt_denoise_params: the library reads at most struct_bytes; later fields keep
                                         their defaults.  struct_bytes below 8 is RT_ERR_INVALID_ARG */
    uint32_t struct_bytes;            /* sizeof(rt_adaptive_params) as the caller compiled it */
    int32_t  min_spp;                 /* 16: samples every pixel gets first (>= 2) */
    int32_t  batch_spp;               /* 16: samples added per round to each pixel still going on (>= 1) */
    int32_t  max_spp;                 /* 256: cap (>= min_spp, <= 65536); n_p <= min_spp + R * batch_spp <= max_spp */
    float    threshold;               /* 0.02: relative standard error of the mean luminance to stop at (>= 0, finite; 0 = never stop early) */
} rt_adaptive_params;
/* Defaults into *p, struct_bytes = sizeof(rt_adaptive_params). */
void rt_adaptive_params_init(rt_adaptive_params *p);
/* d_fb_sum: 3 floats per pixel, d_spp: 1 int32 per pixel, d_moments: NULL or 2 floats per pixel — DEVICE memory, compacted like
 * rt_render's buffer (rt_shard_rows() x image_width pixels). */
rt_status rt_render_adaptive(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard, const rt_adaptive_params *params,
                             float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing);
/* rt_tonemap of an adaptive frame: d_rgb8[3p + c] = u8(256*clamp(sqrt(d_fb_sum[3p + c] * inv_p), 0, 0.999)) with
 * inv_p = (float)(1.0 / (double)d_spp[p]) — rt_tonemap's arithmetic at divisor n_p, so each pixel's bytes equal rt_tonemap's of the
 * uniform frame at n_p.  num_pixels pixels; device pointers; enqueued on hip_stream. */
rt_status rt_tonemap_spp(const float *d_fb_sum, const int32_t *d_spp, uint8_t *d_rgb8, int64_t num_pixels, void *hip_stream);

/* ---- the stopping rule of the adaptive calls: rule 1, the neighbourhood rule -----------------------------------
 * rt_render_adaptive_rule is rt_render_adaptive with a choice of stopping rule.  stop == NULL or rule == 0: rt_render_adaptive, bit for
 * bit — the same kernels and launches.  rule == 1 changes goes_on alone: the statistics, the rounds, R, the counts n_p = min_spp +
 * k * batch_spp and the per-pixel parity promise are rt_render_adaptive's.
 *
 * Rule 1.  At a judgement where the pixels still going on have n samples (float32, in this order, nothing fused, division correctly
 * rounded; t = threshold):
 *     mean    = S1 / (float)n;   var = fmaxf(0, (S2 - S1 * mean) / (float)(n - 1));
 *     noisy_p = var / (float)n > (t * t) * (mean + 0.01f)
 *     c_p     = (p is still going on) && noisy_p
 *     goes_on_p = n + batch_spp <= max_spp && (t == 0 || c_q holds for some q in N(p))
 * A NaN makes noisy_p false.  threshold = 0 never stops early, as under rule 0.
 * The window.  N(p) is p and those of its 8 image neighbours that lie in the call's buffer: at the image border the window is clipped.
 * Under a shard a row above or below counts only when it is a row of the same band of this part — the two rows are adjacent both in
 * the image and in the compacted buffer; a pixel on the first or last row of a band sees no row of another part.  So the frame of a
 * sharded render is NOT the rows of the whole frame's render under rule 1 (under rule 0 it is): each part is a frame of its own.
 * Stopping.  A pixel goes on iff it went on in every earlier judgement and goes_on_p holds now; a pixel that stops never resumes.  It
 * stops only when its whole window, itself included, is quiet, so its own c is false from then on and its statistics are frozen: the
 * rule never reads a neighbour's count.
 * Checks: rt_render_adaptive's, and right after its rt_adaptive_params checks RT_ERR_INVALID_ARG for stop->struct_bytes below 8 or a
 * rule outside 0 … 1 (the message names rt_render_adaptive_rule) — before anything is enqueued.  Limits, stream contract, handle state,
 * timing and the max_depth <= 0 case (counts by the rule: min_spp, or min_spp + R * batch_spp when threshold = 0) are
 * rt_render_adaptive's.  Work under rule 1: two small launches per judgement instead of one, and one byte per pixel on the handle. */
typedef struct rt_stop_params {       /* IN, grows like rt_adaptive_params: the library reads at most struct_bytes; below 8 = RT_ERR_INVALID_ARG */
    uint32_t struct_bytes;            /* sizeof(rt_stop_params) as the caller compiled it */
    int32_t  rule;                    /* 0 (default): the pixel's own relative error (rt_render_adaptive); 1: the neighbourhood rule */
    int32_t  reserved[2];             /* 0 */
} rt_stop_params;
/* Defaults into *p, struct_bytes = sizeof(rt_stop_params). */
void rt_stop_params_init(rt_stop_params *p);
rt_status rt_render_adaptive_rule(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard, const rt_adaptive_params *params,
                                  const rt_stop_params *stop, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream,
                                  int32_t sync, rt_timing *timing);
/* Probe (tests): ONE judgement of either rule over device arrays, through the kernels the rounds launch — so that the window logic
 * can be fed moments nobody rendered.  The buffer is rows x width pixels (rows: of the call's buffer — a shard's compacted rows;
 * shard gives band_rows and num_parts, NULL = one band); d_moments: (S1, S2) per pixel; d_going_on_in: one byte per pixel, non-zero =
 * the pixel is still going on with n samples (NULL = every pixel); d_goes_on_out: one byte per pixel, 1 = it goes on to the next
 * round, else 0.  params gives batch_spp, max_spp and threshold (min_spp is checked and otherwise unused).  Every byte of the mask set
 * takes the first judgement's launches (every pixel), anything else a round's (a list).  Allocates, copies and waits: not for a hot
 * path.  RT_ERR_INVALID_ARG: rt_render_adaptive's parameter checks, the stop checks above, width or rows below 1, n below 2, a bad
 * shard, d_moments or d_goes_on_out NULL; RT_ERR_UNSUPPORTED: more than 2^24 pixels. */
rt_status rt_adaptive_judge(int32_t width, int32_t rows, const rt_shard *shard, const rt_adaptive_params *params, const rt_stop_params *stop,
                            int32_t n, const float *d_moments, const uint8_t *d_going_on_in, uint8_t *d_goes_on_out, void *hip_stream);

/* ---- denoising an adaptively sampled frame: rt_denoise with per-pixel counts and the samples' own variance -------
 * rt_denoise's filter for the whole-frame outputs of rt_render_adaptive or rt_render_lit_adaptive: d_fb_sum, d_spp and, optionally,
 * d_moments.  Each pixel is normalised and remodulated by its own count, and with d_moments the variance that steers the luminance
 * edge-stopping is the variance of the pixel's mean luminance as its own samples estimate it (SVGF's per-pixel variance, Schied et
 * al. 2017 §4.2, filtered by the paper's 3x3 Gaussian) instead of the 3x3 spatial estimate.  aov holds the sums of rt_render_aov[_samples]
 * or rt_render_aov_lens for the same camera at a uniform aov_samples per pixel (typically min_spp); albedo_sum, normal_sum, depth_sum
 * and hit_count are required.  The workspace is rt_denoise's (rt_denoise_workspace_bytes), params rt_denoise_params.
 *
 * The arithmetic extends rt_denoise's contract (same rules: float32 in the order written, nothing fused, correctly rounded division
 * and sqrtf, exp = expf).  n = d_spp[p], inv_p = (float)(1.0 / (double)n) as rt_tonemap_spp computes it, A = aov_samples,
 * invA = (float)(1.0 / (double)A).  A pixel is a HIT pixel when hit_count > 0 and n >= 1.
 *   Every other pixel (sky, or a count below 1): out = fb_sum bit for bit; such a pixel is never a tap of another pixel.
 *   Prepass, per hit pixel:  c_k = fb_sum_k * inv_p,  a_k = albedo_sum_k * invA,  d_k = fmaxf(a_k, 1e-3f),  L_k = c_k / d_k;
 *     n (the unit normal), z and lum are rt_denoise's.
 *   Sample variance (only with d_moments; (S1, S2) the pixel's moments):  v = 0 when n < 2; otherwise
 *     mean = S1 / (float)n,  vs = fmaxf(0, (S2 - S1 * mean) / (float)(n - 1))  (rt_render_adaptive's var),  vm = vs / (float)n,
 *     dl = lum(d_0, d_1, d_2),  v = vm / (dl * dl): the variance of the mean luminance carried into demodulated space as if the
 *     albedo were grey.
 *   Second prepass, per hit pixel p:  gz_p is rt_denoise's.  With d_moments == NULL var_p is rt_denoise's 3x3 luminance variance.
 *     With d_moments it is the 3x3 Gaussian of v: dy = -1..1 outer, dx = -1..1 inner, hit pixels inside the image only,
 *     g = k[|dx|] * k[|dy|] with k = {1/2, 1/4};  G += g,  SV += g * v_q  (both from 0);  var_p = SV / G.
 *   Iterations: rt_denoise's, on (L, var).
 *   Remodulation, per hit pixel: out_k = (L_k * d_k) * (float)n  (with iterations = 0: the prepass's L).
 * d_out has an adaptive frame's convention (each pixel the sum over its own n samples): rt_tonemap_spp(d_out, d_spp, …) takes it.
 * Identities, bit for bit: with d_moments == NULL and every d_spp[p] == S == aov_samples, d_out is rt_denoise's at S; out == fb_sum on
 * every pixel that is not a hit pixel.
 *
 * Enqueues on hip_stream (NULL = default stream): no allocation, no synchronisation.  All pointers but aov and params are DEVICE
 * memory.  RT_ERR_INVALID_ARG: a required pointer (d_spp included) NULL, width or height below 1, aov_samples outside 1 … 65536, a
 * parameter outside its range, workspace_bytes below rt_denoise_workspace_bytes, d_out or the workspace overlapping an input (d_spp
 * counts as 4 bytes per pixel, d_moments as 8) or each other.  RT_ERR_UNSUPPORTED: more than 2^24 pixels.  Every check comes before
 * any HIP call. */
rt_status rt_denoise_spp(const float *d_fb_sum, const int32_t *d_spp, const float *d_moments /* NULL or 2 floats per pixel */,
                         const rt_aov_buffers *aov, int32_t aov_samples, int32_t width, int32_t height,
                         const rt_denoise_params *params, void *d_workspace, uint64_t workspace_bytes, float *d_out, void *hip_stream);

/* ---- temporal denoising of adaptively sampled frames: rt_denoise_temporal with per-pixel counts ----------------
 * rt_denoise_temporal's reprojected history for the whole-frame outputs of rt_render_adaptive[_rule] or rt_render_lit_adaptive[_rule]
 * (pinhole frames: the reprojection is a pinhole's): d_fb_sum, d_spp and, optionally, d_moments, as rt_denoise_spp takes them.  The
 * history is blended with the frame by the samples behind each, not by frames, and the variance of the blend is propagated through
 * it.  aov holds the sums of rt_render_aov[_samples] for the same camera at a uniform aov_samples per pixel; all five buffers are
 * required, first_prim included.  cam (HOST memory) supplies the image size and the reprojection camera; its samples_per_pixel is
 * ignored.  The workspace is rt_denoise_workspace_bytes, each history rt_denoise_history_bytes.
 *
 * The arithmetic extends the contracts above (same rules: float32 in the order written, nothing fused, correctly rounded division
 * and sqrtf, exp = expf; rt_denoise_temporal's constants and dot).
 *   Hit pixels, prepass, sample variance and second prepass: rt_denoise_spp's (n = d_spp[p], inv_p, invA; a HIT pixel has hit_count > 0
 *     and n >= 1), giving per hit pixel L_cur, d, n, z, gz and var_cur: with d_moments the 3x3 Gaussian of v, without it rt_denoise's
 *     3x3 spatial variance.  The second prepass always runs, also with iterations = 0.
 *   Every pixel that is not a hit pixel: out = fb_sum bit for bit, its four history records are zero, and it is never a tap.
 *   Temporal pass, per hit pixel p = (x, y), with prim = first_prim_p, m1 = lum(L_cur) and nf = (float)n:
 *     X, reach2, the projection, the four taps in their order and the four conditions of a tap that counts are rt_denoise_temporal's.
 *       The history is EMPTY when history_prev is NULL or its header is not one this call writes for this width, height and use of
 *       d_moments (an all-zero buffer and a history of rt_denoise_temporal are empty).  With cnt_q and V_q the fourth floats of tap
 *       q's position and normal records, the taps that count accumulate, from 0: W += w, S_k += w * Lh_q,k, SM1 += w * M1_q,
 *       SM2 += w * M2_q, SN += w * len_q, SC += w * cnt_q, SV += w * V_q.
 *     With W >= min_weight: len = fminf(SN / W + 1, max_len);  ch = SC / W,  s = ch + nf,  a = nf / s,  cnt = s;  when !(a >= min_alpha):
 *       a = min_alpha and cnt = nf / min_alpha;  b = 1 - a;
 *       L_k = b * (S_k / W) + a * L_cur,k,  M1 = b * (SM1 / W) + a * m1,  M2 = b * (SM2 / W) + a * (m1 * m1);
 *       V = (b * b) * (SV / W) + (a * a) * var_cur.
 *     Otherwise the pixel is disoccluded: L = L_cur, M1 = m1, M2 = m1 * m1, len = 1, cnt = nf, V = var_cur.
 *     With d_moments: var = V.  Without: var = len >= moments_len ? fmaxf(0, M2 - M1 * M1) : var_cur.
 *   Iterations: rt_denoise's, on (L, var).  Remodulation, per hit pixel: out_k = (L_k * d_k) * nf  (with iterations = 0: of L).
 * d_out has an adaptive frame's convention: rt_tonemap_spp(d_out, d_spp, …) takes it.
 * Identity, bit for bit: with an empty history and iterations >= 1, d_out is rt_denoise_spp's output, with and without d_moments.
 *
 * History buffer: rt_denoise_temporal's size, header layout and planes, with uint32 magic 0x32485452, the header's fourth word 1
 * when written without d_moments and 2 when written with, cnt in the position record's fourth float and V in the normal record's:
 *   colour (L'_0, L'_1, L'_2, var')   moments (M1, M2, len, prim)   position (X_0, X_1, X_2, cnt)   normal (n_0, n_1, n_2, V)
 * rt_denoise_temporal takes a history of this call as empty, and this call one of rt_denoise_temporal's or of the other use of
 * d_moments: alternating the calls on one pair of buffers restarts the history each time.
 *
 * Enqueues on hip_stream (NULL = default stream): no allocation, no synchronisation.  All pointers but aov, cam and params are DEVICE
 * memory.  The checks are rt_denoise_temporal's, in its order and with its codes, with d_spp required, aov_samples outside 1 … 65536
 * where it checks samples_per_pixel, and d_spp (4 bytes per pixel) and d_moments (8) among the inputs of every overlap check.  Every
 * check comes before any HIP call. */
rt_status rt_denoise_temporal_spp(const float *d_fb_sum, const int32_t *d_spp, const float *d_moments /* NULL or 2 floats per pixel */,
                                  const rt_aov_buffers *aov, int32_t aov_samples, const rt_camera_data *cam,
                                  const rt_denoise_params *params, const void *d_history_prev, void *d_history_next, uint64_t history_bytes,
                                  void *d_workspace, uint64_t workspace_bytes, float *d_out, void *hip_stream);

/* ---- a history-aware stopping rule: the adaptive calls with a prior from rt_denoise_temporal_spp's history ---------
 * In an animation denoised by rt_denoise_temporal_spp a pixel whose blended estimate is already quiet need not be sampled to the
 * frame's own target again.  rt_adaptive_prior turns the history the next rt_denoise_temporal_spp will read into a PRIOR per pixel
 * of the frame about to be rendered, (ch, vh): the samples behind the pixel's reprojected history and the variance of its mean
 * luminance in the frame's own space.  The _prior calls are the _rule calls whose rules compare ve, the variance that
 * rt_denoise_temporal_spp's blend will carry for the pixel (before its spatial filter), where the _rule calls compare the variance
 * vm of the frame's own mean.  Pinhole frames: the reprojection is a pinhole's.
 *
 * rt_adaptive_prior covers a whole frame of cam (HOST memory: image size and reprojection camera; samples_per_pixel ignored).  aov
 * holds the sums of rt_render_aov[_samples] for that frame at a uniform aov_samples = A per pixel; all five buffers are required.
 * d_prior receives 2 floats per pixel.  Arithmetic by the rules of the denoise sections (float32 in the order written, nothing fused,
 * correctly rounded division and sqrtf), invA = (float)(1.0 / (double)A):
 *   A pixel with hit_count == 0: (0, 0).
 *   A hit pixel p = (x, y): the unit normal n and the depth z are rt_denoise's prepass, prim = first_prim_p,
 *     d_k = fmaxf(albedo_sum_k * invA, 1e-3f), dl = lum(d_0, d_1, d_2).
 *     X, reach2, the projection, the four taps in their order and the four conditions of a tap that counts are rt_denoise_temporal's.
 *     The history is taken only when d_history_prev is non-NULL, has magic 0x32485452, this width and height and the mode word 2
 *     (written with moments); anything else — NULL, all zero, another size, rt_denoise_temporal's magic, mode 1 — is EMPTY.
 *     The taps that count accumulate, from 0: W += w, SC += w * cnt_q, SV += w * V_q.
 *     With a history taken and W >= min_weight: ch = SC / W, vh = (SV / W) * (dl * dl) — rt_denoise_spp's v = vm / (dl * dl) undone.
 *     Otherwise (0, 0).
 * Reads the moments, position and normal planes of the history, never the colour plane.  Enqueues one launch on hip_stream: no
 * allocation, no synchronisation.  The checks are rt_denoise_temporal_spp's, in its order and with its codes, under this call's name
 * and all before any HIP call: a NULL aov, cam or d_prior, a missing AOV buffer, width or height below 1, A outside 1 … 65536
 * (RT_ERR_INVALID_ARG); more than 2^24 pixels (RT_ERR_UNSUPPORTED); with a history given, history_bytes below
 * rt_denoise_history_bytes; a history that is not 16-byte aligned; d_prior (8 bytes per pixel) overlapping the history or an AOV buffer
 * (RT_ERR_INVALID_ARG). */
rt_status rt_adaptive_prior(const rt_aov_buffers *aov, int32_t aov_samples, const rt_camera_data *cam, const void *d_history_prev,
                            uint64_t history_bytes, float *d_prior, void *hip_stream);
/* The _rule calls with a prior: their arguments, then d_prior — DEVICE memory, 2 floats (ch, vh) per LOCAL pixel, compacted like d_spp
 * (under a shard the caller supplies the part's rows of a whole-frame prior).  d_prior == NULL: the _rule call bit for bit, the same
 * kernels and launches.  At a judgement of a pixel with n samples, nf = (float)n, t = threshold (float32, in this order, nothing fused):
 *     mean = S1 / nf;   var = fmaxf(0, (S2 - S1 * mean) / (float)(n - 1));   vm = var / nf;
 *     if (ch > 0 && vh >= 0) { s = ch + nf;  a = nf / s;  if (!(a >= 0.2f)) a = 0.2f;  b = 1 - a;  ve = (b * b) * vh + (a * a) * vm; }
 *     else ve = vm;
 *     rule 0:  goes_on = n + batch_spp <= max_spp && (t == 0 || ve > (t * t) * (mean * mean + 1e-4f))
 *     rule 1:  noisy_p = ve > (t * t) * (mean + 0.01f);  the window, c_p and goes_on_p are rt_render_adaptive_rule's
 * a and b are rt_denoise_temporal_spp's blend weights.  A NaN ch or vh fails the test: the pixel is judged by its own samples.  A prior
 * of all zeros gives ve = vm, the expression the _rule calls compare: that frame is the _rule call's bit for bit.  Everything else is
 * the _rule call's: statistics, rounds, R, the counts min_spp + k * batch_spp, a pixel that stops never resumes, the per-pixel parity
 * promise (each pixel bit-identical to rt_render / rt_render_lit at its own count), threshold = 0, and the max_depth <= 0 case, where
 * the prior is not read.  Checks: the _rule call's, with its messages; right after its stop checks, and so before anything is
 * enqueued, RT_ERR_INVALID_ARG when d_prior (8 bytes per local pixel, as cam and shard give their number) overlaps d_fb_sum, d_spp or
 * d_moments — the message names the _prior call. */
rt_status rt_render_adaptive_prior(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard, const rt_adaptive_params *params,
                                   const rt_stop_params *stop, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream,
                                   int32_t sync, rt_timing *timing, const float *d_prior);
/* (rt_render_lit_adaptive_prior, the same on the lit path, is declared beside rt_render_lit_adaptive_rule below) */
/* rt_adaptive_judge with a prior (tests): its arguments, then d_prior (2 floats per pixel of the buffer; NULL: rt_adaptive_judge's
 * launches).  Its checks under this call's name, and RT_ERR_INVALID_ARG when d_prior overlaps d_goes_on_out. */
rt_status rt_adaptive_judge_prior(int32_t width, int32_t rows, const rt_shard *shard, const rt_adaptive_params *params,
                                  const rt_stop_params *stop, int32_t n, const float *d_moments, const uint8_t *d_going_on_in,
                                  uint8_t *d_goes_on_out, void *hip_stream, const float *d_prior);

/* ---- thin-lens depth of field and shutter motion blur ---------------------------------------------------------
 * rt_render_samples / rt_render_aov_samples with a camera that has a lens and / or an open shutter.  Pixel (i, j), sample s; the
 * draws come from the same RNG as the pinhole's, and the path goes on from the state they leave:
 *   1. the seed is as always; ox, oy are drawn exactly as the pinhole camera draws them;
 *   2. time, only when cam_close != NULL: tau = random_float; each of origin, pixel00_loc, pixel_delta_u and pixel_delta_v becomes
 *      X = X0 + tau * (X1 - X0) per component (0: cam_open, 1: cam_close);
 *   3. lens, only when lens_radius > 0: (lx, ly) by rejection, as random_in_unit_sphere does it — repeat
 *      lx = random_range(-1, 1); ly = random_range(-1, 1) (x first) while lx*lx + ly*ly >= 1;
 *   4. pinhole ray: S = (((P00 + i*du) + j*dv) + ox*du) + oy*dv (i, j as floats), D = S - O.  With lens_radius == 0 the ray is (O, D);
 *   5. thin lens, otherwise: n = cross(du, dv) = (du1*dv2 - du2*dv1, du2*dv0 - du0*dv2, du0*dv1 - du1*dv0);
 *      dimg = fabsf(dot(P00 - O, n)) / sqrtf(dot(n, n)); k = focus_distance / dimg; focus point F = O + k*D;
 *      uh = du / sqrtf(dot(du, du)), vh = dv / sqrtf(dot(dv, dv)); lens point L = (O + (R*lx)*uh) + (R*ly)*vh; the ray is (L, F - L).
 * Float32 throughout, in the order written, nothing fused, division and sqrtf correctly rounded.  With cam_close == NULL and
 * lens_radius == 0 the call is rt_render_samples / rt_render_aov_samples bit for bit.  Sums run over samples sample_first … in sample
 * order, starting from 0.
 * Checks and limits: rt_render_samples's (rows of a shard only: no tiles, no rt_context).  Before anything is enqueued,
 * RT_ERR_INVALID_ARG for: cam_close differing from cam_open in width, height, spp, max_depth or background; a negative, NaN or
 * infinite lens_radius; with the lens on, a focus_distance that is not positive and finite, or a camera (either end) with
 * dot(P00 - O, n) == 0.  A pose between the ends can still degenerate; then the arithmetic above defines the result.
 * Handle state: the calls leave the handle's own decisions alone, as rt_render_aov does — its walk choice, a pause of the guarded walk,
 * the re-pack of its tree, its cached view lists and what rt_last_timing reports.  The guarded walk serves a lens frame only where every
 * ray origin it can make lies within the reach its margins were sized for; otherwise the exact walk runs (timing->guarded says which).
 * Results are the same bits on every walk.  timing (may be NULL): this call's record (kernel_ms and flagged_samples with sync != 0). */
typedef struct rt_lens_params {   /* IN, grows like rt_adaptive_params: the library reads at most struct_bytes; < 8 = RT_ERR_INVALID_ARG */
    uint32_t struct_bytes;        /* sizeof(rt_lens_params) as the caller compiled it */
    float    lens_radius;         /* 0 (default): pinhole, no lens draws.  >= 0, finite, world units */
    float    focus_distance;      /* 10: distance of the plane in focus from the camera origin along the image plane's normal
                                     (> 0, finite; read only when lens_radius > 0) */
} rt_lens_params;
/* Defaults into *p, struct_bytes = sizeof(rt_lens_params). */
void rt_lens_params_init(rt_lens_params *p);
/* rt_render_samples with a camera that has a lens and / or an open shutter (cam_close NULL: no motion; lens NULL: defaults). */
rt_status rt_render_lens(rt_scene *scene, const rt_camera_data *cam_open, const rt_camera_data *cam_close, const rt_lens_params *lens,
                         const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);
/* rt_render_aov_samples with the same camera rays (first hit of the lens / motion ray). */
rt_status rt_render_aov_lens(rt_scene *scene, const rt_camera_data *cam_open, const rt_camera_data *cam_close, const rt_lens_params *lens,
                             const rt_shard *shard, int32_t sample_first, const rt_aov_buffers *buffers, void *hip_stream, int32_t sync,
                             rt_timing *timing);
/* Probe for tests, HOST memory: the camera ray of n (i, j, s) samples (ijs: 3 int32 each; origins, directions: 3 floats each), made by
 * the device code the kernels inline, and the RNG state after the camera's draws (final_seed: 1 word each).  Runs on the current
 * device. */
rt_status rt_lens_camera_rays(const rt_camera_data *cam_open, const rt_camera_data *cam_close, const rt_lens_params *lens,
                              int32_t n, const int32_t *ijs, float *origins, float *directions, uint32_t *final_seed);

/* ---- next-event estimation: direct light sampling of emissive spheres with MIS ---------------------------------
 * rt_render_samples with one light sample at every diffuse event, combined with the path's own (BSDF) sample by multiple importance
 * sampling.  The estimator has rt_render's expectation; float32 throughout, in the order written, nothing fused, division and sqrtf
 * correctly rounded.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2; random_float(s): s = wang_hash(s), (float)s / 2^32.
 *   Emitter table (built on a handle's first rt_render_nee and kept): the spheres, in sphere order, with radius > 0 whose material's
 *     emit components are all finite and >= 0 and not all 0.  w_i = (e0 + e1 + e2) * r^2, summed in double; cdf_i = (float)(prefix
 *     sum through i / total), the last one 1; pmf_i = cdf_i - cdf_{i-1} in float (cdf_{-1} = 0): the probability the pick below
 *     gives.  Emissive planes are found by the path alone (weight 1) unless sample_planes = 1 (below); other emitters always are.
 *   Streams: the path draws exactly what rt_render_samples draws, from the same seed.  The light samples draw from their own state,
 *     nee = wang_hash(wang_hash(base + s) ^ RT_NEE_STREAM_KEY), base = wang_hash(i * W + j), with random_float.
 *   Diffuse event: a LAMBERTIAN hit, or a METAL hit whose branch draw chose the hemisphere branch, at the point x of closest-hit query
 *     k (the camera ray is query 0), with face-forwarded normal n, albedo a (texture-modulated) and throughput beta before it is
 *     multiplied by the attenuation.  When k + 1 < max_depth and the table is not empty, one light sample; its draws stop at the
 *     first step that gives no contribution:
 *     1. u = random_float(nee); e = the smallest entry with u < cdf_e; none (u == 1): no contribution.
 *     2. (c, r) = sphere e; w = c - x; d2 = dot(w, w); rr = r * r; !(d2 > rr): none; cos_max = sqrtf(1 - rr / d2); om = 1 - cos_max;
 *        om <= 0: none; pdf_cone = 1 / (RT_NEE_TWO_PI * om).
 *     3. u1 = random_float(nee); cos_t = 1 - u1 * om; sin_t = sqrtf(fmaxf(0, 1 - cos_t * cos_t)); then (px, py) by rejection: repeat
 *        px = -1 + 2 * random_float(nee), py = -1 + 2 * random_float(nee) (x first) while q2 = px*px + py*py is >= 1 or == 0;
 *        q = sqrtf(q2), cx = px / q, cy = py / q.  len = sqrtf(d2), wn = (w0 / len, w1 / len, w2 / len); the basis of Duff et al.
 *        2017: sg = copysignf(1, wn2), ba = -1 / (sg + wn2), bb = (wn0 * wn1) * ba,
 *        t1 = (1 + ((sg * wn0) * wn0) * ba, sg * bb, -sg * wn0), t2 = (bb, sg + (wn1 * wn1) * ba, -wn1);
 *        sx = sin_t * cx, sy = sin_t * cy; wl_k = (t1_k * sx + t2_k * sy) + wn_k * cos_t.
 *     4. !(dot(wl, n) > 0): none.  Otherwise the shadow ray (x, wl): its closest hit over (0.001, 1e30) in the reference's visit order
 *        contributes only if it is sphere e.  pb = RT_NEE_PB, pl = pmf_e * pdf_cone,
 *        f = mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;  contribution_k = ((beta_k * a_k) * emit_e,k) * f.
 *   BSDF hits: the hit of the query k + 1 ray that leaves a diffuse event at x, on a sphere e of the table, adds
 *     (beta_k * emit_k) * w_b instead of beta_k * emit_k: w_b = mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0 ? 0 : 1), with
 *     pl = pmf_e * pdf_cone by step 2 from x (0 where step 2 gives none).  Every other emission term — camera rays, hits after
 *     DIELECTRIC or specular METAL events, planes, spheres outside the table — and the background keep weight 1.
 *   Order: at each vertex the emission term first, then the vertex's light sample; sums over samples sample_first … in sample order
 *     from 0.  Where no diffuse event takes a light sample (an empty table, a scene without diffuse surfaces) the call is
 *     rt_render_samples bit for bit.
 *   sample_planes = 1 (read only when struct_bytes >= 12, an older 8-byte caller gets 0): the emitter table also holds the
 *     emissive QUAD, ELLIPSE and TRIANGLE planes.  Its entries are the spheres of the table above, in sphere order, then the planes, in
 *     plane order, whose type is one of the three, whose material's (any type) emit components are all finite and >= 0 and not all 0,
 *     and whose area A is finite and > 0: A = (float)(k * sqrt(dot(n, n))) in double, n = cross(u, v) in double from the float u, v,
 *     k = 1 (QUAD), pi / 4 (ELLIPSE), 1 / 2 (TRIANGLE).  Weights in double: a sphere's (e0 + e1 + e2) * r^2 as above, a plane's
 *     (e0 + e1 + e2) * A / pi (both: emission x largest projected area / pi); cdf and pmf as above.  A scene without such a plane has
 *     the same table under both settings, and every call is then sample_planes = 0 bit for bit.  A handle keeps both tables.
 *     The light sample is step 1, then by the kind of entry e: a sphere takes steps 2 to 4; plane e (rt_plane base, u, v, normal) takes
 *     2p. QUAD: a = random_float(nee), b = random_float(nee).  TRIANGLE: the same two draws, then if a + b > 1: a = 1 - a, b = 1 - b.
 *         ELLIPSE: step 3's rejection loop (px first) repeated while q2 >= 1; a = 0.5f + 0.5f * px, b = 0.5f + 0.5f * py.
 *         y_k = (base_k + a * u_k) + b * v_k.
 *     3p. w = y - x; d2 = dot(w, w); !(d2 > 0): none; len = sqrtf(d2); wl_k = w_k / len; cos_l = fabsf(dot(normal, wl));
 *         !(cos_l >= 1e-8f): none; pa = d2 / (cos_l * A); pl = pmf_e * pa.
 *     4p. !(dot(wl, n) > 0): none.  Otherwise the shadow ray (x, wl): its closest hit over (0.001, 1e30) in the reference's visit order
 *         contributes only if it is plane e (a sample whose ray misses its own plane by rounding at the rim counts nothing); f and the
 *         contribution are step 4's with this pl and the plane's material's emit.  Emission is two-sided: no facing test on the light.
 *     BSDF hits: the hit of the query k + 1 ray that leaves a diffuse event at x, on a plane e of the table at the point p, is weighted
 *     by w_b with pl from step 3p for w = p - x (0 where 3p gives none).  Planes outside the table keep weight 1.
 *   select = 1 (read only when struct_bytes >= 16, an older caller gets 0): the entry of a light sample is picked by a light
 *     tree — a bounding-sphere hierarchy over the entries of the table that sample_planes selects, descended by an importance that knows
 *     the shaded point (Conty Estevez and Kulla 2018).  select = 0 runs the kernels of the power table, bit for bit.  A handle keeps a tree
 *     per table, built on the first call that selects it, from the read-back the tables are made from.  An empty table samples nothing
 *     under either setting.
 *     Tree: built on the host in double from the float scene data, over the table's N entries in table order.  Entry e has a centre c_e,
 *       a radius rho_e and its table weight w_e (above, in double).  Sphere: its centre and r.  QUAD and ELLIPSE: c_k = (base_k + 0.5 * u_k)
 *       + 0.5 * v_k, rho = 0.5 * max(|u + v|, |u - v|).  TRIANGLE: c_k = base_k + (u_k + v_k) / 3, rho = the largest of |base - c|,
 *       |(base + u) - c|, |(base + v) - c|.  |a| = sqrt((a0*a0 + a1*a1) + a2*a2).
 *       The node over a list S of entries: m_k = 0.5 * (min_e(c_e,k - rho_e) + max_e(c_e,k + rho_e)), R = max_e(|c_e - m| + rho_e); stored
 *       as float: centre (float)m_k, radius nextafterf((float)R, +inf), weight W = (float)(sum over S of w_e / sum over all entries of w_e),
 *       both sums in list order.  |S| = 1: a leaf naming its entry.  Otherwise the split axis is the one on which the centres c_e extend
 *       furthest (max - min; ties: x, then y, then z); S is sorted by that coordinate with a stable sort (equal coordinates keep list
 *       order); the left child is the node over the first ceil(|S| / 2), the right child the node over the rest, and the node stores the
 *       fallback q = (float)(W_left / (W_left + W_right)) of the children's double sums.  Nodes are numbered in preorder (a node, its left
 *       subtree, its right subtree).  Entry e has a path of depth_e <= ceil(log2 N) steps: bit i set when step i goes right, LSB first.
 *     Pick (in place of step 1; the steps 2 to 4 and 2p to 4p follow from the same state): p = 1.0f at the root.  At an interior node, for
 *       each child c (centre m, radius R, weight W as stored): w = m - x; d2 = dot(w, w); I_c = W / fmaxf(d2, R * R).  s = I_L + I_R;
 *       pL = (s > 0 && s < INFINITY) ? I_L / s : q.  u = random_float(nee), one fresh draw per level: u < pL goes left with p = p * pL,
 *       otherwise right with p = p * (1.0f - pL).  At the leaf e is its entry and pmf_e(x) = p takes the place of the table's pmf_e in pl;
 *       f and the contribution are unchanged.  A tree of one entry draws nothing and has pmf = 1: select = 1 is not select = 0 bit for bit
 *       even there (the table's pick draws u).  The importance knows distance and extent only: no normal or orientation term.
 *     BSDF hits: the table entry of the hit is found as above; pmf_e(x) is the same product, computed root-down along the entry's stored
 *       path from the ray's origin x, with the same expressions in the same order, and w_b is as written (pl = 0 gives weight 1: an entry
 *       the pick cannot reach from x).
 * Checks and limits: rt_render_samples's (rows of a shard only: no tiles, no rt_context); every refusal comes before anything is
 *   glossy = 1 (read only when struct_bytes >= 20, an older caller gets 0): METAL's reflect branch takes light samples too.
 *     glossy = 0 is the call as written above, bit for bit.  The same switch exists in rt_env_params — its mode must be 1 or 2 to matter —
 *     and acts on that light; rt_render_lit and its adaptive forms read each light's switch from its own params.
 *     pg(w; r, fuzz), the density in solid angle of unit(r + fuzz * B), B uniform in the unit ball, r a unit vector — the integral of
 *       t^2 over the chord the direction w cuts through the ball of radius fuzz about r, over the ball's volume:
 *         c = dot(w, r); ff = fuzz * fuzz; disc = (c * c - 1) + ff; !(disc > 0): pg = 0.  s = sqrtf(disc); t2 = c + s; !(t2 > 0): pg = 0.
 *         t1 = c - s; f3 = ff * fuzz.  t1 > 0: pg = (s * (3 * (c * c) + s * s)) / (RT_NEE_TWO_PI * f3) — the factored form, no
 *         cancellation; otherwise (fuzz > 1: the vertex is inside the ball) pg = ((t2 * t2) * t2) / ((2 * RT_NEE_TWO_PI) * f3).
 *     Glossy event: a METAL hit at query k whose branch draw chose the reflect branch (random_float < 0.8f), with
 *       fuzz >= RT_GLOSSY_MIN_FUZZ, k + 1 < max_depth, the light on (a table that is not empty) and its glossy = 1.  Below that fuzz the
 *       event is a mirror as before: no sample, and its ray keeps weight 1 (unbiased: the choice depends on the vertex alone; and pg, at
 *       most about 1 / (pi fuzz^2), stays finite).  r = reflect(unit(d), n) as the path computes it; the main stream draws what it draws
 *       without the switch — the branch draw, the point in the unit sphere — and new_d = r + fuzz * in_sphere, absorbed when
 *       !(dot(new_d, n) > 0), is the same next ray.
 *     Its light sample: the steps above (1, then 2 to 4 or 2p to 4p; the tree's pick under select = 1) from the nee state, the same draws
 *       in the same order, with pb = pg(wl; r, fuzz) in place of RT_NEE_PB in f — wl as the steps give it — and one more way to give no
 *       contribution after !(dot(wl, n) > 0): pb == 0.  The draws are consumed either way; a sample without contribution casts no shadow
 *       ray (rt_trace_samples_*'s rays do not count one).  contribution_k = ((beta_k * a_k) * emit_e,k) * f with the METAL's albedo a.
 *       The sample is taken whether or not new_d is absorbed: it estimates the branch's integral, independently of the path's draw.
 *     The ray that leaves a glossy event carries pc = pg(unit(new_d); r, fuzz): its hit on a table entry is weighted by w_b with pc in
 *       place of pb (light alone: pl > 0 ? 0 : 1), and pc == 0 — pg rounded to 0 at the lobe's rim — means weight 1, never 0 / 0.
 *     Identities, bit for bit: glossy = 1 on a scene without METAL of fuzz >= RT_GLOSSY_MIN_FUZZ, or with an empty table, = glossy = 0.
 * Checks and limits: rt_render_samples's (rows of a shard only: no tiles, no rt_context); every refusal comes before anything is
 * enqueued; RT_ERR_INVALID_ARG for params with struct_bytes below 8, mis outside {0, 1}, sample_planes outside {0, 1}, select outside
 * {0, 1} or glossy outside {0, 1} (checked in that order).  The light samples run on the
 * reference-order walk only.  Handle state: the call leaves the handle's own decisions alone, as rt_render_lens does — its walk choice,
 * a pause of the guarded walk, the re-pack of its tree, its cached view lists and what rt_last_timing reports; timing (may be NULL)
 * is this call's record (kernel_ms with sync != 0). */
#define RT_NEE_STREAM_KEY 0x4E454531u
#define RT_NEE_TWO_PI 6.28318548f          /* (float)(2 pi) */
#define RT_NEE_PB 0.159154937f             /* (float)(1 / (2 pi)): the density of the uniform-hemisphere direction */
#define RT_GLOSSY_MIN_FUZZ 0.0009765625f   /* 2^-10: a METAL reflect branch below this fuzz is a mirror — no light sample (glossy = 1) */
typedef struct rt_nee_params {   /* IN, grows like rt_lens_params: the library reads at most struct_bytes; < 8 = RT_ERR_INVALID_ARG */
    uint32_t struct_bytes;       /* sizeof(rt_nee_params) as the caller compiled it */
    int32_t  mis;                /* 1 (default): power heuristic; 0: light sampling alone (the BSDF hit of a table sphere counts 0) */
    int32_t  sample_planes;      /* 0 (default): spheres only; 1: emissive QUAD / ELLIPSE / TRIANGLE planes are sampled too (struct_bytes >= 12) */
    int32_t  select;             /* 0 (default): the entry by the power table's cdf; 1: by the light tree (struct_bytes >= 16) */
    int32_t  glossy;             /* 0 (default): light samples at diffuse events only; 1: at METAL's reflect branch too (struct_bytes >= 20) */
} rt_nee_params;
/* Defaults into *p, struct_bytes = sizeof(rt_nee_params). */
void rt_nee_params_init(rt_nee_params *p);
/* rt_render_samples with next-event estimation (params NULL: defaults). */
rt_status rt_render_nee(rt_scene *scene, const rt_camera_data *cam, const rt_nee_params *params, const rt_shard *shard, int32_t sample_first,
                        float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: the sphere-only emitter table (built if the handle has none yet).  *count = its length; the first
 * min(cap, count) entries go to sphere_index, cdf and pmf (each may be NULL when cap is 0). */
rt_status rt_nee_light_table(rt_scene *scene, int32_t cap, int32_t *sphere_index, float *cdf, float *pmf, int32_t *count);
/* Probe for tests, HOST memory: the emitter table that params select (NULL: the defaults), built if the handle has none yet.  kind: 0 a
 * sphere, 1 a plane; index: the sphere or plane index; area: A of a plane, 0 for a sphere.  count and cap as above; the parameter checks
 * are rt_render_nee's and come first. */
rt_status rt_nee_emitter_table(rt_scene *scene, const rt_nee_params *params, int32_t cap, int32_t *kind, int32_t *index, float *cdf, float *pmf,
                               float *area, int32_t *count);
/* Probe for tests, HOST memory: the light tree over the table that params select (NULL: the defaults; select itself is checked, not read),
 * built if the handle has none yet.  Per node, in preorder: sphere (centre and radius, 4 floats), weight, q (0 at a leaf), left and right
 * (node indices, -1 at a leaf) and entry (-1 at an interior node); per table entry: path and depth.  *node_count = 2 N - 1 (0 for an empty
 * table), *entry_count = N; the first min(cap, count) rows go to each column (each may be NULL when its cap is 0).  The parameter checks
 * are rt_render_nee's and come first. */
rt_status rt_nee_light_tree(rt_scene *scene, const rt_nee_params *params, int32_t cap_nodes, int32_t cap_entries, float *sphere, float *weight,
                            float *q, int32_t *left, int32_t *right, int32_t *entry, uint32_t *path, int32_t *depth, int32_t *node_count,
                            int32_t *entry_count);
/* Probe for tests, HOST memory: rt_trace_samples for the estimator of rt_render_nee — radiance, rays (closest-hit queries, shadow rays
 * included), the path's final RNG state and the light samples' final state per (i, j, s). */
rt_status rt_trace_samples_nee(rt_scene *scene, const rt_camera_data *cam, const rt_nee_params *params, int32_t n, const int32_t *ijs,
                               float *radiance, int32_t *rays, uint32_t *final_seed, uint32_t *final_nee_seed);

/* ---- image-based lighting: an environment map with importance sampling -----------------------------------------
 * rt_render_samples whose miss is a lookup in an environment map instead of cam->background, with one light sample of the map at
 * every diffuse event, combined with the path's own (BSDF) sample by multiple importance sampling.  float32 throughout, in the
 * order written, nothing fused, division and sqrtf correctly rounded; dot(a, b) = (a0*b0 + a1*b1) + a2*b2; random_float(s) as above;
 * sg(x) = x >= 0 ? 1 : -1 (so sg(-0) = 1).
 *   The map: n x n texels, OCTAHEDRAL, pole axis +y (get_sphere_uv's).  Texel (ix, iy) — rgb[(iy * n + ix) * 3 …] — covers
 *     u in [-1 + 2 ix / n, -1 + 2 (ix + 1) / n), v likewise from iy.  decode(u, v): y = (1 - |u|) - |v|; y >= 0: (x, z) = (u, v); else
 *     x = (1 - |v|) * sg(u), z = (1 - |u|) * sg(v); the octahedron point p = (x, y, z), the direction p normalised.
 *     texel(d): s = (|d0| + |d1|) + |d2|; p = (d0 / s, d1 / s, d2 / s); p1 >= 0: (u, v) = (p0, p2); else u = (1 - |p2|) * sg(p0),
 *     v = (1 - |p0|) * sg(p2); t = ((u + 1) * 0.5f) * (float)n; ix = t >= 0 ? (t < (float)n ? (int)t : n - 1) : 0 (NaN: 0); iy from v.
 *     Lookup is the nearest texel: E(d) = rgb of texel(d).  No trigonometry on the device.
 *   The sampling table (built by rt_env_create on the host, kept on the device): texel centre uc = -1 + (2 ix + 1) / n, vc likewise,
 *     pc = decode(uc, vc), l2 = (pc0*pc0 + pc1*pc1) + pc2*pc2, all in double; weight w = ((r + g) + b) * (((2 / n) * (2 / n)) /
 *     (l2 * sqrt(l2))) in double — radiance times the texel's solid angle.  Row iy's weight is the sum of its texels' in ix order, the
 *     total the sum of the rows' in iy order.  Marginal: row_cdf_iy = (float)(prefix through iy / total), the last one 1;
 *     row_pmf_iy = row_cdf_iy - row_cdf_{iy-1} in float (cdf_{-1} = 0).  Conditional of row iy, the same rule over its texels with the
 *     row's weight as total; a row of weight 0 has all zeros.  total == 0 (an all-black map): the table is EMPTY.
 *     pj(ix, iy) = row_pmf_iy * col_pmf_iy,ix (float).
 *   Density with respect to solid angle of a direction whose octahedron point is p (|p0| + |p1| + |p2| = 1) in texel (ix, iy):
 *     q2 = dot(p, p); q = sqrtf(q2); pl = (pj(ix, iy) * (((float)n * (float)n) * 0.25f)) * (q2 * q); 0 where the table is empty.
 *   Parameters (rt_env_params): mode, scale, rot (rows R0, R1, R2 of the world → environment rotation: de = (dot(R0, d), dot(R1, d),
 *     dot(R2, d))), camera_visible.  sE(d) = (scale * E0, scale * E1, scale * E2) of texel(de).
 *   The path draws exactly what rt_render_samples draws, from the same seed.  A closest-hit query k (the camera ray is query 0) with
 *     direction d that hits nothing adds term = beta_k * sE(d); when the ray left a diffuse event (below), mode != 0 and the table is
 *     not empty, term * w_b instead (w_b * term_c per component): p = de / s as texel(de) computes it, pl as above,
 *     w_b = mode == 1 ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0 ? 0 : 1), pb = RT_NEE_PB.  camera_visible == 0: a query 0 miss adds
 *     beta_0 * cam->background instead.  Emission of spheres and planes keeps weight 1.
 *   Diffuse event: rt_render_nee's definition (LAMBERTIAN, or METAL's hemisphere branch), at the hit point x of query k with
 *     face-forwarded normal n, albedo a and throughput beta_k before the attenuation.  When k + 1 < max_depth, mode != 0 and the
 *     table is not empty, one light sample from its own state env = wang_hash(wang_hash(base + s) ^ RT_ENV_STREAM_KEY),
 *     base = wang_hash(i * W + j); its draws stop at the first step that gives no contribution:
 *     1. ua = random_float(env); iy = the smallest row with ua < row_cdf_iy; none: no contribution.
 *     2. ub = random_float(env); ix = the smallest texel of row iy with ub < col_cdf_iy,ix; none: no contribution.
 *     3. uc = random_float(env), ud = random_float(env); h = 2.0f / (float)n; u = ((float)ix + uc) * h - 1; v = ((float)iy + ud) * h - 1;
 *        p = decode(u, v); q2 = dot(p, p); q = sqrtf(q2); we = (p0 / q, p1 / q, p2 / q);
 *        wl_c = (R0_c * we0 + R1_c * we1) + R2_c * we2 (the transpose: environment → world).
 *     4. !(dot(wl, n) > 0): none.  Otherwise the shadow ray (x, wl) over (0.001, 1e30), an occlusion query: it contributes only if it
 *        hits NOTHING.  pl = (pj(ix, iy) * (((float)n * (float)n) * 0.25f)) * (q2 * q);
 *        f = mode == 1 ? (pb * pl) / (pl * pl + pb * pb) : pb / pl;  contribution_c = ((beta_k,c * a_c) * (scale * E_c(ix, iy))) * f.
 *   Order: at each vertex the emission / miss term first, then the vertex's light sample; sums over samples in sample order.
 *   Identities, bit for bit: mode 0 with every texel equal to c and scale 1, any rot = rt_render_samples with background c; an all-black
 *     map, any mode = rt_render_samples with background 0.
 * Checks and limits: rt_render_nee's (rows of a shard only: no tiles, no rt_context; every refusal before anything is enqueued; the
 * handle's walk decisions, view lists and rt_last_timing left alone).  RT_ERR_INVALID_ARG: params with struct_bytes below 8, mode
 * outside {0, 1, 2}, scale negative or not finite, camera_visible outside {0, 1}, rot with |dot(Ra, Rb) - (a == b)| above 1e-4 for
 * some pair of rows, glossy outside {0, 1}, a null env, an env created on another device than the scene's.
 *   glossy = 1 (the first of the former reserved slots; rt_env_params_init leaves it 0): rt_render_nee's glossy events with this light —
 *     the event needs mode != 0 and a table that is not empty; its sample is steps 1 to 4 from the env state with pb = pg(wl; r, fuzz)
 *     and pb == 0 as one more "none"; the ray that leaves it carries pc = pg(unit(new_d); r, fuzz), and its miss is weighted by w_b with
 *     pc for pb (pc == 0: weight 1).  glossy = 0, a scene without METAL of fuzz >= RT_GLOSSY_MIN_FUZZ, mode 0 or an empty table: the
 *     call as written above, bit for bit. */
#define RT_ENV_STREAM_KEY 0x454E5631u
#define RT_ENV_MAX_N 4096
typedef struct rt_env rt_env;
/* rgb: HOST memory, n x n x 3 floats (copied).  RT_ERR_INVALID_ARG: null pointers, n < 1, n > RT_ENV_MAX_N, a texel that is negative,
 * NaN or infinite.  The object lives on the calling thread's current device; it is read-only afterwards and may be shared by any
 * number of scenes of that device and destroyed before or after them (not while a render that uses it is in flight). */
rt_status rt_env_create(const float *rgb, int32_t n, rt_env **out_env);
rt_status rt_env_destroy(rt_env *env);
typedef struct rt_env_params {   /* IN, grows like rt_nee_params: the library reads at most struct_bytes; < 8 = RT_ERR_INVALID_ARG */
    uint32_t struct_bytes;       /* sizeof(rt_env_params) as the caller compiled it */
    int32_t  mode;               /* 0: the path alone; 1 (default): MIS by the power heuristic; 2: light sampling alone */
    float    scale;              /* 1 (default): multiplies the map's radiance; finite, >= 0 */
    float    rot[9];             /* identity (default): rows of the world → environment rotation */
    int32_t  camera_visible;     /* 1 (default); 0: camera rays that miss add cam->background instead (compositing) */
    int32_t  glossy;             /* 0 (default); 1: light samples at METAL's reflect branch too (rt_render_nee, "glossy = 1"); modes 1 and 2 */
    int32_t  reserved[2];        /* 0: room to grow */
} rt_env_params;
/* Defaults into *p, struct_bytes = sizeof(rt_env_params). */
void rt_env_params_init(rt_env_params *p);
/* rt_render_samples lit by the environment (params NULL: defaults). */
rt_status rt_render_env(rt_scene *scene, const rt_camera_data *cam, const rt_env *env, const rt_env_params *params, const rt_shard *shard,
                        int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: the sampling table as the device holds it (read back).  *count = n, or 0 for an empty table; row_cdf and
 * row_pmf get n floats; col_cdf and col_pmf the n floats of row `row`'s conditional (0 <= row < n).  Any output may be NULL. */
rt_status rt_env_table(const rt_env *env, int32_t row, float *row_cdf, float *row_pmf, float *col_cdf, float *col_pmf, int32_t *count);
/* Probe for tests, HOST memory: n directions (3 n floats) through the DEVICE's lookup (no rotation): texel = iy * n + ix, radiance
 * (3 n floats, unscaled) and pl per direction. */
rt_status rt_env_lookup(const rt_env *env, int32_t n, const float *directions, int32_t *texel, float *radiance, float *pl);
/* Probe for tests, HOST memory: rt_trace_samples for the estimator of rt_render_env — radiance, rays (closest-hit queries plus shadow
 * rays, one each), the path's final RNG state and the light samples' final state per (i, j, s). */
rt_status rt_trace_samples_env(rt_scene *scene, const rt_camera_data *cam, const rt_env *env, const rt_env_params *params, int32_t n,
                               const int32_t *ijs, float *radiance, int32_t *rays, uint32_t *final_seed, uint32_t *final_env_seed);
/* Host helper (no device, host libm; not part of the bit-exact contract): a lat-long image (w x h x 3 floats, row 0 at the +y pole,
 * column by get_sphere_uv's u: phi = atan2(-z, x) + pi, u = phi / 2 pi; v = acos(y) / pi from the top) resampled into out (n x n x 3):
 * each texel the mean of the nearest lat-long pixels at a 4 x 4 grid of points inside it. */
rt_status rt_env_from_equirect(const float *rgb, int32_t w, int32_t h, int32_t n, float *out);

/* ---- emitters, environment and lens in one frame -----------------------------------------------------------------
 * rt_render_lens's camera in front of a path that takes rt_render_nee's light sample of the emitter table AND rt_render_env's light
 * sample of an environment at every diffuse event.  No new arithmetic: every expression is one of the three sections above, float32
 * in the order written there, nothing fused, division and sqrtf correctly rounded; this section fixes composition and order only.
 *   Camera: steps 1 … 5 of rt_render_lens — ox, oy, then tau when cam_close != NULL, then (lx, ly) when lens_radius > 0.  The path goes
 *     on from the RNG state those draws leave.
 *   Streams: nee = wang_hash(wang_hash(base + s) ^ RT_NEE_STREAM_KEY), env = wang_hash(wang_hash(base + s) ^ RT_ENV_STREAM_KEY),
 *     base = wang_hash(i * W + j), as in the single calls: the camera's extra draws do not move them.  A light that is off (the
 *     emitters: sample_emitters == 0 or an empty table; the environment: env == NULL, mode 0 or an empty table) never advances its
 *     state; rt_trace_samples_lit reports it as initialised.
 *   At the vertex of closest-hit query k, in this order:
 *     1. the emission or miss term.  A hit on a sphere (nee->sample_planes = 1: an entry) of the emitter table by a ray that left a diffuse event adds
 *        (beta_k * emit_k) * w_b with rt_render_nee's w_b when sample_emitters != 0 (nothing to weight where the table is empty);
 *     2. a miss adds rt_render_env's miss term when env != NULL — with its w_b after a diffuse event when mode != 0 and the map's
 *        table is not empty, and with its camera_visible rule for query 0 — and beta_k * cam->background otherwise;
 *     3. every other emission keeps weight 1;
 *     4. at a diffuse event with k + 1 < max_depth: the emitter sample, rt_render_nee's steps 1 … 4 from the nee state; its shadow
 *        ray's closest hit must be sphere e (nee->sample_planes = 1: steps 2p … 4p for a plane entry, and the hit must be entry e); its contribution is added to the sample's radiance as soon as it is known to count;
 *     5. at the same event: the environment sample, rt_render_env's steps 1 … 4 from the env state; its shadow ray is an occlusion
 *        query from the same point x; its contribution is added after the emitter's.
 *   Glossy events (nee->glossy, env_params->glossy): a METAL reflect vertex with fuzz >= RT_GLOSSY_MIN_FUZZ and
 *     k + 1 < max_depth is a glossy event when at least one light is on with its switch at 1.  It takes the emitter sample, then the
 *     environment sample, each if its own light is on and its own switch is 1 — the order of a diffuse vertex — and the ray that leaves
 *     it is weighted (by pc) only against the lights whose switch is 1; against the other it keeps weight 1.
 *   Spheres are hits and the map is misses: the two estimators never weight the same radiance, each keeps its own two-strategy MIS
 *   against the BSDF ray, and the sum has rt_render's expectation under that map.
 *   Identities, bit for bit: env == NULL, no lens, no motion, sample_emitters = 1 = rt_render_nee with the same nee parameters;
 *     sample_emitters = 0 (or an empty emitter table) with env != NULL, no lens, no motion = rt_render_env; sample_emitters = 0 and
 *     env == NULL = rt_render_lens, and so rt_render_samples without lens and motion.
 * Checks and limits: the union of rt_render_lens's, rt_render_nee's and rt_render_env's, in that order, every refusal before anything
 * is enqueued (nee is read only when sample_emitters != 0, env_params only when env != NULL); lit == NULL means the defaults;
 * RT_ERR_INVALID_ARG for a struct_bytes below 8 and for sample_emitters outside {0, 1}.  Rows of a shard only: no tiles, no rt_context.
 * Handle state: as rt_render_nee — the handle's walk choice, a pause of the guarded walk, the re-pack, the view lists and rt_last_timing
 * are left alone; the emitter tables (the sphere-only one and sample_planes = 1's) are the handle's two tables, built together by whichever
 * of rt_render_nee / rt_render_lit comes first.  The
 * light samples run on the reference-order walk only (timing->guarded is 0); timing (may be NULL) is this call's record. */
typedef struct rt_lit_params {          /* IN, grows like rt_env_params: the library reads at most struct_bytes; < 8 = RT_ERR_INVALID_ARG */
    uint32_t struct_bytes;              /* sizeof(rt_lit_params) as the caller compiled it */
    int32_t  sample_emitters;           /* 1 (default): light samples of the handle's emitter table; 0: none */
    const rt_camera_data *cam_close;    /* NULL (default): no motion */
    const rt_lens_params *lens;         /* NULL: rt_lens_params_init's defaults (pinhole) */
    const rt_nee_params  *nee;          /* NULL: defaults; read only when sample_emitters != 0 */
    const rt_env         *env;          /* NULL: no environment — a miss adds cam->background */
    const rt_env_params  *env_params;   /* NULL: defaults; read only when env != NULL */
} rt_lit_params;
/* Defaults into *p, struct_bytes = sizeof(rt_lit_params). */
void rt_lit_params_init(rt_lit_params *p);
/* rt_render_samples from the lens camera with both light samples (lit NULL: defaults — emitter sampling, pinhole, no environment). */
rt_status rt_render_lit(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_shard *shard,
                        int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: rt_trace_samples for the estimator of rt_render_lit — radiance, rays (closest-hit queries plus every
 * shadow ray of either kind), the path's final RNG state and both light streams' final states per (i, j, s). */
rt_status rt_trace_samples_lit(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, int32_t n, const int32_t *ijs,
                               float *radiance, int32_t *rays, uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed);

/* ---- direct and indirect light in separate frames --------------------------------------------------------------------
 * rt_render_lit's sample, its radiance written as two components.  The split draws nothing and changes no branch: rays, the path and the
 * nee and env streams are rt_render_lit's under the same lit.
 *   A sample of rt_render_lit is a sum of non-negative contributions, added in a fixed order: a vertex's emission or the miss term, then
 *   the verdicts of the light samples taken at that vertex (the emitter's, then the environment's).
 *   A diffuse event is a vertex that scatters diffusely: LAMBERTIAN, and METAL's 20 % branch.  METAL's reflect branch (any fuzz, glossy
 *   event or not) and DIELECTRIC are not diffuse events.
 *   A path has a stage.  0: no diffuse event yet; 1: the last vertex was the path's first diffuse event; 2: crossed.  The vertex that the
 *   ray leaving the first diffuse event finds adds its emission or miss term, MIS weight included, while still in stage 1; immediately
 *   after that add the path crosses.
 *   Every contribution added before the crossing is DIRECT: lamps and sky seen directly, in mirrors or through glass; the light samples of
 *   glossy events before the first diffuse event; both light samples of the first diffuse event; what its BSDF ray finds.  Every
 *   contribution added after the crossing is INDIRECT.  A path that ends before it crosses is all direct.  Both halves of every MIS pair
 *   land in the same component, and the definition depends on no switch (mis, sample_planes, select, glossy, the environment's mode).
 *   Each component is summed in float32 in rt_render_lit's order, from zero: direct is the sample's radiance when the path crosses (or
 *   ends), indirect what is added from zero after the crossing.  So with max_depth <= 2 direct is rt_render_lit's sample bit for bit and
 *   indirect is 0; in general direct + indirect differs from it only by the order of summing at most 3 * max_depth + 1 non-negative
 *   floats.
 * rt_render_lit_split: d_direct_sum and d_indirect_sum (DEVICE, 3 floats per local pixel each, like d_fb_sum) receive each component's
 * sum over samples sample_first … sample_first + spp - 1, added strictly in sample order.  Checks: rt_render_lit's, in its order; then
 * RT_ERR_INVALID_ARG for either output NULL or the two overlapping.  Rows of a shard only.  Handle state and timing: as rt_render_lit.
 * rt_config.pass_spp and workspace_bytes are honoured; the pass's slab holds both components, so a given budget admits half the samples
 * per pass.  No samples or no depth: both frames zero.
 * rt_trace_samples_lit_split: rt_trace_samples_lit's probe (HOST memory) with the radiance in two columns, direct and indirect. */
rt_status rt_render_lit_split(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_shard *shard,
                              int32_t sample_first, float *d_direct_sum, float *d_indirect_sum, void *hip_stream, int32_t sync, rt_timing *timing);
rt_status rt_trace_samples_lit_split(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, int32_t n, const int32_t *ijs,
                                     float *direct, float *indirect, int32_t *rays, uint32_t *final_seed, uint32_t *final_nee_seed,
                                     uint32_t *final_env_seed);

/* ---- adaptive sampling on the lit path ----------------------------------------------------------------------------
 * rt_render_adaptive's rounds on rt_render_lit's estimator.  No new arithmetic: the sample is the section above's, the statistics and
 * the rule are the adaptive section's, float32 in the order written there, nothing fused; this section fixes the composition only.
 *
 * Per-pixel parity.  Pixel p receives n_p samples, namely samples sample_first … sample_first + n_p - 1 of rt_render_lit's estimator
 * under the same lit — the lens and shutter, the emitter table with mis, sample_planes and select, the environment with its mode — and
 * d_fb_sum[p] equals, bit for bit, pixel p of rt_render_lit with samples_per_pixel = n_p and the same sample_first: the sum added in
 * sample order, starting from 0.  d_spp[p] = n_p, and n_p is min_spp + k * batch_spp for some k >= 0 with n_p <= max_spp.
 * cam_open->samples_per_pixel is ignored (cam_close, when given, still has to agree with cam_open in it).
 *
 * Statistics and rule: rt_render_adaptive's, from rt_adaptive_params.  y = (0.2126f*r + 0.7152f*g) + 0.0722f*b of the radiance
 * (r, g, b) rt_render_lit adds for the sample — its light-sample contributions and MIS weights included; S1 += y, S2 += y*y, float32,
 * from 0, in sample order; goes_on(S1, S2, n) as written there, judged after the min_spp samples and after every round but the last of
 * R = (max_spp - min_spp) / batch_spp.  d_moments (may be NULL) receives (S1, S2) per pixel.
 *
 * Identities, bit for bit: threshold = 0 gives rt_render_lit at min_spp + R * batch_spp samples, every count equal to that;
 * sample_emitters = 0, env == NULL, no lens, no motion and sample_first = 0 give rt_render_adaptive's d_fb_sum, d_spp and d_moments.
 *
 * Checks, all before anything is enqueued, in this order: (1) rt_render_adaptive's parameter checks with its codes (params NULL is
 * refused; lit NULL means the defaults); (2) rt_render_lit's — lens, then nee when sample_emitters != 0, then env_params when
 * env != NULL; (3) RT_ERR_INVALID_ARG for sample_first < 0 and RT_ERR_UNSUPPORTED for sample_first + min_spp + R * batch_spp above
 * 2^30; (4) RT_ERR_INVALID_ARG for d_fb_sum or d_spp NULL; (5) the scene's and the camera's, as rt_render_lit; (6) RT_ERR_UNSUPPORTED
 * for pixels x batch_spp at or above 2^31 - 4096 when R > 0.  Rows of a shard only: no tiles, no rt_context.
 *
 * Work.  All R rounds are enqueued up front; which pixels go on, and how many, lives on the device only, and a round whose list is
 * empty costs a few empty launches.  With sync == 0 the call only enqueues (it may wait for the stream once, when it grows the
 * handle's buffers).  max_depth <= 0: zero sums and moments, the counts by the rule (min_spp, or min_spp + R * batch_spp when
 * threshold = 0).
 * Handle state: as rt_render_lit — the walk choice, a pause of the guarded walk, the view lists and rt_last_timing are left alone; the
 * emitter tables and light trees are the handle's, built by whichever call comes first.  The moments, lists, work indices and counters
 * are rt_render_adaptive's handle buffers: a handle renders one frame at a time.
 * timing (may be NULL) is this call's record: kernel_ms from the first to the last kernel of the call (sync != 0), trace_launches =
 * the min_spp frame's passes + R, num_workgroups = the grid of the rounds' trace launches when R > 0 and the min_spp frame's first
 * pass's otherwise, traced_samples = pixels x min_spp (the rest is the sum of d_spp, which the caller has), guarded = 0.
 * d_fb_sum: 3 floats per pixel, d_spp: 1 int32 per pixel, d_moments: NULL or 2 floats per pixel — DEVICE memory, compacted like
 * rt_render's buffer.  rt_tonemap_spp turns the frame into bytes. */
rt_status rt_render_lit_adaptive(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_adaptive_params *params,
                                 const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp, float *d_moments,
                                 void *hip_stream, int32_t sync, rt_timing *timing);

/* rt_render_lit_adaptive with a choice of stopping rule (the stopping-rule section above): stop == NULL or rule == 0 is
 * rt_render_lit_adaptive bit for bit; rule == 1 judges by the neighbourhood rule, everything else — estimator, statistics, rounds,
 * parity, handle state, timing — unchanged.  The stop checks come right after check (1), before (2); their message names
 * rt_render_lit_adaptive_rule. */
rt_status rt_render_lit_adaptive_rule(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_adaptive_params *params,
                                      const rt_stop_params *stop, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp,
                                      float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing);
/* rt_render_lit_adaptive_rule with a prior ("a history-aware stopping rule" above): its arguments, then d_prior. */
rt_status rt_render_lit_adaptive_prior(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit,
                                       const rt_adaptive_params *params, const rt_stop_params *stop, const rt_shard *shard,
                                       int32_t sample_first, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream,
                                       int32_t sync, rt_timing *timing, const float *d_prior);

/* ---- participating medium ---------------------------------------------------------------------------------------
 * rt_render_lit's estimator — lens, shutter, the emitter table with mis / sample_planes / select / glossy, the environment with its mode
 * and glossy — with ONE homogeneous grey medium in a region of space: all space, a ball or an axis-aligned box.  Between two vertices a
 * path ray may scatter in the medium instead of reaching its surface; every light sample is attenuated by the medium it crosses.
 * float32 in the order written, nothing fused, division and sqrtf correctly rounded; log_libm and exp_libm are csrc/rt_device_math.h's
 * stated algorithms (float in, a double table and polynomial, one rounding to float).  FOUR_PI = 2.0f * RT_NEE_TWO_PI.
 *
 * Stream.  med = wang_hash(wang_hash(base + s) ^ RT_MEDIUM_STREAM_KEY), base = wang_hash(i * W + j), with random_float.  The path, nee
 *   and env streams draw exactly what they draw in rt_render_lit for the same sequence of vertices; the medium never touches them, except
 *   that a medium vertex stands where a surface vertex would have stood.  Without an event med is never advanced.
 *
 * Region on a ray.  interval(o, d, t_end) of the ray o + t d over [0, t_end] (t_end may be +inf) is [t0, t1], or empty:
 *   region 0 (all space): t0 = 0, t1 = t_end.
 *   region 1 (ball, centre a, radius R = b[0]): oc = o - a; A = lensq(d); hb = dot(oc, d); cc = lensq(oc) - R * R; disc = hb * hb - A * cc;
 *     empty unless disc > 0; sq = sqrtf(disc); ta = (-hb - sq) / A; tb = (-hb + sq) / A; t0 = ta > 0 ? ta : 0; t1 = tb < t_end ? tb : t_end.
 *   region 2 (box, lo = a, hi = b): t0 = 0, t1 = t_end; then for the axes x, y, z in turn: when d_k == 0 the interval is empty unless
 *     lo_k < o_k and o_k < hi_k (no division); otherwise ta = (lo_k - o_k) / d_k, tb = (hi_k - o_k) / d_k, swapped when ta > tb, then
 *     t0 = ta when ta > t0 and t1 = tb when tb < t1.
 *   In every region the interval is empty unless t1 > t0.  The region ignores surfaces.
 *
 * Segment.  For every PATH ray (o, d) whose closest-hit query k has finished — a hit at parameter t_hit, or a miss: t_hit = +inf — with
 *   sigma_t > 0: len = sqrtf(lensq(d)) (directions are not unit), [t0, t1] = interval(o, d, t_hit).  An empty interval: no draw, and the
 *   vertex is rt_render_lit's.
 * Free flight.  u = random_float(med).  u == 0: no event.  Otherwise s = -log_libm(u) / sigma_t, and there is an event iff
 *   s < (t1 - t0) * len, at x = o + (t0 + s / len) * d (componentwise o_k + t * d_k).  No event: the surface vertex (or the miss) of
 *   rt_render_lit with UNCHANGED throughput — sampling the distance of a grey medium has weight 1, so the path never calls exp.
 * Medium vertex (counts as vertex k for max_depth; medium_events counts them).  ud = unit(d).  beta_in = beta; beta = beta * albedo.  If
 *   all three channels of the new beta are 0 the path ends here, before any draw.  If k + 1 >= max_depth the path ends here as well.
 *   Otherwise, in this order:
 *   1. the emitter sample when the emitters are on, then the environment sample when the environment is sampled: rt_render_lit's steps
 *      4 and 5 from x with beta_in, a = albedo, no hemisphere test (there is no normal), and pb = ph(dot(ud, wl) / sqrtf(lensq(wl))) for
 *      the sampled direction wl; pb == 0: no contribution;
 *   2. the next direction: cos_t from one med draw u1 — g == 0: cos_t = 1 - 2 * u1; otherwise q = (1 - g * g) / ((1 - g) + (2 * g) * u1),
 *      cos_t = ((1 + g * g) - q * q) / (2 * g), clamped to [-1, 1] — sin_t = sqrtf(max(0, 1 - cos_t * cos_t)); the azimuth (cx, cy) from
 *      med by rt_render_nee's disc loop (px, py = random_float(med, -1, 1) until 0 < px^2 + py^2 < 1, divided by the root); Duff's basis
 *      (t1, t2) of rt_render_nee's step 3 around ud; new_d = (t1 * (sin_t * cx) + t2 * (sin_t * cy)) + ud * cos_t.  The next ray is
 *      (x, new_d) with throughput beta (weight 1: the phase function is sampled exactly), and it carries pb = ph(cos_t) the way a glossy
 *      event's ray carries pg: the emitter entry or the miss it finds is weighted with that pb against every light that is on; a ph that
 *      rounds to 0 is "none".
 *   ph(c): g == 0: 1 / FOUR_PI; otherwise den = (1 + g * g) - (2 * g) * c, ph = (1 - g * g) / (FOUR_PI * (den * sqrtf(den))).
 * Transmittance.  Every light-sample contribution c, from a surface vertex or a medium one, is added as Tr * c, Tr = exp_libm(-(sigma_t *
 *   L)), L = (t1 - t0) * len of interval(x, wl, t_end) of its shadow ray: t_end is the parameter of the hit the emitter's shadow ray
 *   reached (known at the verdict), +inf for the environment's.  An empty interval: Tr = 1 exactly, exp is not called.  With region 0 and
 *   sigma_t > 0 the environment's Tr is 0: the environment counts as not sampled for the whole call (no light sample is drawn, its stream
 *   never advances, and a miss keeps weight 1).
 *   The MIS weights stay those of the directional densities alone: both strategies estimate the same integrand f * Tr * Le — the light
 *   sample carries Tr as a factor, the path ray carries it as its probability of surviving to the light — so Tr cancels from the ratio of
 *   the two strategies' densities, and w_l + w_b = 1 per direction as before.
 *
 * Identities, bit for bit: medium == NULL or sigma_t == 0 = rt_render_lit with the same lit (and every probe column: medium_events 0, the
 *   med state as initialised).  sigma_t > 0 with a region that no path ray and no shadow ray of the frame touches = rt_render_lit as well,
 *   through the medium's own kernels.
 * Left out: ~~heterogeneous~~ (rt_render_volume, "density grid" below) or ~~chromatic extinction~~ (rt_render_chroma, "chromatic extinction" below); more than one region; regions bounded by scene surfaces (fog inside a glass ball that
 *   sits in the region is still fog); ~~emission in the medium~~ (rt_render_glow, "emission in the medium" below); the guarded walk; tiles and rt_context; ~~rt_render_lit_adaptive with a
 *   medium~~ (rt_render_volume_adaptive, "adaptive sampling under fog" below), ~~AOVs of the medium and the denoisers' handling of it~~ (rt_render_aov_volume, "AOVs under fog" below; the first-hit AOVs do not see it).
 * Checks, all before anything is enqueued: rt_render_lit's parameter checks come first, in its order (lens, nee, env_params); then the
 *   medium's, still before the scene is looked at; then the scene's and the camera's as in rt_render_lit.  RT_ERR_INVALID_ARG for struct_bytes below 8,
 *   region outside {0, 1, 2}, a sigma_t that is negative, NaN or infinite, an albedo channel outside [0, 1], |g| > 0.95 or NaN, a ball's
 *   radius <= 0 (or NaN), a box with lo_k >= hi_k in any axis (region 1 and 2 also need finite a and b).  a and b are read only for the
 *   region that uses them.  Rows of a shard only: no tiles, no rt_context.  Handle state and timing: as rt_render_lit. */
#define RT_MEDIUM_STREAM_KEY 0x4D454431u   /* "MED1" */
typedef struct rt_medium_params {   /* IN, caller-sized like rt_lit_params */
    uint32_t struct_bytes;
    int32_t  region;        /* 0: all space, 1: ball (centre, radius), 2: axis-aligned box (lo, hi) */
    float    sigma_t;       /* extinction per unit length, grey, >= 0 and finite; 0 = no medium */
    float    albedo[3];     /* single-scattering albedo per channel, each in [0, 1] */
    float    g;             /* Henyey–Greenstein anisotropy, |g| <= 0.95; 0 = isotropic (its own branch, no division by g) */
    float    a[3], b[3];    /* ball: centre = a, radius = b[0] > 0; box: lo = a < hi = b componentwise */
} rt_medium_params;
/* Defaults into *p: region 0, sigma_t 0 (no medium), albedo 1, g 0, a = b = 0; struct_bytes = sizeof(rt_medium_params). */
void rt_medium_params_init(rt_medium_params *p);
/* rt_render_lit under the medium (medium NULL: the defaults — no medium). */
rt_status rt_render_medium(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                           const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: rt_trace_samples_lit for the estimator of rt_render_medium, with the number of medium vertices and the
 * medium stream's final state per (i, j, s) as well. */
rt_status rt_trace_samples_medium(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                  int32_t n, const int32_t *ijs, float *radiance, int32_t *rays, int32_t *medium_events,
                                  uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed, uint32_t *final_medium_seed);

/* ---- density grid ------------------------------------------------------------------------------------------------
 * rt_render_medium's estimator with a HETEROGENEOUS extinction in its box region: the density is piecewise constant on a regular grid of
 * nx * ny * nz cells that fills the box, and cell c has the extinction sigma_c = sigma_t * rho_c (one float32 product).  Albedo and g stay
 * the medium's.  Everything of "participating medium" holds as written there — the stream, the interval, the medium vertex, the light
 * samples, the MIS weights — except the two places where the extinction enters: the free flight of a path ray and the optical depth
 * of a shadow ray.  Both run ONE walk through the cells the ray's interval crosses (regular tracking: the free flight is exact by
 * inversion with a single draw of med, the optical depth is a deterministic sum).  float32 in the order written, nothing fused, division
 * correctly rounded.
 *
 * Walk of the ray o + t d over its interval [t0, t1] = interval(o, d, t_end) of the box (lo = a, hi = b), len = sqrtf(lensq(d)).  An empty
 *   interval: no walk, no draw, no cells.  Per axis k with n_k cells:
 *   w_k = (hi_k - lo_k) / (float)n_k;  plane_k(m) = lo_k for m == 0, hi_k for m == n_k (the box's own face, not lo + n * w), otherwise
 *     lo_k + (float)m * w_k.
 *   Entry: p_k = o_k + t0 * d_k; c_k = (int)floorf((p_k - lo_k) / w_k), clamped to [0, n_k - 1].
 *   tnext_k = (plane_k(c_k + 1) - o_k) / d_k for d_k > 0, (plane_k(c_k) - o_k) / d_k for d_k < 0, +inf for d_k == 0: recomputed from the
 *     plane at every cell, never accumulated.
 *   Per cell: ta = the previous cell's tb (t0 at the first cell).  tm = tnext_x, axis x; ty < tm: tm = ty, axis y; tz < tm: tm = tz, axis z
 *     (ties go to x before y before z).  tb = tm < t1 ? tm : t1, raised to ta when below it.  seg = (tb - ta) * len (never negative).  The
 *     cell (c_x, c_y, c_z) is visited with seg (below).  The walk stops when tb >= t1; otherwise c_axis moves by one in the direction of
 *     d_axis, and the walk stops when that leaves the grid.  One axis moves per step, so a walk visits at most n_x + n_y + n_z cells, and
 *     the walk is cut there.
 * Free flight (every finished PATH ray with a non-empty interval).  u = random_float(med); u == 0: no event and no walk.  rem =
 *   -log_libm(u).  A visited cell with sigma_c > 0: s = rem / sigma_c; s < seg: an event at t = ta + s / len, x = o + t * d (componentwise
 *   o_k + t * d_k), and the walk ends; otherwise rem = rem - sigma_c * seg.  A cell with sigma_c == 0 changes nothing.  No event in any
 *   cell: the surface vertex (or the miss) of rt_render_lit with unchanged throughput.  The medium vertex at x is rt_render_medium's.
 * Transmittance (the two shadow verdicts).  acc = 0; every visited cell: acc = acc + sigma_c * seg, in visit order; Tr = exp_libm(-acc).
 *   An empty interval: Tr = 1 exactly, exp is not called.
 *
 * Identities, bit for bit: a 1 x 1 x 1 grid of density 1 = rt_render_medium with the same box (through the grid's own kernels: tnext of
 *   the only cell is the box's own exit, so tb = t1 and seg = (t1 - t0) * len).  volume == NULL = rt_render_medium with the same
 *   arguments, whatever its region.  sigma_t == 0 = rt_render_lit.  A grid of zeros = rt_render_lit in radiance, rays and the path, nee
 *   and env streams; med advances one draw per non-empty path interval.
 * Left out: ~~chromatic extinction~~ (rt_render_chroma, "chromatic extinction" below); more than one region or grid; ~~emission in the medium~~ (rt_render_glow, "emission in the medium" below); interpolation between cells (trilinear or any
 *   other: the density is piecewise constant); ~~rt_render_lit_adaptive with a grid~~ (rt_render_volume_adaptive, "adaptive sampling under fog"
 *   below); ~~AOVs of the medium~~ (rt_render_aov_volume, "AOVs under fog" below); tiles and rt_context.
 * rt_volume: the grid on the device it was created on (the calling thread's current one), like an rt_env.  density is HOST memory, nx * ny
 *   * nz floats, copied: cell (x, y, z) at (z * ny + y) * nx + x.  RT_ERR_INVALID_ARG for a null pointer, a dimension below 1 or above
 *   RT_VOLUME_MAX_N, a density that is negative, NaN or infinite.  A volume outlives every call that was given it; destroy it after the
 *   last such call has finished.  A volume on another device than the scene is refused.
 * Checks of the calls, all before anything is enqueued: rt_render_medium's, in its order up to and including the medium's; then, with a
 *   volume, RT_ERR_INVALID_ARG unless medium is given with region == 2; then the null scene and the volume's device against the scene's; then the scene's and the camera's as in rt_render_lit.  Rows
 *   of a shard only: no tiles, no rt_context.  Handle state and timing: as rt_render_lit. */
#define RT_VOLUME_MAX_N 256
typedef struct rt_volume rt_volume;
rt_status rt_volume_create(const float *density, int32_t nx, int32_t ny, int32_t nz, rt_volume **out_volume);
rt_status rt_volume_destroy(rt_volume *volume);
/* rt_render_medium with the grid in the medium's box (volume NULL: rt_render_medium itself). */
rt_status rt_render_volume(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                           const rt_volume *volume, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream,
                           int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: rt_trace_samples_medium's columns for the estimator of rt_render_volume, and cells: the grid cells
 * visited per sample, path rays and shadow rays together (0 without a volume).  It only counts. */
rt_status rt_trace_samples_volume(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                  const rt_volume *volume, int32_t n, const int32_t *ijs, float *radiance, int32_t *rays,
                                  int32_t *medium_events, uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed,
                                  uint32_t *final_medium_seed, int32_t *cells);

/* ---- chromatic extinction ------------------------------------------------------------------------------------------
 * rt_render_volume's estimator — the medium in its region, with or without a density grid in its box — with an extinction that differs per
 * colour channel: channel k has sigma_k = sigma_t * tint[k], one float32 product made on the host.  Region, albedo, g, the box, the grid and
 * RT_MEDIUM_STREAM_KEY stay the medium's and the volume's.  Everything of "participating medium" and "density grid" holds as written there
 * except the two places where the extinction enters: the free flight of a path ray, which samples its distance by ONE channel's
 * extinction and carries a weight per channel from then on, and the transmittance of a shadow ray, which is per channel.  float32 in the
 * order written, nothing fused, division correctly rounded; log_libm and exp_libm as in "participating medium".
 *
 * Density length A of a non-empty interval [t0, t1] of a ray (o, d), len = sqrtf(lensq(d)).  Without a grid: A = (t1 - t0) * len.  With a
 *   grid: the walk of "density grid" with sigma_t taken as 1 (sigma_c = 1.0f * rho_c = rho_c): A = acc, acc = acc + rho_c * seg over the
 *   visited cells in visit order.  A free-flight walk keeps that sum as well, over the cells it passed without an event.
 * Transmittance of channel k over A: Tr_k = 1 exactly when sigma_k == 0 (no multiplication: A may be +inf); otherwise
 *   Tr_k = exp_libm(-(sigma_k * A)).
 * Free flight (every finished PATH ray with a non-empty interval).  u = random_float(med); u == 0: no event, unchanged throughput, nothing
 *   more is drawn.  Otherwise uc = random_float(med), j = min(2, (int)(uc * 3.0f)), and the target R = +inf when sigma_j == 0, otherwise
 *   R = -log_libm(u) / sigma_j.  Without a grid there is an event iff R < (t1 - t0) * len, at t = t0 + R / len.  With a grid the free-flight
 *   walk of "density grid" runs on rho_c with rem = R: a visited cell with rho_c > 0: s = rem / rho_c; s < seg: an event at t = ta + s / len;
 *   otherwise rem = rem - rho_c * seg.  x = o + t * d.  At an event A = R, the target itself; without one A is the whole interval's.
 * Weights: single-sample MIS over the three channels (the balance heuristic of the three distance densities, each chosen with
 *   probability 1/3), unbiased per channel.
 *   Event: e_k = sigma_k * Tr_k; den = (e_0 + e_1) + e_2; beta_k = beta_k * w_k, w_k = min(3.0f, (3.0f * e_k) / den); then the medium vertex of "participating
 *     medium" at x, unchanged (its beta_in is this weighted beta).
 *   No event: den = (Tr_0 + Tr_1) + Tr_2; beta_k = beta_k * w_k, w_k = min(3.0f, (3.0f * Tr_k) / den); then the surface vertex or the miss of rt_render_lit.
 *   Each weight lies in [0, 3]: each term of den is one of the numerators over 3, so the exact quotient cannot pass 3; the float32 one can,
 *   by one ulp (the product and the quotient each round), which the min takes back.  den > 0 in both cases: the channel that was
 *   sampled contributes Tr_j of about u (and sigma_j > 0) at an event; without one Tr_j > u, up to rounding, or Tr_j = 1 (sigma_j == 0).
 * Shadow rays.  Channel k of a light-sample contribution is multiplied by Tr_k over the A of its shadow ray's interval.  An empty interval
 *   leaves it unchanged, and exp is not called.
 * MIS.  The weights of the light samples stay those of the directional densities: the path's survival to a light is now an unbiased
 *   per-channel ESTIMATE of Tr_k instead of Tr_k itself, and the weights depend on the direction only.
 * Region 0: as in "participating medium" — with sigma_t > 0 the environment is not sampled, even when some sigma_k is 0: the path's misses
 *   carry the environment.
 *
 * Identities, bit for bit: tint[0] == tint[1] == tint[2] == e hands the call over whole to rt_render_volume (which hands on to
 *   rt_render_medium or rt_render_lit as it does) with the medium's sigma_t replaced by the float product sigma_t * e; this covers chroma
 *   == NULL, the default tint and e == 0, and the probe's cells column is then that call's.  So does a medium with sigma_t == 0 (or no
 *   medium) under any tint.  A 1 x 1 x 1 grid of density 1 = the homogeneous box under the same tint, through the grid's own chroma kernels
 *   (s = R / 1, acc = seg).  volume == NULL = the homogeneous chroma kernels, in any region.
 * Left out: ~~the adaptive call with a tint~~ (rt_render_fog_adaptive, "adaptive sampling on every fog rung" below); the AOV and denoise calls with a tint; choosing the channel by the path's throughput instead of uniformly; a tint per
 *   cell; ~~emission in the medium~~ (rt_render_glow, "emission in the medium" below); tiles and rt_context; the guarded walk.
 * Checks, all before anything is enqueued: rt_render_volume's, in its order up to and including the volume's region check; then
 *   RT_ERR_INVALID_ARG for struct_bytes below 8, a tint channel that is negative, NaN or infinite, a product sigma_t * tint[k] that is not
 *   finite — still before the scene is looked at; then the null scene, and rt_render_volume's remaining checks.  The messages name
 *   rt_render_chroma (rt_trace_samples_chroma).  Handle state and timing: as rt_render_lit. */
typedef struct rt_chroma_params {   /* IN, caller-sized like rt_medium_params */
    uint32_t struct_bytes;
    float    tint[3];       /* the factor on sigma_t per channel, each >= 0 and finite */
} rt_chroma_params;
/* Defaults into *p: tint = 1, 1, 1 (grey: rt_render_volume itself); struct_bytes = sizeof(rt_chroma_params). */
void rt_chroma_params_init(rt_chroma_params *p);
/* rt_render_volume under the tint (chroma NULL: the defaults; volume NULL: no grid). */
rt_status rt_render_chroma(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                           const rt_volume *volume, const rt_chroma_params *chroma, const rt_shard *shard, int32_t sample_first,
                           float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: rt_trace_samples_volume's columns for the estimator of rt_render_chroma. */
rt_status rt_trace_samples_chroma(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                  const rt_volume *volume, const rt_chroma_params *chroma, int32_t n, const int32_t *ijs, float *radiance,
                                  int32_t *rays, int32_t *medium_events, uint32_t *final_seed, uint32_t *final_nee_seed,
                                  uint32_t *final_env_seed, uint32_t *final_medium_seed, int32_t *cells);

/* ---- emission in the medium ----------------------------------------------------------------------------------------
 * rt_render_volume's estimator — the medium in its region, with or without a density grid in its box — with a medium that also EMITS: fire,
 * glowing gas.  The emission coefficient at a point is radiance_k * h, with h = 1 over the whole region (source 0), the density of the
 * point's cell (source 1) or the value of the point's cell in a second grid of the volume's dimensions, the heat (source 2).  Everything of
 * "participating medium" and "density grid" holds as written there, with one addition: after the free flight of every finished PATH ray
 * with a non-empty interval, and before anything that vertex itself adds to the sample's colour, the radiance the medium emitted towards the
 * ray's origin is added.  No draw, no exp and no shadow ray are added: the ray's own free flight is an unbiased track-length estimator — it
 * ends at a distance S with P(S > t) = Tr(t), and the integral of Tr(t) * eps(t) over the interval is the expectation of eps integrated
 * over the stretch the flight flew.  float32 in the order written, nothing fused, division correctly rounded; log_libm as in "participating
 * medium".
 *
 * Without a grid (source 0 only).  whole = (t1 - t0) * len.  The flight is the grey one: u = random_float(med); u == 0: D = whole and there
 *   is no event.  Otherwise s = -log_libm(u) / sigma_t; an event iff s < whole, at t = t0 + s / len; D = s at an event, whole without one.
 *   D finite: color_k = color_k + beta_k * (radiance_k * D), beta the throughput the ray arrived with (before the medium vertex's albedo).
 *   D = +inf (region 0, a miss, u == 0 — nothing else): nothing is added.
 * With a grid.  E = 0.  rem = +inf when u == 0 — the walk still runs, finds no event and counts its cells — otherwise rem = -log_libm(u).
 *   Every visited cell: h_c = 1.0f, rho_c or heat_c by source; seg as in "density grid".  sigma_c > 0: s = rem / sigma_c; s < seg:
 *   E = E + h_c * s, an event at t = ta + s / len, and the walk ends; otherwise rem = rem - sigma_c * seg.  Every cell that is passed
 *   without an event, sigma_c == 0 or not: E = E + h_c * seg.  Then color_k = color_k + beta_k * (radiance_k * E).
 * Then the medium vertex at the event, or the surface vertex or the miss, unchanged.  Shadow rays emit nothing and are attenuated as before.
 *   The glow is found by path rays only and never light-sampled: it has weight 1 and enters no MIS weight.  The environment rule of region
 *   0 is unchanged.
 * Probe: rt_trace_samples_volume's columns and glow_length, the float32 sum of D or E over the sample's path rays in order (0 after a
 *   handover); cells counts the walk under u == 0 as well.
 *
 * Identities, bit for bit: glow == NULL or radiance 0, 0, 0 hands the call over whole to rt_render_volume with the same arguments (heat is
 *   checked but not read).  A 1 x 1 x 1 grid of density 1 under source 0 or 1 = the homogeneous box under source 0, through the grid's own
 *   glow kernels (s = rem / sigma_t, E = 0 + 1 * s).  Source 2 with a heat grid equal to the density grid = source 1.
 * Left out: ~~light-sampling the glow (fire lights a room by the paths that happen to cross it)~~ (rt_render_glow_sampled, "light samples of the glow" below); a glow with sigma_t == 0 (the estimator rides
 *   on the free flight); a glow under a tint (rt_render_chroma); ~~the adaptive call with a glow~~ (rt_render_fog_adaptive, "adaptive sampling on every fog rung" below); the AOV and denoise calls with a glow; trilinear heat (h is
 *   piecewise constant like the density); blackbody colour from temperature; tiles and rt_context; the guarded walk.
 * Checks, all before anything is enqueued: rt_render_volume's, in its order up to and including the volume's region check; then
 *   RT_ERR_INVALID_ARG for struct_bytes below 8, source outside {0, 1, 2}, a radiance channel that is negative, NaN or infinite, a non-zero
 *   radiance without a medium or with sigma_t == 0 (a glow without extinction has no kernel), source 1 or 2 without a volume, source 2
 *   without heat or with a heat grid of other dimensions than the volume's, heat given under source 0 or 1 — still before the scene is
 *   looked at; then the null scene, heat's device (and the volume's) against the scene's, and rt_render_volume's remaining checks.  The
 *   messages name rt_render_glow (rt_trace_samples_glow).  Handle state and timing: as rt_render_lit. */
typedef struct rt_glow_params {   /* IN, caller-sized like rt_chroma_params */
    uint32_t struct_bytes;
    int32_t  source;        /* 0: uniform over the region (h = 1); 1: the density grid (h_c = rho_c); 2: a heat grid (h_c = heat_c) */
    float    radiance[3];   /* emitted radiance per unit length at h = 1, per channel, each >= 0 and finite; 0, 0, 0 = no glow */
} rt_glow_params;
/* Defaults into *p: source 0, radiance 0, 0, 0 (no glow: rt_render_volume itself); struct_bytes = sizeof(rt_glow_params). */
void rt_glow_params_init(rt_glow_params *p);
/* rt_render_volume with the glow (glow NULL: the defaults; volume NULL: no grid; heat: an rt_volume of the volume's dimensions, source 2 only). */
rt_status rt_render_glow(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                         const rt_volume *volume, const rt_glow_params *glow, const rt_volume *heat, const rt_shard *shard, int32_t sample_first,
                         float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: rt_trace_samples_volume's columns and glow_length for the estimator of rt_render_glow. */
rt_status rt_trace_samples_glow(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                const rt_volume *volume, const rt_glow_params *glow, const rt_volume *heat, int32_t n, const int32_t *ijs,
                                float *radiance, int32_t *rays, int32_t *medium_events, uint32_t *final_seed, uint32_t *final_nee_seed,
                                uint32_t *final_env_seed, uint32_t *final_medium_seed, int32_t *cells, float *glow_length);

/* ---- light samples of the glow --------------------------------------------------------------------------------------
 * rt_render_glow's estimator over a density grid, with the glowing medium as a third light that a vertex can aim at: beside the emitter's
 * and the environment's sample, a sampling vertex takes one of the glow, and the track-length add of the path ray that leaves the vertex
 * is weighted against it by the power heuristic (or by 0: light sampling alone).  Everything of "emission in the medium" holds as written
 * there.  float32 in the order written, nothing fused, division correctly rounded, exp_libm as in "participating medium".
 *
 * A point of the emitting volume has the kernel 1 / r^2 — infinite variance at a vertex inside or next to the glow — so the sample chooses
 * a DIRECTION, and the whole line along it is evaluated.  With wx, wy, wz the cell's widths as in "density grid":
 * glow_pl(o, d), the density in solid angle of the direction d at o: "density grid"'s walk, cell for cell, over interval(o, d, +inf); an
 *   empty interval gives 0.  len = sqrt(lensq(d)), q = 0; every visited cell c with its stretch [ta, tb]: seg = (tb - ta) * len,
 *   ra = ta * len, rb = tb * len, q = q + pc_c * (seg * ((rb * rb + rb * ra) + ra * ra)).  pl = q * inv3v, inv3v = 1.0f / (3.0f * ((wx * wy)
 *   * wz)) — the sum over the cells of pc_c (rb^3 - ra^3) / (3 V_cell).
 * glow_line(o, d, t_end), the emission along the ray per unit radiance: the walk over interval(o, d, t_end); Tr = 1, G = 0; every visited
 *   cell: x = sigma_c * seg, e = exp_libm(-x), m = x < 0.0625f ? seg * (1.0f - x * (0.5f - x * (1.0f / 6.0f - x * (1.0f / 24.0f)))) :
 *   (1.0f - e) / sigma_c (the series' error is below x^4 / 120; it covers sigma_c == 0), G = G + Tr * (h_c * m), Tr = Tr * e.  h_c by source.
 *
 * The light sample.  Where: every diffuse event, every medium vertex, and METAL's glossy events (fuzz >= RT_GLOSSY_MIN_FUZZ) when emitters
 *   are sampled with nee.glossy = 1 — whether or not the emitter table holds an entry; each only with depth + 1 < max_depth, as the other
 *   samples.  It is drawn from the med stream behind the emitter's and the environment's sample — at a medium vertex behind the draws of
 *   the next direction as well — six draws in this order: us, ur, uc, ux, uy, uz.  z = pick(slab_cdf, nz, us), y = pick(row_cdf + z * ny,
 *   ny, ur), x = pick(cell_cdf + (z * ny + y) * nx, nx, uc), pick the rule of rt_env's table (the smallest e with u < cdf[e]); a pick that
 *   finds nothing: no sample.  p = (a0 + ((float)x + ux) * wx, a1 + ((float)y + uy) * wy, a2 + ((float)z + uz) * wz), dir = p - vertex.
 *   No sample when lensq(dir) == 0; at a surface when !(dot(dir, n) > 0); when pb == 0 at a glossy event or a medium vertex, pb the BSDF
 *   strategy's density (RT_NEE_PB, pg or ph) at dir / sqrt(lensq(dir)), divided per component; when !(pl > 0), pl = glow_pl(vertex, dir).
 *   Otherwise f = mis ? (pb * pl) / (pl * pl + pb * pb) : pb / pl, and a shadow ray (vertex, dir) is traced as a full closest-hit query,
 *   after the emitter's and the environment's.  At its verdict, with a non-empty interval: G = glow_line(vertex, dir, closest hit or +inf),
 *   color_k = color_k + (beta_in_k * a_k) * (f * (radiance_k * G)), a the vertex's albedo.  The adds of a vertex: emitter, environment, glow.
 * The path side.  The add beta * radiance * E of a path ray that left such a vertex — with or without a sample there — is scaled by
 *   wb = mis ? (pb * pb) / (pb * pb + pl * pl) : (pl > 0 ? 0 : 1), pb the value the ray carries (RT_NEE_PB, pg, ph; a carried 0 is none),
 *   pl = glow_pl of the ray: color_k = color_k + wb * (beta_k * (radiance_k * E)).  Camera rays, rays out of DIELECTRIC, mirror METAL and
 *   glossy METAL without the switch have weight 1 and walk nothing more.  Nothing else of the ray is weighted.
 *
 * rt_glow_sampler: the table, built once from the grids on the device they live on.  h_c = 1, rho_c or heat_c by source.  In float64, in
 *   index order: a row's sum over its cells (x), a slab's over its rows' sums (y), the total over the slabs' sums (z).  cell_cdf[(z * ny +
 *   y) * nx + x] = (float)(running sum of the row / the row's sum), row_cdf[z * ny + y] likewise of the slab's rows, slab_cdf[z] of the
 *   slabs; the last entry of every cdf with a positive sum is 1.0f, a cdf with sum 0 is all zero.  pc_c = (slab_pmf * row_pmf) * cell_pmf,
 *   each pmf the float32 difference of adjacent cdf entries (the first entry itself), stored per cell.  All h == 0: the sampler is empty.
 *   A sampler belongs to its source, its volume and (source 2) its heat grid, and is destroyed before them.
 * Probe: rt_trace_samples_glow's columns and glow_samples, the number of glow shadow rays (they count in rays too); cells counts the
 *   cells of glow_pl's and glow_line's walks as well.
 *
 * Identities, bit for bit: params NULL, sample == 0, an empty sampler or radiance 0, 0, 0 hands the call over whole to rt_render_glow
 *   (rt_trace_samples_glow; glow_samples 0).  max_depth = 1 under mis 0 or 1 = rt_render_glow's radiance, through these kernels.
 * Left out: a tint; ~~the adaptive call~~ (rt_render_fog_adaptive, "adaptive sampling on every fog rung" below); the AOV and denoise calls; a glow without a grid (a homogeneous box can pass a 1 x 1 x 1 grid); a sample that
 *   picks the cell by its distance to the vertex; tiles and rt_context; the guarded walk.
 * Checks, all before anything is enqueued: rt_render_glow's parameter checks in its order; then RT_ERR_INVALID_ARG for struct_bytes below
 *   8, sample or mis outside {0, 1}, sample = 1 without a volume, sample = 1 without a sampler, a sampler built for another source, other
 *   dimensions or other grids than the call's — still before the scene is looked at; then the null scene, the volume's, the heat's and
 *   the sampler's device against the scene's, and rt_render_glow's remaining checks.  The messages name rt_render_glow_sampled
 *   (rt_trace_samples_glow_sampled); a call that is handed over is rt_render_glow's from there on, and what that call still refuses
 *   (the camera, the environment's device, …) names rt_render_glow.  Handle state and timing: as rt_render_lit. */
typedef struct rt_glow_sample_params {   /* IN, caller-sized like rt_glow_params */
    uint32_t struct_bytes;
    int32_t  sample;        /* 0: off — rt_render_glow itself; 1: the glow is light-sampled */
    int32_t  mis;           /* 1: power heuristic; 0: light sampling alone */
} rt_glow_sample_params;
/* Defaults into *p: sample 0, mis 1; struct_bytes = sizeof(rt_glow_sample_params). */
void rt_glow_sample_params_init(rt_glow_sample_params *p);
typedef struct rt_glow_sampler rt_glow_sampler;
/* The table of `volume` under `source` (heat: source 2 only, the volume's dimensions), on the volume's device, which must be the calling
 * thread's current one.  RT_ERR_INVALID_ARG for a null argument, source outside {0, 1, 2}, heat that is missing under source 2, of other
 * dimensions or on another device, or given under source 0 or 1. */
rt_status rt_glow_sampler_create(const rt_volume *volume, int32_t source, const rt_volume *heat, rt_glow_sampler **out_sampler);
rt_status rt_glow_sampler_destroy(rt_glow_sampler *sampler);
/* The table as the device holds it, HOST memory, each pointer optional: slab_cdf (nz), the rows' cdf of slab z (ny), the cells' cdf and
 * the cells' pc of row y of slab z (nx each); *count = nx * ny * nz, or 0 for an empty sampler. */
rt_status rt_glow_sampler_table(const rt_glow_sampler *sampler, int32_t z, int32_t y, float *slab_cdf, float *row_cdf, float *cell_cdf, float *pc_row,
                                int32_t *count);
/* rt_render_glow with light samples of the glow (sample NULL: the defaults — rt_render_glow itself; sampler: read under sample = 1). */
rt_status rt_render_glow_sampled(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                 const rt_volume *volume, const rt_glow_params *glow, const rt_volume *heat, const rt_glow_sample_params *sample,
                                 const rt_glow_sampler *sampler, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream,
                                 int32_t sync, rt_timing *timing);
/* Probe for tests, HOST memory: rt_trace_samples_glow's columns and glow_samples for the estimator of rt_render_glow_sampled. */
rt_status rt_trace_samples_glow_sampled(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                        const rt_volume *volume, const rt_glow_params *glow, const rt_volume *heat, const rt_glow_sample_params *sample,
                                        const rt_glow_sampler *sampler, int32_t n, const int32_t *ijs, float *radiance, int32_t *rays,
                                        int32_t *medium_events, uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed,
                                        uint32_t *final_medium_seed, int32_t *cells, float *glow_length, int32_t *glow_samples);

/* ---- adaptive sampling under fog -----------------------------------------------------------------------------------
 * rt_render_lit_adaptive_prior's rule, statistics, rounds and prior on rt_render_volume's estimator.  No new arithmetic: a sample is
 * rt_render_volume's under the same lit, medium and volume; the moments, the stopping rules and the prior are those of the adaptive
 * sections above.  stop == NULL or rule == 0, and d_prior == NULL, mean what they mean in rt_render_lit_adaptive_prior.
 *
 * Per-pixel parity.  Pixel p receives samples sample_first … sample_first + n_p - 1 of rt_render_volume; d_fb_sum[p] is rt_render_volume's
 * pixel at samples_per_pixel = n_p and the same sample_first (added in sample order from 0); d_spp[p] = n_p in {min_spp + k * batch_spp <=
 * max_spp}; d_moments (NULL or 2 floats per pixel) holds (S1, S2) of the luminance of the radiance as rt_render_volume adds it —
 * transmittance factors, the medium vertices' light samples and the MIS weights included — float32, in sample order.
 *
 * Identities, bit for bit, in all three outputs: threshold = 0 is rt_render_volume at min_spp + R * batch_spp, every count equal to that.
 * volume == NULL is the same call on rt_render_medium's estimator (the medium's kernels), whatever the region.  A 1 x 1 x 1 grid of density
 * 1 equals volume == NULL with the same box.  medium == NULL or sigma_t == 0 is rt_render_lit_adaptive_prior with the same remaining
 * arguments, handed over after this call's own parameter checks.  A grid of zeros, and a region that no ray of the frame touches, give
 * rt_render_lit_adaptive_prior's outputs through the fog kernels.
 *
 * Checks, all before anything is enqueued, in this order: rt_render_adaptive's parameter checks; the stop parameters'; the prior's;
 * rt_render_lit's (lens, nee, env_params); the medium's; the volume's (a medium with region 2); the sample range of sample_first + min_spp
 * + R * batch_spp; d_fb_sum or d_spp NULL; the null scene; the volume's device against the scene's; the scene's and the camera's as in
 * rt_render_lit; RT_ERR_UNSUPPORTED for pixels x batch_spp at or above 2^31 - 4096 when R > 0.  Messages name rt_render_volume_adaptive.
 * max_depth <= 0: zero sums and moments, the counts by the rule.  Rows of a shard only: no tiles, no rt_context.  Handle state, buffers
 * and timing: as rt_render_lit_adaptive (trace_launches = the min_spp frame's passes + R).
 * Left out: tiles and rt_context; the guarded walk; ~~the denoisers on fogged frames~~ (rt_render_aov_volume, "AOVs under fog" below);
 *   empty-space skipping. */
rt_status rt_render_volume_adaptive(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                    const rt_volume *volume, const rt_adaptive_params *params, const rt_stop_params *stop, const float *d_prior,
                                    const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp, float *d_moments,
                                    void *hip_stream, int32_t sync, rt_timing *timing);

/* ---- AOVs under fog --------------------------------------------------------------------------------------------------
 * The guides rt_denoise and rt_denoise_spp want for a frame of rt_render_medium, rt_render_volume or rt_render_volume_adaptive: the five
 * buffers of rt_render_aov_lens, in which a sample whose camera ray crosses the medium carries the medium's albedo, a normal that faces
 * the camera and a depth inside the fog, each blended with its surface's by the transmittance of the camera ray — and counts as covered
 * even when it hit no surface.  The call takes the beauty call's own lit, medium and volume; of lit only cam_close and lens shape the
 * result, the rest is checked and ignored.  rt_aov_buffers is unchanged; the transmittance is a separate buffer.
 *
 * Deterministic: no draw beyond the camera ray's.  float32 in the order written, nothing fused, division and sqrtf correctly rounded,
 * exp_libm as everywhere.  For sample s of pixel (i, j), sample_first <= s < sample_first + spp, in sample order:
 *   1. (o, d) is the sample's camera ray as rt_render_aov_lens makes it.  A first hit is rt_render_aov's: parameter t_hit, per-sample
 *      albedo a, face-forwarded normal n.  A miss has t_hit = +inf and a = the background.
 *   2. [t0, t1] = interval(o, d, t_hit) of "participating medium"; len = sqrtf(lensq(d)).  Without a volume tau = sigma_t * ((t1 - t0) *
 *      len); with a volume tau is acc of the transmittance walk of "density grid".  Tr = exp_libm(-tau), F = 1 - Tr.
 *   3. The sample is CLEAR when the interval is empty or F == 0: it adds exactly what rt_render_aov_lens adds for it (a clear miss: the
 *      background to the albedo, no count), and 1 to the transmittance.
 *   4. Every other sample is COVERED.  t_fog without a volume: s = RT_AOV_FOG_REM / sigma_t; t_fog = t0 + s / len when s < (t1 - t0) *
 *      len, otherwise t1.  With a volume: the free-flight walk of "density grid" with rem = RT_AOV_FOG_REM in the place of -log_libm(u);
 *      t_fog is its event's t, and t1 without an event.  (t_fog is finite in every region: all-space fog always has the event on a miss.)
 *      ud = unit(d), the medium vertex's.  The sample adds
 *        albedo_sum[k] += Tr * a[k] + F * medium.albedo[k]
 *        normal_sum[k] += Tr * n[k] - F * ud[k]   (a hit)        normal_sum[k] += -(F * ud[k])   (a miss)
 *        depth_sum     += Tr * t_hit + F * t_fog  (a hit)        depth_sum     += t_fog          (a miss)
 *        hit_count     += 1  (a hit or a miss)                   transmittance_sum += Tr
 *      The fog's normal faces the camera: neighbouring fog pixels agree, and a covered pixel never has the zero normal at which
 *      rt_denoise gives a tap no weight.
 *   5. first_prim is rt_render_aov_lens's: the surface of sample sample_first, -1 for a miss, covered or not.
 *
 * Identities, bit for bit in the five buffers: medium == NULL or sigma_t == 0 is rt_render_aov_lens (its kernels, after this call's own
 *   checks; the transmittance is (float)spp).  volume == NULL uses the homogeneous formulas in every region.  A 1 x 1 x 1 grid of density
 *   1, through the grid kernels, equals volume == NULL with the same box.  A grid of zeros, and a region no camera ray touches, give
 *   rt_render_aov_lens's buffers through the fog kernels.
 * Checks, all before anything is enqueued: the buffers first, as in rt_render_aov (all five NULL is an error, with a transmittance pointer
 *   as well); then rt_render_volume's in its order (lit, the medium's, the volume's region 2, the null scene, the volume's device); then
 *   rt_render_aov_samples' sample range and frame checks.  Every message names rt_render_aov_volume.  spp <= 0: zero sums, first_prim -1,
 *   transmittance 0.  Rows of a shard only: no tiles, no rt_context.  Handle state and rt_last_timing: as rt_render_aov_lens leaves them.
 * Left out: the temporal filters (their reprojection takes depth_sum for a surface point, which a fog-blended depth is not); tiles and
 *   rt_context; a separate in-scatter / surface split of the beauty frame. */
#define RT_AOV_FOG_REM 0.693147182f   /* (float)ln 2: the optical depth at which half of the light has met the medium */
rt_status rt_render_aov_volume(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                               const rt_volume *volume, const rt_shard *shard, int32_t sample_first, const rt_aov_buffers *buffers,
                               float *d_transmittance_sum /* NULL or 1 float per pixel */, void *hip_stream, int32_t sync, rt_timing *timing);

/* ---- adaptive sampling on every fog rung -------------------------------------------------------------------------------
 * rt_render_volume_adaptive's rule, statistics, rounds and prior on the estimator of whichever fog call the arguments name: the medium, a
 * density grid, then either a tint ("chromatic extinction") or a glow ("emission in the medium"), and light samples of the glow ("light
 * samples of the glow").  No new arithmetic: a sample is the rung's frame call's — rt_render_medium, rt_render_volume, rt_render_chroma,
 * rt_render_glow or rt_render_glow_sampled, the one that call itself would run after its own hand-overs under the same lit, medium,
 * volume, chroma, glow, heat, sample and sampler; the moments, the stopping rules and the prior are those of the adaptive sections above.
 * stop == NULL or rule == 0, and d_prior == NULL, mean what they mean in rt_render_lit_adaptive_prior.
 *
 * Per-pixel parity.  Pixel p receives samples sample_first … sample_first + n_p - 1 of the rung's frame call; d_fb_sum[p] is that call's
 * pixel at samples_per_pixel = n_p and the same sample_first (added in sample order from 0); d_spp[p] = n_p in {min_spp + k * batch_spp <=
 * max_spp}; d_moments (NULL or 2 floats per pixel) holds (S1, S2) of the luminance of the radiance as that call adds it — the per-channel
 * weights of a tint, the track-length emission and the glow's light samples with their MIS weights included — float32, in sample order.
 *
 * Identities, bit for bit, in all three outputs: threshold = 0 is the rung's frame call at min_spp + R * batch_spp, every count equal to
 * that.  chroma, glow and sample all NULL is rt_render_volume_adaptive with the same remaining arguments (and from there on its own
 * identities: volume == NULL, no medium, a 1 x 1 x 1 grid of density 1).  Equal tints e are the grey call at sigma_t * e.  Radiance 0, 0, 0
 * is the call without a glow.  sample->sample == 0, an empty sampler or a dark glow is the call without a sample.  Each identity runs the
 * lower rung's kernels, as the frame calls' hand-overs do.
 *
 * Checks, all before anything is enqueued, in this order: rt_render_adaptive's parameter checks; the stop parameters'; the prior's; fog ==
 * NULL or fog->struct_bytes below 8 (every field is optional by size: a shorter struct has the ones behind its end NULL); chroma together with
 * glow (a call takes a tint or a glow, not both, because no frame call renders both: decided by the pointers alone, whatever they point
 * to); then the parameter checks of the highest rung the pointers ask for, in that frame call's order (rt_render_lit's, the medium's, the
 * volume's, the tint's or the glow's, the sample's; heat and sampler are not looked at below their rung, and beside a tint — where there
 * is no glow to aim at — neither are sample and sampler: the call is the tint's); the sample range
 * of sample_first + min_spp + R * batch_spp; d_fb_sum or d_spp NULL; the null scene; the volume's, the heat's and the sampler's device
 * against the scene's; the scene's and the camera's as in rt_render_lit; RT_ERR_UNSUPPORTED for pixels x batch_spp at or above 2^31 - 4096
 * when R > 0.  Every message names rt_render_fog_adaptive, after a hand-over too.  max_depth <= 0: zero sums and moments, the counts by the
 * rule.  Rows of a shard only.  Handle state, buffers and timing: as rt_render_volume_adaptive.
 * Left out: AOVs and the denoisers for a tinted medium (a per-channel transmittance guide is a design of its own); rtp_main's --fog-denoise
 *   on --fog-adaptive; a tint together with a glow; tiles and rt_context; the guarded walk. */
typedef struct rt_fog_params {   /* IN, caller-sized; the pointers are read during the call only */
    uint32_t struct_bytes;
    const rt_medium_params *medium;         /* NULL: no medium */
    const rt_volume *volume;                /* NULL: no grid */
    const rt_chroma_params *chroma;         /* NULL: no tint */
    const rt_glow_params *glow;             /* NULL: no glow */
    const rt_volume *heat;                  /* source 2 only */
    const rt_glow_sample_params *sample;    /* NULL: no light samples of the glow */
    const rt_glow_sampler *sampler;         /* read under sample = 1 */
} rt_fog_params;
/* Defaults into *p: every pointer NULL; struct_bytes = sizeof(rt_fog_params). */
void rt_fog_params_init(rt_fog_params *p);
rt_status rt_render_fog_adaptive(rt_scene *scene, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_fog_params *fog,
                                 const rt_adaptive_params *params, const rt_stop_params *stop, const float *d_prior, const rt_shard *shard,
                                 int32_t sample_first, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream, int32_t sync,
                                 rt_timing *timing);

/* Milliseconds of the most recent rt_render kernel of this scene (waits for it). */
rt_status rt_last_kernel_ms(rt_scene *scene, float *ms);
/* The whole rt_timing of the most recent rt_render of this scene (waits for it). */
rt_status rt_last_timing(rt_scene *scene, rt_timing *timing);

/* Convenience for hosts without their own device allocator: the whole of Camera::render up to
 * and including its cudaMemcpy D2H (src/camera.cu:198-209) into a HOST buffer. */
rt_status rt_render_to_host(rt_scene *scene, const rt_camera_data *cam, const rt_shard *shard,
                            float *h_fb_sum, rt_timing *timing);

/* Per-sample probe used by the parity tests: for n (i, j, s) triples (ijs = 3*n int32) returns the
 * radiance ray_color returns for that sample (3*n floats), the number of rays traced (n int32)
 * and the RNG state after the path (n uint32).  All pointers are HOST memory. */
rt_status rt_trace_samples(rt_scene *scene, const rt_camera_data *cam, int32_t n, const int32_t *ijs,
                           float *radiance, int32_t *rays, uint32_t *final_seed);

/* Ray-level probe used by the parity tests: hit_scene (include/scene.h:23-35) for n arbitrary rays
 * (origins/directions = 3*n floats each, HOST memory) with the interval (0.001, 1e30) ray_color
 * uses.  hit[k] = 1/0; t[k] and prim[k] (2*index + type, type 0 sphere / 1 plane) are written for
 * hits only. */
rt_status rt_closest_hits(rt_scene *scene, int32_t n, const float *origins, const float *directions,
                          int32_t *hit, float *t, int32_t *prim);

/* Device buffer management for hosts that do not link the HIP runtime themselves: replace
 * gpu_render's cudaMalloc / cudaFree of the framebuffer (src/camera.cu:295,348) and
 * Camera::render's cudaMemcpy device→host (src/camera.cu:209). */
rt_status rt_device_alloc(uint64_t bytes, void **out_device_ptr);
rt_status rt_device_free(void *device_ptr);
rt_status rt_copy_to_host(void *host_dst, const void *device_src, uint64_t bytes);

/* Device-side saver arithmetic ("next" row f1; ISaver::writeColor, src/camera.cu:138-153):
 * d_rgb8[k] = u8(256*clamp(sqrt(d_fb_sum[k] * (1/divisor)),0,0.999)).  Device pointers. */
rt_status rt_tonemap(const float *d_fb_sum, uint8_t *d_rgb8, int64_t num_floats, int32_t divisor,
                     void *hip_stream);

/* ---- multi-GPU: one frame sharded over the GPUs of one node ------------------------------------------
 * The reference has no multi-GPU path (src/camera.cu:290-349 renders on the current device).  A context owns, per
 * device, a stream, a replica of the scene, that device's rows of the frame and an RCCL communicator (single
 * process; RCCL is bound at run time and only needed for more than one device).  rt_render_sharded() renders the
 * interleaved row bands (band b → device b % N, as rt_shard) on all devices concurrently and rt_gather()s them:
 * ONE grouped ncclSend per device / ncclRecv on the root over xGMI, then the root puts the bands at their image rows.
 * The assembled frame is bit-identical to a one-device rt_render.  One host thread drives a context. */
typedef struct rt_context rt_context;

/* num_devices <= 0: every GPU of the node.  device_ordinals NULL: 0 … num_devices-1.  The first device is the root. */
rt_status rt_context_create(int32_t num_devices, const int32_t *device_ordinals, rt_context **out_ctx);
rt_status rt_context_destroy(rt_context *ctx);
int32_t rt_context_num_devices(const rt_context *ctx);
/* "rccl" (ncclSend/ncclRecv, also for a one-device context when librccl is present), "local" (one device, no RCCL) or
 * "copy" (device_ordinals lists a device more than once — a rehearsal of an N-way shard on fewer GPUs: the rows move
 * with device copies, RCCL does not admit one GPU twice). */
const char *rt_context_transport(const rt_context *ctx);
/* rt_scene_create_ex on every device of the context (replaces the context's previous scene). */
rt_status rt_context_scene_create(rt_context *ctx, const rt_scene_desc *desc, const rt_config *cfg);
/* Camera::render for the whole node: d_fb_sum_root is image_height*image_width*3 floats on the ROOT device; returns
 * when the assembled frame is there.  band_rows <= 0: 8.  timings: NULL or num_devices entries (per-device rt_timing; every entry initialised with rt_timing_init — the first entry's struct_bytes is the array stride).
 * Stream contract: the context works on non-blocking streams of its own.  rt_render_sharded and rt_gather drain the root
 * device (hipDeviceSynchronize) before they write d_fb_sum_root, so work the caller queued on that buffer earlier, on any
 * stream, is complete by then; they return after their own writes are complete.  The caller must not use the buffer from
 * another thread during the call.  With more than one device the RCCL transport has run on real hardware only as a
 * one-device self-gather so far. */
rt_status rt_render_sharded(rt_context *ctx, const rt_camera_data *cam, int32_t band_rows, float *d_fb_sum_root,
                            rt_timing *timings);
/* The collective alone: assembles the rows the devices hold from the last rt_render_sharded of this geometry. */
rt_status rt_gather(rt_context *ctx, int32_t image_width, int32_t image_height, int32_t band_rows, float *d_fb_sum_root);

/* Thread-local text of the last failing call ("" if none). */
const char *rt_get_last_error_string(void);

/* Build identification: "rtp_amd <version> gfx950 parity=<0|1>". */
const char *rt_version_string(void);

#ifdef __cplusplus
}
#endif
#endif /* RTP_AMD_H */
