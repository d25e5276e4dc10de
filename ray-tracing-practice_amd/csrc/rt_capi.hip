// rt_capi.hip — implementation of the C ABI in include/rtp_amd.h on top of the gfx950 kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtp_amd.h"
#include "rt_accel.h"
#include "rt_build.h"
#include "rt_device_math.h"
#include "rt_kernel.hip.inc"
#include "rt_primary.hip.inc"
#include "rt_aov.hip.inc"
#include "rt_adaptive.hip.inc"
#include "rt_nee.hip.inc"
#include "rt_env.hip.inc"
#include "rt_light.hip.inc"
#include "rt_split.hip.inc"
#include "rt_medium.hip.inc"
#include "rt_volume.hip.inc"
#include "rt_glow.hip.inc"
#include "rt_glow_sample.hip.inc"
#include "rt_chroma.hip.inc"
#include "rt_aov_fog.hip.inc"
// Developer build only (make dev → librtp_amd_dev.so, -DRTP_DEV_BUILD): the rt_debug_* entry points (exhaustive on-device checks of
// recip / sqrt_cr / sphere_root, the device LBVH builder on its own, the tripwire, the RTP_STATS counters) at the end of this file.
// The shipped library contains none of them.

namespace {

thread_local std::string g_last_error;

rt_status fail(rt_status st, const std::string &msg) {
    g_last_error = msg;
    return st;
}

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(e_ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP,                   \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                              \
    } while (0)

// Only rt_config_from_env() (an explicit call of the host) reads the environment.
int env_int(const char *name, int fallback) {
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : fallback;
}

// rt_config.workspace_bytes == 0: a sixteenth of the device's memory (18 GB of an MI355X's 288 GB).  The sample slab of a
// pass is the only large allocation of a scene handle and is grown on demand to what the frames actually need: 12.4 GB for
// one 1920x1080x500-spp pass.  A smaller budget only cuts the frame into more passes: 4 GiB → 3 passes, 1.9 % slower
// (each extra pass costs the drain of a trace launch and one more re-walk launch, ≈1.7 ms).
#ifndef RTP_BY_PIXEL_MIN
#define RTP_BY_PIXEL_MIN 96         /* samples per pixel and pass from which the primary-visibility pass takes a wave per PIXEL (configs[4], passes of 125: 10.6 instead of 11.9 ms; S-rtiow at 100 spp: 1.84 vs 1.91) */
#endif
using rtaccel::kWorkspaceShareOfDevice;
using rtaccel::kSampleBytes;

constexpr uint32_t kLdsLimit = 160 * 1024;
using rtaccel::kMaxPasses;               // (rt_accel.h: plan_passes)
constexpr int kTimedPasses = 64;        // trace launches individually timed per call
constexpr uint32_t kResumeBits = 18;    // resume table: 2^18 entries

// Counter block of a scene handle (uint32 words): work counters of the trace launches, of the exact
// re-walk launches, the flagged-sample counts (one each per pass), then 16 developer words.
#ifndef RTP_TAPER_FACTOR
#define RTP_TAPER_FACTOR 2          /* reservations shrink to remaining / (this x waves) */
#endif
constexpr int kQueueWork = 0, kQueueRework = kMaxPasses, kQueueFlag = 2 * kMaxPasses, kQueueStats = 3 * kMaxPasses;
constexpr int kQueueDirty = 3 * kMaxPasses + 16;      // per pass: pixels with a flagged sample (overlapped re-walk)
constexpr int kQueueAbandon = 4 * kMaxPasses + 16;    // per pass: the guarded launch gave up part-way (render_kernel, flag_reserve)
constexpr int kQueueHoles = 5 * kMaxPasses + 16;      // per pass: slots of the flagged-sample list reserved and never filled (flag_chunk_drain)
constexpr int kQueueWords = 6 * kMaxPasses + 16;
static_assert(kQueueHoles - kQueueFlag == (int)rtk::kFlagHolesWords, "the holes word sits where the kernels look for it");
// LDS of a guarded kernel that is neither tables nor stacks nor work ranges: its constants block and, behind it, two words per wave
// (of at most sixteen) for the wave's chunk of the flagged-sample list (rt_kernel.hip.inc: fill_consts, flag_collect)
constexpr uint32_t kGuardBlockBytes = 16u * (uint32_t)rtk::kConstRows + (uint32_t)(rtk::kSimpleBlock / rtk::kWave) * 8u;
// What a render call leaves for the NEXT one to read (rt_scene::feedback): per pass the flagged count and the abandon word, copied
// to pinned host memory at the end of the call, with an event — the handle's decision to step aside from the guarded walk needs no
// rt_last_timing and no synchronisation of the caller's.
constexpr int kFeedbackSlots = 4;
constexpr uint32_t kDefaultBailShare = 64;            // of 256: 25 % (rt_config.guard_bail_share)
constexpr uint32_t kDefaultBailLatest = 2;            // of 8: a pass is given up in its first quarter or not at all
constexpr uint32_t kDefaultBailFloor = 96;            // of 1024: 9.4 % of the pass on the list before it is given up (swept with kDefaultBailLatest: docs/LOG.md round 4)
constexpr uint32_t kExploreShare = 1;                 // of 256: a guarded frame that flagged more than 0.4 % is timed against an exact one …
constexpr float kExploreOverhead = 0.15f;             // … and so is one that spent more than this share of its time outside the trace launch

// Traversal (rt_config.traversal).  EXACT ("threaded"): the caller's tree in the reference's own visit order — the
// result is the reference's by construction.  GUARDED (AUTO's choice where the scene is eligible): near-first walk
// of an SAH tree over inflated leaf boxes; every sample whose result could depend on the visit order
// is flagged and re-walked in threaded mode, so the frame is the same (docs/LOG.md §3b).
// Trees of a few dozen primitives have nothing to gain from a second walk (random scenes of 20-60 spheres: the guarded frame
// 1.3-1.4 x the exact one — its re-walk launch is a fixed half millisecond); everything else eligible gets the
// guarded one (the reference's default scene, ~200 primitives: 12.4 vs 9.0 Gsamples/s).
bool guarded_wanted(const rt_config &cfg, int64_t primitives) {
    if (cfg.traversal == RT_TRAVERSAL_GUARDED) return true;
    return primitives >= cfg.guard_min_primitives;
}

void config_defaults(rt_config &c) {
    std::memset(&c, 0, sizeof(c));
    c.struct_bytes = (uint32_t)sizeof(rt_config);
    c.tree_build = RT_BUILD_HOST_SAH;
    c.guard_gamma_ulps = 0.0f;
    c.traversal = RT_TRAVERSAL_AUTO;
    c.guard_min_primitives = 64;
    c.guard_repack = 1;
    c.kernel = RT_KERNEL_AUTO;
    c.workspace_bytes = 0;
    c.scene_in_lds = 1;
    c.lds_treelet = 1;
    c.reserve_taper = 1;
    c.wide_nodes = 0;
    c.guard_bail_share = 0;
    c.guard_front_primitives = 0;
    c.reuse_view_lists = 0;
    c.resume_flagged = 0;
    c.dark_kernel = 0;
}

// A caller compiled against an older, shorter rt_config: its fields, defaults for the rest.
rt_config config_from_caller(const rt_config *in) {
    rt_config c;
    config_defaults(c);
    if (in && in->struct_bytes >= 8) {
        const size_t n = in->struct_bytes < sizeof(rt_config) ? in->struct_bytes : sizeof(rt_config);
        std::memcpy(&c, in, n);
        c.struct_bytes = (uint32_t)sizeof(rt_config);
    }
    if (c.guard_min_primitives < 0) c.guard_min_primitives = 0;
    return c;
}

// Pair nodes the LDS-resident guarded walk can hold at two workgroups per CU with a stack of seven entries (what render_impl's own
// fit test comes to for the sphere-only build and the general one) — PackOptions::lds_pair_budget: scenes beyond it are packed for
// the walk through L1 / L2 where that costs nothing.  An estimate is enough: both walks render the same frame.
int32_t lds_pair_budget(const rt_scene_desc &d) {
    bool plain = d.num_planes == 0;          // the sphere-only build: no planes, no textures (absorbing glass aside: the estimate may be a little generous)
    for (int i = 0; plain && i < d.num_materials; ++i) plain = d.materials[i].texture_id == 0;
    const int64_t budget = (int64_t)kLdsLimit / 2;
    const int64_t lanes = plain ? rtk::kSimpleBlock : rtk::kBlock;
    const int64_t fixed = (int64_t)d.num_spheres * 16 + ((int64_t)d.num_spheres + 3) / 4 * 16 + (int64_t)d.num_planes * 80 +
                          (plain ? 0 : (int64_t)d.num_materials * 16 * RTP_LDS_MAT_ROWS) + 16 * rtk::kConstRows + (lanes / 64) * (8 + 32 * 4) + 7 * lanes * 4;
    const int64_t nodes = (budget - fixed) / rtk::kOctNodeBytes;
    return (int32_t)(nodes < 1 ? 1 : nodes);
}

rtaccel::PackOptions pack_options(const rt_config &cfg, const rt_scene_desc *d = nullptr) {
    rtaccel::PackOptions o;
    if (d && cfg.scene_in_lds != 0) o.lds_pair_budget = lds_pair_budget(*d);
    o.dynamic = cfg.guard_dynamic_margins;
    if (cfg.guard_gamma_ulps > 0.0f) o.gamma = (double)cfg.guard_gamma_ulps * 5.9604644775390625e-8;
    o.leaf_table = cfg.guard_exact_leaf_table != 0;
    o.front_max = cfg.guard_front_primitives < 0 ? 0 : rtaccel::kMaxFront;
    return o;
}
uint32_t bail_share_of(const rt_config &cfg) {      // in 1/256ths; 0 = never
    if (cfg.guard_bail_share < 0) return 0u;
    const uint32_t s = cfg.guard_bail_share == 0 ? kDefaultBailShare : (uint32_t)cfg.guard_bail_share;
    return s > 255u ? 255u : s;
}
// … and what must be on the list before a pass is given up, in 1/1024ths of the pass (RTP_BAIL_FLOOR: for measurements)
uint32_t bail_floor() {
    static const uint32_t f = [] { const int v = env_int("RTP_BAIL_FLOOR", (int)kDefaultBailFloor); return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }();
    return f;
}
uint32_t bail_latest() {          // … and until when, in eighths of the pass (RTP_BAIL_LATEST)
    static const uint32_t f = [] { const int v = env_int("RTP_BAIL_LATEST", (int)kDefaultBailLatest); return (uint32_t)(v < 1 ? 1 : v > 8 ? 8 : v); }();
    return f;
}
// Out-structures (rt_timing, rt_config; include/rtp_amd.h) are written at the size the caller was compiled with and not a byte beyond
template <class T>
void copy_out(const T &src, T *dst, uint32_t caller_bytes) {
    const uint32_t n = caller_bytes < sizeof(T) ? caller_bytes : (uint32_t)sizeof(T);
    std::memcpy(dst, &src, n);
    dst->struct_bytes = n;
}
rt_status timing_check(const rt_timing *t) {
    if (t && t->struct_bytes < 8) { g_last_error = "rt_timing.struct_bytes is not set (rt_timing_init)"; return RT_ERR_INVALID_ARG; }
    return RT_OK;
}
void timing_out(const rt_timing &src, rt_timing *dst) {
    if (dst) copy_out(src, dst, dst->struct_bytes);
}
bool gamma_unproven(const rt_config &cfg) {
    return cfg.guard_gamma_ulps > 0.0f && (double)cfg.guard_gamma_ulps * 5.9604644775390625e-8 < (double)rtaccel::kGuardGammaBound;
}
// (RT_KERNEL_WAVEFRONT and rt_config.wide_nodes = 1 were experiments, retired: −37 % and −6 % on S-rtiow; docs/LOG.md)
rt_status refuse_retired(const rt_config &cfg) {
    if (cfg.kernel == RT_KERNEL_WAVEFRONT) return fail(RT_ERR_UNSUPPORTED, "RT_KERNEL_WAVEFRONT was an experiment and has been retired: not in this library");
    if (cfg.wide_nodes > 0) return fail(RT_ERR_UNSUPPORTED, "rt_config.wide_nodes = 1 was an experiment and has been retired: not in this library");
    return RT_OK;
}

// The clock of one family of calls (rt_scene::clock): a start and a stop event around everything a call enqueues and, where the family
// counts on the device, counter words of its own.  One per family, so that rt_last_timing goes on reporting the last rt_render after an
// AOV, lens or lit call.
enum { kClockRender, kClockAov, kClockAdaptive, kClockLens, kClockLight, kNumClocks };
struct CallClock {
    hipEvent_t first = nullptr, last = nullptr;
    uint32_t *words = nullptr;
    rt_status make(size_t num_words = 0) {          // by the family's first call
        if (num_words && !words) HIP_TRY(hipMalloc((void **)&words, num_words * sizeof(uint32_t)));
        if (!first) HIP_TRY(hipEventCreate(&first));
        if (!last) HIP_TRY(hipEventCreate(&last));
        return RT_OK;
    }
    rt_status start(hipStream_t stream) { HIP_TRY(hipEventRecord(first, stream)); return RT_OK; }
    rt_status stop(hipStream_t stream) { HIP_TRY(hipEventRecord(last, stream)); return RT_OK; }
    rt_status elapsed(float &ms) {                  // waits for the call to finish
        HIP_TRY(hipEventSynchronize(last));
        HIP_TRY(hipEventElapsedTime(&ms, first, last));
        return RT_OK;
    }
    void destroy() {
        if (first) (void)hipEventDestroy(first);
        if (last) (void)hipEventDestroy(last);
        (void)hipFree(words);
    }
};

}  // namespace

struct rt_scene {
    int device = 0;
    rt_config cfg{};
    float4 *tnodes = nullptr, *xnodes = nullptr;
    int32_t num_tnodes = 0, num_top = 0, num_top_pairs = 0;
    float4 *hnodes = nullptr;       // pair records with binary16 planes (guarded walk from global memory)
    float4 *whnodes = nullptr;      // the same tree as 4-wide nodes (binary16 boxes: step_wide_par); null: pair nodes only
    int32_t num_wide = 0, wroot = rtk::kDone, wide_depth = 0;
    float4 *nodes = nullptr, *spheres = nullptr, *planes = nullptr, *materials = nullptr, *tex_data = nullptr;
    int32_t *sphere_mat = nullptr;
    int4 *tex_info = nullptr;
    uint32_t *queue = nullptr;      // counter block, see kQueue*
    float *slab = nullptr;          // per-sample radiance workspace of one pass (3 floats per sample), grown on demand
    size_t slab_floats = 0;
    rtaccel::Packed::Guard guard;   // guarded-walk eligibility and parameters
    // host copies of what the guard depends on: a camera outside the reach the margins were sized for makes
    // rt_render re-pack the guarded walk's tree for it (reach only ever grows)
    std::vector<rt_sphere> host_spheres;
    std::vector<rt_plane> host_planes;
    std::vector<rt_bvh_node> host_nodes;
    bool device_built = false;
    int repacks = 0;
    bool repack_refused = false;    // a re-pack for a far camera was not eligible: do not try again
    bool guard_paused = false;      // a frame abandoned a guarded pass or flagged more than the bail share of its samples: later frames use the exact walk
    // feedback of the last few render calls (kFeedbackSlots): [0, passes) flagged counts, [kMaxPasses, kMaxPasses + passes) abandon words
    struct Feedback {
        uint32_t *host = nullptr; hipEvent_t start = nullptr, done = nullptr;
        bool pending = false, guarded = false, exploring = false;
        int passes = 0; uint64_t samples = 0, serial = 0;
    };
    Feedback feedback[kFeedbackSlots];
    int feedback_next = 0;
    // RT_TRAVERSAL_AUTO's cost model is a measurement: a guarded frame that flagged more than kExploreShare of its samples makes the
    // handle render ONE frame with the exact walk and keep whichever was faster per sample (judge_frame)
    double guarded_ns_per_sample = 0.0, exact_ns_per_sample = 0.0;
    bool explore_exact = false;
    uint64_t frame_serial = 0;      // render calls so far (a feedback slot knows which one it belongs to)
    uint32_t trip_test = 0;         // developer build: rt_debug_trip_test
    const uint32_t *last_traced_pixels = nullptr;     // device word of the last call's primary-visibility pass (null: every pixel was traced)
    int32_t last_spp = 0;
    float4 *leaf_boxes = nullptr, *plane_leaf_boxes = nullptr;   // exact leaf boxes (final check of the guarded walk)
    uint32_t *flag_list = nullptr;  // work indices of flagged samples, grown on demand
    // resume table (rt_kernel.hip.inc): where a flagged sample's path stood when the flagged ray was armed — 2^18 tags + 64-byte states
    // (17 MB), made with the first guarded frame; a device short of memory renders without it (flagged samples restart from the camera)
    uint32_t *resume_tag = nullptr; float4 *resume_state = nullptr;
    size_t flag_cap = 0;
    // overlapped re-walk: the exact re-walk + the accumulation of the pixels it touches run on aux_stream beside the
    // accumulation of all other pixels on the caller's stream
    uint32_t *dirty = nullptr, *dirty_list = nullptr;      // per local pixel: mark, list of marked pixels
    size_t dirty_cap = 0;
    hipStream_t aux_stream = nullptr, list_stream = nullptr;      // (list_stream: the marked pixels are listed beside the re-walk)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_listed = nullptr;
    uint32_t *cand = nullptr;       // primary visibility: per local pixel rtk::kCandWords words (candidate leaves), grown on demand
    size_t cand_pixels = 0;
    // what the lists in `cand` (and the fetch order behind them) were made for: a call with the same view of the same tree on the
    // same stream — the next sample batch of a progressive render, the next frame of a still — reuses them (0.4 ms at 1080p)
    struct CandKey { float view[12]; int32_t dims[9]; int repacks; hipStream_t stream; bool valid = false; } cand_key;
    int32_t num_internal = 0, num_spheres = 0, num_planes = 0, num_materials = 0, root = rtk::kDone, tree_depth = 0;
    // one clock per family of calls: kClockRender (rt_render*, rt_render_adaptive's min_spp round) is made with the handle and counts in
    // `queue`; rt_render_aov has a counter word of its own, rt_render_lens a counter block, the lit calls a work counter per pass — so
    // that rt_last_timing and the handle's judgement of its guarded walk keep reading what the last rt_render left
    CallClock clock[kNumClocks];
    std::vector<hipEvent_t> pass_events;   // per pass: before the primary pass, before the trace launch, after it, after the exact re-walk (first kTimedPasses passes)
    int timed_passes = 0;
    rt_timing last{};
    int last_passes = 0;
    uint64_t last_samples = 0;
    bool timed = false;
    bool durations_read = false;    // rt_last_timing has measured the timed render's durations once: it reports those from then on
    int num_cus = 0;
    uint64_t device_bytes = 0;      // total memory of the device (workspace default: a sixteenth of it)
    float build_ms = 0.0f;          // device BVH build time (RTP_BUILD=device), else 0
    bool absorbing_glass = false;   // some DIELECTRIC material has a non-zero absorption (Beer-Lambert code needed)
    bool dark = false;              // no material emits and no albedo exceeds 1 (rt_accel.h, scene_emits / albedo_bounded): a path's radiance is +0 until it leaves the scene
    std::vector<hipEvent_t> aov_events;    // rt_render_aov, per timed pass: before the primary pass, before the resolve launch, after it
    // rt_render_adaptive (rt_adaptive.hip.inc): the moments of a caller who passes none (2 floats per local pixel), two lists of pixels
    // (2 x adapt_pixels words: one round reads the previous round's list while it writes its own), the work indices of a round
    // (adapt_work_cap words) and three counter words per round (list length, work indices, trace queue); grown on demand
    float *adapt_mom = nullptr;
    uint32_t *adapt_list = nullptr, *adapt_work = nullptr, *adapt_counters = nullptr;
    size_t adapt_mom_pixels = 0, adapt_pixels = 0, adapt_work_cap = 0, adapt_counter_words = 0;
    // rule 1 (rt_render_adaptive_rule): c, one byte per local pixel
    uint8_t *adapt_flag = nullptr;
    size_t adapt_flag_pixels = 0;
    // rt_render_nee (rt_nee.hip.inc): the emitter table, made by the handle's first call (host copy + device columns)
    bool nee_built = false;
    std::vector<int32_t> nee_index;
    std::vector<float> nee_cdf, nee_pmf;
    int32_t *nee_index_dev = nullptr;
    float *nee_cdf_dev = nullptr, *nee_pmf_dev = nullptr;
    // … and the table of sample_planes = 1 (spheres, then planes: code = 2 * index + kind), made by the same call.  Without a qualifying
    // plane it is the first table again and is never handed to a kernel (emit_planes == 0: no device columns)
    std::vector<int32_t> emit_code;
    std::vector<float> emit_cdf, emit_pmf, emit_area;
    int32_t emit_spheres = 0, emit_planes = 0;
    int32_t *emit_code_dev = nullptr;
    float *emit_cdf_dev = nullptr, *emit_pmf_dev = nullptr, *emit_area_dev = nullptr;
    // … and the light trees of select = 1, one per table ([0] the sphere-only one, [1] the two-kind one), each built by
    // the first call that selects it from what the tables' read-back left: every entry's centre (3 doubles), radius and weight
    struct LightTreeHost {
        bool built = false;
        std::vector<float> node;               // 8 words per node, preorder: centre, radius, weight, q, right, entry (int bits)
        std::vector<uint32_t> path;            // per entry
        std::vector<int32_t> depth;
        float4 *node_dev = nullptr;
        uint32_t *path_dev = nullptr;
        int32_t *depth_dev = nullptr;
    } tree[2];
    std::vector<double> emit_geom;             // per entry of the two-kind table (the sphere-only one is its first emit_spheres): c0 c1 c2 rho w
};

namespace {

template <class T>
rt_status upload(const std::vector<T> &host, void **dev) {
    *dev = nullptr;
    if (host.empty()) return RT_OK;
    HIP_TRY(hipMalloc(dev, host.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

using rtaccel::make_magic;

void normalise_shard(const rt_shard *in, int32_t height, rt_shard &out) {
    if (!in || in->num_parts <= 1 || in->band_rows <= 0) {
        out.band_rows = height > 0 ? height : 1;
        out.num_parts = 1;
        out.part = 0;
    } else {
        out = *in;
    }
}

// A scene's tables live on the device it was created on: calls from a thread whose current device is another one
// would launch there with this device's pointers.
rt_status check_device(const rt_scene *sc) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return fail(RT_ERR_HIP, "hipGetDevice failed");
    if (cur != sc->device)
        return fail(RT_ERR_INVALID_ARG, "scene was created on device " + std::to_string(sc->device) + " but the calling thread's current device is " +
                                            std::to_string(cur) + " (call rt_set_device first)");
    return RT_OK;
}

struct Tile { int32_t x0, y0, w, h; };
rt_status fill_params(const rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, rtk::KParams &P, const Tile *tile = nullptr) {
    std::memset(&P, 0, sizeof(P));
    if (!sc || !cam) return fail(RT_ERR_INVALID_ARG, "null scene or camera");
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(RT_ERR_INVALID_ARG, "image size must be positive");
    // (tile offsets travel in 24 bits of the guarded kernels' constants block: fill_consts)
    if (cam->image_width >= (1 << 24) || cam->image_height >= (1 << 24)) return fail(RT_ERR_UNSUPPORTED, "image width or height of 2^24 or more");
    if (shard && shard->num_parts > 1 && (shard->part < 0 || shard->part >= shard->num_parts || shard->band_rows <= 0))
        return fail(RT_ERR_INVALID_ARG, "bad shard");
    std::memcpy(P.origin, cam->origin.e, 12);
    std::memcpy(P.p00, cam->pixel00_loc.e, 12);
    std::memcpy(P.du, cam->pixel_delta_u.e, 12);
    std::memcpy(P.dv, cam->pixel_delta_v.e, 12);
    std::memcpy(P.bg, cam->background.e, 12);
    P.width = cam->image_width;
    P.height = cam->image_height;
    P.spp = cam->samples_per_pixel;
    P.max_depth = cam->max_depth;
    rt_shard s;
    normalise_shard(shard, cam->image_height, s);
    P.band_rows = s.band_rows;
    P.num_parts = s.num_parts;
    P.part = s.part;
    P.local_rows = rt_shard_rows(cam->image_height, shard);
    P.row_w = P.width;
    if (tile) {             // a rectangle of the image instead of row bands
        if (shard && shard->num_parts > 1) return fail(RT_ERR_INVALID_ARG, "a tile and a shard in one call");
        if (tile->w <= 0 || tile->h <= 0 || tile->x0 < 0 || tile->y0 < 0 || (int64_t)tile->x0 + tile->w > cam->image_width ||
            (int64_t)tile->y0 + tile->h > cam->image_height)
            return fail(RT_ERR_INVALID_ARG, "tile outside the image");
        P.local_rows = tile->h;
        P.row_w = tile->w;
        P.tile_x0 = tile->x0;
        P.tile_y0 = tile->y0;
    }
    P.nodes = sc->nodes; P.hnodes = sc->hnodes; P.num_internal = sc->num_internal; P.root = sc->root;
    P.whnodes = sc->whnodes; P.wroot = sc->wroot;
    P.tnodes = sc->tnodes; P.num_tnodes = sc->num_tnodes;
    P.xnodes = sc->xnodes; P.num_top = sc->num_top;
    P.spheres = sc->spheres; P.num_spheres = sc->num_spheres;
    P.planes = sc->planes; P.num_planes = sc->num_planes;
    P.materials = sc->materials; P.num_materials = sc->num_materials;
    P.sphere_mat = sc->sphere_mat;
    P.tex_data = sc->tex_data; P.tex_info = sc->tex_info;
    P.queue = sc->queue;
    if ((uint64_t)P.local_rows * (uint64_t)P.row_w > (1u << 24)) return fail(RT_ERR_UNSUPPORTED, "more than 2^24 pixels per call");
    P.total_work = 0;      // set per pass in rt_render
    P.stats = sc->queue + kQueueStats;
    P.trip_test = sc->trip_test;
    {
        const uint64_t pixels = (uint64_t)P.local_rows * (uint64_t)P.row_w;
        if (!make_magic((uint32_t)P.row_w, pixels + 1, P.magic_width) ||
            !make_magic((uint32_t)P.band_rows, (uint64_t)P.local_rows + 1, P.magic_band))
            return fail(RT_ERR_UNSUPPORTED, "image too large for the work index arithmetic");
    }
    P.stack_levels = 0;
    P.leaf_boxes = sc->leaf_boxes;
    P.plane_leaf_boxes = sc->plane_leaf_boxes;
    std::memcpy(P.g_center, sc->guard.center, 12);
    P.g_d0sq = sc->guard.d0_sq;
    P.g_rs = sc->guard.cluster_radius;
    P.g_fark = sc->guard.far_k;
    P.g_dynk = sc->guard.dyn_k;
    {   // step_pair_par: sqrt(k) with the walk's slack, and sqrt(k) sqrt(3) r_max — both rounded up
        // (sqrt(k) also multiplies the kernel's APPROXIMATE sqrt of |d|^2 — one ulp — and rounds in a float product: 4e-6 on top)
        const double sk = std::sqrt((double)sc->guard.dyn_k * (double)rtk::kDynSlack) * (1.0 + 4e-6);
        P.g_dyn_sqrtk = std::nextafterf((float)sk, INFINITY);
        P.g_dyn_b = std::nextafterf((float)(sk * 1.7320508075688772 * (double)sc->guard.dyn_rmax * (1.0 + 1e-6)), INFINITY);
        P.g_dyn_c3 = std::nextafterf((float)(sk * 1.7320508075688772), INFINITY);
        P.g_dyn_kslack = std::nextafterf((float)((double)sc->guard.dyn_k * (double)rtk::kDynSlack), INFINITY);
    }
    P.num_front = sc->guard.num_front;
    std::memcpy(P.front_code, sc->guard.front_code, sizeof(P.front_code));
    std::memcpy(P.front_box, sc->guard.front_box, sizeof(P.front_box));
    std::memcpy(P.g_box, sc->guard.box, 24);
    P.k_inner = sc->cfg.k_inner > 0 ? sc->cfg.k_inner : 24;
    P.k_shade = sc->cfg.k_shade > 0 ? sc->cfg.k_shade : 48;
    P.chunk = 64u;      // set per pass in rt_render
    return RT_OK;
}

// Re-pack the guarded walk's tree with margins that cover ray origins at `cam` (see rt_render).
rt_status repack_for_camera(rt_scene *sc, const float cam[3], hipStream_t stream) {
    rt_scene_desc d{};
    d.spheres = sc->host_spheres.data(); d.num_spheres = (int32_t)sc->host_spheres.size();
    d.planes = sc->host_planes.data(); d.num_planes = (int32_t)sc->host_planes.size();
    d.nodes = sc->host_nodes.data(); d.num_nodes = (int32_t)sc->host_nodes.size();
    // materials and textures do not enter the tree: one dummy material satisfies the index validation
    std::vector<rt_sphere> spheres(sc->host_spheres);
    std::vector<rt_plane> planes(sc->host_planes);
    for (rt_sphere &s : spheres) s.material_idx = 0;
    for (rt_plane &p : planes) p.material_idx = 0;
    rt_material dummy{};
    d.spheres = spheres.data();
    d.planes = planes.data();
    d.materials = &dummy; d.num_materials = 1;
    rtaccel::Packed pk;
    const std::string err = rtaccel::pack_scene(d, rtaccel::TreeMode::Guarded, pk, pack_options(sc->cfg, &d), cam);
    if (!err.empty()) return fail(RT_ERR_INVALID_ARG, "re-pack for a far camera: " + err);
    if (!pk.guard.ok) {          // margins for that distance would swallow the tree: such cameras get the exact walk
        sc->repack_refused = true;
        return RT_OK;
    }
    HIP_TRY(hipStreamSynchronize(stream));          // the old tables may still be in use on this stream
    float4 *nodes = nullptr, *hnodes = nullptr, *whnodes = nullptr, *leaf_boxes = nullptr, *plane_leaf_boxes = nullptr;
    rt_status st = RT_OK;
    if ((st = upload(pk.nodes, (void **)&nodes)) != RT_OK || (st = upload(pk.hnodes, (void **)&hnodes)) != RT_OK ||
        (st = upload(pk.whnodes, (void **)&whnodes)) != RT_OK ||
        (st = upload(pk.leaf_boxes, (void **)&leaf_boxes)) != RT_OK || (st = upload(pk.plane_leaf_boxes, (void **)&plane_leaf_boxes)) != RT_OK) {
        (void)hipFree(nodes); (void)hipFree(hnodes); (void)hipFree(whnodes); (void)hipFree(leaf_boxes); (void)hipFree(plane_leaf_boxes);
        return st;
    }
    (void)hipFree(sc->nodes); (void)hipFree(sc->hnodes); (void)hipFree(sc->whnodes);
    (void)hipFree(sc->leaf_boxes); (void)hipFree(sc->plane_leaf_boxes);
    sc->nodes = nodes; sc->hnodes = hnodes; sc->whnodes = whnodes; sc->leaf_boxes = leaf_boxes; sc->plane_leaf_boxes = plane_leaf_boxes;
    sc->num_wide = pk.num_wide; sc->wroot = pk.wroot; sc->wide_depth = pk.wide_depth;
    sc->num_internal = pk.num_internal;
    sc->num_top_pairs = pk.num_top_pairs;
    sc->root = pk.root;
    sc->tree_depth = pk.max_depth;
    sc->guard = pk.guard;
    sc->repacks++;
    return RT_OK;
}

}  // namespace

// for rt_multi.hip (same library, not exported)
__attribute__((visibility("hidden"))) void rt_internal_set_error(const std::string &msg) { g_last_error = msg; }

extern "C" {

const char *rt_get_last_error_string(void) { return g_last_error.c_str(); }

// parity: the arithmetic flags the bit-for-bit claims rest on (no contraction, IEEE divide / sqrt, denormals kept, no fast-math) —
// the Makefile passes -DRTP_PARITY_FLAGS=1 together with them, and only with them; dev: the developer build (see above)
#if defined(RTP_PARITY_FLAGS) && !defined(__FAST_MATH__)
#define RTP_VERSION_PARITY "1"
#else
#define RTP_VERSION_PARITY "0"
#endif
#ifdef RTP_DEV_BUILD
#define RTP_VERSION_DEV "1"
#else
#define RTP_VERSION_DEV "0"
#endif
const char *rt_version_string(void) { return "rtp_amd 0.5 gfx950 parity=" RTP_VERSION_PARITY " dev=" RTP_VERSION_DEV; }

rt_status rt_set_device(int32_t device_ordinal) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(RT_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device_ordinal));
    return RT_OK;
}

// (the header's macro of the same name calls rt_config_init_sized with the caller's sizeof; this is the symbol FFI bindings reach)
void (rt_config_init)(rt_config *cfg) {
    if (cfg) config_defaults(*cfg);
}
void rt_config_init_sized(rt_config *cfg, uint32_t struct_bytes) {
    if (!cfg || struct_bytes < 8) return;
    rt_config c;
    config_defaults(c);
    copy_out(c, cfg, struct_bytes);
}

void rt_config_from_env(rt_config *user) {
    if (!user || user->struct_bytes < 8) return;
    // (on a copy of the library's size: a caller compiled against a shorter rt_config gets back only the fields it has)
    rt_config full = config_from_caller(user);
    rt_config *cfg = &full;
    auto str_is = [](const char *name, const char *value) { const char *v = getenv(name); return v && std::string(v) == value; };
    if (str_is("RTP_TRAVERSAL", "threaded") || str_is("RTP_TRAVERSAL", "exact")) cfg->traversal = RT_TRAVERSAL_EXACT;
    if (str_is("RTP_TRAVERSAL", "guarded")) cfg->traversal = RT_TRAVERSAL_GUARDED;
    if (str_is("RTP_BUILD", "device")) cfg->tree_build = RT_BUILD_DEVICE_LBVH;
    if (str_is("RTP_KERNEL", "mega")) cfg->kernel = RT_KERNEL_MEGA;
    if (str_is("RTP_KERNEL", "wavefront")) cfg->kernel = RT_KERNEL_WAVEFRONT;
    if (const char *v = getenv("RTP_GUARD_GAMMA_ULPS")) cfg->guard_gamma_ulps = (float)atof(v);
    cfg->guard_exact_leaf_table = env_int("RTP_GUARD_TABLE", cfg->guard_exact_leaf_table);
    cfg->guard_dynamic_margins = env_int("RTP_GUARD_DYNAMIC", cfg->guard_dynamic_margins);
    cfg->guard_min_primitives = env_int("RTP_GUARD_MIN_PRIMS", cfg->guard_min_primitives);
    cfg->guard_keep = env_int("RTP_GUARD_KEEP", cfg->guard_keep);
    if (env_int("RTP_NO_REPACK", 0)) cfg->guard_repack = 0;
    if (const char *v = getenv("RTP_SLAB_GIB")) { const double g = atof(v); if (g > 0) cfg->workspace_bytes = (uint64_t)(g * 1073741824.0); }
    cfg->pass_spp = env_int("RTP_PASS_SPP", cfg->pass_spp);
    cfg->stack_levels = env_int("RTP_STACK_LEVELS", cfg->stack_levels);
    cfg->flag_capacity = (uint32_t)env_int("RTP_FLAG_CAP", (int)cfg->flag_capacity);
    if (env_int("RTP_NO_LDS_SCENE", 0)) cfg->scene_in_lds = 0;
    if (env_int("RTP_NO_TREELET", 0)) cfg->lds_treelet = 0;
    cfg->workgroups_per_cu = env_int("RTP_WGS_PER_CU", cfg->workgroups_per_cu);
    cfg->k_inner = env_int("RTP_K_INNER", cfg->k_inner);
    cfg->k_shade = env_int("RTP_K_SHADE", cfg->k_shade);
    cfg->reserve_chunk = env_int("RTP_CHUNK", cfg->reserve_chunk);
    cfg->wavefront_paths = env_int("RTP_WF_PATHS", cfg->wavefront_paths);
    cfg->wavefront_exchange = env_int("RTP_WF_EXCHANGE", cfg->wavefront_exchange);
    if (env_int("RTP_NO_TAPER", 0)) cfg->reserve_taper = 0;
    cfg->wide_nodes = env_int("RTP_WIDE", cfg->wide_nodes);
    if (env_int("RTP_NO_SIMPLE", 0)) cfg->sphere_only_kernel = -1;
    if (env_int("RTP_NO_DARK", 0)) cfg->dark_kernel = -1;
    if (env_int("RTP_NO_OVERLAP", 0)) cfg->overlap_rework = -1;
    if (env_int("RTP_NO_PRIMARY", 0)) cfg->primary_visibility = -1;
    cfg->guard_bail_share = env_int("RTP_BAIL_SHARE", cfg->guard_bail_share);
    if (env_int("RTP_NO_FRONT", 0)) cfg->guard_front_primitives = -1;
    if (env_int("RTP_NO_VIEW_CACHE", 0)) cfg->reuse_view_lists = -1;
    if (env_int("RTP_NO_RESUME", 0)) cfg->resume_flagged = -1;
    copy_out(full, user, user->struct_bytes);
}

rt_status rt_scene_create(const rt_scene_desc *desc, rt_scene **out_scene) { return rt_scene_create_ex(desc, nullptr, out_scene); }

rt_status rt_scene_set_config(rt_scene *sc, const rt_config *cfg) {
    if (!sc || !cfg) return fail(RT_ERR_INVALID_ARG, "null argument");
    rt_config c = config_from_caller(cfg);
    // create-time fields keep the values the tables were built with
    c.tree_build = sc->cfg.tree_build;
    c.guard_gamma_ulps = sc->cfg.guard_gamma_ulps;
    c.guard_exact_leaf_table = sc->cfg.guard_exact_leaf_table;
    c.guard_dynamic_margins = sc->cfg.guard_dynamic_margins;
    c.guard_front_primitives = sc->cfg.guard_front_primitives;
    sc->cfg = c;
    return RT_OK;
}

rt_status rt_scene_get_config(const rt_scene *sc, rt_config *cfg) {
    if (!sc || !cfg) return fail(RT_ERR_INVALID_ARG, "null argument");
    if (cfg->struct_bytes < 8) return fail(RT_ERR_INVALID_ARG, "rt_config.struct_bytes is not set (rt_config_init)");
    copy_out(sc->cfg, cfg, cfg->struct_bytes);
    return RT_OK;
}

rt_status rt_scene_create_ex(const rt_scene_desc *desc, const rt_config *user_cfg, rt_scene **out_scene) {
    if (!desc || !out_scene) return fail(RT_ERR_INVALID_ARG, "null argument");
    *out_scene = nullptr;
    const rt_config cfg = config_from_caller(user_cfg);
    if (cfg.guard_gamma_ulps < 0.0f || !(cfg.guard_gamma_ulps == cfg.guard_gamma_ulps)) return fail(RT_ERR_INVALID_ARG, "guard_gamma_ulps must be >= 0");
    rtaccel::Packed pk;
    const rtaccel::PackOptions popt = pack_options(cfg, desc);
    // RT_BUILD_DEVICE_LBVH: the guarded walk's tree is built on the GPU (LBVH, rt_build.hip) instead of the host's SAH
    // builder — any tree over the inflated leaves gives the same image (docs/LOG.md §3b)
    const bool device_build = cfg.tree_build == RT_BUILD_DEVICE_LBVH;
    std::string err = rtaccel::pack_scene(*desc, device_build ? rtaccel::TreeMode::GuardedLeaves : rtaccel::TreeMode::Guarded, pk, popt);
    if (!err.empty()) return fail(RT_ERR_INVALID_ARG, err);
    if (device_build && !pk.guard.ok) {       // not eligible for the guarded walk: nothing to build, exact walk only
        err = rtaccel::pack_scene(*desc, rtaccel::TreeMode::Guarded, pk, popt);
        if (!err.empty()) return fail(RT_ERR_INVALID_ARG, err);
    }

    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device");
    rt_scene *sc = new (std::nothrow) rt_scene;
    if (!sc) return fail(RT_ERR_OUT_OF_MEMORY, "host allocation failed");
    sc->cfg = cfg;
    rt_status st = RT_OK;
    auto bail = [&](rt_status s) { rt_scene_destroy(sc); return s; };
    if (hipGetDevice(&sc->device) != hipSuccess) return bail(fail(RT_ERR_HIP, "hipGetDevice failed"));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, sc->device) != hipSuccess) return bail(fail(RT_ERR_HIP, "hipGetDeviceProperties failed"));
    sc->num_cus = prop.multiProcessorCount;
    sc->device_bytes = (uint64_t)prop.totalGlobalMem;
    if (device_build && pk.guard.ok) {
        rtbuild::DeviceTree tree;
        const std::string berr = rtbuild::build_lbvh(pk.guard_leaf_boxes.data(), pk.guard_leaf_codes.data(), (int32_t)pk.guard_leaf_codes.size(), tree);
        if (!berr.empty()) return bail(fail(RT_ERR_HIP, "device BVH build: " + berr));
        sc->nodes = (float4 *)tree.nodes;
        sc->hnodes = (float4 *)tree.hnodes;
        pk.num_internal = tree.num_internal;
        pk.root = tree.root;
        pk.max_depth = tree.depth;
        pk.num_top_pairs = 0;
        sc->build_ms = tree.build_ms;
    } else {
        if ((st = upload(pk.nodes, (void **)&sc->nodes)) != RT_OK) return bail(st);
        if ((st = upload(pk.hnodes, (void **)&sc->hnodes)) != RT_OK) return bail(st);
        if ((st = upload(pk.whnodes, (void **)&sc->whnodes)) != RT_OK) return bail(st);
        sc->num_wide = pk.num_wide; sc->wroot = pk.wroot; sc->wide_depth = pk.wide_depth;
    }
    if ((st = upload(pk.tnodes, (void **)&sc->tnodes)) != RT_OK) return bail(st);
    sc->num_tnodes = pk.num_tnodes;
    if ((st = upload(pk.xnodes, (void **)&sc->xnodes)) != RT_OK) return bail(st);
    sc->num_top = pk.num_top;
    if ((st = upload(pk.spheres, (void **)&sc->spheres)) != RT_OK) return bail(st);
    if ((st = upload(pk.planes, (void **)&sc->planes)) != RT_OK) return bail(st);
    if ((st = upload(pk.materials, (void **)&sc->materials)) != RT_OK) return bail(st);
    if ((st = upload(pk.sphere_mat, (void **)&sc->sphere_mat)) != RT_OK) return bail(st);
    if ((st = upload(pk.tex_data, (void **)&sc->tex_data)) != RT_OK) return bail(st);
    if ((st = upload(pk.tex_info, (void **)&sc->tex_info)) != RT_OK) return bail(st);
    if ((st = upload(pk.leaf_boxes, (void **)&sc->leaf_boxes)) != RT_OK) return bail(st);
    if ((st = upload(pk.plane_leaf_boxes, (void **)&sc->plane_leaf_boxes)) != RT_OK) return bail(st);
    sc->guard = pk.guard;
    for (int32_t m = 0; m < desc->num_materials; ++m) {
        const rt_material &mat = desc->materials[m];
        if (mat.type == RT_MAT_DIELECTRIC && !(mat.absorption.e[0] == 0.0f && mat.absorption.e[1] == 0.0f && mat.absorption.e[2] == 0.0f)) sc->absorbing_glass = true;
    }
    sc->dark = !rtaccel::scene_emits(desc->materials, desc->num_materials) && rtaccel::albedo_bounded(desc->materials, desc->num_materials);
    if (pk.guard.ok) {
        sc->host_spheres.assign(desc->spheres, desc->spheres + desc->num_spheres);
        sc->host_planes.assign(desc->planes, desc->planes + desc->num_planes);
        sc->host_nodes.assign(desc->nodes, desc->nodes + desc->num_nodes);
        sc->device_built = device_build;
    }
    if (hipMalloc((void **)&sc->queue, kQueueWords * 4) != hipSuccess) return bail(fail(RT_ERR_OUT_OF_MEMORY, "hipMalloc(queue) failed"));
    if (sc->clock[kClockRender].make() != RT_OK) return bail(fail(RT_ERR_HIP, "hipEventCreate failed"));
    sc->num_internal = pk.num_internal;
    sc->num_top_pairs = pk.num_top_pairs;
    sc->num_spheres = (int32_t)pk.sphere_mat.size();
    sc->num_planes = (int32_t)(pk.planes.size() / 20);
    sc->num_materials = (int32_t)(pk.materials.size() / 12);
    sc->root = pk.root;
    sc->tree_depth = pk.max_depth;
    *out_scene = sc;
    return RT_OK;
}

rt_status rt_scene_destroy(rt_scene *sc) {
    if (!sc) return RT_OK;
    (void)hipFree(sc->tnodes);
    (void)hipFree(sc->xnodes);
    (void)hipFree(sc->nodes); (void)hipFree(sc->hnodes); (void)hipFree(sc->whnodes);
    (void)hipFree(sc->spheres); (void)hipFree(sc->planes); (void)hipFree(sc->materials);
    (void)hipFree(sc->sphere_mat); (void)hipFree(sc->tex_data); (void)hipFree(sc->tex_info); (void)hipFree(sc->queue); (void)hipFree(sc->slab);
    (void)hipFree(sc->leaf_boxes); (void)hipFree(sc->plane_leaf_boxes); (void)hipFree(sc->flag_list);
    (void)hipFree(sc->dirty); (void)hipFree(sc->dirty_list); (void)hipFree(sc->cand);
    (void)hipFree(sc->resume_tag); (void)hipFree(sc->resume_state);
    if (sc->aux_stream) (void)hipStreamDestroy(sc->aux_stream);
    if (sc->list_stream) (void)hipStreamDestroy(sc->list_stream);
    if (sc->ev_listed) (void)hipEventDestroy(sc->ev_listed);
    if (sc->ev_fork) (void)hipEventDestroy(sc->ev_fork);
    if (sc->ev_join) (void)hipEventDestroy(sc->ev_join);
    for (hipEvent_t e : sc->pass_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : sc->aov_events) (void)hipEventDestroy(e);
    for (CallClock &c : sc->clock) c.destroy();         // (every family's events and counter words)
    (void)hipFree(sc->adapt_mom); (void)hipFree(sc->adapt_list); (void)hipFree(sc->adapt_work); (void)hipFree(sc->adapt_counters);
    (void)hipFree(sc->adapt_flag);
    (void)hipFree(sc->nee_index_dev); (void)hipFree(sc->nee_cdf_dev); (void)hipFree(sc->nee_pmf_dev);
    (void)hipFree(sc->emit_code_dev); (void)hipFree(sc->emit_cdf_dev); (void)hipFree(sc->emit_pmf_dev); (void)hipFree(sc->emit_area_dev);
    for (auto &t : sc->tree) { (void)hipFree(t.node_dev); (void)hipFree(t.path_dev); (void)hipFree(t.depth_dev); }
    for (rt_scene::Feedback &f : sc->feedback) {
        if (f.done) { if (f.pending) (void)hipEventSynchronize(f.done); (void)hipEventDestroy(f.done); }
        if (f.start) (void)hipEventDestroy(f.start);
        if (f.host) (void)hipHostFree(f.host);
    }
    delete sc;
    return RT_OK;
}

const char *rt_scene_guard_reason(const rt_scene *sc) {
    if (!sc) return "null scene";
    return sc->guard.ok ? "" : sc->guard.reason.c_str();
}

int32_t rt_shard_rows(int32_t image_height, const rt_shard *shard) {
    if (image_height <= 0) return 0;
    if (!shard || shard->num_parts <= 1 || shard->band_rows <= 0) return image_height;
    const int64_t band = shard->band_rows, parts = shard->num_parts, part = shard->part;
    if (part < 0 || part >= parts) return 0;
    const int64_t cycle = band * parts;
    const int64_t full = image_height / cycle, rem = image_height % cycle;
    int64_t rows = full * band;
    const int64_t start = part * band;
    if (rem > start) rows += (rem - start < band) ? rem - start : band;
    return (int32_t)rows;
}

}  // extern "C"

namespace {
// The handle's own judgement of its guarded walk, from what a finished render call left behind (its flagged counts, abandon words
// and event times): a pass that gave up, or more flagged samples overall than the bail share, and the following frames go to the
// exact walk; a frame that flagged more than kExploreShare makes the next AUTO frame an exact one, and the faster of the two per
// sample stays (rt_config.guard_keep: the guarded walk stays whatever happens).
// passes beyond the individually timed ones are priced at the mean of the timed ones
float untimed_scale(int passes, int timed) { return (float)passes / (float)timed; }
// trace / re-walk / primary-pass time of the handle's most recent frame, from its per-pass events (the frame must be done)
rt_status frame_parts(rt_scene *sc, float &trace, float &rework, float &primary) {
    trace = rework = primary = 0.0f;
    for (int p = 0; p < sc->timed_passes; ++p) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, sc->pass_events[4 * p], sc->pass_events[4 * p + 1]));
        primary += ms;
        HIP_TRY(hipEventElapsedTime(&ms, sc->pass_events[4 * p + 1], sc->pass_events[4 * p + 2]));
        trace += ms;
        HIP_TRY(hipEventElapsedTime(&ms, sc->pass_events[4 * p + 2], sc->pass_events[4 * p + 3]));
        rework += ms;
    }
    if (sc->timed_passes > 0) {
        const float scale = untimed_scale((int)sc->last.trace_launches, sc->timed_passes);
        trace *= scale; rework *= scale; primary *= scale;
        float ms = 0.0f;          // + the per-pixel candidate lists, made once per call before the first pass
        HIP_TRY(hipEventElapsedTime(&ms, sc->clock[kClockRender].first, sc->pass_events[0]));
        primary += ms;
    }
    return RT_OK;
}
rt_status judge_frame(rt_scene *sc, rt_scene::Feedback &f) {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, f.start, f.done));
    const double ns = f.samples ? (double)ms * 1e6 / (double)f.samples : 0.0;
    const uint32_t share = bail_share_of(sc->cfg);
    if (f.guarded) {
        uint64_t total = 0;
        uint32_t gave_up = 0;
        // (list slots handed out less the ones nobody filled: rt_kernel.hip.inc, flag_chunk_drain)
        for (int p = 0; p < f.passes; ++p) { total += f.host[p] - f.host[2 * kMaxPasses + p]; gave_up += f.host[kMaxPasses + p] != 0u ? 1u : 0u; }
        if (share != 0u && (gave_up != 0u || total * 256u > (uint64_t)share * f.samples)) sc->guard_paused = true;
        if (gave_up == 0u) sc->guarded_ns_per_sample = ns;
        // worth a measurement?  many flagged samples, or much time spent on what the exact walk does not need (the primary pass,
        // the re-walk launch) — the guarded trace launch would have to be faster by that much just to draw level
        bool doubt = total * 256u > (uint64_t)kExploreShare * f.samples;
        if (!doubt && f.serial == sc->frame_serial && sc->timed) {       // (the per-pass events are this frame's: nothing was enqueued after it)
            float trace = 0.0f, rework = 0.0f, primary = 0.0f;
            if (const rt_status st = frame_parts(sc, trace, rework, primary)) return st;
            doubt = rework + primary > kExploreOverhead * ms;
        }
        if (share != 0u && !sc->guard_paused && sc->exact_ns_per_sample == 0.0 && doubt) sc->explore_exact = true;
    } else if (f.exploring) {
        sc->exact_ns_per_sample = ns;
        sc->explore_exact = false;
        if (sc->guarded_ns_per_sample > 0.0 && ns < 0.95 * sc->guarded_ns_per_sample) sc->guard_paused = true;
    }
    return RT_OK;
}
// feedback slots whose frames have finished are read (wait_all: every pending one is waited for)
rt_status poll_feedback(rt_scene *sc, bool wait_all) {
    for (int k = 0; k < kFeedbackSlots; ++k) {
        rt_scene::Feedback &f = sc->feedback[(sc->feedback_next + k) % kFeedbackSlots];      // oldest first
        if (!f.pending) continue;
        if (wait_all) HIP_TRY(hipEventSynchronize(f.done));
        const hipError_t e = hipEventQuery(f.done);
        if (e == hipErrorNotReady) continue;
        HIP_TRY(e);
        f.pending = false;
        if (const rt_status st = judge_frame(sc, f)) return st;
    }
    return RT_OK;
}
// the slot of the frame about to be enqueued
rt_status acquire_feedback(rt_scene *sc, rt_scene::Feedback **out) {
    rt_scene::Feedback &f = sc->feedback[sc->feedback_next];
    sc->feedback_next = (sc->feedback_next + 1) % kFeedbackSlots;
    if (f.pending) {                   // the caller is kFeedbackSlots frames ahead of the device: wait for the oldest
        HIP_TRY(hipEventSynchronize(f.done));
        f.pending = false;
        if (const rt_status st = judge_frame(sc, f)) return st;
    }
    if (!f.host) {
        HIP_TRY(hipHostMalloc((void **)&f.host, 3 * kMaxPasses * sizeof(uint32_t), hipHostMallocDefault));
        HIP_TRY(hipEventCreate(&f.start));
        HIP_TRY(hipEventCreate(&f.done));
    }
    *out = &f;
    return RT_OK;
}
// Rows of the sample slab start on 128-byte lines (32 slots x 12 B = 3 lines) — except for passes shorter than that, whose rows are
// only padded to the 16 bytes the accumulate kernels' row reads need (a 4K frame at 1 spp: 0.4 GB instead of 3.2 GB)
uint32_t slab_pitch_of(int pass) { return pass < 32 ? (uint32_t)((pass + 3) & ~3) : (uint32_t)((pass + 31) & ~31); }
// The passes of a call (rt_accel.h, plan_passes) and a slab that holds one of them: three floats per (local pixel, slot)
// (slabs: how many of them lie side by side — rt_render_lit_split's two: the budget, given or derived, is shared between them)
rt_status reserve_slab(rt_scene *sc, uint32_t num_pixels, int32_t spp, hipStream_t stream, rtaccel::PassPlan &plan, uint32_t slabs = 1) {
    const rt_config &cfg = sc->cfg;
    const uint64_t budget = cfg.workspace_bytes ? (cfg.workspace_bytes / slabs ? cfg.workspace_bytes / slabs : 1) : 0;
    plan = rtaccel::plan_passes(num_pixels, spp, budget, sc->device_bytes / slabs, cfg.pass_spp);
    if (plan.passes < 1) return fail(RT_ERR_UNSUPPORTED, "image too large for the work index arithmetic");
    if (plan.passes > kMaxPasses) return fail(RT_ERR_UNSUPPORTED, "more than 1024 passes (samples_per_pixel above 65536, or above 64512 at 2^24 pixels)");
    int pass_size = plan.pass_size;
    size_t need = (size_t)num_pixels * (size_t)slab_pitch_of(pass_size) * 3 * slabs;
    if (sc->slab_floats < need) {
        HIP_TRY(hipStreamSynchronize(stream));
        (void)hipFree(sc->slab);
        sc->slab = nullptr;
        sc->slab_floats = 0;
        for (;;) {      // a device short of memory gets shorter passes, not an error
            const hipError_t e = hipMalloc((void **)&sc->slab, need * sizeof(float));
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            if (e != hipErrorOutOfMemory || pass_size <= 64) HIP_TRY(e);
            pass_size = pass_size / 2 < 64 ? 64 : pass_size / 2;
            plan = rtaccel::PassPlan::uniform(spp, pass_size);      // (shorter than before: within the bound too)
            need = (size_t)num_pixels * (size_t)slab_pitch_of(pass_size) * 3 * slabs;
        }
        sc->slab_floats = need;
    }
    return RT_OK;
}
// Room for the per-pixel candidate lists of the primary-visibility pass (64 bytes per pixel) + 16 bytes per pixel for the fetch
// order's table (a row of rtk::kOrderRowWords words per pixel) and 12 per 256 pixels for its counting sort (order_* kernels).
// A device short of memory renders without the pass rather than not at all: prim = false.
rt_status reserve_view_lists(rt_scene *sc, uint32_t num_pixels, hipStream_t stream, bool &prim) {
    if (!prim || sc->cand_pixels >= (size_t)num_pixels) return RT_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    (void)hipFree(sc->cand);
    sc->cand = nullptr;
    sc->cand_pixels = 0;
    sc->cand_key.valid = false;
    const size_t cand_words = (size_t)num_pixels * (rtk::kCandWords + rtk::kOrderRowWords) + 3 * (((size_t)num_pixels + rtk::kOrderBlock - 1) / rtk::kOrderBlock);
    if (hipMalloc((void **)&sc->cand, cand_words * sizeof(uint32_t)) == hipSuccess) {
        sc->cand_pixels = (size_t)num_pixels;
    } else {
        (void)hipGetLastError();
        sc->cand = nullptr;
        prim = false;
    }
    return RT_OK;
}
// P's view of them: the lists, the fetch order's table behind them (16-byte rows on a 64-byte boundary: kCandWords words per pixel before
// it) and, behind the table, the sort's counts with the count of pixels with a list (counts[2 * blocks] after the scan)
void bind_view_lists(const rt_scene *sc, rtk::KParams &P, uint32_t num_pixels, bool prim) {
    P.cand = prim ? sc->cand : nullptr;
    P.order = prim ? sc->cand + sc->cand_pixels * rtk::kCandWords : nullptr;
    P.traced_pixels = prim ? P.order + sc->cand_pixels * rtk::kOrderRowWords + 2 * (((size_t)num_pixels + rtk::kOrderBlock - 1) / rtk::kOrderBlock) : nullptr;
}
// The candidate lists and the fetch order made from them, for this view on this stream — unless the handle holds them already
// (rt_config.reuse_view_lists): the same camera, image, shard and tree on the same stream
rt_status make_view_lists(rt_scene *sc, const rt_camera_data *cam, const rtk::KParams &P, uint32_t num_pixels, hipStream_t stream) {
    rt_scene::CandKey key{};
    std::memcpy(key.view + 0, cam->origin.e, 12); std::memcpy(key.view + 3, cam->pixel00_loc.e, 12);
    std::memcpy(key.view + 6, cam->pixel_delta_u.e, 12); std::memcpy(key.view + 9, cam->pixel_delta_v.e, 12);
    const int32_t dims[9] = {P.width, P.height, P.local_rows, P.band_rows, P.num_parts, P.part, P.row_w, P.tile_x0, P.tile_y0};
    std::memcpy(key.dims, dims, sizeof(dims));
    key.repacks = sc->repacks; key.stream = stream; key.valid = true;
    const bool cand_cached = sc->cfg.reuse_view_lists >= 0 && sc->cand_key.valid && std::memcmp(key.view, sc->cand_key.view, sizeof(key.view)) == 0 &&
                             std::memcmp(key.dims, sc->cand_key.dims, sizeof(key.dims)) == 0 && key.repacks == sc->cand_key.repacks && key.stream == sc->cand_key.stream;
    if (cand_cached) return RT_OK;
    sc->cand_key.valid = false;          // (valid again once the launches below are queued)
    const double coord_max = rtbeam::coord_bound(cam->origin.e, cam->pixel00_loc.e, cam->pixel_delta_u.e, cam->pixel_delta_v.e, cam->image_width, cam->image_height);
    hipLaunchKernelGGL(rtk::cand_kernel, dim3((num_pixels + 255u) / 256u), dim3(256), 0, stream, P, sc->cand, coord_max);
    HIP_TRY(hipGetLastError());
    // the order the trace kernel fetches the pixels in: expensive ones first (rt_primary.hip.inc)
    uint32_t *order = sc->cand + sc->cand_pixels * rtk::kCandWords, *counts = order + sc->cand_pixels * rtk::kOrderRowWords;
    const uint32_t order_blocks = (num_pixels + (uint32_t)rtk::kOrderBlock - 1u) / (uint32_t)rtk::kOrderBlock;
    hipLaunchKernelGGL(rtk::order_count_kernel, dim3(order_blocks), dim3(rtk::kOrderBlock), 0, stream, (const uint32_t *)sc->cand, num_pixels, order_blocks, counts);
    hipLaunchKernelGGL(rtk::order_scan_kernel, dim3(1), dim3(1024), 0, stream, counts, 3u * order_blocks);
    hipLaunchKernelGGL(rtk::order_scatter_kernel, dim3(order_blocks), dim3(rtk::kOrderBlock), 0, stream, P, (const uint32_t *)sc->cand, num_pixels, order_blocks,
                       (const uint32_t *)counts, order);
    HIP_TRY(hipGetLastError());
    sc->cand_key = key;
    return RT_OK;
}
// the primary-visibility pass of one pass of samples: (hit distance, primitive, seed) into each sample's slot of the slab
void launch_primary(const rt_scene *sc, const rtk::KParams &P, uint32_t num_pixels, hipStream_t stream) {
    int pgrid = sc->num_cus * 8;                            // 256-thread workgroups: 8 waves per SIMD
    const bool by_pixel = P.pass_count >= RTP_BY_PIXEL_MIN;  // a wave per pixel once a pixel (nearly) fills it twice
    const uint32_t units = by_pixel ? (num_pixels + 3u) / 4u : (P.total_work + 255u) / 256u;
    if ((uint32_t)pgrid > units) pgrid = (int)units;
    if (by_pixel) {
        if (P.num_planes > 0) hipLaunchKernelGGL(rtk::primary_pixel_kernel<true>, dim3(pgrid), dim3(256), 0, stream, P);
        else hipLaunchKernelGGL(rtk::primary_pixel_kernel<false>, dim3(pgrid), dim3(256), 0, stream, P);
    } else if (P.num_planes > 0) hipLaunchKernelGGL(rtk::primary_kernel<true>, dim3(pgrid), dim3(256), 0, stream, P);
    else hipLaunchKernelGGL(rtk::primary_kernel<false>, dim3(pgrid), dim3(256), 0, stream, P);
}
// ---- rt_render's steps: the walk and its launch shapes (plan_launch), the buffers they need, the passes, the record of the frame

// The margins were sized for ray origins within origin_radius of origin_center, and those of the small spheres for origins within
// sqrt(d0_sq) of their cluster (NaN coordinates are within nothing)
bool camera_within(const rt_camera_data *cam, const float c[3], double radius_sq) {
    const double dx = (double)cam->origin.e[0] - c[0], dy = (double)cam->origin.e[1] - c[1], dz = (double)cam->origin.e[2] - c[2];
    return dx * dx + dy * dy + dz * dz <= radius_sq;
}
// … and both with room to spare where the small spheres' margins matter, as the primary-visibility pass needs them: it takes
// camera rays from the guarded walk's tree, so the far-origin test must never fire for one (the device compares in float: a hair of
// slack)
bool camera_inside_margins(const rt_scene *sc, const rt_camera_data *cam) {
    return camera_within(cam, sc->guard.origin_center, (double)sc->guard.origin_radius * sc->guard.origin_radius) &&
           !(sc->guard.num_small > 0 && !camera_within(cam, sc->guard.center, (double)sc->guard.d0_sq * (1.0 - 1e-5)));
}
// The guarded walk is the handle's choice for this scene: eligible, not ruled out by rt_config, wanted at this size, not paused
bool guarded_chosen(const rt_scene *sc, const rtk::KParams &P) {
    const rt_config &cfg = sc->cfg;
    return sc->guard.ok && cfg.traversal != RT_TRAVERSAL_EXACT && P.root >= 0 && guarded_wanted(cfg, (int64_t)P.num_spheres + P.num_planes) &&
           !(sc->guard_paused && !cfg.guard_keep);
}

// Step 2 of rt_render: the exact or the guarded walk, and the guarded walk's tree re-packed for a camera beyond its margins (which
// changes the handle's tables: P is filled again)
rt_status choose_traversal(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const Tile *tile, hipStream_t stream, rtk::KParams &P,
                           bool &guarded, bool &exploring) {
    const rt_config &cfg = sc->cfg;
    // only for eligible scenes (and, below, for cameras within the margins and tables that leave room for a useful stack)
    guarded = guarded_chosen(sc, P);
    // (AUTO only: one exact frame to time the guarded walk against — judge_frame)
    exploring = guarded && sc->explore_exact && cfg.traversal == RT_TRAVERSAL_AUTO && !cfg.guard_keep;
    if (exploring) guarded = false;
    if (!guarded) return RT_OK;
    // A camera outside the margins gets the tree re-packed with margins for where it is (once per growth of the reach; the exact
    // walk's tables do not change).
    const bool far_cam = !camera_within(cam, sc->guard.origin_center, (double)sc->guard.origin_radius * sc->guard.origin_radius) ||
                         (sc->guard.num_small > 0 && !camera_within(cam, sc->guard.center, (double)sc->guard.d0_sq));
    if (far_cam && !sc->repack_refused && std::isfinite(cam->origin.e[0]) && std::isfinite(cam->origin.e[1]) && std::isfinite(cam->origin.e[2]) &&
        cfg.guard_repack) {
        rt_status st = repack_for_camera(sc, cam->origin.e, stream);
        if (st != RT_OK) return st;
        float *fb = P.fb;
        if ((st = fill_params(sc, cam, shard, P, tile)) != RT_OK) return st;       // table pointers and guard parameters changed
        P.fb = fb;
    }
    if (!camera_within(cam, sc->guard.origin_center, (double)sc->guard.origin_radius * sc->guard.origin_radius)) guarded = false;
    if (sc->repack_refused && sc->guard.num_small > 0 && !camera_within(cam, sc->guard.center, (double)sc->guard.d0_sq)) guarded = false;
    return RT_OK;
}

// Step 2 of a lens frame (rt_render_lens): the handle's walk as it stands — no re-pack, no exploring frame, nothing of the handle
// changes — and the guarded walk only where EVERY ray origin the camera can make lies within the reach its margins were sized for.
// A lens point is O + R (lx uh + ly vh) with unit uh, vh and lx^2 + ly^2 < 1: its distance from the pose's origin is below
// R (|lx| + |ly|) < sqrt(2) R whatever the angle between du and dv (a caller's skewed camera, or an interpolated pose).  The pose's
// origin lies on the segment between the two ends' origins, and the reach is a ball: both ends checked with the radius reduced by
// sqrt(2) R cover every pose between them (a hair of slack for the rounding of the interpolated pose and of the lens point).
bool lens_guarded(const rt_scene *sc, const rtk::KParams &P, const rtk::LensCam &C) {
    if (!guarded_chosen(sc, P)) return false;
    auto within = [&](int end, const float c[3], double reach) {
        reach -= std::sqrt(2.0) * (double)C.radius;
        if (!(reach > 0.0)) return false;
        const double dx = (double)C.o[end][0] - c[0], dy = (double)C.o[end][1] - c[1], dz = (double)C.o[end][2] - c[2];
        return dx * dx + dy * dy + dz * dz <= reach * reach * (1.0 - 1e-5);
    };
    for (int end = 0; end <= C.motion; ++end) {
        if (!within(end, sc->guard.origin_center, (double)sc->guard.origin_radius)) return false;
        if (sc->guard.num_small > 0 && !within(end, sc->guard.center, std::sqrt((double)sc->guard.d0_sq))) return false;
    }
    return true;
}

// Launch shape of one walk: tables in LDS or not, LDS bytes per workgroup, workgroups per CU, stack rows per lane, treelet records
struct Shape { bool in_lds; uint32_t lds_bytes; int wgs_per_cu; int32_t stack_levels; int32_t num_top; };
enum class Walk { Exact, ExactSimple, Guarded };
struct LaunchPlan {
    Walk walk = Walk::Exact;
    Shape exact{}, exact_s{}, fast{};       // the exact walk, its sphere-only build, the guarded walk
    bool wide = false;                      // guarded walk on the 4-wide nodes (step_wide_par)
    bool dyn = false;                       // guarded walk with distance-aware margins
    bool simple = false;                    // guarded walk, sphere-only build
    bool prim = false;                      // primary-visibility pass before the trace launch
    bool dark = false;                      // the sphere-only octant walk behind the primary pass, in a scene without emitters: its build without a radiance accumulator
    bool overlap = false;                   // exact re-walk on the handle's second stream
    bool resume = false;                    // resume table for flagged samples
    uint32_t flag_chunk_words = 0;          // LDS words per wave for its chunk of the flagged-sample list (rt_kernel.hip.inc, flag_collect): 2, or 0
    int32_t k_inner = 0, k_shade = 0;       // vote thresholds of the trace launch
    bool guarded() const { return walk == Walk::Guarded; }
    bool sphere_only() const { return walk == Walk::ExactSimple || (walk == Walk::Guarded && simple); }
    uint32_t block() const { return sphere_only() ? (uint32_t)rtk::kSimpleBlock : (uint32_t)rtk::kBlock; }      // threads per workgroup of the trace launch
    const Shape &trace_shape() const { return walk == Walk::Guarded ? fast : (walk == Walk::ExactSimple ? exact_s : exact); }
};

// Step 3 of rt_render: the launch shapes of the walks, from the handle's tables, its config and P alone (no HIP call, nothing
// of the handle changes).  `guarded`: what choose_traversal decided; the plan may still fall back to the exact walk.
// pinhole = false (lens frames): neither sphere-only build (no lens instantiation of them: the general builds of the same walks) nor
// the primary-visibility pass.
LaunchPlan plan_launch(const rt_scene *sc, const rt_camera_data *cam, const rtk::KParams &P, bool guarded, bool pinhole = true) {
    const rt_config &cfg = sc->cfg;
    LaunchPlan L;
    const uint32_t waves = rtk::kBlock / rtk::kWave;
    const uint32_t pool_bytes = waves * 8u;                  // per-wave reserved work range
    const uint64_t prim_f4 = (uint64_t)P.num_spheres + (uint64_t)P.num_planes * 5 + (uint64_t)P.num_materials * RTP_LDS_MAT_ROWS +      // LDS keeps the first RTP_LDS_MAT_ROWS of the 3 material rows
                             ((uint64_t)P.num_spheres + 3) / 4;

    // ---- exact (threaded) walk
    Shape &exact = L.exact;
    {
        const uint64_t scene_bytes = (((uint64_t)P.num_tnodes + 1) * 2 + prim_f4) * 16;
        exact.in_lds = cfg.scene_in_lds && scene_bytes + pool_bytes <= kLdsLimit;
        // big scene: the top of the tree (explicit-link records [0, num_top)) is staged in LDS
        exact.num_top = (exact.in_lds || !cfg.lds_treelet) ? 0 : P.num_top;
        const uint64_t per_wg = exact.in_lds ? scene_bytes + pool_bytes : pool_bytes + (uint64_t)exact.num_top * 32u;
        // workgroups per CU: what the register budget admits (RTP_MIN_WAVES waves per SIMD), unless that
        // many LDS-resident scene copies do not fit next to each other
        exact.wgs_per_cu = cfg.workgroups_per_cu;
        if (exact.wgs_per_cu <= 0) {
            exact.wgs_per_cu = RTP_MIN_WAVES * 256 / rtk::kBlock;
            while (exact.wgs_per_cu > 1 && (uint64_t)exact.wgs_per_cu * per_wg > kLdsLimit) --exact.wgs_per_cu;
        }
        if (exact.wgs_per_cu < 1) exact.wgs_per_cu = 1;
        exact.lds_bytes = (uint32_t)per_wg;
    }
    // The sphere-only build of the exact walk (render_kernel<true, true, …, kSimple>: no plane, texture or absorption code, material
    // rows from global memory, node records in the 64-byte octant layout of step_threaded_oct; 64 registers, 1024-thread
    // workgroups, 8 waves per SIMD) for WHOLE passes of scenes that have none of those: S-rtiow 5 210 against 4 855 Msamples/s.
    // The re-walk of a list keeps the general build: it is a few long paths, and those run slower in the tighter kernel
    // (headline frame: re-walk 3.1 ms instead of 1.7).
    bool exact_simple = exact.in_lds && cfg.sphere_only_kernel >= 0 && P.num_planes == 0 && sc->tex_data == nullptr && !sc->absorbing_glass &&
                        cfg.workgroups_per_cu == 0 && P.num_spheres > 0 && pinhole;
    if (exact_simple) {
        const uint64_t simple_bytes = (((uint64_t)P.num_tnodes + 1) * 4 + (uint64_t)P.num_spheres + ((uint64_t)P.num_spheres + 3) / 4) * 16;
        const uint64_t simple_pool = (uint64_t)(rtk::kSimpleBlock / rtk::kWave) * 8u + 16u * rtk::kConstRows;      // work ranges + the constants block
        L.exact_s.in_lds = true;
        L.exact_s.wgs_per_cu = rtk::kSimpleWaves * 256 / rtk::kSimpleBlock;
        L.exact_s.lds_bytes = (uint32_t)(simple_bytes + simple_pool);
        if ((uint64_t)L.exact_s.wgs_per_cu * L.exact_s.lds_bytes > kLdsLimit) exact_simple = false;
    }

    // ---- guarded near-first walk: only where its tables leave room for a useful stack
    // 4-wide nodes (where the scene has them: a host-built tree with at least one inner node) for scenes with distance-aware
    // margins (step_wide_par: half the dependent record loads of the pair walk and, with the growth in parametric form, fewer
    // instructions per ray — configs[4] +1.7 %).  (step_wide_par tells an empty child slot by its box — the finite inverted
    // (65504, -65504) of the binary16 table — which holds while the growth stays below 65504: it never exceeds dyn_k x (twice the
    // radius every ray origin lies within)^2)
    const bool dyn_scene = sc->guard.dyn_k > 0.0f;          // distance-aware margins (big or widely spread scenes)
    const double growth_max = (double)sc->guard.dyn_k * 4.0 * (double)sc->guard.origin_radius * (double)sc->guard.origin_radius;
    bool wide = sc->whnodes != nullptr && sc->num_wide > 0 && cfg.wide_nodes == 0 && dyn_scene && growth_max < 16384.0;
    bool simple = false;
    Shape &fast = L.fast;
    if (guarded) {
        uint32_t gblock = (uint32_t)rtk::kBlock;           // threads per workgroup of the guarded pass
        int gwgs_per_cu = RTP_MIN_WAVES * 256 / (int)gblock;
        // fp32 records when LDS-resident: 5 float4 per pair node in the octant layout the kernel stages (rt_kernel.hip.inc, step_octant)
        // + the guarded kernels' constants block
        uint64_t table_bytes = ((uint64_t)P.num_internal * 5 + prim_f4) * 16 + kGuardBlockBytes;
        const int32_t deepest = wide ? 3 * sc->wide_depth : sc->tree_depth;          // a wide node leaves up to three children waiting
        const int32_t want = deepest + 1 > 2 ? deepest + 1 : 2;       // never overflows
        uint32_t per_level = gblock * 4u;
        uint32_t pool_extra = 0;       // (the sphere-only builds have four more waves' work ranges than pool_bytes counts)
        // the sphere-only build of the octant walk (render_kernel<…, kSimple>: 1024-thread workgroups, 8 waves per SIMD): no planes,
        // no textures, leaf boxes recomputed from the spheres; its LDS holds no material rows (all three come from global memory),
        // which pays for the wider stack rows of 1024 lanes
        const bool plain = cfg.sphere_only_kernel >= 0 && P.num_planes == 0 && sc->tex_data == nullptr && P.leaf_boxes == nullptr &&
                           cfg.workgroups_per_cu == 0 && !sc->absorbing_glass && pinhole;
        if (plain && !dyn_scene && cfg.scene_in_lds != 0) {
            const uint64_t simple_bytes = ((uint64_t)P.num_internal * 5 + (uint64_t)P.num_spheres + ((uint64_t)P.num_spheres + 3) / 4) * 16;
            const uint64_t budget = kLdsLimit / 2;
            const int64_t fit = simple_bytes + pool_bytes + 256 < budget ? (int64_t)((budget - simple_bytes - pool_bytes - 256) / ((uint64_t)rtk::kSimpleBlock * 4u)) : 0;
            if (fit >= 6 || fit >= want) {          // at least the sentinel + 5 levels: below that the re-walk launch eats the gain
                simple = true;
                gblock = (uint32_t)rtk::kSimpleBlock;
                gwgs_per_cu = rtk::kSimpleWaves * 256 / rtk::kSimpleBlock;
                table_bytes = simple_bytes + ((uint64_t)(rtk::kSimpleBlock / rtk::kWave) * 8u - pool_bytes) + kGuardBlockBytes;      // + the four extra waves' work ranges + the constants block
                per_level = gblock * 4u;
            }
        }
        // … and of the walk through L1 / L2 for scenes with distance-aware margins (step_pair_par on pair nodes: the 4-wide step does
        // not fit 64 registers): sphere-only scenes beyond what LDS holds — S-rtiow x 785 … 99 857 spheres: +7 … +10 % over the general
        // build on 4-wide nodes (8.1 / 7.7 / 6.7 / 3.9 against 7.5 / 7.2 / 6.2 / 3.6 Gsamples/s; tools/size_sweep.py)
        if (plain && dyn_scene) {
            simple = true;
            wide = false;
            gblock = (uint32_t)rtk::kSimpleBlock;
            gwgs_per_cu = rtk::kSimpleWaves * 256 / rtk::kSimpleBlock;
            per_level = gblock * 4u;
            pool_extra = (uint32_t)(rtk::kSimpleBlock / rtk::kWave) * 8u - pool_bytes;
        }
        // tables in LDS when they leave room for a useful stack at full occupancy; else they are read
        // through L1/L2 and LDS holds only the stacks
        auto levels_for = [&](uint64_t scene_bytes, int wgs_per_cu) -> int32_t {
            const uint64_t budget = kLdsLimit / (uint64_t)wgs_per_cu;
            if (scene_bytes + pool_bytes >= budget) return 0;
            const int64_t fit = (int64_t)((budget - scene_bytes - pool_bytes) / per_level);
            return (int32_t)(fit < want ? fit : want);
        };
        const int32_t min_levels = want < 4 ? want : 4;          // a shorter stack flags too many rays
        fast.wgs_per_cu = gwgs_per_cu;
        // Scenes with distance-aware margins always take their records through L1 / L2 (step_pair_par: 32-byte binary16 records, a
        // full stack, two workgroups per CU whatever the size of the tree).  The LDS-resident form of that walk lost on every
        // random scene it was tried on — tables of a thousand nodes leave room for one workgroup per CU or for a stack of four,
        // and the rays a short stack hands to the exact walk cost more than L1 does: tools/dyn_probe.py, docs/LOG.md round 4.
        fast.in_lds = cfg.scene_in_lds != 0 && !dyn_scene;
        if (fast.in_lds) {
            fast.stack_levels = levels_for(table_bytes, fast.wgs_per_cu);
            while (fast.wgs_per_cu > 1 && fast.stack_levels < min_levels) fast.stack_levels = levels_for(table_bytes, --fast.wgs_per_cu);
            if (fast.stack_levels < min_levels) fast.in_lds = false;
        }
        // (step_pair_par / step_wide_par, the walks of scenes with distance-aware margins, keep a sentinel in level 0 — one level
        // more for the same twelve entries — and two rows of per-ray values behind the stack)
        const int32_t extra_rows = dyn_scene ? 2 : 0;
        if (!fast.in_lds) {
            // tables through L1/L2: a 12-entry stack per lane (deeper ones are rare enough to flag), the rest of
            // the workgroup's LDS share holds the top of the tree
            fast.wgs_per_cu = gwgs_per_cu;
            const uint64_t budget = kLdsLimit / (uint64_t)fast.wgs_per_cu;
            const int64_t fit = budget > pool_bytes + pool_extra + kGuardBlockBytes ? (int64_t)((budget - pool_bytes - pool_extra - kGuardBlockBytes) / per_level) : 0;
            // (the 4-wide walk leaves up to three children of a node waiting, and LDS holds nothing but the stacks: twenty entries)
            const int32_t cap = (dyn_scene ? (wide ? 21 : 13) : 12) + extra_rows;
            fast.stack_levels = (int32_t)std::min<int64_t>(std::min<int64_t>(fit, want + extra_rows), cap);
        }
        if (const int forced = cfg.stack_levels) fast.stack_levels = forced + extra_rows < fast.stack_levels ? forced + extra_rows : fast.stack_levels;
        if (fast.stack_levels - extra_rows < (want < 2 ? want : 2)) guarded = false;
        // (the walks of scenes with distance-aware margins read every record through L1 / L2: no treelet)
        if (!fast.in_lds && cfg.lds_treelet && !dyn_scene) {
            const uint64_t budget = kLdsLimit / (uint64_t)fast.wgs_per_cu;
            const uint64_t used = pool_bytes + (uint64_t)fast.stack_levels * per_level + kGuardBlockBytes;
            const int64_t fit = budget > used ? (int64_t)((budget - used) / 32) : 0;
            fast.num_top = (int32_t)(fit < sc->num_top_pairs ? fit : sc->num_top_pairs);
        }
        if ((!fast.in_lds && !dyn_scene) || fast.wgs_per_cu != gwgs_per_cu) simple = false;      // (cannot happen after the fit test above; the general kernel is always right)
        fast.lds_bytes = (uint32_t)((fast.in_lds ? table_bytes : (uint64_t)fast.num_top * 32 + pool_extra + kGuardBlockBytes) + pool_bytes +
                                    (uint64_t)fast.stack_levels * per_level);
        if (const int w = cfg.workgroups_per_cu) { if ((uint64_t)w * fast.lds_bytes <= kLdsLimit) fast.wgs_per_cu = w; }
        L.flag_chunk_words = 2u;          // (the wave's chunk of the flagged-sample list: inside kGuardBlockBytes)
    }
    L.walk = guarded ? Walk::Guarded : (exact_simple ? Walk::ExactSimple : Walk::Exact);
    L.wide = guarded && wide;
    L.simple = simple;
    L.dyn = guarded && dyn_scene;
    // (not with a capped flag list or an unproven margin: a list that overflowed makes the re-walk rewrite EVERY slab entry
    // while the other stream sums the rows of unflagged pixels — harmless only where both walks give the same bits)
    L.overlap = guarded && cfg.overlap_rework >= 0 && cfg.flag_capacity == 0 && !gamma_unproven(cfg);
    // Primary visibility without a walk (rt_primary.hip.inc): the pair-node walks of render_kernel — the LDS-resident octant walk
    // with static margins, and the walk with distance-aware margins (through L1/L2) — and a camera inside the margins
    L.prim = pinhole && guarded && (L.dyn || fast.in_lds) && cfg.primary_visibility >= 0 && sc->nodes != nullptr && P.max_depth < rtk::kMaxPrimDepth &&
             camera_inside_margins(sc, cam);
    // … and behind it, for the sphere-only octant walk of a scene in which nothing emits, the build that carries no radiance
    // (rt_kernel.hip.inc, kDark; else render_emit_kernel.  rt_render, rt_render_tile and rt_render_samples: render_impl drops it for
    // the call that keeps its kernel)
    L.dark = L.prim && L.simple && fast.in_lds && !L.dyn && sc->dark && cfg.dark_kernel >= 0;
    // resume table: not for paths longer than the depth field
    L.resume = guarded && cfg.resume_flagged >= 0 && P.max_depth < rtk::kMaxPrimDepth;
    // vote thresholds: the octant walk's (its pair steps are cheaper, so a block of them is worth starting for fewer idle lanes
    // and a shade step is worth waiting for a few more): re-swept after step_octant, +1.0 %.  Scenes with distance-aware margins
    // (records through L1/L2, step_pair_par / step_wide_par): a block of steps costs memory round trips on top of its
    // instructions — worth starting only for a nearly full wave (S-100k, swept 16-52 x 44-56: +4 %)
    const int32_t k_inner = guarded && fast.in_lds ? 32 : (L.dyn ? 48 : 24), k_shade = guarded && (fast.in_lds || L.dyn) ? 52 : 48;
    L.k_inner = cfg.k_inner > 0 ? cfg.k_inner : k_inner;
    L.k_shade = cfg.k_shade > 0 ? cfg.k_shade : k_shade;
    return L;
}

// a handle buffer of at least `need` elements (its contents are not kept)
template <class T>
rt_status grow(T *&buf, size_t &have, size_t need, hipStream_t stream) {
    if (have >= need) return RT_OK;
    HIP_TRY(hipStreamSynchronize(stream));          // (the old one may still be in use on this stream)
    (void)hipFree(buf);
    buf = nullptr;
    have = 0;
    HIP_TRY(hipMalloc((void **)&buf, need * sizeof(T)));
    have = need;
    return RT_OK;
}
// Step 4 of rt_render: the handle's buffers for this call, grown where they are short.  A device short of memory for the view lists
// renders without the primary-visibility pass (plan.prim = false).
rt_status reserve_buffers(rt_scene *sc, const rtk::KParams &P, uint32_t num_pixels, hipStream_t stream, LaunchPlan &plan, rtaccel::PassPlan &passes) {
    const rt_config &cfg = sc->cfg;
    if (const rt_status st = reserve_slab(sc, num_pixels, P.spp, stream, passes)) return st;
    if (plan.guarded()) {
        // flagged-sample list: a quarter of a pass's samples (a fuller list means "re-walk everything")
        const size_t cap = (size_t)num_pixels * (size_t)passes.pass_size / 4 + 65536;
        if (const rt_status st = grow(sc->flag_list, sc->flag_cap, cap, stream)) return st;
        if (cfg.overlap_rework >= 0 && sc->dirty_cap < (size_t)num_pixels) {
            HIP_TRY(hipStreamSynchronize(stream));
            (void)hipFree(sc->dirty); (void)hipFree(sc->dirty_list);
            sc->dirty = sc->dirty_list = nullptr;
            sc->dirty_cap = 0;
            HIP_TRY(hipMalloc((void **)&sc->dirty, (size_t)num_pixels * sizeof(uint32_t)));
            HIP_TRY(hipMalloc((void **)&sc->dirty_list, (size_t)num_pixels * sizeof(uint32_t)));
            sc->dirty_cap = (size_t)num_pixels;
        }
        if (cfg.overlap_rework >= 0 && !sc->aux_stream) {
            HIP_TRY(hipStreamCreateWithFlags(&sc->aux_stream, hipStreamNonBlocking));
            HIP_TRY(hipStreamCreateWithFlags(&sc->list_stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&sc->ev_listed, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&sc->ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&sc->ev_join, hipEventDisableTiming));
        }
    }
    // resume table (made with the first guarded frame that uses it; a device short of memory renders without it)
    if (plan.resume && sc->resume_tag == nullptr) {
        if (hipMalloc((void **)&sc->resume_tag, sizeof(uint32_t) << kResumeBits) != hipSuccess ||
            hipMalloc((void **)&sc->resume_state, (size_t)64 << kResumeBits) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(sc->resume_tag); (void)hipFree(sc->resume_state);
            sc->resume_tag = nullptr; sc->resume_state = nullptr;
        }
    }
    return reserve_view_lists(sc, num_pixels, stream, plan.prim);
}

// The trace kernel of a plan (render_kernel<kLds, kThreaded, kDyn, kWide, kSimple, kPrim>)
const void *trace_kernel(const LaunchPlan &L) {
    using rtk::render_kernel;
    if (L.walk == Walk::ExactSimple) return (const void *)render_kernel<true, true, false, false, true>;
    if (L.walk == Walk::Exact) return L.exact.in_lds ? (const void *)render_kernel<true, true> : (const void *)render_kernel<false, true>;
    if (L.wide)          // distance-aware margins on 4-wide nodes (step_wide_par)
        return L.prim ? (const void *)render_kernel<false, false, true, true, false, true> : (const void *)render_kernel<false, false, true, true>;
    if (L.dyn && L.simple)          // sphere-only scenes beyond what LDS holds: step_pair_par at 64 registers, 8 waves per SIMD
        return L.prim ? (const void *)render_kernel<false, false, true, false, true, true> : (const void *)render_kernel<false, false, true, false, true>;
    if (L.dyn) return L.prim ? (const void *)render_kernel<false, false, true, false, false, true> : (const void *)render_kernel<false, false, true>;
    if (L.fast.in_lds && L.simple && L.prim)        // behind the primary pass: the build for scenes without emitters, or the one that carries radiance
        return L.dark ? (const void *)render_kernel<true, false, false, false, true, true> : (const void *)rtk::render_emit_kernel;
    if (L.fast.in_lds && L.simple) return (const void *)render_kernel<true, false, false, false, true>;
    if (L.fast.in_lds) return L.prim ? (const void *)render_kernel<true, false, false, false, false, true> : (const void *)render_kernel<true, false>;
    return (const void *)render_kernel<false, false>;
}

// … and of a lens frame (render_lens_kernel<kLds, kThreaded, kDyn, kWide>: the general builds only, plan_launch with pinhole = false)
const void *lens_trace_kernel(const LaunchPlan &L) {
    using rtk::render_lens_kernel;
    if (L.walk != Walk::Guarded) return L.exact.in_lds ? (const void *)render_lens_kernel<true, true> : (const void *)render_lens_kernel<false, true>;
    if (L.wide) return (const void *)render_lens_kernel<false, false, true, true>;
    if (L.dyn) return (const void *)render_lens_kernel<false, false, true>;
    if (L.fast.in_lds) return (const void *)render_lens_kernel<true, false>;
    return (const void *)render_lens_kernel<false, false>;
}

// (second: the second kernel argument — render_lens_kernel's LensCam, a lit trace kernel's light table; null for render_kernel.
// third: lit_render_kernel's LensCam behind its light; null for every other kernel.  fourth: lit_split_render_kernel's second slab behind
// that — the address of the pointer; null for every other kernel)
hipError_t launch(const void *kernel, uint32_t block, int grid, uint32_t lds, hipStream_t stream, const rtk::KParams &KP, const void *second = nullptr,
                  const void *third = nullptr, const void *fourth = nullptr) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    void *args[] = {(void *)&KP};
    void *more_args[] = {(void *)&KP, (void *)second, (void *)third, (void *)fourth};
    e = hipLaunchKernel(kernel, dim3(grid), dim3(block), second ? more_args : args, lds, stream);
    const hipError_t last = hipGetLastError();
    return e != hipSuccess ? e : last;
}

// Work indices a wave reserves per atomicAdd on the pass's counter.  6144 waves hammering ONE address with an atomic per 64 samples
// was the bottleneck of the whole kernel (5.05 -> 6.25 Gsamples/s with 512 per atomic); small frames keep at least 16 reservations
// per wave so the tail stays balanced.  Near the end of the pass reservations shrink to remaining / (RTP_TAPER_FACTOR x waves),
// rounded to a power of two: taper_shift.
void reservation(uint32_t total_work, uint64_t waves_total, uint32_t &chunk, uint32_t &taper_shift) {
    uint64_t per = (uint64_t)total_work / (waves_total * 16u * 64u);
    per = per < 1 ? 1 : (per > 16 ? 16 : per);      // 1024 per atomic with 8192 waves: +1 % over 512 (32: the same, 64: the tail shows)
    chunk = (uint32_t)(64u * per);
    taper_shift = 1;
    while (((uint64_t)1 << taper_shift) < RTP_TAPER_FACTOR * waves_total) ++taper_shift;
}

// samples [pass_first, pass_first + pass_count) of every pixel: work index = pixel * pass_count + slot, below the bound of the
// kernels' 32-bit arithmetic.  A call for samples [sample_first, sample_first + spp) shifts every pass by sample_first (checked by
// check_sample_range: below 2^30).
rt_status set_pass(rtk::KParams &P, const rtaccel::PassPlan &passes, int pass, uint32_t num_pixels, int32_t sample_first) {
    P.pass_first = sample_first + passes.first(pass);
    P.pass_count = passes.count(pass);
    P.total_work = num_pixels * (uint32_t)P.pass_count;
    if ((uint64_t)num_pixels * (uint64_t)P.pass_count >= (1ull << 31) - 4096 || !make_magic((uint32_t)P.pass_count, (uint64_t)P.total_work + 64, P.magic_count))
        return fail(RT_ERR_UNSUPPORTED, "image too large for the work index arithmetic");
    return RT_OK;
}

// rt_render_samples / rt_render_aov_samples: samples [sample_first, sample_first + spp) — the kernels carry sample indices as int32
rt_status check_sample_range(const char *what, int32_t sample_first, int32_t spp) {
    if (sample_first < 0) return fail(RT_ERR_INVALID_ARG, std::string(what) + ": sample_first is negative");
    if ((int64_t)sample_first + (int64_t)spp > (int64_t)1 << 30)
        return fail(RT_ERR_UNSUPPORTED, std::string(what) + ": sample_first + samples_per_pixel above 2^30");
    return RT_OK;
}

// ---- what the frame drivers share (render_impl, aov_impl, adaptive_impl, render_light_impl) -----------------------------------------
// What every render-type call checks before it enqueues anything, in the order its errors are reported, and what it sets up: P, the
// stream, the pixel count, *timing zeroed.  missing: the message for a required buffer that is NULL (null: none is); light_device: the
// device of a light that is an object of its own (null: none); late(): the call's own last refusal, after the shared ones and before
// *timing is written.  nothing_to_do(): a shard without rows — the caller returns RT_OK.
struct Frame {
    rtk::KParams P;
    hipStream_t stream = nullptr;
    uint32_t num_pixels = 0;
    bool nothing_to_do() const { return P.local_rows == 0; }
};
template <class Late>
rt_status frame_prologue(const char *what, const rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const Tile *tile, int32_t sample_first,
                         const int *light_device, const char *missing, void *hip_stream, rt_timing *timing, Frame &F, Late late) {
    rt_status st = fill_params(sc, cam, shard, F.P, tile);
    if (st != RT_OK) return st;
    if ((st = check_sample_range(what, sample_first, F.P.spp)) != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    if (light_device && *light_device != sc->device) return fail(RT_ERR_INVALID_ARG, std::string(what) + ": the environment was created on another device than the scene");
    if (missing) return fail(RT_ERR_INVALID_ARG, missing);
    if ((st = timing_check(timing)) != RT_OK) return st;
    F.num_pixels = (uint32_t)F.P.local_rows * (uint32_t)F.P.row_w;
    if ((st = late()) != RT_OK) return st;
    F.stream = (hipStream_t)hip_stream;
    timing_out(rt_timing{}, timing);
    return RT_OK;
}
rt_status nothing_late() { return RT_OK; }
// no samples, or no depth: the reference's loops add nothing — all-zero sums
rt_status blank_frame(float *d_fb_sum, const Frame &F, int32_t sync) {
    HIP_TRY(hipMemsetAsync(d_fb_sum, 0, (size_t)F.num_pixels * 3 * sizeof(float), F.stream));
    if (sync) HIP_TRY(hipStreamSynchronize(F.stream));
    return RT_OK;
}

// P's view of the sample slab (after reserve_slab / reserve_buffers), with rows for passes of pass_size samples
void bind_slab(const rt_scene *sc, rtk::KParams &P, uint32_t num_pixels, int pass_size) {
    P.slab = sc->slab;
    P.num_pixels = num_pixels;
    P.slab_pitch = slab_pitch_of(pass_size);
}
// Workgroups of a trace launch: what fills the device at the shape's occupancy, fewer where spp samples of every pixel do not need them
int grid_for(const rt_scene *sc, const Shape &sh, uint32_t num_pixels, int32_t spp) {
    const uint32_t max_wgs = (uint32_t)(((uint64_t)num_pixels * (spp < 64 ? spp : 64) + rtk::kBlock - 1) / rtk::kBlock);
    int wgs = sc->num_cus * sh.wgs_per_cu;
    if ((uint32_t)wgs > max_wgs) wgs = (int)max_wgs;
    return wgs < 1 ? 1 : wgs;
}
// registers and scratch of a kernel as the loaded code object reports them → rt_timing
void kernel_resources(const void *kernel, uint32_t &vgprs, uint32_t &scratch) {
    hipFuncAttributes attr;
    const bool known = hipFuncGetAttributes(&attr, kernel) == hipSuccess;
    vgprs = known ? (uint32_t)attr.numRegs : 0u;
    scratch = known ? (uint32_t)attr.localSizeBytes : 0u;
}
// … and of the exact re-walk of a list (flagged samples, the rounds of rt_render_adaptive): the exact walk's general build
const void *rewalk_kernel(LaunchPlan L, bool lens = false) {
    L.walk = Walk::Exact;
    return lens ? lens_trace_kernel(L) : trace_kernel(L);
}
// Its parameters: the exact walk's own vote thresholds and treelet, no stack, and a list at the finest granularity, without taper
void set_exact_rewalk(rtk::KParams &R, const rt_config &cfg, const LaunchPlan &plan) {
    R.k_inner = cfg.k_inner > 0 ? cfg.k_inner : 24;
    R.k_shade = cfg.k_shade > 0 ? cfg.k_shade : 48;
    R.stack_levels = 0;
    R.num_top = plan.exact.num_top;
    R.chunk = 64u;
    R.taper_shift = 0;
}
// accumulate_kernel: a pass's slab rows (P.slab, P.pass_count of them per pixel) added to P.fb strictly in sample order.  Which pixels:
struct Acc {
    int32_t first_pass = 0;                                     // the sums start from zero
    uint32_t *dirty = nullptr;                                  // the overlapped re-walk's marks
    const uint32_t *list = nullptr, *list_count = nullptr;      // only these pixels (accumulate_kernel<true>)
    const uint32_t *abandon = nullptr;                          // the pass's abandon word: set, the launch stands down — or,
    uint32_t run_if_abandoned = 0u;                             // … with this, runs only then
    static Acc every_pixel(int pass) { Acc a; a.first_pass = pass == 0 ? 1 : 0; return a; }
    static Acc unmarked(int pass, uint32_t *dirty, const uint32_t *abandon) { Acc a = every_pixel(pass); a.dirty = dirty; a.abandon = abandon; return a; }
    static Acc onto_sums(const uint32_t *list, const uint32_t *count) { Acc a; a.list = list; a.list_count = count; return a; }      // (rt_render_adaptive's rounds)
    static Acc marked(int pass, uint32_t *dirty, const uint32_t *list, const uint32_t *count, const uint32_t *abandon) {
        Acc a = onto_sums(list, count); a.first_pass = pass == 0 ? 1 : 0; a.dirty = dirty; a.abandon = abandon; return a;
    }
    // the third launch of a pass the guarded launch gave up: every pixel, once the re-walk of everything is done
    static Acc abandoned_pass(int pass, const uint32_t *abandon) { Acc a = every_pixel(pass); a.abandon = abandon; a.run_if_abandoned = 1u; return a; }
};
// the accumulate launches' shape: a wave per 64 pixels
dim3 acc_grid(uint32_t num_pixels) { return dim3((num_pixels + 64 * rtk::kAccWaves - 1) / (64 * rtk::kAccWaves)); }
// (a listed launch's pixels have rows: no sky pixel among them — no candidate lists, no background)
void launch_accumulate(hipStream_t stream, const rtk::KParams &P, const Acc &a) {
    if (a.list)
        hipLaunchKernelGGL(rtk::accumulate_kernel<true>, acc_grid(P.num_pixels), dim3(64 * rtk::kAccWaves), 0, stream, P.fb, (const float *)P.slab, P.num_pixels, P.slab_pitch,
                           P.pass_count, a.first_pass, a.dirty, a.list, a.list_count, (const uint32_t *)nullptr, 0u, 0.0f, 0.0f, 0.0f, a.abandon, a.run_if_abandoned);
    else
        hipLaunchKernelGGL(rtk::accumulate_kernel<false>, acc_grid(P.num_pixels), dim3(64 * rtk::kAccWaves), 0, stream, P.fb, (const float *)P.slab, P.num_pixels, P.slab_pitch,
                           P.pass_count, a.first_pass, a.dirty, a.list, a.list_count, (const uint32_t *)P.cand, (uint32_t)rtk::kCandWords, P.bg[0], P.bg[1], P.bg[2],
                           a.abandon, a.run_if_abandoned);
}
// moments_kernel<false> (rt_render_adaptive's min_spp round): the pass's luminance moments of every pixel added to mom (first_pass: from zero)
void launch_moments(hipStream_t stream, float *mom, const rtk::KParams &P, int32_t first_pass) {
    hipLaunchKernelGGL(rtk::moments_kernel<false>, dim3((P.num_pixels + rtk::kAdaptBlock - 1) / rtk::kAdaptBlock), dim3(rtk::kAdaptBlock), 0, stream, mom,
                       (const float *)P.slab, P.num_pixels, P.slab_pitch, P.pass_count, first_pass, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                       (const uint32_t *)P.cand, (uint32_t)rtk::kCandWords, P.bg[0], P.bg[1], P.bg[2]);
}
// per-pass timing events of a family, made on demand
rt_status grow_events(std::vector<hipEvent_t> &events, size_t n) {
    while (events.size() < n) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        events.push_back(e);
    }
    return RT_OK;
}
// What the launch plan of a frame says in an rt_timing
rt_timing plan_timing(const rt_scene *sc, const LaunchPlan &plan, int wgs, int passes, const void *trace) {
    const Shape &shape = plan.trace_shape();
    rt_timing t{};
    t.num_workgroups = (uint32_t)wgs;
    t.workgroup_size = plan.block();
    t.lds_bytes = shape.lds_bytes;
    t.scene_in_lds = shape.in_lds ? 1u : 0u;
    t.trace_launches = (uint32_t)passes;
    t.guarded = plan.guarded() ? 1u : 0u;
    t.guard_unproven = (plan.guarded() && gamma_unproven(sc->cfg)) ? 1u : 0u;
    t.kernel = RT_KERNEL_MEGA;
    t.guard_dynamic = plan.dyn ? 1u : 0u;
    t.front_primitives = plan.guarded() ? (uint32_t)sc->guard.num_front : 0u;
    t.wide_nodes = plan.wide ? 1u : 0u;
    t.sphere_only = plan.sphere_only() ? 1u : 0u;
    t.dark_kernel = plan.dark ? (RTP_DARK_CARRY != 0 ? 1u : 2u) : 0u;
    t.primary_visibility = plan.prim ? 1u : 0u;
    kernel_resources(trace, t.trace_vgprs, t.trace_scratch_bytes);
    return t;
}
// What a finished frame left in its counter block: the flagged samples (list slots handed out less the ones nobody filled) and the
// passes the guarded launch gave up → t; the abort word of a developer build's tripwire → an error
rt_status read_counters(const uint32_t *queue, int passes, rt_timing &t) {
    if (t.guarded) {
        std::vector<uint32_t> counts((size_t)passes), gave_up((size_t)passes), holes((size_t)passes);
        HIP_TRY(hipMemcpy(counts.data(), queue + kQueueFlag, counts.size() * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(holes.data(), queue + kQueueHoles, holes.size() * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(gave_up.data(), queue + kQueueAbandon, gave_up.size() * 4, hipMemcpyDeviceToHost));
        t.flagged_samples = 0;
        t.abandoned_passes = 0;
        for (size_t p = 0; p < counts.size(); ++p) {
            t.flagged_samples += counts[p] - holes[p];
            t.abandoned_passes += gave_up[p] != 0u ? 1u : 0u;
        }
    }
    uint32_t abort_code = 0;
    HIP_TRY(hipMemcpy(&abort_code, queue + kQueueStats + 15, 4, hipMemcpyDeviceToHost));
    if (abort_code != 0) return fail(RT_ERR_HIP, "render kernel aborted (protocol timeout, code " + std::to_string(abort_code) + ")");
    return RT_OK;
}

// What a frame of render_impl's is to the handle.  A frame of its history (rt_render*, the min_spp round of rt_render_adaptive) counts in
// the handle's counter block, is timed by the handle's clock and per-pass events, reports to a feedback slot for the handle's judgement
// of its guarded walk, owns the key of the view lists and is what rt_last_timing describes (sc->last*).  A frame outside it
// (rt_render_lens) has the handle's walk machinery and none of its memory of past frames: a clock and a counter block of its own, no
// per-pass events, no feedback, and its record goes to the caller alone.
struct FrameBook {
    bool history = true;
    CallClock *clock = nullptr;
    uint32_t *queue = nullptr;                  // the counter block the frame counts in (kQueue*)
    int timed_passes = 0;                       // passes with events of their own
    rt_scene::Feedback *feedback = nullptr;     // the slot the frame reports to
};
// before the first launch: the counter block cleared, the feedback slot taken, the clock started
rt_status open_book(rt_scene *sc, bool history, int passes, hipStream_t stream, FrameBook &B) {
    rt_status st = RT_OK;
    B.history = history;
    B.clock = &sc->clock[history ? kClockRender : kClockLens];
    if (!history && (st = B.clock->make(kQueueWords)) != RT_OK) return st;
    B.queue = history ? sc->queue : B.clock->words;
    HIP_TRY(hipMemsetAsync(B.queue, 0, kQueueWords * 4, stream));
    if (history) {
        if ((st = acquire_feedback(sc, &B.feedback)) != RT_OK) return st;
        HIP_TRY(hipEventRecord(B.feedback->start, stream));
        B.timed_passes = passes < kTimedPasses ? passes : kTimedPasses;
        if ((st = grow_events(sc->pass_events, 4 * (size_t)B.timed_passes)) != RT_OK) return st;
        sc->timed_passes = 0;
    }
    return B.clock->start(stream);
}
// after the last launch: the clock stopped, and the frame's record — to the caller alone, or left with the handle for later calls
rt_status close_book(rt_scene *sc, const FrameBook &B, const rt_timing &record, const rtk::KParams &P, int passes, bool exploring, hipStream_t stream,
                     int32_t sync, rt_timing *timing) {
    rt_status st = B.clock->stop(stream);
    if (st != RT_OK) return st;
    const uint64_t samples = (uint64_t)P.num_pixels * (uint64_t)P.spp;
    if (!B.history) {
        rt_timing t = record;
        t.traced_samples = samples;
        t.guard_paused = sc->guard_paused ? 1u : 0u;
        if (sync) {
            if ((st = B.clock->elapsed(t.kernel_ms)) != RT_OK) return st;
            if ((st = read_counters(B.queue, passes, t)) != RT_OK) return st;
        }
        timing_out(t, timing);
        return RT_OK;
    }
    // flagged counts and abandon words of this call → pinned host memory, and the frame's end, for a later call's poll_feedback
    rt_scene::Feedback &f = *B.feedback;
    if (record.guarded) {
        HIP_TRY(hipMemcpyAsync(f.host, B.queue + kQueueFlag, (size_t)passes * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(f.host + kMaxPasses, B.queue + kQueueAbandon, (size_t)passes * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(f.host + 2 * kMaxPasses, B.queue + kQueueHoles, (size_t)passes * 4, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipEventRecord(f.done, stream));
    f.pending = true;
    f.guarded = record.guarded != 0u;
    f.exploring = exploring;
    f.passes = passes;
    f.samples = samples;
    f.serial = ++sc->frame_serial;
    sc->timed = true;
    sc->durations_read = false;
    sc->last = record;
    sc->last_passes = passes;
    sc->last_samples = samples;
    sc->last_traced_pixels = record.primary_visibility ? P.traced_pixels : nullptr;
    sc->last_spp = P.spp;
    if (sync) return rt_last_timing(sc, timing);
    timing_out(sc->last, timing);
    return RT_OK;
}

// rt_render, rt_render_tile and rt_render_samples: whole rows of a shard, or a rectangle; samples [sample_first, sample_first + spp).
// moments (rt_render_adaptive's min_spp round; null for every other call): each pass's luminance moments are added there as well.
// lens (rt_render_lens; null for every other call): every sample starts from the lens / moving camera (render_lens_kernel), without
// candidate lists or a re-pack, and the frame is none of the handle's history (FrameBook): *timing gets this call's record.
rt_status render_impl(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const Tile *tile, float *d_fb_sum, void *hip_stream,
                      int32_t sync, rt_timing *timing, int32_t sample_first = 0, float *moments = nullptr, const rtk::LensCam *lens = nullptr) {
    // ---- 1. validate, fill P
    Frame F;
    rt_status st = frame_prologue("rt_render_samples", sc, cam, shard, tile, sample_first, nullptr, d_fb_sum ? nullptr : "null framebuffer", hip_stream, timing, F,
                                  nothing_late);
    if (st != RT_OK) return st;
    rtk::KParams &P = F.P;
    const rt_config &cfg = sc->cfg;
    const hipStream_t stream = F.stream;
    const uint32_t num_pixels = F.num_pixels;
    const bool history = lens == nullptr;
    P.fb = d_fb_sum;
    // what earlier frames of this handle reported about their guarded walk (no wait: whatever has landed by now)
    if (history && (st = poll_feedback(sc, false)) != RT_OK) return st;
    if (F.nothing_to_do()) return RT_OK;
    if (P.spp <= 0 || P.max_depth <= 0) {
        if ((st = blank_frame(d_fb_sum, F, sync)) != RT_OK) return st;
        if (history) sc->timed = false;
        return RT_OK;
    }

    // ---- 2. the walk, the tree re-packed for a far camera
    bool guarded = false, exploring = false;
    if ((st = refuse_retired(cfg)) != RT_OK) return st;
    if (lens) guarded = lens_guarded(sc, P, *lens);
    else if ((st = choose_traversal(sc, cam, shard, tile, stream, P, guarded, exploring)) != RT_OK) return st;
    // ---- 3. launch shapes
    LaunchPlan plan = plan_launch(sc, cam, P, guarded, lens == nullptr);
    guarded = plan.guarded();
    if (moments != nullptr) plan.dark = false;        // (rt_render_adaptive's min_spp round keeps its kernel)
    // ---- 4. buffers.  Samples per pass (rt_accel.h, plan_passes): as many as the workspace budget admits (rt_config.workspace_bytes,
    // default a sixteenth of the device; 12 bytes per sample), at least 64 where the work-index bound allows, and never more than the
    // bound num_pixels * pass + 64 <= 2^30 of the kernel's 32-bit work index (div_magic, kFlagHole, kAbandonedCounter) —
    // a forced rt_config.pass_spp included; the passes of a frame are made equally long.
    // Fewer, larger launches amortise the end-of-launch tail — on a row shard of an N-GPU frame
    // the pass grows N-fold, so a launch keeps the size it has on one GPU.
    rtaccel::PassPlan passes;
    if ((st = reserve_buffers(sc, P, num_pixels, stream, plan, passes)) != RT_OK) return st;
    const bool prim = plan.prim;
    bind_slab(sc, P, num_pixels, passes.pass_size);
    bind_view_lists(sc, P, num_pixels, prim);
    P.k_inner = plan.k_inner;
    P.k_shade = plan.k_shade;

    // ---- 5. the passes
    const Shape &trace_shape = plan.trace_shape();
    const int wgs = grid_for(sc, trace_shape, num_pixels, P.spp), rework_wgs = grid_for(sc, plan.exact, num_pixels, P.spp);
    const void *trace = lens ? lens_trace_kernel(plan) : trace_kernel(plan);
    const void *rework = rewalk_kernel(plan, lens != nullptr);
    const rt_timing record = plan_timing(sc, plan, wgs, passes.passes, trace);
    const bool overlap = plan.overlap;
    // an early return between the fork to the second stream and the join must not leave that stream running unobserved
    struct JoinOnExit {
        rt_scene *sc; hipStream_t stream; bool forked = false, listing = false;
        ~JoinOnExit() {
            if (forked && hipEventRecord(sc->ev_join, sc->aux_stream) == hipSuccess) (void)hipStreamWaitEvent(stream, sc->ev_join, 0);
            if (listing) (void)hipStreamWaitEvent(stream, sc->ev_listed, 0);
        }
    } join_guard{sc, stream};
    FrameBook book;
    if ((st = open_book(sc, history, passes.passes, stream, book)) != RT_OK) return st;
    uint32_t *const queue = book.queue;
    P.stats = queue + kQueueStats;
    if (prim) {
        if ((st = make_view_lists(sc, cam, P, num_pixels, stream)) != RT_OK) return st;
    } else if (history) {
        sc->cand_key.valid = false;
    }
    if (guarded) {
        // near-first walk; samples it cannot vouch for go to the list …
        P.stack_levels = plan.fast.stack_levels;
        P.num_top = plan.fast.num_top;
        P.flag_list = sc->flag_list;
        P.resume_tag = plan.resume ? sc->resume_tag : nullptr;
        P.resume_state = plan.resume ? sc->resume_state : nullptr;
        P.resume_shift = plan.resume ? 32u - kResumeBits : 0u;
        P.dirty = overlap ? sc->dirty : nullptr;
        P.dirty_list = overlap ? sc->dirty_list : nullptr;
        P.flag_cap = (uint32_t)(sc->flag_cap < 0xffffffffu ? sc->flag_cap : 0xffffffffu);
        if (const uint32_t tiny = cfg.flag_capacity) P.flag_cap = tiny < P.flag_cap ? tiny : P.flag_cap;   // test hook: overflow path
        P.flag_chunk_words = plan.flag_chunk_words;
        // in-launch bail-out (not for a caller who insists on the guarded walk)
        P.bail_share = cfg.guard_keep ? 0u : bail_share_of(cfg);
        P.bail_floor = bail_floor();
        P.bail_latest = bail_latest();
    } else {
        P.stack_levels = 0;
        P.num_top = plan.exact.num_top;
        if (plan.walk == Walk::ExactSimple) {
            P.flag_chunk_words = 0;
            P.bail_share = 0;
        }
    }
    const uint64_t waves_total = (uint64_t)wgs * (plan.block() / rtk::kWave);
    for (int pass = 0; pass < passes.passes; ++pass) {
        // samples [pass_first, pass_first + pass_count) of every pixel, traced in any order into the slab …
        const bool timed_pass = pass < book.timed_passes;
        if (timed_pass) HIP_TRY(hipEventRecord(sc->pass_events[4 * pass], stream));
        if ((st = set_pass(P, passes, pass, num_pixels, sample_first)) != RT_OK) return st;
        P.queue = queue + kQueueWork + pass;
        P.work_list = nullptr;
        reservation(P.total_work, waves_total, P.chunk, P.taper_shift);
        if (const int forced = cfg.reserve_chunk) P.chunk = (uint32_t)(64u * (uint64_t)(forced > 0 ? forced : 1));
        if (!cfg.reserve_taper) P.taper_shift = 0;
        if (prim) {
            // primary visibility of this pass's samples: (hit distance, primitive) into each sample's slot of the slab
            launch_primary(sc, P, num_pixels, stream);
            HIP_TRY(hipGetLastError());
        }
        if (timed_pass) HIP_TRY(hipEventRecord(sc->pass_events[4 * pass + 1], stream));
        if (guarded) {
            // resume table: cleared per pass (1 MB of tags)
            if (P.resume_tag != nullptr) HIP_TRY(hipMemsetAsync(sc->resume_tag, 0, sizeof(uint32_t) << kResumeBits, stream));
            P.flag_count = queue + kQueueFlag + pass;
            if (overlap) HIP_TRY(hipMemsetAsync(sc->dirty, 0, (size_t)num_pixels * sizeof(uint32_t), stream));      // this pass's marks (8 MB at 1080p: microseconds)
            P.dirty_count = queue + kQueueDirty + pass;
            P.abandon = P.bail_share != 0u ? queue + kQueueAbandon + pass : nullptr;
            rtk::fill_consts(P);          // (everything the constants block copies is final now)
            HIP_TRY(launch(trace, plan.block(), wgs, trace_shape.lds_bytes, stream, P, lens));
            if (timed_pass) HIP_TRY(hipEventRecord(sc->pass_events[4 * pass + 2], stream));
            // … and are walked again in the reference's order, overwriting their slab entries
            rtk::KParams R = P;
            set_exact_rewalk(R, cfg, plan);
            R.queue = queue + kQueueRework + pass;
            R.work_list = sc->flag_list;
            R.work_count = queue + kQueueFlag + pass;
            R.work_cap = P.flag_cap;
            // … unless the list turns out to be the whole pass (overflow, abandoned guarded pass): a trace launch's reservations
            reservation(P.total_work, (uint64_t)rework_wgs * (rtk::kBlock / rtk::kWave), R.full_chunk, R.full_taper);
            R.dirty = nullptr;
            hipStream_t rework_stream = stream;       // the exact re-walk may go to the handle's second stream (overlap_rework)
            if (overlap) {
                // the re-walk and the accumulation of the pixels it touches on the second stream …
                HIP_TRY(hipEventRecord(sc->ev_fork, stream));
                HIP_TRY(hipStreamWaitEvent(sc->aux_stream, sc->ev_fork, 0));
                join_guard.forked = true;
                rework_stream = sc->aux_stream;
                // the pixels the trace launch marked, as a list for the second accumulate launch — made on a third stream beside the
                // re-walk (0.2 ms at 1080p that would otherwise lengthen the re-walk's chain past the other pixels' accumulation)
                HIP_TRY(hipStreamWaitEvent(sc->list_stream, sc->ev_fork, 0));
                hipLaunchKernelGGL(rtk::dirty_compact_kernel, dim3((num_pixels + rtk::kDirtyPixels - 1) / rtk::kDirtyPixels), dim3(rtk::kDirtyBlock), 0, sc->list_stream,
                                   (const uint32_t *)sc->dirty, num_pixels, sc->dirty_list, queue + kQueueDirty + pass);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(sc->ev_listed, sc->list_stream));
                join_guard.listing = true;
            }
            HIP_TRY(launch(rework, (uint32_t)rtk::kBlock, rework_wgs, plan.exact.lds_bytes, rework_stream, R, lens));
        } else {
            if (plan.walk == Walk::ExactSimple) rtk::fill_consts(P);          // (its launch constants come from the LDS block, like the guarded sphere-only build's)
            HIP_TRY(launch(trace, plan.block(), wgs, trace_shape.lds_bytes, stream, P, lens));
        }
        if (timed_pass) {
            if (!guarded) HIP_TRY(hipEventRecord(sc->pass_events[4 * pass + 2], stream));
            HIP_TRY(hipEventRecord(sc->pass_events[4 * pass + 3], overlap ? sc->aux_stream : stream));
            sc->timed_passes = pass + 1;
        }
        // … then added to the pixel sums strictly in sample order
        if (overlap) {
            // the pixels the re-walk may touch on the second stream, once they are listed …
            // (a pass the guarded launch gave up has rows nobody traced yet: both launches stand down — P.abandon — and a third one,
            // after the re-walk of everything, sums every pixel)
            HIP_TRY(hipStreamWaitEvent(sc->aux_stream, sc->ev_listed, 0));
            join_guard.listing = false;
            launch_accumulate(sc->aux_stream, P, Acc::marked(pass, sc->dirty, sc->dirty_list, queue + kQueueDirty + pass, P.abandon));
            HIP_TRY(hipEventRecord(sc->ev_join, sc->aux_stream));
            // … while every other pixel is accumulated here
            launch_accumulate(stream, P, Acc::unmarked(pass, sc->dirty, P.abandon));
            HIP_TRY(hipStreamWaitEvent(stream, sc->ev_join, 0));
            join_guard.forked = false;
            if (P.abandon) launch_accumulate(stream, P, Acc::abandoned_pass(pass, P.abandon));
        } else {
            launch_accumulate(stream, P, Acc::every_pixel(pass));
        }
        // rt_render_adaptive: the pass's luminance moments, once every row of it is final — on this stream after the join with the
        // overlapped re-walk, and after the third accumulate launch of an abandoned pass
        if (moments) launch_moments(stream, moments, P, pass == 0 ? 1 : 0);
    }
    HIP_TRY(hipGetLastError());
    // ---- 6. what the frame leaves: for the caller, and (a frame of the handle's history) for later calls
    return close_book(sc, book, record, P, passes.passes, exploring, stream, sync, timing);
}

// rt_render_aov and rt_render_aov_tile (rt_aov.hip.inc).  The handle's state it may change is only what any call shares: the slab, the
// candidate lists (and their key, so that a beauty frame of the same view reuses them).  No feedback slot, no re-pack, no counter
// block, no per-pass events of rt_render: what the handle decides next, and what rt_last_timing reports, stay those of its
// rt_render calls.
// lens (rt_render_aov_lens): every sample's first hit from the lens / moving camera's ray, without candidate lists (those of the
// handle stay as they are).
// fog (rt_render_aov_volume, with lens): the lens frame's records, accumulated under the medium (rt_aov_fog.hip.inc); fog->tr, or without
// fog d_tr, takes the transmittance sums.  what: the call the sample-range refusals name.
rt_status aov_impl(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const Tile *tile, const rt_aov_buffers *buffers, void *hip_stream,
                   int32_t sync, rt_timing *timing, int32_t sample_first = 0, const rtk::LensCam *lens = nullptr, const char *what = "rt_render_aov_samples",
                   const rtk::AovFog *fog = nullptr, float *d_tr = nullptr) {
    // (the buffers first: a caller's mistake there is reported as such whatever else is wrong)
    if (!buffers || buffers->struct_bytes < 16u) return fail(RT_ERR_INVALID_ARG, "null AOV buffers (or struct_bytes below 16)");
    rt_aov_buffers b{};
    std::memcpy(&b, buffers, buffers->struct_bytes < sizeof(b) ? buffers->struct_bytes : sizeof(b));
    if (!b.albedo_sum && !b.normal_sum && !b.depth_sum && !b.hit_count && !b.first_prim) return fail(RT_ERR_INVALID_ARG, "every AOV buffer is NULL");
    Frame F;
    rt_status st = frame_prologue(what, sc, cam, shard, tile, sample_first, nullptr, nullptr, hip_stream, timing, F, nothing_late);
    if (st != RT_OK) return st;
    if (F.nothing_to_do()) return RT_OK;
    if (fog) d_tr = fog->tr;
    rtk::KParams &P = F.P;
    const rt_config &cfg = sc->cfg;
    const hipStream_t stream = F.stream;
    const uint32_t num_pixels = F.num_pixels;
    const rtk::AovOut out{b.albedo_sum, b.normal_sum, b.depth_sum, b.hit_count, b.first_prim};
    if (P.spp <= 0) {       // no samples: zero sums, no hit
        if (out.albedo) HIP_TRY(hipMemsetAsync(out.albedo, 0, (size_t)num_pixels * 12, stream));
        if (out.normal) HIP_TRY(hipMemsetAsync(out.normal, 0, (size_t)num_pixels * 12, stream));
        if (out.depth) HIP_TRY(hipMemsetAsync(out.depth, 0, (size_t)num_pixels * 4, stream));
        if (out.hits) HIP_TRY(hipMemsetAsync(out.hits, 0, (size_t)num_pixels * 4, stream));
        if (out.prim) HIP_TRY(hipMemsetAsync(out.prim, 0xff, (size_t)num_pixels * 4, stream));
        if (d_tr) HIP_TRY(hipMemsetAsync(d_tr, 0, (size_t)num_pixels * 4, stream));
        if (sync) HIP_TRY(hipStreamSynchronize(stream));
        return RT_OK;
    }
    // Candidate lists where the handle's next beauty frame of this view would take its camera rays from them: the guarded walk is
    // its choice (not paused, not an exact frame forced by rt_config), and its tree's margins already cover this camera — rt_render
    // would re-pack the tree for a camera outside them; this call does not, and walks the reference's order instead.
    bool prim = guarded_chosen(sc, P) && cfg.kernel != RT_KERNEL_WAVEFRONT && cfg.primary_visibility >= 0 && sc->nodes != nullptr &&
                (sc->guard.dyn_k > 0.0f || cfg.scene_in_lds != 0);
    if (prim && (lens || !camera_inside_margins(sc, cam))) prim = false;
    rtaccel::PassPlan plan;
    if ((st = reserve_slab(sc, num_pixels, P.spp, stream, plan)) != RT_OK) return st;
    const int passes = plan.passes;
    bind_slab(sc, P, num_pixels, plan.pass_size);
    if ((st = reserve_view_lists(sc, num_pixels, stream, prim)) != RT_OK) return st;
    bind_view_lists(sc, P, num_pixels, prim);
    // (the call's own clock and counter word — records the reference-order walk resolved — and per-pass events)
    CallClock &clock = sc->clock[kClockAov];
    if ((st = clock.make(1)) != RT_OK) return st;
    uint32_t *const walked = clock.words;
    const int timed = passes < kTimedPasses ? passes : kTimedPasses;
    if ((st = grow_events(sc->aov_events, 3 * (size_t)timed)) != RT_OK) return st;
    if ((st = clock.start(stream)) != RT_OK) return st;
    HIP_TRY(hipMemsetAsync(walked, 0, sizeof(uint32_t), stream));
    if (prim) {
        if ((st = make_view_lists(sc, cam, P, num_pixels, stream)) != RT_OK) return st;
    } else if (!lens) {
        sc->cand_key.valid = false;         // (as rt_render does: the next call with lists makes them anew)
    }
    for (int pass = 0; pass < passes; ++pass) {
        const bool timed_pass = pass < timed;
        if ((st = set_pass(P, plan, pass, num_pixels, sample_first)) != RT_OK) return st;
        if (timed_pass) HIP_TRY(hipEventRecord(sc->aov_events[3 * pass], stream));
        if (prim) {
            launch_primary(sc, P, num_pixels, stream);
            HIP_TRY(hipGetLastError());
        }
        if (timed_pass) HIP_TRY(hipEventRecord(sc->aov_events[3 * pass + 1], stream));
        // (1) the records of pixels without a list (every record, without lists) through the reference-order walk
        const uint32_t units = prim ? (num_pixels + 3u) / 4u : (P.total_work + 255u) / 256u;
        const uint32_t rgrid = std::min<uint32_t>(units, (uint32_t)sc->num_cus * 8u);
        if (lens) hipLaunchKernelGGL(rtk::aov_resolve_lens_kernel, dim3(rgrid), dim3(256), 0, stream, P, *lens);
        else if (prim) hipLaunchKernelGGL(rtk::aov_resolve_kernel<false>, dim3(rgrid), dim3(256), 0, stream, P, walked);
        else hipLaunchKernelGGL(rtk::aov_resolve_kernel<true>, dim3(rgrid), dim3(256), 0, stream, P, walked);
        HIP_TRY(hipGetLastError());
        if (timed_pass) HIP_TRY(hipEventRecord(sc->aov_events[3 * pass + 2], stream));
        // (2) … added to the pixel's sums in sample order
        if (fog && fog->V.rho) hipLaunchKernelGGL(rtk::aov_accumulate_fog_kernel<true>, acc_grid(num_pixels), dim3(64 * rtk::kAccWaves), 0, stream, P, *lens, *fog, out, pass == 0 ? 1 : 0);
        else if (fog) hipLaunchKernelGGL(rtk::aov_accumulate_fog_kernel<false>, acc_grid(num_pixels), dim3(64 * rtk::kAccWaves), 0, stream, P, *lens, *fog, out, pass == 0 ? 1 : 0);
        else if (lens) hipLaunchKernelGGL(rtk::aov_accumulate_lens_kernel, acc_grid(num_pixels), dim3(64 * rtk::kAccWaves), 0, stream, P, *lens, out, pass == 0 ? 1 : 0, walked);
        else hipLaunchKernelGGL(rtk::aov_accumulate_kernel, acc_grid(num_pixels), dim3(64 * rtk::kAccWaves), 0, stream, P, out, pass == 0 ? 1 : 0, walked);
        HIP_TRY(hipGetLastError());
    }
    if (!fog && d_tr) {         // no medium: every sample is clear
        hipLaunchKernelGGL(rtk::aov_fog_fill_kernel, dim3((num_pixels + 255u) / 256u), dim3(256), 0, stream, d_tr, num_pixels, (float)P.spp);
        HIP_TRY(hipGetLastError());
    }
    if ((st = clock.stop(stream)) != RT_OK) return st;
    rt_timing t{};
    t.primary_visibility = prim ? 1u : 0u;
    if (sync) {
        if ((st = clock.elapsed(t.kernel_ms)) != RT_OK) return st;
        float primary = 0.0f, rework = 0.0f, ms = 0.0f;
        for (int p = 0; p < timed; ++p) {
            HIP_TRY(hipEventElapsedTime(&ms, sc->aov_events[3 * p], sc->aov_events[3 * p + 1]));
            primary += ms;
            HIP_TRY(hipEventElapsedTime(&ms, sc->aov_events[3 * p + 1], sc->aov_events[3 * p + 2]));
            rework += ms;
        }
        // (+ the lists, made before the first pass)
        primary *= untimed_scale(passes, timed);
        rework *= untimed_scale(passes, timed);
        HIP_TRY(hipEventElapsedTime(&ms, clock.first, sc->aov_events[0]));
        t.primary_ms = prim ? primary + ms : 0.0f;
        t.rework_ms = rework;
        const uint64_t samples = (uint64_t)num_pixels * (uint64_t)P.spp;
        t.traced_samples = samples;
        t.flagged_samples = samples;
        if (prim) {
            uint32_t traced = 0, resolved = 0;
            HIP_TRY(hipMemcpy(&traced, P.traced_pixels, 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&resolved, walked, 4, hipMemcpyDeviceToHost));
            t.traced_samples = (uint64_t)traced * (uint64_t)P.spp;
            t.flagged_samples = resolved;
        }
    }
    timing_out(t, timing);
    return RT_OK;
}

// rt_render_adaptive (rtp_amd.h).  The min_spp round is an ordinary rt_render frame (render_impl: its walk, its feedback,
// its decisions) that also keeps the luminance moments; every later round traces the samples [n, n + batch) of the pixels still going
// on with the reference-order walk on a list of work indices, adds them onto the running sums (accumulate_kernel<true>) and the
// moments, and judges them again.  Every round is enqueued up front: the lists and their lengths live on the device only.
void adaptive_defaults(rt_adaptive_params &p) {
    std::memset(&p, 0, sizeof(p));
    p.struct_bytes = (uint32_t)sizeof(p);
    p.min_spp = 16;
    p.batch_spp = 16;
    p.max_spp = 256;
    p.threshold = 0.02f;
}
// the parameter checks of rt_render_adaptive and rt_render_lit_adaptive (what: the call's name) → a: the caller's fields over the defaults
rt_status adaptive_check(const char *what, const rt_adaptive_params *params, rt_adaptive_params &a) {
    const std::string w(what);
    if (!params || params->struct_bytes < 8) return fail(RT_ERR_INVALID_ARG, w + ": null params (or struct_bytes below 8)");
    adaptive_defaults(a);
    std::memcpy(&a, params, params->struct_bytes < sizeof(a) ? params->struct_bytes : sizeof(a));
    if (a.min_spp < 2) return fail(RT_ERR_INVALID_ARG, w + ": min_spp below 2");
    if (a.batch_spp < 1) return fail(RT_ERR_INVALID_ARG, w + ": batch_spp below 1");
    if (a.max_spp < a.min_spp) return fail(RT_ERR_INVALID_ARG, w + ": max_spp below min_spp");
    if (!(a.threshold >= 0.0f) || !std::isfinite(a.threshold)) return fail(RT_ERR_INVALID_ARG, w + ": threshold negative, NaN or infinite");
    if (a.max_spp > 65536) return fail(RT_ERR_UNSUPPORTED, w + ": max_spp above 65536");
    return RT_OK;
}
// rt_stop_params of the _rule calls (what: the old call's name; suffix: what the _rule call adds to it — nothing for a call that takes
// the stop parameters from the start) → the rule; NULL is rule 0
rt_status stop_check(const char *what, const rt_stop_params *stop, int32_t &rule, const char *suffix = "_rule") {
    rule = 0;
    if (!stop) return RT_OK;
    const std::string w = std::string(what) + suffix;
    if (stop->struct_bytes < 8) return fail(RT_ERR_INVALID_ARG, w + ": rt_stop_params struct_bytes below 8");
    rule = stop->rule;
    if (rule != 0 && rule != 1) return fail(RT_ERR_INVALID_ARG, w + ": rule outside 0 … 1");
    return RT_OK;
}
// What rt_render_adaptive and rt_render_lit_adaptive share — the two differ in the frame that takes the min_spp samples and in the kernel
// that traces a round's list.
// The moments: the caller's d_moments, or the handle's own buffer
rt_status adaptive_moments(rt_scene *sc, uint32_t num_pixels, float *d_moments, hipStream_t stream, float *&mom) {
    mom = d_moments;
    if (mom) return RT_OK;
    if (const rt_status st = grow(sc->adapt_mom, sc->adapt_mom_pixels, (size_t)num_pixels * 2, stream)) return st;
    mom = sc->adapt_mom;
    return RT_OK;
}
// The handle's other buffers: lists, counters and — where there are rounds — work indices and a slab with rows of a round's batch.  grow
// never shrinks, so after this the slab holds a batch; a reserve_slab that runs later may free and shorten it (rt_render_adaptive checks,
// rt_render_lit_adaptive reserves its frame's slab first)
rt_status adaptive_reserve(rt_scene *sc, uint32_t num_pixels, int32_t rounds, int32_t batch, int32_t rule, hipStream_t stream) {
    rt_status st;
    if (rule == 1 && (st = grow(sc->adapt_flag, sc->adapt_flag_pixels, (size_t)num_pixels, stream)) != RT_OK) return st;
    if ((st = grow(sc->adapt_list, sc->adapt_pixels, (size_t)num_pixels * 2, stream)) != RT_OK) return st;
    if ((st = grow(sc->adapt_counters, sc->adapt_counter_words, (size_t)3 * (size_t)(rounds + 1), stream)) != RT_OK) return st;
    if (rounds > 0) {
        if ((st = grow(sc->adapt_work, sc->adapt_work_cap, (size_t)num_pixels * (size_t)batch, stream)) != RT_OK) return st;
        if ((st = grow(sc->slab, sc->slab_floats, (size_t)num_pixels * slab_pitch_of(batch) * 3, stream)) != RT_OK) return st;
    }
    return RT_OK;
}
// No depth: every sample is 0, so is every moment — and the rule stops every pixel at min_spp unless the threshold is 0
rt_status adaptive_no_depth(const rt_adaptive_params &a, float *mom, int32_t *d_spp, uint32_t num_pixels, hipStream_t stream) {
    const int32_t rounds = (a.max_spp - a.min_spp) / a.batch_spp;
    HIP_TRY(hipMemsetAsync(mom, 0, (size_t)num_pixels * 8, stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_spp, a.threshold == 0.0f ? a.min_spp + rounds * a.batch_spp : a.min_spp, num_pixels, stream));
    return RT_OK;
}
// After the min_spp frame (sums in P.fb, moments in mom): every pixel is judged and its count written, then every round is enqueued —
// expand the list of pixels still going on into work indices, trace them, add them onto the sums in slot order and onto the moments,
// judge again.  Lists and their lengths live on the device only.  Round r (1 …) traces samples [first + (r - 1) batch, … + batch) of the
// listed pixels — work index = local pixel * batch + slot, in the pixel's own slab row — by trace(P) → hipError_t: one launch on P, whose
// pass, slab, list (work_list, work_count, work_cap) and queue are set here.
// One judgement of the pixels with n samples — those of list_in (null: every local pixel) — into list_out / count_out and the counts.
// Rule 0: adaptive_select_kernel.  Rule 1 (flag: one byte per pixel, W: the buffer's shape): the flag kernel, then the select kernel
// that reads the windows; with threshold 0 nothing is judged noisy or quiet — every pixel goes on while the cap allows — which is rule
// 0's launch.  prior (null: none): the prior variants of the select and flag kernels (rt_render_adaptive_prior), which compare ve.
rtk::AdaptWindow adapt_window(int32_t width, int32_t rows, int32_t band_rows, int32_t num_parts) {
    rtk::AdaptWindow W;
    W.width = (uint32_t)width;
    W.rows = (uint32_t)rows;
    W.band_rows = (uint32_t)band_rows;
    W.banded = num_parts > 1 ? 1u : 0u;
    return W;
}
rt_status adaptive_judge(const rt_adaptive_params &a, int32_t rule, const float *mom, const float *prior, int32_t *d_spp, uint8_t *flag,
                         const rtk::AdaptWindow &W, uint32_t num_pixels, const uint32_t *list_in, const uint32_t *count_in, uint32_t *list_out,
                         uint32_t *count_out, int32_t n, hipStream_t stream) {
    const dim3 pix_grid((num_pixels + rtk::kAdaptBlock - 1) / rtk::kAdaptBlock), pix_block(rtk::kAdaptBlock);
    const int32_t batch = a.batch_spp;
    if (prior && (rule != 1 || a.threshold == 0.0f)) {
        if (!list_in)
            hipLaunchKernelGGL(rtk::adaptive_select_prior_kernel<true>, pix_grid, pix_block, 0, stream, mom, prior, d_spp, num_pixels,
                               (const uint32_t *)nullptr, (const uint32_t *)nullptr, list_out, count_out, n, batch, a.max_spp, a.threshold);
        else
            hipLaunchKernelGGL(rtk::adaptive_select_prior_kernel<false>, pix_grid, pix_block, 0, stream, mom, prior, d_spp, num_pixels, list_in, count_in,
                               list_out, count_out, n, batch, a.max_spp, a.threshold);
    } else if (prior) {
        if (!list_in)
            hipLaunchKernelGGL(rtk::adaptive_flag_prior_kernel<true>, pix_grid, pix_block, 0, stream, mom, prior, flag, num_pixels, (const uint32_t *)nullptr,
                               (const uint32_t *)nullptr, n, a.threshold);
        else
            hipLaunchKernelGGL(rtk::adaptive_flag_prior_kernel<false>, pix_grid, pix_block, 0, stream, mom, prior, flag, num_pixels, list_in, count_in, n,
                               a.threshold);
        if (!list_in)
            hipLaunchKernelGGL(rtk::adaptive_select_near_kernel<true>, pix_grid, pix_block, 0, stream, (const uint8_t *)flag, d_spp, num_pixels, W,
                               (const uint32_t *)nullptr, (const uint32_t *)nullptr, list_out, count_out, n, batch, a.max_spp);
        else
            hipLaunchKernelGGL(rtk::adaptive_select_near_kernel<false>, pix_grid, pix_block, 0, stream, (const uint8_t *)flag, d_spp, num_pixels, W, list_in,
                               count_in, list_out, count_out, n, batch, a.max_spp);
    } else if (rule != 1 || a.threshold == 0.0f) {
        if (!list_in)
            hipLaunchKernelGGL(rtk::adaptive_select_kernel<true>, pix_grid, pix_block, 0, stream, mom, d_spp, num_pixels, (const uint32_t *)nullptr,
                               (const uint32_t *)nullptr, list_out, count_out, n, batch, a.max_spp, a.threshold);
        else
            hipLaunchKernelGGL(rtk::adaptive_select_kernel<false>, pix_grid, pix_block, 0, stream, mom, d_spp, num_pixels, list_in, count_in, list_out,
                               count_out, n, batch, a.max_spp, a.threshold);
    } else if (!list_in) {
        hipLaunchKernelGGL(rtk::adaptive_flag_kernel<true>, pix_grid, pix_block, 0, stream, mom, flag, num_pixels, (const uint32_t *)nullptr,
                           (const uint32_t *)nullptr, n, a.threshold);
        hipLaunchKernelGGL(rtk::adaptive_select_near_kernel<true>, pix_grid, pix_block, 0, stream, (const uint8_t *)flag, d_spp, num_pixels, W,
                           (const uint32_t *)nullptr, (const uint32_t *)nullptr, list_out, count_out, n, batch, a.max_spp);
    } else {
        hipLaunchKernelGGL(rtk::adaptive_flag_kernel<false>, pix_grid, pix_block, 0, stream, mom, flag, num_pixels, list_in, count_in, n, a.threshold);
        hipLaunchKernelGGL(rtk::adaptive_select_near_kernel<false>, pix_grid, pix_block, 0, stream, (const uint8_t *)flag, d_spp, num_pixels, W, list_in,
                           count_in, list_out, count_out, n, batch, a.max_spp);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
template <class Trace>
rt_status adaptive_rounds(rt_scene *sc, const rt_adaptive_params &a, int32_t rule, rtk::KParams &P, float *mom, const float *prior, int32_t *d_spp,
                          uint32_t num_pixels, int32_t first, hipStream_t stream, Trace trace) {
    const int32_t batch = a.batch_spp, rounds = (a.max_spp - a.min_spp) / a.batch_spp;
    const dim3 pix_grid((num_pixels + rtk::kAdaptBlock - 1) / rtk::kAdaptBlock), pix_block(rtk::kAdaptBlock);
    const uint64_t expand_items = (uint64_t)num_pixels * (uint64_t)batch;
    const uint32_t expand_grid = (uint32_t)std::min<uint64_t>((expand_items + rtk::kAdaptBlock - 1) / rtk::kAdaptBlock, (uint64_t)sc->num_cus * 8u);
    uint32_t *lists[2] = {sc->adapt_list, sc->adapt_list + num_pixels};
    uint32_t *const counters = sc->adapt_counters;          // round r (1 …): [3(r-1)] its list's length, [3(r-1) + 1] its work indices, [3(r-1) + 2] its queue
    const rtk::AdaptWindow W = adapt_window(P.row_w, P.local_rows, P.band_rows, P.num_parts);
    rt_status st;
    HIP_TRY(hipMemsetAsync(counters, 0, (size_t)3 * (size_t)(rounds + 1) * sizeof(uint32_t), stream));
    int32_t n = a.min_spp;
    if ((st = adaptive_judge(a, rule, mom, prior, d_spp, sc->adapt_flag, W, num_pixels, nullptr, nullptr, lists[0], counters, n, stream)) != RT_OK) return st;
    if (rounds > 0) {
        bind_slab(sc, P, num_pixels, batch);
        P.pass_count = batch;
        P.total_work = num_pixels * (uint32_t)batch;
        if (!make_magic((uint32_t)batch, (uint64_t)P.total_work + 64, P.magic_count)) return fail(RT_ERR_UNSUPPORTED, "image too large for the work index arithmetic");
        P.work_list = sc->adapt_work;
        P.work_cap = P.total_work;                              // (the list never stands for "every sample")
    }
    for (int32_t r = 1; r <= rounds; ++r) {
        const uint32_t *list = lists[(r - 1) & 1];
        const uint32_t *listed = counters + 3 * (r - 1);
        hipLaunchKernelGGL(rtk::adaptive_expand_kernel, dim3(expand_grid), pix_block, 0, stream, list, listed, (uint32_t)batch, sc->adapt_work,
                           counters + 3 * (r - 1) + 1);
        P.pass_first = first + (r - 1) * batch;
        P.work_count = counters + 3 * (r - 1) + 1;
        P.queue = counters + 3 * (r - 1) + 2;
        HIP_TRY(trace(P));
        launch_accumulate(stream, P, Acc::onto_sums(list, listed));
        hipLaunchKernelGGL(rtk::moments_kernel<true>, pix_grid, pix_block, 0, stream, mom, (const float *)P.slab, num_pixels, P.slab_pitch, batch, 0, list, listed,
                           (const uint32_t *)nullptr, 0u, 0.0f, 0.0f, 0.0f);
        n += batch;
        HIP_TRY(hipGetLastError());
        if (r < rounds && (st = adaptive_judge(a, rule, mom, prior, d_spp, sc->adapt_flag, W, num_pixels, list, listed, lists[r & 1], counters + 3 * r, n, stream)) != RT_OK)
            return st;
    }
    return RT_OK;
}
// The check of the _prior calls (what: the new call's name), right after the stop checks: d_prior (8 bytes per local pixel; null: none)
// shares no byte with what the call writes.  The local pixel count is what cam and shard give without a scene; where they give none (a
// null camera, an image or a part without pixels) a later check refuses the call or the call has nothing to do.
rt_status prior_check(const char *what, const float *d_prior, const rt_camera_data *cam, const rt_shard *shard, const float *d_fb_sum,
                      const int32_t *d_spp, const float *d_moments) {
    if (!d_prior || !cam || cam->image_width <= 0) return RT_OK;
    const uint64_t num_pixels = (uint64_t)rt_shard_rows(cam->image_height, shard) * (uint64_t)cam->image_width;
    const uintptr_t lo = (uintptr_t)d_prior, hi = lo + (uintptr_t)num_pixels * 8;
    const auto shares = [&](const void *ptr, uintptr_t bytes) { return ptr && lo < (uintptr_t)ptr + bytes && (uintptr_t)ptr < hi; };
    if (shares(d_fb_sum, (uintptr_t)num_pixels * 12) || shares(d_spp, (uintptr_t)num_pixels * 4) || shares(d_moments, (uintptr_t)num_pixels * 8))
        return fail(RT_ERR_INVALID_ARG, std::string(what) + ": d_prior overlaps d_fb_sum, d_spp or d_moments");
    return RT_OK;
}
rt_status adaptive_impl(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const rt_adaptive_params *params, const rt_stop_params *stop,
                        const float *d_prior, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing) {
    // ---- 1. every check before anything is enqueued
    rt_adaptive_params a;
    int32_t rule;
    if (const rt_status cs = adaptive_check("rt_render_adaptive", params, a)) return cs;
    if (const rt_status cs = stop_check("rt_render_adaptive", stop, rule)) return cs;
    if (const rt_status cs = prior_check("rt_render_adaptive_prior", d_prior, cam, shard, d_fb_sum, d_spp, d_moments)) return cs;
    if (!cam) return fail(RT_ERR_INVALID_ARG, "null scene or camera");
    rt_camera_data base = *cam;
    base.samples_per_pixel = a.min_spp;
    const int32_t batch = a.batch_spp, rounds = (a.max_spp - a.min_spp) / a.batch_spp;
    Frame F;
    rt_status st = frame_prologue("rt_render_adaptive", sc, &base, shard, nullptr, 0, nullptr,
                                  d_fb_sum && d_spp ? nullptr : "rt_render_adaptive: null framebuffer or sample counts", hip_stream, timing, F, [&] {
        if (rounds > 0 && (uint64_t)F.num_pixels * (uint64_t)batch >= (1ull << 31) - 4096)
            return fail(RT_ERR_UNSUPPORTED, "rt_render_adaptive: pixels x batch_spp beyond the work index arithmetic");
        return RT_OK;
    });
    if (st != RT_OK) return st;
    if (F.nothing_to_do()) return RT_OK;
    rtk::KParams &P = F.P;
    const hipStream_t stream = F.stream;
    const uint32_t num_pixels = F.num_pixels;

    // ---- 2. the handle's buffers
    float *mom;
    if ((st = adaptive_moments(sc, num_pixels, d_moments, stream, mom)) != RT_OK) return st;
    if ((st = adaptive_reserve(sc, num_pixels, rounds, batch, rule, stream)) != RT_OK) return st;
    const size_t slab_need = rounds > 0 ? (size_t)num_pixels * slab_pitch_of(batch) * 3 : 0;
    CallClock &clock = sc->clock[kClockAdaptive];
    if ((st = clock.make()) != RT_OK) return st;
    if ((st = clock.start(stream)) != RT_OK) return st;

    // ---- 3. the min_spp round: rt_render's frame, with the moments
    if ((st = render_impl(sc, &base, shard, nullptr, d_fb_sum, hip_stream, 0, nullptr, 0, mom)) != RT_OK) return st;
    if (P.max_depth <= 0) {
        // (render_impl wrote all-zero sums without a pass)
        if ((st = adaptive_no_depth(a, mom, d_spp, num_pixels, stream)) != RT_OK) return st;
        if ((st = clock.stop(stream)) != RT_OK) return st;
        if (sync) HIP_TRY(hipStreamSynchronize(stream));
        return RT_OK;
    }
    if (sc->slab_floats < slab_need) return fail(RT_ERR_OUT_OF_MEMORY, "rt_render_adaptive: the sample slab shrank below a round's batch");

    // ---- 4. the rounds: the exact walk's launch shape for this view (the tables may have been re-packed by the frame: P anew)
    if ((st = fill_params(sc, &base, shard, P)) != RT_OK) return st;
    const LaunchPlan plan = plan_launch(sc, &base, P, false);
    P.fb = d_fb_sum;
    set_exact_rewalk(P, sc->cfg, plan);          // (lists: finest granularity, as the exact re-walk of flagged samples)
    P.cand = nullptr; P.order = nullptr; P.traced_pixels = nullptr;       // every sample starts from the camera
    P.resume_tag = nullptr; P.resume_state = nullptr; P.abandon = nullptr; P.dirty = nullptr; P.dirty_list = nullptr;
    const void *exact = rewalk_kernel(plan);
    const int wgs = grid_for(sc, plan.exact, num_pixels, batch);
    reservation(num_pixels * (uint32_t)batch, (uint64_t)wgs * (rtk::kBlock / rtk::kWave), P.full_chunk, P.full_taper);
    st = adaptive_rounds(sc, a, rule, P, mom, d_prior, d_spp, num_pixels, a.min_spp, stream,
                         [&](const rtk::KParams &KP) { return launch(exact, (uint32_t)rtk::kBlock, wgs, plan.exact.lds_bytes, stream, KP); });
    if (st != RT_OK) return st;
    if ((st = clock.stop(stream)) != RT_OK) return st;
    if (!sync) return RT_OK;
    // what rt_last_timing reports for the min_spp round, with the whole call's kernel_ms and every trace launch of it
    rt_timing t;
    rt_timing_init(&t);
    if ((st = rt_last_timing(sc, &t)) != RT_OK) return st;
    if ((st = clock.elapsed(t.kernel_ms)) != RT_OK) return st;
    t.trace_launches += (uint32_t)rounds;
    timing_out(t, timing);
    return RT_OK;
}

// ---- what the lit calls share: the frame driver of rt_render_nee / rt_render_env / rt_render_lit, the probe of rt_trace_samples and its
// lit kin.  The passes of render_impl (plan_passes, the slab, accumulate_kernel in sample order) with a trace kernel of rt_light.hip.inc as
// the trace launch; nothing of the handle's walk machinery is touched.
//   light_device: the device of a light that is an object of its own (null: the light is the handle's);
//   with_light(frame): makes the light, once the call is known to trace, and returns frame(kernel, &light) — the kernel of that light's
//   type, (KParams, Light) or, with lens, (KParams, Light, LensCam): rt_render_lit's — while the light lives
// Workgroups per CU of a lit trace kernel as the loaded code object allows, and the grid of a launch on `work` work indices: what fills
// the device, fewer where the work does not give every wave a chunk
int light_wgs_per_cu(const void *kernel) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, rtk::kLightBlock, 0) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    return per_cu;
}
int light_grid(int wgs, uint32_t work) {
    const int waves_per_wg = rtk::kLightBlock / rtk::kWave;
    const uint32_t need = (work + rtk::kLightChunk - 1) / rtk::kLightChunk;          // waves that can get work at all
    int grid = wgs;
    if ((uint64_t)grid * waves_per_wg > need) grid = (int)((need + waves_per_wg - 1) / waves_per_wg);
    return grid < 1 ? 1 : grid;
}
// The passes of a light frame: each pass's trace launch (kernel on P, light and — rt_render_lit's kernels — lens; its work counter is
// queue[pass]) and its accumulate.  moments (rt_render_lit_adaptive's min_spp frame; null for every other call): each pass's luminance
// moments are added there as well — every pixel of a light frame has a slab row.  first_grid: the first pass's workgroups.
rt_status light_passes(const void *kernel, const void *light, const rtk::LensCam *lens, rtk::KParams &P, const rtaccel::PassPlan &passes, uint32_t num_pixels,
                       int32_t sample_first, int wgs, uint32_t *queue, hipStream_t stream, float *moments, uint32_t &first_grid) {
    for (int pass = 0; pass < passes.passes; ++pass) {
        if (const rt_status st = set_pass(P, passes, pass, num_pixels, sample_first)) return st;
        P.queue = queue + pass;
        const int grid = light_grid(wgs, P.total_work);
        HIP_TRY(launch(kernel, (uint32_t)rtk::kLightBlock, grid, 0, stream, P, light, lens));
        launch_accumulate(stream, P, Acc::every_pixel(pass));
        if (moments) launch_moments(stream, moments, P, pass == 0 ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if (pass == 0) first_grid = (uint32_t)grid;
    }
    return RT_OK;
}
template <class WithLight>
rt_status render_light_impl(const char *what, const int *light_device, WithLight with_light, rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard,
                            int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing, const rtk::LensCam *lens = nullptr) {
    Frame F;
    rt_status st = frame_prologue(what, sc, cam, shard, nullptr, sample_first, light_device, d_fb_sum ? nullptr : "null framebuffer", hip_stream, timing, F,
                                  [&] { return refuse_retired(sc->cfg); });
    if (st != RT_OK) return st;
    if (F.nothing_to_do()) return RT_OK;
    rtk::KParams &P = F.P;
    const hipStream_t stream = F.stream;
    const uint32_t num_pixels = F.num_pixels;
    if (P.spp <= 0 || P.max_depth <= 0) return blank_frame(d_fb_sum, F, sync);
    return with_light([&](const void *kernel, const void *light) -> rt_status {
        P.fb = d_fb_sum;
        rtaccel::PassPlan passes;
        if ((st = reserve_slab(sc, num_pixels, P.spp, stream, passes)) != RT_OK) return st;
        bind_slab(sc, P, num_pixels, passes.pass_size);          // (no candidate lists: fill_params left P.cand and P.order null)
        const int per_cu = light_wgs_per_cu(kernel);
        rt_timing t{};
        kernel_resources(kernel, t.trace_vgprs, t.trace_scratch_bytes);
        // (a clock and work counters of the lit calls' own, one per pass — one set: a handle renders one frame at a time)
        CallClock &clock = sc->clock[kClockLight];
        if ((st = clock.make(kMaxPasses)) != RT_OK) return st;
        HIP_TRY(hipMemsetAsync(clock.words, 0, kMaxPasses * 4, stream));
        if ((st = clock.start(stream)) != RT_OK) return st;
        if ((st = light_passes(kernel, light, lens, P, passes, num_pixels, sample_first, sc->num_cus * per_cu, clock.words, stream, nullptr, t.num_workgroups)) != RT_OK)
            return st;
        if ((st = clock.stop(stream)) != RT_OK) return st;
        t.workgroup_size = (uint32_t)rtk::kLightBlock;
        t.trace_launches = (uint32_t)passes.passes;
        t.kernel = RT_KERNEL_MEGA;
        t.traced_samples = (uint64_t)num_pixels * (uint64_t)P.spp;
        t.guard_paused = sc->guard_paused ? 1u : 0u;
        if (sync) {
            if ((st = clock.elapsed(t.kernel_ms)) != RT_OK) return st;
            t.trace_ms = t.kernel_ms;
        }
        timing_out(t, timing);
        return RT_OK;
    });
}

// a caller's params struct over the defaults already in `into` (compiled against an older, shorter struct: the fields it has)
template <class T>
rt_status take_params(const std::string &what, const char *name, const T *params, T &into) {
    if (params && params->struct_bytes < 8u) return fail(RT_ERR_INVALID_ARG, what + ": " + name + ".struct_bytes below 8");
    if (params) std::memcpy(&into, params, params->struct_bytes < sizeof(T) ? params->struct_bytes : sizeof(T));
    return RT_OK;
}
// Device buffers of one probe-style call, freed on every path out of it
struct Scratch {
    std::vector<void *> owned;
    template <class T> hipError_t alloc(T *&p, size_t bytes) {
        const hipError_t e = hipMalloc((void **)&p, bytes);
        if (e == hipSuccess) owned.push_back((void *)p);
        return e;
    }
    ~Scratch() { for (void *p : owned) (void)hipFree(p); }
};

// rt_trace_samples, rt_trace_samples_nee, rt_trace_samples_env, rt_trace_samples_lit: the (i, j, s) triples checked against cam and
// uploaded, launch_probe(P, d_light_seed, d_light_seed2) run on P with the probe columns set, the columns downloaded.
//   what: the prefix of the call's messages; final_light_seed, final_light_seed2: the lit probes' light-sample RNG states (null: no
//   such column)
template <class LaunchProbe>
rt_status run_probe(const std::string &what, rtk::KParams &P, const rt_camera_data *cam, int32_t n, const int32_t *ijs, float *radiance, int32_t *rays,
                    uint32_t *final_seed, uint32_t *final_light_seed, uint32_t *final_light_seed2, LaunchProbe launch_probe) {
    if (n == 0) return RT_OK;
    for (int32_t k = 0; k < n; ++k)
        if (ijs[3 * k] < 0 || ijs[3 * k] >= cam->image_width || ijs[3 * k + 1] < 0 || ijs[3 * k + 1] >= cam->image_height || ijs[3 * k + 2] < 0)
            return fail(RT_ERR_INVALID_ARG, what + "sample coordinate out of range");
    int32_t *d_ijs = nullptr, *d_rays = nullptr;
    float *d_rad = nullptr;
    uint32_t *d_seed = nullptr, *d_light = nullptr, *d_light2 = nullptr;
    Scratch mem;
    if (mem.alloc(d_ijs, (size_t)n * 12) != hipSuccess || mem.alloc(d_rad, (size_t)n * 12) != hipSuccess || mem.alloc(d_rays, (size_t)n * 4) != hipSuccess ||
        mem.alloc(d_seed, (size_t)n * 4) != hipSuccess || (final_light_seed && mem.alloc(d_light, (size_t)n * 4) != hipSuccess) ||
        (final_light_seed2 && mem.alloc(d_light2, (size_t)n * 4) != hipSuccess))
        return fail(RT_ERR_OUT_OF_MEMORY, what + "hipMalloc failed");
    if (hipMemcpy(d_ijs, ijs, (size_t)n * 12, hipMemcpyHostToDevice) != hipSuccess) return fail(RT_ERR_HIP, what + "hipMemcpy H2D failed");
    P.probe_ijs = d_ijs; P.probe_rad = d_rad; P.probe_rays = d_rays; P.probe_seed = d_seed; P.probe_n = n;
    if (const rt_status st = launch_probe(P, d_light, d_light2)) return st;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(radiance, d_rad, (size_t)n * 12, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rays, d_rays, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(final_seed, d_seed, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && final_light_seed) e = hipMemcpy(final_light_seed, d_light, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && final_light_seed2) e = hipMemcpy(final_light_seed2, d_light2, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_ERR_HIP, what + "probe kernel: " + hipGetErrorString(e));
    return RT_OK;
}
}  // namespace

extern "C" {

rt_status rt_render(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, float *d_fb_sum, void *hip_stream,
                    int32_t sync, rt_timing *timing) {
    return render_impl(sc, cam, shard, nullptr, d_fb_sum, hip_stream, sync, timing, 0);
}

rt_status rt_render_samples(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, int32_t sample_first, float *d_fb_sum,
                            void *hip_stream, int32_t sync, rt_timing *timing) {
    return render_impl(sc, cam, shard, nullptr, d_fb_sum, hip_stream, sync, timing, sample_first);
}

rt_status rt_render_tile(rt_scene *sc, const rt_camera_data *cam, int32_t tile_x0, int32_t tile_y0, int32_t tile_w, int32_t tile_h,
                         float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    const Tile tile{tile_x0, tile_y0, tile_w, tile_h};
    return render_impl(sc, cam, nullptr, &tile, d_fb_sum, hip_stream, sync, timing);
}

void rt_aov_buffers_init(rt_aov_buffers *b) {
    if (!b) return;
    std::memset(b, 0, sizeof(*b));
    b->struct_bytes = (uint32_t)sizeof(*b);
}

rt_status rt_render_aov(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const rt_aov_buffers *buffers, void *hip_stream,
                        int32_t sync, rt_timing *timing) {
    return aov_impl(sc, cam, shard, nullptr, buffers, hip_stream, sync, timing, 0);
}

rt_status rt_render_aov_samples(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, int32_t sample_first, const rt_aov_buffers *buffers,
                                void *hip_stream, int32_t sync, rt_timing *timing) {
    return aov_impl(sc, cam, shard, nullptr, buffers, hip_stream, sync, timing, sample_first);
}

rt_status rt_render_aov_tile(rt_scene *sc, const rt_camera_data *cam, int32_t tile_x0, int32_t tile_y0, int32_t tile_w, int32_t tile_h,
                             const rt_aov_buffers *buffers, void *hip_stream, int32_t sync, rt_timing *timing) {
    const Tile tile{tile_x0, tile_y0, tile_w, tile_h};
    return aov_impl(sc, cam, nullptr, &tile, buffers, hip_stream, sync, timing);
}

void rt_adaptive_params_init(rt_adaptive_params *p) {
    if (p) adaptive_defaults(*p);
}

rt_status rt_render_adaptive(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const rt_adaptive_params *params, float *d_fb_sum,
                             int32_t *d_spp, float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing) {
    return adaptive_impl(sc, cam, shard, params, nullptr, nullptr, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing);
}
void rt_stop_params_init(rt_stop_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
}
rt_status rt_render_adaptive_rule(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const rt_adaptive_params *params,
                                  const rt_stop_params *stop, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream, int32_t sync,
                                  rt_timing *timing) {
    return adaptive_impl(sc, cam, shard, params, stop, nullptr, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing);
}
rt_status rt_render_adaptive_prior(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, const rt_adaptive_params *params,
                                   const rt_stop_params *stop, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream, int32_t sync,
                                   rt_timing *timing, const float *d_prior) {
    return adaptive_impl(sc, cam, shard, params, stop, d_prior, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing);
}


// ---- rt_render_lens / rt_render_aov_lens / rt_lens_camera_rays (rtp_amd.h) -------------------------------------
void rt_lens_params_init(rt_lens_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
    p->lens_radius = 0.0f;
    p->focus_distance = 10.0f;
}

namespace {
// dot(P00 - O, cross(du, dv)) in the header's float order: 0 leaves the plane in focus undefined
float lens_plane_dot(const rt_camera_data *c) {
    const float *o = c->origin.e, *p = c->pixel00_loc.e, *u = c->pixel_delta_u.e, *v = c->pixel_delta_v.e;
    const float n0 = u[1] * v[2] - u[2] * v[1], n1 = u[2] * v[0] - u[0] * v[2], n2 = u[0] * v[1] - u[1] * v[0];
    const float e0 = p[0] - o[0], e1 = p[1] - o[1], e2 = p[2] - o[2];
    return e0 * n0 + e1 * n1 + e2 * n2;
}
// the checks every lens call makes before anything is enqueued → the kernels' camera pair
rt_status lens_setup(const char *what, const rt_camera_data *open, const rt_camera_data *close, const rt_lens_params *params, rtk::LensCam &C) {
    const std::string w(what);
    if (!open) return fail(RT_ERR_INVALID_ARG, w + ": null camera");
    rt_lens_params lp;
    rt_lens_params_init(&lp);
    if (const rt_status st = take_params(w, "rt_lens_params", params, lp)) return st;
    if (close && (close->image_width != open->image_width || close->image_height != open->image_height ||
                  close->samples_per_pixel != open->samples_per_pixel || close->max_depth != open->max_depth ||
                  std::memcmp(close->background.e, open->background.e, sizeof(open->background.e)) != 0))
        return fail(RT_ERR_INVALID_ARG, w + ": cam_close differs from cam_open in width, height, spp, max_depth or background");
    if (!(std::isfinite(lp.lens_radius) && lp.lens_radius >= 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": lens_radius must be finite and >= 0");
    if (lp.lens_radius > 0.0f) {
        if (!(std::isfinite(lp.focus_distance) && lp.focus_distance > 0.0f))
            return fail(RT_ERR_INVALID_ARG, w + ": focus_distance must be positive and finite");
        if (lens_plane_dot(open) == 0.0f || (close && lens_plane_dot(close) == 0.0f))
            return fail(RT_ERR_INVALID_ARG, w + ": the camera origin lies in its image plane (dot(P00 - O, n) == 0)");
    }
    C = rtk::LensCam{};
    const rt_camera_data *ends[2] = {open, close ? close : open};
    for (int e = 0; e < 2; ++e)
        for (int k = 0; k < 3; ++k) {
            C.o[e][k] = ends[e]->origin.e[k];
            C.p00[e][k] = ends[e]->pixel00_loc.e[k];
            C.du[e][k] = ends[e]->pixel_delta_u.e[k];
            C.dv[e][k] = ends[e]->pixel_delta_v.e[k];
        }
    C.radius = lp.lens_radius;
    C.focus = lp.focus_distance;
    C.motion = close ? 1 : 0;
    C.width = open->image_width;
    return RT_OK;
}
}  // namespace

rt_status rt_render_lens(rt_scene *sc, const rt_camera_data *cam_open, const rt_camera_data *cam_close, const rt_lens_params *lens,
                         const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    rtk::LensCam C;
    if (const rt_status st = lens_setup("rt_render_lens", cam_open, cam_close, lens, C)) return st;
    if (!sc) return fail(RT_ERR_INVALID_ARG, "rt_render_lens: null scene");
    return render_impl(sc, cam_open, shard, nullptr, d_fb_sum, hip_stream, sync, timing, sample_first, nullptr, &C);
}

rt_status rt_render_aov_lens(rt_scene *sc, const rt_camera_data *cam_open, const rt_camera_data *cam_close, const rt_lens_params *lens,
                             const rt_shard *shard, int32_t sample_first, const rt_aov_buffers *buffers, void *hip_stream, int32_t sync,
                             rt_timing *timing) {
    rtk::LensCam C;
    if (const rt_status st = lens_setup("rt_render_aov_lens", cam_open, cam_close, lens, C)) return st;
    if (!sc) return fail(RT_ERR_INVALID_ARG, "rt_render_aov_lens: null scene");
    return aov_impl(sc, cam_open, shard, nullptr, buffers, hip_stream, sync, timing, sample_first, &C);
}

rt_status rt_lens_camera_rays(const rt_camera_data *cam_open, const rt_camera_data *cam_close, const rt_lens_params *lens, int32_t n,
                              const int32_t *ijs, float *origins, float *directions, uint32_t *final_seed) {
    rtk::LensCam C;
    if (const rt_status st = lens_setup("rt_lens_camera_rays", cam_open, cam_close, lens, C)) return st;
    if (n < 0) return fail(RT_ERR_INVALID_ARG, "rt_lens_camera_rays: negative count");
    if (n == 0) return RT_OK;
    if (!ijs || !origins || !directions || !final_seed) return fail(RT_ERR_INVALID_ARG, "rt_lens_camera_rays: null argument");
    int32_t *d_ijs = nullptr;
    float *d_o = nullptr, *d_d = nullptr;
    uint32_t *d_s = nullptr;
    Scratch mem;
    HIP_TRY(mem.alloc(d_ijs, (size_t)n * 12));
    HIP_TRY(mem.alloc(d_o, (size_t)n * 12));
    HIP_TRY(mem.alloc(d_d, (size_t)n * 12));
    HIP_TRY(mem.alloc(d_s, (size_t)n * 4));
    HIP_TRY(hipMemcpy(d_ijs, ijs, (size_t)n * 12, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(rtk::lens_ray_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, C, (const int32_t *)d_ijs, n, d_o, d_d, d_s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(origins, d_o, (size_t)n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(directions, d_d, (size_t)n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(final_seed, d_s, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- rt_render_nee / rt_nee_light_table / rt_trace_samples_nee (rtp_amd.h) ---------------------------------------
void rt_nee_params_init(rt_nee_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
    p->mis = 1;
}

namespace {
// what a call's rt_nee_params say, after their checks
struct NeeSetup {
    int32_t mis = 1;
    int32_t planes = 0;           // sample_planes
    int32_t select = 0;           // 0: the power table; 1: the light tree
    int32_t glossy = 0;           // 1: METAL's reflect branch takes light samples too (the glossy kernels)
};
rt_status nee_setup(const char *what, const rt_nee_params *params, NeeSetup &N) {
    const std::string w(what);
    rt_nee_params np;
    rt_nee_params_init(&np);
    if (const rt_status st = take_params(w, "rt_nee_params", params, np)) return st;
    if (params && params->struct_bytes < 12u) np.sample_planes = 0;          // (an older caller's struct ends before the field)
    if (np.mis != 0 && np.mis != 1) return fail(RT_ERR_INVALID_ARG, w + ": mis must be 0 or 1");
    if (params && params->struct_bytes < 16u) np.select = 0;
    if (np.sample_planes != 0 && np.sample_planes != 1) return fail(RT_ERR_INVALID_ARG, w + ": sample_planes must be 0 or 1");
    if (np.select != 0 && np.select != 1) return fail(RT_ERR_INVALID_ARG, w + ": select must be 0 or 1");
    if (params && params->struct_bytes < 20u) np.glossy = 0;
    if (np.glossy != 0 && np.glossy != 1) return fail(RT_ERR_INVALID_ARG, w + ": glossy must be 0 or 1");
    N.glossy = np.glossy;
    N.mis = np.mis;
    N.planes = np.sample_planes;
    N.select = np.select;
    return RT_OK;
}

// cdf and pmf of the header from an emitter table's weights: double prefix sums, the last cdf entry 1, pmf the float difference
void nee_cdf_of(const std::vector<double> &weight, std::vector<float> &cdf, std::vector<float> &pmf) {
    const size_t n = weight.size();
    cdf.assign(n, 0.0f);
    pmf.assign(n, 0.0f);
    double total = 0.0;
    for (double x : weight) total += x;
    double run = 0.0;
    for (size_t k = 0; k < n; ++k) {
        run += weight[k];
        cdf[k] = k + 1 == n ? 1.0f : (float)(run / total);
        pmf[k] = cdf[k] - (k == 0 ? 0.0f : cdf[k - 1]);
    }
}

// The emitter tables of the header — the sphere-only one and the one of sample_planes = 1 — from the handle's own device tables (read
// back once: rt_scene_create keeps no host copy of them)
rt_status nee_table_ensure(rt_scene *sc) {
    if (sc->nee_built) return RT_OK;
    const int32_t ns = sc->num_spheres, nm = sc->num_materials, npl = sc->num_planes;
    std::vector<float4> spheres((size_t)ns), materials((size_t)nm * 3), planes((size_t)npl * 5);
    if (npl > 0) HIP_TRY(hipMemcpy(planes.data(), sc->planes, planes.size() * sizeof(float4), hipMemcpyDeviceToHost));
    std::vector<int32_t> smat((size_t)ns);
    if (ns > 0) {
        HIP_TRY(hipMemcpy(spheres.data(), sc->spheres, (size_t)ns * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(smat.data(), sc->sphere_mat, (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    if (nm > 0) HIP_TRY(hipMemcpy(materials.data(), sc->materials, materials.size() * sizeof(float4), hipMemcpyDeviceToHost));
    // emit of material m as a light's: its sum in double, or a negative number when m does not qualify
    auto emit_sum = [&](int32_t m) {
        if (m < 0 || m >= nm) return -1.0;
        const float4 e = materials[(size_t)m * 3 + 1];
        const float ev[3] = {e.x, e.y, e.z};
        bool ok = true, lit = false;
        for (float c : ev) {
            if (!(std::isfinite(c) && c >= 0.0f)) ok = false;
            if (c > 0.0f) lit = true;
        }
        return ok && lit ? (double)e.x + (double)e.y + (double)e.z : -1.0;
    };
    std::vector<int32_t> index;
    std::vector<double> weight, geom;
    for (int32_t i = 0; i < ns; ++i) {
        const float r = spheres[(size_t)i].w;
        const double e = emit_sum(smat[(size_t)i]);
        if (!(r > 0.0f) || e < 0.0) continue;
        index.push_back(i);
        weight.push_back(e * ((double)r * (double)r));
        const float4 s = spheres[(size_t)i];
        geom.insert(geom.end(), {(double)s.x, (double)s.y, (double)s.z, (double)r, weight.back()});
    }
    const size_t n = index.size();
    std::vector<float> cdf, pmf;
    nee_cdf_of(weight, cdf, pmf);
    // the second table: the first one's spheres, then the planes that qualify
    std::vector<int32_t> code;
    std::vector<float> area(n, 0.0f);
    for (int32_t i : index) code.push_back(2 * i);
    for (int32_t i = 0; i < npl; ++i) {
        const float4 P1 = planes[(size_t)i * 5 + 1], U = planes[(size_t)i * 5 + 2], V = planes[(size_t)i * 5 + 3];
        int32_t type, m;
        std::memcpy(&type, &P1.w, 4);
        std::memcpy(&m, &U.w, 4);
        if (type != RT_PLANE_QUAD && type != RT_PLANE_ELLIPSE && type != RT_PLANE_TRIANGLE) continue;
        const double e = emit_sum(m);
        if (e < 0.0) continue;
        const double ux = U.x, uy = U.y, uz = U.z, vx = V.x, vy = V.y, vz = V.z;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double k = type == RT_PLANE_QUAD ? 1.0 : (type == RT_PLANE_ELLIPSE ? 3.14159265358979323846 / 4.0 : 0.5);
        const float A = (float)(k * std::sqrt((nx * nx + ny * ny) + nz * nz));
        if (!(std::isfinite(A) && A > 0.0f)) continue;
        code.push_back(2 * i + 1);
        area.push_back(A);
        weight.push_back(e * (double)A / 3.14159265358979323846);
        // (the light tree's bound of the entry: header, "Tree")
        const float4 B = planes[(size_t)i * 5 + 4];
        const double b[3] = {B.x, B.y, B.z}, u[3] = {ux, uy, uz}, v[3] = {vx, vy, vz};
        double c[3], rho = 0.0;
        auto len3 = [](double x, double y, double z) { return std::sqrt((x * x + y * y) + z * z); };
        if (type == RT_PLANE_TRIANGLE) {
            for (int k = 0; k < 3; ++k) c[k] = b[k] + (u[k] + v[k]) / 3.0;
            const double d0 = len3(b[0] - c[0], b[1] - c[1], b[2] - c[2]);
            const double d1 = len3((b[0] + u[0]) - c[0], (b[1] + u[1]) - c[1], (b[2] + u[2]) - c[2]);
            const double d2 = len3((b[0] + v[0]) - c[0], (b[1] + v[1]) - c[1], (b[2] + v[2]) - c[2]);
            rho = std::max(d0, std::max(d1, d2));
        } else {
            for (int k = 0; k < 3; ++k) c[k] = (b[k] + 0.5 * u[k]) + 0.5 * v[k];
            rho = 0.5 * std::max(len3(u[0] + v[0], u[1] + v[1], u[2] + v[2]), len3(u[0] - v[0], u[1] - v[1], u[2] - v[2]));
        }
        geom.insert(geom.end(), {c[0], c[1], c[2], rho, weight.back()});
    }
    const int32_t emit_planes = (int32_t)(code.size() - n);
    std::vector<float> ecdf, epmf;
    nee_cdf_of(weight, ecdf, epmf);
    if (n > 0) {
        if (const rt_status st = upload(index, (void **)&sc->nee_index_dev)) return st;
        if (const rt_status st = upload(cdf, (void **)&sc->nee_cdf_dev)) return st;
        if (const rt_status st = upload(pmf, (void **)&sc->nee_pmf_dev)) return st;
    }
    if (emit_planes > 0) {
        if (const rt_status st = upload(code, (void **)&sc->emit_code_dev)) return st;
        if (const rt_status st = upload(ecdf, (void **)&sc->emit_cdf_dev)) return st;
        if (const rt_status st = upload(epmf, (void **)&sc->emit_pmf_dev)) return st;
        if (const rt_status st = upload(area, (void **)&sc->emit_area_dev)) return st;
    }
    sc->emit_code = std::move(code);
    sc->emit_cdf = std::move(ecdf);
    sc->emit_pmf = std::move(epmf);
    sc->emit_area = std::move(area);
    sc->emit_spheres = (int32_t)n;
    sc->emit_planes = emit_planes;
    sc->emit_geom = std::move(geom);
    sc->nee_index = std::move(index);
    sc->nee_cdf = std::move(cdf);
    sc->nee_pmf = std::move(pmf);
    sc->nee_built = true;
    return RT_OK;
}

rtk::NeeTable nee_table_of(const rt_scene *sc, int32_t mis) {
    rtk::NeeTable T;
    T.index = sc->nee_index_dev;
    T.cdf = sc->nee_cdf_dev;
    T.pmf = sc->nee_pmf_dev;
    T.count = (int32_t)sc->nee_index.size();
    T.mis = mis;
    return T;
}
// does a call with these parameters run the two-kind kernels?  Only where the table holds a plane: without one both tables are the same
// and the sphere-only kernels give sample_planes = 0 bit for bit (the tables must have been made: nee_table_ensure)
bool emit_planes_on(const rt_scene *sc, const NeeSetup &N) { return N.planes != 0 && sc->emit_planes > 0; }
rtk::EmitTable emit_table_of(const rt_scene *sc, int32_t mis) {
    rtk::EmitTable T;
    T.code = sc->emit_code_dev;
    T.cdf = sc->emit_cdf_dev;
    T.pmf = sc->emit_pmf_dev;
    T.area = sc->emit_area_dev;
    T.count = (int32_t)sc->emit_code.size();
    T.spheres = sc->emit_spheres;
    T.mis = mis;
    return T;
}


// ---- the light tree (header, "Tree") -----------------------------------------------------------------------------------
// which table a call's parameters select: 1 the two-kind one (it holds a plane), 0 the sphere-only one
int tree_which(const rt_scene *sc, const NeeSetup &N) { return emit_planes_on(sc, N) ? 1 : 0; }
int32_t tree_entries(const rt_scene *sc, int which) { return (int32_t)(which ? sc->emit_code.size() : sc->nee_index.size()); }
// does the call run the tree kernels?  (an empty table samples nothing: the kernels of select = 0; the tables must have been made)
bool tree_on(const rt_scene *sc, const NeeSetup &N) { return N.select == 1 && tree_entries(sc, tree_which(sc, N)) > 0; }

struct TreeBuilder {
    const double *geom;                        // 5 per entry: c0 c1 c2 rho w
    double total;
    std::vector<float> node;
    std::vector<uint32_t> path;
    std::vector<int32_t> depth;
    // the node over list S (reached by `bits` in `level` steps): its index; *weight_out: the double sum of its weights in list order
    int32_t build(std::vector<int32_t> &S, uint32_t bits, int32_t level, double *weight_out) {
        const int32_t id = (int32_t)(node.size() / 8);
        node.resize(node.size() + 8);
        double lo[3], hi[3], clo[3], chi[3], W = 0.0;
        for (size_t k = 0; k < S.size(); ++k) {
            const double *g = geom + 5 * (size_t)S[k];
            for (int a = 0; a < 3; ++a) {
                const double l = g[a] - g[3], h = g[a] + g[3];
                if (k == 0 || l < lo[a]) lo[a] = l;
                if (k == 0 || h > hi[a]) hi[a] = h;
                if (k == 0 || g[a] < clo[a]) clo[a] = g[a];
                if (k == 0 || g[a] > chi[a]) chi[a] = g[a];
            }
            W += g[4];
        }
        double m[3], R = 0.0;
        for (int a = 0; a < 3; ++a) m[a] = 0.5 * (lo[a] + hi[a]);
        for (int32_t e : S) {
            const double *g = geom + 5 * (size_t)e;
            const double dx = g[0] - m[0], dy = g[1] - m[1], dz = g[2] - m[2];
            const double r = std::sqrt((dx * dx + dy * dy) + dz * dz) + g[3];
            if (r > R) R = r;
        }
        float rec[8] = {(float)m[0], (float)m[1], (float)m[2], std::nextafterf((float)R, INFINITY), (float)(W / total), 0.0f, 0.0f, 0.0f};
        int32_t right = -1, entry = -1;
        if (S.size() == 1) {
            entry = S[0];
            path[(size_t)entry] = bits;
            depth[(size_t)entry] = level;
        } else {
            int axis = 0;
            for (int a = 1; a < 3; ++a)
                if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
            std::stable_sort(S.begin(), S.end(), [&](int32_t x, int32_t y) { return geom[5 * (size_t)x + axis] < geom[5 * (size_t)y + axis]; });
            const size_t nl = (S.size() + 1) / 2;
            std::vector<int32_t> L(S.begin(), S.begin() + (ptrdiff_t)nl), Rr(S.begin() + (ptrdiff_t)nl, S.end());
            double wl = 0.0, wr = 0.0;
            build(L, bits, level + 1, &wl);
            right = build(Rr, bits | (1u << level), level + 1, &wr);
            rec[5] = (float)(wl / (wl + wr));
        }
        std::memcpy(&rec[6], &right, 4);
        std::memcpy(&rec[7], &entry, 4);
        std::memcpy(&node[(size_t)id * 8], rec, sizeof(rec));
        if (weight_out) *weight_out = W;
        return id;
    }
};
// the tree of table `which`, built on its first use (the tables must have been made)
rt_status tree_ensure(rt_scene *sc, int which) {
    auto &t = sc->tree[which];
    if (t.built) return RT_OK;
    const int32_t n = tree_entries(sc, which);
    if (n > 0) {
        TreeBuilder B;
        B.geom = sc->emit_geom.data();
        B.total = 0.0;
        for (int32_t e = 0; e < n; ++e) B.total += B.geom[5 * (size_t)e + 4];
        B.path.assign((size_t)n, 0u);
        B.depth.assign((size_t)n, 0);
        std::vector<int32_t> all((size_t)n);
        for (int32_t e = 0; e < n; ++e) all[(size_t)e] = e;
        B.build(all, 0u, 0, nullptr);
        if (const rt_status st = upload(B.node, (void **)&t.node_dev)) return st;
        if (const rt_status st = upload(B.path, (void **)&t.path_dev)) return st;
        if (const rt_status st = upload(B.depth, (void **)&t.depth_dev)) return st;
        t.node = std::move(B.node);
        t.path = std::move(B.path);
        t.depth = std::move(B.depth);
    }
    t.built = true;
    return RT_OK;
}
rtk::LightTree light_tree_of(const rt_scene *sc, int which) {
    rtk::LightTree L;
    L.node = sc->tree[which].node_dev;
    L.path = sc->tree[which].path_dev;
    L.depth = sc->tree[which].depth_dev;
    return L;
}
rtk::TreeTable tree_table_of(const rt_scene *sc, int32_t mis) { return rtk::TreeTable{nee_table_of(sc, mis), light_tree_of(sc, 0)}; }
rtk::TreeEmitTable tree_emit_table_of(const rt_scene *sc, int32_t mis) { return rtk::TreeEmitTable{emit_table_of(sc, mis), light_tree_of(sc, 1)}; }

// Which emitter table a call uses — and so, by the table's type, which kernels: the rule of every lit call, once.  Makes the tables (and
// the tree, where the call selects by it) on their first use and returns f(table), called exactly once: the tree over the two-kind or the
// sphere-only table (tree_on), else the two-kind table (emit_planes_on), else the sphere-only one.  emitters off (rt_lit_params.
// sample_emitters = 0): an empty sphere-only table, and nothing is made.  (extern "C++": a template, among the entry points)
// The order in which f(…) is named below — NeeTable, TreeEmitTable, TreeTable, EmitTable — is the order in which the kernels a call site
// names are instantiated, and so the layout of the device code: reordering these returns moves kernels in the code object.
extern "C++" template <class F>
rt_status with_emitter_table(rt_scene *sc, const NeeSetup &N, bool emitters, F &&f) {
    if (!emitters) return f(rtk::NeeTable{});
    if (const rt_status st = nee_table_ensure(sc)) return st;
    const bool planes = emit_planes_on(sc, N);
    if (tree_on(sc, N)) {
        if (const rt_status st = tree_ensure(sc, planes ? 1 : 0)) return st;
        return planes ? f(tree_emit_table_of(sc, N.mis)) : f(tree_table_of(sc, N.mis));
    }
    return planes ? f(emit_table_of(sc, N.mis)) : f(nee_table_of(sc, N.mis));
}

}  // namespace

rt_status rt_render_nee(rt_scene *sc, const rt_camera_data *cam, const rt_nee_params *params, const rt_shard *shard, int32_t sample_first,
                        float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    NeeSetup N;
    if (const rt_status st = nee_setup("rt_render_nee", params, N)) return st;
    if (!sc) return fail(RT_ERR_INVALID_ARG, "rt_render_nee: null scene");
    auto with_table = [&](auto frame) {
        return with_emitter_table(sc, N, true, [&](const auto &T) {
            using Table = std::decay_t<decltype(T)>;
            return frame(N.glossy ? (const void *)rtk::light_gloss_render_kernel<Table> : (const void *)rtk::light_render_kernel<Table>, &T);
        });
    };
    return render_light_impl("rt_render_nee", nullptr, with_table, sc, cam, shard, sample_first, d_fb_sum, hip_stream, sync, timing);
}

rt_status rt_nee_light_table(rt_scene *sc, int32_t cap, int32_t *sphere_index, float *cdf, float *pmf, int32_t *count) {
    if (!sc || !count || cap < 0 || (cap > 0 && (!sphere_index || !cdf || !pmf))) return fail(RT_ERR_INVALID_ARG, "rt_nee_light_table: null argument or negative cap");
    if (const rt_status st = check_device(sc)) return st;
    if (const rt_status st = nee_table_ensure(sc)) return st;
    const int32_t n = (int32_t)sc->nee_index.size();
    *count = n;
    const int32_t m = cap < n ? cap : n;
    for (int32_t k = 0; k < m; ++k) {
        sphere_index[k] = sc->nee_index[(size_t)k];
        cdf[k] = sc->nee_cdf[(size_t)k];
        pmf[k] = sc->nee_pmf[(size_t)k];
    }
    return RT_OK;
}

rt_status rt_nee_emitter_table(rt_scene *sc, const rt_nee_params *params, int32_t cap, int32_t *kind, int32_t *index, float *cdf, float *pmf,
                               float *area, int32_t *count) {
    NeeSetup N;
    if (const rt_status st = nee_setup("rt_nee_emitter_table", params, N)) return st;
    if (!sc || !count || cap < 0 || (cap > 0 && (!kind || !index || !cdf || !pmf || !area)))
        return fail(RT_ERR_INVALID_ARG, "rt_nee_emitter_table: null argument or negative cap");
    if (const rt_status st = check_device(sc)) return st;
    if (const rt_status st = nee_table_ensure(sc)) return st;
    const bool planes = N.planes != 0;
    const int32_t n = (int32_t)(planes ? sc->emit_code.size() : sc->nee_index.size());
    *count = n;
    const int32_t m = cap < n ? cap : n;
    for (int32_t k = 0; k < m; ++k) {
        kind[k] = planes ? (sc->emit_code[(size_t)k] & 1) : 0;
        index[k] = planes ? (sc->emit_code[(size_t)k] >> 1) : sc->nee_index[(size_t)k];
        cdf[k] = planes ? sc->emit_cdf[(size_t)k] : sc->nee_cdf[(size_t)k];
        pmf[k] = planes ? sc->emit_pmf[(size_t)k] : sc->nee_pmf[(size_t)k];
        area[k] = planes ? sc->emit_area[(size_t)k] : 0.0f;
    }
    return RT_OK;
}

rt_status rt_nee_light_tree(rt_scene *sc, const rt_nee_params *params, int32_t cap_nodes, int32_t cap_entries, float *sphere, float *weight, float *q,
                            int32_t *left, int32_t *right, int32_t *entry, uint32_t *path, int32_t *depth, int32_t *node_count, int32_t *entry_count) {
    NeeSetup N;
    if (const rt_status st = nee_setup("rt_nee_light_tree", params, N)) return st;
    if (!sc || !node_count || !entry_count || cap_nodes < 0 || cap_entries < 0 || (cap_nodes > 0 && (!sphere || !weight || !q || !left || !right || !entry)) ||
        (cap_entries > 0 && (!path || !depth)))
        return fail(RT_ERR_INVALID_ARG, "rt_nee_light_tree: null argument or negative cap");
    if (const rt_status st = check_device(sc)) return st;
    if (const rt_status st = nee_table_ensure(sc)) return st;
    const int which = tree_which(sc, N);
    if (const rt_status st = tree_ensure(sc, which)) return st;
    const auto &t = sc->tree[which];
    const int32_t nn = (int32_t)(t.node.size() / 8), ne = (int32_t)t.path.size();
    *node_count = nn;
    *entry_count = ne;
    for (int32_t k = 0; k < (cap_nodes < nn ? cap_nodes : nn); ++k) {
        const float *rec = &t.node[(size_t)k * 8];
        std::memcpy(sphere + 4 * k, rec, 16);
        weight[k] = rec[4];
        q[k] = rec[5];
        std::memcpy(&right[k], &rec[6], 4);
        std::memcpy(&entry[k], &rec[7], 4);
        left[k] = right[k] >= 0 ? k + 1 : -1;
    }
    for (int32_t k = 0; k < (cap_entries < ne ? cap_entries : ne); ++k) {
        path[k] = t.path[(size_t)k];
        depth[k] = t.depth[(size_t)k];
    }
    return RT_OK;
}

rt_status rt_trace_samples_nee(rt_scene *sc, const rt_camera_data *cam, const rt_nee_params *params, int32_t n, const int32_t *ijs,
                               float *radiance, int32_t *rays, uint32_t *final_seed, uint32_t *final_nee_seed) {
    NeeSetup N;
    if (const rt_status st = nee_setup("rt_trace_samples_nee", params, N)) return st;
    if (n < 0 || (n > 0 && (!ijs || !radiance || !rays || !final_seed || !final_nee_seed))) return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_nee: null argument");
    rtk::KParams P;
    rt_status st = fill_params(sc, cam, nullptr, P);
    if (st != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    return run_probe("rt_trace_samples_nee: ", P, cam, n, ijs, radiance, rays, final_seed, final_nee_seed, nullptr, [&](const rtk::KParams &KP, uint32_t *d_nee, uint32_t *) {
        return with_emitter_table(sc, N, true, [&](const auto &T) {
            using Table = std::decay_t<decltype(T)>;
            if (N.glossy) hipLaunchKernelGGL(rtk::light_gloss_probe_kernel<Table>, dim3((n + 255) / 256), dim3(256), 0, 0, KP, T, d_nee);
            else hipLaunchKernelGGL(rtk::light_probe_kernel<Table>, dim3((n + 255) / 256), dim3(256), 0, 0, KP, T, d_nee);
            return RT_OK;
        });
    });
}

// ---- rt_env / rt_render_env / rt_env_table / rt_env_lookup / rt_trace_samples_env (rtp_amd.h) ---------------------
// An environment: the texels (r, g, b, pj) and both cdf tables on the device it was created on.  The table is built here, on the
// host, in double (the header's sums, in its order) — once per environment.
struct rt_env {
    int device = 0;
    int32_t n = 0;
    bool empty = true;                 // an all-black map: no light samples
    float4 *texels = nullptr;          // n * n
    float *row_cdf = nullptr;          // n
    float *col_cdf = nullptr;          // n * n
};

void rt_env_params_init(rt_env_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
    p->mode = 1;
    p->scale = 1.0f;
    p->rot[0] = p->rot[4] = p->rot[8] = 1.0f;
    p->camera_visible = 1;
}

namespace {
// (u, v) → the octahedron point, in double: the header's decode
void env_decode_d(double u, double v, double p[3]) {
    const double y = (1.0 - std::fabs(u)) - std::fabs(v);
    p[1] = y;
    if (y >= 0.0) {
        p[0] = u;
        p[2] = v;
    } else {
        p[0] = (1.0 - std::fabs(v)) * (u >= 0.0 ? 1.0 : -1.0);
        p[2] = (1.0 - std::fabs(u)) * (v >= 0.0 ? 1.0 : -1.0);
    }
}

// cdf_i = (float)(prefix / total), the last one 1, over n weights; a total of 0 gives zeros
void env_cdf(const double *w, int32_t n, double total, float *cdf) {
    double run = 0.0;
    for (int32_t k = 0; k < n; ++k) {
        run += w[k];
        cdf[k] = total > 0.0 ? (k + 1 == n ? 1.0f : (float)(run / total)) : 0.0f;
    }
}

rt_status env_setup(const char *what, const rt_env_params *params, rt_env_params &np) {
    const std::string w(what);
    rt_env_params_init(&np);
    if (const rt_status st = take_params(w, "rt_env_params", params, np)) return st;
    if (np.mode < 0 || np.mode > 2) return fail(RT_ERR_INVALID_ARG, w + ": mode must be 0, 1 or 2");
    if (!(std::isfinite(np.scale) && np.scale >= 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": scale must be finite and not negative");
    if (np.camera_visible != 0 && np.camera_visible != 1) return fail(RT_ERR_INVALID_ARG, w + ": camera_visible must be 0 or 1");
    if (np.glossy != 0 && np.glossy != 1) return fail(RT_ERR_INVALID_ARG, w + ": glossy must be 0 or 1");
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (double)np.rot[3 * a + k] * (double)np.rot[3 * b + k];
            if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-4)) return fail(RT_ERR_INVALID_ARG, w + ": the rows of rot are not orthonormal");
        }
    return RT_OK;
}

rt_status env_check(const char *what, const rt_env *env) {
    if (!env) return fail(RT_ERR_INVALID_ARG, std::string(what) + ": null environment");
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return fail(RT_ERR_HIP, "hipGetDevice failed");
    if (cur != env->device) return fail(RT_ERR_INVALID_ARG, std::string(what) + ": the environment was created on another device than the calling thread's current one");
    return RT_OK;
}

rtk::EnvDev env_dev_of(const rt_env *env, const rt_env_params &np) {
    rtk::EnvDev E;
    E.texels = env->texels;
    E.row_cdf = env->row_cdf;
    E.col_cdf = env->col_cdf;
    E.n = env->n;
    E.sampled = (np.mode != 0 && !env->empty) ? 1 : 0;
    E.mis = np.mode == 1 ? 1 : 0;
    E.camera_visible = np.camera_visible;
    E.scale = np.scale;
    for (int k = 0; k < 9; ++k) E.rot[k] = np.rot[k];
    E.dens = ((float)env->n * (float)env->n) * 0.25f;
    E.h = 2.0f / (float)env->n;
    return E;
}
}  // namespace

rt_status rt_env_create(const float *rgb, int32_t n, rt_env **out_env) {
    if (!rgb || !out_env) return fail(RT_ERR_INVALID_ARG, "rt_env_create: null argument");
    *out_env = nullptr;
    if (n < 1 || n > RT_ENV_MAX_N) return fail(RT_ERR_INVALID_ARG, "rt_env_create: n must be 1 … " + std::to_string(RT_ENV_MAX_N));
    const size_t nn = (size_t)n * (size_t)n;
    for (size_t k = 0; k < nn * 3; ++k)
        if (!(std::isfinite(rgb[k]) && rgb[k] >= 0.0f)) return fail(RT_ERR_INVALID_ARG, "rt_env_create: a texel is negative, NaN or infinite");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RT_ERR_NO_DEVICE, "rt_env_create: no current HIP device");
    }
    // texel weights (radiance x solid angle) and the rows' sums, in double
    std::vector<double> w(nn), row_w((size_t)n);
    const double cell = (2.0 / (double)n) * (2.0 / (double)n);
    double total = 0.0;
    for (int32_t iy = 0; iy < n; ++iy) {
        const double vc = -1.0 + (double)(2 * iy + 1) / (double)n;
        double row = 0.0;
        for (int32_t ix = 0; ix < n; ++ix) {
            const double uc = -1.0 + (double)(2 * ix + 1) / (double)n;
            double p[3];
            env_decode_d(uc, vc, p);
            const double l2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
            const float *t = rgb + ((size_t)iy * n + ix) * 3;
            const double wt = (((double)t[0] + (double)t[1]) + (double)t[2]) * (cell / (l2 * std::sqrt(l2)));
            w[(size_t)iy * n + ix] = wt;
            row += wt;
        }
        row_w[(size_t)iy] = row;
        total += row;
    }
    std::vector<float> row_cdf((size_t)n), col_cdf(nn);
    env_cdf(row_w.data(), n, total, row_cdf.data());
    for (int32_t iy = 0; iy < n; ++iy) env_cdf(w.data() + (size_t)iy * n, n, total > 0.0 ? row_w[(size_t)iy] : 0.0, col_cdf.data() + (size_t)iy * n);
    std::vector<float4> texels(nn);
    for (int32_t iy = 0; iy < n; ++iy) {
        const float rp = row_cdf[(size_t)iy] - (iy == 0 ? 0.0f : row_cdf[(size_t)iy - 1]);
        for (int32_t ix = 0; ix < n; ++ix) {
            const size_t k = (size_t)iy * n + ix;
            const float cp = col_cdf[k] - (ix == 0 ? 0.0f : col_cdf[k - 1]);
            texels[k] = make_float4(rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2], rp * cp);
        }
    }
    rt_env *env = new (std::nothrow) rt_env();
    if (!env) return fail(RT_ERR_OUT_OF_MEMORY, "rt_env_create: out of host memory");
    env->device = dev;
    env->n = n;
    env->empty = !(total > 0.0);
    rt_status st = upload(texels, (void **)&env->texels);
    if (st == RT_OK) st = upload(row_cdf, (void **)&env->row_cdf);
    if (st == RT_OK) st = upload(col_cdf, (void **)&env->col_cdf);
    if (st != RT_OK) {
        (void)rt_env_destroy(env);
        return st;
    }
    *out_env = env;
    return RT_OK;
}

rt_status rt_env_destroy(rt_env *env) {
    if (!env) return RT_OK;
    (void)hipFree(env->texels);
    (void)hipFree(env->row_cdf);
    (void)hipFree(env->col_cdf);
    delete env;
    return RT_OK;
}

rt_status rt_env_table(const rt_env *env, int32_t row, float *row_cdf, float *row_pmf, float *col_cdf, float *col_pmf, int32_t *count) {
    if (const rt_status st = env_check("rt_env_table", env)) return st;
    const int32_t n = env->n;
    if (row < 0 || row >= n) return fail(RT_ERR_INVALID_ARG, "rt_env_table: row out of range");
    std::vector<float> r((size_t)n), c((size_t)n);
    HIP_TRY(hipMemcpy(r.data(), env->row_cdf, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c.data(), env->col_cdf + (size_t)row * n, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (int32_t k = 0; k < n; ++k) {
        if (row_cdf) row_cdf[k] = r[(size_t)k];
        if (row_pmf) row_pmf[k] = r[(size_t)k] - (k == 0 ? 0.0f : r[(size_t)k - 1]);
        if (col_cdf) col_cdf[k] = c[(size_t)k];
        if (col_pmf) col_pmf[k] = c[(size_t)k] - (k == 0 ? 0.0f : c[(size_t)k - 1]);
    }
    if (count) *count = env->empty ? 0 : n;
    return RT_OK;
}

rt_status rt_env_lookup(const rt_env *env, int32_t n, const float *directions, int32_t *texel, float *radiance, float *pl) {
    if (n < 0 || (n > 0 && (!directions || !texel || !radiance || !pl))) return fail(RT_ERR_INVALID_ARG, "rt_env_lookup: null argument or negative count");
    if (const rt_status st = env_check("rt_env_lookup", env)) return st;
    if (n == 0) return RT_OK;
    float *d_dir = nullptr, *d_rad = nullptr, *d_pl = nullptr;
    int32_t *d_tex = nullptr;
    Scratch mem;
    HIP_TRY(mem.alloc(d_dir, (size_t)n * 12));
    HIP_TRY(mem.alloc(d_rad, (size_t)n * 12));
    HIP_TRY(mem.alloc(d_pl, (size_t)n * 4));
    HIP_TRY(mem.alloc(d_tex, (size_t)n * 4));
    HIP_TRY(hipMemcpy(d_dir, directions, (size_t)n * 12, hipMemcpyHostToDevice));
    rt_env_params np;
    rt_env_params_init(&np);
    const rtk::EnvDev E = env_dev_of(env, np);
    hipLaunchKernelGGL(rtk::env_lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, E, n, (const float *)d_dir, d_tex, d_rad, d_pl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(texel, d_tex, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(radiance, d_rad, (size_t)n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pl, d_pl, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_env_from_equirect(const float *rgb, int32_t w, int32_t h, int32_t n, float *out) {
    if (!rgb || !out || w < 1 || h < 1 || n < 1 || n > RT_ENV_MAX_N) return fail(RT_ERR_INVALID_ARG, "rt_env_from_equirect: null argument or size out of range");
    const int sub = 4;
    const double pi = 3.14159265358979323846;
    for (int32_t iy = 0; iy < n; ++iy)
        for (int32_t ix = 0; ix < n; ++ix) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int b = 0; b < sub; ++b)
                for (int a = 0; a < sub; ++a) {
                    const double u = -1.0 + 2.0 * ((double)ix + ((double)a + 0.5) / sub) / (double)n;
                    const double v = -1.0 + 2.0 * ((double)iy + ((double)b + 0.5) / sub) / (double)n;
                    double p[3];
                    env_decode_d(u, v, p);
                    const double len = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
                    const double theta = std::acos(std::fmin(1.0, std::fmax(-1.0, p[1] / len)));
                    const double phi = std::atan2(-p[2], p[0]) + pi;
                    int32_t px = (int32_t)(phi / (2.0 * pi) * (double)w), py = (int32_t)(theta / pi * (double)h);
                    px = px < 0 ? 0 : (px >= w ? w - 1 : px);
                    py = py < 0 ? 0 : (py >= h ? h - 1 : py);
                    const float *t = rgb + ((size_t)py * w + px) * 3;
                    for (int c = 0; c < 3; ++c) acc[c] += (double)t[c];
                }
            for (int c = 0; c < 3; ++c) out[((size_t)iy * n + ix) * 3 + c] = (float)(acc[c] / (double)(sub * sub));
        }
    return RT_OK;
}

rt_status rt_render_env(rt_scene *sc, const rt_camera_data *cam, const rt_env *env, const rt_env_params *params, const rt_shard *shard,
                        int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    rt_env_params np;
    if (const rt_status st = env_setup("rt_render_env", params, np)) return st;
    if (!env) return fail(RT_ERR_INVALID_ARG, "rt_render_env: null environment");
    if (!sc) return fail(RT_ERR_INVALID_ARG, "rt_render_env: null scene");
    auto with_env = [&](auto frame) {
        const rtk::EnvDev E = env_dev_of(env, np);
        return frame(np.glossy ? (const void *)rtk::light_gloss_render_kernel<rtk::EnvDev> : (const void *)rtk::light_render_kernel<rtk::EnvDev>, &E);
    };
    return render_light_impl("rt_render_env", &env->device, with_env, sc, cam, shard, sample_first, d_fb_sum, hip_stream, sync, timing);
}

rt_status rt_trace_samples_env(rt_scene *sc, const rt_camera_data *cam, const rt_env *env, const rt_env_params *params, int32_t n,
                               const int32_t *ijs, float *radiance, int32_t *rays, uint32_t *final_seed, uint32_t *final_env_seed) {
    rt_env_params np;
    if (const rt_status st = env_setup("rt_trace_samples_env", params, np)) return st;
    if (!env) return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_env: null environment");
    if (n < 0 || (n > 0 && (!ijs || !radiance || !rays || !final_seed || !final_env_seed))) return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_env: null argument");
    rtk::KParams P;
    rt_status st = fill_params(sc, cam, nullptr, P);
    if (st != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    if (env->device != sc->device) return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_env: the environment was created on another device than the scene");
    return run_probe("rt_trace_samples_env: ", P, cam, n, ijs, radiance, rays, final_seed, final_env_seed, nullptr, [&](const rtk::KParams &KP, uint32_t *d_env, uint32_t *) {
        if (np.glossy) hipLaunchKernelGGL(rtk::light_gloss_probe_kernel<rtk::EnvDev>, dim3((n + 255) / 256), dim3(256), 0, 0, KP, env_dev_of(env, np), d_env);
        else hipLaunchKernelGGL(rtk::light_probe_kernel<rtk::EnvDev>, dim3((n + 255) / 256), dim3(256), 0, 0, KP, env_dev_of(env, np), d_env);
        return RT_OK;
    });
}

// ---- rt_render_lit / rt_trace_samples_lit (rtp_amd.h): emitters, environment and lens in one frame -------------------
void rt_lit_params_init(rt_lit_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
    p->sample_emitters = 1;
}

namespace {
// What a lit call is made of, after the checks of its three components in their order (lens, emitters, environment)
struct LitSetup {
    rtk::LensCam C;
    bool lens = false;            // the camera draws more than the pinhole's: the kLens kernels
    bool emitters = true;
    NeeSetup nee;
    const rt_env *env = nullptr;
    rt_env_params ep;
};
rt_status lit_setup(const char *what, const rt_camera_data *cam_open, const rt_lit_params *lit, LitSetup &S) {
    rt_lit_params lp;
    rt_lit_params_init(&lp);
    if (const rt_status st = take_params(what, "rt_lit_params", lit, lp)) return st;
    if (lp.sample_emitters != 0 && lp.sample_emitters != 1) return fail(RT_ERR_INVALID_ARG, std::string(what) + ": sample_emitters must be 0 or 1");
    if (const rt_status st = lens_setup(what, cam_open, lp.cam_close, lp.lens, S.C)) return st;
    S.lens = S.C.motion != 0 || S.C.radius > 0.0f;
    S.emitters = lp.sample_emitters != 0;
    if (S.emitters)
        if (const rt_status st = nee_setup(what, lp.nee, S.nee)) return st;
    S.env = lp.env;
    if (S.env)
        if (const rt_status st = env_setup(what, lp.env_params, S.ep)) return st;
    return RT_OK;
}
// The kernels' light: the call's emitter table (with_emitter_table; emitters off: an empty one) and the environment (none: off).
// Returns f(light), light a Lit<Table> of the table's type — a GlossLit<Table> when a light's glossy switch is on
extern "C++" template <class F>
rt_status with_lit(rt_scene *sc, const LitSetup &S, F &&f) {
    return with_emitter_table(sc, S.nee, S.emitters, [&](const auto &table) {
        using Table = std::decay_t<decltype(table)>;
        auto fill = [&](rtk::Lit<Table> &T) {
            T.N = table;
            if (S.env) {
                T.E = env_dev_of(S.env, S.ep);
                T.env_on = 1;
            }
        };
        const int32_t gn = S.emitters && S.nee.glossy ? 1 : 0, ge = S.env && S.ep.glossy ? 1 : 0;
        if (gn || ge) {
            rtk::GlossLit<Table> G{};
            fill(G);
            G.gn = gn;
            G.ge = ge;
            return f(G);
        }
        rtk::Lit<Table> T{};
        fill(T);
        return f(T);
    });
}
// the frame kernel of a lit light (any of the four types) from the call's camera, and its list variant
struct LitKernels {
    const void *frame, *list;
};
extern "C++" template <class Light>
LitKernels lit_kernels_of(bool lens, const Light &T) {
    if (lens) return {rtk::lit_frame_kernel_of<true>(T), rtk::lit_list_kernel_of<true>(T)};
    return {rtk::lit_frame_kernel_of<false>(T), rtk::lit_list_kernel_of<false>(T)};
}
}  // namespace

rt_status rt_render_lit(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_shard *shard, int32_t sample_first,
                        float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    LitSetup S;
    if (const rt_status st = lit_setup("rt_render_lit", cam_open, lit, S)) return st;
    if (!sc) return fail(RT_ERR_INVALID_ARG, "rt_render_lit: null scene");
    auto with_light = [&](auto frame) { return with_lit(sc, S, [&](const auto &T) { return frame(lit_kernels_of(S.lens, T).frame, &T); }); };
    return render_light_impl("rt_render_lit", S.env ? &S.env->device : nullptr, with_light, sc, cam_open, shard, sample_first, d_fb_sum, hip_stream, sync, timing,
                             &S.C);
}

// ---- rt_render_lit_adaptive (rtp_amd.h): rt_render_adaptive's rule and rounds on rt_render_lit's estimator.  The min_spp
// frame is render_light_impl's passes with the moments; the rounds are rt_render_adaptive's (adaptive_rounds) with the list variant of
// the frame's kernel as their trace launch.  Every round is enqueued up front; the light is made once.
namespace {
// The adaptive lit calls from their frame prologue on (rt_render_lit_adaptive_prior, rt_render_volume_adaptive): the caller has made its
// parameter checks, down to the null scene.  with_light(f) makes the call's light once and returns f(frame kernel, its list variant,
// &light); `what` starts every refusal.
extern "C++" template <class WithLight>
rt_status lit_adaptive_run(const char *what, rt_scene *sc, const rt_camera_data *cam_open, const LitSetup &S, const rt_adaptive_params &a, int32_t rule,
                           const float *d_prior, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp, float *d_moments,
                           void *hip_stream, int32_t sync, rt_timing *timing, WithLight &&with_light) {
    rt_status st;
    const int32_t batch = a.batch_spp, rounds = (a.max_spp - a.min_spp) / a.batch_spp;
    rt_camera_data base = *cam_open;
    base.samples_per_pixel = a.min_spp;
    Frame F;
    st = frame_prologue(what, sc, &base, shard, nullptr, sample_first, S.env ? &S.env->device : nullptr, nullptr, hip_stream, timing, F, [&] {
        if (rounds > 0 && (uint64_t)F.num_pixels * (uint64_t)batch >= (1ull << 31) - 4096)
            return fail(RT_ERR_UNSUPPORTED, std::string(what) + ": pixels x batch_spp beyond the work index arithmetic");
        return refuse_retired(sc->cfg);
    });
    if (st != RT_OK) return st;
    if (F.nothing_to_do()) return RT_OK;
    rtk::KParams &P = F.P;
    const hipStream_t stream = F.stream;
    const uint32_t num_pixels = F.num_pixels;

    // ---- 2. the handle's buffers (rt_render_adaptive's: a handle renders one frame at a time) and a slab for the frame's passes — the
    // frame's slab first: reserve_slab may free and shorten the slab, the batch's grow after it cannot
    float *mom;
    if ((st = adaptive_moments(sc, num_pixels, d_moments, stream, mom)) != RT_OK) return st;
    if (P.max_depth <= 0) {
        HIP_TRY(hipMemsetAsync(d_fb_sum, 0, (size_t)num_pixels * 3 * sizeof(float), stream));
        if ((st = adaptive_no_depth(a, mom, d_spp, num_pixels, stream)) != RT_OK) return st;
        if (sync) HIP_TRY(hipStreamSynchronize(stream));
        return RT_OK;
    }
    rtaccel::PassPlan passes;
    if ((st = reserve_slab(sc, num_pixels, a.min_spp, stream, passes)) != RT_OK) return st;
    if ((st = adaptive_reserve(sc, num_pixels, rounds, batch, rule, stream)) != RT_OK) return st;

    // ---- 3. the light, once, and the two kernels it needs: the frame's and its list variant
    return with_light([&](const void *frame_kernel, const void *list_kernel, const auto *light) -> rt_status {
        const auto &T = *light;
        rt_timing t{};
        kernel_resources(rounds > 0 ? list_kernel : frame_kernel, t.trace_vgprs, t.trace_scratch_bytes);
        CallClock &clock = sc->clock[kClockLight];
        if ((st = clock.make(kMaxPasses)) != RT_OK) return st;
        HIP_TRY(hipMemsetAsync(clock.words, 0, kMaxPasses * 4, stream));
        if ((st = clock.start(stream)) != RT_OK) return st;

        // ---- 4. the min_spp frame: rt_render_lit's passes, with the moments
        P.fb = d_fb_sum;
        bind_slab(sc, P, num_pixels, passes.pass_size);
        if ((st = light_passes(frame_kernel, &T, &S.C, P, passes, num_pixels, sample_first, sc->num_cus * light_wgs_per_cu(frame_kernel), clock.words, stream, mom,
                               t.num_workgroups)) != RT_OK)
            return st;

        // ---- 5. every pixel is judged; then the rounds, on a list whose length only the device knows (the grid: for the worst case —
        // every pixel goes on)
        int grid = 0;
        if (rounds > 0) {
            grid = light_grid(sc->num_cus * light_wgs_per_cu(list_kernel), num_pixels * (uint32_t)batch);
            t.num_workgroups = (uint32_t)grid;
        }
        st = adaptive_rounds(sc, a, rule, P, mom, d_prior, d_spp, num_pixels, sample_first + a.min_spp, stream,
                             [&](const rtk::KParams &KP) { return launch(list_kernel, (uint32_t)rtk::kLightBlock, grid, 0, stream, KP, &T, &S.C); });
        if (st != RT_OK) return st;
        if ((st = clock.stop(stream)) != RT_OK) return st;
        t.workgroup_size = (uint32_t)rtk::kLightBlock;
        t.trace_launches = (uint32_t)(passes.passes + rounds);
        t.kernel = RT_KERNEL_MEGA;
        t.traced_samples = (uint64_t)num_pixels * (uint64_t)a.min_spp;          // (the rounds': the sum of d_spp, which only the device knows)
        t.guard_paused = sc->guard_paused ? 1u : 0u;
        if (sync) {
            if ((st = clock.elapsed(t.kernel_ms)) != RT_OK) return st;
        }
        timing_out(t, timing);
        return RT_OK;
    });
}
}  // namespace

rt_status rt_render_lit_adaptive_prior(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_adaptive_params *params,
                                       const rt_stop_params *stop, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp,
                                       float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing, const float *d_prior) {
    // every check before anything is enqueued
    const char *what = "rt_render_lit_adaptive";
    rt_adaptive_params a;
    int32_t rule;
    rt_status st = adaptive_check(what, params, a);
    if (st != RT_OK) return st;
    if ((st = stop_check(what, stop, rule)) != RT_OK) return st;
    if ((st = prior_check("rt_render_lit_adaptive_prior", d_prior, cam_open, shard, d_fb_sum, d_spp, d_moments)) != RT_OK) return st;
    LitSetup S;
    if ((st = lit_setup(what, cam_open, lit, S)) != RT_OK) return st;
    if ((st = check_sample_range(what, sample_first, a.min_spp + (a.max_spp - a.min_spp) / a.batch_spp * a.batch_spp)) != RT_OK) return st;
    if (!d_fb_sum || !d_spp) return fail(RT_ERR_INVALID_ARG, "rt_render_lit_adaptive: null framebuffer or sample counts");
    if (!sc) return fail(RT_ERR_INVALID_ARG, "rt_render_lit_adaptive: null scene");
    return lit_adaptive_run(what, sc, cam_open, S, a, rule, d_prior, shard, sample_first, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing, [&](auto run) {
        return with_lit(sc, S, [&](const auto &T) { return run(lit_kernels_of(S.lens, T).frame, lit_kernels_of(S.lens, T).list, &T); });
    });
}

rt_status rt_render_lit_adaptive_rule(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_adaptive_params *params,
                                      const rt_stop_params *stop, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp,
                                      float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing) {
    return rt_render_lit_adaptive_prior(sc, cam_open, lit, params, stop, shard, sample_first, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing, nullptr);
}

rt_status rt_render_lit_adaptive(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_adaptive_params *params,
                                 const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream,
                                 int32_t sync, rt_timing *timing) {
    return rt_render_lit_adaptive_rule(sc, cam_open, lit, params, nullptr, shard, sample_first, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing);
}

// The probe of the stopping rules (rtp_amd.h): one judgement over caller-made moments and a going-on mask, through adaptive_judge — the
// launches of the rounds.  Test infrastructure: it allocates, copies and waits.
// (what: the call's name, which every refusal starts with; d_prior: rt_adaptive_judge_prior's, null for none)
static rt_status judge_impl(const char *what, int32_t width, int32_t rows, const rt_shard *shard, const rt_adaptive_params *params,
                            const rt_stop_params *stop, int32_t n, const float *d_moments, const uint8_t *d_going_on_in, uint8_t *d_goes_on_out,
                            void *hip_stream, const float *d_prior) {
    const std::string w(what);
    rt_adaptive_params a;
    int32_t rule;
    rt_status st = adaptive_check(what, params, a);
    if (st != RT_OK) return st;
    if (stop) {
        if (stop->struct_bytes < 8) return fail(RT_ERR_INVALID_ARG, w + ": rt_stop_params struct_bytes below 8");
        if (stop->rule != 0 && stop->rule != 1) return fail(RT_ERR_INVALID_ARG, w + ": rule outside 0 … 1");
    }
    rule = stop ? stop->rule : 0;
    if (width < 1 || rows < 1) return fail(RT_ERR_INVALID_ARG, w + ": width or rows below 1");
    if ((uint64_t)width * (uint64_t)rows > (1u << 24)) return fail(RT_ERR_UNSUPPORTED, w + ": more than 2^24 pixels");
    if (n < 2) return fail(RT_ERR_INVALID_ARG, w + ": n below 2");
    if (shard && shard->num_parts > 1 && (shard->part < 0 || shard->part >= shard->num_parts || shard->band_rows <= 0))
        return fail(RT_ERR_INVALID_ARG, w + ": bad shard");
    if (!d_moments || !d_goes_on_out) return fail(RT_ERR_INVALID_ARG, w + ": null moments or output");
    const hipStream_t stream = (hipStream_t)hip_stream;
    const uint32_t num_pixels = (uint32_t)width * (uint32_t)rows;
    if (d_prior && (uintptr_t)d_prior < (uintptr_t)d_goes_on_out + num_pixels && (uintptr_t)d_goes_on_out < (uintptr_t)d_prior + (uintptr_t)num_pixels * 8)
        return fail(RT_ERR_INVALID_ARG, w + ": d_prior overlaps d_goes_on_out");
    rt_shard s;
    normalise_shard(shard, rows, s);
    const rtk::AdaptWindow W = adapt_window(width, rows, s.band_rows, s.num_parts);
    // the pixels going on, as the list a round would hand on (null mask, or every byte set: every pixel — the first judgement's launch)
    std::vector<uint8_t> mask(num_pixels, 1);
    if (d_going_on_in) {
        HIP_TRY(hipMemcpyAsync(mask.data(), d_going_on_in, num_pixels, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    std::vector<uint32_t> list;
    for (uint32_t q = 0; q < num_pixels; ++q)
        if (mask[q]) list.push_back(q);
    const bool all = list.size() == num_pixels;
    // one allocation: list in, list out, two counters, counts, flags
    uint32_t *words = nullptr;
    const size_t num_words = (size_t)num_pixels * 3 + 2;
    HIP_TRY(hipMalloc((void **)&words, num_words * sizeof(uint32_t) + num_pixels));
    uint32_t *list_in = words, *list_out = words + num_pixels, *counts = words + 2 * (size_t)num_pixels;
    int32_t *spp = (int32_t *)(counts + 2);
    uint8_t *flag = (uint8_t *)(words + num_words);
    const uint32_t host_counts[2] = {(uint32_t)list.size(), 0u};
    auto body = [&]() -> rt_status {
        HIP_TRY(hipMemsetAsync(words, 0, num_words * sizeof(uint32_t) + num_pixels, stream));
        if (!list.empty()) HIP_TRY(hipMemcpyAsync(list_in, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(counts, host_counts, sizeof(host_counts), hipMemcpyHostToDevice, stream));
        if ((st = adaptive_judge(a, rule, d_moments, d_prior, spp, flag, W, num_pixels, all ? nullptr : list_in, all ? nullptr : counts, list_out, counts + 1, n,
                                 stream)) != RT_OK)
            return st;
        uint32_t kept = 0;
        HIP_TRY(hipMemcpyAsync(&kept, counts + 1, sizeof(kept), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (kept > num_pixels) return fail(RT_ERR_HIP, w + ": the list is longer than the image");
        std::vector<uint32_t> out(kept);
        if (kept) HIP_TRY(hipMemcpyAsync(out.data(), list_out, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        std::fill(mask.begin(), mask.end(), (uint8_t)0);
        for (const uint32_t q : out) {
            if (q >= num_pixels) return fail(RT_ERR_HIP, w + ": a listed pixel outside the image");
            mask[q] = 1;
        }
        HIP_TRY(hipMemcpyAsync(d_goes_on_out, mask.data(), num_pixels, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return RT_OK;
    };
    st = body();
    (void)hipFree(words);
    return st;
}
rt_status rt_adaptive_judge(int32_t width, int32_t rows, const rt_shard *shard, const rt_adaptive_params *params, const rt_stop_params *stop, int32_t n,
                            const float *d_moments, const uint8_t *d_going_on_in, uint8_t *d_goes_on_out, void *hip_stream) {
    return judge_impl("rt_adaptive_judge", width, rows, shard, params, stop, n, d_moments, d_going_on_in, d_goes_on_out, hip_stream, nullptr);
}
rt_status rt_adaptive_judge_prior(int32_t width, int32_t rows, const rt_shard *shard, const rt_adaptive_params *params, const rt_stop_params *stop,
                                  int32_t n, const float *d_moments, const uint8_t *d_going_on_in, uint8_t *d_goes_on_out, void *hip_stream,
                                  const float *d_prior) {
    return judge_impl("rt_adaptive_judge_prior", width, rows, shard, params, stop, n, d_moments, d_going_on_in, d_goes_on_out, hip_stream, d_prior);
}

rt_status rt_trace_samples_lit(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, int32_t n, const int32_t *ijs, float *radiance,
                               int32_t *rays, uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed) {
    LitSetup S;
    if (const rt_status st = lit_setup("rt_trace_samples_lit", cam_open, lit, S)) return st;
    if (n < 0 || (n > 0 && (!ijs || !radiance || !rays || !final_seed || !final_nee_seed || !final_env_seed)))
        return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_lit: null argument");
    rtk::KParams P;
    rt_status st = fill_params(sc, cam_open, nullptr, P);
    if (st != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    if (S.env && S.env->device != sc->device) return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_lit: the environment was created on another device than the scene");
    return run_probe("rt_trace_samples_lit: ", P, cam_open, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed,
                     [&](const rtk::KParams &KP, uint32_t *d_nee, uint32_t *d_env) {
        return with_lit(sc, S, [&](const auto &T) {
            using Table = decltype(T.N);
            const dim3 grid((n + 255) / 256), block(256);
            if constexpr (rtk::kLitGlossy<std::decay_t<decltype(T)>>) {
                if (S.lens) hipLaunchKernelGGL((rtk::lit_gloss_probe_kernel<true, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env);
                else hipLaunchKernelGGL((rtk::lit_gloss_probe_kernel<false, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env);
            } else {
                if (S.lens) hipLaunchKernelGGL((rtk::lit_probe_kernel<true, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env);
                else hipLaunchKernelGGL((rtk::lit_probe_kernel<false, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env);
            }
            return RT_OK;
        });
    });
}

// ---- rt_render_lit_split / rt_trace_samples_lit_split (rtp_amd.h): rt_render_lit's sample in two components.  The frame
// is render_light_impl's with two slabs side by side in the handle's one (the second is an argument of the split kernels alone: KParams is
// what it was) and an accumulate per component.
rt_status rt_render_lit_split(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_shard *shard, int32_t sample_first,
                              float *d_direct_sum, float *d_indirect_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    const char *what = "rt_render_lit_split";
    LitSetup S;
    if (const rt_status st = lit_setup(what, cam_open, lit, S)) return st;
    if (!sc) return fail(RT_ERR_INVALID_ARG, "rt_render_lit_split: null scene");
    Frame F;
    rt_status st = frame_prologue(what, sc, cam_open, shard, nullptr, sample_first, S.env ? &S.env->device : nullptr, nullptr, hip_stream, timing, F, [&]() -> rt_status {
        if (const rt_status late = refuse_retired(sc->cfg)) return late;
        if (!d_direct_sum || !d_indirect_sum) return fail(RT_ERR_INVALID_ARG, "rt_render_lit_split: null framebuffer");
        const uintptr_t a = (uintptr_t)d_direct_sum, b = (uintptr_t)d_indirect_sum, bytes = (uintptr_t)F.num_pixels * 12;
        if (a == b || (a < b + bytes && b < a + bytes)) return fail(RT_ERR_INVALID_ARG, "rt_render_lit_split: d_direct_sum and d_indirect_sum overlap");
        return RT_OK;
    });
    if (st != RT_OK) return st;
    if (F.nothing_to_do()) return RT_OK;
    rtk::KParams &P = F.P;
    const hipStream_t stream = F.stream;
    const uint32_t num_pixels = F.num_pixels;
    if (P.spp <= 0 || P.max_depth <= 0) {
        HIP_TRY(hipMemsetAsync(d_direct_sum, 0, (size_t)num_pixels * 3 * sizeof(float), stream));
        return blank_frame(d_indirect_sum, F, sync);
    }
    return with_lit(sc, S, [&](const auto &T) -> rt_status {
        const void *kernel = S.lens ? rtk::lit_split_kernel_of<true>(T) : rtk::lit_split_kernel_of<false>(T);
        rtaccel::PassPlan passes;
        if ((st = reserve_slab(sc, num_pixels, P.spp, stream, passes, 2)) != RT_OK) return st;
        bind_slab(sc, P, num_pixels, passes.pass_size);
        P.fb = d_direct_sum;
        float *second = sc->slab + (size_t)num_pixels * (size_t)P.slab_pitch * 3;
        rtk::KParams Q = P;          // the indirect component's accumulate: the second slab into its own sums
        const int wgs = sc->num_cus * light_wgs_per_cu(kernel);
        rt_timing t{};
        kernel_resources(kernel, t.trace_vgprs, t.trace_scratch_bytes);
        CallClock &clock = sc->clock[kClockLight];
        if ((st = clock.make(kMaxPasses)) != RT_OK) return st;
        HIP_TRY(hipMemsetAsync(clock.words, 0, kMaxPasses * 4, stream));
        if ((st = clock.start(stream)) != RT_OK) return st;
        for (int pass = 0; pass < passes.passes; ++pass) {
            if ((st = set_pass(P, passes, pass, num_pixels, sample_first)) != RT_OK) return st;
            P.queue = clock.words + pass;
            const int grid = light_grid(wgs, P.total_work);
            HIP_TRY(launch(kernel, (uint32_t)rtk::kLightBlock, grid, 0, stream, P, &T, &S.C, &second));
            Q = P;
            Q.fb = d_indirect_sum;
            Q.slab = second;
            launch_accumulate(stream, P, Acc::every_pixel(pass));
            launch_accumulate(stream, Q, Acc::every_pixel(pass));
            HIP_TRY(hipGetLastError());
            if (pass == 0) t.num_workgroups = (uint32_t)grid;
        }
        if ((st = clock.stop(stream)) != RT_OK) return st;
        t.workgroup_size = (uint32_t)rtk::kLightBlock;
        t.trace_launches = (uint32_t)passes.passes;
        t.kernel = RT_KERNEL_MEGA;
        t.traced_samples = (uint64_t)num_pixels * (uint64_t)P.spp;
        t.guard_paused = sc->guard_paused ? 1u : 0u;
        if (sync) {
            if ((st = clock.elapsed(t.kernel_ms)) != RT_OK) return st;
            t.trace_ms = t.kernel_ms;
        }
        timing_out(t, timing);
        return RT_OK;
    });
}

rt_status rt_trace_samples_lit_split(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, int32_t n, const int32_t *ijs, float *direct,
                                     float *indirect, int32_t *rays, uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed) {
    LitSetup S;
    if (const rt_status st = lit_setup("rt_trace_samples_lit_split", cam_open, lit, S)) return st;
    if (n < 0 || (n > 0 && (!ijs || !direct || !indirect || !rays || !final_seed || !final_nee_seed || !final_env_seed)))
        return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_lit_split: null argument");
    rtk::KParams P;
    rt_status st = fill_params(sc, cam_open, nullptr, P);
    if (st != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    if (S.env && S.env->device != sc->device)
        return fail(RT_ERR_INVALID_ARG, "rt_trace_samples_lit_split: the environment was created on another device than the scene");
    float *d_indirect = nullptr;
    Scratch mem;
    if (n > 0 && mem.alloc(d_indirect, (size_t)n * 12) != hipSuccess) return fail(RT_ERR_OUT_OF_MEMORY, "rt_trace_samples_lit_split: hipMalloc failed");
    st = run_probe("rt_trace_samples_lit_split: ", P, cam_open, n, ijs, direct, rays, final_seed, final_nee_seed, final_env_seed,
                   [&](const rtk::KParams &KP, uint32_t *d_nee, uint32_t *d_env) {
        return with_lit(sc, S, [&](const auto &T) {
            using Table = decltype(T.N);
            const dim3 grid((n + 255) / 256), block(256);
            if constexpr (rtk::kLitGlossy<std::decay_t<decltype(T)>>) {
                if (S.lens) hipLaunchKernelGGL((rtk::lit_gloss_split_probe_kernel<true, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env, d_indirect);
                else hipLaunchKernelGGL((rtk::lit_gloss_split_probe_kernel<false, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env, d_indirect);
            } else {
                if (S.lens) hipLaunchKernelGGL((rtk::lit_split_probe_kernel<true, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env, d_indirect);
                else hipLaunchKernelGGL((rtk::lit_split_probe_kernel<false, Table>), grid, block, 0, 0, KP, T, S.C, d_nee, d_env, d_indirect);
            }
            return RT_OK;
        });
    });
    if (st != RT_OK || n == 0) return st;
    // (run_probe synchronised the device before it copied its own columns back)
    if (hipMemcpy(indirect, d_indirect, (size_t)n * 12, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(RT_ERR_HIP, "rt_trace_samples_lit_split: hipMemcpy D2H failed");
    return RT_OK;
}

// ---- rt_render_medium / rt_trace_samples_medium and the fog calls above them: one setup (fog_setup), one light
// (with_fog_light), one frame tail (fog_frame) and one probe tail (fog_probe) under rt_render_lit with a medium (§25), a density grid in
// its box (§28; its AOVs §33, its adaptive call §29), a tint (§34) or a glow (§35), and light samples of the glow (§36).
void rt_medium_params_init(rt_medium_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
    p->albedo[0] = p->albedo[1] = p->albedo[2] = 1.0f;
}
void rt_chroma_params_init(rt_chroma_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
    p->tint[0] = p->tint[1] = p->tint[2] = 1.0f;
}
void rt_glow_params_init(rt_glow_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
}
void rt_glow_sample_params_init(rt_glow_sample_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
    p->mis = 1;
}

// the density grid of rt_render_volume (rt_volume_create, below)
struct rt_volume {
    int device = 0;
    int32_t nx = 0, ny = 0, nz = 0;
    float *rho = nullptr;              // nx * ny * nz, x fastest
};
// the table of rt_render_glow_sampled (rt_glow_sampler_create, below)
struct rt_glow_sampler {
    int device = 0;
    int32_t source = 0, nx = 0, ny = 0, nz = 0;
    const rt_volume *volume = nullptr, *heat = nullptr;          // what it was built from (compared, never read again)
    bool empty = false;
    float *slab_cdf = nullptr, *row_cdf = nullptr, *cell_cdf = nullptr, *pc = nullptr;
};

namespace {
// the medium's checks (after rt_render_lit's parameter checks, before the scene is looked at) → M; M.sigma_t == 0: no medium
rt_status medium_setup(const char *what, const rt_medium_params *medium, rtk::MediumDev &M) {
    const std::string w(what);
    rt_medium_params mp;
    rt_medium_params_init(&mp);
    if (const rt_status st = take_params(w, "rt_medium_params", medium, mp)) return st;
    if (mp.region < 0 || mp.region > 2) return fail(RT_ERR_INVALID_ARG, w + ": region must be 0, 1 or 2");
    if (!(std::isfinite(mp.sigma_t) && mp.sigma_t >= 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": sigma_t must be finite and not negative");
    for (int k = 0; k < 3; ++k)
        if (!(mp.albedo[k] >= 0.0f && mp.albedo[k] <= 1.0f)) return fail(RT_ERR_INVALID_ARG, w + ": an albedo channel outside [0, 1]");
    if (!(std::fabs(mp.g) <= 0.95f)) return fail(RT_ERR_INVALID_ARG, w + ": |g| must be at most 0.95");
    if (mp.region != 0)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(mp.a[k]) || !std::isfinite(mp.b[mp.region == 1 ? 0 : k]))
                return fail(RT_ERR_INVALID_ARG, w + ": the region's a and b must be finite");
    if (mp.region == 1 && !(mp.b[0] > 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": the ball's radius must be positive");
    if (mp.region == 2)
        for (int k = 0; k < 3; ++k)
            if (!(mp.a[k] < mp.b[k])) return fail(RT_ERR_INVALID_ARG, w + ": the box needs lo < hi in every axis");
    M.region = mp.region;
    M.sigma_t = mp.sigma_t;
    M.g = mp.g;
    for (int k = 0; k < 3; ++k) {
        M.albedo[k] = mp.albedo[k];
        M.a[k] = mp.a[k];
        M.b[k] = mp.b[k];
    }
    return RT_OK;
}
// The medium kernels' light: with_lit's, always with the float carry (a GlossLit<Table>, its switches the call's), and the medium beside
// it.  Under a medium that fills all space no environment sample can count (its Tr is 0): the environment is not sampled
extern "C++" template <class F>
rt_status with_medium_lit(rt_scene *sc, const LitSetup &S, const rtk::MediumDev &M, F &&f) {
    return with_emitter_table(sc, S.nee, S.emitters, [&](const auto &table) {
        using Table = std::decay_t<decltype(table)>;
        rtk::MediumLit<Table> T{};
        T.G.N = table;
        if (S.env) {
            T.G.E = env_dev_of(S.env, S.ep);
            T.G.env_on = 1;
            if (M.region == 0) T.G.E.sampled = 0;
        }
        T.G.gn = S.emitters && S.nee.glossy ? 1 : 0;
        T.G.ge = S.env && S.ep.glossy ? 1 : 0;
        T.M = M;
        return f(T);
    });
}
// with_medium_lit with the grid beside the medium
extern "C++" template <class F>
rt_status with_volume_lit(rt_scene *sc, const LitSetup &S, const rtk::MediumDev &M, const rt_volume *volume, F &&f) {
    return with_medium_lit(sc, S, M, [&](const auto &ML) {
        const rtk::VolumeLit<std::decay_t<decltype(ML.G.N)>> T{ML, {volume->rho, volume->nx, volume->ny, volume->nz}};
        return f(T);
    });
}

// The columns a fog probe has beyond the lit probe's (the caller's on the host, the probe's own on the device): the medium stream's
// final state and the event count of every fog call, the grid's cells, the glow's length, the glow's light samples.  Null: the call has no
// such column
struct FogColumns {
    uint32_t *med;
    int32_t *events, *cells;
    float *glow_length;
    int32_t *glow_samples;
};
// the probe kernel of a light with fog, on the columns its light has
extern "C++" template <bool kLens, class Table>
void launch_fog_probe(const rtk::KParams &KP, const rtk::MediumLit<Table> &T, const rtk::LensCam &C, int32_t n, uint32_t *d_nee, uint32_t *d_env, const FogColumns &d) {
    hipLaunchKernelGGL((rtk::medium_probe_kernel<kLens, Table>), dim3((n + 255) / 256), dim3(256), 0, 0, KP, T, C, d_nee, d_env, d.med, d.events);
}
extern "C++" template <bool kLens, class Table>
void launch_fog_probe(const rtk::KParams &KP, const rtk::VolumeLit<Table> &T, const rtk::LensCam &C, int32_t n, uint32_t *d_nee, uint32_t *d_env, const FogColumns &d) {
    hipLaunchKernelGGL((rtk::volume_probe_kernel<kLens, Table>), dim3((n + 255) / 256), dim3(256), 0, 0, KP, T, C, d_nee, d_env, d.med, d.events, d.cells);
}
extern "C++" template <bool kLens, class Base>
void launch_fog_probe(const rtk::KParams &KP, const rtk::ChromaLit<Base> &T, const rtk::LensCam &C, int32_t n, uint32_t *d_nee, uint32_t *d_env, const FogColumns &d) {
    hipLaunchKernelGGL((rtk::chroma_probe_kernel<kLens, Base>), dim3((n + 255) / 256), dim3(256), 0, 0, KP, T, C, d_nee, d_env, d.med, d.events, d.cells);
}
extern "C++" template <bool kLens, class Base>
void launch_fog_probe(const rtk::KParams &KP, const rtk::GlowLit<Base> &T, const rtk::LensCam &C, int32_t n, uint32_t *d_nee, uint32_t *d_env, const FogColumns &d) {
    hipLaunchKernelGGL((rtk::glow_probe_kernel<kLens, Base>), dim3((n + 255) / 256), dim3(256), 0, 0, KP, T, C, d_nee, d_env, d.med, d.events, d.cells, d.glow_length);
}
extern "C++" template <bool kLens, class Table>
void launch_fog_probe(const rtk::KParams &KP, const rtk::GlowSampleLit<Table> &T, const rtk::LensCam &C, int32_t n, uint32_t *d_nee, uint32_t *d_env, const FogColumns &d) {
    hipLaunchKernelGGL((rtk::glow_sample_probe_kernel<kLens, Table>), dim3((n + 255) / 256), dim3(256), 0, 0, KP, T, C, d_nee, d_env, d.med, d.events, d.cells,
                       d.glow_length, d.glow_samples);
}
// The chroma kernels' light (rt_render_chroma): the medium's or the grid's with sigma_t = 1, and the three channels' extinctions beside it
extern "C++" template <class F>
rt_status with_chroma_lit(rt_scene *sc, const LitSetup &S, const rtk::MediumDev &M, const rt_volume *volume, const float *sigma, F &&f) {
    rtk::MediumDev M1 = M;
    M1.sigma_t = 1.0f;
    auto chroma = [&](const auto &B) {
        const rtk::ChromaLit<std::decay_t<decltype(B)>> T{B, sigma[0], sigma[1], sigma[2]};
        return f(T);
    };
    return volume ? with_volume_lit(sc, S, M1, volume, chroma) : with_medium_lit(sc, S, M1, chroma);
}
// The glow kernels' light (rt_render_glow): the medium's or the grid's as the grey kernels hold it, and the radiance beside it; over a grid
// also the cells' h (heat: null = 1, source 0; the density itself, source 1; a heat grid's values, source 2: with_fogged_light)
struct GlowDev {
    float radiance[3];
    const float *heat;
};
extern "C++" template <class F>
rt_status with_glow_lit(rt_scene *sc, const LitSetup &S, const rtk::MediumDev &M, const rt_volume *volume, const GlowDev &G, F &&f) {
    if (volume)
        return with_volume_lit(sc, S, M, volume, [&](const auto &B) {
            const rtk::GlowLit<std::decay_t<decltype(B)>> T{B, G.radiance[0], G.radiance[1], G.radiance[2], G.heat};
            return f(T);
        });
    return with_medium_lit(sc, S, M, [&](const auto &B) {
        const rtk::GlowLit<std::decay_t<decltype(B)>> T{B, G.radiance[0], G.radiance[1], G.radiance[2]};
        return f(T);
    });
}
// The sampled glow kernels' light (rt_render_glow_sampled): the glow's over the grid, and the sampler's table beside it
extern "C++" template <class F>
rt_status with_glow_sample_lit(rt_scene *sc, const LitSetup &S, const rtk::MediumDev &M, const rt_volume *volume, const GlowDev &G, const rtk::GlowSamplerDev &Q, F &&f) {
    return with_volume_lit(sc, S, M, volume, [&](const auto &B) {
        const rtk::GlowSampleLit<std::decay_t<decltype(B.G.N)>> T{{B, G.radiance[0], G.radiance[1], G.radiance[2], G.heat}, Q};
        return f(T);
    });
}

// The ladder of the fog calls, each rung the one below with one thing more: a medium, a grid in its box, then either a tint or a glow, and
// light samples of the glow.  A call names the rung it goes up to (fog_setup) and refuses under that rung's name
enum FogRung { kFogMedium, kFogVolume, kFogTint, kFogGlow, kFogSample };
const char *const kFogFrame[] = {"rt_render_medium", "rt_render_volume", "rt_render_chroma", "rt_render_glow", "rt_render_glow_sampled"};
const char *const kFogProbe[] = {"rt_trace_samples_medium", "rt_trace_samples_volume", "rt_trace_samples_chroma", "rt_trace_samples_glow",
                                 "rt_trace_samples_glow_sampled"};
// What a fog call is made of, after its parameter checks.  What a call has not (or has without effect) stays as it is here, and the call
// is the lower rung's by that alone: grey (no tint, equal tints, no medium: M.sigma_t then holds sigma_t * e), dark (no glow, radiance 0),
// not sampled (no sample, an empty sampler, a dark glow)
struct FogSetup {
    FogRung rung = kFogMedium;          // how far up the ladder the call goes
    LitSetup S;
    rtk::MediumDev M{};                 // sigma_t == 0: no medium
    const rt_volume *volume = nullptr;
    float sigma[3] = {0.0f, 0.0f, 0.0f};
    bool grey = true;
    GlowDev G{};                        // (heat: with_fogged_light fills it — the handles are not read before the scene has been looked at)
    const rt_volume *heat = nullptr;
    int32_t source = 0;
    bool dark = true;
    rtk::GlowSamplerDev Q{};
    const rt_glow_sampler *sampler = nullptr;          // of a call that asks for samples (also an empty one's, for its device's check)
    bool sampled = false;
};
// the caller's arguments that the rungs' checks look at, lowest rung first (left out or null: not the call's, or not given)
struct FogArgs {
    const rt_lit_params *lit;
    const rt_medium_params *medium;
    const rt_volume *volume;
    const rt_chroma_params *chroma;
    const rt_glow_params *glow;
    const rt_volume *heat;
    const rt_glow_sample_params *sample;
    const rt_glow_sampler *sampler;
};
// The parameter checks of a fog call up to its rung, in the ladder's order — lit, medium, volume, then the tint's or the glow's, then the
// sample's: everything before the scene is looked at.  What lies above the rung is not looked at
rt_status fog_setup(const char *what, FogRung rung, const rt_camera_data *cam_open, const FogArgs &A, FogSetup &X) {
    const auto [lit, medium, volume, chroma, glow, heat, sample, sampler] = A;
    const std::string w(what);
    X.rung = rung;
    if (const rt_status st = lit_setup(what, cam_open, lit, X.S)) return st;
    if (const rt_status st = medium_setup(what, medium, X.M)) return st;
    if (volume && !(medium && X.M.region == 2)) return fail(RT_ERR_INVALID_ARG, w + ": a volume needs a medium with region 2 (the box the grid fills)");
    X.volume = volume;
    if (rung == kFogTint) {
        rt_chroma_params cp;
        rt_chroma_params_init(&cp);
        if (const rt_status st = take_params(w, "rt_chroma_params", chroma, cp)) return st;
        for (int k = 0; k < 3; ++k)
            if (!(std::isfinite(cp.tint[k]) && cp.tint[k] >= 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": a tint channel is negative, NaN or infinite");
        for (int k = 0; k < 3; ++k) {
            X.sigma[k] = X.M.sigma_t * cp.tint[k];
            if (!std::isfinite(X.sigma[k])) return fail(RT_ERR_INVALID_ARG, w + ": sigma_t * tint is not finite in a channel");
        }
        X.grey = (cp.tint[0] == cp.tint[1] && cp.tint[1] == cp.tint[2]) || !(X.M.sigma_t > 0.0f);
        if (X.grey) X.M.sigma_t = X.sigma[0];
    }
    if (rung >= kFogGlow) {
        rt_glow_params gp;
        rt_glow_params_init(&gp);
        if (const rt_status st = take_params(w, "rt_glow_params", glow, gp)) return st;
        if (gp.source < 0 || gp.source > 2) return fail(RT_ERR_INVALID_ARG, w + ": source must be 0, 1 or 2");
        for (int k = 0; k < 3; ++k)
            if (!(std::isfinite(gp.radiance[k]) && gp.radiance[k] >= 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": a radiance channel is negative, NaN or infinite");
        X.dark = gp.radiance[0] == 0.0f && gp.radiance[1] == 0.0f && gp.radiance[2] == 0.0f;
        if (!X.dark && !(X.M.sigma_t > 0.0f))
            return fail(RT_ERR_INVALID_ARG, w + ": a glow needs a medium with sigma_t > 0 (the emission rides on the free flight: a glow without extinction has no kernel)");
        if (gp.source != 0 && !volume) return fail(RT_ERR_INVALID_ARG, w + ": source 1 and 2 need a volume (the grid the emission follows)");
        if (gp.source == 2 && !heat) return fail(RT_ERR_INVALID_ARG, w + ": source 2 needs a heat grid");
        if (gp.source == 2 && (heat->nx != volume->nx || heat->ny != volume->ny || heat->nz != volume->nz))
            return fail(RT_ERR_INVALID_ARG, w + ": the heat grid's dimensions differ from the volume's");
        if (gp.source != 2 && heat) return fail(RT_ERR_INVALID_ARG, w + ": a heat grid is for source 2 only");
        for (int k = 0; k < 3; ++k) X.G.radiance[k] = gp.radiance[k];
        X.source = gp.source;
        X.heat = heat;
    }
    if (rung == kFogSample) {
        rt_glow_sample_params sp;
        rt_glow_sample_params_init(&sp);
        if (const rt_status st = take_params(w, "rt_glow_sample_params", sample, sp)) return st;
        if (sp.sample != 0 && sp.sample != 1) return fail(RT_ERR_INVALID_ARG, w + ": sample must be 0 or 1");
        if (sp.mis != 0 && sp.mis != 1) return fail(RT_ERR_INVALID_ARG, w + ": mis must be 0 or 1");
        if (!sample || sp.sample == 0) return RT_OK;
        if (!volume) return fail(RT_ERR_INVALID_ARG, w + ": light samples of the glow need a volume (a homogeneous box can pass a 1 x 1 x 1 grid of density 1)");
        if (!sampler) return fail(RT_ERR_INVALID_ARG, w + ": sample = 1 needs a sampler (rt_glow_sampler_create)");
        if (sampler->source != X.source) return fail(RT_ERR_INVALID_ARG, w + ": the sampler was built for another source than the call's");
        if (sampler->nx != volume->nx || sampler->ny != volume->ny || sampler->nz != volume->nz)
            return fail(RT_ERR_INVALID_ARG, w + ": the sampler's dimensions differ from the volume's");
        if (sampler->volume != volume || sampler->heat != heat) return fail(RT_ERR_INVALID_ARG, w + ": the sampler was built from other grids than the call's");
        X.Q = {sampler->slab_cdf, sampler->row_cdf, sampler->cell_cdf, sampler->pc, sp.mis};
        X.sampler = sampler;
        X.sampled = !sampler->empty && !X.dark;
    }
    return RT_OK;
}
// the null scene's refusal, then the device of every handle the call holds against the scene's
rt_status fog_scene(const std::string &w, const rt_scene *sc, const FogSetup &X) {
    if (!sc) return fail(RT_ERR_INVALID_ARG, w + ": null scene");
    if (X.volume && X.volume->device != sc->device) return fail(RT_ERR_INVALID_ARG, w + ": the volume was created on another device than the scene");
    if (X.heat && X.heat->device != sc->device) return fail(RT_ERR_INVALID_ARG, w + ": the heat grid was created on another device than the scene");
    if (X.sampler && X.sampler->device != sc->device) return fail(RT_ERR_INVALID_ARG, w + ": the sampler was created on another device than the scene");
    return RT_OK;
}
// the rung whose kernels a call runs, by what it holds: the hand-overs, all at once (no medium at all: with_fog_light's)
FogRung fog_rung_of(const FogSetup &X) { return X.sampled ? kFogSample : !X.dark ? kFogGlow : !X.grey ? kFogTint : X.volume ? kFogVolume : kFogMedium; }
// The light of a call with a medium (M.sigma_t > 0), of fog_rung_of's rung: a GlowSampleLit, GlowLit, ChromaLit, VolumeLit or MediumLit
extern "C++" template <class F>
rt_status with_fogged_light(rt_scene *sc, const FogSetup &X, F &&f) {
    if (!X.dark) {
        GlowDev G = X.G;
        G.heat = X.source == 0 ? nullptr : (X.source == 1 ? X.volume->rho : X.heat->rho);
        if (X.sampled) return with_glow_sample_lit(sc, X.S, X.M, X.volume, G, X.Q, f);
        return with_glow_lit(sc, X.S, X.M, X.volume, G, f);
    }
    if (!X.grey) return with_chroma_lit(sc, X.S, X.M, X.volume, X.sigma, f);
    return X.volume ? with_volume_lit(sc, X.S, X.M, X.volume, f) : with_medium_lit(sc, X.S, X.M, f);
}
// the light of a fog call: no medium is with_lit's (a Lit or GlossLit)
extern "C++" template <class F>
rt_status with_fog_light(rt_scene *sc, const FogSetup &X, F &&f) {
    return X.M.sigma_t > 0.0f ? with_fogged_light(sc, X, f) : with_lit(sc, X.S, f);
}
// The frame calls behind their parameter checks: the scene and the devices under the call's own name, then render_light_impl under the
// name of the rung the call has become
rt_status fog_frame(const FogSetup &X, rt_scene *sc, const rt_camera_data *cam_open, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream,
                    int32_t sync, rt_timing *timing) {
    if (const rt_status st = fog_scene(kFogFrame[X.rung], sc, X)) return st;
    const LitSetup &S = X.S;
    auto with_light = [&](auto frame) { return with_fog_light(sc, X, [&](const auto &T) { return frame(lit_kernels_of(S.lens, T).frame, &T); }); };
    return render_light_impl(kFogFrame[fog_rung_of(X)], S.env ? &S.env->device : nullptr, with_light, sc, cam_open, shard, sample_first, d_fb_sum, hip_stream, sync, timing,
                             &S.C);
}
// The probe calls behind their parameter checks.  `out` holds the columns of the call's rung (the others null); a column of a rung the
// call has left on the way down is filled on the way back: cells 0, glow_length 0, glow_samples 0, and under no medium no event and the
// medium stream's state as initialised.  The order is every probe's own: the glow rungs look at the scene and the devices
// and hand over before the preamble, the volume and the medium behind it, and the lower rungs look at the volume's device last
rt_status fog_probe(const FogSetup &X, rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, int32_t n, const int32_t *ijs, float *radiance,
                    int32_t *rays, uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed, const FogColumns &out) {
    const LitSetup &S = X.S;
    if (n < 0 || (n > 0 && (!ijs || !radiance || !rays || !out.events || !final_seed || !final_nee_seed || !final_env_seed || !out.med ||
                            (X.rung >= kFogVolume && !out.cells) || (X.rung >= kFogGlow && !out.glow_length) || (X.rung == kFogSample && !out.glow_samples))))
        return fail(RT_ERR_INVALID_ARG, std::string(kFogProbe[X.rung]) + ": null argument");
    rt_status st;
    if (X.rung >= kFogGlow && (st = fog_scene(kFogProbe[X.rung], sc, X)) != RT_OK) return st;
    // (a call above the medium's is the volume's at the lowest until the preamble has passed)
    FogRung rung = X.rung == kFogMedium ? kFogMedium : std::max(fog_rung_of(X), kFogVolume);
    rtk::KParams P;
    if ((st = fill_params(sc, cam_open, nullptr, P)) != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    if (S.env && S.env->device != sc->device)
        return fail(RT_ERR_INVALID_ARG, std::string(kFogProbe[rung]) + ": the environment was created on another device than the scene");
    if (X.rung < kFogGlow && (st = fog_scene(kFogProbe[rung], sc, X)) != RT_OK) return st;
    if (n == 0) return RT_OK;
    if (rung == kFogVolume && !(X.volume && X.M.sigma_t > 0.0f)) rung = kFogMedium;
    const std::string w(kFogProbe[rung]);
    const FogColumns own{out.med, out.events, rung >= kFogVolume ? out.cells : nullptr, rung >= kFogGlow ? out.glow_length : nullptr,
                         rung == kFogSample ? out.glow_samples : nullptr};
    if (!(X.M.sigma_t > 0.0f)) {          // no medium (the rung is the medium's): rt_trace_samples_lit's columns
        if ((st = rt_trace_samples_lit(sc, cam_open, lit, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed)) != RT_OK) return st;
        for (int32_t k = 0; k < n; ++k) {
            out.events[k] = 0;
            const uint32_t base = rtd::wang_hash((uint32_t)ijs[3 * k] * (uint32_t)cam_open->image_width + (uint32_t)ijs[3 * k + 1]);
            out.med[k] = rtd::wang_hash(rtd::wang_hash(base + (uint32_t)ijs[3 * k + 2]) ^ RT_MEDIUM_STREAM_KEY);
        }
    } else {
        FogColumns d{};
        Scratch mem;
        if (mem.alloc(d.med, (size_t)n * 4) != hipSuccess || mem.alloc(d.events, (size_t)n * 4) != hipSuccess ||
            (own.cells && mem.alloc(d.cells, (size_t)n * 4) != hipSuccess) || (own.glow_length && mem.alloc(d.glow_length, (size_t)n * 4) != hipSuccess) ||
            (own.glow_samples && mem.alloc(d.glow_samples, (size_t)n * 4) != hipSuccess))
            return fail(RT_ERR_OUT_OF_MEMORY, w + ": hipMalloc failed");
        st = run_probe(w + ": ", P, cam_open, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed, [&](const rtk::KParams &KP, uint32_t *d_nee, uint32_t *d_env) {
            return with_fogged_light(sc, X, [&](const auto &T) {
                if (S.lens) launch_fog_probe<true>(KP, T, S.C, n, d_nee, d_env, d);
                else launch_fog_probe<false>(KP, T, S.C, n, d_nee, d_env, d);
                return RT_OK;
            });
        });
        if (st != RT_OK) return st;
        // (run_probe has waited for the device)
        if (hipMemcpy(own.med, d.med, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(own.events, d.events, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            (own.cells && hipMemcpy(own.cells, d.cells, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
            (own.glow_length && hipMemcpy(own.glow_length, d.glow_length, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
            (own.glow_samples && hipMemcpy(own.glow_samples, d.glow_samples, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess))
            return fail(RT_ERR_HIP, w + ": hipMemcpy D2H failed");
    }
    for (int32_t k = 0; k < n; ++k) {
        if (out.cells && !own.cells) out.cells[k] = 0;
        if (out.glow_length && !own.glow_length) out.glow_length[k] = 0.0f;
        if (out.glow_samples && !own.glow_samples) out.glow_samples[k] = 0;
    }
    return RT_OK;
}
}  // namespace

rt_status rt_render_medium(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_shard *shard,
                           int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogFrame[kFogMedium], kFogMedium, cam_open, {lit, medium}, X)) return st;
    return fog_frame(X, sc, cam_open, shard, sample_first, d_fb_sum, hip_stream, sync, timing);
}

rt_status rt_trace_samples_medium(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, int32_t n,
                                  const int32_t *ijs, float *radiance, int32_t *rays, int32_t *medium_events, uint32_t *final_seed, uint32_t *final_nee_seed,
                                  uint32_t *final_env_seed, uint32_t *final_medium_seed) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogProbe[kFogMedium], kFogMedium, cam_open, {lit, medium}, X)) return st;
    return fog_probe(X, sc, cam_open, lit, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed, {final_medium_seed, medium_events, nullptr, nullptr, nullptr});
}

// ---- rt_volume / rt_render_volume / rt_trace_samples_volume (rtp_amd.h, "density grid"): rt_render_medium with a density
// grid in its box.  No volume is rt_render_medium itself, sigma_t == 0 rt_render_lit; otherwise the kernels of rt_volume.hip.inc.
rt_status rt_volume_create(const float *density, int32_t nx, int32_t ny, int32_t nz, rt_volume **out_volume) {
    if (!density || !out_volume) return fail(RT_ERR_INVALID_ARG, "rt_volume_create: null argument");
    *out_volume = nullptr;
    if (nx < 1 || ny < 1 || nz < 1 || nx > RT_VOLUME_MAX_N || ny > RT_VOLUME_MAX_N || nz > RT_VOLUME_MAX_N)
        return fail(RT_ERR_INVALID_ARG, "rt_volume_create: every dimension must be 1 … " + std::to_string(RT_VOLUME_MAX_N));
    const size_t count = (size_t)nx * (size_t)ny * (size_t)nz;
    for (size_t k = 0; k < count; ++k)
        if (!(std::isfinite(density[k]) && density[k] >= 0.0f)) return fail(RT_ERR_INVALID_ARG, "rt_volume_create: a density is negative, NaN or infinite");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RT_ERR_NO_DEVICE, "rt_volume_create: no current HIP device");
    }
    rt_volume *vol = new (std::nothrow) rt_volume();
    if (!vol) return fail(RT_ERR_OUT_OF_MEMORY, "rt_volume_create: out of host memory");
    vol->device = dev;
    vol->nx = nx;
    vol->ny = ny;
    vol->nz = nz;
    const rt_status st = upload(std::vector<float>(density, density + count), (void **)&vol->rho);
    if (st != RT_OK) {
        (void)rt_volume_destroy(vol);
        return st;
    }
    *out_volume = vol;
    return RT_OK;
}

rt_status rt_volume_destroy(rt_volume *volume) {
    if (!volume) return RT_OK;
    (void)hipFree(volume->rho);
    delete volume;
    return RT_OK;
}

rt_status rt_render_volume(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                           const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    const FogRung rung = volume ? kFogVolume : kFogMedium;          // (no volume is rt_render_medium from its first check on)
    FogSetup X;
    if (const rt_status st = fog_setup(kFogFrame[rung], rung, cam_open, {lit, medium, volume}, X)) return st;
    return fog_frame(X, sc, cam_open, shard, sample_first, d_fb_sum, hip_stream, sync, timing);
}

// ---- rt_render_aov_volume (rtp_amd.h, "AOVs under fog"): rt_render_aov_lens's frame (aov_impl) with the accumulation of
// rt_aov_fog.hip.inc.  Of lit only the camera shapes the result.  No medium is rt_render_aov_lens's own kernels, and a transmittance of spp.
rt_status rt_render_aov_volume(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                               const rt_shard *shard, int32_t sample_first, const rt_aov_buffers *buffers, float *d_transmittance_sum, void *hip_stream,
                               int32_t sync, rt_timing *timing) {
    const char *what = "rt_render_aov_volume";
    // (the buffers first, as aov_impl has them)
    if (!buffers || buffers->struct_bytes < 16u) return fail(RT_ERR_INVALID_ARG, "rt_render_aov_volume: null AOV buffers (or struct_bytes below 16)");
    rt_aov_buffers b{};
    std::memcpy(&b, buffers, buffers->struct_bytes < sizeof(b) ? buffers->struct_bytes : sizeof(b));
    if (!b.albedo_sum && !b.normal_sum && !b.depth_sum && !b.hit_count && !b.first_prim) return fail(RT_ERR_INVALID_ARG, "rt_render_aov_volume: every AOV buffer is NULL");
    FogSetup X;
    if (const rt_status st = fog_setup(what, kFogVolume, cam_open, {lit, medium, volume}, X)) return st;
    if (const rt_status st = fog_scene(what, sc, X)) return st;
    const LitSetup &S = X.S;
    if (!(X.M.sigma_t > 0.0f)) return aov_impl(sc, cam_open, shard, nullptr, buffers, hip_stream, sync, timing, sample_first, &S.C, what, nullptr, d_transmittance_sum);
    rtk::AovFog G{};
    G.M = X.M;
    if (volume) G.V = rtk::VolumeDev{volume->rho, volume->nx, volume->ny, volume->nz};
    G.tr = d_transmittance_sum;
    return aov_impl(sc, cam_open, shard, nullptr, buffers, hip_stream, sync, timing, sample_first, &S.C, what, &G);
}

// ---- rt_render_volume_adaptive (rtp_amd.h): rt_render_lit_adaptive_prior's steps (lit_adaptive_run) on rt_render_volume's
// estimator — the frame kernel of the medium or of the grid for the min_spp frame, its list variant for the rounds.  No medium is
// rt_render_lit_adaptive_prior itself, once this call's own checks have passed.
rt_status rt_render_volume_adaptive(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                                    const rt_adaptive_params *params, const rt_stop_params *stop, const float *d_prior, const rt_shard *shard,
                                    int32_t sample_first, float *d_fb_sum, int32_t *d_spp, float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing) {
    const char *what = "rt_render_volume_adaptive";
    rt_adaptive_params a;
    int32_t rule;
    rt_status st = adaptive_check(what, params, a);
    if (st != RT_OK) return st;
    if ((st = stop_check(what, stop, rule, "")) != RT_OK) return st;
    if ((st = prior_check(what, d_prior, cam_open, shard, d_fb_sum, d_spp, d_moments)) != RT_OK) return st;
    FogSetup X;
    if ((st = fog_setup(what, kFogVolume, cam_open, {lit, medium, volume}, X)) != RT_OK) return st;
    if ((st = check_sample_range(what, sample_first, a.min_spp + (a.max_spp - a.min_spp) / a.batch_spp * a.batch_spp)) != RT_OK) return st;
    if (!d_fb_sum || !d_spp) return fail(RT_ERR_INVALID_ARG, "rt_render_volume_adaptive: null framebuffer or sample counts");
    if ((st = fog_scene(what, sc, X)) != RT_OK) return st;
    if (!(X.M.sigma_t > 0.0f))
        return rt_render_lit_adaptive_prior(sc, cam_open, lit, params, stop, shard, sample_first, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing, d_prior);
    const LitSetup &S = X.S;
    return lit_adaptive_run(what, sc, cam_open, S, a, rule, d_prior, shard, sample_first, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing, [&](auto run) {
        return with_fog_light(sc, X, [&](const auto &T) { return run(lit_kernels_of(S.lens, T).frame, lit_kernels_of(S.lens, T).list, &T); });
    });
}

rt_status rt_trace_samples_volume(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                                  int32_t n, const int32_t *ijs, float *radiance, int32_t *rays, int32_t *medium_events, uint32_t *final_seed,
                                  uint32_t *final_nee_seed, uint32_t *final_env_seed, uint32_t *final_medium_seed, int32_t *cells) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogProbe[kFogVolume], kFogVolume, cam_open, {lit, medium, volume}, X)) return st;
    return fog_probe(X, sc, cam_open, lit, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed, {final_medium_seed, medium_events, cells, nullptr, nullptr});
}

// ---- rt_render_chroma / rt_trace_samples_chroma (rtp_amd.h, "chromatic extinction"): rt_render_volume with an extinction
// per channel.  Equal tints (and no medium) are rt_render_volume itself at sigma_t * e; otherwise the kernels of rt_chroma.hip.inc.
rt_status rt_render_chroma(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                           const rt_chroma_params *chroma, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync,
                           rt_timing *timing) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogFrame[kFogTint], kFogTint, cam_open, {lit, medium, volume, chroma}, X)) return st;
    return fog_frame(X, sc, cam_open, shard, sample_first, d_fb_sum, hip_stream, sync, timing);
}

rt_status rt_trace_samples_chroma(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                                  const rt_chroma_params *chroma, int32_t n, const int32_t *ijs, float *radiance, int32_t *rays, int32_t *medium_events,
                                  uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed, uint32_t *final_medium_seed, int32_t *cells) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogProbe[kFogTint], kFogTint, cam_open, {lit, medium, volume, chroma}, X)) return st;
    return fog_probe(X, sc, cam_open, lit, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed, {final_medium_seed, medium_events, cells, nullptr, nullptr});
}

// ---- rt_render_glow / rt_trace_samples_glow (rtp_amd.h, "emission in the medium"): rt_render_volume with a medium that
// emits.  No glow (NULL, or radiance 0, 0, 0) is rt_render_volume itself; otherwise the kernels of rt_glow.hip.inc.
rt_status rt_render_glow(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                         const rt_glow_params *glow, const rt_volume *heat, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream,
                         int32_t sync, rt_timing *timing) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogFrame[kFogGlow], kFogGlow, cam_open, {lit, medium, volume, nullptr, glow, heat}, X)) return st;
    return fog_frame(X, sc, cam_open, shard, sample_first, d_fb_sum, hip_stream, sync, timing);
}

rt_status rt_trace_samples_glow(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                                const rt_glow_params *glow, const rt_volume *heat, int32_t n, const int32_t *ijs, float *radiance, int32_t *rays,
                                int32_t *medium_events, uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed, uint32_t *final_medium_seed,
                                int32_t *cells, float *glow_length) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogProbe[kFogGlow], kFogGlow, cam_open, {lit, medium, volume, nullptr, glow, heat}, X)) return st;
    return fog_probe(X, sc, cam_open, lit, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed, {final_medium_seed, medium_events, cells, glow_length, nullptr});
}

// ---- rt_glow_sampler / rt_render_glow_sampled / rt_trace_samples_glow_sampled (rtp_amd.h, "light samples of the glow"):
// rt_render_glow over a grid with the glow as a third light.  No sample (NULL, sample == 0), an empty sampler or no glow is rt_render_glow
// itself; otherwise the kernels of rt_glow_sample.hip.inc.
rt_status rt_glow_sampler_create(const rt_volume *volume, int32_t source, const rt_volume *heat, rt_glow_sampler **out_sampler) {
    if (!volume || !out_sampler) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_create: null argument");
    *out_sampler = nullptr;
    if (source < 0 || source > 2) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_create: source must be 0, 1 or 2");
    if (source == 2 && !heat) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_create: source 2 needs a heat grid");
    if (source != 2 && heat) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_create: a heat grid is for source 2 only");
    if (heat && (heat->nx != volume->nx || heat->ny != volume->ny || heat->nz != volume->nz))
        return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_create: the heat grid's dimensions differ from the volume's");
    if (heat && heat->device != volume->device) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_create: the heat grid was created on another device than the volume");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RT_ERR_NO_DEVICE, "rt_glow_sampler_create: no current HIP device");
    }
    if (dev != volume->device) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_create: the volume was created on another device than the current one");
    const int32_t nx = volume->nx, ny = volume->ny, nz = volume->nz;
    const size_t rows = (size_t)nz * (size_t)ny, count = rows * (size_t)nx;
    std::vector<float> h(count, 1.0f);
    if (source != 0) HIP_TRY(hipMemcpy(h.data(), source == 1 ? volume->rho : heat->rho, count * 4, hipMemcpyDeviceToHost));
    // the sums, float64 in index order: a row's over its cells, a slab's over its rows', the total over the slabs'
    std::vector<double> row_sum(rows, 0.0), slab_sum((size_t)nz, 0.0);
    double total = 0.0;
    for (size_t r = 0; r < rows; ++r)
        for (int32_t x = 0; x < nx; ++x) row_sum[r] += (double)h[r * (size_t)nx + (size_t)x];
    for (int32_t z = 0; z < nz; ++z) {
        for (int32_t y = 0; y < ny; ++y) slab_sum[(size_t)z] += row_sum[(size_t)z * (size_t)ny + (size_t)y];
        total += slab_sum[(size_t)z];
    }
    // a cdf over n values with sum `sum`: the float32 of running sum / sum, the last entry 1.0f; sum 0: all zero
    auto cdf_of = [](auto value, int32_t n, double sum, float *cdf) {
        double run = 0.0;
        for (int32_t k = 0; k < n; ++k) {
            run += value(k);
            cdf[k] = sum > 0.0 ? (float)(run / sum) : 0.0f;
        }
        if (sum > 0.0) cdf[n - 1] = 1.0f;
    };
    std::vector<float> slab_cdf((size_t)nz), row_cdf(rows), cell_cdf(count), pc(count);
    cdf_of([&](int32_t z) { return slab_sum[(size_t)z]; }, nz, total, slab_cdf.data());
    for (int32_t z = 0; z < nz; ++z)
        cdf_of([&](int32_t y) { return row_sum[(size_t)z * (size_t)ny + (size_t)y]; }, ny, slab_sum[(size_t)z], row_cdf.data() + (size_t)z * (size_t)ny);
    for (size_t r = 0; r < rows; ++r)
        cdf_of([&](int32_t x) { return (double)h[r * (size_t)nx + (size_t)x]; }, nx, row_sum[r], cell_cdf.data() + r * (size_t)nx);
    auto pmf_of = [](const float *cdf, int32_t k) { return cdf[k] - (k == 0 ? 0.0f : cdf[k - 1]); };
    for (int32_t z = 0; z < nz; ++z)
        for (int32_t y = 0; y < ny; ++y) {
            const size_t r = (size_t)z * (size_t)ny + (size_t)y;
            const float sr = pmf_of(slab_cdf.data(), z) * pmf_of(row_cdf.data() + (size_t)z * (size_t)ny, y);
            for (int32_t x = 0; x < nx; ++x) pc[r * (size_t)nx + (size_t)x] = sr * pmf_of(cell_cdf.data() + r * (size_t)nx, x);
        }
    rt_glow_sampler *q = new (std::nothrow) rt_glow_sampler();
    if (!q) return fail(RT_ERR_OUT_OF_MEMORY, "rt_glow_sampler_create: out of host memory");
    q->device = dev;
    q->source = source;
    q->nx = nx;
    q->ny = ny;
    q->nz = nz;
    q->volume = volume;
    q->heat = heat;
    q->empty = !(total > 0.0);
    rt_status st = upload(slab_cdf, (void **)&q->slab_cdf);
    if (st == RT_OK) st = upload(row_cdf, (void **)&q->row_cdf);
    if (st == RT_OK) st = upload(cell_cdf, (void **)&q->cell_cdf);
    if (st == RT_OK) st = upload(pc, (void **)&q->pc);
    if (st != RT_OK) {
        (void)rt_glow_sampler_destroy(q);
        return st;
    }
    *out_sampler = q;
    return RT_OK;
}

rt_status rt_glow_sampler_destroy(rt_glow_sampler *sampler) {
    if (!sampler) return RT_OK;
    (void)hipFree(sampler->slab_cdf);
    (void)hipFree(sampler->row_cdf);
    (void)hipFree(sampler->cell_cdf);
    (void)hipFree(sampler->pc);
    delete sampler;
    return RT_OK;
}

rt_status rt_glow_sampler_table(const rt_glow_sampler *sampler, int32_t z, int32_t y, float *slab_cdf, float *row_cdf, float *cell_cdf, float *pc_row,
                                int32_t *count) {
    if (!sampler) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_table: null sampler");
    if (z < 0 || z >= sampler->nz || y < 0 || y >= sampler->ny) return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_table: slab or row out of range");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sampler->device) {
        (void)hipGetLastError();
        return fail(RT_ERR_INVALID_ARG, "rt_glow_sampler_table: the sampler was created on another device than the current one");
    }
    const size_t nx = (size_t)sampler->nx, ny = (size_t)sampler->ny, row = (size_t)z * ny + (size_t)y;
    if (slab_cdf) HIP_TRY(hipMemcpy(slab_cdf, sampler->slab_cdf, (size_t)sampler->nz * 4, hipMemcpyDeviceToHost));
    if (row_cdf) HIP_TRY(hipMemcpy(row_cdf, sampler->row_cdf + (size_t)z * ny, ny * 4, hipMemcpyDeviceToHost));
    if (cell_cdf) HIP_TRY(hipMemcpy(cell_cdf, sampler->cell_cdf + row * nx, nx * 4, hipMemcpyDeviceToHost));
    if (pc_row) HIP_TRY(hipMemcpy(pc_row, sampler->pc + row * nx, nx * 4, hipMemcpyDeviceToHost));
    if (count) *count = sampler->empty ? 0 : sampler->nx * sampler->ny * sampler->nz;
    return RT_OK;
}

rt_status rt_render_glow_sampled(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium, const rt_volume *volume,
                                 const rt_glow_params *glow, const rt_volume *heat, const rt_glow_sample_params *sample, const rt_glow_sampler *sampler,
                                 const rt_shard *shard, int32_t sample_first, float *d_fb_sum, void *hip_stream, int32_t sync, rt_timing *timing) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogFrame[kFogSample], kFogSample, cam_open, {lit, medium, volume, nullptr, glow, heat, sample, sampler}, X)) return st;
    return fog_frame(X, sc, cam_open, shard, sample_first, d_fb_sum, hip_stream, sync, timing);
}

rt_status rt_trace_samples_glow_sampled(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_medium_params *medium,
                                        const rt_volume *volume, const rt_glow_params *glow, const rt_volume *heat, const rt_glow_sample_params *sample,
                                        const rt_glow_sampler *sampler, int32_t n, const int32_t *ijs, float *radiance, int32_t *rays, int32_t *medium_events,
                                        uint32_t *final_seed, uint32_t *final_nee_seed, uint32_t *final_env_seed, uint32_t *final_medium_seed, int32_t *cells,
                                        float *glow_length, int32_t *glow_samples) {
    FogSetup X;
    if (const rt_status st = fog_setup(kFogProbe[kFogSample], kFogSample, cam_open, {lit, medium, volume, nullptr, glow, heat, sample, sampler}, X)) return st;
    return fog_probe(X, sc, cam_open, lit, n, ijs, radiance, rays, final_seed, final_nee_seed, final_env_seed,
                     {final_medium_seed, medium_events, cells, glow_length, glow_samples});
}

// ---- rt_render_fog_adaptive (rtp_amd.h, "adaptive sampling on every fog rung"): rt_render_volume_adaptive's steps
// (lit_adaptive_run) on the estimator of the rung the arguments name — fog_setup at the highest rung the pointers ask for, then the frame
// kernel and the list variant of the light with_fog_light makes, which is the lower rung's after a hand-over and with_lit's without a medium.
void rt_fog_params_init(rt_fog_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_bytes = (uint32_t)sizeof(*p);
}

rt_status rt_render_fog_adaptive(rt_scene *sc, const rt_camera_data *cam_open, const rt_lit_params *lit, const rt_fog_params *fog, const rt_adaptive_params *params,
                                 const rt_stop_params *stop, const float *d_prior, const rt_shard *shard, int32_t sample_first, float *d_fb_sum, int32_t *d_spp,
                                 float *d_moments, void *hip_stream, int32_t sync, rt_timing *timing) {
    const char *what = "rt_render_fog_adaptive";
    rt_adaptive_params a;
    int32_t rule;
    rt_status st = adaptive_check(what, params, a);
    if (st != RT_OK) return st;
    if ((st = stop_check(what, stop, rule, "")) != RT_OK) return st;
    if ((st = prior_check(what, d_prior, cam_open, shard, d_fb_sum, d_spp, d_moments)) != RT_OK) return st;
    if (!fog || fog->struct_bytes < 8u) return fail(RT_ERR_INVALID_ARG, "rt_render_fog_adaptive: null rt_fog_params (or struct_bytes below 8)");
    rt_fog_params f{};
    std::memcpy(&f, fog, fog->struct_bytes < sizeof(f) ? fog->struct_bytes : sizeof(f));
    if (f.chroma && f.glow) return fail(RT_ERR_INVALID_ARG, "rt_render_fog_adaptive: a call takes a tint or a glow, not both (no frame call renders a tint together with a glow)");
    // (a sample beside a tint has no glow to aim at: the tint's call, and the sample is above its rung)
    const FogRung rung = f.chroma ? kFogTint : f.sample ? kFogSample : f.glow ? kFogGlow : kFogVolume;
    FogSetup X;
    if ((st = fog_setup(what, rung, cam_open, {lit, f.medium, f.volume, f.chroma, f.glow, f.heat, f.sample, f.sampler}, X)) != RT_OK) return st;
    if ((st = check_sample_range(what, sample_first, a.min_spp + (a.max_spp - a.min_spp) / a.batch_spp * a.batch_spp)) != RT_OK) return st;
    if (!d_fb_sum || !d_spp) return fail(RT_ERR_INVALID_ARG, "rt_render_fog_adaptive: null framebuffer or sample counts");
    if ((st = fog_scene(what, sc, X)) != RT_OK) return st;
    const LitSetup &S = X.S;
    return lit_adaptive_run(what, sc, cam_open, S, a, rule, d_prior, shard, sample_first, d_fb_sum, d_spp, d_moments, hip_stream, sync, timing, [&](auto run) {
        return with_fog_light(sc, X, [&](const auto &T) { return run(lit_kernels_of(S.lens, T).frame, lit_kernels_of(S.lens, T).list, &T); });
    });
}

void rt_timing_init(rt_timing *t) {
    if (!t) return;
    std::memset(t, 0, sizeof(*t));
    t->struct_bytes = (uint32_t)sizeof(*t);
}

rt_status rt_last_timing(rt_scene *sc, rt_timing *timing) {
    if (!sc) return fail(RT_ERR_INVALID_ARG, "null argument");
    if (const rt_status ts = timing_check(timing)) return ts;
    if (sc->timed) {
        // (measured once per render: hipEventElapsedTime of one recorded pair can come back a nanosecond apart once later work has
        // recorded events of its own — an adaptive call, say — and the record of a finished render does not change: DESIGN.md §40)
        float kernel = 0.0f, sum = 0.0f, rework = 0.0f, primary = 0.0f;
        if (const rt_status ps = sc->clock[kClockRender].elapsed(kernel)) return ps;
        if (const rt_status ps = frame_parts(sc, sum, rework, primary)) return ps;
        if (!sc->durations_read) {
            sc->last.kernel_ms = kernel;
            sc->last.trace_ms = sum;
            sc->last.rework_ms = rework;
            sc->last.primary_ms = sc->last.primary_visibility ? primary : 0.0f;
            sc->durations_read = true;
        }
        // (the frame is done, so what it left for the handle's judgement has landed as well: a scene the guarded walk keeps handing
        // back — dense overlaps, a camera inside a sphere, … — is cheaper on the exact walk alone; later frames of this handle use it)
        if (const rt_status ps = poll_feedback(sc, true)) return ps;
        sc->last.guard_paused = sc->guard_paused ? 1u : 0u;
        sc->last.traced_samples = sc->last_samples;
        if (sc->last_traced_pixels) {
            uint32_t traced = 0;
            HIP_TRY(hipMemcpy(&traced, sc->last_traced_pixels, 4, hipMemcpyDeviceToHost));
            sc->last.traced_samples = (uint64_t)traced * (uint64_t)sc->last_spp;
        }
        if (const rt_status ps = read_counters(sc->queue, sc->last_passes, sc->last)) return ps;
    }
    timing_out(sc->last, timing);
    return RT_OK;
}

#ifdef RTP_DEV_BUILD
// Developer hook (not part of the ABI header): the proof by exhaustion behind rt_device_math.h's recip() and sqrt_cr().
// Runs every one of the 2^32 binary32 bit patterns through them on the current device and counts the inputs whose result
// differs in any bit from the compiler's correctly rounded 1.0f / x and sqrtf(x) (NaN results count as equal to NaN).
// out[0]: mismatches of recip, out[1]: of sqrt_cr, out[2]: inputs compared.  Both must be 0.
namespace rtk {
__global__ void __launch_bounds__(256) fast_math_check_kernel(unsigned long long *out) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    unsigned long long bad_r = 0, bad_s = 0, seen = 0;
    for (uint64_t b = tid; b < (1ull << 32); b += stride) {
        const float x = __uint_as_float((uint32_t)b);
        const float wr = 1.0f / x, gr = rtd::recip(x);
        const float ws = sqrtf(x), gs = rtd::sqrt_cr(x);
        bad_r += (__float_as_uint(wr) != __float_as_uint(gr)) && !(wr != wr && gr != gr);
        bad_s += (__float_as_uint(ws) != __float_as_uint(gs)) && !(ws != ws && gs != gs);
        ++seen;
    }
    atomicAdd(&out[0], bad_r); atomicAdd(&out[1], bad_s); atomicAdd(&out[2], seen);
}
}  // namespace rtk
// The same for test_sphere's root selection (rt_kernel.hip.inc, sphere_root: both quotients from one fp64 reciprocal, no
// scaling): n operand sets (half_b, D, a, closest) — half of them raw random bit patterns (every exponent, infinities, NaN,
// denormals, zeros), half with exponents near the scene's scale — through sphere_root and through sphere_root_plain, the
// reference's form with the compiler's division.  out[0]: sets where "accepted" differs or the accepted t differs in any
// bit, out[1]: sets with an accepted root, out[2]: sets compared.
namespace rtk {
__global__ void __launch_bounds__(256) sphere_root_check_kernel(unsigned long long *out, unsigned long long n) {
    const uint64_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0, hits = 0, seen = 0;
    for (uint64_t i = tid; i < n; i += stride) {
        uint32_t h = rtd::wang_hash((uint32_t)i ^ 0x9e3779b9u) + (uint32_t)(i >> 32) * 0x85ebca6bu;
        uint32_t w[4];
        for (int k = 0; k < 4; ++k) { h = rtd::wang_hash(h + 0x632be5abu * (k + 1)); w[k] = h; }
        if (i & 1) {            // exponents within 2^-20 .. 2^20 of 1, random mantissas and signs
            for (int k = 0; k < 4; ++k) w[k] = (w[k] & 0x807fffffu) | ((107u + ((w[k] >> 23) & 255u) % 41u) << 23);
        }
        const float half_b = __uint_as_float(w[0]);
        const float disc = __uint_as_float(w[1] & 0x7fffffffu);          // test_sphere has returned for D < 0
        const float a = __uint_as_float(w[2] & 0x7fffffffu);             // a = |d|^2
        const float closest = __uint_as_float(w[3] & 0x7fffffffu);
        const double sq = (double)rtd::sqrt_cr(disc), nb = (double)(-half_b), da = (double)a;
        float tf = 0.0f, tp = 0.0f;
        const bool of = sphere_root(nb, sq, da, closest, tf), op = sphere_root_plain(nb, sq, da, closest, tp);
        bad += (of != op) || (of && __float_as_uint(tf) != __float_as_uint(tp));
        hits += op;
        ++seen;
    }
    atomicAdd(&out[0], bad); atomicAdd(&out[1], hits); atomicAdd(&out[2], seen);
}
}  // namespace rtk
// (both: a result block of three counters, zeroed, the check kernel run on it, copied to out)
static rt_status run_math_check(bool roots, uint64_t n, uint64_t out[3]) {
    if (!out) return fail(RT_ERR_INVALID_ARG, "null argument");
    unsigned long long *d = nullptr;
    Scratch mem;
    HIP_TRY(mem.alloc(d, 24));
    HIP_TRY(hipMemset(d, 0, 24));
    if (roots) hipLaunchKernelGGL(rtk::sphere_root_check_kernel, dim3(4096), dim3(256), 0, 0, d, (unsigned long long)n);
    else hipLaunchKernelGGL(rtk::fast_math_check_kernel, dim3(4096), dim3(256), 0, 0, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d, 24, hipMemcpyDeviceToHost));
    return RT_OK;
}
rt_status rt_debug_check_sphere_roots(uint64_t n, uint64_t out[3]) { return run_math_check(true, n, out); }
rt_status rt_debug_check_fast_math(uint64_t out[3]) { return run_math_check(false, 0, out); }

// Developer hooks (not part of the ABI header): the device LBVH builder (rt_build.hip) on its own, for the node-by-node check
// against a host reference (tests/dev_tree_checks.py, tests/lbvh_reference.py).
// rt_debug_guard_leaves: the inflated leaf boxes (6 floats each) and leaf codes a handle with tree_build = RT_BUILD_DEVICE_LBVH
// hands to build_lbvh for this scene and config.  *n_inout: capacity of the buffers in leaves (ignored when both are null), on
// return the number of leaves.  Fails when the scene is not eligible for the guarded walk (nothing would be built).
rt_status rt_debug_guard_leaves(const rt_scene_desc *d, const rt_config *cfg, float *boxes, int32_t *codes, int32_t *n_inout) {
    if (!d || !n_inout) return fail(RT_ERR_INVALID_ARG, "null argument");
    const rt_config c = config_from_caller(cfg);
    rtaccel::Packed pk;
    const std::string err = rtaccel::pack_scene(*d, rtaccel::TreeMode::GuardedLeaves, pk, pack_options(c, d));
    if (!err.empty()) return fail(RT_ERR_INVALID_ARG, err);
    if (!pk.guard.ok) return fail(RT_ERR_INVALID_ARG, "not eligible for the guarded walk: " + pk.guard.reason);
    const int32_t n = (int32_t)pk.guard_leaf_codes.size();
    if (boxes || codes) {
        if (!boxes || !codes || *n_inout < n) return fail(RT_ERR_INVALID_ARG, "leaf buffers missing or too small");
        std::memcpy(boxes, pk.guard_leaf_boxes.data(), sizeof(float) * 6 * (size_t)n);
        std::memcpy(codes, pk.guard_leaf_codes.data(), sizeof(int32_t) * (size_t)n);
    }
    *n_inout = n;
    return RT_OK;
}

// rt_debug_build_lbvh: build_lbvh on the caller's n leaves; copies the num_internal fp32 pair records (16 floats each) to
// nodes_out and the binary16 ones (8 floats each) to hnodes_out — both with room for n - 1 records — and sets
// info = {root, num_internal, depth, 0}.  The device tree is freed; nothing is rendered.
rt_status rt_debug_build_lbvh(const float *boxes, const int32_t *codes, int32_t n, float *nodes_out, float *hnodes_out, int32_t info[4]) {
    if (!boxes || !codes || !info || n <= 0 || (n > 1 && (!nodes_out || !hnodes_out))) return fail(RT_ERR_INVALID_ARG, "null argument or n <= 0");
    rtbuild::DeviceTree tree;
    const std::string err = rtbuild::build_lbvh(boxes, codes, n, tree);
    if (!err.empty()) return fail(RT_ERR_HIP, "device BVH build: " + err);
    info[0] = tree.root; info[1] = tree.num_internal; info[2] = tree.depth; info[3] = 0;
    hipError_t e = hipSuccess;
    if (tree.num_internal < 0 || tree.num_internal > n - 1) {
        (void)hipFree(tree.nodes); (void)hipFree(tree.hnodes);
        return fail(RT_ERR_HIP, "device BVH build: " + std::to_string(tree.num_internal) + " records for " + std::to_string(n) + " leaves");
    }
    if (tree.num_internal > 0) {
        e = hipMemcpy(nodes_out, tree.nodes, 64 * (size_t)tree.num_internal, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hnodes_out, tree.hnodes, 32 * (size_t)tree.num_internal, hipMemcpyDeviceToHost);
    }
    (void)hipFree(tree.nodes); (void)hipFree(tree.hnodes);
    HIP_TRY(e);
    return RT_OK;
}

// Developer hook (not part of the ABI header): the next render calls of this scene inject the fault the tripwire exists for
// (rt_kernel.hip.inc, RTP_TRIPWIRE) — rt_last_timing must then fail with RT_ERR_HIP and the tripwire's code instead of the
// launch hanging.  0 switches it off again.
rt_status rt_debug_trip_test(rt_scene *sc, uint32_t on) {
    if (!sc) return fail(RT_ERR_INVALID_ARG, "null argument");
    sc->trip_test = on;
    return RT_OK;
}

// Developer hook (not part of the ABI header): raw counters of an RTP_STATS build.
rt_status rt_debug_read_stats(rt_scene *sc, uint32_t out[16]) {
    if (!sc || !out) return fail(RT_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, sc->queue + kQueueStats, 60, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Developer hook (not part of the ABI header): the fog family's ray routines on the caller's rays, one ray per lane, for the ray-by-ray
// check against the CPU restatements (tests/dev_fog_ray_checks.py, tests/fog_ray_cases.py).  The kernel calls the inline
// functions the render kernels call — medium_interval, volume_walk, chroma_flight / chroma_tr, glow_flight, glow_pl, glow_line — on lights
// whose emitter table is value-initialised (these routines never read it), and writes eight words per ray:
//   0  medium_interval                                   hit, t0, t1
//   1  volume_walk<false> as fog_tr uses it              hit, acc, cells, exp_libm(-acc)
//   2  volume_walk<true> with rem = arg                  hit, event, v (the event's t, else the rem left over), cells
//   3  chroma_flight to the target R = arg, chroma_tr    hit, event, t, A (R at an event, as fog_vertex holds it), cells, tr of the three sigma_k
//   4  glow_flight of the draw u = arg                   hit, event, t, E, cells
//   5  glow_pl                                           pl, cells
//   6  glow_line                                         hit, G, cells
// An empty interval writes hit = 0 and zeros, an absent event t = 0; the words a routine does not name are 0.
namespace rtk {
struct FogRays {
    int32_t routine, n, grid;          // grid: 3 and 4 run on the VolumeLit base (else on the MediumLit one)
    MediumDev M;
    VolumeDev V;
    const float *heat, *pc;
    float s0, s1, s2;
    const float *o, *d, *t_end, *arg;
    uint32_t *out;
};
__global__ void __launch_bounds__(256) fog_rays_kernel(const FogRays A) {
    using Table = NeeTable;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.n) return;
    const f3 o = mk(A.o[3 * g], A.o[3 * g + 1], A.o[3 * g + 2]), d = mk(A.d[3 * g], A.d[3 * g + 1], A.d[3 * g + 2]);
    const float t_end = A.t_end[g], arg = A.arg[g];
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    FogCount n;
    float t0, t1;
    if (A.routine == 5) {
        w[0] = __float_as_uint(glow_pl(A.M, A.V, A.pc, o, d, n.cells));
        w[1] = (uint32_t)n.cells;
    } else if (A.routine == 6) {
        float G;
        if (glow_line(A.M, A.V, A.heat, o, d, t_end, G, n.cells)) {
            w[0] = 1;
            w[1] = __float_as_uint(G);
            w[2] = (uint32_t)n.cells;
        }
    } else if (medium_interval(A.M, o, d, t_end, t0, t1)) {
        w[0] = 1;
        const float len = sqrt_cr(lensq(d));
        if (A.routine == 0) {
            w[1] = __float_as_uint(t0);
            w[2] = __float_as_uint(t1);
        } else if (A.routine == 1) {
            float acc = 0.0f;
            volume_walk<false>(A.M, A.V, o, d, t0, t1, len, acc, n.cells);
            w[1] = __float_as_uint(acc);
            w[2] = (uint32_t)n.cells;
            w[3] = __float_as_uint(exp_libm(-acc));
        } else if (A.routine == 2) {
            float v = arg;
            w[1] = volume_walk<true>(A.M, A.V, o, d, t0, t1, len, v, n.cells) ? 1 : 0;
            w[2] = __float_as_uint(v);
            w[3] = (uint32_t)n.cells;
        } else if (A.routine == 3) {
            float t = 0.0f, Ad = 0.0f;
            bool event;
            if (A.grid) {
                VolumeLit<Table> B{};
                B.M = A.M;
                B.V = A.V;
                event = chroma_flight(B, o, d, t0, t1, len, arg, t, Ad, n);
            } else {
                MediumLit<Table> B{};
                B.M = A.M;
                event = chroma_flight(B, o, d, t0, t1, len, arg, t, Ad, n);
            }
            if (event) Ad = arg;
            w[1] = event ? 1 : 0;
            w[2] = event ? __float_as_uint(t) : 0;
            w[3] = __float_as_uint(Ad);
            w[4] = (uint32_t)n.cells;
            w[5] = __float_as_uint(chroma_tr(A.s0, Ad));
            w[6] = __float_as_uint(chroma_tr(A.s1, Ad));
            w[7] = __float_as_uint(chroma_tr(A.s2, Ad));
        } else {
            float t = 0.0f, E = 0.0f;
            bool event;
            if (A.grid) {
                GlowLit<VolumeLit<Table>> T{};
                T.B.M = A.M;
                T.B.V = A.V;
                T.heat = A.heat;
                event = glow_flight(T, o, d, t0, t1, len, arg, t, E, n);
            } else {
                GlowLit<MediumLit<Table>> T{};
                T.B.M = A.M;
                event = glow_flight(T, o, d, t0, t1, len, arg, t, E, n);
            }
            w[1] = event ? 1 : 0;
            w[2] = event ? __float_as_uint(t) : 0;
            w[3] = __float_as_uint(E);
            w[4] = (uint32_t)n.cells;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) A.out[8 * (size_t)g + k] = w[k];
}
}  // namespace rtk
// rt_debug_fog_rays: routine 0 … 6 (above) over n rays (o, d: 3 floats each; t_end and arg: one each; all host arrays) → out, 8 words per
// ray (a host array).  The medium, the grid, the heat (source 0: h = 1; 1: the density; 2: the heat grid, of the volume's dimensions) and
// the sampler are the public objects, converted as the render calls convert them: medium_setup's checks, the extinctions sigma_t * tint[k]
// over a base of sigma_t = 1 (routine 3), the cells' h by the source (4 and 6), the sampler's pc (5).  0 needs no grid; 1, 2, 5 and 6 need
// one; 3 and 4 run on the grid's base with one and on the homogeneous base without
rt_status rt_debug_fog_rays(int32_t routine, const rt_medium_params *medium, const rt_volume *volume, int32_t source, const rt_volume *heat,
                            const rt_glow_sampler *sampler, const float *tint, int32_t n, const float *o, const float *d, const float *t_end, const float *arg,
                            uint32_t *out) {
    const std::string w("rt_debug_fog_rays");
    if (routine < 0 || routine > 6) return fail(RT_ERR_INVALID_ARG, w + ": unknown routine " + std::to_string(routine));
    if (n <= 0 || !o || !d || !t_end || !arg || !out) return fail(RT_ERR_INVALID_ARG, w + ": null argument or n <= 0");
    rtk::FogRays A{};
    if (const rt_status st = medium_setup("rt_debug_fog_rays", medium, A.M)) return st;
    if (routine != 0 && !(A.M.sigma_t > 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": the routines behind the interval need sigma_t > 0");
    const bool needs_grid = routine == 1 || routine == 2 || routine == 5 || routine == 6;
    if (needs_grid && !volume) return fail(RT_ERR_INVALID_ARG, w + ": this routine needs a volume");
    if (volume && !(medium && A.M.region == 2)) return fail(RT_ERR_INVALID_ARG, w + ": a volume needs a medium with region 2 (the box the grid fills)");
    if (source < 0 || source > 2) return fail(RT_ERR_INVALID_ARG, w + ": source must be 0, 1 or 2");
    if (source != 0 && !volume) return fail(RT_ERR_INVALID_ARG, w + ": source 1 and 2 need a volume");
    if ((source == 2) != (heat != nullptr)) return fail(RT_ERR_INVALID_ARG, w + ": a heat grid is for source 2, and source 2 needs one");
    if (heat && (heat->nx != volume->nx || heat->ny != volume->ny || heat->nz != volume->nz))
        return fail(RT_ERR_INVALID_ARG, w + ": the heat grid's dimensions differ from the volume's");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if ((volume && volume->device != dev) || (heat && heat->device != dev) || (sampler && sampler->device != dev))
        return fail(RT_ERR_INVALID_ARG, w + ": a handle was created on another device than the current one");
    if (routine == 5) {
        if (!sampler || sampler->empty || !sampler->pc) return fail(RT_ERR_INVALID_ARG, w + ": glow_pl needs a sampler that is not empty");
        if (sampler->source != source || sampler->volume != volume || sampler->heat != heat)
            return fail(RT_ERR_INVALID_ARG, w + ": the sampler was built for another source or from other grids than the call's");
        A.pc = sampler->pc;
    }
    if (routine == 3) {
        if (!tint) return fail(RT_ERR_INVALID_ARG, w + ": chroma_flight needs a tint");
        float sigma[3];
        for (int k = 0; k < 3; ++k) {
            if (!(std::isfinite(tint[k]) && tint[k] >= 0.0f)) return fail(RT_ERR_INVALID_ARG, w + ": a tint channel is negative, NaN or infinite");
            sigma[k] = A.M.sigma_t * tint[k];
            if (!std::isfinite(sigma[k])) return fail(RT_ERR_INVALID_ARG, w + ": sigma_t * tint is not finite in a channel");
        }
        A.s0 = sigma[0];
        A.s1 = sigma[1];
        A.s2 = sigma[2];
        A.M.sigma_t = 1.0f;
    }
    A.routine = routine;
    A.n = n;
    A.grid = volume ? 1 : 0;
    if (volume) A.V = rtk::VolumeDev{volume->rho, volume->nx, volume->ny, volume->nz};
    A.heat = source == 0 ? nullptr : (source == 1 ? volume->rho : heat->rho);
    float *d_o = nullptr, *d_d = nullptr, *d_t = nullptr, *d_arg = nullptr;
    uint32_t *d_out = nullptr;
    Scratch mem;
    const size_t n3 = (size_t)n * 12, n1 = (size_t)n * 4, n8 = (size_t)n * 32;
    if (mem.alloc(d_o, n3) != hipSuccess || mem.alloc(d_d, n3) != hipSuccess || mem.alloc(d_t, n1) != hipSuccess || mem.alloc(d_arg, n1) != hipSuccess ||
        mem.alloc(d_out, n8) != hipSuccess)
        return fail(RT_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_o, o, n3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_d, d, n3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_t, t_end, n1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_arg, arg, n1, hipMemcpyHostToDevice));
    A.o = d_o;
    A.d = d_d;
    A.t_end = d_t;
    A.arg = d_arg;
    A.out = d_out;
    hipLaunchKernelGGL(rtk::fog_rays_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, n8, hipMemcpyDeviceToHost));
    return RT_OK;
}

// Developer hook (not part of the ABI header): the light-sampling routines on the caller's vertices, one vertex per lane, for the
// vertex-by-vertex check against the CPU restatements (tests/dev_light_vertex_checks.py, tests/light_vertex_cases.py).  The
// kernel calls the inline functions the render kernels call — light_sample, light_emitted, light_miss, nee_pick, tree_pick, tree_pmf,
// emit_find / nee_find, gloss_pg, PbPhase — on the light the lit calls would hand their kernels, and writes 16 words per vertex:
//   0  light_sample on the emitter table, under the call's Pb     ok, dir (3), c (3), code, seed after
//   1  light_sample on the environment, under the call's Pb       ok, dir (3), c (3), seed after
//   2  light_emitted of the ray (o = x, d = v) that found         the bool carry's (3), the float carry's with carry = n[0] (3);
//      primitive code `seed` at closest = s                       emitted going in is beta * a
//   3  light_miss of the environment, direction v                 depth 0 and 1 with the bool carry (3 + 3), depth 1 and 0 with the float
//                                                                 carry n[0] (3 + 3)
//   4  the picks alone                                            nee_pick(u = s); on a tree: tree_pick's entry, its p, seed after,
//                                                                 tree_pmf(e = (int)n[0], x); emit_find / nee_find of code / sphere `seed`
//   5  the two densities                                          gloss_pg(w = x, r = v, fuzz = s), PbPhase{ud = n, g = s}(w = x)
// A refused sample writes ok = 0, zeros and the seed after; the words a routine does not name are 0.  Pb: 0 PbDiffuse, 1 PbGlossy{r = v,
// fuzz = s}, 2 PbPhase{ud = n, g = s} (with n = ud, as the medium vertex passes it).
extern "C++" {
namespace rtk {
struct LightVertices {
    int32_t routine, n;
    const float *x, *nv, *v, *s;
    const uint32_t *seed;
    f3 a, beta;
    uint32_t *out;
};
template <int kPb> struct PbOf;
template <> struct PbOf<0> {
    __device__ static PbDiffuse make(f3, f3, float) { return PbDiffuse{}; }
};
template <> struct PbOf<1> {
    __device__ static PbGlossy make(f3, f3 v, float s) { return gloss_pb(v, s); }
};
template <> struct PbOf<2> {
    __device__ static PbPhase make(f3 nv, f3, float s) {
        PbPhase p;
        p.ud = nv;
        p.g = s;
        return p;
    }
};
__device__ __forceinline__ void put3(uint32_t *w, f3 c) {
    w[0] = __float_as_uint(c.x);
    w[1] = __float_as_uint(c.y);
    w[2] = __float_as_uint(c.z);
}
template <class Light, int kPb>
__global__ void __launch_bounds__(256) light_vertices_kernel(const KParams P, const Light T, const LightVertices A) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.n) return;
    const f3 x = ld3(A.x + 3 * g), nv = ld3(A.nv + 3 * g), v = ld3(A.v + 3 * g);
    const float s = A.s[g];
    const uint32_t seed = A.seed[g];
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = 0;
    if (A.routine == 0 || A.routine == 1) {
        uint32_t ls = seed;
        f3 dir = mk(0, 0, 0), c = mk(0, 0, 0);
        int32_t code = 0;
        if (light_sample(P, T, ls, x, nv, A.a, A.beta, PbOf<kPb>::make(nv, v, s), dir, c, code)) {
            w[0] = 1;
            put3(w + 1, dir);
            put3(w + 4, c);
            if (A.routine == 0) w[7] = (uint32_t)code;
        }
        w[A.routine == 0 ? 8 : 7] = ls;
    }
    if constexpr (kPb == 0) {
        if (A.routine == 2 || A.routine == 3) {
            Lane L;
            L.o = x;
            L.d = v;
            L.closest = s;
            L.hit = A.routine == 2 ? (int32_t)seed : -1;
            L.beta = A.beta;
            L.color = mk(0, 0, 0);
            L.seed = 0;
            L.depth = 0;
            const float carry = nv.x;
            if (A.routine == 2) {
                const f3 emitted = mul(A.beta, A.a);
                put3(w + 0, light_emitted(P, T, L, L.hit >> 1, (L.hit & 1) != 0, true, emitted));
                put3(w + 3, light_emitted(P, T, L, L.hit >> 1, (L.hit & 1) != 0, carry, emitted));
            } else {
                put3(w + 0, light_miss(P, T, L, true));
                put3(w + 9, light_miss(P, T, L, carry));
                L.depth = 1;
                put3(w + 3, light_miss(P, T, L, true));
                put3(w + 6, light_miss(P, T, L, carry));
            }
        }
        if constexpr (kEmitterTable<Light>) {
            if (A.routine == 4) {
                const auto &B = emitter_base(T);
                w[0] = (uint32_t)nee_pick(B, s);
                if constexpr (std::is_same_v<Light, TreeTable> || std::is_same_v<Light, TreeEmitTable>) {
                    uint32_t ls = seed;
                    float p;
                    w[1] = (uint32_t)tree_pick(T.L, ls, x, p);
                    w[2] = __float_as_uint(p);
                    w[3] = ls;
                    w[4] = __float_as_uint(tree_pmf(T.L, (int32_t)nv.x, x));
                }
                if constexpr (std::is_same_v<std::decay_t<decltype(B)>, NeeTable>) w[5] = (uint32_t)nee_find(B, (int32_t)seed);
                else w[5] = (uint32_t)emit_find(B, (int32_t)seed);
            }
        }
        if (A.routine == 5) {
            w[0] = __float_as_uint(gloss_pg(x, v, s));
            PbPhase ph;
            ph.ud = nv;
            ph.g = s;
            w[1] = __float_as_uint(ph(x));
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) A.out[16 * (size_t)g + k] = w[k];
}
}  // namespace rtk
template <class Light>
void launch_light_vertices(const rtk::KParams &P, const Light &T, const rtk::LightVertices &A, int32_t pb) {
    const dim3 grid((A.n + 255) / 256), block(256);
    if (pb == 1) hipLaunchKernelGGL((rtk::light_vertices_kernel<Light, 1>), grid, block, 0, 0, P, T, A);
    else if (pb == 2) hipLaunchKernelGGL((rtk::light_vertices_kernel<Light, 2>), grid, block, 0, 0, P, T, A);
    else hipLaunchKernelGGL((rtk::light_vertices_kernel<Light, 0>), grid, block, 0, 0, P, T, A);
}
}  // extern "C++"
// rt_debug_light_vertices: routine 0 … 5 (above) under Pb kind pb over n vertices (x, nv, v: 3 floats each; s and seed: one each; all host
// arrays) → out, 16 words per vertex (a host array).  ab: the call's albedo a and throughput beta (6 floats).  The scene, the emitter
// parameters, the environment (routines 1 and 3; else it may be null) and its parameters are the public objects, converted as the render
// calls convert them: nee_setup and env_setup's checks, with_emitter_table's choice of table, env_dev_of, and the KParams fill_params
// makes of the scene and the camera (the background and max_depth).  What a routine uses as an index is checked here, before any launch:
// routine 2's code must name a primitive of the scene, routine 4's entry (int)n[0] an entry of the tree's table.  pb = 1 is refused when
// the light's glossy switch is off (no call runs PbGlossy then); routines 2 … 5 take pb = 0
rt_status rt_debug_light_vertices(rt_scene *sc, const rt_camera_data *cam, const rt_nee_params *nee, const rt_env *env, const rt_env_params *env_params,
                                  int32_t routine, int32_t pb, int32_t n, const float *x, const float *nv, const float *v, const float *s,
                                  const uint32_t *seed, const float *ab, uint32_t *out) {
    const std::string w("rt_debug_light_vertices");
    if (routine < 0 || routine > 5) return fail(RT_ERR_INVALID_ARG, w + ": unknown routine " + std::to_string(routine));
    if (pb < 0 || pb > 2 || (routine > 1 && pb != 0)) return fail(RT_ERR_INVALID_ARG, w + ": pb must be 0, 1 or 2, and 0 for the routines 2 to 5");
    if (n <= 0 || !x || !nv || !v || !s || !seed || !ab || !out) return fail(RT_ERR_INVALID_ARG, w + ": null argument or n <= 0");
    NeeSetup N;
    if (const rt_status st = nee_setup("rt_debug_light_vertices", nee, N)) return st;
    rt_env_params np;
    if (const rt_status st = env_setup("rt_debug_light_vertices", env_params, np)) return st;
    const bool sky = routine == 1 || routine == 3;
    if (sky && !env) return fail(RT_ERR_INVALID_ARG, w + ": this routine needs an environment");
    if (pb == 1 && !(sky ? np.glossy : N.glossy)) return fail(RT_ERR_INVALID_ARG, w + ": pb = 1 needs the light's glossy switch");
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(ab[k])) return fail(RT_ERR_INVALID_ARG, w + ": a or beta is not finite");
    rtk::KParams P;
    if (const rt_status st = fill_params(sc, cam, nullptr, P)) return st;
    if (const rt_status st = check_device(sc)) return st;
    if (sky && env->device != sc->device) return fail(RT_ERR_INVALID_ARG, w + ": the environment was created on another device than the scene");
    for (int32_t k = 0; k < n; ++k) {
        for (int c = 0; c < 3; ++c)
            if (!(std::isfinite(x[3 * k + c]) && std::isfinite(nv[3 * k + c]) && std::isfinite(v[3 * k + c]) && std::isfinite(s[k])))
                return fail(RT_ERR_INVALID_ARG, w + ": a vertex is not finite");
        if (routine == 2) {
            const int32_t code = (int32_t)seed[k];
            if (code < 0 || (code >> 1) >= ((code & 1) ? sc->num_planes : sc->num_spheres))
                return fail(RT_ERR_INVALID_ARG, w + ": a code names no primitive of the scene");
        }
    }
    rtk::LightVertices A{};
    A.routine = routine;
    A.n = n;
    A.a = rtk::mk(ab[0], ab[1], ab[2]);
    A.beta = rtk::mk(ab[3], ab[4], ab[5]);
    float *d_x = nullptr, *d_n = nullptr, *d_v = nullptr, *d_s = nullptr;
    uint32_t *d_seed = nullptr, *d_out = nullptr;
    Scratch mem;
    const size_t n3 = (size_t)n * 12, n1 = (size_t)n * 4, n16 = (size_t)n * 64;
    if (mem.alloc(d_x, n3) != hipSuccess || mem.alloc(d_n, n3) != hipSuccess || mem.alloc(d_v, n3) != hipSuccess || mem.alloc(d_s, n1) != hipSuccess ||
        mem.alloc(d_seed, n1) != hipSuccess || mem.alloc(d_out, n16) != hipSuccess)
        return fail(RT_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    HIP_TRY(hipMemcpy(d_x, x, n3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_n, nv, n3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_v, v, n3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_s, s, n1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_seed, seed, n1, hipMemcpyHostToDevice));
    A.x = d_x;
    A.nv = d_n;
    A.v = d_v;
    A.s = d_s;
    A.seed = d_seed;
    A.out = d_out;
    rt_status st = RT_OK;
    if (sky) {
        launch_light_vertices(P, env_dev_of(env, np), A, pb);
    } else {
        st = with_emitter_table(sc, N, true, [&](const auto &T) {
            using Table = std::decay_t<decltype(T)>;
            constexpr bool tree = std::is_same_v<Table, rtk::TreeTable> || std::is_same_v<Table, rtk::TreeEmitTable>;
            int32_t count;
            if constexpr (tree) count = T.N.count;
            else count = T.count;
            if ((routine == 0 || routine == 2) && count <= 0) return fail(RT_ERR_INVALID_ARG, w + ": the emitter table is empty (light_on is false: no call samples it)");
            if constexpr (tree) {
                if (routine == 4)
                    for (int32_t k = 0; k < n; ++k) {
                        if (!(nv[3 * k] >= 0.0f && nv[3 * k] < (float)count)) return fail(RT_ERR_INVALID_ARG, w + ": tree_pmf's entry is outside the table");
                    }
            }
            launch_light_vertices(P, T, A, pb);
            return RT_OK;
        });
    }
    if (st != RT_OK) return st;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, n16, hipMemcpyDeviceToHost));
    return RT_OK;
}

#endif      // RTP_DEV_BUILD

rt_status rt_last_kernel_ms(rt_scene *sc, float *ms) {
    if (!sc || !ms) return fail(RT_ERR_INVALID_ARG, "null argument");
    *ms = 0.0f;
    if (!sc->timed) return RT_OK;
    return sc->clock[kClockRender].elapsed(*ms);
}

rt_status rt_render_to_host(rt_scene *sc, const rt_camera_data *cam, const rt_shard *shard, float *h_fb_sum, rt_timing *timing) {
    if (!sc || !cam || !h_fb_sum) return fail(RT_ERR_INVALID_ARG, "null argument");
    const int32_t rows = rt_shard_rows(cam->image_height, shard);
    const size_t bytes = (size_t)rows * (size_t)(cam->image_width > 0 ? cam->image_width : 0) * 3 * sizeof(float);
    if (bytes == 0) return RT_OK;
    float *d_fb = nullptr;
    Scratch mem;
    HIP_TRY(mem.alloc(d_fb, bytes));
    rt_status st = rt_render(sc, cam, shard, d_fb, nullptr, 1, timing);
    if (st == RT_OK && hipMemcpy(h_fb_sum, d_fb, bytes, hipMemcpyDeviceToHost) != hipSuccess) st = fail(RT_ERR_HIP, "hipMemcpy D2H failed");
    return st;
}

rt_status rt_trace_samples(rt_scene *sc, const rt_camera_data *cam, int32_t n, const int32_t *ijs, float *radiance,
                           int32_t *rays, uint32_t *final_seed) {
    if (n < 0 || (n > 0 && (!ijs || !radiance || !rays || !final_seed))) return fail(RT_ERR_INVALID_ARG, "null argument");
    rtk::KParams P;
    rt_status st = fill_params(sc, cam, nullptr, P);
    if (st != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    return run_probe("", P, cam, n, ijs, radiance, rays, final_seed, nullptr, nullptr, [&](const rtk::KParams &KP, uint32_t *, uint32_t *) {
        hipLaunchKernelGGL(rtk::probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, KP);
        return RT_OK;
    });
}

rt_status rt_closest_hits(rt_scene *sc, int32_t n, const float *origins, const float *directions, int32_t *hit, float *t, int32_t *prim) {
    if (!sc || n < 0 || (n > 0 && (!origins || !directions || !hit || !t || !prim))) return fail(RT_ERR_INVALID_ARG, "null argument");
    if (n == 0) return RT_OK;
    rt_camera_data cam{};
    cam.image_width = cam.image_height = 1;
    cam.samples_per_pixel = cam.max_depth = 1;
    rtk::KParams P;
    rt_status st = fill_params(sc, &cam, nullptr, P);
    if (st != RT_OK) return st;
    if ((st = check_device(sc)) != RT_OK) return st;
    float *d_o = nullptr, *d_d = nullptr, *d_t = nullptr;
    int32_t *d_hit = nullptr, *d_prim = nullptr;
    Scratch mem;
    const size_t n3 = (size_t)n * 12, n1 = (size_t)n * 4;
    if (mem.alloc(d_o, n3) != hipSuccess || mem.alloc(d_d, n3) != hipSuccess || mem.alloc(d_t, n1) != hipSuccess || mem.alloc(d_hit, n1) != hipSuccess ||
        mem.alloc(d_prim, n1) != hipSuccess)
        return fail(RT_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    hipError_t e = hipMemcpy(d_o, origins, n3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_d, directions, n3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_t, 0, n1);
    if (e == hipSuccess) e = hipMemset(d_prim, 0xff, n1);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rtk::closest_hit_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, P, d_o, d_d, n, d_hit, d_t, d_prim);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(hit, d_hit, n1, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(t, d_t, n1, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(prim, d_prim, n1, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("closest-hit probe: ") + hipGetErrorString(e));
    return RT_OK;
}

rt_status rt_device_alloc(uint64_t bytes, void **out) {
    if (!out) return fail(RT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (bytes == 0) return RT_OK;
    HIP_TRY(hipMalloc(out, bytes));
    return RT_OK;
}

rt_status rt_device_free(void *p) {
    if (p) HIP_TRY(hipFree(p));
    return RT_OK;
}

rt_status rt_copy_to_host(void *dst, const void *src, uint64_t bytes) {
    if (bytes == 0) return RT_OK;
    if (!dst || !src) return fail(RT_ERR_INVALID_ARG, "null argument");
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_tonemap(const float *d_fb_sum, uint8_t *d_rgb8, int64_t num_floats, int32_t divisor, void *hip_stream) {
    if (num_floats <= 0) return RT_OK;
    if (!d_fb_sum || !d_rgb8) return fail(RT_ERR_INVALID_ARG, "null argument");
    const float inv = (float)(1.0 / (double)(float)divisor);     // pixel_color / samplesPerPixel, include/vec3.h:97
    int64_t blocks = (num_floats + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rtk::tonemap_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, d_fb_sum, d_rgb8, num_floats, inv);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

rt_status rt_tonemap_spp(const float *d_fb_sum, const int32_t *d_spp, uint8_t *d_rgb8, int64_t num_pixels, void *hip_stream) {
    if (num_pixels <= 0) return RT_OK;
    if (!d_fb_sum || !d_spp || !d_rgb8) return fail(RT_ERR_INVALID_ARG, "null argument");
    if (num_pixels > ((int64_t)1 << 40)) return fail(RT_ERR_UNSUPPORTED, "rt_tonemap_spp: more than 2^40 pixels");
    const int64_t n = 3 * num_pixels;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rtk::tonemap_spp_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, d_fb_sum, d_spp, d_rgb8, n);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

}  // extern "C"
