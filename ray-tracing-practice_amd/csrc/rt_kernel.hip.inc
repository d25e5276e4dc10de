// rt_kernel.hip.inc — the gfx950 render kernel (included by rt_capi.hip).
//
// Replaces the reference's render_kernel + ray_color + hit_scene/hit_bvh + hit_sphere/hit_plane
// + material_scatter (src/camera.cu:17-34,218-252; include/bvh.h:19-65; include/sphere.h:24-53;
// include/plane.h:57-96; include/materials.h:70-140).
//
// Shape of the computation (not the reference's one-thread-per-pixel grid):
//   * the unit of work is one SAMPLE: a frame is rendered in passes of S samples per pixel (S from
//     the slab budget, the whole frame where it fits);
//     render_kernel traces the samples of a pass in any order into a slab of per-sample
//     radiances and accumulate_kernel then adds them to the pixel sums in sample order (float
//     addition is not associative; the reference adds in order, src/camera.cu:27-31);
//   * persistent workgroups (768 threads, two per CU: 6 waves per SIMD; the sphere-only build of the guarded walk 1024
//     threads, 8 waves per SIMD); the traversal tables (nodes, spheres, planes, one material row) are staged once into
//     LDS, together with a small block of launch constants that would otherwise be spilled scalar registers;
//   * a wave reserves up to 1024 consecutive samples (of one or two pixels) with one atomic and deals them 64 at a time
//     (ballot + mbcnt), so its lanes start with coherent primary rays; a lane that finishes a path takes the next sample;
//   * each lane is a small state machine: BOX/PAIR (test one node's box / both child boxes), LEAF (test a primitive),
//     SHADE (material + scatter + next ray or next sample).  A wave runs one kind of step at a
//     time for the lanes that want it, chosen from ballots of the lane states, so lanes whose
//     path ended early are re-armed at the next SHADE step instead of idling until the slowest
//     path of the wave is done.
//
// Traversal, two walks with the same result (docs/LOG.md §3, §3b):
//   * exact ("threaded", kThreaded = true): the caller's BVH in the reference's own visit order (node
//     table with skip links, no stack), so every box and primitive test sees the same running
//     closest-hit distance as hit_bvh does — bit-identical even where float round-off makes the
//     result order dependent;
//   * guarded (kThreaded = false): near-first walk of this library's SAH tree over inflated leaf boxes
//     (two boxes per step — LDS records laid out so that the ray's octant selects near and far planes by address,
//     step_octant — short LDS stack).  Whatever could make its result differ from the
//     reference's — a final hit in front of its own leaf box, an exact tie, a full stack, a ray from
//     beyond the distance the inflation was sized for — flags the SAMPLE, which a second launch
//     re-walks exactly.
// Camera rays (kPrim = true, rt_primary.hip.inc): where the guarded walk's tables allow it, a pass BEFORE this kernel has found
// the first hit of every sample from a per-pixel candidate list and left it in the sample's slot of the slab; a lane that takes
// a new sample reads it there and goes through the shade step it is already in — the walk only sees rays that left a surface.
// The per-primitive arithmetic is the reference's, evaluated without FMA contraction (see rt_device_math.h).
// What shaped the instruction selection: the measured cost of each instruction kind on this SIMD (docs/LOG.md §5g).
#pragma once

namespace rtk {

using namespace rtd;

constexpr int kWave = 64;
constexpr int32_t kDone = INT32_MIN;     // traversal finished / no hit
#ifndef RTP_BLOCK
#define RTP_BLOCK 768
#endif
#ifndef RTP_MIN_WAVES
#define RTP_MIN_WAVES 6
#endif
#ifndef RTP_UNROLL
#define RTP_UNROLL 4
#endif
#ifndef RTP_LDS_MAT_ROWS
#define RTP_LDS_MAT_ROWS 1        /* material rows kept in LDS (row 0: albedo + type; row 1, emission + fuzz, and row 2 come from global memory) */
#endif
#ifndef RTP_UNROLL_WIDE
#define RTP_UNROLL_WIDE 3       /* steps on 4-wide nodes per vote (each does the work of two pair steps; 1: -0.6 %, 3 as good as any on configs[4]) */
#endif
// ---- tripwire (developer build) -------------------------------------------------------------------------------------------
// The wave's step-kind vote relies on an invariant nothing else enforces: every live lane is exactly ONE of walking (node >= 0),
// stuck at a leaf with its park slot full, or finished (node == kDone).  A lane in none of them is never offered a step — the
// vote picks nothing for it, the loop spins, and the launch ends in a watchdog kill of the box (round 3's "second park slot"
// experiment did exactly that).  With RTP_TRIPWIRE the kernel checks the partition at every vote and counts main-loop rounds in
// which no lane's state changed; either failing writes a code to the abort word (stats[15]: rt_last_timing returns RT_ERR_HIP
// with it) and the wave leaves the kernel — a failed assert instead of a hung GPU.  KParams::trip_test injects the fault.
#ifndef RTP_TRIPWIRE
#ifdef RTP_DEV_BUILD
#define RTP_TRIPWIRE 1
#else
#define RTP_TRIPWIRE 0
#endif
#endif
constexpr uint32_t kTripPartition = 0x54524901u;     // a live lane that is neither walking, stuck nor finished
constexpr uint32_t kTripNoProgress = 0x54524902u;    // kTripRounds rounds of the main loop without any lane changing state
constexpr int kTripRounds = 4096;
#ifdef RTP_STATS
// Developer build only: per-phase step/lane counters, summed into P.queue[8..] at kernel end.
#define RTP_COUNT(slot, lanes) do { st_iters[slot]++; st_lanes[slot] += (uint32_t)__popcll(__ballot(lanes)); } while (0)
#define RTP_STAMP(slot) do { const uint64_t now_ = __builtin_amdgcn_s_memtime(); st_cycles[slot] += now_ - st_last; st_last = now_; } while (0)
#define RTP_WHY(k) (1 << (26 + (k)))      /* diagnostic: which guard flagged the sample (0 stack, 1 tie, 2 final, 3 origin) */
#else
#define RTP_COUNT(slot, lanes) do { } while (0)
#define RTP_STAMP(slot) do { } while (0)
#define RTP_WHY(k) 0
#endif
constexpr int kBlock = RTP_BLOCK;            // threads per workgroup; RTP_MIN_WAVES waves per SIMD are resident
// The sphere-only specialisation of the octant walk (render_kernel<…, kSimple = true>: no plane and no texture code, all
// material rows from global memory) needs 64 VGPRs instead of 80: 1024-thread workgroups, two per CU, 8 waves per SIMD.
constexpr int kSimpleBlock = 1024;
constexpr int kSimpleWaves = 8;

using Magic = rtaccel::Magic;         // (rt_accel.h: make_magic)

struct KParams {
    // CameraData (include/camera.cuh:86-95)
    float origin[3], p00[3], du[3], dv[3], bg[3];
    int32_t width, height, spp, max_depth;
    // rows rendered by this call (rt_shard) …
    int32_t local_rows, band_rows, num_parts, part;
    // … or the rectangle (rt_render_tile): row_w pixels per local row (the image width for whole rows), first column and row
    int32_t row_w, tile_x0, tile_y0;
    // scene tables (global memory)
    const float4 *nodes;     int32_t num_internal; int32_t root;     // guarded walk, fp32 pair records (LDS-resident scenes)
    const float4 *hnodes;                                            // the same records with binary16 planes (global-memory scenes)
    const float4 *whnodes;   int32_t wroot;                          // guarded walk with distance-aware margins, 4-wide nodes (binary16 boxes)
    const float4 *tnodes;    int32_t num_tnodes;          // reference-order (threaded) node table
    const float4 *xnodes;    int32_t num_top;             // explicit-link copy, records [0,num_top) = LDS treelet
    const float4 *spheres;   int32_t num_spheres;
    const float4 *planes;    int32_t num_planes;
    const float4 *materials; int32_t num_materials;
    const int32_t *sphere_mat;
    const float4 *tex_data;  const int4 *tex_info;
    // output + work queue
    float *fb;
    float *slab;             // per-sample radiance of the current pass: 3 floats at [local pixel][slot], slab_pitch slots per pixel
    uint32_t slab_pitch;     // pass_count rounded up to a multiple of 32 (rows start on 128-byte lines)
    uint32_t num_pixels;     // local pixels of this call
    int32_t pass_first, pass_count;   // samples pass_first .. pass_first + pass_count - 1
    Magic magic_count, magic_width, magic_band;       // reciprocals of pass_count, width, band_rows (div_magic)
    uint32_t *queue;         // next work index (one counter per pass)
    uint32_t chunk;          // work indices a wave reserves per atomic (multiple of 64) …
    uint32_t taper_shift;    // … shrinking to (remaining >> taper_shift) near the end of the pass
    uint32_t full_chunk, full_taper;   // the same for an exact re-walk that turns out to cover the whole pass
    uint32_t *stats;         // RTP_STATS builds only (and the abort word, stats[15])
    uint32_t trip_test;      // RTP_TRIPWIRE builds: 1 = one lane is put into a state the vote does not know (fault injection)
    uint32_t total_work;     // work indices of this pass: local pixels * pass_count
    int32_t stack_levels;    // LDS stack rows per lane
    int32_t k_inner, k_shade; // scheduling thresholds (lanes)
    // guarded near-first walk (docs/LOG.md §3b): exact leaf boxes for the final check, the far-origin test,
    // and the list of samples handed to the exact walk
    const float4 *leaf_boxes;          // per sphere, or null: boxes are fl(c -/+ r)
    const float4 *plane_leaf_boxes;    // per plane
    float g_center[3]; float g_d0sq, g_rs, g_fark; float g_box[6];
    float g_dynk;                      // distance-aware margins (kDyn kernels): box growth per squared distance to the farthest corner
    float g_dyn_sqrtk, g_dyn_b;        // … in the parametric form of step_pair_par: sqrt(dyn_k) and sqrt(dyn_k) * sqrt(3) * (largest small radius), rounded up
    float g_dyn_c3, g_dyn_kslack;      // sqrt(dyn_k) * sqrt(3); dyn_k with the walk's slack (products the kernel would otherwise hold in vector registers)
    // front primitives (rt_accel.h, Packed::Guard): not in the guarded walk's tree — every ray tests them as it is armed
    // (arm_ray), the per-pixel candidate lists take them from here (cand_kernel): codes 2 * index + type, inflated leaf boxes
    int32_t num_front; int32_t front_code[4]; float front_box[4 * 6];
    uint32_t *flag_list; uint32_t *flag_count; uint32_t flag_cap;
    // in-launch bail-out of a guarded pass (retire_sample): one word per pass, set by the wave that finds the flagged share of
    // the samples handed out so far above bail_share / 256 — every wave stops fetching at its next reservation, the exact walk
    // then takes the WHOLE pass (its launch reads the same word) and the accumulate launches choose by it.  null: never
    uint32_t *abandon; uint32_t bail_share; uint32_t bail_floor, bail_latest;        // (bail_floor: in 1/1024ths of the pass, bail_latest: in eighths)
    // a wave that keeps flagging reserves slots of the list kFlagChunk at a time; its chunk lives in flag_chunk_words (2, or 0: none to
    // spare) LDS words per wave (flag_collect)
    uint32_t flag_chunk_words;
    // Where a flagged sample's path stood when its ray was armed (resume table: below, "the flagged-sample list"): tags (work index
    // + 1; 0: free) and 64-byte states, resume_mask + 1 entries; null: the exact walk restarts every flagged sample from the camera
    uint32_t *resume_tag; float4 *resume_state; uint32_t resume_shift;
    // pixels with a flagged sample in this pass (accumulated after the exact re-walk, beside which the other pixels are summed):
    // a mark per local pixel, the list of marked pixels, its length — null when the re-walk is not overlapped
    uint32_t *dirty; uint32_t *dirty_list; uint32_t *dirty_count;
    // work taken from a list instead of [0, total_work): the exact re-walk of flagged samples
    const uint32_t *work_list; const uint32_t *work_count; uint32_t work_cap;
    // the guarded kernels' constants block as the host lays it out (fill_consts): the workgroup copies it to LDS, 16 bytes at a time
    uint32_t consts[14 * 4];
    // primary visibility (rt_primary.hip.inc): per local pixel kCandWords words — the number of candidate leaves of the pixel's
    // primary rays (kCandNone: no list) and their codes; null: every sample walks the tree from the camera
    const uint32_t *cand;
    // … and the order the trace kernel takes the pixels in (order_* kernels): one row of kOrderRowWords words (16 bytes) per position
    // of the fetch order — the centre of that pixel on the image plane (what camera_ray builds from the pixel) and the local pixel
    const uint32_t *order;
    const uint32_t *traced_pixels;      // one word: how many pixels the table's front part holds (those with candidates; the others are finished by the primary pass)
    // probe mode (rt_trace_samples)
    const int32_t *probe_ijs; float *probe_rad; int32_t *probe_rays; uint32_t *probe_seed; int32_t probe_n;
};

struct Lane {
    f3 o, d, inv;
    float closest;
    int32_t hit;       // primitive code (2*index + type) of the closest hit so far, -1 = none
    int32_t node;      // guarded walk: >= 0 inner node, < 0 leaf code; exact walk: next node index;
                       // kDone = traversal finished
    int32_t sp;        // guarded walk: stack entries; exact walk: pending primitive code + 1, 0 = none
    int32_t pend;      // guarded walk (render_kernel): leaf code of a parked primitive test, 0 = none
    float e;           // step_pair_par: the growth the children of the lane's current node are tested with
    uint32_t seed;
    f3 beta, color;
    int32_t depth;
};

__device__ __forceinline__ f3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ int32_t as_int(float f) { return __float_as_int(f); }

// kClamp (the guarded walks): 1 / d is kept CLAMPED to +-1e18 — what their box tests want (below) — so that the lane holds one
// copy of it, not the exact one for the final check beside a clamped one for the walk; inv_exact() gives the exact value back.
template <bool kClamp = false>
__device__ __forceinline__ void begin_ray(Lane &L, f3 o, f3 d, int32_t root) {
    L.o = o;
    L.d = d;
    // AABB::hit computes 1 / direction[a] per call (include/aabb.h:44); it is the same value every time
#if RTP_FAST_RCP_SQRT && defined(__HIP_DEVICE_COMPILE__)
    // (rt_device_math.h, recip: the three estimates share ONE fence test and one fallback branch)
    L.inv = mk(recip_estimate(d.x), recip_estimate(d.y), recip_estimate(d.z));
    if (__builtin_expect(!(recip_in_fence(d.x) && recip_in_fence(d.y) && recip_in_fence(d.z)), 0)) L.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
#else
    L.inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
#endif
    if (kClamp) L.inv = mk(__builtin_amdgcn_fmed3f(L.inv.x, -1e18f, 1e18f), __builtin_amdgcn_fmed3f(L.inv.y, -1e18f, 1e18f), __builtin_amdgcn_fmed3f(L.inv.z, -1e18f, 1e18f));
    L.closest = 1e30f;            // Interval(0.001f, 1e30f), src/camera.cu:226
    L.hit = -1;
    L.node = root;
    L.sp = 0;
    L.pend = 0;
}

// kSent (the octant walk of render_kernel): L.sp is a BYTE offset into the lane's stack column (256 bytes per level: one
// v_add instead of a shift-and-add per access) and level 0 holds kDone for good, written once per kernel — a pop needs no
// "anything left?" test, the lane that pops the sentinel is simply finished and never pops again.
constexpr int32_t kLevelBytes = kWave * 4;
template <bool kSent = false>
__device__ __forceinline__ void pop(Lane &L, const uint32_t *stack) {
    if (kSent) {
        L.sp -= kLevelBytes;
        L.node = (int32_t)*reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(stack) + L.sp);
    } else if (L.sp > 0) {
        L.sp--;
        L.node = (int32_t)stack[L.sp * kWave];
    } else {
        L.node = kDone;
    }
}

// AABB::hit (include/aabb.h:42-65) for one box given as lo/hi per axis; returns hit and the
// clipped entry distance (used only to order the two children).
// 1 / direction as AABB::hit divides it (include/aabb.h:44), from a lane whose copy may be the clamped one (begin_ray<true>): a
// component short of the clamp IS the exact value; one at it (|d| <= 1e-18, or 0: 1 / d infinite) is divided again — the same
// IEEE quotient begin_ray made.  Rare enough for the branch to be skipped by whole waves.
__device__ __forceinline__ f3 inv_exact(const Lane &L) {
    f3 v = L.inv;
    if (__builtin_expect(!(fabsf(v.x) < 1e18f && fabsf(v.y) < 1e18f && fabsf(v.z) < 1e18f), 0)) v = mk(1.0f / L.d.x, 1.0f / L.d.y, 1.0f / L.d.z);
    return v;
}
// kClamped: the lane's 1 / d is the clamped copy (begin_ray<true>)
template <bool kClamped = false>
__device__ __forceinline__ bool slab(const Lane &L0, float lox, float loy, float loz, float hix, float hiy, float hiz,
                                      float t_far, float &t_enter) {
    struct { f3 o, inv; } L = {L0.o, kClamped ? inv_exact(L0) : L0.inv};
    const bool sx = L.inv.x < 0, sy = L.inv.y < 0, sz = L.inv.z < 0;
    const float nx = sx ? hix : lox, fx = sx ? lox : hix;     // the swap of t1/t2, applied to the planes
    const float ny = sy ? hiy : loy, fy = sy ? loy : hiy;
    const float nz = sz ? hiz : loz, fz = sz ? loz : hiz;
    const float t1x = (nx - L.o.x) * L.inv.x, t2x = (fx - L.o.x) * L.inv.x;
    const float t1y = (ny - L.o.y) * L.inv.y, t2y = (fy - L.o.y) * L.inv.y;
    const float t1z = (nz - L.o.z) * L.inv.z, t2z = (fz - L.o.z) * L.inv.z;
    // "if (t1 > min) min = t1" ignores NaN exactly like fmaxf does; same for the far side
    const float tmin = fmaxf(fmaxf(fmaxf(0.001f, t1x), t1y), t1z);
    const float tmax = fminf(fminf(fminf(t_far, t2x), t2y), t2z);
    t_enter = tmin;
    return tmax > tmin;     // not (max <= min)
}

// Conservative slab test of the guarded walk (see step_inner).
__device__ __forceinline__ bool slab_fused(f3 inv, f3 noi, float lox, float loy, float loz, float hix, float hiy, float hiz,
                                            float t_far, float &t_enter) {
    const float ax = __builtin_fmaf(lox, inv.x, noi.x), bx = __builtin_fmaf(hix, inv.x, noi.x);
    const float ay = __builtin_fmaf(loy, inv.y, noi.y), by = __builtin_fmaf(hiy, inv.y, noi.y);
    const float az = __builtin_fmaf(loz, inv.z, noi.z), bz = __builtin_fmaf(hiz, inv.z, noi.z);
    const float tmin = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.001f));
    const float tmax = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), t_far));
    t_enter = tmin;
    return tmax > tmin;
}

// Lane::depth bit: this sample's result could depend on the visit order → it is re-walked exactly.
// The bit also ends the path at the next shade step (depth >= max_depth).
constexpr int32_t kFlagBit = 1 << 30;
// Lane::depth bits of the kPrim kernels (the path length proper stays below 2^22: rt_render checks max_depth):
constexpr int32_t kEndBit = 1 << 25;    // the path was ended by its last scatter; the sample is stored at the next shade step
constexpr int32_t kFreshBit = 1 << 24;  // the hit in L.hit / L.closest is a camera ray's, found AND checked against its exact leaf box by the primary pass
constexpr int32_t kArmBit = 1 << 23;    // L.o / L.d hold a camera ray that still has to be armed (a sample of a pixel without a candidate list)
constexpr int32_t kNoResumeBit = 1 << 22; // the flag was raised after the shade step had begun to draw random numbers: the exact walk restarts the sample (below)
constexpr int32_t kMaxPrimDepth = 1 << 22;
// What the primary-visibility pass leaves in the second word of a sample's record (the first is the hit distance):
// a primitive code (2 index + type) >= 0, or
constexpr int32_t kPrimMiss = -1;       // the primary ray hits nothing
constexpr int32_t kPrimFlag = -2;       // a tie between two candidates, or a hit in front of its own leaf box: the sample goes to the exact walk
constexpr int32_t kPrimWalk = -3;       // the pixel has no candidate list: the sample walks the tree from the camera
#ifndef RTP_PRIM_ROUNDS
#define RTP_PRIM_ROUNDS 1               /* kPrim shade step: at most this many store / fetch rounds (1: a wave whose lanes all drew sky samples comes
                                           straight back through the empty vote anyway; 2 and 6 measured 1.3 % slower) … */
#endif
#ifndef RTP_PRIM_REFILL
#define RTP_PRIM_REFILL 24              /* … a further one only for at least this many lanes */
#endif
#ifndef RTP_PRIM_RESHADE
#define RTP_PRIM_RESHADE 24             /* … and a further material pass only for at least this many lanes */
#endif
// Box tests of the guarded walk use closest * (1 + 2^-20): slack for the rounding of the slab
// arithmetic, so that a primitive whose computed hit lies inside the (inflated) box is never pruned.
constexpr float kGuardSlack = 1.0f + 9.5367431640625e-7f;

// One step of the guarded near-first walk: both child boxes of an SAH node, near child
// next, far child pushed.  A full stack flags the sample instead of growing.
// kTop: nodes [0, num_top) are read from `top` (the LDS treelet of a scene whose table stays in global
// memory), the others from `nodes`.
typedef float pk2 __attribute__((ext_vector_type(2)));      // one v_pk_*_f32 operand

template <bool kTop, bool kHalf, class NodeTab>
__device__ __forceinline__ void step_inner(Lane &L, NodeTab nodes, const float4 *top, int32_t num_top, uint32_t *stack, int32_t levels) {
    float e0, e1;
    const float t_far = L.closest * kGuardSlack;
    // These boxes are this library's own (inflated) ones, so the test only has to be conservative,
    // not the reference's arithmetic: t = plane * (1/d) - o * (1/d) as one fused multiply-add per
    // plane, near/far by min/max.  Its rounding (about an ulp of the coordinates) is part of the
    // margin budget (rt_accel.cpp, kGuardGamma and the floor on the inflation).
    // 1/d is +-inf for a ray parallel to an axis; inf - inf would poison the fused form, so the walk uses a
    // finite stand-in (any |1/d| >= 1e18 puts the planes of that axis "infinitely" far away just as well)
    const f3 inv = mk(__builtin_amdgcn_fmed3f(L.inv.x, -1e18f, 1e18f), __builtin_amdgcn_fmed3f(L.inv.y, -1e18f, 1e18f),
                      __builtin_amdgcn_fmed3f(L.inv.z, -1e18f, 1e18f));
    const f3 noi = mk(-(L.o.x * inv.x), -(L.o.y * inv.y), -(L.o.z * inv.z));
    bool h0, h1;
    int32_t c0, c1;
    if (kHalf) {
        // 32-byte node (tables read through L1/L2: half the traffic): 12 binary16 box planes, rounded outward
        // by the packer, + two child codes; (float)half feeds the multiply-add directly (v_fma_mix_f32)
        float4 A, B;
        if (kTop && L.node < num_top) {
            A = top[2 * L.node + 0];
            B = top[2 * L.node + 1];
        } else {
            A = nodes[2 * L.node + 0];
            B = nodes[2 * L.node + 1];
        }
        typedef _Float16 half8 __attribute__((ext_vector_type(8)));
        typedef _Float16 half4 __attribute__((ext_vector_type(4)));
        const half8 ha = __builtin_bit_cast(half8, A);                       // lo0.x hi0.x lo0.y hi0.y lo0.z hi0.z lo1.x hi1.x
        const half4 hb = __builtin_bit_cast(half4, make_float2(B.x, B.y));   // lo1.y hi1.y lo1.z hi1.z
        float b0[6] = {(float)ha[0], (float)ha[2], (float)ha[4], (float)ha[1], (float)ha[3], (float)ha[5]};
        float b1[6] = {(float)ha[6], (float)hb[0], (float)hb[2], (float)ha[7], (float)hb[1], (float)hb[3]};
        h0 = slab_fused(inv, noi, b0[0], b0[1], b0[2], b0[3], b0[4], b0[5], t_far, e0);
        h1 = slab_fused(inv, noi, b1[0], b1[1], b1[2], b1[3], b1[4], b1[5], t_far, e1);
        c0 = as_int(B.z);
        c1 = as_int(B.w);
    } else {
        // 64-byte node (LDS-resident tables): fp32 planes — outward rounding to binary16 would grow the small
        // boxes of S-rtiow by as much as their inflation and cost 2 %.  (Tried: the LDS copy stored axis by axis so that
        // one v_pk_fma_f32 makes the plane distances of both children — 6 instead of 12 multiply-adds, 3.5 % SLOWER.)
        const float4 A = nodes[4 * L.node + 0];
        const float4 B = nodes[4 * L.node + 1];
        const float4 C = nodes[4 * L.node + 2];
        const float4 D = nodes[4 * L.node + 3];
        float b0[6] = {A.x, A.y, A.z, A.w, B.x, B.y};
        float b1[6] = {B.z, B.w, C.x, C.y, C.z, C.w};
        h0 = slab_fused(inv, noi, b0[0], b0[1], b0[2], b0[3], b0[4], b0[5], t_far, e0);
        h1 = slab_fused(inv, noi, b1[0], b1[1], b1[2], b1[3], b1[4], b1[5], t_far, e1);
        c0 = as_int(D.x);
        c1 = as_int(D.y);
    }
    const bool second_first = h1 && (!h0 || e1 < e0);
    const int32_t near_c = second_first ? c1 : c0;
    const int32_t far_c = second_first ? c0 : c1;
    if (h0 && h1) {
        if (L.sp < levels) {
            stack[L.sp * kWave] = (uint32_t)far_c;
            L.sp++;
        } else {
            L.depth |= kFlagBit | RTP_WHY(0);
        }
    }
    if (h0 || h1) L.node = near_c;
    else pop(L, stack);
}

// The pair step of scenes with distance-aware margins (rt_accel.cpp, Packed::Guard::dyn_k: the leaves carry only the rounding
// floor and the walk grows every box it tests) — binary16 records read through L1 / L2:
//   * every dword of a record is the (lo, hi) pair of one axis of one child.  Rotating it by 16 bits where 1/d is negative
//     on that axis puts the plane the ray meets FIRST into the low half: near and far are picked by one full-rate
//     v_alignbit per dword instead of a min and a max per pair of plane distances (half rate), and the binary16 values feed
//     the multiply-adds directly;
//   * the growth is applied in ray parameter space: t_near - e |1/d|, t_far + e |1/d| (rounds 2-3 grew the planes themselves,
//     nineteen instructions per child, then took e from the farthest corner of the union of the two children, twenty-eight per
//     step: docs/LOG.md).
// No child slot of these tables is empty: every inner node of the SAH tree and of the device-built tree has two children (the
// packer checks its own: rt_accel.cpp, pair_tables).
constexpr float kDynSlack = 1.0009765625f;       // relative slack on the growth (host: rt_capi.hip fill_params folds it into the kernel's constants)
// The growth in PARAMETRIC form (round 4).
// What the growth of a box has to cover is k x^2 for every small sphere q below it whose test can still matter — one with an
// accepted computed hit at a parameter t_c <= closest — x = |o - c_q|, k = dyn_k.  The farthest corner of the box bounds x; so
// does the RAY: the computed hit point P = o + t_c d lies inside q's leaf box [c -/+ r] grown by eps_q = k x^2 (docs/LOG.md
// §3b), so x <= |o - P| + |P - c_q| <= t_c |d| + sqrt(3) (r_q + eps_q).  Induction down the tree: let e bound k x^2 for every
// such q below node M (the root: the corner bound, once per ray).  M's children are tested grown by e, which holds P for every
// q below them: t_c lies inside the child's grown, clipped slab interval, t_c <= T = its exit parameter (<= t_far), and so
//     x <= T |d| + sqrt(3) (r_max + e)      →      E(T, e) = k (T |d| + sqrt(3) r_max + sqrt(3) e)^2
// bounds k x^2 for every such q below THAT child: the growth its own children are tested with (never more than e itself: e
// holds for them too).  A node that comes off the stack gets the ray's own bound, er — the corner bound of the whole tree,
// lowered to E(closest, er) whenever a hit is found — which holds for every node.
// Cost: the growth is known BEFORE the planes are read, so it goes into the addends of the twelve multiply-adds (-o/d -/+ e |1/d|:
// three multiplications, six additions) and the step ends with one multiply-add, one fma and a square for the child it
// descends into — 13 vector instructions where the corner of the union of the two boxes took 28 (tools/nearfirst_study.c
// MODEL=1 GROW=4: S-100k 18.85 pair steps per ray against 19.22 with the corner rule — the bound is tighter for the big boxes
// at the top of the tree, looser by one step after a pop).
// Per ray (arm_ray): ea = sqrt(k) |d| (rounded up) and er live in two rows of the lane's LDS stack, L.e in a register.
// Rounding: the relative 2^-10 of kDynSlack is in sqrt_k and b (host, rt_capi.hip fill_params); the plane distances round as
// as ever (docs/LOG.md §3b, floor of the margins).
struct DynPar { float b, c3; int32_t er_row, ea_row; };      // sqrt(k) sqrt(3) r_max; sqrt(k) sqrt(3); byte offsets of the two rows in the lane's stack column
__device__ __forceinline__ float par_growth(float T, float ea, float e, const DynPar &dp) {
    const float s = __builtin_fmaf(e, dp.c3, __builtin_fmaf(T, ea, dp.b));
    return s * s;
}
template <class NodeTab>
__device__ __forceinline__ void step_pair_par(Lane &L, NodeTab nodes, uint32_t *stack, int32_t levels, const DynPar &dp) {
    const float t_far = L.closest * kGuardSlack;
    const f3 inv = mk(__builtin_amdgcn_fmed3f(L.inv.x, -1e18f, 1e18f), __builtin_amdgcn_fmed3f(L.inv.y, -1e18f, 1e18f),
                      __builtin_amdgcn_fmed3f(L.inv.z, -1e18f, 1e18f));
    const f3 noi = mk(-(L.o.x * inv.x), -(L.o.y * inv.y), -(L.o.z * inv.z));
    // the growth, in ray parameter space, goes into the addends: near planes get -o/d - e |1/d|, far planes -o/d + e |1/d|
    const float gx = L.e * fabsf(inv.x), gy = L.e * fabsf(inv.y), gz = L.e * fabsf(inv.z);
    const f3 an = mk(noi.x - gx, noi.y - gy, noi.z - gz), af = mk(noi.x + gx, noi.y + gy, noi.z + gz);
    // (every record through L1 / L2: an LDS treelet for the top of the tree cost eight vector instructions a step in choosing
    // between two address spaces and bought nothing L1 does not give — configs[4] 3 715 against 3 655 Msamples/s)
    const float4 A = nodes[2 * L.node + 0], B = nodes[2 * L.node + 1];
    typedef __attribute__((address_space(3))) const float lds_cf;
    const uint32_t col = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)stack;
    const float er = *(lds_cf *)(uintptr_t)(col + (uint32_t)dp.er_row), ea = *(lds_cf *)(uintptr_t)(col + (uint32_t)dp.ea_row);
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const uint32_t rx = (__float_as_uint(inv.x) >> 27) & 16u, ry = (__float_as_uint(inv.y) >> 27) & 16u, rz = (__float_as_uint(inv.z) >> 27) & 16u;
    auto planes = [](float w, uint32_t r) { const uint32_t u = __float_as_uint(w); return __builtin_bit_cast(half2v, __builtin_amdgcn_alignbit(u, u, r)); };
    const half2v x0 = planes(A.x, rx), y0 = planes(A.y, ry), z0 = planes(A.z, rz), x1 = planes(A.w, rx), y1 = planes(B.x, ry), z1 = planes(B.y, rz);
    const float n0x = __builtin_fmaf((float)x0[0], inv.x, an.x), f0x = __builtin_fmaf((float)x0[1], inv.x, af.x);
    const float n1x = __builtin_fmaf((float)x1[0], inv.x, an.x), f1x = __builtin_fmaf((float)x1[1], inv.x, af.x);
    const float n0y = __builtin_fmaf((float)y0[0], inv.y, an.y), f0y = __builtin_fmaf((float)y0[1], inv.y, af.y);
    const float n1y = __builtin_fmaf((float)y1[0], inv.y, an.y), f1y = __builtin_fmaf((float)y1[1], inv.y, af.y);
    const float n0z = __builtin_fmaf((float)z0[0], inv.z, an.z), f0z = __builtin_fmaf((float)z0[1], inv.z, af.z);
    const float n1z = __builtin_fmaf((float)z1[0], inv.z, an.z), f1z = __builtin_fmaf((float)z1[1], inv.z, af.z);
    const float e0 = fmaxf(fmaxf(n0x, n0y), fmaxf(n0z, 0.001f)), q0 = fminf(fminf(f0x, f0y), fminf(f0z, t_far));
    const float e1 = fmaxf(fmaxf(n1x, n1y), fmaxf(n1z, 0.001f)), q1 = fminf(fminf(f1x, f1y), fminf(f1z, t_far));
    const int32_t c0 = as_int(B.z), c1 = as_int(B.w);
    const bool h0 = q0 > e0, h1 = q1 > e1;           // (no empty child slots in these tables: above)
    const bool second_first = h1 & !(h0 & (e0 <= e1));
    const int32_t near_c = second_first ? c1 : c0;
    const int32_t far_c = second_first ? c0 : c1;
    const float near_q = second_first ? q1 : q0;
    if (h0 && h1) {          // (as step_octant: a full stack without a branch)
        const int32_t top_at = levels * kLevelBytes - kLevelBytes;
        const int32_t room = top_at - L.sp;
        L.depth |= (int32_t)(((uint32_t)room >> 1) & (uint32_t)kFlagBit) | (room < 0 ? RTP_WHY(0) : 0);
        const int32_t at = L.sp < top_at ? L.sp : top_at;
        *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(stack) + at) = (uint32_t)far_c;
        L.sp = at + kLevelBytes;
    }
    if (h0 || h1) {
        L.node = near_c;
        L.e = fminf(L.e, par_growth(near_q, ea, L.e, dp));
    } else {
        pop<true>(L, stack);
        L.e = er;
    }
}

// step_pair_par on the 4-WIDE form of the tree (rt_accel.cpp: the SAH tree collapsed; 64-byte records — per axis the four
// children's (lo, hi) binary16 pairs, then the four child codes): half as many dependent record loads per ray, and — now that the
// growth is three multiplications and six additions a NODE, not nineteen instructions a child — fewer vector instructions per
// ray as well (round 3's step_wide, which grew every child box from its own farthest corner, lost 34 % on S-100k).  The nearest
// hit child is entered (lowest slot among equals), the other hit children wait on the stack, slot 3 first; growth as in
// step_pair_par: every child tested with the node's e, the entered child's own from its exit parameter, a node off the stack gets
// the ray's bound.  Empty child slots hold the finite inverted box (65504, -65504) the packer's directed rounding makes of the
// "never hit" box: exit < entry for any ray and any growth below 65504.
// Stack: entries beyond the top go over the top one and flag the sample (checked once per step, not per entry).
template <class NodeTab>
__device__ __forceinline__ void step_wide_par(Lane &L, NodeTab nodes, uint32_t *stack, int32_t levels, const DynPar &dp) {
    const float t_far = L.closest * kGuardSlack;
    const f3 inv = L.inv;         // (clamped to +-1e18 by begin_ray<true>: this walk's lanes hold no other copy)
    const f3 noi = mk(-(L.o.x * inv.x), -(L.o.y * inv.y), -(L.o.z * inv.z));
    const float gx = L.e * fabsf(inv.x), gy = L.e * fabsf(inv.y), gz = L.e * fabsf(inv.z);
    const f3 an = mk(noi.x - gx, noi.y - gy, noi.z - gz), af = mk(noi.x + gx, noi.y + gy, noi.z + gz);
    const float4 X = nodes[4 * L.node + 0], Y = nodes[4 * L.node + 1], Z = nodes[4 * L.node + 2], C = nodes[4 * L.node + 3];
    typedef __attribute__((address_space(3))) const float lds_cf;
    const uint32_t col = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)stack;
    const float er = *(lds_cf *)(uintptr_t)(col + (uint32_t)dp.er_row), ea = *(lds_cf *)(uintptr_t)(col + (uint32_t)dp.ea_row);
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const uint32_t rx = (__float_as_uint(inv.x) >> 27) & 16u, ry = (__float_as_uint(inv.y) >> 27) & 16u, rz = (__float_as_uint(inv.z) >> 27) & 16u;
    auto planes = [](float w, uint32_t r) { const uint32_t u = __float_as_uint(w); return __builtin_bit_cast(half2v, __builtin_amdgcn_alignbit(u, u, r)); };
    const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
    const int32_t code[4] = {as_int(C.x), as_int(C.y), as_int(C.z), as_int(C.w)};
    float key[4], q[4];
    bool h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const half2v px = planes(xs[k], rx), py = planes(ys[k], ry), pz = planes(zs[k], rz);
        const float nx = __builtin_fmaf((float)px[0], inv.x, an.x), fx = __builtin_fmaf((float)px[1], inv.x, af.x);
        const float ny = __builtin_fmaf((float)py[0], inv.y, an.y), fy = __builtin_fmaf((float)py[1], inv.y, af.y);
        const float nz = __builtin_fmaf((float)pz[0], inv.z, an.z), fz = __builtin_fmaf((float)pz[1], inv.z, af.z);
        const float e = fmaxf(fmaxf(nx, ny), fmaxf(nz, 0.001f));
        q[k] = fminf(fminf(fx, fy), fminf(fz, t_far));
        h[k] = q[k] > e;
        key[k] = h[k] ? e : 3.0e38f;
    }
    const float m = fminf(fminf(key[0], key[1]), fminf(key[2], key[3]));
    const bool any = m < 3.0e38f;
    const bool s0 = key[0] == m, s1 = !s0 & (key[1] == m), s2 = !(s0 | s1) & (key[2] == m);
    const int32_t near_c = s0 ? code[0] : (s1 ? code[1] : (s2 ? code[2] : code[3]));
    const float near_q = s0 ? q[0] : (s1 ? q[1] : (s2 ? q[2] : q[3]));
    const bool s3 = !(s0 | s1 | s2);
    const bool push[4] = {h[0] && !s0, h[1] && !s1, h[2] && !s2, h[3] && !s3};
    const int32_t top_at = levels * kLevelBytes - kLevelBytes;
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (push[k]) {
            const int32_t at = L.sp < top_at ? L.sp : top_at;
            *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(stack) + at) = (uint32_t)code[k];
            L.sp += kLevelBytes;
        }
    {       // an entry (or three) too many: over the top one they went, the sample goes to the exact walk
        const int32_t room = top_at + kLevelBytes - L.sp;
        L.depth |= (int32_t)(((uint32_t)room >> 1) & (uint32_t)kFlagBit) | (room < 0 ? RTP_WHY(0) : 0);
        L.sp = L.sp < top_at + kLevelBytes ? L.sp : top_at + kLevelBytes;
    }
    if (any) {
        L.node = near_c;
        L.e = fminf(L.e, par_growth(near_q, ea, L.e, dp));
    } else {
        pop<true>(L, stack);
        L.e = er;
    }
}

// step_inner for the LDS-resident pair table in the OCTANT layout (render_kernel stages it from the 64-byte records).
// 80 bytes per node: per axis six floats lo0 lo1 hi0 hi1 lo0 lo1 (children 0 and 1), then the two child codes.  The 16
// bytes at (axis base + 8 * s), s = sign bit of 1/d on that axis, are (near0 near1 far0 far1): which plane of a slab the
// ray meets first is picked by the ADDRESS of one ds_read2_b64, not by min/max of the two plane distances — on gfx950
// v_min/v_max/v_cmp/v_cndmask issue at half the rate of v_fma/v_add/v_mul (tools/micro/valu_rates.hip), and the slab
// test of step_inner spends 12 of them per step on exactly that.  fma is monotonic, so near = min and far = max of the
// two distances bit for bit: the walk is the same walk.  L.node is the node's BYTE offset in the table here (the links
// are staged pre-multiplied), so no address arithmetic beyond the three octant offsets remains.
constexpr int kOctNodeBytes = 80;
typedef float oct4 __attribute__((ext_vector_type(4), aligned(8)));
__device__ __forceinline__ void step_octant(Lane &L, uint32_t *stack, int32_t levels) {
    const float t_far = L.closest * kGuardSlack;
    const f3 inv = mk(__builtin_amdgcn_fmed3f(L.inv.x, -1e18f, 1e18f), __builtin_amdgcn_fmed3f(L.inv.y, -1e18f, 1e18f),
                      __builtin_amdgcn_fmed3f(L.inv.z, -1e18f, 1e18f));
    const f3 noi = mk(-(L.o.x * inv.x), -(L.o.y * inv.y), -(L.o.z * inv.z));
    // L.node IS the record's LDS address (the staged links are addresses): three adds make the octant's three read
    // addresses, the codes sit at a constant offset
    typedef __attribute__((address_space(3))) const oct4 lds_oct4;
    typedef int int2v __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const int2v lds_int2;
    const uint32_t rec = (uint32_t)L.node;
    const uint32_t kx = (__float_as_uint(inv.x) >> 28) & 8u, ky = (__float_as_uint(inv.y) >> 28) & 8u, kz = (__float_as_uint(inv.z) >> 28) & 8u;
    const oct4 X = *(lds_oct4 *)(uintptr_t)(rec + kx);                   // near0 near1 far0 far1
    const oct4 Y = *(lds_oct4 *)(uintptr_t)(rec + (24u + ky));
    const oct4 Z = *(lds_oct4 *)(uintptr_t)(rec + (48u + kz));
    const int2v codes = *(lds_int2 *)(uintptr_t)(rec + 72u);
    const float n0x = __builtin_fmaf(X.x, inv.x, noi.x), n1x = __builtin_fmaf(X.y, inv.x, noi.x);
    const float f0x = __builtin_fmaf(X.z, inv.x, noi.x), f1x = __builtin_fmaf(X.w, inv.x, noi.x);
    const float n0y = __builtin_fmaf(Y.x, inv.y, noi.y), n1y = __builtin_fmaf(Y.y, inv.y, noi.y);
    const float f0y = __builtin_fmaf(Y.z, inv.y, noi.y), f1y = __builtin_fmaf(Y.w, inv.y, noi.y);
    const float n0z = __builtin_fmaf(Z.x, inv.z, noi.z), n1z = __builtin_fmaf(Z.y, inv.z, noi.z);
    const float f0z = __builtin_fmaf(Z.z, inv.z, noi.z), f1z = __builtin_fmaf(Z.w, inv.z, noi.z);
    const float e0 = fmaxf(fmaxf(n0x, n0y), fmaxf(n0z, 0.001f)), x0 = fminf(fminf(f0x, f0y), fminf(f0z, t_far));
    const float e1 = fmaxf(fmaxf(n1x, n1y), fmaxf(n1z, 0.001f)), x1 = fminf(fminf(f1x, f1y), fminf(f1z, t_far));
    const bool h0 = x0 > e0, h1 = x1 > e1;
    const int32_t c0 = codes.x, c1 = codes.y;
    // (bitwise on purpose: `h1 && (…)` makes the compiler open an exec-mask region just to skip one v_cmp — five scalar
    // instructions, and the scalar pipe is the busiest one in this loop)
    const bool second_first = h1 & !(h0 & (e0 <= e1));
    const int32_t near_c = second_first ? c1 : c0;
    const int32_t far_c = second_first ? c0 : c1;
    if (h0 && h1) {
        // A full stack without a branch: the entry goes over the top one (a child code like any other, so the walk stays a
        // walk of valid nodes and ends) and the sample is flagged for the exact walk, by arithmetic: room < 0 iff the stack is full.
        const int32_t top = levels * kLevelBytes - kLevelBytes;
        const int32_t room = top - L.sp;
        L.depth |= (int32_t)(((uint32_t)room >> 1) & (uint32_t)kFlagBit) | (room < 0 ? RTP_WHY(0) : 0);
        const int32_t at = L.sp < top ? L.sp : top;
        *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(stack) + at) = (uint32_t)far_c;
        L.sp = at + kLevelBytes;
    }
    if (h0 || h1) L.node = near_c;
    else pop<true>(L, stack);
}

// Root selection of hit_sphere (include/sphere.h:35-45): root = (-half_b - sqrtD) / a in double; if its float value is not in
// [0.001, closest], (-half_b + sqrtD) / a; returns whether a root was accepted and which.  nb = -half_b, sq = sqrtf(D), da = a.
// sphere_root_plain is the reference's form with the compiler's division (kept for rt_debug_check_sphere_roots and as the
// host-side meaning of sphere_root); a quotient has the sign of its numerator (a > 0), so a root whose numerator is <= 0
// fails 0.001 <= root without dividing, and when the near root is beyond `closest` the far one, larger still, is too.
__device__ __forceinline__ bool sphere_root_plain(double nb, double sq, double da, float closest, float &t) {
    bool ok = false, second = true;
    t = 0.0f;
    const double num1 = nb - sq;
    if (num1 > 0.0) {
        t = (float)(num1 / da);
        ok = (0.001f <= t) && (t <= closest);
        second = t < 0.001f;
    }
    if (!ok && second) {
        const double num2 = nb + sq;
        if (num2 > 0.0) {
            t = (float)(num2 / da);
            ok = (0.001f <= t) && (t <= closest);
        }
    }
    return ok;
}
__device__ __forceinline__ double sphere_root_rcp(double da);
template <bool kLazyFar = false>
__device__ __forceinline__ bool sphere_root_with(double nb, double sq, double da, double y, float closest, float &t);
__device__ __forceinline__ bool sphere_root(double nb, double sq, double da, float closest, float &t) {
#ifdef __HIP_DEVICE_COMPILE__
    // Both roots from ONE reciprocal.  The compiler's correctly rounded n / d is: v_div_scale (n, d), y = v_rcp_f64(d), two
    // Newton steps on y, q0 = n*y, r = fma(-d, q0, n), q = v_div_fmas(r, y, q0), v_div_fixup.  With operands that began as
    // binary32 (|exponent| <= 149 of the 1022 a double has) the scaling never engages — v_div_scale returns its operand,
    // v_div_fmas is a plain fma — so the same instructions WITHOUT the three scale/fix-up ones give the same bits for every
    // finite quotient, and the reciprocal with its Newton steps (v_rcp_f64 alone is 16 cycles of SIMD time, the four fma 19) is
    // shared by the two numerators.  Where the operands are not finite or d is 0 the sequences differ only in WHICH of
    // inf / NaN / 0 comes out, and all of those fail 0.001 <= t <= closest alike; an accepted t is finite, positive and
    // normal, i.e. the common case.  (rt_debug_check_sphere_roots runs 2^32 operand sets through both forms.)
    // A wave runs both divisions of the plain form whenever ANY lane needs them — with 30 lanes in a leaf step that is
    // always — so skipping roots that cannot matter saved little and cost a nest of exec-mask regions; this form has none.
    const double y = sphere_root_rcp(da);
    return sphere_root_with(nb, sq, da, y, closest, t);
#else
    return sphere_root_plain(nb, sq, da, closest, t);
#endif
}
#ifdef __HIP_DEVICE_COMPILE__
// (the two halves of sphere_root: the reciprocal of a = |d|^2 belongs to the RAY — a caller that tests several spheres
// against one ray, the primary-visibility pass, makes it once)
__device__ __forceinline__ double sphere_root_rcp(double da) {
    const double y0 = __builtin_amdgcn_rcp(da);
    const double y1 = __builtin_fma(y0, __builtin_fma(-da, y0, 1.0), y0);
    return __builtin_fma(y1, __builtin_fma(-da, y1, 1.0), y1);
}
// kLazyFar (the primary-visibility pass: rays that start outside nearly every sphere): the far root is made only if some
// lane's near root lies below the interval.  Where the near root is above it the far root is too — both are the correctly
// rounded quotients of n1 <= n2 by the same a > 0, rounded to float: monotone — so leaving it out changes nothing.
template <bool kLazyFar>
__device__ __forceinline__ bool sphere_root_with(double nb, double sq, double da, double y, float closest, float &t) {
    const double n1 = nb - sq;
    const double p1 = n1 * y;
    const float t1 = (float)__builtin_fma(__builtin_fma(-da, p1, n1), y, p1);
    const bool ok1 = (0.001f <= t1) & (t1 <= closest);
    float t2 = t1;
    bool ok2 = false;
    if (!kLazyFar || __any(!(t1 >= 0.001f))) {
        const double n2 = nb + sq;
        const double p2 = n2 * y;
        t2 = (float)__builtin_fma(__builtin_fma(-da, p2, n2), y, p2);
        ok2 = (0.001f <= t2) & (t2 <= closest);
    }
    t = ok1 ? t1 : t2;                  // the far root only if the near one is not in the interval
    return ok1 | ok2;
}
#else
__device__ __forceinline__ double sphere_root_rcp(double da) { return 1.0 / da; }
template <bool kLazyFar>
__device__ __forceinline__ bool sphere_root_with(double nb, double sq, double da, double, float closest, float &t) { return sphere_root_plain(nb, sq, da, closest, t); }
#endif

// hit_sphere (include/sphere.h:24-53), root selection only; the hit record is rebuilt at shading.
template <bool kGuard = false>
__device__ __forceinline__ void test_sphere(Lane &L, float4 s, int32_t prim) {
    const f3 oc = sub(L.o, mk(s.x, s.y, s.z));
    const float a = lensq(L.d);
    const float half_b = dot(oc, L.d);
    const float c = lensq(oc) - s.w * s.w;
    const float disc = half_b * half_b - a * c;
    if (disc < 0) return;
    const double sq = (double)sqrt_cr(disc);
    const double nb = (double)(-half_b);
    const double da = (double)a;
    float t;
    const bool ok = sphere_root(nb, sq, da, L.closest, t);
    if (ok) {
        // contains() accepts root == closest (include/interval.h), so on an exact tie the reference
        // keeps whichever primitive it visits LAST: order dependent → exact walk
        if (kGuard && t == L.closest && L.hit >= 0) L.depth |= kFlagBit | RTP_WHY(1);
        L.closest = t;
        L.hit = prim;
    }
}

// (Tried in round 4 for the front primitives — the ground sphere every ray tests as it is armed, and last in every pixel's candidate
// list: leaving out both fp64 roots where float estimates, with a margin of 2^-20, say that no root can be accepted — numerators
// <= 0, larger root below 0.001, smaller positive root beyond `closest` (the ground sphere under a floor quad).  Bit-identical,
// and slower: headline trace 78.5 -> 79.4 ms, primary pass 5.6 -> 6.0 ms, configs[4] unchanged.  The roots run for the whole
// wave whenever ONE lane needs them, which is nearly always, and the estimates are eight more instructions: docs/LOG.md round 4.)
// The same test with the ray's own constants — a = |d|^2, (double)a and its reciprocal (sphere_root_rcp) — made by the caller.
template <bool kGuard = false, bool kLazyFar = false>
__device__ __forceinline__ void test_sphere_ray(Lane &L, float4 s, int32_t prim, float a, double da, double y) {
    const f3 oc = sub(L.o, mk(s.x, s.y, s.z));
    const float half_b = dot(oc, L.d);
    const float c = lensq(oc) - s.w * s.w;
    const float disc = half_b * half_b - a * c;
    if (disc < 0) return;
    const double sq = (double)sqrt_cr(disc);
    const double nb = (double)(-half_b);
    float t;
    if (sphere_root_with<kLazyFar>(nb, sq, da, y, L.closest, t)) {
        if (kGuard && t == L.closest && L.hit >= 0) L.depth |= kFlagBit | RTP_WHY(1);      // exact tie: see test_sphere
        L.closest = t;
        L.hit = prim;
    }
}
// the constants of a ray that every sphere test needs: a = |d|^2, (double)a, 1 / (double)a — test_sphere's own expressions, so
// test_sphere_ray<kGuard, false> with them gives test_sphere<kGuard>'s bits.  The primary pass makes them once per sample, the trace
// kernel of a scene without emitters (the headline kernel, RTP_BODY_CARRY) once per armed ray: there the lane keeps them.
struct RayConst { float a; double da, y; };
__device__ __forceinline__ RayConst ray_const(const Lane &L) {
    RayConst r;
    r.a = lensq(L.d);
    r.da = (double)r.a;
    r.y = sphere_root_rcp(r.da);
    return r;
}

// hit_plane + is_interior_* (include/plane.h:30-96), acceptance only.
template <bool kGuard = false, class PlaneTab>
__device__ __forceinline__ void test_plane(Lane &L, PlaneTab planes, int32_t idx, int32_t prim) {
    const float4 P0 = planes[5 * idx + 0];
    const f3 n = mk(P0.x, P0.y, P0.z);
    const float denom = dot(n, L.d);
    if ((double)fabsf(denom) < 1e-8) return;
    const float t = (P0.w - dot(n, L.o)) / denom;     // double quotient narrowed == float quotient
    if (!((0.001f <= t) && (t <= L.closest))) return;
    const float4 P1 = planes[5 * idx + 1];
    const float4 P2 = planes[5 * idx + 2];
    const float4 P3 = planes[5 * idx + 3];
    const float4 P4 = planes[5 * idx + 4];
    const f3 ph = sub(add(L.o, scale(t, L.d)), mk(P4.x, P4.y, P4.z));
    const f3 w = mk(P1.x, P1.y, P1.z);
    const float alpha = dot(w, cross(ph, mk(P3.x, P3.y, P3.z)));
    const float beta = dot(w, cross(mk(P2.x, P2.y, P2.z), ph));
    const int32_t type = as_int(P1.w);
    bool inside = true;
    if (type == RT_PLANE_QUAD) {
        inside = (0.0f <= alpha) && (alpha <= 1.0f) && (0.0f <= beta) && (beta <= 1.0f);
    } else if (type == RT_PLANE_ELLIPSE) {
        const float ea = alpha - 0.5f, eb = beta - 0.5f;     // powf(x, 2) == x*x
        inside = !(ea * ea + eb * eb > 0.25f);
    } else if (type == RT_PLANE_TRIANGLE) {
        const double da = alpha, db = beta;
        inside = !(da < 0 || db < 0 || (da + db) > 1);
    }
    if (inside) {
        if (kGuard && t == L.closest && L.hit >= 0) L.depth |= kFlagBit | RTP_WHY(1);     // exact tie: see test_sphere
        L.closest = t;
        L.hit = prim;
    }
}

template <class SphereTab, class PlaneTab>
__device__ __forceinline__ void step_leaf(Lane &L, SphereTab spheres, PlaneTab planes, const uint32_t *stack) {
    const int32_t code = -(L.node + 1);
    const int32_t idx = code >> 1;
    if (code & 1) test_plane<true>(L, planes, idx, code);
    else test_sphere<true>(L, spheres[idx], code);
    pop(L, stack);
}

// ---- parked primitive tests (guarded walk of render_kernel) -------------------------------------------------------
// A lane that reaches a leaf does not stop for the primitive test: it parks the leaf code in L.pend and walks on with the
// next node from its stack; the wave's next LEAF step tests every parked primitive, of lanes that are stuck (a second
// leaf reached, or nothing left to walk) and of lanes that are still walking alike.  Lanes that used to idle through the
// wave's pair steps until enough others wanted a leaf step now take part in them.  The later pruning costs 4 % more box
// and primitive tests (tools/nearfirst_study.c DEFER=4: 11.25 / 1.94 instead of 10.79 / 1.86 per ray on S-rtiow); the
// result is that of the walk without parking — the guarded walk's argument does not depend on the order of its tests.
// (Tried in round 4 for the scenes read through L1 / L2: the lane that parks a sphere leaf sends for the sphere's record with a
// global_load_lds — gfx950's load straight into LDS, no register — into a 16-byte slot of a 1 KB buffer of its wave, so that the
// leaf step opens with a ds_read instead of a round trip through L2.  BASELINE configs[4]: 3 105 against 3 172 Msamples/s without
// it — the 12 KB of buffers come out of the LDS treelet and the addressing cost seven spilled registers; docs/LOG.md, round 4.)
template <bool kSent = false>
__device__ __forceinline__ bool park_leaf(Lane &L, const uint32_t *stack) {      // (true: a node came off the stack)
    if (L.node < 0 && L.node != kDone && L.pend == 0) {
        L.pend = L.node;
        pop<kSent>(L, stack);
        return true;
    }
    return false;
}

// kPark = false: the test alone (the caller parks: step_pair_par's kernels have the lane's growth to look after)
template <bool kSent = false, bool kSimple = false, bool kPark = true, class SphereTab, class PlaneTab>
__device__ __forceinline__ void step_leaf_parked(Lane &L, SphereTab spheres, PlaneTab planes, const uint32_t *stack) {
    const int32_t code = -(L.pend + 1);
    const int32_t idx = code >> 1;
    if (!kSimple && (code & 1)) test_plane<true>(L, planes, idx, code);
    else test_sphere<true>(L, spheres[idx], code);
    L.pend = 0;
    if (kPark) park_leaf<kSent>(L, stack);          // a lane that was stuck at a second leaf parks that one and walks on
}
// … of a sphere-only scene, with the ray's constants the lane carries (RTP_BODY_CARRY: arm_ray made them, ray_const)
template <bool kSent, class SphereTab>
__device__ __forceinline__ void step_leaf_parked_ray(Lane &L, SphereTab spheres, const uint32_t *stack, float ray_a, double ray_y) {
    const int32_t code = -(L.pend + 1);
    test_sphere_ray<true, false>(L, spheres[code >> 1], code, ray_a, (double)ray_a, ray_y);
    L.pend = 0;
    park_leaf<kSent>(L, stack);
}

// ---- threaded (reference-order) traversal --------------------------------------------------------
// Exactly hit_bvh's sequence of box and primitive tests (include/bvh.h:28-63): the caller's nodes
// in the order hit_bvh pops them, a hit box continues with the next node, a missed one jumps over
// its subtree.  No stack and no ordering decision: the running `closest` at every test is the
// reference's, so even the tests that are sensitive to it (a primitive whose computed hit lies a
// few ulps in front of its own leaf box) come out the same.
constexpr int32_t kBlocked = INT32_MIN;                        // sign bit of Lane::node in threaded mode

// One node of the threaded table: A = (lo.x, hi.x, lo.y, hi.y), B = (lo.z, hi.z, skip, prim + 1).
// Same arithmetic as slab(): t = (plane - origin) * (1 / dir) per plane, the pair of one axis in
// one packed instruction, near/far picked by the sign of 1/dir AFTER the multiply (the same two
// products either way), then max/min folds that ignore NaN like the reference's comparisons.
template <class NodeTab>
__device__ __forceinline__ void step_threaded(Lane &L, NodeTab tnodes, int32_t num_tnodes) {
    const float4 A = tnodes[2 * L.node + 0];
    float4 B = tnodes[2 * L.node + 1];
    // keep skip/prim in the one 16-byte read (otherwise hipcc sinks two dword reads into a
    // divergent branch on the box result and each step pays a second LDS round trip)
    asm volatile("" : "+v"(B.z), "+v"(B.w));
    const pk2 tx = (pk2{A.x, A.y} - pk2{L.o.x, L.o.x}) * pk2{L.inv.x, L.inv.x};
    const pk2 ty = (pk2{A.z, A.w} - pk2{L.o.y, L.o.y}) * pk2{L.inv.y, L.inv.y};
    const pk2 tz = (pk2{B.x, B.y} - pk2{L.o.z, L.o.z}) * pk2{L.inv.z, L.inv.z};
    const bool sx = L.inv.x < 0, sy = L.inv.y < 0, sz = L.inv.z < 0;
    const float nx = sx ? tx.y : tx.x, fx = sx ? tx.x : tx.y;
    const float ny = sy ? ty.y : ty.x, fy = sy ? ty.x : ty.y;
    const float nz = sz ? tz.y : tz.x, fz = sz ? tz.x : tz.y;
    const float tmin = fmaxf(fmaxf(fmaxf(nx, ny), nz), 0.001f);
    const float tmax = fminf(fminf(fminf(fx, fy), fz), L.closest);
    const bool h = tmax > tmin;
    // Link encoding (rt_accel.cpp): the sign bit of `node` means "no box test wanted": set while a
    // primitive test is pending (leaf records carry it in B.w) and on the link that ends the walk.
    const int32_t leaf = as_int(B.w);            // 0 for inner nodes, (2*index+type+1) | sign for leaves
    L.sp = h ? leaf : 0;
    L.node = h ? ((L.node + 1) | (leaf & kBlocked)) : as_int(B.z);
}

// step_threaded on the OCTANT layout of the LDS copy (the sphere-only build of the exact walk stages it): 64 bytes per node — per
// axis (lo hi hi lo), then (skip link, leaf word).  The eight bytes at (axis base + 8 s), s = sign bit of 1/d on that axis, are
// (near plane, far plane): what the two selects per axis of step_threaded pick AFTER the multiplication is picked here by the
// address, before it — the same two products either way, six v_cndmask (half rate) fewer per step.  Arithmetic and fold order are
// step_threaded's, i.e. AABB::hit's (include/aabb.h:42-65).
constexpr int kOctThreadedBytes = 64;
__device__ __forceinline__ void step_threaded_oct(Lane &L, uint32_t table_lds) {
    typedef float f2v __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const f2v lds_f2;
    typedef int i2v __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const i2v lds_i2;
    const uint32_t rec = table_lds + ((uint32_t)L.node << 6);
    const uint32_t kx = (__float_as_uint(L.inv.x) >> 28) & 8u, ky = (__float_as_uint(L.inv.y) >> 28) & 8u, kz = (__float_as_uint(L.inv.z) >> 28) & 8u;
    const f2v X = *(lds_f2 *)(uintptr_t)(rec + kx);                  // near, far
    const f2v Y = *(lds_f2 *)(uintptr_t)(rec + (16u + ky));
    const f2v Z = *(lds_f2 *)(uintptr_t)(rec + (32u + kz));
    i2v link = *(lds_i2 *)(uintptr_t)(rec + 48u);
    asm volatile("" : "+v"(link));        // (keep the one 8-byte read: see step_threaded)
    const pk2 tx = (pk2{X.x, X.y} - pk2{L.o.x, L.o.x}) * pk2{L.inv.x, L.inv.x};
    const pk2 ty = (pk2{Y.x, Y.y} - pk2{L.o.y, L.o.y}) * pk2{L.inv.y, L.inv.y};
    const pk2 tz = (pk2{Z.x, Z.y} - pk2{L.o.z, L.o.z}) * pk2{L.inv.z, L.inv.z};
    const float tmin = fmaxf(fmaxf(fmaxf(tx.x, ty.x), tz.x), 0.001f);
    const float tmax = fminf(fminf(fminf(tx.y, ty.y), tz.y), L.closest);
    const bool h = tmax > tmin;
    const int32_t leaf = link.y;
    L.sp = h ? leaf : 0;
    L.node = h ? ((L.node + 1) | (leaf & kBlocked)) : link.x;
}

// The same step on the explicit-link table (scenes too big for LDS): records [0, num_top) — the
// top levels of the tree — are read from the LDS treelet, deeper ones through L1/L2.
__device__ __forceinline__ void step_threaded_x(Lane &L, const float4 *top, const float4 *deep, int32_t num_top) {
    float4 A, B;
    if (L.node < num_top) {
        A = top[2 * L.node + 0];
        B = top[2 * L.node + 1];
    } else {
        A = deep[2 * L.node + 0];
        B = deep[2 * L.node + 1];
    }
    asm volatile("" : "+v"(B.z), "+v"(B.w));
    const pk2 tx = (pk2{A.x, A.y} - pk2{L.o.x, L.o.x}) * pk2{L.inv.x, L.inv.x};
    const pk2 ty = (pk2{A.z, A.w} - pk2{L.o.y, L.o.y}) * pk2{L.inv.y, L.inv.y};
    const pk2 tz = (pk2{B.x, B.y} - pk2{L.o.z, L.o.z}) * pk2{L.inv.z, L.inv.z};
    const bool sx = L.inv.x < 0, sy = L.inv.y < 0, sz = L.inv.z < 0;
    const float nx = sx ? tx.y : tx.x, fx = sx ? tx.x : tx.y;
    const float ny = sy ? ty.y : ty.x, fy = sy ? ty.x : ty.y;
    const float nz = sz ? tz.y : tz.x, fz = sz ? tz.x : tz.y;
    const float tmin = fmaxf(fmaxf(fmaxf(nx, ny), nz), 0.001f);
    const float tmax = fminf(fminf(fminf(fx, fy), fz), L.closest);
    const bool h = tmax > tmin;
    // inner record: z = miss link, w = hit link;  leaf record: z = next link, w = sign | (prim + 1)
    const int32_t lw = as_int(B.w);
    const bool is_leaf = lw < 0;
    const bool pend = h && is_leaf && (lw & ~kBlocked) != 0;
    const int32_t next = (h && !is_leaf) ? lw : as_int(B.z);
    L.sp = pend ? lw : 0;
    L.node = pend ? (next | kBlocked) : next;
}

template <bool kSimple = false, class SphereTab, class PlaneTab>
__device__ __forceinline__ void leaf_threaded(Lane &L, SphereTab spheres, PlaneTab planes) {
    const int32_t code = (L.sp & ~kBlocked) - 1;
    const int32_t idx = code >> 1;
    if (!kSimple && (code & 1)) test_plane(L, planes, idx, code);
    else test_sphere(L, spheres[idx], code);
    L.sp = 0;
    L.node &= ~kBlocked;                         // go on with the node after the leaf
}

// tex2D_cpu (include/materials.h:20-51), x0/y0 wrapped as well.
__device__ __forceinline__ f3 sample_texture(const KParams &P, int32_t tex_index, float u, float v) {
    const int4 info = P.tex_info[tex_index];
    const int W = info.y, H = info.z;
    const float4 *d = P.tex_data + info.x;
    u = u - floorf(u);
    v = v - floorf(v);
    const float px = u * (float)W;
    const float py = (1.0f - v) * (float)H;
    const int x0 = (int)px, y0 = (int)py;
    const int x1 = (x0 + 1) % W, y1 = (y0 + 1) % H;
    const float dx = px - (float)x0, dy = py - (float)y0;
    const int x0w = x0 % W, y0w = y0 % H;
    const float4 t00 = d[y0w * W + x0w], t10 = d[y0w * W + x1], t01 = d[y1 * W + x0w], t11 = d[y1 * W + x1];
    const f3 top = add(scale(1.0f - dx, mk(t00.x, t00.y, t00.z)), scale(dx, mk(t10.x, t10.y, t10.z)));
    const f3 bot = add(scale(1.0f - dx, mk(t01.x, t01.y, t01.z)), scale(dx, mk(t11.x, t11.y, t11.z)));
    return add(scale(1.0f - dy, top), scale(dy, bot));
}

// Final check of the guarded walk for a ray that ended with a hit (L.hit >= 0, L.closest = t): hit_bvh reaches
// this primitive for every running closest >= t only if the ray enters the caller's own leaf box BEFORE t.  If not,
// whether the reference accepts it depends on its visit order → false = flag the sample.
template <bool kSimple = false, bool kClamped = false, class SphereTab>
__device__ __forceinline__ bool guard_final_check(const Lane &L, const KParams &P, SphereTab spheres) {
    const int32_t code = L.hit;
    const int32_t idx = code >> 1;
    float enter;
    bool in;
    if (!kSimple && ((code & 1) || P.leaf_boxes)) {
        const float4 *tab = (code & 1) ? P.plane_leaf_boxes : P.leaf_boxes;
        const float4 B0 = tab[2 * idx], B1 = tab[2 * idx + 1];
        in = slab<kClamped>(L, B0.x, B0.z, B1.x, B0.y, B0.w, B1.y, 1e30f, enter);
    } else {     // every leaf box is exactly (centre - radius, centre + radius) in float: no table needed
        const float4 sp = spheres[idx];
        in = slab<kClamped>(L, sp.x - sp.w, sp.y - sp.w, sp.z - sp.w, sp.x + sp.w, sp.y + sp.w, sp.z + sp.w, 1e30f, enter);
    }
    return in && (L.closest > enter);
}

// The uniform-hemisphere scatter direction from an already drawn point in the unit sphere: random_in_hemisphere +
// the near_zero fallback.  include/materials.h has these lines twice — the LAMBERTIAN case (:74-76) and METAL's
// non-specular branch (:91-93); shade() reaches this ONE routine for both, so the reference images that pin METAL
// cover LAMBERTIAN's arithmetic as well (tests/test_host.py checks the single call site).
__device__ __forceinline__ f3 scatter_diffuse_dir(f3 in_sphere, f3 normal) {
    const f3 u = unit(in_sphere);
    f3 dir = dot(u, normal) > 0.0f ? u : neg(u);
    if (near_zero(dir)) dir = normal;
    return dir;
}

// One iteration of ray_color's loop body after hit_scene returned (src/camera.cu:226-249):
// returns true when a scattered ray was armed in L, false when the path is finished.
// kMatStride: float4 rows per material in `materials` (3 = the global table; 2 = the LDS copy, which holds only the
// two rows every hit needs — the third, absorption and index of refraction, is read from the global table by
// the DIELECTRIC branch alone; the 16 bytes per material saved buy three more entries of traversal stack).
// kSimple: the scene has no planes, no textures, no leaf-box table and no absorbing DIELECTRIC: those branches are compiled out.
// kDark: every material's `emit` is +0 and no albedo component exceeds 1 in magnitude (rtaccel::scene_emits, albedo_bounded: the host
// checked; a kSimple scene has no texture and no absorption to scale beta by), so beta — a product of albedos — stays finite and each
// addition to the radiance below is (+0) + beta * (+0) = +0: they are compiled out and L.color is never touched.
template <bool kGuard = false, int kMatStride = 3, bool kSimple = false, bool kPrim = false, bool kClamped = false, bool kDark = false, class SphereTab, class PlaneTab, class MatTab, class IdxTab>
__device__ __forceinline__ bool shade(Lane &L, const KParams &P, SphereTab spheres, PlaneTab planes, MatTab materials,
                                      IdxTab sphere_mat, f3 &out_o, f3 &out_d) {
    if (kGuard && (L.depth & kFlagBit)) return false;     // the exact walk redoes this sample
    if (L.hit < 0) {
        static_assert(!kDark || kPrim, "a kDark kernel retires a ray that left the scene in its shade step's own store round");
        if (!kDark) L.color = add(L.color, mul(L.beta, mk(P.bg[0], P.bg[1], P.bg[2])));
        return false;
    }
    const int32_t code = L.hit;
    const int32_t idx = code >> 1;
    const float t = L.closest;
    // (kPrim kernels: a camera ray's hit was checked by the primary pass — and comes without 1 / direction)
    const bool checked = kPrim && (L.depth & kFreshBit) != 0;
    if (kPrim) L.depth &= ~kFreshBit;
    if (kGuard && !(checked | guard_final_check<kSimple, kClamped>(L, P, spheres))) {
        L.depth |= kFlagBit | RTP_WHY(2);
        return false;
    }
    const f3 point = add(L.o, scale(t, L.d));        // r.at(rec.t)
    f3 normal;
    bool front;
    int32_t mat_idx;
    float tu = 0.0f, tv = 0.0f;
    const bool is_plane = !kSimple && (code & 1) != 0;
    f3 outward = mk(0, 0, 0);
    if (is_plane) {
        const float4 P0 = planes[5 * idx + 0];
        const float4 P2 = planes[5 * idx + 2];
        outward = mk(P0.x, P0.y, P0.z);
        mat_idx = as_int(P2.w);
    } else {
        const float4 s = spheres[idx];
        outward = divs(sub(point, mk(s.x, s.y, s.z)), s.w);
        mat_idx = sphere_mat[idx];
    }
    front = dot(L.d, outward) < 0;                   // set_face_normal, include/hittable_object.h:17-20
    normal = front ? outward : neg(outward);

    const float4 MA = materials[kMatStride * mat_idx + 0];     // albedo, type | texture_id << 2
    // emit, fuzz: with one row per material in LDS (kMatStride == 1) this row comes from the global table — issued here,
    // first needed after the rejection-sampling loop
    const float4 ME = kMatStride >= 2 ? materials[kMatStride * mat_idx + 1] : P.materials[3 * mat_idx + 1];
    const int32_t type = as_int(MA.w) & 3;
    const int32_t tex_id = kSimple ? 0 : (as_int(MA.w) >> 2);
    f3 albedo = mk(MA.x, MA.y, MA.z);
    if (tex_id != 0) {
        if (is_plane) {                                // rec.u/v = alpha/beta of hit_plane
            const float4 P1 = planes[5 * idx + 1];
            const float4 P2 = planes[5 * idx + 2];
            const float4 P3 = planes[5 * idx + 3];
            const float4 P4 = planes[5 * idx + 4];
            const f3 ph = sub(point, mk(P4.x, P4.y, P4.z));
            const f3 w = mk(P1.x, P1.y, P1.z);
            tu = dot(w, cross(ph, mk(P3.x, P3.y, P3.z)));
            tv = dot(w, cross(mk(P2.x, P2.y, P2.z), ph));
        } else {                                       // get_sphere_uv, include/sphere.h:16-22
            const float theta = acos_libm(outward.y);            // (the host libm's algorithms: rt_device_math.h)
            const float phi = (float)((double)atan2_libm(-outward.z, outward.x) + 3.14159265358979323846);
            tu = (float)((double)phi / (2 * 3.14159265358979323846));
            tv = (float)((double)theta / 3.14159265358979323846);
        }
        albedo = mul(albedo, sample_texture(P, tex_id - 1, tu, tv));
    }
    // final_color += beta * emitted (src/camera.cu:239) — added below, once the row has had the loop's time to arrive;
    // beta does not change before that
    const f3 beta_in = L.beta;

    // ---- material_scatter (include/materials.h:70-140).  The RNG draws happen in the reference's
    // order per material; the rejection-sampled point in the unit sphere that LAMBERTIAN and both
    // METAL branches need is drawn in ONE loop shared by all those lanes.
    f3 new_o = point, new_d = normal, att = albedo;
    f3 glass_offset = mk(0, 0, 0);       // kPrim: the 1e-4 step off a DIELECTRIC's surface (the new origin is made at the end)
    const bool is_lamb = type == RT_MAT_LAMBERTIAN;
    const bool is_metal = type == RT_MAT_METAL;
    const bool is_glass = type == RT_MAT_DIELECTRIC;
    if (!(is_lamb || is_metal || is_glass)) {                        // DIFFUSE_LIGHT (:135-137)
        if (!kDark) L.color = add(L.color, mul(beta_in, mk(ME.x, ME.y, ME.z)));
        return false;
    }
    // absorption and index of refraction live in global memory (kMatStride == 2): issue the read NOW, so that its
    // latency runs under the rejection-sampling loop below instead of stalling the DIELECTRIC branch
    float4 MB = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    if (is_glass) {
        if (kSimple) MB.w = reinterpret_cast<const float *>(P.materials + 3 * mat_idx + 2)[3];     // (no absorbing glass in such a scene: the index of refraction alone)
        else MB = kMatStride >= 3 ? materials[kMatStride * mat_idx + 2] : P.materials[3 * mat_idx + 2];
    }
    bool metal_reflect = false;
    if (is_metal) metal_reflect = random_float(L.seed) < 0.8f;       // p_metal draw comes first (:82-83)
    f3 in_sphere = mk(0, 0, 0);
    if (is_lamb || is_metal) in_sphere = random_in_unit_sphere(L.seed);
    if (!kDark) L.color = add(L.color, mul(beta_in, mk(ME.x, ME.y, ME.z)));      // final_color += beta * emitted
    f3 ud = mk(0, 0, 0);
    if (metal_reflect || is_glass) ud = unit(L.d);                   // unit_vector(r_in.direction())
    if (is_glass) {                                                  // :98-133
        const float ir = MB.w;                                       // MB: absorption, ir (read above)
        const float ratio = front ? ME.w : ir;                       // ME.w of a DIELECTRIC row: (float)(1.0 / ir), made by the packer
        const float cos_theta = fminf(dot(neg(ud), normal), 1.0f);
        const float sin_theta = sqrt_cr(1.0f - cos_theta * cos_theta);
        const bool cannot_refract = ratio * sin_theta > 1.0f;
        bool do_reflect = cannot_refract;
        if (!cannot_refract) {                                       // MA.x / MA.y of a DIELECTRIC row: r0^2 per side
            const float rnd = random_float(L.seed);
            if (kGuard) {
                // (rt_device_math.h: decided by the neighbours of the rounded x^5; a draw inside their two-ulp window — one in
                // ~1e7 — sends the sample to the exact walk, whose shade step evaluates the libm's powf itself)
                const int b = schlick_bracket(cos_theta, front ? MA.x : MA.y, rnd);
                if (b < 0) { L.depth |= kFlagBit | kNoResumeBit | RTP_WHY(2); return false; }
                do_reflect = b != 0;
            } else {
                do_reflect = schlick_exceeds(cos_theta, front ? MA.x : MA.y, rnd);
            }
        }
        new_d = do_reflect ? reflect(ud, normal) : refract(ud, normal, ratio);
        att = mk(1.0f, 1.0f, 1.0f);
        // (kSimple: no DIELECTRIC of the scene absorbs — rt_render checks — so the transmission is exactly 1, the survival
        // probability exactly 1 and the roulette draw, which can be 1.0 but not more, never ends the path; only the draw remains)
        if (!kSimple && !front) {
            const float dist = sqrt_cr(lensq(sub(point, L.o)));
            // exp(-0 * d) is exactly 1: skip the evaluation for non-absorbing glass
            const f3 tr = mk(MB.x == 0.0f ? 1.0f : exp_libm(-MB.x * dist), MB.y == 0.0f ? 1.0f : exp_libm(-MB.y * dist),
                             MB.z == 0.0f ? 1.0f : exp_libm(-MB.z * dist));
            att = mul(att, tr);
        }
        const float p = fmaxf(att.x, fmaxf(att.y, att.z));
        if (random_float(L.seed) > p && !kSimple) return false;      // Russian roulette
        if (!kSimple && p != 1.0f) att = scale(recip(p), att);       // 1/1 is 1 and 1 * att is att: non-absorbing glass skips the division
        const float side = dot(new_d, normal) > 0 ? 1.0f : -1.0f;
        if (kPrim) glass_offset = scale(side, scale(1e-4f, normal));
        else new_o = add(point, scale(side, scale(1e-4f, normal)));
    } else if (metal_reflect) {                                      // :84-88
        new_d = add(reflect(ud, normal), scale(ME.w, in_sphere));
        if (!(dot(new_d, normal) > 0)) return false;
    } else {                                                         // LAMBERTIAN (:74-76) and METAL's 20 % branch (:90-93)
        new_d = scatter_diffuse_dir(in_sphere, normal);
    }
    L.beta = mul(L.beta, att);
    L.depth++;
    if (L.depth >= P.max_depth) return false;
    if (kPrim) {
        // The lane's old ray is spent: the new one takes its place, no second copy alive across the step.  The hit point is made
        // AGAIN here, from the ray that is still in place (the same expression, the same bits; the fence keeps the compiler from
        // merging the two, which would hold three registers across the whole step — the ones the 64-register build lacks)
        float t_again = L.closest;
        asm volatile("" : "+v"(t_again));
        const f3 point_again = add(L.o, scale(t_again, L.d));
        L.o = is_glass ? add(point_again, glass_offset) : point_again;
        L.d = new_d;
    } else {
        out_o = new_o;
        out_d = new_d;
    }
    return true;
}

// ---- the launch constants of the shade step's tail, from LDS (kSimple) ---------------------------------------------------
// The 8-waves-per-SIMD build has 64 VGPRs and the same 102 SGPRs as any kernel; what the sample store / fetch / camera-ray code
// reads from the kernel argument does not fit next to the exec-mask temporaries of the walk, so the compiler spilled it to VGPR
// lanes and restored it with some 70 v_readlane_b32 per shade step (half-rate VALU, §5g).  The workgroup keeps those constants in a
// small LDS block instead (written once, read with broadcast ds_read_b128 — LDS instructions, not VALU):
//   [0..2] guard_origin: centre + d0^2 | rs, fark, box x | box y z          [3] du, p00.x   [4] dv, p00.y   [5] origin, p00.z
//   [6] magic_count.m .s-32, magic_width.m .s-32                                  [7] width, slab_pitch, pass_first, pass_count
//   [8] flag_list, flag_count (pointers as two words each)   [9] dirty, dirty_list   [10] dirty_count, flag_cap, chunk   [11] queue, taper_shift
//   [11].w flag_chunk_words | bail_share << 8 | bail_floor << 16
//   [12] order (kPrim: the row — pixel centre, local pixel — each position of the fetch order stands for), abandon
//   [13] the codes of the front primitives (kNoFront: none in that slot)
typedef float f4v __attribute__((ext_vector_type(4)));       // (a native vector: HIP's float4 struct has no address-space-qualified copy)
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const f4v lds_cfloat4;
typedef __attribute__((address_space(3))) const u4v lds_cuint4;
constexpr int kConstRows = 14;
constexpr uint32_t kNoFront = 0xffffffffu;
// host: lay the block out in the kernel argument (after every field it copies is final, i.e. right before the launch)
inline void fill_consts(KParams &P) {
    auto f = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
    auto lo = [](const void *q) { return (uint32_t)(uintptr_t)q; };
    auto hi = [](const void *q) { return (uint32_t)((uintptr_t)q >> 32); };
    const uint32_t rows[kConstRows][4] = {
        {f(P.g_center[0]), f(P.g_center[1]), f(P.g_center[2]), f(P.g_d0sq)},
        {f(P.g_rs), f(P.g_fark), f(P.g_box[0]), f(P.g_box[1])},
        {f(P.g_box[2]), f(P.g_box[3]), f(P.g_box[4]), f(P.g_box[5])},
        {f(P.du[0]), f(P.du[1]), f(P.du[2]), f(P.p00[0])},
        {f(P.dv[0]), f(P.dv[1]), f(P.dv[2]), f(P.p00[1])},
        {f(P.origin[0]), f(P.origin[1]), f(P.origin[2]), f(P.p00[2])},
        // (the two shift counts take five bits; the tile's first column and row ride in the bits above)
        {P.magic_count.m, ((P.magic_count.s - 32u) & 31u) | ((uint32_t)P.tile_x0 << 8), P.magic_width.m, ((P.magic_width.s - 32u) & 31u) | ((uint32_t)P.tile_y0 << 8)},
        {(uint32_t)P.row_w, P.slab_pitch, (uint32_t)P.pass_first, (uint32_t)P.pass_count},
        {lo(P.flag_list), hi(P.flag_list), lo(P.flag_count), hi(P.flag_count)},
        {lo(P.dirty), hi(P.dirty), lo(P.dirty_list), hi(P.dirty_list)},
        {lo(P.dirty_count), hi(P.dirty_count), P.flag_cap, P.chunk},
        {lo(P.queue), hi(P.queue), P.taper_shift, P.flag_chunk_words | (P.bail_share << 8) | (P.bail_floor << 16) | (P.bail_latest << 24)},
        {lo(P.order), hi(P.order), lo(P.abandon), hi(P.abandon)},
        {P.num_front > 0 ? (uint32_t)P.front_code[0] : kNoFront, P.num_front > 1 ? (uint32_t)P.front_code[1] : kNoFront,
         P.num_front > 2 ? (uint32_t)P.front_code[2] : kNoFront, P.num_front > 3 ? (uint32_t)P.front_code[3] : kNoFront},
    };
    std::memcpy(P.consts, rows, sizeof(rows));
}
__device__ __forceinline__ void write_consts(const KParams &P, uint32_t consts_lds, int tid) {
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    if (tid < kConstRows * 4) ((lds_u32 *)(uintptr_t)consts_lds)[tid] = P.consts[tid];
}
__device__ __forceinline__ uint32_t *ptr_from(uint32_t lo, uint32_t hi) { return reinterpret_cast<uint32_t *>((uintptr_t)lo | ((uintptr_t)hi << 32)); }
// div_magic with its operands in vector registers: the d == 1 case (m == 0) by select, not by a branch
// (s >= 32 whenever m != 0 — make_magic: s = 31 + floor(log2 d), d >= 2 — so the quotient is the high half of the product
// shifted by s - 32: v_mul_hi_u32 + a 32-bit shift instead of a 64-bit multiply-add and a 64-bit shift)
// (the constants block holds s - 32, masked to five bits for the d == 1 record)
__device__ __forceinline__ uint32_t div_magic_v(uint32_t n, uint32_t m, uint32_t s_minus_32) {
    const uint32_t r = __umulhi(n, m) >> (s_minus_32 & 31u);        // (the word's upper bits carry a tile offset)
    return m ? r : n;
}

// The centre of pixel (i, j) on the image plane: this very expression, in this order, is what order_scatter_kernel (rt_primary.hip.inc)
// leaves in the pixel's row of the fetch-order table, compiled in the same translation unit with the same flags.
__device__ __forceinline__ f3 pixel_center(f3 p00, f3 du, f3 dv, int32_t i, int32_t j) { return add(add(p00, scale((float)i, du)), scale((float)j, dv)); }
// camera_ray (below, its kFromLds form) behind the pixel's centre — kPrim takes the centre from the fetch-order table (map_fetch).
// (A function of its own, not a call from camera_ray: the other kernels keep the code they had, instruction for instruction.)
__device__ __forceinline__ void camera_ray_from_center(Lane &L, f3 center, uint32_t seed1, f3 &out_o, f3 &out_d, uint32_t consts_lds) {
    uint32_t seed = seed1;
    const float ox = (float)seed * 2.3283064365386962890625e-10f - 0.5f;
    const f4v a = ((lds_cfloat4 *)(uintptr_t)consts_lds)[3], b = ((lds_cfloat4 *)(uintptr_t)consts_lds)[4], c = ((lds_cfloat4 *)(uintptr_t)consts_lds)[5];
    const f3 du = mk(a.x, a.y, a.z), dv = mk(b.x, b.y, b.z);
    const float oy = random_float(seed) - 0.5f;
    const f3 sample = add(add(center, scale(ox, du)), scale(oy, dv));
    const f3 org = mk(c.x, c.y, c.z);
    L.seed = seed;
    L.beta = mk(1.0f, 1.0f, 1.0f);
    L.color = mk(0.0f, 0.0f, 0.0f);
    L.depth = 0;
    out_o = org;
    out_d = sub(sample, org);
}
// Seeds + CameraData::get_ray (src/camera.cu:25-29, include/camera.cuh:97-109).
// seed1: the RNG state after the first draw's hash, wang_hash(wang_hash(base_seed + s)) — the value the primary-visibility
// pass leaves in the third word of a sample's record, so that the trace kernel does not hash the pixel and the sample again.
template <bool kFromLds = false>
__device__ __forceinline__ void camera_ray(Lane &L, const KParams &P, int32_t i, int32_t j, uint32_t seed1, f3 &out_o, f3 &out_d, uint32_t consts_lds = 0) {
    uint32_t seed = seed1;
    const float ox = (float)seed * 2.3283064365386962890625e-10f - 0.5f;       // random_float's value for this state
    if (kFromLds) {
        const f4v a = ((lds_cfloat4 *)(uintptr_t)consts_lds)[3], b = ((lds_cfloat4 *)(uintptr_t)consts_lds)[4], c = ((lds_cfloat4 *)(uintptr_t)consts_lds)[5];
        const f3 du = mk(a.x, a.y, a.z), dv = mk(b.x, b.y, b.z);
        const f3 center = pixel_center(mk(a.w, b.w, c.w), du, dv, i, j);
        const float oy = random_float(seed) - 0.5f;
        const f3 sample = add(add(center, scale(ox, du)), scale(oy, dv));
        const f3 org = mk(c.x, c.y, c.z);
        L.seed = seed;
        L.beta = mk(1.0f, 1.0f, 1.0f);
        L.color = mk(0.0f, 0.0f, 0.0f);
        L.depth = 0;
        out_o = org;
        out_d = sub(sample, org);
        return;
    }
    // (direct member reads of the kernel argument: scalar loads into SGPRs; through a pointer — ld3(P.du) — the compiler
    // emitted per-lane global loads with a wait on every use, one exposed memory round trip per shade step)
    const f3 du = mk(P.du[0], P.du[1], P.du[2]), dv = mk(P.dv[0], P.dv[1], P.dv[2]);
    const f3 center = pixel_center(mk(P.p00[0], P.p00[1], P.p00[2]), du, dv, i, j);
    const float oy = random_float(seed) - 0.5f;
    const f3 sample = add(add(center, scale(ox, du)), scale(oy, dv));
    const f3 org = mk(P.origin[0], P.origin[1], P.origin[2]);
    L.seed = seed;
    L.beta = mk(1.0f, 1.0f, 1.0f);
    L.color = mk(0.0f, 0.0f, 0.0f);
    L.depth = 0;
    out_o = org;
    out_d = sub(sample, org);
}
__device__ __forceinline__ uint32_t sample_seed1(uint32_t base_seed, int32_t s) { return wang_hash(wang_hash(base_seed + (uint32_t)s)); }
template <bool kFromLds = false>
__device__ __forceinline__ void start_sample(Lane &L, const KParams &P, int32_t i, int32_t j, uint32_t base_seed, int32_t s,
                                             f3 &out_o, f3 &out_d, uint32_t consts_lds = 0) {
    camera_ray<kFromLds>(L, P, i, j, sample_seed1(base_seed, s), out_o, out_d, consts_lds);
}

// ---- thin lens and open shutter (rt_render_lens; include/rtp_amd.h, rt_lens_params) -------------------------------------------
// The camera pair at the two ends of the shutter (index 0: open, 1: close) and the lens.  Uniform over a launch: a kernel argument.
struct LensCam {
    float o[2][3], p00[2][3], du[2][3], dv[2][3];
    float radius, focus;       // lens radius (0: pinhole, no lens draws), distance of the plane in focus
    int32_t motion;            // 1: a time is drawn per sample and the pose interpolated, 0: the open camera
    int32_t width;             // image width (the per-pixel seed)
};
__device__ __forceinline__ f3 lens_pose(const float (&x)[2][3], int32_t motion, float tau) {
    const f3 x0 = mk(x[0][0], x[0][1], x[0][2]);
    if (!motion) return x0;
    return add(x0, scale(tau, sub(mk(x[1][0], x[1][1], x[1][2]), x0)));       // X0 + tau * (X1 - X0), per component
}
__device__ __forceinline__ f3 div_cr(f3 v, float t) { return mk(v.x / t, v.y / t, v.z / t); }      // correctly rounded quotients (parity flags)
// The header's arithmetic, in its order: ox, oy as camera_ray draws them, then tau (motion), then (lx, ly) by rejection (lens); the
// pinhole ray (O, S - O); with a lens, the ray from the lens point through the point where the pinhole ray meets the plane in focus.
// The path goes on from the RNG state the draws leave.
__device__ __forceinline__ void lens_camera_ray(Lane &L, const LensCam &C, int32_t i, int32_t j, uint32_t seed1, f3 &out_o, f3 &out_d) {
    uint32_t seed = seed1;
    const float ox = (float)seed * 2.3283064365386962890625e-10f - 0.5f;
    const float oy = random_float(seed) - 0.5f;
    const float tau = C.motion ? random_float(seed) : 0.0f;
    const f3 org = lens_pose(C.o, C.motion, tau), p00 = lens_pose(C.p00, C.motion, tau);
    const f3 du = lens_pose(C.du, C.motion, tau), dv = lens_pose(C.dv, C.motion, tau);
    float lx = 0.0f, ly = 0.0f;
    const bool lens = C.radius > 0.0f;
    if (lens) {
        do {                    // random_in_unit_sphere's rejection in two dimensions: x first
            lx = -1.0f + 2.0f * random_float(seed);
            ly = -1.0f + 2.0f * random_float(seed);
        } while (lx * lx + ly * ly >= 1.0f);
    }
    const f3 center = add(add(p00, scale((float)i, du)), scale((float)j, dv));
    const f3 sample = add(add(center, scale(ox, du)), scale(oy, dv));
    f3 o = org, d = sub(sample, org);
    if (lens) {
        const f3 n = cross(du, dv);
        const float dimg = fabsf(dot(sub(p00, org), n)) / sqrt_cr(dot(n, n));
        const float k = C.focus / dimg;
        const f3 focus = add(org, scale(k, d));
        const f3 uh = div_cr(du, sqrt_cr(dot(du, du))), vh = div_cr(dv, sqrt_cr(dot(dv, dv)));
        o = add(add(org, scale(C.radius * lx, uh)), scale(C.radius * ly, vh));
        d = sub(focus, o);
    }
    L.seed = seed;
    L.beta = mk(1.0f, 1.0f, 1.0f);
    L.color = mk(0.0f, 0.0f, 0.0f);
    L.depth = 0;
    out_o = o;
    out_d = d;
}

// n / d with a host-made reciprocal: m = floor(2^s / d) + 1, s = 31 + floor(log2 d), packed as
// (m, s).  Exact for n < 2^30 (n * d < 2^s, checked on the host in make_magic; rt_accel.h, plan_passes keeps every work
// index of a pass and the 64 behind it below 2^30); two multiplies
// instead of the ~25-instruction integer division.  m == 0 encodes d == 1.
__device__ __forceinline__ uint32_t div_magic(uint32_t n, Magic g) {
    return g.m ? (uint32_t)(((uint64_t)n * (uint64_t)g.m) >> g.s) : n;
}

// The value ray_color returns for the sample with work index w → its 12-byte record of the slab.  Pixel-major
// ([pixel][slot]): the samples of a pixel are traced side by side by the lanes of one wave, so their records fill
// whole cache lines while those are still in the XCD's L2 — with the round-1 layout ([slot][pixel], 16-byte records)
// every line collected its 8 records from 8 different pixels, often from different XCDs, and HBM saw 2.07 x the
// bytes.  accumulate_kernel transposes through LDS to read it coalesced.
template <bool kFromLds = false>
__device__ __forceinline__ void store_sample(const KParams &P, uint32_t w, f3 color, uint32_t consts_lds = 0) {
    if (kFromLds) {
        const u4v mg = ((lds_cuint4 *)(uintptr_t)consts_lds)[6], wd = ((lds_cuint4 *)(uintptr_t)consts_lds)[7];
        const uint32_t sq = div_magic_v(w, mg.x, mg.y);
        const uint32_t sk = w - sq * wd.w;
        float *rec = P.slab + (size_t)(sq * wd.y + sk) * 3;        // pixels x pitch < 2^32 (the pass fits the 32-bit work index): one 64-bit multiply-add
        rec[0] = color.x; rec[1] = color.y; rec[2] = color.z;
        return;
    }
    const uint32_t sq = P.pass_count == 64 ? (w >> 6) : div_magic(w, P.magic_count);
    const uint32_t sk = w - sq * (uint32_t)P.pass_count;
    float *rec = P.slab + ((size_t)sq * P.slab_pitch + sk) * 3;
    rec[0] = color.x; rec[1] = color.y; rec[2] = color.z;
}

// local pixel q of the call's rows (a tile, or a shard's bands) → image pixel
__device__ __forceinline__ void local_to_image(const KParams &P, uint32_t q, int32_t &pi, int32_t &pj) {
    const uint32_t pjl = div_magic(q, P.magic_width);
    pi = (int32_t)(q - pjl * (uint32_t)P.row_w) + P.tile_x0;
    // local row → image row: band b = pjl / band_rows belongs to part, bands interleave
    if (P.num_parts == 1) {
        pj = (int32_t)pjl + P.tile_y0;
    } else {
        const uint32_t band = div_magic(pjl, P.magic_band);
        pj = (int32_t)((band * (uint32_t)P.num_parts + (uint32_t)P.part) * (uint32_t)P.band_rows + (pjl - band * (uint32_t)P.band_rows));
    }
}
// work index of a pass → (local pixel, slot) → image pixel and first ray of the sample
// (kFromLds: also returns the image width and the pass's first sample, which the caller needs next)
template <bool kFromLds = false>
__device__ __forceinline__ void map_work(const KParams &P, uint32_t w, int32_t &pi, int32_t &pj, uint32_t &k, uint32_t consts_lds = 0,
                                         uint32_t *width_out = nullptr, int32_t *first_out = nullptr, uint32_t *record_out = nullptr) {
    if (kFromLds) {
        const u4v mg = ((lds_cuint4 *)(uintptr_t)consts_lds)[6], wd = ((lds_cuint4 *)(uintptr_t)consts_lds)[7];
        const uint32_t q = div_magic_v(w, mg.x, mg.y);
        k = w - q * wd.w;
        if (record_out) *record_out = q * wd.y + k;          // the sample's record of the slab (store_sample)
        const uint32_t pjl = div_magic_v(q, mg.z, mg.w);
        pi = (int32_t)(q - pjl * wd.x + (mg.y >> 8));
        if (P.num_parts == 1) {
            pj = (int32_t)(pjl + (mg.w >> 8));
        } else {
            const uint32_t band = div_magic(pjl, P.magic_band);
            pj = (int32_t)((band * (uint32_t)P.num_parts + (uint32_t)P.part) * (uint32_t)P.band_rows + (pjl - band * (uint32_t)P.band_rows));
        }
        *width_out = (uint32_t)P.width;
        *first_out = (int32_t)wd.z;
        return;
    }
    const uint32_t q = P.pass_count == 64 ? (w >> 6) : div_magic(w, P.magic_count);
    k = w - q * (uint32_t)P.pass_count;
    if (record_out) *record_out = q * P.slab_pitch + k;
    local_to_image(P, q, pi, pj);
}

// kPrim: the work index counts in fetch order (expensive pixels first).  Position of the fetch order → its row of the table
// (order_scatter_kernel, rt_primary.hip.inc): the pixel's centre on the image plane and the local pixel, in ONE 16-byte load where
// there was the pixel's word, so nothing of the pixel's own arithmetic (column, row, band, two conversions, the centre's six products
// and sums) is left to the few lanes that fetch.  The sample is known by pixel * count + slot from here on (canonical), and
// record is its slot of the slab (store_sample).
constexpr int kOrderRowWords = 4;
__device__ __forceinline__ void map_fetch(uint32_t w, uint32_t consts_lds, uint32_t &canonical, uint32_t &record, f3 &center) {
    const u4v mg = ((lds_cuint4 *)(uintptr_t)consts_lds)[6], wd = ((lds_cuint4 *)(uintptr_t)consts_lds)[7];
    const uint32_t pos = div_magic_v(w, mg.x, mg.y);
    const uint32_t k = w - pos * wd.w;
    typedef uint32_t u2v __attribute__((ext_vector_type(2)));
    const u2v od = *(__attribute__((address_space(3))) const u2v *)(uintptr_t)(consts_lds + 16u * 12u);
    const u4v row = *reinterpret_cast<const u4v *>(ptr_from(od.x, od.y) + (size_t)pos * kOrderRowWords);
    center = mk(__uint_as_float(row.x), __uint_as_float(row.y), __uint_as_float(row.z));
    canonical = row.w * wd.w + k;
    record = row.w * wd.y + k;
}

__device__ __forceinline__ int lane_rank(uint64_t mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Lane state predicates.  Ordered mode: node >= 0 inner, node < 0 (not kDone) leaf.
// Threaded mode: sp != 0 → a primitive test is pending, else node != kDone → next box test.
// Threaded mode: node >= 0 → box test wanted; node < 0 with sp != 0 → primitive test pending;
// node < 0 with sp == 0 → walk finished (or lane idle).
template <bool kThreaded>
__device__ __forceinline__ bool wants_leaf(const Lane &L, int32_t end_node) {
    return kThreaded ? (L.sp != 0) : (L.node < 0 && L.node != end_node);
}
template <bool kThreaded>
__device__ __forceinline__ bool wants_inner(const Lane &L, int32_t end_node) {
    (void)end_node;
    return L.node >= 0;
}
template <bool kThreaded>
__device__ __forceinline__ bool traversal_finished(const Lane &L, int32_t end_node) {
    return kThreaded ? (L.node < 0 && L.sp == 0) : (L.node == end_node);
}

// Far-origin test of the guarded walk.  The inflation of the small spheres' boxes covers paths that
// start within sqrt(g_d0sq) of their cluster.  A ray from farther away is safe if it stays clear
// of the cluster's box grown by the margin that distance asks for; otherwise the sample is flagged.
// kFromLds: the twelve constants come from a block the workgroup keeps in LDS (three broadcast ds_read_b128) instead of
// scalar registers: in the 8-waves-per-SIMD build they were SGPR spills, restored with 24 v_readlane per shade step.
template <bool kFromLds = false>
__device__ __forceinline__ void guard_origin(Lane &L, const KParams &P, uint32_t consts_lds = 0) {
    f4v c0, c1, c2;
    if (kFromLds) {
        c0 = ((lds_cfloat4 *)(uintptr_t)consts_lds)[0];
    } else {
        c0 = f4v{P.g_center[0], P.g_center[1], P.g_center[2], P.g_d0sq};
    }
    const f3 q = sub(L.o, mk(c0.x, c0.y, c0.z));
    const float dd = dot(q, q);
    if (dd > c0.w) {
        if (kFromLds) {
            c1 = ((lds_cfloat4 *)(uintptr_t)consts_lds)[1];
            c2 = ((lds_cfloat4 *)(uintptr_t)consts_lds)[2];
        } else {
            c1 = f4v{P.g_rs, P.g_fark, P.g_box[0], P.g_box[1]};
            c2 = f4v{P.g_box[2], P.g_box[3], P.g_box[4], P.g_box[5]};
        }
        const float reach = sqrt_cr(dd) + c1.x;
        const float grow = c1.y * reach * reach;
        float enter;
        const bool in = slab(L, c1.z - grow, c2.x - grow, c2.z - grow, c1.w + grow, c2.y + grow,
                             c2.w + grow, 1e30f, enter);
        if (in || !(grow < 1e30f)) {
            L.depth |= kFlagBit | RTP_WHY(3);
            L.node = kDone;           // nothing to walk: the next shade step retires the sample
        }
    }
}

// ---- the flagged-sample list (guarded kernels) ------------------------------------------------------------------------------
// A sample the guarded walk cannot vouch for goes on a list the exact walk works off (retire_sample calls flag_collect).
//   * the lanes that are flagged together append together: ranks from one ballot, one atomic on the list's counter for all of them;
//   * a wave that keeps flagging reserves list slots kFlagChunk at a time.  An atomic on that ONE address takes its turn at about
//     11 ns whoever issues it: per lane, a scene that flags 46 % of its samples spent 250 ms of a 16 ms frame there (round 3); per
//     wave and shade step, one that flags 35 % still spent 65 ms of a 79 ms launch there (round 4: 690 overlapping spheres, the
//     camera among them).  The wave's chunk [next, end) lives in two LDS words (flag_chunk_words per wave: 2, or 0 where LDS has
//     none to spare — then every append is its own atomic, as before).  The first kFlagChunkAfter samples a wave flags are appended
//     one step at a time all the same: a frame that flags a few samples per wave (the headline frame: 22) gets the list it always
//     got, and the short-list rule of the re-walk (render_kernel) sees its true length;
//   * what a wave has not used of its last chunk when it leaves is filled with kFlagHole — the re-walk's fetch passes over those —
//     and counted in the word kFlagHolesWords behind the list's counter (the host reports counter - holes);
//   * the lane that made the atomic prices the pass: list slots handed out so far (flagged samples, plus at most a chunk per wave)
//     against samples handed out so far (the pass's work counter); above bail_share / 256 it sets the pass's abandon word
//     (KParams::abandon);
//   * the sample's pixel is only MARKED (dirty_compact_kernel lists the marks after the launch).
constexpr uint32_t kAbandonedCounter = 0x40000000u;   // what an abandoned pass's work counter is raised to
constexpr uint32_t kFlagChunk = 64u;                  // list slots per reservation of a wave in chunk mode (>= the lanes of a wave)
constexpr uint32_t kFlagChunkAfter = 64u;             // … which a wave enters once it has flagged this many samples
constexpr uint32_t kFlagHole = 0xffffffffu;           // list entry nobody filled (work indices stay below 2^30)
constexpr uint32_t kFlagHolesWords = 3u * 1024u + 16u;      // holes word = flag_count + this (rt_capi.hip: kQueueHoles - kQueueFlag)
typedef __attribute__((address_space(3))) volatile uint32_t lds_chunk_word;
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u2v lds_cu2;
typedef __attribute__((address_space(3))) const uint32_t lds_cu1;
// (chunk_lds: where the chunk words of the workgroup's waves begin — behind the constants block: render_kernel makes it)
__device__ __forceinline__ lds_chunk_word *flag_chunk_of(uint32_t chunk_lds, uint32_t words, uint32_t wave) {
    return (lds_chunk_word *)(uintptr_t)chunk_lds + wave * words;
}
// word 0: next free slot of the wave's chunk — while word 1 (its end) is 0: how many samples the wave has flagged so far
__device__ __forceinline__ void flag_chunk_init(uint32_t chunk_lds, uint32_t words, int wave, int lane) {
    if (words != 0u && lane < 2) flag_chunk_of(chunk_lds, words, (uint32_t)wave)[lane] = 0u;
}
// (everything the wave's lanes agree on — pointers, limits, counts — is read from the constants block into SCALAR registers, right
// where it is used: this code runs inside the shade step with the lane's path live, and each vector register it holds on to is one
// the hot shade step has to spill)
__device__ __forceinline__ uint32_t lds_s32(uint32_t addr) { return __builtin_amdgcn_readfirstlane(*(lds_cu1 *)(uintptr_t)addr); }
__device__ __forceinline__ uint32_t *lds_sptr(uint32_t addr) { const uint32_t lo = lds_s32(addr), hi = lds_s32(addr + 4u); return ptr_from(lo, hi); }
// `want` list slots with one atomic (rank 0's) → where they begin; the pass is priced on the way
__device__ __forceinline__ uint32_t flag_reserve(uint32_t consts_lds, uint32_t pool_lds, uint32_t total_work, int rank, uint32_t want) {
    uint32_t base = 0;
    if (rank == 0) base = atomicAdd(lds_sptr(consts_lds + 16u * 8u + 8u), want);
    base = __builtin_amdgcn_readfirstlane(base);
    const uint32_t share = (lds_s32(consts_lds + 16u * 11u + 12u) >> 8) & 255u;
    if (share != 0u) {
        // (both counts below 2^31, share < 256 and floor < 256: 32-bit arithmetic; a floor of 64 Ki samples' worth against early noise)
        // "handed out so far" = where this wave's own latest reservation ends (the high half of its range word in LDS; 0 once the
        // pass is dry).  NOT a load of the counter itself: an agent-scope load of that one hot address takes its turn among the
        // reservations' atomics like an atomic — 115 k of them made a 3.4 ms launch take 6.4 ms
        uint32_t handed = __builtin_amdgcn_readfirstlane(*(lds_chunk_word *)(uintptr_t)(pool_lds + 4u));      // (volatile: the range word changes)
        if (handed == 0u || handed > total_work) handed = total_work;
        // … and flagged so far against the WHOLE pass (bail_floor, in 1/1024ths of it): the fetch order puts the pixels with the
        // most candidate leaves first, so the share among the first samples can be several times the frame's (1 512 spheres, 3.5 %
        // flagged overall, gave up at once; so did 83 spheres at 1.8 %).  A pass that ends below the floor is never given up
        const uint32_t floor = (lds_s32(consts_lds + 16u * 11u + 12u) >> 16) & 255u, latest = lds_s32(consts_lds + 16u * 11u + 12u) >> 24;
        // … and only early in a pass (bail_latest, in eighths of it): giving up means the exact walk renders ALL of it, what is
        // left of the guarded launch included — a pass that crossed the floor with its last samples took 1.54 x the exact walk's
        // time.
        // (What giving up costs is the samples up to the floor — the expensive pixels come first: 3 % of a 1280 x 720 x 48 pass's
        // samples were a quarter of its time — not what the waves still hold: dropping their reservations, or starting the pass
        // with reservations of 64, bought nothing measurable; the latter cost every small frame a millisecond of atomics.)
        if (base + want > ((handed >> 8) + 256u) * share && base + want > (total_work >> 10) * floor && handed < (total_work >> 3) * latest) {
            uint32_t *abandon = lds_sptr(consts_lds + 16u * 12u + 8u);
            if (rank == 0 && abandon != nullptr) {
                __hip_atomic_store(abandon, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // every later reservation finds the pass dry: the counter jumps beyond the last work index (indices stay below
                // 2^30, reservations add at most a few million more: no wrap)
                atomicMax(lds_sptr(consts_lds + 16u * 11u), kAbandonedCounter);
            }
        }
    }
    return base;
}
// called by the lanes whose sample is flagged, together
__device__ __forceinline__ void flag_collect(uint32_t w_flagged, uint32_t consts_lds, uint32_t chunk_lds, uint32_t pool_lds, uint32_t wave, uint32_t total_work) {
    const uint64_t fm = __ballot(1);
    const int rank = lane_rank(fm);
    const uint32_t lanes = (uint32_t)__popcll(fm);
    const uint32_t words = lds_s32(consts_lds + 16u * 11u + 12u) & 255u;
    uint32_t slot;
    if (words == 0u) {
        slot = flag_reserve(consts_lds, pool_lds, total_work, rank, lanes) + (uint32_t)rank;
    } else {
        lds_chunk_word *l_chunk = flag_chunk_of(chunk_lds, words, wave);
        const uint32_t next = __builtin_amdgcn_readfirstlane(l_chunk[0]), end = __builtin_amdgcn_readfirstlane(l_chunk[1]);
        if (end == 0u && next < kFlagChunkAfter) {          // a wave's first few: exactly the slots they need
            slot = flag_reserve(consts_lds, pool_lds, total_work, rank, lanes) + (uint32_t)rank;
            if (rank == 0) l_chunk[0] = next + lanes;
        } else {
            const uint32_t room = end != 0u ? end - next : 0u;
            if (lanes <= room) {
                slot = next + (uint32_t)rank;
                if (rank == 0) l_chunk[0] = next + lanes;
            } else {                                        // the old chunk's last slots, then the first of a new one
                const uint32_t base = flag_reserve(consts_lds, pool_lds, total_work, rank, kFlagChunk);
                slot = (uint32_t)rank < room ? next + (uint32_t)rank : base + ((uint32_t)rank - room);
                if (rank == 0) { l_chunk[0] = base + (lanes - room); l_chunk[1] = base + kFlagChunk; }
            }
        }
    }
    if (slot < lds_s32(consts_lds + 16u * 10u + 8u)) lds_sptr(consts_lds + 16u * 8u)[slot] = w_flagged;
    // … and its pixel to the second accumulate launch
    uint32_t *dirty = lds_sptr(consts_lds + 16u * 9u);
    if (dirty) dirty[div_magic_v(w_flagged, lds_s32(consts_lds + 16u * 6u), lds_s32(consts_lds + 16u * 6u + 4u))] = 1u;
}
// end of the kernel, all lanes: the slots of the wave's last chunk nobody filled
__device__ __forceinline__ void flag_chunk_drain(uint32_t consts_lds, uint32_t chunk_lds, uint32_t wave, int lane) {
    const uint32_t words = *(lds_cu1 *)(uintptr_t)(consts_lds + 16u * 11u + 12u) & 255u;
    if (words == 0u) return;
    lds_chunk_word *l_chunk = flag_chunk_of(chunk_lds, words, wave);
    const uint32_t next = __builtin_amdgcn_readfirstlane(l_chunk[0]), end = __builtin_amdgcn_readfirstlane(l_chunk[1]);
    if (end == 0u || next >= end) return;
    const uint32_t slot = next + (uint32_t)lane;
    if (slot < end && slot < lds_s32(consts_lds + 16u * 10u + 8u)) lds_sptr(consts_lds + 16u * 8u)[slot] = kFlagHole;
    if (lane == 0) atomicAdd(lds_sptr(consts_lds + 16u * 8u + 8u) + kFlagHolesWords, end - next);
}

// ---- resume table ---------------------------------------------------------------------------------------------------------
// The exact walk used to redo a flagged sample from its camera ray — but everything up to the ray that was flagged is the same
// in both walks (an unflagged ray's closest hit IS hit_bvh's), and the lane still holds that ray and the path's state as they were
// when the ray was armed: the flag ends the path before the shade step changes anything.  The retiring lane leaves them in a
// direct-mapped table (slot = hash of the work index, claimed with one compare-and-swap on the tag: a slot already taken means
// this sample is redone from the camera, as before), and the exact re-walk of the LIST resumes from there: the launch ends with its
// longest path, and a path flagged at a random bounce has half its bounces behind it.  (A flag raised inside the shade step —
// the Schlick window — comes after random draws: kNoResumeBit, restart.)
__device__ __forceinline__ uint32_t resume_slot(uint32_t w, uint32_t shift) { return (w * 0x9E3779B1u) >> shift; }
__device__ __forceinline__ void resume_save(const KParams &P, uint32_t w, const Lane &L) {
    const uint32_t slot = resume_slot(w, P.resume_shift);
    if (atomicCAS(&P.resume_tag[slot], 0u, w + 1u) != 0u) return;
    float4 *st = P.resume_state + 4 * (size_t)slot;
    st[0] = make_float4(L.o.x, L.o.y, L.o.z, L.d.x);
    st[1] = make_float4(L.d.y, L.d.z, L.beta.x, L.beta.y);
    st[2] = make_float4(L.beta.z, L.color.x, L.color.y, L.color.z);
    st[3] = make_float4(__uint_as_float(L.seed), __int_as_float(L.depth & (kNoResumeBit - 1)), 0.0f, 0.0f);
}
__device__ __forceinline__ bool resume_load(const KParams &P, uint32_t w, Lane &L, f3 &ray_o, f3 &ray_d) {
    const uint32_t slot = resume_slot(w, P.resume_shift);
    if (P.resume_tag[slot] != w + 1u) return false;
    const float4 *st = P.resume_state + 4 * (size_t)slot;
    const float4 a = st[0], b = st[1], c = st[2], d = st[3];
    ray_o = mk(a.x, a.y, a.z);
    ray_d = mk(a.w, b.x, b.y);
    L.beta = mk(b.z, b.w, c.x);
    L.color = mk(c.y, c.z, c.w);
    L.seed = __float_as_uint(d.x);
    L.depth = __float_as_int(d.y);
    return true;
}

// ---- the render kernel ---------------------------------------------------------------------------
// kLds: traversal tables staged in LDS (else read through L1/L2).
// kThreaded: reference-order traversal of the caller's tree (bit-exact with the reference also
// where its result depends on visit order); else near-first traversal of the SAH child-pair tree.
// kDyn: guarded walk with distance-aware margins (step_pair_par), kWide: on the 4-wide nodes (step_wide_par).  Without them the
// LDS-resident guarded walk is the octant walk (step_octant).
// kSimple: the sphere-only specialisation of the octant walk (above, kSimpleBlock).
constexpr uint32_t kShortListLanes = 8;      // exact re-walk: up to this many paths per wave count as a short list (below)
// The trace kernels' body is one text, rt_render_body.inc, included by each; RTP_CAMERA_START is how it starts a sample's path.
//
// The headline kernel, render_kernel<true, false, false, false, true, true> — the sphere-only octant walk fed by the primary pass — is
// built for a scene in which nothing emits (kDark; rt_scene_create: no material with an `emit` bit pattern other than +0, no albedo
// beyond 1).  There the radiance a path carries is +0 from its camera ray until the ray that leaves the scene, so the lane holds no
// Lane::color: a retired sample is (+0) + beta * background or +0, and a flagged one leaves zeros in the resume table (the exact
// re-walk, not specialised, reads them back as ever).  RTP_BODY_CARRY: the three registers hold the ray's own constants of the sphere
// test instead (ray_const: |d|^2 and the fp64 reciprocal with its Newton steps, which test_sphere remakes for each of a ray's 2.9
// tests) — made once where the ray is armed.  A scene of that shape WITH emitters, or rt_config.dark_kernel = -1, takes render_emit_kernel
// below: the same instantiation without kDark, instruction for instruction what the headline kernel was before.  (The name of the
// headline kernel stays with the kernel the headline scene runs: profiles, tools and tests know it by that name.)
#ifndef RTP_DARK_CARRY
#define RTP_DARK_CARRY 1        /* 0: kDark without the carried constants (the A/B of docs/LOG.md round 32) */
#endif
template <bool kLds, bool kThreaded, bool kDyn = false, bool kWide = false, bool kSimple = false, bool kPrim = false>
__global__ void __launch_bounds__(kSimple ? kSimpleBlock : RTP_BLOCK, kSimple ? kSimpleWaves : RTP_MIN_WAVES) render_kernel(const KParams P) {
    constexpr bool kDark = false;
#define RTP_BODY_CARRY 0
#define RTP_CAMERA_START(L_, P_, i_, j_, base_, s_, o_, d_, lds_) start_sample<kConsts>(L_, P_, i_, j_, base_, s_, o_, d_, lds_)
#include "rt_render_body.inc"
#undef RTP_CAMERA_START
#undef RTP_BODY_CARRY
}
// (the headline kernel: an explicit specialisation, so that the lines of the body only it compiles — RTP_BODY_CARRY — are its own)
template <>
__global__ void __launch_bounds__(kSimpleBlock, kSimpleWaves) render_kernel<true, false, false, false, true, true>(const KParams P) {
    constexpr bool kLds = true, kThreaded = false, kDyn = false, kWide = false, kSimple = true, kPrim = true;
    constexpr bool kDark = true;
#define RTP_BODY_CARRY RTP_DARK_CARRY
#define RTP_CAMERA_START(L_, P_, i_, j_, base_, s_, o_, d_, lds_) start_sample<kConsts>(L_, P_, i_, j_, base_, s_, o_, d_, lds_)
#include "rt_render_body.inc"
#undef RTP_CAMERA_START
#undef RTP_BODY_CARRY
}
__global__ void __launch_bounds__(kSimpleBlock, kSimpleWaves) render_emit_kernel(const KParams P) {
    constexpr bool kLds = true, kThreaded = false, kDyn = false, kWide = false, kSimple = true, kPrim = true;
    constexpr bool kDark = false;
#define RTP_BODY_CARRY 0
#define RTP_CAMERA_START(L_, P_, i_, j_, base_, s_, o_, d_, lds_) start_sample<kConsts>(L_, P_, i_, j_, base_, s_, o_, d_, lds_)
#include "rt_render_body.inc"
#undef RTP_CAMERA_START
#undef RTP_BODY_CARRY
}
// Lens frames (rt_render_lens): the general builds of every walk, every sample started from its camera by lens_camera_ray.  The
// camera pair rides in a kernel argument of its own (scalar loads into SGPRs); the pinhole kernels' argument stays what it was.
template <bool kLds, bool kThreaded, bool kDyn = false, bool kWide = false>
__global__ void __launch_bounds__(RTP_BLOCK, RTP_MIN_WAVES) render_lens_kernel(const KParams P, const LensCam C) {
    constexpr bool kSimple = false, kPrim = false;        // (no sphere-only build, no candidate lists)
    constexpr bool kDark = false;
#define RTP_BODY_CARRY 0
#define RTP_CAMERA_START(L_, P_, i_, j_, base_, s_, o_, d_, lds_) lens_camera_ray(L_, C, i_, j_, sample_seed1(base_, s_), o_, d_)
#include "rt_render_body.inc"
#undef RTP_CAMERA_START
#undef RTP_BODY_CARRY
}

// ---- probe kernel: one lane traces one (i, j, s) sample with the exact walk's step functions -------
__global__ void __launch_bounds__(256) probe_kernel(const KParams P) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P.probe_n) return;
    const int32_t i = P.probe_ijs[3 * g], j = P.probe_ijs[3 * g + 1], s = P.probe_ijs[3 * g + 2];
    Lane L;
    const uint32_t base_seed = wang_hash((uint32_t)i * (uint32_t)P.width + (uint32_t)j);
    f3 ray_o, ray_d;
    start_sample(L, P, i, j, base_seed, s, ray_o, ray_d);
    begin_ray(L, ray_o, ray_d, 0);
    int32_t rays = 0;
    if (P.max_depth > 0) {
        for (;;) {
            rays++;
            while (!traversal_finished<true>(L, kBlocked)) {
                if (L.sp != 0) leaf_threaded(L, P.spheres, P.planes);
                else step_threaded(L, P.tnodes, P.num_tnodes);
            }
            if (!shade(L, P, P.spheres, P.planes, P.materials, P.sphere_mat, ray_o, ray_d)) break;
            begin_ray(L, ray_o, ray_d, 0);
        }
    }
    P.probe_rad[3 * g] = L.color.x; P.probe_rad[3 * g + 1] = L.color.y; P.probe_rad[3 * g + 2] = L.color.z;
    P.probe_rays[g] = rays;
    P.probe_seed[g] = L.seed;
}

// ---- lens probe (rt_lens_camera_rays): the camera ray of n (i, j, s) samples and the RNG state after the camera's draws ----
__global__ void __launch_bounds__(256) lens_ray_kernel(const LensCam C, const int32_t *ijs, int32_t n, float *org, float *dir, uint32_t *seed_out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const int32_t i = ijs[3 * g], j = ijs[3 * g + 1], s = ijs[3 * g + 2];
    Lane L;
    f3 o, d;
    lens_camera_ray(L, C, i, j, sample_seed1(wang_hash((uint32_t)i * (uint32_t)C.width + (uint32_t)j), s), o, d);
    org[3 * g] = o.x; org[3 * g + 1] = o.y; org[3 * g + 2] = o.z;
    dir[3 * g] = d.x; dir[3 * g + 1] = d.y; dir[3 * g + 2] = d.z;
    seed_out[g] = L.seed;
}

// ---- ray probe: hit_scene for arbitrary rays (rt_closest_hits), exact walk ---------------------------
__global__ void __launch_bounds__(256) closest_hit_kernel(const KParams P, const float *org, const float *dir, int32_t n,
                                                          int32_t *hit, float *t, int32_t *prim) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    Lane L;
    begin_ray(L, mk(org[3 * g], org[3 * g + 1], org[3 * g + 2]), mk(dir[3 * g], dir[3 * g + 1], dir[3 * g + 2]), 0);
    while (!traversal_finished<true>(L, kBlocked)) {
        if (L.sp != 0) leaf_threaded(L, P.spheres, P.planes);
        else step_threaded(L, P.tnodes, P.num_tnodes);
    }
    hit[g] = L.hit >= 0 ? 1 : 0;
    if (L.hit >= 0) { t[g] = L.closest; prim[g] = L.hit; }
}

// ---- pixels with a flagged sample: marks → list ---------------------------------------------------------------------------
// The trace kernel only MARKS the pixel of a flagged sample (a plain store; it used to append it as well, with an exchange per
// sample and an atomic on the list's one counter per pixel).  This kernel, between the trace launch and the second accumulate
// launch, lists the marked pixels: one atomic per workgroup.  The order of the list means nothing.
constexpr int kDirtyBlock = 256;              // threads per workgroup …
constexpr int kDirtyPixels = 4 * kDirtyBlock;  // … of four consecutive pixels each (one 16-byte load of marks)
__global__ void __launch_bounds__(kDirtyBlock) dirty_compact_kernel(const uint32_t *dirty, uint32_t num_pixels, uint32_t *list, uint32_t *count) {
    __shared__ uint32_t wave_total[kDirtyBlock / kWave], block_base;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t q0 = (blockIdx.x * (uint32_t)kDirtyBlock + threadIdx.x) * 4u;
    uint32_t mark[4] = {0u, 0u, 0u, 0u};
    if (q0 + 3u < num_pixels) {
        const uint4 v = *reinterpret_cast<const uint4 *>(dirty + q0);
        mark[0] = v.x; mark[1] = v.y; mark[2] = v.z; mark[3] = v.w;
    } else {
        for (int j = 0; j < 4; ++j) if (q0 + (uint32_t)j < num_pixels) mark[j] = dirty[q0 + (uint32_t)j];
    }
    // position of each marked pixel among the wave's: slot by slot (the order of the list means nothing)
    uint32_t at[4], total = 0;
    for (int j = 0; j < 4; ++j) {
        const uint64_t m = __ballot(mark[j] != 0u);
        at[j] = total + (uint32_t)lane_rank(m);
        total += (uint32_t)__popcll(m);
    }
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kDirtyBlock / kWave; ++w) { const uint32_t n = wave_total[w]; wave_total[w] = sum; sum += n; }
        block_base = sum ? atomicAdd(count, sum) : 0u;
    }
    __syncthreads();
    const uint32_t base = block_base + wave_total[wave];
    for (int j = 0; j < 4; ++j) if (mark[j] != 0u) list[base + at[j]] = q0 + (uint32_t)j;
}

// ---- in-order accumulation: framebuffer[pixel] += the pass's samples, one after the other -------------
// The reference adds ray_color results to pixel_color in sample order (src/camera.cu:27-31); float
// addition is not associative, so the same order is kept here: one lane owns one pixel and adds
// the slab's samples s = first, first+1, ... onto the running sum left by the previous pass.
// The slab is pixel-major (store_sample): a wave takes 64 consecutive pixels and walks their rows 16 slots at a
// time — the 64 x 192-byte segments of a tile are fetched with 16-byte loads (consecutive lanes, consecutive
// addresses within a row), transposed through LDS (row stride 52 floats: aligned and conflict-free for b128 both ways),
// and each lane then reads ITS pixel's 16 samples and adds them in order.
constexpr int kAccSlots = 16;                 // slots per tile (192 bytes of a row; rows start on 128-byte lines: pitch % 32 == 0).  Measured per
                                              // 12.4 GB pass: 16 slots x 4 waves per block 2.96 ms; 8 x 4: 3.63; 32 x 2: 4.97
constexpr int kAccRow = kAccSlots * 3 + 4;    // floats per pixel row of the LDS tile (stride 52: aligned and conflict-free for b128 both ways)
constexpr int kAccWaves = 4;                  // waves per block (13 KB of LDS each)
// Overlap with the exact re-walk (rt_capi.hip): launched with `dirty` it leaves the pixels marked there alone — their rows
// are still being rewritten — and a second launch, after the re-walk, takes its pixels from `list` (kList).
template <bool kList = false>
__global__ void __launch_bounds__(kAccWaves * 64) accumulate_kernel(float *fb, const float *slab, uint32_t num_pixels, uint32_t pitch, int32_t count,
                                                                   int32_t first_pass, uint32_t *dirty = nullptr, const uint32_t *list = nullptr,
                                                                   const uint32_t *list_count = nullptr, const uint32_t *cand = nullptr, uint32_t cand_stride = 0,
                                                                   float bg_r = 0.0f, float bg_g = 0.0f, float bg_b = 0.0f,
                                                                   const uint32_t *abandon = nullptr, uint32_t run_if_abandoned = 0u) {
    __shared__ float4 tile4[kAccWaves][64 * kAccRow / 4];
    // A guarded pass that gave up part-way (render_kernel, flag_write) leaves rows nobody traced: the two launches that run BESIDE
    // the exact re-walk stand down (run_if_abandoned = 0) and a third one, after it, sums every pixel (run_if_abandoned = 1).
    if (abandon != nullptr && (*abandon != 0u) != (run_if_abandoned != 0u)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t pg = (blockIdx.x * (uint32_t)kAccWaves + (uint32_t)wave) * 64u;          // first pixel (kList: first list entry) of this wave
    if (kList) num_pixels = *list_count;
    if (pg >= num_pixels) return;
    if (kList) {
        // Pixels from the list: each lane walks its own pixel's row with 16-byte loads (a tenth of the slab at most, and
        // the list is short: no transpose).  Four samples = three loads.
        const bool on = pg + (uint32_t)lane < num_pixels;
        if (!on) return;
        const uint32_t q = list[pg + (uint32_t)lane];      // (the marks stay: the other launch may still be reading them; rt_render clears them before the next pass)
        f3 sum = mk(0.0f, 0.0f, 0.0f);
        if (!first_pass) sum = mk(fb[3 * (size_t)q], fb[3 * (size_t)q + 1], fb[3 * (size_t)q + 2]);
        const float *row = slab + (size_t)q * pitch * 3;
        int32_t s = 0;
        for (; s + 4 <= count; s += 4) {
            const float4 a = *reinterpret_cast<const float4 *>(row + 3 * s), b = *reinterpret_cast<const float4 *>(row + 3 * s + 4),
                         c = *reinterpret_cast<const float4 *>(row + 3 * s + 8);
            sum = add(sum, mk(a.x, a.y, a.z));
            sum = add(sum, mk(a.w, b.x, b.y));
            sum = add(sum, mk(b.z, b.w, c.x));
            sum = add(sum, mk(c.y, c.z, c.w));
        }
        for (; s < count; ++s) sum = add(sum, mk(row[3 * s], row[3 * s + 1], row[3 * s + 2]));
        fb[3 * (size_t)q] = sum.x; fb[3 * (size_t)q + 1] = sum.y; fb[3 * (size_t)q + 2] = sum.z;
        return;
    }
    const uint32_t q = pg + (uint32_t)lane;
    const bool valid = q < num_pixels && !(dirty && dirty[q < num_pixels ? q : 0u] != 0u);
    float *tile = reinterpret_cast<float *>(tile4[wave]);
    f3 sum = mk(0.0f, 0.0f, 0.0f);
    if (valid && !first_pass) sum = mk(fb[3 * (size_t)q], fb[3 * (size_t)q + 1], fb[3 * (size_t)q + 2]);
    const uint32_t npix = num_pixels - pg < 64u ? num_pixels - pg : 64u;
    // Sky pixels (no candidate leaf, rt_primary.hip.inc): every sample of theirs is 0 + 1 * background (src/camera.cu:222-229)
    // — nobody wrote their rows and nobody reads them; the same `count` additions, in the same order, from a register.
    const bool sky = cand != nullptr && q < num_pixels && cand[(size_t)q * cand_stride] == 0u;
    const f3 sky_sample = add(mk(0.0f, 0.0f, 0.0f), mul(mk(1.0f, 1.0f, 1.0f), mk(bg_r, bg_g, bg_b)));
    const f3 first_sum = sum;
    auto sky_sum = [&]() { f3 t = first_sum; for (int32_t s = 0; s < count; ++s) t = add(t, sky_sample); return t; };
    if (cand != nullptr && __ballot(sky) == __ballot(q < num_pixels)) {        // a wave of nothing but sky
        if (valid) { const f3 t = sky_sum(); fb[3 * (size_t)q] = t.x; fb[3 * (size_t)q + 1] = t.y; fb[3 * (size_t)q + 2] = t.z; }
        return;
    }
    if (npix == 64u && (pitch % kAccSlots) == 0u) {
        // Full wave, whole tiles: the loads of tile t+1 are in flight (in registers) while tile t is summed out of LDS.
        // One load instruction covers 5 pixels x 12 float4 (lanes 0..59: 192 contiguous bytes per pixel); 13 of them cover
        // the 64 pixels (the last one 4), so instruction j reads at lane-constant offsets from row 5j — one address per
        // lane, scalar strides, nothing indexed at run time.
        constexpr int kF4 = kAccSlots * 3 / 4;            // 12 float4 per pixel and tile
        constexpr int kPer = 64 / kF4;                    // 5 pixels per load instruction
        constexpr int kLoads = (64 + kPer - 1) / kPer;    // 13
        const uint32_t lp = (uint32_t)lane / (uint32_t)kF4, lf = (uint32_t)lane - lp * (uint32_t)kF4;
        const bool on = lp < (uint32_t)kPer;              // lanes 60..63 sit out
        // (every lane loads — lanes 60..63 and the rows past the 64th re-read a valid address — so that the values stay in
        // registers; only the LDS writes are masked)
        const uint32_t lpc = on ? lp : 0u;
        const float *src = slab + (size_t)(pg + lpc) * pitch * 3 + lf * 4u;
        float *dst = tile + lp * kAccRow + lf * 4u;
        const size_t row_stride = (size_t)kPer * pitch * 3;          // floats between the rows of consecutive instructions
        const size_t last_stride = lpc + (uint32_t)((kLoads - 1) * kPer) < 64u ? (size_t)(kLoads - 1) * row_stride : 0;
        typedef float f4n __attribute__((ext_vector_type(4)));       // (a native vector: the HIP float4 struct array stayed in scratch)
        f4n v[kLoads];
#pragma unroll
        for (int j = 0; j < kLoads; ++j) v[j] = *reinterpret_cast<const f4n *>(src + (j == kLoads - 1 ? last_stride : (size_t)j * row_stride));
        for (uint32_t s0 = 0; s0 < (uint32_t)count; s0 += kAccSlots) {
#pragma unroll
            for (int j = 0; j < kLoads; ++j)
                if (on && (uint32_t)(j * kPer) + lp < 64u) *reinterpret_cast<f4n *>(dst + j * kPer * kAccRow) = v[j];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            if (s0 + kAccSlots < (uint32_t)count) {
                const float *nxt = src + (size_t)(s0 + kAccSlots) * 3;
#pragma unroll
                for (int j = 0; j < kLoads; ++j) v[j] = *reinterpret_cast<const f4n *>(nxt + (j == kLoads - 1 ? last_stride : (size_t)j * row_stride));
            }
            const uint32_t nv = (uint32_t)count - s0 < (uint32_t)kAccSlots ? (uint32_t)count - s0 : (uint32_t)kAccSlots;
            const float *row = tile + lane * kAccRow;
            uint32_t s = 0;
            for (; s + 4 <= nv; s += 4) {
                const float4 a = *reinterpret_cast<const float4 *>(row + 3 * s), b = *reinterpret_cast<const float4 *>(row + 3 * s + 4),
                             c = *reinterpret_cast<const float4 *>(row + 3 * s + 8);
                sum = add(sum, mk(a.x, a.y, a.z));
                sum = add(sum, mk(a.w, b.x, b.y));
                sum = add(sum, mk(b.z, b.w, c.x));
                sum = add(sum, mk(c.y, c.z, c.w));
            }
            for (; s < nv; ++s) sum = add(sum, mk(row[3 * s], row[3 * s + 1], row[3 * s + 2]));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
        if (sky) sum = sky_sum();        // (its row holds nothing)
        if (valid) { fb[3 * (size_t)q] = sum.x; fb[3 * (size_t)q + 1] = sum.y; fb[3 * (size_t)q + 2] = sum.z; }      // (not valid: a pixel left to the list launch)
        return;
    }
    for (uint32_t s0 = 0; s0 < (uint32_t)count; s0 += kAccSlots) {
        const uint32_t ns = pitch - s0 < (uint32_t)kAccSlots ? pitch - s0 : (uint32_t)kAccSlots;      // slots of this tile (padding included: multiple of 4)
        const uint32_t seg4 = ns * 3u / 4u;                                                           // float4s per pixel segment
        const uint32_t total4 = npix * seg4;
        for (uint32_t k = (uint32_t)lane; k < total4; k += 64u) {
            const uint32_t pl = k / seg4, f4 = k - pl * seg4;
            const float4 v = *reinterpret_cast<const float4 *>(slab + ((size_t)(pg + pl) * pitch + s0) * 3 + f4 * 4u);
            *reinterpret_cast<float4 *>(tile + pl * kAccRow + f4 * 4u) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       // the tile is this wave's own: wait for its LDS writes, no barrier
        const uint32_t nv = (uint32_t)count - s0 < (uint32_t)kAccSlots ? (uint32_t)count - s0 : (uint32_t)kAccSlots;   // real samples in the tile
        if (valid) {
            const float *row = tile + lane * kAccRow;
            uint32_t s = 0;
            for (; s + 4 <= nv; s += 4) {        // four samples = three aligned 16-byte LDS reads
                const float4 a = *reinterpret_cast<const float4 *>(row + 3 * s), b = *reinterpret_cast<const float4 *>(row + 3 * s + 4),
                             c = *reinterpret_cast<const float4 *>(row + 3 * s + 8);
                sum = add(sum, mk(a.x, a.y, a.z));
                sum = add(sum, mk(a.w, b.x, b.y));
                sum = add(sum, mk(b.z, b.w, c.x));
                sum = add(sum, mk(c.y, c.z, c.w));
            }
            for (; s < nv; ++s) sum = add(sum, mk(row[3 * s], row[3 * s + 1], row[3 * s + 2]));
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       // reads done before the next tile overwrites
    }
    if (sky) sum = sky_sum();
    if (valid) { fb[3 * (size_t)q] = sum.x; fb[3 * (size_t)q + 1] = sum.y; fb[3 * (size_t)q + 2] = sum.z; }
}

// ---- saver arithmetic on the device ("next" row f1) -------------------------------------------------
__global__ void tonemap_kernel(const float *fb, uint8_t *out, int64_t n, float inv_divisor) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < n; k += stride) out[k] = tonemap_u8(fb[k], inv_divisor);
}

}  // namespace rtk
