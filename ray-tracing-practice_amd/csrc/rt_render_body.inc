// rt_render_body.inc — the body of the trace kernels (included by rt_kernel.hip.inc, inside render_kernel and render_lens_kernel).
//
// One text for both, so that the pinhole kernels compile to exactly the code they did before lens frames existed: each kernel defines
// RTP_CAMERA_START, how a sample's camera ray is made from (lane, params, i, j, base seed, sample, out origin, out direction, LDS
// constants), before including this file, and RTP_BODY_CARRY (0, or 1: the lane keeps its ray's sphere-test constants, which only the
// headline kernel's build for scenes without emitters does: kDark) — text the other kernels do not compile at all, since even two
// unused variables that a lambda captures moved registers about in their listings.
    static_assert(!kPrim || !kThreaded, "primary visibility feeds the guarded walk");
    static_assert(!kDark || (kLds && !kThreaded && !kDyn && !kWide && kSimple && kPrim), "the kernel of scenes without emitters is a variant of the sphere-only octant walk fed by the primary pass");
    static_assert(!RTP_BODY_CARRY || kDark, "the ray's constants take the registers of Lane::color");
    constexpr int kBlock = kSimple ? kSimpleBlock : rtk::kBlock;      // (shadows the namespace constant inside this kernel)
    static_assert(!kWide || kDyn, "the 4-wide nodes are walked only with distance-aware margins (step_wide_par)");
    static_assert(!kSimple || (kLds && !kDyn && !kWide) || (!kLds && !kThreaded && kDyn && !kWide),
                  "kSimple is a variant of the LDS-resident walks — the octant walk, and the exact walk — and of the pair walk through L1 / L2 (step_pair_par)");
    extern __shared__ float4 smem[];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    constexpr bool kGuard = !kThreaded;                  // the near-first walk always runs guarded

    // work indices: [0, total_work), or the entries of a list (exact re-walk of flagged samples; a
    // list that overflowed its capacity means "every sample")
    const uint32_t *work_list = kThreaded ? P.work_list : nullptr;        // (only the exact re-walk is ever launched on a list)
    uint32_t total_work = P.total_work;
    if (work_list) {
        const uint32_t listed = *P.work_count;
        // (a list that overflowed, or a guarded pass that gave up part-way: every sample of the pass)
        if (listed > P.work_cap || (P.abandon != nullptr && *P.abandon != 0u)) work_list = nullptr;
        else total_work = listed;
    }
    if (kPrim) total_work = *P.traced_pixels * (uint32_t)P.pass_count;       // sky pixels are not this kernel's
    if (total_work == 0) return;

    const bool kTreelet = !kLds && kThreaded;          // big scene, exact walk: only the top of the tree lives in LDS
    const bool kTopPairs = !kLds && !kThreaded;        // big scene, guarded walk: likewise
    constexpr bool kOct = kLds && !kThreaded;               // every LDS-resident guarded walk is the octant walk (step_octant)
    constexpr bool kOctT = kThreaded && kLds && kSimple;          // exact walk, sphere-only build: octant-addressed node records (step_threaded_oct)
    static_assert(!kDyn || (!kLds && !kThreaded), "scenes with distance-aware margins walk through L1 / L2 (step_pair_par, step_wide_par)");
    constexpr bool kDynPair = kDyn && !kWide;              // distance-aware margins on pair nodes: step_pair_par
    constexpr bool kWidePar = kDyn && kWide;               // … on 4-wide nodes: step_wide_par
    constexpr bool kSent = kOct || kDyn;                   // the lane's stack with a sentinel at level 0 and a byte-offset stack pointer (pop<true>)
    constexpr bool kDynPar = kDyn;                         // the growth of the boxes in parametric form, two per-ray rows behind the lane's stack
    // step_pair_par: the last two rows of the lane's stack column hold the ray's own growth bound and sqrt(k) |d|
    const int32_t walk_levels = kDynPar ? P.stack_levels - 2 : P.stack_levels;
    const DynPar dyn_par = {P.g_dyn_b, P.g_dyn_c3, walk_levels * kLevelBytes, walk_levels * kLevelBytes + kLevelBytes};
    const int n_node4 = kLds ? (kThreaded ? (P.num_tnodes + 1) * (kOctT ? 4 : 2) : P.num_internal * (kOct ? 5 : 4))     // + the end sentinel
                             : P.num_top * 2;
    const int n_sph4 = kLds ? P.num_spheres : 0;
    const int n_pl4 = kLds ? P.num_planes * 5 : 0;
    const int n_mat4 = (kLds && !kSimple) ? P.num_materials * RTP_LDS_MAT_ROWS : 0;      // kSimple: every material row from global memory
    const int n_smat4 = kLds ? (P.num_spheres + 3) / 4 : 0;
    float4 *l_nodes = smem;
    // LDS address of the pair table (step_octant keeps node ADDRESSES in L.node and in the links)
    const int32_t oct_base = (int32_t)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4 *)l_nodes;
    float4 *l_spheres = smem + n_node4;
    float4 *l_planes = l_spheres + n_sph4;
    float4 *l_mats = l_planes + n_pl4;
    int32_t *l_smat = reinterpret_cast<int32_t *>(l_mats + n_mat4);
    uint32_t *l_stack = reinterpret_cast<uint32_t *>(l_mats + n_mat4 + n_smat4) + wave * (P.stack_levels * kWave) + lane;
    // (an LDS pointer by type: as a volatile generic pointer these four accesses were flat_load/flat_store sc0 sc1, each
    // followed by s_waitcnt vmcnt(0) lgkmcnt(0))
    typedef __attribute__((address_space(3))) volatile uint32_t lds_word;
    lds_word *l_pool = (lds_word *)(reinterpret_cast<uint32_t *>(l_mats + n_mat4 + n_smat4) + (kBlock / kWave) * (P.stack_levels * kWave) + wave * 2);
    if (lane == 0) { l_pool[0] = 0; l_pool[1] = 0; }      // empty range
    // (the ranges of all waves of the workgroup as 64-bit words, next | end << 32.  Indices are taken with ONE atomic add of the
    // number wanted — by the owner, and once the pass has run dry by the other waves: the sum's old value says what was there;
    // an add on an empty range only pushes next further past end, and the owner's refill overwrites it.  Work indices stay
    // below 2^31 (rt_render checks), so next never carries into end.)
    typedef __attribute__((address_space(3))) uint64_t lds_u64;
    lds_u64 *l_pool64 = (lds_u64 *)(l_pool - wave * 2);
    constexpr uint32_t kPoolDry = 0x80000000u;            // next >= this with end == 0: the owner has seen the pass's counter beyond the last sample
    auto pool_take = [&](int j, uint32_t n, uint32_t &next, uint32_t &end) -> bool {      // one lane: up to n indices of wave j's range
        const uint64_t old = __hip_atomic_fetch_add(&l_pool64[j], (uint64_t)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        next = (uint32_t)old;
        end = (uint32_t)(old >> 32);
        return next < end;
    };
    // guarded builds: a block of rarely used launch constants behind the work ranges (write_consts)
    const uint32_t consts_lds = (uint32_t)(uintptr_t)(lds_word *)(reinterpret_cast<uint32_t *>(l_mats + n_mat4 + n_smat4) + (kBlock / kWave) * (P.stack_levels * kWave) + (kBlock / kWave) * 2);
    constexpr bool kConsts = !kThreaded || kSimple;      // every guarded build keeps the constants block, and the 64-register build of the exact walk
    if (kConsts) write_consts(P, consts_lds, tid);
    if (kSent) l_stack[0] = (uint32_t)kDone;              // level 0 of every lane's stack: the sentinel of pop<true>
    const float4 *g_nodes = kThreaded ? P.tnodes : (kWide ? P.whnodes : (kLds ? P.nodes : P.hnodes));
    if (kTreelet || kTopPairs) {
        const float4 *src = kTreelet ? P.xnodes : P.hnodes;
        for (int k = tid; k < n_node4; k += kBlock) l_nodes[k] = src[k];
        __syncthreads();
    }
    if (kLds) {
        if (kOctT) {
            // threaded records (lo.x hi.x lo.y hi.y | lo.z hi.z skip leaf) → the 64-byte octant layout of step_threaded_oct
            for (int k = tid; k <= P.num_tnodes; k += kBlock) {
                const float4 A = g_nodes[2 * k + 0], B = g_nodes[2 * k + 1];
                l_nodes[4 * k + 0] = make_float4(A.x, A.y, A.y, A.x);
                l_nodes[4 * k + 1] = make_float4(A.z, A.w, A.w, A.z);
                l_nodes[4 * k + 2] = make_float4(B.x, B.y, B.y, B.x);
                l_nodes[4 * k + 3] = make_float4(B.z, B.w, 0.0f, 0.0f);
            }
        } else if (kOct) {
            // 64-byte pair records (lo0 xyz, hi0 xyz, lo1 xyz, hi1 xyz, code0, code1) → the 80-byte octant layout of
            // step_octant; links to inner nodes become byte offsets
            for (int k = tid; k < P.num_internal; k += kBlock) {
                const float4 A = g_nodes[4 * k + 0], B = g_nodes[4 * k + 1], C = g_nodes[4 * k + 2], D = g_nodes[4 * k + 3];
                const int32_t c0 = as_int(D.x), c1 = as_int(D.y);
                const float l0 = __int_as_float(c0 >= 0 ? oct_base + c0 * kOctNodeBytes : c0), l1 = __int_as_float(c1 >= 0 ? oct_base + c1 * kOctNodeBytes : c1);
                l_nodes[5 * k + 0] = make_float4(A.x, B.z, A.w, C.y);      // x: lo0 lo1 hi0 hi1
                l_nodes[5 * k + 1] = make_float4(A.x, B.z, A.y, B.w);      // x: lo0 lo1 | y: lo0 lo1
                l_nodes[5 * k + 2] = make_float4(B.x, C.z, A.y, B.w);      // y: hi0 hi1 lo0 lo1
                l_nodes[5 * k + 3] = make_float4(A.z, C.x, B.y, C.w);      // z: lo0 lo1 hi0 hi1
                l_nodes[5 * k + 4] = make_float4(A.z, C.x, l0, l1);        // z: lo0 lo1 | codes
            }
        } else {
            for (int k = tid; k < n_node4; k += kBlock) l_nodes[k] = g_nodes[k];
        }
        for (int k = tid; k < n_sph4; k += kBlock) l_spheres[k] = P.spheres[k];
        for (int k = tid; k < n_pl4; k += kBlock) l_planes[k] = P.planes[k];
        for (int k = tid; k < n_mat4; k += kBlock)       // the first RTP_LDS_MAT_ROWS rows of each material
            l_mats[k] = P.materials[3 * (k / RTP_LDS_MAT_ROWS) + (k % RTP_LDS_MAT_ROWS)];
        for (int k = tid; k < P.num_spheres; k += kBlock) l_smat[k] = P.sphere_mat[k];
        __syncthreads();
    }
    const float4 *nodes = kLds ? l_nodes : g_nodes;
    const float4 *spheres = kLds ? l_spheres : P.spheres;
    const float4 *planes = kLds ? l_planes : P.planes;
    const float4 *materials = (kLds && !kSimple) ? l_mats : P.materials;
    const int32_t *sphere_mat = kLds ? l_smat : P.sphere_mat;
    // threaded: "walk finished / idle" is any negative node with no primitive pending
    const int32_t end_node = kThreaded ? kBlocked : kDone;
    const int32_t first_node = kThreaded ? 0 : (kWide ? P.wroot : (kOct && P.root >= 0 ? oct_base + P.root * kOctNodeBytes : P.root));

    Lane L;
    L.node = end_node; L.hit = -1; L.sp = 0; L.pend = 0; L.depth = 0; L.closest = 0; L.seed = 0; L.e = 0;
    L.o = L.d = L.inv = L.beta = L.color = mk(0, 0, 0);
#if RTP_BODY_CARRY
    // the constants of the lane's ray that every sphere test needs — |d|^2 and its fp64 reciprocal (ray_const) — made by arm_ray
    float ray_a = 0.0f;
    double ray_y = 0.0;
#endif
    constexpr bool kDefer = !kThreaded;        // parked primitive tests (guarded walk)
    // a lane with nothing left to walk goes to the shade step with its parked test still open: the step tests it first
    auto finished = [&]() { return kDefer ? (L.node == kDone) : traversal_finished<kThreaded>(L, end_node); };
    auto stuck_at_leaf = [&]() { return kDefer ? (L.pend != 0 && L.node < 0 && L.node != kDone) : wants_leaf<kThreaded>(L, end_node); };
#ifdef RTP_EXIT_HIST
    const uint64_t exit_hist_t0 = __builtin_amdgcn_s_memrealtime();
    uint32_t exit_hist_fetch = (uint32_t)exit_hist_t0, exit_hist_dead = (uint32_t)exit_hist_t0;       // when the lane took its last sample / found the pass dry
#endif
    bool alive = true;
    // Exact re-walk of a SHORT list: as few paths per wave as the grid allows.  The lanes of a wave shade together, so a
    // path shares every bounce with the slowest ray of its wave — and the launch ends with its longest path (tens of
    // bounces among the flagged samples of any frame).  Alone in its wave a path runs at its own pace: the re-walk of a
    // 400 x 225 x 16 frame's 248 samples took 0.73 ms with 64 paths per wave, 0.55 ms one per wave; 16 735 samples (1200 x 800 x
    // 100) 1.19 → 0.99 ms at three per wave.  A long list fills its waves as before (178 459 samples of the headline frame:
    // 1.2 ms in full waves, 2.2 ms at 29 per wave — twice the wave-steps for the same paths).
    bool short_list = false;
    if (kThreaded && work_list) {
        const uint32_t waves_total = gridDim.x * (uint32_t)(kBlock / kWave);
        const uint32_t per_wave = (total_work + waves_total - 1u) / waves_total;
        short_list = per_wave <= kShortListLanes;
        if (short_list && (uint32_t)lane >= per_wave) alive = false;
    }
    bool path_open = false;          // a sample is in flight
    uint32_t w_cur = 0;              // work index (pixel * pass_count + slot) of the sample in flight

#ifdef RTP_STATS
    uint32_t st_iters[4] = {0, 0, 0, 0}, st_lanes[4] = {0, 0, 0, 0};
    uint64_t st_cycles[7] = {0, 0, 0, 0, 0, 0, 0}, st_last = __builtin_amdgcn_s_memtime();
    uint32_t st_fetch_rounds = 0;          // kPrim: rounds of (A) in which some lane of the wave fetched (each traced sample is fetched once)
#endif
    // the flagged-sample list: flag_collect above, called where a sample is retired
    const uint32_t chunk_lds = consts_lds + 16u * (uint32_t)kConstRows;       // the flag stages: behind the constants block
    if (kConsts) flag_chunk_init(chunk_lds, P.flag_chunk_words, wave, lane);
    // ---- the parts of a SHADE step ----------------------------------------------------------------------------------
    // the value ray_color returns for the sample in flight → its slot of the slab; a flagged sample goes on the lists
    auto retire_sample = [&]() {
        store_sample<kConsts>(P, w_cur, L.color, consts_lds);
#ifdef RTP_STATS
#ifndef RTP_STATS_SHADE_SPLIT
        if (kGuard && (L.depth & kFlagBit)) for (int k = 0; k < 3; ++k) if (L.depth & RTP_WHY(k)) atomicAdd(&P.stats[12 + k], 1u);    // [15] is the abort word
#endif
#endif
        if (kGuard && (L.depth & kFlagBit)) {      // rare: hand the sample to the exact walk
            if (P.resume_tag != nullptr && !(L.depth & kNoResumeBit)) resume_save(P, w_cur, L);
            const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
            flag_collect(w_cur, consts_lds, chunk_lds, consts_lds - ((uint32_t)(kBlock / kWave) - wave_u) * 8u, wave_u, total_work);
        }
        path_open = false;
    };
    // the next sample of the wave's reservation → its camera ray (alive = false when the pass has run dry).  kPrim: also the
    // record the primary-visibility pass left in the sample's slot of the slab (closest-hit distance, code)
    auto fetch_sample = [&](f3 &ray_o, f3 &ray_d, float &prim_t, int32_t &prim_code) {
        while (alive && !path_open) {
            // Next sample.  Work index w = pixel * pass_count + slot: consecutive indices are the
            // samples of one pixel in this pass, so a wave that reserves 64 consecutive
            // indices traces one pixel's samples side by side (coherent primary rays).  The
            // reservation [next, end) lives in LDS (two dwords per wave): lanes that are not
            // in this loop right now must see the update the next time they come here.
            const uint64_t m = __ballot(1);
            const int rank = lane_rank(m);
            const uint32_t n = (uint32_t)__popcll(m);
            uint32_t pool_next = 0, pool_end = 0;
            if (rank == 0 && !pool_take(wave, n, pool_next, pool_end)) {
                // one atomic per `chunk` samples; near the end of the pass the reservations shrink
                // with what is left (guided self-scheduling: remaining / (2 x waves), in units of 64),
                // so the last waves do not sit on 512 samples while the others have run dry
                uint32_t want = P.chunk, taper = P.taper_shift;
                // (the exact re-walk of a WHOLE pass — list overflowed, guarded pass abandoned — reserves like a trace launch, not in
                // the 64s a short list wants: 44 M samples in reservations of 64 were 7 ms of atomics on a 1.8 ms frame)
                if (kThreaded && P.work_list != nullptr && work_list == nullptr) { want = P.full_chunk; taper = P.full_taper; }
                uint32_t *queue = P.queue;
                if (kConsts) {
                    const u4v c = ((lds_cuint4 *)(uintptr_t)consts_lds)[10], d = ((lds_cuint4 *)(uintptr_t)consts_lds)[11];
                    want = c.w; taper = d.z; queue = ptr_from(d.x, d.y);
                }
                const bool known_dry = pool_end == 0u && pool_next >= kPoolDry;
                constexpr uint32_t kWaves = (uint32_t)(kBlock / kWave);
                // (a guarded pass that has been given up — flag_write — has had its counter pushed beyond every work index: the
                // reservation below comes back dry, no word to poll)
                {
                if (!known_dry) {
                    const uint32_t left = total_work > pool_end ? total_work - pool_end : 0u;
                    const uint32_t share = (left >> taper) & ~63u;
                    if (share < want) want = share < 64u ? 64u : share;
                    if (kThreaded && short_list) want = n;      // exactly what the asking lanes take (a reservation of 64 would be one wave's for good)
                    pool_next = atomicAdd(queue, want);
                    pool_end = pool_next + want;
                }
                if (!known_dry && pool_next < total_work) {
                    l_pool64[wave] = (uint64_t)(pool_next + (n < want ? n : want)) | ((uint64_t)pool_end << 32);
                } else {
                    // The pass has run dry: what the other waves of the workgroup still hold is taken from them, one wave per
                    // round of this loop — 64 samples reserved by a wave whose lanes are all busy are a generation of paths
                    // that would start only as its own lanes come free, long after everyone else has left (wave exit times
                    // of a launch were spread over 1.5 ms).
                    // (which wave to ask is kept in the dry mark itself: the adds on a dry range — failed takes, n <= 64 each —
                    // leave the bits above 2^20 alone.  A wave that still has something is asked again next time; one that
                    // has nothing is passed for good: ranges only shrink once the pass is dry.)
                    const uint32_t ask = known_dry ? (pool_next - kPoolDry) >> 20 : 1u;       // 1 .. kWaves - 1; kWaves: every wave had nothing
                    const bool took = ask < kWaves && pool_take((int)(((uint32_t)wave + ask) % kWaves), n, pool_next, pool_end);
                    const uint32_t ask_next = took ? ask : (ask < kWaves ? ask + 1u : kWaves);
                    l_pool64[wave] = (uint64_t)(kPoolDry + (ask_next << 20));
                    if (!took) {
                        pool_next = total_work;             // nothing there (waves left to ask: the lanes come round again)
                        pool_end = ask_next >= kWaves ? total_work + n : total_work;
                    }
                }
                }
            }
            pool_next = __builtin_amdgcn_readfirstlane(pool_next);
            pool_end = __builtin_amdgcn_readfirstlane(pool_end);
            const uint32_t avail = pool_end - pool_next;
            const uint32_t w = pool_next + (uint32_t)rank;
            const bool got = (uint32_t)rank < avail;
            if (!got) continue;                         // range exhausted before my rank: go around
#ifdef RTP_EXIT_HIST
            if (w >= total_work) exit_hist_dead = (uint32_t)__builtin_amdgcn_s_memrealtime(); else exit_hist_fetch = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
            if (w >= total_work) { alive = false; break; }
            {
                int32_t pi, pj;
                uint32_t k;
                const uint32_t wm = work_list ? work_list[w] : w;
                if (kThreaded && work_list != nullptr && wm == kFlagHole) continue;      // a slot its wave never filled (flag_chunk_drain)
                uint32_t width = (uint32_t)P.width;
                int32_t first = P.pass_first;
                uint32_t record = 0;
                uint32_t wc = wm;           // kPrim: wm counts in fetch order (expensive pixels first); wc = pixel * count + slot is the sample's name
                f3 center;
                if constexpr (kPrim) {      // the pixel's row of the fetch-order table: its centre on the image plane and its name
                    static_assert(kConsts, "primary visibility feeds guarded kernels: all of them keep the constants block");
                    map_fetch(wm, consts_lds, wc, record, center);
                } else {
                    map_work<kConsts>(P, wm, pi, pj, k, consts_lds, &width, &first);
                }
                if (kPrim) {            // (hit distance, code, RNG state after the first draw's hash)
                    // (all twelve bytes in ONE load: read word by word, the third — needed only where the ray hit something — came
                    // with a second round trip behind the wait for the first two)
                    typedef float rec3 __attribute__((ext_vector_type(3), aligned(4)));
                    const rec3 rec = *reinterpret_cast<const rec3 *>(P.slab + (size_t)record * 3);
                    prim_t = rec.x;
                    prim_code = __float_as_int(rec.y);
                    if (prim_code != kPrimMiss) {
                        camera_ray_from_center(L, center, __float_as_uint(rec.z), ray_o, ray_d, consts_lds);
                    } else {            // no ray: the next store / fetch round adds beta * background = the background to this sample
                        L.beta = mk(1.0f, 1.0f, 1.0f);
                        L.color = mk(0.0f, 0.0f, 0.0f);
                        L.depth = 0;
                    }
                } else if (kThreaded && work_list != nullptr && P.resume_tag != nullptr && resume_load(P, wm, L, ray_o, ray_d)) {
                    // (the exact re-walk of a flagged sample goes on from the ray that was flagged: resume table)
                } else {
                    const uint32_t base_seed = wang_hash((uint32_t)pi * width + (uint32_t)pj);
                    RTP_CAMERA_START(L, P, pi, pj, base_seed, first + (int32_t)k, ray_o, ray_d, consts_lds);
                }
                w_cur = wc;
                path_open = true;
            }
        }
    };
    // rows of the lane's stack column that are not stack entries (step_pair_par's per-ray values), by byte offset
    auto lane_row = [&](int32_t row_bytes) -> float { return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(l_stack) + row_bytes); };
    auto set_lane_row = [&](int32_t row_bytes, float v) { *reinterpret_cast<float *>(reinterpret_cast<char *>(l_stack) + row_bytes) = v; };
    // the one place a ray is armed
    auto arm_ray = [&](f3 ray_o, f3 ray_d) {
        begin_ray<kWidePar>(L, ray_o, ray_d, first_node);
        if (kSent) L.sp = kLevelBytes;              // above the sentinel
        if (kDefer && L.node < 0 && L.node != kDone) { L.pend = L.node; L.node = kDone; }      // a tree of one primitive
        if (kGuard && !kDyn) guard_origin<kConsts>(L, P, consts_lds);
#if RTP_BODY_CARRY      // |d|^2 and its fp64 reciprocal, once for every sphere test of this ray: the front primitives' below, the parked ones'
        { const RayConst rc = ray_const(L); ray_a = rc.a; ray_y = rc.y; }
#endif
        // Front primitives (rt_accel.h): the few primitives that span the scene are not in the tree; every ray tests them here,
        // where all armed lanes of the wave do the same thing on the same record, and walks with their hit as its `closest`.
        // Which primitives are tested first makes no difference to the result: ties are flagged (test_sphere / test_plane).
        if (kGuard) {
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const uint32_t code = kConsts ? lds_s32(consts_lds + 16u * 13u + 4u * (uint32_t)f)
                                              : (f < P.num_front ? (uint32_t)P.front_code[f] : kNoFront);
                if (code == kNoFront) break;
                if (!kSimple && (code & 1u)) test_plane<true>(L, planes, (int32_t)(code >> 1), (int32_t)code);
#if RTP_BODY_CARRY
                else test_sphere_ray<true, false>(L, spheres[code >> 1], (int32_t)code, ray_a, (double)ray_a, ray_y);
#else
                else test_sphere<true>(L, spheres[code >> 1], (int32_t)code);
#endif
            }
        }
        if (kDynPar) {
            // step_pair_par's per-ray constants: sqrt(k) |d| (rounded up), and the growth that holds for every node — k D^2, D the
            // distance from the origin to the farthest corner of the small spheres' box, or what a hit already in hand allows
            const f4v c1 = ((lds_cfloat4 *)(uintptr_t)consts_lds)[1], c2 = ((lds_cfloat4 *)(uintptr_t)consts_lds)[2];
            const float ea = P.g_dyn_sqrtk * __builtin_amdgcn_sqrtf(lensq(L.d));          // (the host's sqrt(k) carries the 2^-19 that covers the approximate root)
            const float mx = fmaxf(fabsf(L.o.x - c1.z), fabsf(c1.w - L.o.x)), my = fmaxf(fabsf(L.o.y - c2.x), fabsf(c2.y - L.o.y)),
                        mz = fmaxf(fabsf(L.o.z - c2.z), fabsf(c2.w - L.o.z));
            float er = P.g_dyn_kslack * __builtin_fmaf(mz, mz, __builtin_fmaf(my, my, mx * mx));
            er = fminf(er, par_growth(L.closest, ea, er, dyn_par));
            set_lane_row(dyn_par.er_row, er);
            set_lane_row(dyn_par.ea_row, ea);
            L.e = er;
        }
    };

#if RTP_TRIPWIRE
    uint32_t trip_sig = 0xffffffffu;
    int trip_same = 0;
    bool trip_injected = false;
#endif
    for (;;) {
#if RTP_TRIPWIRE
        if (kDefer) {
            // state of the lane as the scheduler sees it (which sample, which ray of it, where in the tree)
            const uint32_t sig = (uint32_t)L.node * 0x9e3779b9u ^ (uint32_t)L.sp * 0x85ebca6bu ^ (uint32_t)L.pend * 0xc2b2ae35u ^ w_cur * 0x27d4eb2fu ^
                                 (uint32_t)L.depth * 0x165667b1u ^ (alive ? 1u : 0u) ^ (path_open ? 2u : 0u) ^ L.seed;
            trip_same = __any(sig != trip_sig) ? 0 : trip_same + 1;
            trip_sig = sig;
            if (trip_same > kTripRounds) {
                if (lane == 0) atomicMax(&P.stats[15], kTripNoProgress);
                break;
            }
            if (P.trip_test == 1u && !trip_injected && blockIdx.x == 0 && wave == 0 && lane == 7 && alive && path_open) {
                L.node = -3;          // a leaf code with the park slot EMPTY: not walking, not stuck, not finished
                L.pend = 0;
                trip_injected = true;
            }
        }
#endif
        // ---- SHADE step: lanes whose traversal is finished (or that have no path yet)
        RTP_COUNT(2, alive && finished());
        if (kPrim) {
            // Primary visibility known in advance (rt_primary.hip.inc): a new sample arrives with its first hit, so it
            // needs no walk but a shade step — this one.  Order inside the step: (A) lanes whose path is over (no hit:
            // background; flagged; ended by the last scatter) store their sample and take the next one, (B) new rays are
            // armed, (C) every lane with a hit to shade — old paths and new samples alike — runs the material code once.
            // A lane that misses therefore goes from the end of one path to the second ray of the next path within one
            // step, and the walk only ever sees rays that left a surface.
            if (alive && finished()) {
#if RTP_BODY_CARRY
                if (L.pend != 0) step_leaf_parked_ray<kSent>(L, spheres, l_stack, ray_a, ray_y);
#else
                if (kDefer && L.pend != 0) step_leaf_parked<kSent, kSimple>(L, spheres, planes, l_stack);
#endif
                auto over = [&]() { return alive && L.node == kDone && (!path_open || (L.hit < 0 && !(L.depth & kArmBit)) || (L.depth & (kFlagBit | kEndBit)) != 0); };
                bool go = over();
                for (int it = 0;; ++it) {
                    // (A): the lane's old path is over, so the camera ray of the next one goes straight into its place
#ifdef RTP_STATS_SHADE_SPLIT
                    st_fetch_rounds += __any(go) ? 1u : 0u;
#endif
                    if (go) {
                        if (path_open) {
                            if (L.hit < 0 && !(L.depth & (kFlagBit | kEndBit)))      // src/camera.cu:227-229: the ray left the scene
                                L.color = add(L.color, mul(L.beta, mk(P.bg[0], P.bg[1], P.bg[2])));
                            retire_sample();
                            // kDark: shade() adds nothing to the radiance, so it is +0 from the camera ray to the sum above — the
                            // same sum, from a constant: a product of -0 still stores as +0 — and with the sample stored it is +0
                            // again, for a lane that finds the pass dry as well: L.color is +0 wherever the loop comes round,
                            // which costs no register
                            if (kDark) L.color = mk(0.0f, 0.0f, 0.0f);
                        }
                        f3 ray_o = mk(0, 0, 0), ray_d = mk(0, 0, 0);
                        float prim_t = 0.0f;
                        int32_t prim_code = kPrimWalk;
                        fetch_sample(ray_o, ray_d, prim_t, prim_code);
                        if (alive) {
                            L.hit = -1;
                            L.pend = 0;
                            // (a sample whose primary ray hits nothing needs no ray at all: the next round stores the background)
                            if (prim_code != kPrimMiss) {
                                L.o = ray_o;
                                L.d = ray_d;
                                if (prim_code >= 0) { L.hit = prim_code; L.closest = prim_t; L.depth |= kFreshBit; }
                                else L.depth |= prim_code == kPrimFlag ? (kFlagBit | RTP_WHY(1)) : kArmBit;
                            }
                        }
                    }
#ifdef RTP_STATS_SHADE_SPLIT
                    RTP_STAMP(4);         // (A): store + fetch, with the wait for the sample's record
#endif
                    // (C) + (B)
                    const bool ready = alive && path_open && L.node == kDone && L.pend == 0 && L.hit >= 0 && !(L.depth & (kFlagBit | kEndBit));
                    const bool arm_walk = alive && (L.depth & kArmBit) != 0;
                    if (it == 0 || (int)__popcll(__ballot(ready)) >= RTP_PRIM_RESHADE || __any(arm_walk)) {
                        RTP_COUNT(3, ready);
                        bool cont = false;
                        if (ready) {
                            f3 unused_o, unused_d;          // (kPrim: shade() leaves the scattered ray in L.o / L.d)
                            cont = shade<kGuard, (kLds && !kSimple) ? RTP_LDS_MAT_ROWS : 3, kSimple, true, kWidePar, kDark>(L, P, spheres, planes, materials, sphere_mat, unused_o, unused_d);
                            if (!cont) L.depth |= kEndBit;
                        }
                        if (arm_walk) L.depth &= ~kArmBit;
                        if (cont || arm_walk) arm_ray(L.o, L.d);
                    }
#ifdef RTP_STATS_SHADE_SPLIT
                    RTP_STAMP(5);         // (C) + (B): material code, next ray armed
#endif
                    go = over();
                    if (!(it + 1 < RTP_PRIM_ROUNDS && (int)__popcll(__ballot(go)) >= RTP_PRIM_REFILL)) break;
                }
            }
        } else
        if (alive && finished()) {
            if (kDefer && L.pend != 0) step_leaf_parked<kSent, kSimple>(L, spheres, planes, l_stack);
            bool cont = false;
            f3 ray_o = mk(0, 0, 0), ray_d = mk(0, 0, 0);
            RTP_COUNT(3, path_open);
            if (path_open) cont = shade<kGuard, (kLds && !kSimple) ? RTP_LDS_MAT_ROWS : 3, kSimple, false, kWidePar>(L, P, spheres, planes, materials, sphere_mat, ray_o, ray_d);
            RTP_STAMP(4);
            if (!cont) {
                float prim_t = 0.0f;
                int32_t prim_code = 0;
                if (path_open) retire_sample();
                fetch_sample(ray_o, ray_d, prim_t, prim_code);
            }
            RTP_STAMP(5);
            if (alive) arm_ray(ray_o, ray_d);
        }
        RTP_STAMP(2);
        if (!__any(alive)) break;

        // ---- traversal steps until enough lanes wait for shading
        for (;;) {
            const bool is_inner = wants_inner<kThreaded>(L, end_node);      // idle/dead lanes hold a negative node
#if RTP_TRIPWIRE
            if (kDefer && __any(alive && path_open && !(is_inner || stuck_at_leaf() || finished()))) {
                if (lane == 0) atomicMax(&P.stats[15], kTripPartition);
                alive = false;           // (every lane of the wave: the outer loop ends at its next test)
                break;
            }
#endif
            const int n_inner = (int)__popcll(__ballot(is_inner));
            bool run_inner = n_inner >= P.k_inner;            // common case: decided by one ballot
            bool is_leaf = false;
            if (!run_inner) {
                is_leaf = alive && stuck_at_leaf();
                const int n_leaf = (int)__popcll(__ballot(is_leaf));
                const int n_alive = (int)__popcll(__ballot(alive));
                const int n_wait = n_alive - n_inner - n_leaf;
                if (n_inner + n_leaf == 0) break;
                if (n_wait >= P.k_shade) break;
                run_inner = n_leaf == 0;
            }
            RTP_STAMP(3);
            if (run_inner) {
                RTP_COUNT(0, is_inner);
                if (is_inner) {
                    if (kTreelet) step_threaded_x(L, l_nodes, P.xnodes, P.num_top);
                    else if (kOctT) step_threaded_oct(L, (uint32_t)oct_base);
                    else if (kThreaded) step_threaded(L, nodes, P.num_tnodes);
                    else if (kWidePar) step_wide_par(L, nodes, l_stack, walk_levels, dyn_par);
                    else if (kOct) step_octant(L, l_stack, P.stack_levels);
                    else if (kDynPair) step_pair_par(L, nodes, l_stack, walk_levels, dyn_par);
                    else step_inner<!kLds, !kLds>(L, nodes, l_nodes, P.num_top, l_stack, P.stack_levels);
                    if (kDefer && park_leaf<kSent>(L, l_stack) && kDynPar) L.e = lane_row(dyn_par.er_row);
                }
#pragma unroll
                for (int u = 1; u < (kWide && !kThreaded ? RTP_UNROLL_WIDE : RTP_UNROLL); ++u) {      // a few more box steps before re-voting
                    RTP_COUNT(0, wants_inner<kThreaded>(L, end_node));
                    if (wants_inner<kThreaded>(L, end_node)) {
                        if (kTreelet) step_threaded_x(L, l_nodes, P.xnodes, P.num_top);
                        else if (kOctT) step_threaded_oct(L, (uint32_t)oct_base);
                    else if (kThreaded) step_threaded(L, nodes, P.num_tnodes);
                        else if (kWidePar) step_wide_par(L, nodes, l_stack, walk_levels, dyn_par);
                        else if (kOct) step_octant(L, l_stack, P.stack_levels);
                        else if (kDynPair) step_pair_par(L, nodes, l_stack, walk_levels, dyn_par);
                        else step_inner<!kLds, !kLds>(L, nodes, l_nodes, P.num_top, l_stack, P.stack_levels);
                        if (kDefer && park_leaf<kSent>(L, l_stack) && kDynPar) L.e = lane_row(dyn_par.er_row);
                    }
                }
                RTP_STAMP(0);
            } else {
                if (kDefer) {       // every parked test, of stuck and of walking lanes alike
                    RTP_COUNT(1, alive && L.pend != 0);
                    if (kDynPar) {
                        if (alive && L.pend != 0) {
                            const float before = L.closest;
                            step_leaf_parked<kSent, kSimple, false>(L, spheres, planes, l_stack);
                            float er = lane_row(dyn_par.er_row);
                            if (L.closest < before) {       // a nearer hit: the ray's own bound comes down with it (step_pair_par)
                                er = fminf(er, par_growth(L.closest, lane_row(dyn_par.ea_row), er, dyn_par));
                                set_lane_row(dyn_par.er_row, er);
                                L.e = fminf(L.e, er);
                            }
                            if (park_leaf<kSent>(L, l_stack)) L.e = er;
                        }
                    } else
#if RTP_BODY_CARRY
                    if (alive && L.pend != 0) step_leaf_parked_ray<kSent>(L, spheres, l_stack, ray_a, ray_y);
#else
                    if (alive && L.pend != 0) step_leaf_parked<kSent, kSimple>(L, spheres, planes, l_stack);
#endif
                } else {
                    RTP_COUNT(1, is_leaf);
                    if (is_leaf) {
                        if (kThreaded) leaf_threaded<kSimple>(L, spheres, planes);
                        else step_leaf(L, spheres, planes, l_stack);
                    }
                }
                RTP_STAMP(1);
            }
        }
    }
    if (kConsts) {
        const uint32_t wave_u = (uint32_t)__builtin_amdgcn_readfirstlane(wave);
        flag_chunk_drain(consts_lds, chunk_lds, wave_u, lane);
    }            // the unused slots of the wave's last chunk of the flagged-sample list
#ifdef RTP_EXIT_HIST      // experiment: when do the waves of a launch run dry?  16 buckets of RTP_EXIT_BUCKET_US from RTP_EXIT_T0_US (wave lifetime, 100 MHz clock)
#ifndef RTP_EXIT_LAST_PATH
    if (lane == 0 && !kThreaded) {
        const int64_t us = (int64_t)((__builtin_amdgcn_s_memrealtime() - exit_hist_t0) / 100u) - (int64_t)RTP_EXIT_T0_US;
        const int64_t b = us < 0 ? 0 : us / (int64_t)RTP_EXIT_BUCKET_US;
        atomicAdd(&P.stats[b > 14 ? 14 : (int)b], 1u);
    }
#else       // of the waves that exit after RTP_EXIT_T0_US: how long did the last path of their last lane(s) take?  (buckets of RTP_EXIT_BUCKET_US)
    if (!kThreaded) {
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        const int64_t us = (int64_t)((now - exit_hist_t0) / 100u);
        if (us >= (int64_t)RTP_EXIT_T0_US && (uint32_t)now - exit_hist_dead < 300u) {
            const uint32_t b = (exit_hist_dead - exit_hist_fetch) / 100u / (uint32_t)RTP_EXIT_BUCKET_US;
            atomicAdd(&P.stats[b > 14u ? 14u : b], 1u);
        }
    }
#endif
#endif
#ifdef RTP_STATS
    if (lane == 0)
        for (int k = 0; k < 4; ++k) {
            atomicAdd(&P.stats[2 * k], st_iters[k]);
            atomicAdd(&P.stats[1 + 2 * k], st_lanes[k] >> 6);     // in units of full waves
            atomicAdd(&P.stats[8 + k], (uint32_t)(st_cycles[k] >> 10));   // kilo-ticks of s_memtime
        }
#ifdef RTP_STATS_SHADE_SPLIT
    if (lane == 0) { atomicAdd(&P.stats[12], (uint32_t)(st_cycles[4] >> 10)); atomicAdd(&P.stats[13], (uint32_t)(st_cycles[5] >> 10)); atomicAdd(&P.stats[14], st_fetch_rounds); }
#endif
#endif
