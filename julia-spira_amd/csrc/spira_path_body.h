// spira_path_body.h — the statements of k_path and of k_path_own (spira_device.h), included into the body of each: NOT a header of its own.
// One text, two kernels.  The including kernel names T, R, BVH, EXT, SPEC, MODE, TRI (k_path: its template parameters; k_path_own: constants) and
//   FIXED = false   k_path: every fact of the pass is a run-time value of PathArgs, and every statement is the one that always stood here;
//   FIXED = true    k_path_own: a full pixel-owning pass of 64 slots with every default knob on (spira_plan.h, own_kernel_ok — the host launches that
//                   kernel nowhere else).  own, priv, sky_runs, pixel_table, reach_masks, cam_consts and mixed are true and k_eff is 64 at compile time,
//                   so a run is the sub-chunks 2 g and 2 g + 1, a row never spans runs, and the arms such a pass never takes (path_of per camera ray,
//                   the all-ones scan mask, round-robin dealing, the slot-major L, the per-lane sky test) are not compiled in.  The statements that
//                   remain are k_path's, in its order and on its operands: same bits, same counters.
// Why an included text and not a __device__ function template: with the body behind a call — __forceinline__, by reference or by value — nine k_path
// instantiations of the main unit compile to other code (the headline's speculative one with 36 bytes of scratch): docs/experiments.md §45.  Included,
// every k_path listing is the parent's, byte for byte.
#ifndef SPIRA_PATH_FIXED
#error "spira_path_body.h is the body of k_path (SPIRA_PATH_FIXED 0) and of k_path_own (SPIRA_PATH_FIXED 1) in spira_device.h, nothing else includes it"
#endif
    constexpr bool FIXED = SPIRA_PATH_FIXED != 0;
    // the including kernel names all of these; there are exactly two combinations: k_path's template parameters with FIXED false, k_path_own's constants
    static_assert((R == 1 || R == 2) && MODE >= 0 && MODE <= 2 && (BVH || EXT || TRI || SPEC || true), "the including kernel names R, MODE, BVH, EXT, TRI, SPEC as constants");
    static_assert(!FIXED || (!BVH && !EXT && !TRI && sizeof(T) == 8 && R == 2 && MODE == 0 && SPIRA_CARRY_KEY && SPIRA_RESOLVE_RUN == 4), "k_path_own: Float64 sphere passes of 64 slots");
    extern __shared__ __attribute__((aligned(32))) unsigned char lds_raw[];
    constexpr uint32_t WPB = kBlock / 64, SUB = 64 * R;
    constexpr bool kRefArray = sizeof(T) == 4;
    // The RNG key of a scatter is mix32(mix32(sA + pixel) ^ sb), mix32(mix32(sB ^ pixel) + sb) with sb = sample << 8 | bounce (rng_key).  With
    // bounce < 256 the `| bounce` is an XOR / an addition of its own, so a path can carry ka = mix32(sA + pixel) ^ (sample << 8) and
    // kb = mix32(sB ^ pixel) + (sample << 8) — two words made once from the camera ray's pixel and sample — and a scatter derives its key with two mixes
    // instead of two divisions (path index -> pixel, sample) and four.  Same bits; the mesh and extension instantiations keep the derivation from q
    // (their parked entries have no room for the words, and the extensions need pixel and sample anyway).
    constexpr bool kCarry = SPIRA_CARRY_KEY && !BVH && !EXT;
    constexpr uint32_t kStageShift = 25, kRefMask = (1u << kStageShift) - 1u;      // a hit reference needs < 2^25; the packet's stage rides above it
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t NW = gridDim.x * WPB, wid = blockIdx.x * WPB + wave;
    const RenderConst<T> &rc = a.rc;
    using Pol = typename std::conditional<SPEC, SpecDiv, ExactDiv>::type;
    Pol pol;                                                     // how this instantiation divides (see SpecDiv)
    if (!SPEC && a.redo_only) {                                  // the launch behind a speculative one: only what that one reported
        uint32_t any = 0;
        for (uint32_t w = 0; w < WPB; ++w) any |= a.redo[blockIdx.x * WPB + w];
        if (!any) return;                                        // (workgroup-uniform, ahead of the barrier in stage_scene)
    }
    T *cam_lds = reinterpret_cast<T *>(lds_raw + scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles) + WPB * SUB * sizeof(Pack4<T>));
    if (threadIdx.x < 12) {                                      // camera: origin, lower-left corner, horizontal, vertical (visible after stage_scene's barrier)
        const Vec<T> *cv = threadIdx.x < 3 ? &rc.cam_origin : (threadIdx.x < 6 ? &rc.cam_llc : (threadIdx.x < 9 ? &rc.cam_hor : &rc.cam_ver));
        const uint32_t cc = threadIdx.x % 3;
        cam_lds[threadIdx.x] = cc == 0 ? cv->x : (cc == 1 ? cv->y : cv->z);
    }
    Pack4<T> *cam_sph = reinterpret_cast<Pack4<T> *>(reinterpret_cast<unsigned char *>(cam_lds) + 128);
    // (not in the extension instantiations: the second copy of the camera rays' scan costs the Float64 one 140 bytes of scratch per lane — glass scene 5.8 -> 6.6 ms)
    constexpr bool kCam = !EXT;
    if (kCam && MODE != 2 && (FIXED ? 1u : a.cam_consts))                       // (the second launch of a mesh pass has no camera rays)
        for (uint32_t i = threadIdx.x; i < a.scene.n_spheres; i += blockDim.x) {
            const T *sp = a.scene.spheres5 + 5 * (size_t)i;
            const Vec<T> oc = rc.cam_origin - mk<T>(sp[0], sp[1], sp[2]);         // :114 with the origin every camera ray has
            Pack4<T> k; k.x = oc.x; k.y = oc.y; k.z = oc.z; k.w = dot(oc, oc) - sp[3] * sp[3];      // :117 (radius*radius as stage_scene makes it)
            cam_sph[i] = k;
        }
    const SceneLds<T> sc = stage_scene<T>(a.scene, lds_raw);     // the only workgroup barrier of the kernel
    const PixelDiv<T> pix_div = pixel_divisors<T>(rc);
    if (!SPEC && a.redo_only) {
        if (!a.redo[wid]) return;                                // wave-uniform; no workgroup barrier follows
        if (lane == 0) atomicAdd(&a.stats->redone_waves, 1ull);
    }
    Pack4<T> *s_rnd = reinterpret_cast<Pack4<T> *>(lds_raw + scene_lds_bytes<T>(a.scene.n_spheres, a.scene.n_materials, a.scene.n_triangles)) + wave * SUB;
    constexpr uint32_t mesh_mode = BVH ? (uint32_t)MODE : 0u;
    const uint32_t kseg = mesh_mode == 2u ? a.resume_k : 1u;
    if (mesh_mode == 2u && wid * kseg >= a.resume_nw) return;    // wave-uniform; no workgroup barrier follows
    const uint32_t region = wid * kseg * a.cap;                  // (a fat wave owns the regions of the k waves it takes over)
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t ref_base = sc.n_spheres + sc.n_triangles;     // references >= ref_base are BVH triangle slots
    // Dense continuation (a.dense_pct > 0, max_depth <= 128; host default 70 %): when at least dense_pct % of a
    // sub-chunk's scattered rays hit again, they
    // stay in registers and go straight into their next stage instead of through the queue — compaction only where it pays (a closed
    // scene never touches the queues; an open one compacts as before).  Packets then carry their own stage (7 bits above the hit
    // reference), because a wave's region may hold hits of different segments.
    const bool mixed = FIXED || mesh_mode != 0u || rc.max_depth <= 128u;      // (the two launches of a mesh pass exist for max_depth <= 128 only: a compile-time fact there,
    const uint32_t dense_pct = mixed ? a.dense_pct : 0u;
    // Deferred mesh traversal (BVH scenes, max_depth <= 128): a ray that reaches the mesh's bounding box is not traversed where it
    // stands — a few lanes of every wave would walk the tree in global memory while the others wait — but parked on the wave's
    // mesh list; sessions (below) walk the parked rays with all 64 lanes, refilled as rays finish; a hit then enters the out queue as a
    // packet of its own stage.  (On the 81 920-triangle scene of config 5 the in-place traversal was 70 % of the frame time.)
    const bool defer = mesh_mode != 0u || (BVH && mixed && a.mesh_list != nullptr);      //  and so is `defer`: neither launch carries the in-place traversal or the stage-less packets of deeper
                                                                                         //  renders — config 5: Float32 4.05 -> 3.88 ms, Float64 5.26 -> 5.11 ms, no spilled VGPR left in the Float64 kernels)
    Pack4<T> *mlist = a.mesh_list + 3 * (size_t)region;
    uint32_t n_rmw = 0, n_store = 0, n_seg = 0, n_enq = 0, n_park = 0;   // (n_park: entries written to the mesh list, wave-uniform)
    uint32_t n_wtrips = 0, n_ltrips = 0;                         // trips of the traversal sessions' walk loop and the lanes walking in them (wave-uniform: scalar registers)
    uint32_t n_in = 0;                                           // packets waiting in this wave's region (rounds >= 1)
    const bool own = FIXED || (!BVH && !EXT && !TRI && sizeof(T) == 8 && a.accum != nullptr);      // a pixel-owning pass (PathArgs::accum)
    const uint32_t n_own = own ? 64u * (FIXED ? 64u : a.k_eff) : 0u;             // its paths of this wave
    const uint32_t n_sub_first = own ? (n_own + SUB - 1) / SUB : (a.n_first + SUB - 1) / SUB;
    // the wave's radiance in a block of its own (PathArgs::l_private): the queue word of path e of the wave is l_base + e instead of the path index
    const bool priv = FIXED || (kCarry && own && a.l_private != 0);
    const uint32_t l_base = priv ? wid * n_own : 0u;
    // All-sky runs (PathArgs::sky_runs): bit g of sky_mask = none of the camera rays of run g's RUN pixels can reach a sphere.  Geometry alone decides
    // (sky_pixel; lane = owned pixel), so the exact launch behind a speculative one finds the same runs.
    constexpr bool kOwnT = !BVH && !EXT && !TRI && sizeof(T) == 8;      // the compile-time part of `own`
    // The loop and the end-of-wave block read the mask from a word of LDS (the camera's 128 bytes hold 96: a word per wave behind them) — kept in a
    // scalar register across the loop it cost the speculative kernel 13 more spilled SGPRs, from LDS 3 (docs/experiments.md §28).
    uint32_t sky_mask = 0;
    uint32_t *sky_word = reinterpret_cast<uint32_t *>(cam_lds + 12) + wave;
    static_assert(12 * sizeof(T) + WPB * sizeof(uint32_t) <= 128 || !kOwnT, "a word per wave behind the camera");
    // The wave's pixel table and its runs' reach words (PathArgs::pixel_table / reach_masks): behind the camera's packets, where the host made room.
    PixelEntry *own_tab = reinterpret_cast<PixelEntry *>(reinterpret_cast<unsigned char *>(cam_lds) + 128 + ((FIXED ? 1u : a.cam_consts) ? a.scene.n_spheres * sizeof(Pack4<T>) : 0));
    uint32_t *reach_word = reinterpret_cast<uint32_t *>(own_tab + WPB * 64) + wave * (64 / SPIRA_RESOLVE_RUN);
    own_tab += wave * 64;
    if constexpr (kOwnT) {
        if (own && ((FIXED ? 1u : a.sky_runs) || (FIXED ? 1u : a.pixel_table) || (FIXED ? 1u : a.reach_masks))) {
            constexpr uint32_t kRun = SPIRA_RESOLVE_RUN, kRuns = 64 / kRun, kRowSlots = 64 / kRun;
            static_assert(kRun == 4 && 2 * 64 * sizeof(Pack3<T>) <= SUB * sizeof(Pack4<T>), "the run mask below is written for runs of 4; a row of terms fits the work list");
            {
                const uint32_t px = owned_pixel(wid, NW, lane);
                bool sky = false;
                uint32_t reach = 0xFFFFFFFFu;                        // (a pixel beyond the tile: its run is no sky run and scans everything)
                uint32_t pi = 1, pj = 1, pixel = 0, sample;
                if (px < rc.tile_pixels) {
                    bool beyond;
                    path_of<T>(rc, px, a.pass, pi, pj, pixel, sample);
                    reach = pixel_reach(cam_lds, rc.width, rc.height, pi, pj, a.scene.spheres5, a.scene.n_spheres, &beyond);
                    sky = reach == 0 && !beyond;                     // sky_pixel
                }
                if (FIXED ? 1u : a.pixel_table) {                                 // what the lane knows of its pixel: kept for the camera rows of the loop
                    PixelEntry &e = own_tab[lane];
                    e.hA = mix32(rc.sA + pixel); e.hB = mix32(rc.sB ^ pixel); e.im1 = pi - 1; e.jm1 = pj - 1; e.pixel = pixel;
                }
                if (FIXED ? 1u : a.reach_masks) {                                 // a run reaches what one of its pixels does
                    reach |= (uint32_t)__shfl_xor((int)reach, 1); reach |= (uint32_t)__shfl_xor((int)reach, 2);
                    if (lane % kRun == 0) reach_word[lane / kRun] = reach;
                }
                unsigned long long b = __ballot(sky);
                b &= b >> 1; b &= b >> 2;                            // bit 4 g: all four pixels of run g (inside the tile, and sky)
                if (FIXED ? 1u : a.sky_runs) for (uint32_t g = 0; g < kRuns; ++g) sky_mask |= (uint32_t)((b >> (kRun * g)) & 1ull) << g;
            }
            // The sky pass.  Run g's paths in the loop's order — rows of RUN pixels x 64 / RUN slots, the loop's own camera ray and sky term — but the
            // terms go to the wave's work list (idle until the loop's first phase 1) and lanes 0 .. RUN-1 add them up in sample order: resolve_pixel's statements.
            Pack3<T> *s_sky = reinterpret_cast<Pack3<T> *>(s_rnd);
            for (uint32_t m = sky_mask; m; m &= m - 1u) {
                const uint32_t g = (uint32_t)__builtin_ctz(m);
                const uint32_t px = owned_pixel(wid, NW, g * kRun + lane % kRun);
                uint32_t pi, pj, pixel, sample0;
                path_of<T>(rc, px, a.pass, pi, pj, pixel, sample0);           // slot 0 of the pixel
                Pack3<T> acc;
                acc.x = 0; acc.y = 0; acc.z = 0;
                if (!a.accum_first && lane < kRun) { const Pack4<T> a0 = a.accum[px]; acc.x = a0.x; acc.y = a0.y; acc.z = a0.z; }
                for (uint32_t s0 = 0; s0 < (FIXED ? 64u : a.k_eff); s0 += kRowSlots) {
                    const uint32_t slot = s0 + lane / kRun;
                    if (slot < (FIXED ? 64u : a.k_eff)) {
                        Vec<T> o_, d_;
                        camera_ray_lds<T>(rc, cam_lds, pix_div, pi, pj, pixel, sample0 + slot, o_, d_, pol);
                        const Vec<T> c = sky_term_x<T, EXT>(d_, mk<T>(1, 1, 1), nullptr);      // :365-366, beta as the loop has it for a camera ray
                        Pack3<T> l; l.x = c.x; l.y = c.y; l.z = c.z;
                        s_sky[lane] = l;
                        ++n_seg; ++n_store;                               // counted as the loop counts a camera ray that leaves the scene
                    }
                    wave_lds_sync();
                    if (lane < kRun) {
                        const uint32_t n = (FIXED ? 64u : a.k_eff) - s0 < kRowSlots ? (FIXED ? 64u : a.k_eff) - s0 : kRowSlots;
                        for (uint32_t k = 0; k < n; ++k) { const Pack3<T> l = s_sky[k * kRun + lane]; acc.x = acc.x + l.x; acc.y = acc.y + l.y; acc.z = acc.z + l.z; }
                    }
                    wave_lds_sync();
                }
                // the finished sum waits in the pixel's slot-0 entry of L (nothing else of the run is touched) for the end-of-wave block
                if (lane < kRun) a.L[priv ? l_base + g * (FIXED ? 64u : a.k_eff) * kRun + lane : px] = acc;
            }
        }
        if (own) { if (lane == 0) *sky_word = sky_mask; wave_lds_sync(); }
    }

    // park a ray on the wave's mesh list (entry = 3 packets: {o, d.x} {d.y, d.z, beta.xy} {beta.z, closest so far, q, object so far + stage of the hit})
    auto park = [&](uint32_t slot_i, const Vec<T> o_, const Vec<T> d_, const Vec<T> beta_, T closest_, uint32_t q_, int prim_, uint32_t stage_hit) {
        Pack4<T> A, B, C;
        A.x = o_.x; A.y = o_.y; A.z = o_.z; A.w = d_.x;
        B.x = d_.y; B.y = d_.z; B.z = beta_.x; B.w = beta_.y;
        C.x = beta_.z; C.y = closest_; C.z = Bits<T>::from_u32(q_); C.w = Bits<T>::from_u32((uint32_t)(prim_ + 1) | (stage_hit << kStageShift));
        mlist[3 * (size_t)slot_i] = A; mlist[3 * (size_t)slot_i + 1] = B; mlist[3 * (size_t)slot_i + 2] = C;
    };
    // Rounds: every packet of the wave's queue advances one stage per round; parked rays re-enter as hit packets after a traversal
    // session, possibly several rounds after they were parked (packets carry their own stage).  Ends when queue and list are empty.
    uint32_t mfill = 0;                                              // entries on the mesh list
    // mode 2: the list starts as the k lists the first launch left, segment j at its wave's region; pfx[j] = entries ahead of segment j
    constexpr int kMaxSeg = 16;
    uint32_t pfx[kMaxSeg + 1];
    bool segmented = false;
    {
        uint32_t cnt = 0;
        if (mesh_mode == 2u && lane < kseg && wid * kseg + lane < a.resume_nw) cnt = a.mesh_count[wid * kseg + lane];
        pfx[0] = 0;
#pragma unroll
        for (int j = 0; j < kMaxSeg; ++j) pfx[j + 1] = pfx[j] + (uint32_t)__builtin_amdgcn_readlane((int)cnt, j);
        if (mesh_mode == 2u) { mfill = pfx[kMaxSeg]; segmented = true; }
    }
    // Mode 1: wave w*k + i works on the sub-chunks of "logical" wave i*(NW/k) + w, so that the k waves a fat wave of the second launch takes over
    // (w*k .. w*k+k-1: contiguous regions) cover image blocks NW/k sub-chunks apart — adjacent blocks see the mesh together or not at all, and
    // fat waves made of them ran 1.5x apart.  (Any bijection will do: the assignment only has to be a pure function of the wave index.)
    const uint32_t first_sub = own ? 0u : (mesh_mode == 1u ? (wid % a.resume_k) * (NW / a.resume_k) + wid / a.resume_k : wid);
    const uint32_t sub_step = own ? 1u : NW;
    MESH_STAT(unsigned long long dbg_t0 = __builtin_readcyclecounter(); unsigned long long dbg_sess = 0, dbg_walk = 0; uint32_t dbg_ns = 0, dbg_ws = 0, dbg_ls = 0, dbg_rf = 0, dbg_rays = 0, dbg_rounds = 0, dbg_ws1 = 0, dbg_ls1 = 0, dbg_h[4] = {0, 0, 0, 0};)
    for (uint32_t round = 0; ; ++round) {
        MESH_STAT(++dbg_rounds;)
        const bool first = mesh_mode != 2u && round == 0;
        const RayQueue<T> qin = a.q[(round + 1) & 1], qout = a.q[round & 1];
        const uint32_t *rin = a.qref[(round + 1) & 1];
        uint32_t *rout = a.qref[round & 1];
        const uint2 *kin = a.qkey[(round + 1) & 1];
        uint2 *kout = a.qkey[round & 1];
        const uint32_t limit = first ? (own ? n_own : a.n_first) : n_in;
        const uint32_t n_sub = first ? n_sub_first : (n_in + SUB - 1) / SUB;
        uint32_t fill = 0;
        for (uint32_t sub = first ? first_sub : 0u; sub < n_sub; sub += first ? sub_step : 1u) {
            if constexpr (kOwnT) if (own && first) {      // a sub-chunk that lies inside one all-sky run holds nothing to deal (wave-uniform)
                const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)*sky_word);
                if constexpr (FIXED) { if ((m >> (sub >> 1)) & 1u) continue; }      // (64 slots: sub-chunks 2 g and 2 g + 1 are run g)
                else {
                    const uint32_t r0 = fastdiv(sub * SUB / SPIRA_RESOLVE_RUN, a.fd_keff), r1 = fastdiv((sub * SUB + SUB - 1) / SPIRA_RESOLVE_RUN, a.fd_keff);
                    if (r0 == r1 && ((m >> r0) & 1u)) continue;
                }
            }
            Vec<T> o[R], beta[R];
            Pending<T> pend[R];                           // between trips pend[r].v holds the direction the hit was reached along
            ExtState<T> ex[R];                            // EXT instantiations only (dead otherwise)
            uint32_t q[R], ent[R], stg[R], ref[R];
            uint32_t ka[R], kb[R];                        // kCarry: the path's half-made RNG key
            bool valid[R];
            uint32_t cmask_sub = 0xFFFFFFFFu;             // FIXED: the run's reach word, read once for both rows (a row never spans runs)
            if constexpr (FIXED) if (first) cmask_sub = (uint32_t)__builtin_amdgcn_readfirstlane((int)reach_word[sub >> 1]);
            // ---------------- the sub-chunk's rays: camera rays + their closest hit (round 0) or queued hits
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t idx = sub * SUB + r * 64 + lane;
                valid[r] = false; stg[r] = round; ref[r] = 0; q[r] = 0; ka[r] = 0; kb[r] = 0;
                pend[r].kind = kDead; pend[r].rough = 0; pend[r].v = mk<T>(0, 0, 0);
                o[r] = mk<T>(0, 0, 0); beta[r] = mk<T>(1, 1, 1);
                bool parked = false; T park_t = 0; int park_prim = -1;
                uint32_t qf = idx;                                // round 0: the camera ray's path index
                bool in = (FIXED && first) || idx < limit;            // (FIXED: all 64 x 64 paths of the wave exist)
                uint32_t own_l = 0, own_slot = 0;                 // pixel-owning pass: whose pixel of the wave's 64 the path is, and which of its slots
                if (own && first) {                               // pixel-owning pass: idx is the wave's path (PathArgs::accum)
                    const uint32_t t = idx / SPIRA_RESOLVE_RUN, run = FIXED ? sub >> 1 : fastdiv(t, a.fd_keff);
                    own_l = run * SPIRA_RESOLVE_RUN + idx % SPIRA_RESOLVE_RUN; own_slot = t - run * (FIXED ? 64u : a.k_eff);
                    const uint32_t px = owned_pixel(wid, NW, own_l);
                    qf = own_slot * rc.tile_pixels + px;
                    in = in && px < rc.tile_pixels;
                    if constexpr (kOwnT && !FIXED) in = in && !((*sky_word >> run) & 1u);       // an all-sky run was summed ahead of the loop (FIXED: its sub-chunks were skipped whole)
                }
                const uint32_t ql = priv ? l_base + idx : qf;              // where the path's radiance lives: what the queue word carries
                if (in) {
                    if (first) {
                        uint32_t pixel, sample, pi, pj;
                        Vec<T> d;
                        q[r] = ql;
                        uint32_t cmask = 0xFFFFFFFFu;             // the spheres this row's camera scan visits (kOwnT; wave-uniform)
                        if constexpr (kOwnT) {
                            uint32_t hA, hB, im1, jm1;
                            if (own && (FIXED ? 1u : a.pixel_table)) {           // the pixel's entry of the wave's table instead of two divisions and two mixes per path
                                const PixelEntry e = own_tab[own_l];
                                hA = e.hA; hB = e.hB; im1 = e.im1; jm1 = e.jm1;
                                sample = rc.sample0 + a.pass * rc.slots + own_slot;
                            } else {
                                path_of<T>(rc, qf, a.pass, pi, pj, pixel, sample);
                                hA = mix32(rc.sA + pixel); hB = mix32(rc.sB ^ pixel); im1 = pi - 1; jm1 = pj - 1;
                            }
                            ka[r] = hA ^ (sample << 8); kb[r] = hB + (sample << 8);
                            camera_ray_lds<T>(cam_lds, pix_div, im1, jm1, hA, hB, sample, o[r], d, pol);
                            // a row inside one run (k_eff a multiple of the row's slots) of a scene the mask has a bit for every sphere of
                            if constexpr (FIXED) cmask = cmask_sub;      // (the host launches k_path_own for 1 .. 32 spheres only)
                            else if (own && a.reach_masks && a.k_eff % (64 / SPIRA_RESOLVE_RUN) == 0 && sc.n_spheres <= 32u)
                                cmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)reach_word[fastdiv((sub * SUB + r * 64) / SPIRA_RESOLVE_RUN, a.fd_keff)]);
                        } else {
                            path_of<T>(rc, qf, a.pass, pi, pj, pixel, sample);
                            if (kCarry) { ka[r] = mix32(rc.sA + pixel) ^ (sample << 8); kb[r] = mix32(rc.sB ^ pixel) + (sample << 8); }
                            camera_ray_lds<T>(rc, cam_lds, pix_div, pi, pj, pixel, sample, o[r], d, pol);
                        }
                        if (EXT) { ex[r].flags = rc.flags; if (rc.flags & kExtSpectral) beta[r] = ext_wavelength<T>(sc, rc.sA, rc.sB, pixel, sample, ex[r]); }
                        T t; uint32_t slot = 0;
                        int prim;
                        if (defer) {
                            if (kCam && (FIXED ? 1u : a.cam_consts)) closest_hit_local<T, Pol, TRI, true>(sc, o[r], d, (T)0.001, t, prim, pol, cam_sph);
                            else closest_hit_local<T, Pol, TRI>(sc, o[r], d, (T)0.001, t, prim, pol);   // :335, spheres and LDS triangles
                            parked = mesh_box_hit<T>(sc, o[r], d, t);
                        } else if (kCam && !BVH && (FIXED ? 1u : a.cam_consts)) {
                            if constexpr (kOwnT) closest_hit_cam_masked<T, Pol>(sc, d, (T)0.001, t, prim, pol, cam_sph, cmask);      // (all ones: the full scan)
                            else closest_hit_local<T, Pol, TRI, true>(sc, o[r], d, (T)0.001, t, prim, pol, cam_sph);
                        }
                        else prim = closest_hit<T, BVH, Pol, TRI>(sc, o[r], d, (T)0.001, t, slot, pol);     // :335
                        ++n_seg;
                        if (parked) { park_t = t; park_prim = prim; pend[r].v = d; }          // parked below, in uniform control flow
                        else if (prim < 0) {                      // the camera ray leaves the scene: sky, :365-366
                            const Vec<T> c = sky_term_x<T, EXT>(d, beta[r], &ex[r]);
                            Pack3<T> l; l.x = c.x; l.y = c.y; l.z = c.z;
                            a.L[ql] = l;
                            ++n_store;
                        } else {
                            valid[r] = true;
                            o[r] = o[r] + d * t;                  // point_at, :138 / :183
                            ref[r] = (BVH && prim >= (int)ref_base) ? ref_base + slot : (uint32_t)prim;
                            pend[r].v = d;
                        }
                    } else {
                        const Pack4<T> A = qin.A[region + idx], B = qin.B[region + idx];
                        const Pack2<T> C = qin.C[region + idx];
                        o[r] = mk<T>(A.x, A.y, A.z);              // the hit point
                        pend[r].v = mk<T>(A.w, B.x, B.y);         // the direction it was reached along
                        beta[r] = mk<T>(B.z, B.w, C.x);
                        q[r] = unpack_q(C.y);
                        uint32_t w;
                        if constexpr (kRefArray) w = rin[region + idx]; else w = unpack_ref(C.y);
                        if (mixed) { stg[r] = w >> kStageShift; ref[r] = w & kRefMask; } else ref[r] = w;
                        if (kCarry) { const uint2 k = kin[region + idx]; ka[r] = k.x; kb[r] = k.y; }
                        valid[r] = true;
                    }
                }
                if (defer && first) {                             // camera rays that reach the mesh's box: onto the mesh list (stage of the hit: 0)
                    const unsigned long long mp = __ballot(parked);
                    if (parked) park(mfill + __popcll(mp & lt_mask), o[r], pend[r].v, beta[r], park_t, q[r], park_prim, 0u);
                    mfill += (uint32_t)__popcll(mp); n_park += (uint32_t)__popcll(mp);
                }
            }
            // ---------------- stages on these rays; normally ONE trip, more while the hits stay dense
            while (true) {
                uint32_t n_list = 0, n_valid = 0;
                // ---- phase 1: the hit of segment stg[r]
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    bool want = false;
                    RngKey key;
                    const Vec<T> d = pend[r].v;
                    pend[r].kind = kDead;
                    if (valid[r]) {
                        uint32_t pixel = 0, sample = 0, pi, pj;
                        const bool scatter = stg[r] + 1 < rc.max_depth;
                        int prim = (int)ref[r]; uint32_t slot = 0;
                        if (BVH && ref[r] >= ref_base) { prim = (int)ref_base; slot = ref[r] - ref_base; }
                        const uint32_t qi = q[r] & 0x7FFFFFFFu;
                        const bool has_l = (q[r] >> 31) != 0;
                        if (EXT) {
                            path_of<T>(rc, qi, a.pass, pi, pj, pixel, sample);
                            ex[r].flags = rc.flags;
                            if (rc.flags & kExtSpectral) (void)ext_wavelength<T>(sc, rc.sA, rc.sB, pixel, sample, ex[r]);
                        }
                        Vec<T> contrib;
                        const bool has_contrib = shade_hit<T, BVH, EXT, Pol, TRI>(sc, o[r], d, prim, slot, beta[r], scatter, contrib, pend[r], &ex[r], pol);
                        // Path radiance L[q]: while bit 31 of q is clear a term is a plain store (0 + x == x exactly); the
                        // load -> add -> store round trip only remains for paths that met an emitter earlier.
                        if (has_contrib) {
                            Pack3<T> l; l.x = contrib.x; l.y = contrib.y; l.z = contrib.z;
                            if (has_l) { const Pack3<T> l0 = a.L[qi]; l.x = l0.x + contrib.x; l.y = l0.y + contrib.y; l.z = l0.z + contrib.z; ++n_rmw; }
                            else ++n_store;
                            a.L[qi] = l;
                            q[r] |= 0x80000000u;
                        } else if (!scatter && !has_l) {          // the path ends here without ever having contributed
                            Pack3<T> l; l.x = 0; l.y = 0; l.z = 0;
                            a.L[qi] = l;
                            ++n_store;
                        }
                        want = (pend[r].kind == kDiffuse || pend[r].kind == kSpecRough);
                        if (want || (EXT && pend[r].kind == kDielectric)) {
                            if (kCarry && mixed) {                // (max_depth <= 128: the bounce fits the low byte)
                                key.hA = mix32(ka[r] ^ stg[r]); key.hB = mix32(kb[r] + stg[r]); key.hBr = (key.hB << 16) | (key.hB >> 16);
                            } else {
                                if (!EXT) path_of<T>(rc, qi, a.pass, pi, pj, pixel, sample);
                                key = rng_key(rc.sA, rc.sB, pixel, sample, stg[r]);
                            }
                            if (EXT && pend[r].kind == kDielectric) dielectric_resolve<T>(pend[r], d, key);     // -> kMirror
                        }
                    }
                    const unsigned long long mv = __ballot(pend[r].kind != kDead);
                    n_valid += (uint32_t)__popcll(mv);
                    const unsigned long long m = __ballot(want);
                    if (want) {                                   // append to the wave's work list
                        ent[r] = n_list + __popcll(m & lt_mask);
                        uint32_t *kw = reinterpret_cast<uint32_t *>(&s_rnd[ent[r]]);
                        kw[0] = key.hA; kw[1] = key.hB;
                    }
                    n_list += (uint32_t)__popcll(m);
                }
                if (n_valid == 0) break;           // wave-uniform: nobody scatters (last segments, or an empty tail)
                wave_lds_sync();
                // ---- phase 2: cooperative random_in_unit_sphere() over the wave's work list
                drain_unit_sphere_list<T>(s_rnd, n_list, lane);
                wave_lds_sync();
                // ---- phase 3: direction, closest hit of segment stg[r] + 1
                uint32_t n_hit = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    bool hit = false, parked3 = false;
                    T park_t3 = 0; int park_prim3 = -1;
                    if (pend[r].kind != kDead) {
                        Vec<T> rnd = mk<T>(0, 0, 0);
                        if (pend[r].kind != kMirror) rnd = RndTry<T>::load(&s_rnd[ent[r]]);
                        const Vec<T> nd = segment_back<T>(o[r], pend[r], rnd, pol);
                        T t; uint32_t slot = 0;
                        int prim;
                        if (defer) {
                            closest_hit_local<T, Pol, TRI>(sc, o[r], nd, (T)0.001, t, prim, pol);   // :335 of the next level, LDS part
                            parked3 = mesh_box_hit<T>(sc, o[r], nd, t);
                        } else prim = closest_hit<T, BVH, Pol, TRI>(sc, o[r], nd, (T)0.001, t, slot, pol); // :335 of the next level
                        ++n_seg;
                        if (parked3) { park_t3 = t; park_prim3 = prim; pend[r].v = nd; }
                        else if (prim < 0) {                          // the path leaves the scene: its last term, :365-366
                            const Vec<T> c = sky_term_x<T, EXT>(nd, beta[r], &ex[r]);
                            const uint32_t qi = q[r] & 0x7FFFFFFFu;
                            Pack3<T> l; l.x = c.x; l.y = c.y; l.z = c.z;
                            if (q[r] >> 31) { const Pack3<T> l0 = a.L[qi]; l.x = l0.x + c.x; l.y = l0.y + c.y; l.z = l0.z + c.z; ++n_rmw; }
                            else ++n_store;
                            a.L[qi] = l;
                        } else {
                            hit = true;
                            o[r] = o[r] + nd * t;                     // point_at, :138 / :183
                            ref[r] = (BVH && prim >= (int)ref_base) ? ref_base + slot : (uint32_t)prim;
                            pend[r].v = nd;
                            ++stg[r];
                        }
                    }
                    if (defer) {                                  // rays that reach the mesh's box wait for the end of the round
                        const unsigned long long mp = __ballot(parked3);
                        if (parked3) park(mfill + __popcll(mp & lt_mask), o[r], pend[r].v, beta[r], park_t3, q[r], park_prim3, stg[r] + 1u);
                        mfill += (uint32_t)__popcll(mp); n_park += (uint32_t)__popcll(mp);
                    }
                    valid[r] = hit;
                    n_hit += (uint32_t)__popcll(__ballot(hit));
                }
                wave_lds_sync();      // the list slots are rewritten by the next trip's / sub-chunk's phase 1
                if (n_hit == 0) break;
                if (dense_pct && n_hit * 100u >= n_valid * dense_pct) continue;     // dense: the hits stay in registers
                // ---- compaction of the hits into this wave's region of the out queue
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const unsigned long long m = __ballot(valid[r]);
                    if (valid[r]) {
                        const uint32_t dst = region + fill + __popcll(m & lt_mask);
                        const Vec<T> nd = pend[r].v;
                        const uint32_t w = mixed ? (ref[r] | (stg[r] << kStageShift)) : ref[r];
                        Pack4<T> A, B; Pack2<T> C;
                        A.x = o[r].x; A.y = o[r].y; A.z = o[r].z; A.w = nd.x;
                        B.x = nd.y; B.y = nd.z; B.z = beta[r].x; B.w = beta[r].y;
                        C.x = beta[r].z; C.y = pack_qref(q[r], w, (T)0);
                        qout.A[dst] = A; qout.B[dst] = B; qout.C[dst] = C;
                        if constexpr (kRefArray) rout[dst] = w;
                        if constexpr (kCarry) kout[dst] = make_uint2(ka[r], kb[r]);
                    }
                    fill += (uint32_t)__popcll(m);
                }
                break;
            }
        }
        if (defer && mesh_mode != 1u && mfill && (mfill >= a.mesh_min_batch || fill == 0)) {
            // ---------------- traversal session over the wave's parked rays.  A divergent node fetch costs the CU the same whether 64 lanes
            // take part or one (profiles/r03_gather_chase.txt), so the wave is kept full: whenever `refill_free` lanes have finished their
            // ray, their results are emitted (hits compacted into the out queue, sky terms for the others) and they take the next parked
            // rays; only the list's last rays run down to the slowest.  (The work list's LDS is idle now: the first stack levels live there.)
            constexpr int kLdsStack = (int)(SUB * sizeof(Pack4<T>) / (64 * sizeof(uint32_t)));      // 8 levels in Float32, 16 in Float64
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // the list was written by this wave's own lanes
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            uint32_t *lstack = reinterpret_cast<uint32_t *>(s_rnd);
            uint32_t stack[kBvhStackD - kLdsStack];
            uint32_t next = 0;                                         // next unread entry (wave-uniform)
            MESH_STAT(const unsigned long long dbg_s0 = __builtin_readcyclecounter(); ++dbg_ns; dbg_rays += mfill;)
#ifdef SPIRA_BVH_SCREEN
            constexpr bool kScreened = sizeof(T) == 8;
#else
            constexpr bool kScreened = false;
#endif
            if constexpr (kScreened) {
            // ---- Float64: the walk runs on Float32 screens (bvh8_step_screened) and a walking lane holds nothing of its ray in Float64: the parked entry is read
            // again when the lane has finished, its candidates go through the scan's own Float64 test there (all finished lanes together: one round trip per
            // candidate of the lane that holds the most), and the result is emitted as in the Float32 session below.
            bool walking = false, finished = false, full = false;      // finished: a result waits to be emitted; full: the candidate list has to be emptied
            uint32_t ent_i = 0;                                        // the lane's parked entry (index into a.mesh_list)
            float dxf = 0, dyf = 0, dzf = 1;
            Bvh8Ray ry; ry.ox = ry.oy = ry.oz = 0; ry.ix = ry.iy = ry.iz = 1; ry.oct = 0; ry.best = 0; ry.tmin = 0; ry.amin = 0;
            Bvh8Walk<T> wk; wk.G = 0; wk.tw = 0; wk.rank = 0; wk.sp = 0; wk.t0 = 0; wk.c0 = wk.c1 = wk.c2 = wk.c3 = 0; wk.nc = 0;
            auto decode = [&](const Pack4<T> A, const Pack4<T> B, const Pack4<T> C, Vec<T> &o_, Vec<T> &d_, Vec<T> &beta_, T &closest, uint32_t &q_, int &prim, uint32_t &slot, uint32_t &stage_hit) {
                o_ = mk<T>(A.x, A.y, A.z); d_ = mk<T>(A.w, B.x, B.y); beta_ = mk<T>(B.z, B.w, C.x);
                closest = C.y;
                q_ = Bits<T>::to_u32(C.z);
                const uint32_t pw = Bits<T>::to_u32(C.w);
                prim = (int)(pw & kRefMask) - 1;                       // the closest object so far: a sphere / LDS triangle, or (an entry written back below) a mesh triangle
                stage_hit = pw >> kStageShift;
                slot = 0;
                if (prim >= (int)ref_base) { slot = (uint32_t)prim - ref_base; prim = (int)ref_base; }
            };
            while (true) {
                // ---- lanes whose candidate list is full: their candidates go through the exact test now, the result so far is written back into the entry (rare)
                if (__any(full)) {
                    if (full) {
                        Pack4<T> *ent = a.mesh_list + 3 * (size_t)ent_i;
                        const Pack4<T> A = ent[0], B = ent[1];
                        Pack4<T> C = ent[2];
                        Vec<T> o_, d_, beta_; T closest; uint32_t q_, slot, stage_hit; int prim;
                        decode(A, B, C, o_, d_, beta_, closest, q_, prim, slot, stage_hit);
                        while (wk.nc) bvh8_resolve_one<T>(sc, wk, ry, o_, d_, (T)0.001, (int)ref_base, closest, prim, slot);
                        C.y = closest;
                        C.w = Bits<T>::from_u32((uint32_t)((prim >= (int)ref_base ? (int)(ref_base + slot) : prim) + 1) | (stage_hit << kStageShift));
                        ent[2] = C;
                        full = false;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
                // ---- emit what is finished (wave-uniform block)
                {
                    Vec<T> o_ = mk<T>(0, 0, 0), d_ = mk<T>(0, 0, 1), beta_ = mk<T>(0, 0, 0);
                    T closest = 0; uint32_t q_ = 0, stage_hit = 0, slot = 0; int prim = -1;
                    if (finished) {
                        // the entry and the newest candidate's Float64 record in ONE round trip (most rays hold at most one candidate)
                        const Pack4<T> *ent = a.mesh_list + 3 * (size_t)ent_i;
                        const bool has = wk.nc != 0;
                        const uint32_t ti = has ? wk.c0 : 0u;
                        const Pack4<T> *rec = sc.bvh_tris + 3 * (size_t)ti;
                        const Pack4<T> A = ent[0], B = ent[1], C = ent[2];
                        const Pack4<T> v0 = rec[0], e1 = rec[1], e2 = rec[2];
                        decode(A, B, C, o_, d_, beta_, closest, q_, prim, slot, stage_hit);
                        if (has) {
                            wk.c0 = wk.c1; wk.c1 = wk.c2; wk.c2 = wk.c3; --wk.nc;
                            T t;
                            if (triangle_test<T>(v0, e1, e2, o_, d_, (T)0.001, closest, t)) {
                                const int p = (int)ref_base + (int)Bits<T>::to_u32(v0.w);
                                if (t < closest || p > prim) { closest = t; prim = p; slot = ti; }      // t == closest: the later object wins
                            }
                        }
                    }
                    while (__any(finished && wk.nc != 0)) {
                        if (finished && wk.nc != 0) bvh8_resolve_one<T>(sc, wk, ry, o_, d_, (T)0.001, (int)ref_base, closest, prim, slot);
                    }
                    const unsigned long long mh = __ballot(finished && prim >= 0);
                    if (finished) {
                        if (prim < 0) {                                   // the ray leaves the scene after all: sky, :365-366
                            const uint32_t qi = q_ & 0x7FFFFFFFu;
                            ExtState<T> ex1; ex1.flags = rc.flags; ex1.bR = 0; ex1.bG = 0; ex1.bB = 0;
                            if (EXT && (rc.flags & kExtSpectral)) {
                                uint32_t pi, pj, pixel, sample;
                                path_of<T>(rc, qi, a.pass, pi, pj, pixel, sample);
                                (void)ext_wavelength<T>(sc, rc.sA, rc.sB, pixel, sample, ex1);
                            }
                            const Vec<T> c = sky_term_x<T, EXT>(d_, beta_, &ex1);
                            Pack3<T> l; l.x = c.x; l.y = c.y; l.z = c.z;
                            if (q_ >> 31) { const Pack3<T> l0 = a.L[qi]; l.x = l0.x + c.x; l.y = l0.y + c.y; l.z = l0.z + c.z; ++n_rmw; }
                            else ++n_store;
                            a.L[qi] = l;
                        } else {
                            const Vec<T> hp = o_ + d_ * closest;          // point_at, :138 / :183
                            const uint32_t w_ = ((prim >= (int)ref_base) ? ref_base + slot : (uint32_t)prim) | (stage_hit << kStageShift);
                            const uint32_t dst = region + fill + __popcll(mh & lt_mask);
                            Pack4<T> A, B; Pack2<T> C;
                            A.x = hp.x; A.y = hp.y; A.z = hp.z; A.w = d_.x;
                            B.x = d_.y; B.y = d_.z; B.z = beta_.x; B.w = beta_.y;
                            C.x = beta_.z; C.y = pack_qref(q_, w_, (T)0);
                            qout.A[dst] = A; qout.B[dst] = B; qout.C[dst] = C;
                            if constexpr (kRefArray) rout[dst] = w_;
                        }
                    }
                    fill += (uint32_t)__popcll(mh);
                    finished = false;
                }
                // ---- refill the free lanes
                const unsigned long long mf = __ballot(!walking);
                const uint32_t take = min((uint32_t)__popcll(mf), mfill - next);
                if (!walking && (uint32_t)__popcll(mf & lt_mask) < take) {
                    const uint32_t e = next + (uint32_t)__popcll(mf & lt_mask);
                    ent_i = region + e;
                    if (segmented) {                               // entry e of the k lists taken over: which list, which entry of it
                        uint32_t seg = 0, off = e;
#pragma unroll
                        for (int j = 1; j < kMaxSeg; ++j) if (e >= pfx[j]) { seg = (uint32_t)j; off = e - pfx[j]; }
                        ent_i = (wid * kseg + seg) * a.cap + off;
                    }
                    const Pack4<T> *ent = a.mesh_list + 3 * (size_t)ent_i;
                    const Pack4<T> A = ent[0], B = ent[1], C = ent[2];
                    const Vec<T> o_ = mk<T>(A.x, A.y, A.z), d_ = mk<T>(A.w, B.x, B.y);
                    T t0;
                    if (bvh8_enter<T>(sc, o_, d_, C.y, ry, t0)) { bvh8_begin<T>(wk, ry, t0, (T)0.001, sc.bvh_root[2].w); dxf = (float)d_.x; dyf = (float)d_.y; dzf = (float)d_.z; walking = true; }
                    else { wk.nc = 0; finished = true; }
                }
                next += take;
                if (!__any(walking)) { if (__any(finished)) continue; break; }
                // ---- walk; leave the loop when enough lanes are free for a refill to pay (or, with the list exhausted, when all are done), or a list is full
                const bool more = next < mfill;
                uint32_t n_now = (uint32_t)__popcll(__ballot(walking));
                while (true) {
                    ++n_wtrips; n_ltrips += n_now;
                    if (walking) {
                        const int st_ = bvh8_step_screened<kLdsStack>(sc.bvh_nodes, sc.bvh_tris32, wk, ry, dxf, dyf, dzf, lstack, stack, lane);
                        if (st_ == kWalkDone) { walking = false; finished = true; }
                        else if (st_ == kWalkFull) full = true;
                    }
                    const uint32_t n_walk = (uint32_t)__popcll(__ballot(walking));
                    n_now = n_walk;
                    if (n_walk == 0 || (more && 64u - n_walk >= a.refill_free) || __any(full)) break;
                }
            }
            } else {
            bool walking = false, finished = false;                    // finished: a result waits to be emitted
            Vec<T> o_ = mk<T>(0, 0, 0), d_ = mk<T>(0, 0, 1), beta_ = mk<T>(0, 0, 0);
            T closest = 0; uint32_t q_ = 0, stage_hit = 0, slot = 0; int prim = -1;
            Bvh8Ray ry; ry.ox = ry.oy = ry.oz = 0; ry.ix = ry.iy = ry.iz = 1; ry.oct = 0; ry.best = 0; ry.tmin = 0; ry.amin = 0;
            Bvh8Walk<T> wk; wk.G = 0; wk.tw = 0; wk.rank = 0; wk.sp = 0; wk.t0 = 0; wk.c0 = wk.c1 = wk.c2 = wk.c3 = 0; wk.nc = 0;
            while (true) {
                // ---- emit what is finished, refill the free lanes (wave-uniform block)
                const unsigned long long mh = __ballot(finished && prim >= 0);
                if (finished) {
                    if (prim < 0) {                                   // the ray leaves the scene after all: sky, :365-366
                        const uint32_t qi = q_ & 0x7FFFFFFFu;
                        ExtState<T> ex1; ex1.flags = rc.flags; ex1.bR = 0; ex1.bG = 0; ex1.bB = 0;
                        if (EXT && (rc.flags & kExtSpectral)) {
                            uint32_t pi, pj, pixel, sample;
                            path_of<T>(rc, qi, a.pass, pi, pj, pixel, sample);
                            (void)ext_wavelength<T>(sc, rc.sA, rc.sB, pixel, sample, ex1);
                        }
                        const Vec<T> c = sky_term_x<T, EXT>(d_, beta_, &ex1);
                        Pack3<T> l; l.x = c.x; l.y = c.y; l.z = c.z;
                        if (q_ >> 31) { const Pack3<T> l0 = a.L[qi]; l.x = l0.x + c.x; l.y = l0.y + c.y; l.z = l0.z + c.z; ++n_rmw; }
                        else ++n_store;
                        a.L[qi] = l;
                    } else {
                        const Vec<T> hp = o_ + d_ * closest;          // point_at, :138 / :183
                        const uint32_t w_ = ((prim >= (int)ref_base) ? ref_base + slot : (uint32_t)prim) | (stage_hit << kStageShift);
                        const uint32_t dst = region + fill + __popcll(mh & lt_mask);
                        Pack4<T> A, B; Pack2<T> C;
                        A.x = hp.x; A.y = hp.y; A.z = hp.z; A.w = d_.x;
                        B.x = d_.y; B.y = d_.z; B.z = beta_.x; B.w = beta_.y;
                        C.x = beta_.z; C.y = pack_qref(q_, w_, (T)0);
                        qout.A[dst] = A; qout.B[dst] = B; qout.C[dst] = C;
                        if constexpr (kRefArray) rout[dst] = w_;
                    }
                }
                fill += (uint32_t)__popcll(mh);
                finished = false;
                const unsigned long long mf = __ballot(!walking);
                const uint32_t take = min((uint32_t)__popcll(mf), mfill - next);
                if (!walking && (uint32_t)__popcll(mf & lt_mask) < take) {
                    const uint32_t e = next + (uint32_t)__popcll(mf & lt_mask);
                    const Pack4<T> *ent = mlist + 3 * (size_t)e;
                    if (segmented) {                               // entry e of the k lists taken over: which list, which entry of it
                        uint32_t seg = 0, off = e;
#pragma unroll
                        for (int j = 1; j < kMaxSeg; ++j) if (e >= pfx[j]) { seg = (uint32_t)j; off = e - pfx[j]; }
                        ent = a.mesh_list + 3 * ((size_t)(wid * kseg + seg) * a.cap + off);
                    }
                    const Pack4<T> A = ent[0], B = ent[1], C = ent[2];
                    o_ = mk<T>(A.x, A.y, A.z); d_ = mk<T>(A.w, B.x, B.y); beta_ = mk<T>(B.z, B.w, C.x);
                    closest = C.y;
                    q_ = Bits<T>::to_u32(C.z);
                    const uint32_t pw = Bits<T>::to_u32(C.w);
                    prim = (int)(pw & kRefMask) - 1;
                    stage_hit = pw >> kStageShift;
                    slot = 0;
                    T t0;
                    if (bvh8_enter<T>(sc, o_, d_, closest, ry, t0)) { bvh8_begin<T>(wk, ry, t0, (T)0.001, sc.bvh_root[2].w); walking = true; }
                    else finished = true;
                }
                next += take;
                if (!__any(walking)) { if (__any(finished)) continue; break; }
                // ---- walk; leave the loop when enough lanes are free for a refill to pay (or, with the list exhausted, when all are done)
                const bool more = next < mfill;
                MESH_STAT(++dbg_rf; const unsigned long long dbg_w0 = __builtin_readcyclecounter();)
                uint32_t n_now = (uint32_t)__popcll(__ballot(walking));
                while (true) {
                    ++n_wtrips; n_ltrips += n_now;
                    MESH_STAT(++dbg_ws; { const uint32_t nl = (uint32_t)__popcll(__ballot(walking)); dbg_ls += nl; if (segmented) { ++dbg_ws1; dbg_ls1 += nl; } ++dbg_h[nl <= 8 ? 0 : (nl <= 24 ? 1 : (nl <= 48 ? 2 : 3))]; })
                    if (walking && !bvh8_step<T, kLdsStack>(sc, wk, ry, o_, d_, (T)0.001, (int)ref_base, closest, prim, slot, lstack, stack, lane)) { walking = false; finished = true; }
                    const uint32_t n_walk = (uint32_t)__popcll(__ballot(walking));
                    n_now = n_walk;
                    if (n_walk == 0 || (more && 64u - n_walk >= a.refill_free)) break;
                }

                MESH_STAT(dbg_walk += __builtin_readcyclecounter() - dbg_w0;)
            }
            }
            mfill = 0;
            segmented = false;                                         // from here on the list is the wave's own (the lists taken over are spent)
            MESH_STAT(dbg_sess += __builtin_readcyclecounter() - dbg_s0;)
        }
        n_in = fill;
        n_enq += fill;
        if (n_in == 0 && (mfill == 0 || mesh_mode == 1u)) break;      // wave-uniform: every path of this wave has ended (mode 1: or rests on the list)
        // The wave now reads what its own lanes have just written: on one CU (one vector L1, one L2) a workgroup-scope
        // release/acquire (wait for the stores) is all that takes.  No other wave ever touches this region.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    for (int sft = 32; sft > 0; sft >>= 1) { n_rmw += __shfl_down(n_rmw, sft); n_seg += __shfl_down(n_seg, sft); n_store += __shfl_down(n_store, sft); }
    const bool again = SPEC && __any(outside_window<T>(pol));    // some quotient of this wave may not be the IEEE one: the exact launch redoes the wave
    if (own && !again && !(SPEC && a.redo_only == 2u)) {        // (a wave rendered again resolves in the exact launch: accum is added to once)
#if SPIRA_PATH_FIXED
        // k_path_own makes its lane index again for this block (mbcnt; it shadows the kernel's `lane`), so that nothing of it is held through the loop:
        // carried, lane / RUN cost the speculative kernel its only scratch.  The preprocessor and not a `FIXED ?` alias: with an alias in k_path's text
        // five Float32 mesh instantiations came out with exchanged operands in two scalar adds (docs/experiments.md §45); this way k_path's tokens are untouched.
        const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#endif
        // Every path of this wave's pixels has ended, and only this wave's lanes stored their radiance: as for the queue region above, waiting
        // for the stores (workgroup-scope release) is all that takes on one CU — no other CU ever wrote these bytes.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint32_t px = owned_pixel(wid, NW, lane);
        bool summed = false;                                     // the pixel of an all-sky run: its sum is ready, in its slot-0 entry
        if constexpr (kOwnT) sky_mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)*sky_word);
        if constexpr (kOwnT) summed = ((sky_mask >> (lane / SPIRA_RESOLVE_RUN)) & 1u) != 0;
        if (summed) {
            const Pack3<T> l = a.L[priv ? l_base + (lane / SPIRA_RESOLVE_RUN) * (FIXED ? 64u : a.k_eff) * SPIRA_RESOLVE_RUN + lane % SPIRA_RESOLVE_RUN : px];
            Pack4<T> acc;
            if (a.accum_first) acc.w = 0; else acc = a.accum[px];
            acc.x = l.x; acc.y = l.y; acc.z = l.z;
            a.accum[px] = acc;
        } else if (px < rc.tile_pixels) {
            if (priv) resolve_pixel_run<T>(a.accum, a.L + l_base + (lane / SPIRA_RESOLVE_RUN) * (FIXED ? 64u : a.k_eff) * SPIRA_RESOLVE_RUN + lane % SPIRA_RESOLVE_RUN, (FIXED ? 64u : a.k_eff), a.accum_first != 0, px);
            else resolve_pixel<T>(a.accum, a.L, rc.tile_pixels, a.k_eff, a.accum_first != 0, px);      // (slot-major L: never with FIXED)
        }
        // k_resolve's fold of the statistics rows, one wave instruction: lane i adds counter i (Stats' first four fields)
        const uint32_t seg = __shfl(n_seg, 0), rmw = __shfl(n_rmw, 0), sto = __shfl(n_store, 0);
        // (lane 4, where the wave summed sky runs: their pixels, in the same instruction)
        if (lane < 4 || (kOwnT && lane == 4 && sky_mask)) {
            unsigned long long *f = lane == 0 ? &a.stats->segments : (lane == 1 ? &a.stats->rays_enqueued : (lane == 2 ? &a.stats->radiance_rmw : (lane == 3 ? &a.stats->radiance_store : &a.stats->sky_pixels)));
            atomicAdd(f, (unsigned long long)(lane == 0 ? seg : (lane == 1 ? n_enq : (lane == 2 ? rmw : (lane == 3 ? sto : SPIRA_RESOLVE_RUN * (uint32_t)__popc(sky_mask))))));
        }
    }
    MESH_STAT(if (lane == 0) { unsigned long long *g = g_mesh_dbg + (mesh_mode == 2u ? 16 : 0);
                               atomicAdd(&g[0], __builtin_readcyclecounter() - dbg_t0); atomicAdd(&g[1], dbg_sess); atomicAdd(&g[2], (unsigned long long)dbg_ns);
                               atomicAdd(&g[3], (unsigned long long)dbg_ws); atomicAdd(&g[4], (unsigned long long)dbg_ls); atomicAdd(&g[5], (unsigned long long)dbg_rf);
                               atomicAdd(&g[6], (unsigned long long)dbg_rays); atomicAdd(&g[7], (unsigned long long)dbg_rounds); atomicAdd(&g[9], dbg_walk); atomicAdd(&g[10], 1ull); atomicAdd(&g[11], (unsigned long long)dbg_ws1); atomicAdd(&g[12], (unsigned long long)dbg_ls1);
                               atomicAdd(&g[8], (unsigned long long)dbg_h[0]); atomicAdd(&g[13], (unsigned long long)dbg_h[1]); atomicAdd(&g[14], (unsigned long long)dbg_h[2]); atomicAdd(&g[15], (unsigned long long)dbg_h[3]); })
    if (lane == 0) {
        if (mesh_mode == 2u) {                     // on top of what the first launch's wave left in the row
            const uint32_t row = 4 * wid * kseg;
            a.blk_stats[row] += n_seg; a.blk_stats[row + 1] += n_rmw; a.blk_stats[row + 2] += n_store; a.blk_stats[row + 3] += n_enq;
        } else {
            a.blk_stats[4 * wid] = n_seg;
            a.blk_stats[4 * wid + 1] = n_rmw;
            a.blk_stats[4 * wid + 2] = n_store;
            a.blk_stats[4 * wid + 3] = n_enq;          // wave-uniform
            if (mesh_mode == 1u) a.mesh_count[wid] = mfill;
        }
        if (SPEC) a.redo[wid] = again ? 1u : 0u;
        if (BVH && n_park && !again && !(SPEC && a.redo_only == 2u)) atomicAdd(&a.stats->rays_parked, (unsigned long long)n_park);      // (a wave rendered again counts there)
        if (BVH && mesh_mode != 1u && n_wtrips && !again && !(SPEC && a.redo_only == 2u)) { atomicAdd(&a.stats->mesh_wave_trips, (unsigned long long)n_wtrips); atomicAdd(&a.stats->mesh_lane_trips, (unsigned long long)n_ltrips); }
    }
