// The body of bt_render_kernel (bt_kernels.hip), included by the kernel template and by its sphere-only specialisations, which
// are the same code under kernel attributes of their own.  In scope where it is included: the launch parameters `BtLaunch P`
// and the constants OUTPUT, LENS, RECTS, VOLS, PACKED (bt_kernels.hip says what they select).
    // ---- a block whose camera rays provably reach no sphere (sphere-only builds without volumes; DESIGN.md 5.15) ----
    // bt_block_mask_kernel has written which sphere rows each block's camera rays can reach and bt_block_order_kernel has
    // listed the blocks that reach any ahead of those that reach none.  The kernel reads the list, not the masks: two
    // wave-uniform (scalar) loads ahead of the LDS staging and its barrier, which the empty blocks do not need (see `bid`
    // below).  The Normal output's miss value depends on the direction and is not shortcut.
    constexpr bool GUIDED = OUTPUT == 4;   // every statement of the guided builds sits behind this constant
    constexpr bool ADAPT = OUTPUT == 5;    // ... and every statement of the adaptive builds behind this one
    constexpr bool AOV = OUTPUT != 0 && !ADAPT;    // the build keeps a path's first hit (the adaptive builds are Full builds)
    constexpr bool CULL = !LENS && !RECTS && !VOLS && !PACKED && OUTPUT != 2 && !GUIDED && !ADAPT;   // (a guided launch writes the Normal output too)
    // The sphere-only builds without volumes, lens or packing (outputs 0 ... 3) keep wave-uniform values out of the SGPR file
    // where that is free (BT_SGPR_DIET, DESIGN.md 5.16): same operations on every (lane, sample), other operand homes.
    constexpr bool DIET = BT_SGPR_DIET && !LENS && !RECTS && !VOLS && !PACKED && OUTPUT <= 3;
    // ---- adaptive sampling: a tile that has converged (DESIGN.md 13) ----
    // bt_adapt_update_kernel has cleared tile_active[tile] once the tile's error estimate fell below the threshold: one
    // wave-uniform (scalar) load ahead of the LDS staging, as the empty-block test below, and read through the same opaque
    // pointer so that nothing of it stays in SGPRs.  The tile's pixels, moments and the segment counter stay untouched.
    if (ADAPT) {
        typedef const __attribute__((address_space(4))) BtLaunch BtLaunchK;
        typedef const __attribute__((address_space(4))) uint32_t ActiveK;
        BtLaunchK *C = (BtLaunchK *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(C));
        const uint32_t slot = blockIdx.x >> (uint32_t)__builtin_ctz((uint32_t)C->slices);
        if (((ActiveK *)C->tile_active)[slot] == 0u) return;
    }
    // Which block this workgroup traces.  The CULL builds take the launch's blocks in bt_block_order_kernel's order: workgroup w <
    // n_live traces the w-th block with a non-zero mask (so the sky at the top of a frame does not hold the first half of the
    // grid); the next ceil(n_empty / slices) workgroups fill `slices` empty blocks each, 256 pixels for 256 threads; the rest
    // of the grid returns at once -- it is dispatched last, while the traced workgroups drain.  Nothing depends on the order
    // in which the hardware starts workgroups.
    uint32_t bid = blockIdx.x;
    if (CULL && P.max_bounces >= 0) {              // (max_bounces < 0 ends every path before its first TRACE: plain launch order)
        // Header, order and everything the fill reads come through a pointer the compiler cannot see through (as the camera
        // event below does): sharing block_ref() and the like with the code after it kept their inputs in SGPRs across
        // this branch, and the loop paid with 18 more spill reloads per iteration (profiles/r10).
        typedef const __attribute__((address_space(4))) BtLaunch BtLaunchK;
        typedef const __attribute__((address_space(4))) uint32_t OrderK;
        BtLaunchK *C = (BtLaunchK *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(C));
        OrderK *ord = (OrderK *)C->block_order;
        const uint32_t n_live = ord[0];
        if (blockIdx.x >= n_live) {
            const uint32_t n_empty = ord[1], log_ns = (uint32_t)__builtin_ctz((uint32_t)C->slices);
            const uint32_t fw = blockIdx.x - n_live;                          // which fill workgroup
            if (fw >= (n_empty + (1u << log_ns) - 1u) >> log_ns) return;
            fill_empty_blocks<OUTPUT>(*(const BtLaunch *)C, (const uint32_t *)C->block_order + BT_ORDER_HEADER + n_live, fw << log_ns, n_empty);
            return;
        }
        bid = ord[BT_ORDER_HEADER + blockIdx.x];
    }
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ uint32_t s_waves_done;      // block queue: waves of this workgroup that have parked all their samples
    __shared__ uint32_t s_next_item;       // the workgroup's work queue (next unclaimed (pixel, sample) pair)
    __shared__ uint32_t s_segments;        // path segments traced by this workgroup
    __shared__ uint32_t s_pool_paths[2], s_pool_waves[2];   // packed builds, drain rounds: live paths / waves that hold any (two sets, alternating)
    if (threadIdx.x == 0) {
        s_waves_done = 0;
        s_next_item = 0;
        s_segments = 0;
        if (PACKED && RECTS && !VOLS && OUTPUT == 0) s_pool_paths[0] = s_pool_paths[1] = s_pool_waves[0] = s_pool_waves[1] = 0;
    }

    // ---- stage the per-lane lookup tables in LDS ----
    SceneLds S;
    {
        unsigned char *p = smem;
        BtPrimLite *lite = (BtPrimLite *)p;        p += sizeof(BtPrimLite) * P.n_prims;
        BtMaterial *mats = (BtMaterial *)p;        p += sizeof(BtMaterial) * P.n_materials;
        BtVolume *vols = (BtVolume *)p;            p += sizeof(BtVolume) * P.n_volumes;
        BtLight *lights = (BtLight *)p;            p += sizeof(BtLight) * P.n_lights;
        BtLightFace *faces = (BtLightFace *)p;     p += sizeof(BtLightFace) * P.n_light_faces;
        float *dens = (float *)p;
        for (int i = threadIdx.x; i < P.n_prims; i += blockDim.x) {
            const BtPrim &R = P.prims[i];
            BtPrimLite l;
            l.c = R.c;
            l.radius = R.radius;
            l.kind_object = (R.kind & BT_PRIM_SHAPE_MASK) | (R.object << 8);
            l.material = R.material;
            l.volume = R.volume;
            l.rcp_radius = ((R.kind & BT_PRIM_SHAPE_MASK) == BT_PRIM_SPHERE && R.radius >= 0x1p-20f && R.radius <= 0x1p20f) ? refined_rcp(R.radius) : 0.0f;
            lite[i] = l;
        }
        for (int i = threadIdx.x; i < P.n_materials; i += blockDim.x) mats[i] = P.materials[i];
        for (int i = threadIdx.x; i < P.n_volumes; i += blockDim.x) vols[i] = P.volumes[i];
        for (int i = threadIdx.x; i < P.n_lights; i += blockDim.x) lights[i] = P.lights[i];
        for (int i = threadIdx.x; i < P.n_light_faces; i += blockDim.x) faces[i] = P.light_faces[i];
        const bool dens_lds = P.n_density > 0 && P.n_density <= BT_DENSITY_LDS_MAX;
        if (dens_lds)
            for (int i = threadIdx.x; i < P.n_density; i += blockDim.x) dens[i] = P.density[i];
        S.lite = lite; S.materials = mats; S.volumes = vols; S.lights = lights; S.faces = faces;
        S.density = dens_lds ? dens : P.density;
        __syncthreads();
    }
    BtVolBox *const vbox = (BtVolBox *)(smem + P.table_lds_bytes);      // VOLS builds: bt_types.h BtVolBox, one per primitive
    if (VOLS && P.vbox_lds_bytes) {
        for (int i = threadIdx.x; i < P.n_prims; i += blockDim.x) {
            const BtPrim &R = P.prims[i];
            BtVolBox bx;
            const V3 c = mk(R.c), hsz = mk(R.radius, R.radius, R.radius);
            const V3 bmin = c - hsz, bmax = c + hsz, size = bmax - bmin;            // sphere.rs:35-38, volume.rs:29-31
            bx.bmin.x = bmin.x; bx.bmin.y = bmin.y; bx.bmin.z = bmin.z;
            bx.size.x = size.x; bx.size.y = size.y; bx.size.z = size.z;
            bx.rcp.x = refined_rcp(size.x); bx.rcp.y = refined_rcp(size.y); bx.rcp.z = refined_rcp(size.z);
            const bool ok = size.x >= 0x1p-20f && size.x <= 0x1p20f && size.y >= 0x1p-20f && size.y <= 0x1p20f &&
                            size.z >= 0x1p-20f && size.z <= 0x1p20f;
            bx.ok = ok ? 1.0f : 0.0f;
            bx.pad0 = bx.pad1 = 0.0f;
            vbox[i] = bx;
        }
        __syncthreads();
    }

    // ---- tile / pixel mapping ----
    // A workgroup owns one pixel block of pxb = 256 / slices pixels (block_ref() above): its pxb * T (pixel, sample) pairs are
    // work items i = k * pxb + pixel, handed out through an LDS counter (one atomic per wave and iteration, see the loop)
    // -- a lane whose path has ended takes the next item, so all 256 lanes stay busy until the block's samples run out, and
    // 64 consecutive items are the same sample of neighbouring pixels (coherent camera rays).  Every sample's value is
    // parked at scratch[block * pxb * T + i]; the last wave to finish adds them to the frame in sample order (end of the
    // kernel).
    const BlockGeom G = block_geom(P);
    const uint32_t pxb = G.pxb, LOG_PXB = G.LOG_PXB;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nn = (uint32_t)(P.subsample_n * P.subsample_n);
    const uint32_t T = (uint32_t)P.samples * nn;       // samples per pixel in this launch
    const uint32_t sample0 = P.sample_base * nn;
    // block queue: this workgroup's one block (`bid` above) -- or, in a packed launch (wg_blocks > 1: gridDim.x
    // workgroups for the launch's blocks), the blocks blockIdx.x, blockIdx.x + gridDim.x, ... behind ONE queue: item
    // i = ((j << log_rows | k) << LOG_PXB) + pixel for sample k of the workgroup's j-th block (rows k >= T are holes: T is
    // padded to a power of two so that neither j nor k costs a division)
    constexpr bool packed = PACKED;
    const uint32_t my_blocks = packed ? P.wg_blocks - (blockIdx.x < P.wg_blocks_rem ? 0u : 1u) : 1u;
    const uint32_t n_items = packed ? (my_blocks << (P.log_rows + LOG_PXB)) : pxb * T;      // work items of this workgroup
    const BlockRef B_own = block_ref(P, G, bid);
    // where this workgroup parks: every workgroup of a packed launch has room for wg_blocks blocks
    auto park = [&]() -> Parked * {
        return (Parked *)P.scratch + (size_t)bid * (packed ? (size_t)P.wg_blocks << (P.log_rows + LOG_PXB) : (size_t)n_items);
    };

    // the lane's current work item: pixel_index keys the Philox counter; park_i = the item's number i = k * pxb + pixel in
    // the block, where its value is parked (+ the workgroup's base; the sample number k comes out of it, one register less
    // than keeping both)
    uint32_t px = 0, py = 0, pixel_index = 0, park_i = 0;

    // per-lane path state
    V3 ro = mk(0, 0, 0), rd = mk(0, 0, -1), beta = mk(1, 1, 1), L = mk(0, 0, 0);
    V3 first = mk(0, 0, 0);            // first non-pass-through albedo / normal (AOV outputs)
    float first_depth = __builtin_inff();
    bool have_first = false;
    int bounce = 0, vbounce = 0, last_object = -1;
    uint32_t event = 0;
    bool pending = true;               // the lane has no ray yet: its next event is the camera ray
    // phase voting (BtLaunch::phase_vote): a lane whose scatter event lost the vote keeps its hit for the next iteration
    constexpr bool VOTE = !RECTS && !LENS;    // pays where the events, not TRACE, are most of an iteration
    bool held = false;
    float held_t = 0.0f;
    int held_info = 0, waited = 0;     // held_info = prim | inside << 29 | p_neg << 30
    // path segments of this lane (bt_stats::segments): counted in 32 bits per lane and added up per workgroup in LDS --
    // one device atomic per workgroup, issued by the wave that sums the block.  (A lane sees at most
    // scratch cap / 12 B / 256 items per launch and bt_api.cpp keeps items x longest path below 2^32 per workgroup.)
    uint32_t segments = 0;
    unsigned long long lens_steps = 0;
    LensState lens;                    // lens extension: the bent segment in progress (LENS builds only)
    bool bent = false;
    lens_begin(P, lens);

    // mod.rs:304-315 -> Chunk::write_* -> Buffer::write_* (buffer.rs:159-178): one sample is done
    // Guided builds: the sample's albedo / normal / depth values are parked by the ONE event that sets have_first, straight from
    // the registers that event holds -- nothing but the flag is carried to the end of the path (seven more live floats would
    // cost the rect build a wave per SIMD and the volume builds spills).  A guide without a frame is neither parked nor summed;
    // the pointers are read where they are used, through a pointer the compiler cannot see through (as the camera block is).
    auto park_guides = [&](const V3 &albedo, const V3 &nrm, float first_t) {
        typedef const __attribute__((address_space(4))) BtLaunch BtLaunchK;
        BtLaunchK *C = (BtLaunchK *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(C));
        const size_t at = (size_t)bid * (packed ? (size_t)P.wg_blocks << (P.log_rows + LOG_PXB) : (size_t)n_items) + park_i;
        if (C->guide_out[0]) ((Parked *)C->guide_scratch[0])[at] = Parked{albedo.x, albedo.y, albedo.z};
        if (C->guide_out[1]) ((Parked *)C->guide_scratch[1])[at] = Parked{nrm.x, nrm.y, nrm.z};
        if (C->guide_out[2]) {
            float depth = (first_t - P.clip_min) / (P.clip_max - P.clip_min);     // finish_sample's OUTPUT == 3 arithmetic
            depth = fminf(fmaxf(depth, 0.0f), 1.0f);
            ((Parked1 *)C->guide_scratch[2])[at] = Parked1{depth};
        }
    };
    // (a path that ends without have_first parks ColorData's defaults; called next to finish_sample, not from inside it, so
    // that the lambda below captures what it always captured)
    auto park_guide_defaults = [&]() { park_guides(mk(0, 0, 0), mk(0, 0, 0), __builtin_inff()); };
    auto finish_sample = [&]() {
        V3 value;
        if (OUTPUT == 0 || GUIDED || ADAPT) {
            value = L;
        } else if (OUTPUT == 3) {
            float depth = (first_depth - P.clip_min) / (P.clip_max - P.clip_min);
            depth = fminf(fmaxf(depth, 0.0f), 1.0f);
            value = mk(depth, depth, depth);
        } else {
            value = first;
        }
        park()[park_i] = Parked{value.x, value.y, value.z};
    };

    // Packed builds, the drain (BtLaunch::pool_records > 0): once the queue is empty the workgroup's waves meet at the end of every
    // iteration, put the paths still in flight into LDS records and take them back densely packed -- waves 1 .. 3 run out of
    // paths and stop issuing instructions for a handful of live lanes each.  Scheduling only: a path's state moves between lanes,
    // its operations and their order do not change.  Every wave takes part in every round (barriers pair up by count) until
    // a round finds no path left.
    PathRec *const pool = (PathRec *)(smem + P.pool_lds_offset);
    // Compiled into the rect build only: measured (profiles/r04y), it takes 4 - 14 % off packed Cornell-box launches and nothing off
    // sphere and volume launches (short drains; marches), whose builds its code made ~5 % slower.
    constexpr bool CAN_COMPACT = PACKED && RECTS && !VOLS && OUTPUT == 0;    // (a PathRec carries no first-hit AOV state)
    const bool compacting = CAN_COMPACT && P.pool_records > 0;
    bool dry_lane = false;             // this lane found the queue empty
    uint32_t drain_it = 0;             // iterations since the wave saw the queue empty (wave-uniform)

    // DIET builds (DESIGN.md 5.16): the loop's hot uniform floats in VGPRs, copied once per workgroup through a register the
    // compiler cannot see through (a VGPR operand issues at the full rate, an SGPR operand at about half) ...
    float clip_min_v = P.clip_min, clip_max_v = P.clip_max, tau_scale_v = P.tau_scale, one_scale_v = P.one_scale;
    if (DIET) asm volatile("" : "+v"(clip_min_v), "+v"(clip_max_v), "+v"(tau_scale_v), "+v"(one_scale_v));
    // ... and the launch constants with one use per iteration are read from the kernarg segment where they are used, as the
    // camera block is: scalar loads that hit the constant cache instead of SGPRs held (or spilled) across the loop
    auto kargs = [&]() {
        typedef const __attribute__((address_space(4))) BtLaunch BtLaunchK;
        BtLaunchK *C = (BtLaunchK *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(C));
        return C;
    };
    BT_PROF_DECL;
#ifdef BT_LANESTAT
    unsigned long long ls_acc[9] = {};
    const unsigned long long ls_all = __ballot(true);
#endif
    for (;;) {
        do {                                              // (`continue` below = on to the latch at the end of the iteration)
        if (compacting && dry_lane && pending) continue;  // the queue is empty and this lane has no path: nothing to do
        BT_LS(0, 1ull);
        BT_LS(8, ls_all & ~__ballot(true));
        BT_PROF(0);                                       // loop overhead / previous iteration's tail
        int ev = EV_GEN;
        // manifold of this iteration's hit (shading events only)
        V3 pos = ro, normal = mk(0, 0, 0);
        float hit_depth = 0.0f;                         // Manifold.t of the hit, for the Depth output
        bool front = false, inside = false, vol_back = false;
        int pobject = -1, mat_index = 0, vol_index = 0;
        V3 prim_c = mk(0, 0, 0);
        float prim_radius = 0.0f;
        int hit_prim = 0;

        BT_LS(1, __ballot(!pending && !(VOTE && held)));
        if (!pending) {
            // ---- TRACE: try_hit (mod.rs:389-402) / try_hit_volume (mod.rs:404-427) ----
            const bool marching = VOLS && last_object >= 0;
            if (!marching) vbounce = 0;                               // sample() -> sample_volume(.., 0), mod.rs:335
            const float tmin = marching ? 0.0f : (DIET ? clip_min_v : P.clip_min);
            const float tmax = marching ? P.volume_step : (DIET ? clip_max_v : P.clip_max);
            HitRec h;
            bool ended = false, captured = false;
            float travelled = 0.0f;
            if (LENS && !marching) {
                // bent segment, marched BT_LENS_BATCH RK4 steps per iteration: (ro, rd) is the photon; at the
                // end they are the chord that hits, or the ray that reaches the root
                if (!bent) {
                    lens_begin(P, lens);
                    bent = true;
                    segments += 1;
                }
                const int r = lens_advance<RECTS>(P, ro, rd, lens, h, BT_LENS_BATCH, lens_steps);
                if (r == 2) continue;                     // still on its way: no event for this lane yet
                bent = false;
                captured = r < 0;
                travelled = lens.travelled;
            } else if (VOTE && held) {                // the hit found one iteration ago (phase voting; it travels in the path's record)
                h.t = held_t;
                h.prim = held_info & 0x1fffffff;
                h.inside = (held_info >> 29) & 1;
                h.p_neg = (held_info >> 30) & 1;
            } else {
                segments += 1;
                h = intersect<RECTS, VOLS, RECTS && !VOLS && !LENS>(P, ro, rd, tmin, tmax, last_object);
            }
            if (captured) {
                ended = true;                         // swallowed by the horizon: the path returns black
            } else if (h.prim < 0) {
                // sample_root (mod.rs:429-452)
                if (DIET) { const auto *C = kargs(); L = L + beta * mk(C->root_color.x, C->root_color.y, C->root_color.z); }
                else L = L + beta * mk(P.root_color);
                if (AOV && !have_first) {
                    have_first = true;
                    if (OUTPUT == 1) first = mk(P.root_albedo);
                    if (OUTPUT == 2) first = P.root_has_albedo ? -rd : mk(0, 0, 0);
                    if (OUTPUT == 3) first_depth = P.root_has_albedo ? P.clip_max : __builtin_inff();
                    if (GUIDED) park_guides(mk(P.root_albedo), P.root_has_albedo ? -rd : mk(0, 0, 0), P.root_has_albedo ? P.clip_max : __builtin_inff());
                }
                ended = true;
            } else {
                const BtPrimLite &pl = S.lite[h.prim];
                const int pshape = pl.kind_object & 0xff;
                pobject = pl.kind_object >> 8;
                prim_c = mk(pl.c);
                prim_radius = pl.radius;
                hit_prim = h.prim;
                hit_depth = LENS ? h.t + travelled : h.t;
                pos = ro + rd * h.t;
                bool vol_face = false;
                if (VOLS && h.inside) {               // generate_volume_manifold (sphere.rs:63-83)
                    inside = true;
                    vol_face = true;
                } else if (!RECTS || pshape == BT_PRIM_SPHERE) { // generate_surface_manifold (sphere.rs:85-119)
                    // normal = (position - centre) / radius (sphere.rs:95-99): div_refined() with the sphere's refined
                    // reciprocal -- the IEEE quotient's bits while every operand is 0 or within [2^-60, 2^60] (it is ~radius
                    // here); a wave with a lane outside that range divides exactly
                    V3 nrm = pos - prim_c;
                    const float nax = fabsf(nrm.x), nay = fabsf(nrm.y), naz = fabsf(nrm.z), rr = pl.rcp_radius;
                    const bool in_range = (rr != 0.0f) & (nax == 0.0f || (nax >= 0x1p-60f && nax <= 0x1p60f)) &
                                          (nay == 0.0f || (nay >= 0x1p-60f && nay <= 0x1p60f)) & (naz == 0.0f || (naz >= 0x1p-60f && naz <= 0x1p60f));
                    if (__ballot(!in_range) == 0ull)
                        nrm = mk(div_refined(nrm.x, pl.radius, rr), div_refined(nrm.y, pl.radius, rr), div_refined(nrm.z, pl.radius, rr));
                    else
                        nrm = mk(nrm.x / pl.radius, nrm.y / pl.radius, nrm.z / pl.radius);
                    front = dot(rd, nrm) < 0.0f;
                    normal = front ? nrm : -nrm;
                    vol_face = VOLS && pl.volume >= 0;
                    vol_back = vol_face && !front;
                } else {                              // rect.rs:138-142
                    front = h.p_neg;
                    normal = front ? prim_c : -prim_c;
                }
                if (vol_face) {
                    vol_index = pl.volume;
                    ev = EV_VOLUME;                   // sample_volume (mod.rs:488-523)
                } else {
                    // sample_surface (mod.rs:454-486): emitted, then Material::shade
                    mat_index = pl.material;
                    const BtMaterial &M = S.materials[mat_index];
                    if (!(VOTE && held)) L = L + beta * mk(M.emitted);
                    if (M.kind == BT_MAT_DIFFUSE) ev = EV_DIFFUSE;
                    else if (M.kind == BT_MAT_METALLIC) ev = EV_METALLIC;
                    else if (M.kind == BT_MAT_GLASS) ev = EV_GLASS;
                    else {
                        // Flat / Emissive: no scatter -> ColorData::from_emitted (mod.rs:483-485)
                        if (AOV && !have_first) {
                            have_first = true;
                            if (OUTPUT == 1) first = mk(M.emitted);
                            if (GUIDED) park_guides(mk(M.emitted), mk(0, 0, 0), __builtin_inff());
                        }
                        ended = true;
                    }
                }
            }
            if (GUIDED && ended && !have_first) park_guide_defaults();
            if (ended) finish_sample();
            if (VOTE && P.phase_vote && ev != EV_GEN) {       // in case this lane's event loses the vote below
                held_t = h.t;
                held_info = h.prim | ((int)h.inside << 29) | ((int)h.p_neg << 30);
            }
        }
        pending = false;
        if (compacting && dry_lane && ev == EV_GEN) {     // the queue is empty: a lane whose path has just ended is done (and has no vote)
            pending = true;
            continue;
        }

        if (VOTE && P.phase_vote) {
            // ---- which events run this iteration?  The kind more lanes want (camera | scatter / volume step); nobody waits
            // more than max_wait iterations.  Everything here is wave-uniform mask arithmetic on the scalar unit; the lane's
            // verdict is its bit of `served_m`.
            const bool want_gen = ev == EV_GEN;
            const unsigned long long m_gen = __ballot(want_gen), m_sc = __ballot(!want_gen);
            const uint32_t n_gen = popc64(m_gen), n_sc = popc64(m_sc);
            // a lane of the losing side that has waited long enough is served in THIS iteration together with the winners
            // (its whole kind runs, as without the vote) -- the majority does not lose an iteration to it
            const unsigned long long starving = __ballot(waited >= P.phase_vote);
            const bool run_gen = n_gen >= n_sc || (starving & m_gen) != 0;
            const bool run_sc = n_sc > n_gen || (starving & m_sc) != 0;
            const unsigned long long served_m = (run_gen ? m_gen : 0ull) | (run_sc ? m_sc : 0ull);
            const bool served = __builtin_amdgcn_inverse_ballot_w64(served_m);
            BT_LS(7, __ballot(!served));
            if (!served) {
                waited += 1;
                pending = want_gen;                   // no ray yet | the hit stays in held_t / held_info
                held = !want_gen;
                continue;
            }
            waited = 0;
            held = false;
        }

        // ---- a lane whose path has ended (or that has none yet) moves on to its next sample ----
        {
            const unsigned long long need = __ballot(ev == EV_GEN);
            if (need) {                                                   // one LDS atomic for the whole wave
                const int leader = __ffsll((long long)need) - 1;
                uint32_t base = 0;
                if ((int)lane == leader) base = atomicAdd(&s_next_item, popc64(need));
                base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
                if (ev == EV_GEN) {
                    const uint32_t i = base + lanes_below(need);
                    if (i >= n_items) {                                   // the block's samples are all taken
                        if (!compacting) goto queue_empty;                // this lane is done
                        dry_lane = true;                                  // the wave learns of it at the end of the iteration
                        pending = true;
                        continue;
                    }
                    park_i = i;                                           // (+ the workgroup's base, see finish_sample)
                    BlockRef B_i = B_own;
                    bool hole = false;
                    if (packed) {                                         // which of the workgroup's blocks, which row of it
                        const uint32_t row = i >> LOG_PXB;
                        B_i = block_ref(P, G, blockIdx.x + (row >> P.log_rows) * gridDim.x);
                        hole = (row & P.row_mask) >= T;
                    }
                    const PixelRef r = pixel_of(P, G, B_i, i & (pxb - 1u));
                    px = r.px;
                    py = r.py;
                    if (!r.in_frame || hole) {
                        pending = true;                                   // pixel outside the frame (edge tile): skip it
                        continue;
                    }
                    pixel_index = py * (DIET ? kargs()->width : P.width) + px;
                }
            }
        }
        BT_PROF(1);                                       // TRACE + hit classification

        BT_LS(2, __ballot(ev == EV_GEN)); BT_LS(3, __ballot(ev == EV_DIFFUSE)); BT_LS(4, __ballot(ev == EV_METALLIC));
        BT_LS(5, __ballot(ev == EV_GLASS)); BT_LS(6, __ballot(ev == EV_VOLUME));
        // ---- the lane's one random event of this iteration (numerics contract N6) ----
        // block queue: the item's sample number comes out of its item number (one register less than keeping both)
        const uint32_t k_now = packed ? (park_i >> LOG_PXB) & P.row_mask : park_i >> LOG_PXB;
        const uint32_t sample_index = sample0 + k_now;
        uint32_t seed_lo = P.seed_lo, seed_hi = P.seed_hi;
        if (DIET) { const auto *C = kargs(); seed_lo = C->seed_lo; seed_hi = C->seed_hi; }
        const U4 u = DIET ? philox_ukeys(pixel_index, sample_index, ev == EV_GEN ? 0u : event, 0u, seed_lo, seed_hi)
                          : philox(pixel_index, sample_index, ev == EV_GEN ? 0u : event, 0u, P.seed_lo, P.seed_hi);
        // slots of the two angular draws: Metallic [0],[1]; Glass [1],[2]; everything else [2],[3]
        const uint32_t w1 = ev == EV_METALLIC ? u.x : (ev == EV_GLASS ? u.y : u.z);
        const uint32_t w2 = ev == EV_METALLIC ? u.y : (ev == EV_GLASS ? u.z : u.w);
        const float r1 = uniform_sample(w1, 0.0f, DIET ? tau_scale_v : P.tau_scale), r2 = uniform_sample(w2, 0.0f, DIET ? one_scale_v : P.one_scale);
        // Volume::shade's scatter decision (volume.rs:26-35) comes first: a march step that passes through needs no
        // sampled direction, and a wave whose lanes all pass through skips the angular draws below altogether
        bool vol_scatter = false;
        if (VOLS && ev == EV_VOLUME) {
            const float density = P.vbox_lds_bytes ? march_density_box(P, S, vol_index, vbox[hit_prim], pos)
                                                   : march_density(P, S, vol_index, prim_c, prim_radius, pos);
            vol_scatter = density >= 1.0f || bernoulli(u.x, density);
        }
        const bool wave_needs_dir = !VOLS || !BT_SKIP_DIR || __ballot(ev != EV_VOLUME || vol_scatter) != 0ull;
        float sn = 0.0f, cs = 0.0f;
        if (wave_needs_dir) sincos_bt(r1, sn, cs);
        BT_PROF(2);                                       // Philox + shared sin/cos

        V3 new_o = pos, dir = rd;
        bool late_end = false;

        if (ev == EV_GEN) {
            // ---- camera ray (mod.rs:271-302, ray.rs:103-113,126-137) ----
            float u_sub = 0.0f, v_sub = 0.0f;
            if (P.subsample_n > 1) {
                const uint32_t n = (uint32_t)P.subsample_n;
                const uint32_t subpx = k_now % (n * n);
                const float width_sub = 1.0f / (float)n;
                u_sub = (float)(subpx % n) * width_sub;
                v_sub = (float)(subpx / n) * width_sub;
            }
            // The camera block of the launch parameters (~30 dwords) is read from the kernarg segment HERE, through
            // a pointer the compiler cannot see through: otherwise it hoists the loads into the prologue, where
            // they live in SGPRs across the whole loop and push other values out into spills.
            typedef const __attribute__((address_space(4))) BtLaunch BtLaunchK;
            BtLaunchK *C = (BtLaunchK *)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(C));
            const V3 mcx = mk(C->cam_cx.x, C->cam_cx.y, C->cam_cx.z), mcy = mk(C->cam_cy.x, C->cam_cy.y, C->cam_cy.z),
                     mcz = mk(C->cam_cz.x, C->cam_cz.y, C->cam_cz.z);
            const float v0 = (float)py * C->pixel_height - 1.0f;
            const float u0 = (float)px * C->pixel_width - 1.0f;
            const float u_offset = u_sub * C->pixel_width + uniform_sample(u.x, C->jitter_u_lo, C->jitter_u_scale);
            const float v_offset = v_sub * C->pixel_height + uniform_sample(u.y, C->jitter_v_lo, C->jitter_v_scale);
            const float uu = u0 + u_offset, vv = v0 + v_offset;
            const float yrot = C->xfov * 0.5f * -uu;
            const float xrot = C->yfov * 0.5f * -vv;
            float sy, cy, sx, cx;
            sincos_small_bt(yrot, sy, cy);              // |angle| <= fov / 2: k = 0 for every frustum below 90 degrees
            sincos_small_bt(xrot, sx, cx);
            const V3 d_cam = mk(-(cx * sy), sx, -(cx * cy));
            // Affine3A * Ray: origin = translation + 0; direction = normalize(normalize_or_zero(M*d)),
            // the outer normalize being the shared one below
            new_o = mk(C->cam_t.x, C->cam_t.y, C->cam_t.z) + mk(0.0f, 0.0f, 0.0f);
            dir = normalize_or_zero(xf_vector(mcx, mcy, mcz, d_cam));
            if (C->has_focus) {                       // mod.rs:286-299; disk angle = r1, radius = r2
                const V3 d1 = normalize(dir);
                const V3 defocus = (mk(C->disk_x.x, C->disk_x.y, C->disk_x.z) * cs + mk(C->disk_y.x, C->disk_y.y, C->disk_y.z) * sn) * r2;
                const V3 defocus_offset = xf_vector(mcx, mcy, mcz, defocus * C->aperture);
                const float frac_f_z = C->focus / fabsf(d_cam.z);
                new_o = new_o + defocus_offset;
                dir = d1 * frac_f_z - defocus_offset;
            }
            beta = mk(1, 1, 1);
            L = mk(0, 0, 0);
            bounce = 0; vbounce = 0; last_object = -1;
            event = 1;
            have_first = false;
            first = mk(0, 0, 0);
            first_depth = __builtin_inff();
            BT_PROF(3);                                   // camera ray
        } else {
            event += 1;
            // ---- direction sample in the local frame (math/distr.rs) ----
            const BtMaterial &M = S.materials[mat_index];
            int light_index = 0;
            bool to_light = false;
            if (ev == EV_DIFFUSE) {
                light_index = (int)__umulhi(u.x, (uint32_t)(DIET ? kargs()->n_lights : P.n_lights));   // material.rs:106-119
                to_light = bernoulli(u.y, 0.5f);                          // Pdf::Mix (:269-275)
            }
            const bool is_cosine = ev == EV_DIFFUSE && !to_light;
            const bool in_frame_of_normal = is_cosine || ev == EV_METALLIC || ev == EV_GLASS;
            // UnitSphere (distr.rs:10-21), UnitHemisphere (:48-59, z = 1 - r2), Cosine (:86-97)
            V3 v = mk(0.0f, 0.0f, 0.0f);
            if (wave_needs_dir) {
                const float sq = sqrt_bt(is_cosine ? r2 : r2 * (1.0f - r2));
                const float lx_ = (is_cosine ? cs : cs * 2.0f) * sq;
                const float ly_ = (is_cosine ? sn : sn * 2.0f) * sq;
                float lz_ = in_frame_of_normal ? 1.0f - r2 : 1.0f - 2.0f * r2;
                if (is_cosine) lz_ = sqrt_bt(1.0f - r2);
                v = mk(lx_, ly_, lz_);
                if (in_frame_of_normal) {
                    V3 z_axis = normalize(normal), x_axis, y_axis;
                    orthonormal_pair(z_axis, x_axis, y_axis);
                    v = (x_axis * lx_ + y_axis * ly_) + z_axis * lz_;
                }
            }

            if (ev == EV_DIFFUSE) {
                if (to_light) {                                           // Pdf::Light (:262-268)
                    const BtLight &Lt = S.lights[light_index];
                    V3 point;
                    if (Lt.kind == BT_LIGHT_SPHERE) {                     // sphere.rs:40-42
                        point = mk(Lt.centre) + v * Lt.radius;
                    } else if (RECTS && Lt.kind == BT_LIGHT_RECT) {
                        point = face_random_point(S.faces[Lt.face_first], u.z, u.w);
                    } else if (RECTS && Lt.kind == BT_LIGHT_CUBOID) {     // cuboid.rs:47-54
                        const U4 e = philox(pixel_index, sample_index, event - 1u, 1u, P.seed_lo, P.seed_hi);
                        const float chosen = uniform_sample(e.x, 0.0f, Lt.total_scale);
                        int index = 0;
#pragma unroll
                        for (int f = 0; f < 5; ++f)
                            if (Lt.cum[f] <= chosen) index = f + 1;
                        point = face_random_point(S.faces[Lt.face_first + index], u.z, u.w);
                    } else {
                        point = mk(Lt.centre);
                    }
                    dir = point - pos;
                } else {
                    dir = v;                                              // Pdf::Diffuse (:224-230)
                }
            } else if (ev == EV_METALLIC) {                               // :231-239
                dir = reflect(rd, normal) + v * M.roughness;
            } else if (ev == EV_GLASS) {                                  // :240-261
                const float ior = front ? M.inv_ior : M.ior;
                const float cos_theta = fminf(dot(-rd, normal), 1.0f);
                const float sin_theta = sqrt_bt(1.0f - cos_theta * cos_theta);
                const float fr = fresnel(rd, normal, ior);
                V3 base;
                if (ior * sin_theta > 1.0f || bernoulli(u.x, fr))
                    base = reflect(rd, normal);
                else
                    base = refract(rd, normal, ior);
                dir = base + v * M.roughness;
            } else if (VOLS) {
                // ---- Volume::shade (volume.rs:26-60) ----
                if (vol_scatter) {
                    if (inside) new_o = pos - (rd * P.volume_step) * u24(u.y);
                    dir = v;
                    beta = beta * mk(0.8f, 0.8f, 0.8f);
                    if (AOV && !have_first) {
                        have_first = true;
                        if (OUTPUT == 1) first = mk(0.8f, 0.8f, 0.8f);
                        if (OUTPUT == 2) first = normal;
                        if (OUTPUT == 3) first_depth = hit_depth;
                        if (GUIDED) park_guides(mk(0.8f, 0.8f, 0.8f), normal, hit_depth);
                    }
                }                                                         // else pass through: Ray::new(pos, rd)
                if (vol_back) {                                           // mod.rs:504-505
                    bounce += 1;
                    last_object = -1;
                } else {                                                  // mod.rs:507-513
                    last_object = pobject;
                    vbounce += 1;
                }
            }
        }

        BT_PROF(4);                                       // scatter direction / volume step
        // Ray::new normalizes (ray.rs:96-101); for the camera this is the last normalize of mod.rs:296-301
        const V3 nd = normalize(dir);

        if (ev == EV_DIFFUSE || ev == EV_METALLIC || ev == EV_GLASS) {
            const BtMaterial &M = S.materials[mat_index];
            bool scatter = true;
            float weight = 1.0f;                                          // material.pdf / shade.pdf
            if (ev == EV_DIFFUSE) {
                const BtLight &Lt = S.lights[(int)__umulhi(u.x, (uint32_t)P.n_lights)];
                const float pd = dot(normal, nd) * 0.318309886183790671538f;   // diffuse_pdf (:301-303)
                const float plight = P.n_lights == 1 ? light_pdf_only_light<RECTS>(P, S, pos, nd) : light_pdf<RECTS>(P, Lt, S, pos, nd);
                const float p = lerpf(pd, plight, 0.5f);                  // :294-296
                scatter = !(fabsf(p) <= 1e-5f);                           // Pdf::pdf (:279-286)
                weight = pd / p;                                          // Material::pdf (:204) / shade.pdf
            }
            if (AOV && !have_first) {
                have_first = true;
                if (scatter) {      // data.albedo ColorData (material.rs:99-104,140-145,169-174)
                    if (OUTPUT == 1) first = mk(M.albedo);
                    if (OUTPUT == 2) first = normal;
                    if (OUTPUT == 3) first_depth = hit_depth;
                    if (GUIDED) park_guides(mk(M.albedo), normal, hit_depth);
                } else {            // ColorData::from_emitted(emitted) (mod.rs:483-485)
                    if (OUTPUT == 1) first = mk(M.emitted);
                    if (GUIDED) park_guides(mk(M.emitted), mk(0, 0, 0), __builtin_inff());
                }
            }
            if (scatter) {
                beta = beta * (mk(M.albedo) * weight);
                bounce += 1;
                last_object = -1;
            } else {
                late_end = true;
            }
        }
        ro = new_o;
        rd = nd;

        // sample() / sample_volumetric() return black past the limits (mod.rs:323-325, 352-354):
        // the path ends before its next TRACE
        if (!late_end) late_end = (VOLS && last_object >= 0) ? (vbounce > P.max_volume_bounces) : (bounce > P.max_bounces);
        if (late_end) {
            if (GUIDED && !have_first) park_guide_defaults();
            finish_sample();
            pending = true;
        }
        BT_PROF(5);                                       // normalize, pdf weight (light_pdf), bookkeeping
        } while (0);
        // ---- the latch: every lane of the wave passes here once per iteration, together -- the drain rounds of the packed builds
        // contain barriers, so they must not sit where lanes that skip the body could run ahead of the others (at the top of the
        // loop the compiler split `round; if (no path) continue;` off as an inner loop of its own: a wave's idle lanes then met
        // the barrier alone, again and again)
        if (compacting && __ballot(dry_lane) != 0ull) {                   // wave-uniform: the queue is empty
            dry_lane = true;
            {                                                             // a round per iteration (every 2nd: +0.7 %, every 4th: +2 %; profiles/r04z, r05x)
                const uint32_t set = drain_it & 1u;
                const bool alive = !pending;                              // a path in flight (possibly holding its hit for the vote)
                const unsigned long long m = __ballot(alive);
                uint32_t base = 0;
                if (lane == 0) {
                    base = atomicAdd(&s_pool_paths[set], popc64(m));
                    if (m) atomicAdd(&s_pool_waves[set], 1u);
                }
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                const uint32_t slot = base + lanes_below(m);
                if (alive && slot < P.pool_records) {
                    PathRec r;
                    r.f[0] = ro.x; r.f[1] = ro.y; r.f[2] = ro.z; r.f[3] = rd.x; r.f[4] = rd.y; r.f[5] = rd.z;
                    r.f[6] = beta.x; r.f[7] = beta.y; r.f[8] = beta.z; r.f[9] = L.x; r.f[10] = L.y; r.f[11] = L.z;
                    r.w[0] = event; r.w[1] = pixel_index; r.w[2] = park_i;
                    r.w[3] = (uint32_t)bounce | ((uint32_t)vbounce << 16);
                    r.w[4] = ((uint32_t)(last_object + 1) & 0xffffffu) | ((uint32_t)waited << 24) | (held ? 0x80000000u : 0u);
                    r.w[5] = __float_as_uint(held_t); r.w[6] = (uint32_t)held_info; r.w[7] = 0u;
                    pool[slot] = r;
                }
                __syncthreads();
                const uint32_t total = *(volatile uint32_t *)&s_pool_paths[set], holders = *(volatile uint32_t *)&s_pool_waves[set];
                if (threadIdx.x == 0) { s_pool_paths[set ^ 1u] = 0; s_pool_waves[set ^ 1u] = 0; }   // next round's set: last read a round ago
                if (total == 0u) break;                                   // no path left in the workgroup: every wave leaves here
                if (total <= P.pool_records && holders > (total + 63u) / 64u) {   // the paths fit fewer waves than hold them now
                    pending = threadIdx.x >= total;
                    if (!pending) {
                        const PathRec r = pool[threadIdx.x];
                        ro = mk(r.f[0], r.f[1], r.f[2]); rd = mk(r.f[3], r.f[4], r.f[5]);
                        beta = mk(r.f[6], r.f[7], r.f[8]); L = mk(r.f[9], r.f[10], r.f[11]);
                        event = r.w[0]; pixel_index = r.w[1]; park_i = r.w[2];
                        bounce = (int)(r.w[3] & 0xffffu); vbounce = (int)(r.w[3] >> 16);
                        last_object = (int)(r.w[4] & 0xffffffu) - 1; waited = (int)((r.w[4] >> 24) & 0x7fu); held = (r.w[4] >> 31) != 0u;
                        held_t = __uint_as_float(r.w[5]); held_info = (int)r.w[6];
                    }
                }
                __syncthreads();                                          // records are read before the next round overwrites them
            }
            drain_it += 1u;
        }
    }
queue_empty:;

    // ---- the end of a workgroup --------------------------------------------------------------------------------------
    // Block queue: the last wave of the workgroup to get here performs `*r += pixel.r` (buffer.rs:159-164) for every parked
    // sample of the block's pixels, in sample order (sum_block).  The parked values were written by waves of this
    // workgroup (same CU, same L1 / L2), so workgroup-scope release / acquire is all the ordering that is needed.
    if (P.counters) {
        uint32_t sg = segments;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sg += __shfl_xor(sg, off, 64);
        if (lane == 0 && sg) atomicAdd(&s_segments, sg);              // LDS; ahead of this wave's s_waves_done below
    }
    if (packed) {
        // one generation of workgroups: nobody waits for this workgroup's wave slots, so its waves meet at a barrier and sum together
        __syncthreads();
        if (P.counters && threadIdx.x == 0) {
            const uint32_t total = *(volatile uint32_t *)&s_segments;
            if (total) atomicAdd(&P.counters[0], (unsigned long long)total);
        }
        sum_blocks(P, G, blockIdx.x, gridDim.x, my_blocks, T, park(), threadIdx.x, blockDim.x, P.out);
        if (GUIDED) {                                                     // each guide's plane, the same additions into its own frame
            const size_t at = (size_t)blockIdx.x * ((size_t)P.wg_blocks << (P.log_rows + LOG_PXB));
            if (P.guide_out[0]) sum_blocks(P, G, blockIdx.x, gridDim.x, my_blocks, T, (const Parked *)P.guide_scratch[0] + at, threadIdx.x, blockDim.x, P.guide_out[0]);
            if (P.guide_out[1]) sum_blocks(P, G, blockIdx.x, gridDim.x, my_blocks, T, (const Parked *)P.guide_scratch[1] + at, threadIdx.x, blockDim.x, P.guide_out[1]);
            if (P.guide_out[2]) sum_blocks(P, G, blockIdx.x, gridDim.x, my_blocks, T, (const Parked1 *)P.guide_scratch[2] + at, threadIdx.x, blockDim.x, P.guide_out[2]);
        }
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        uint32_t arrived = 0;
        if (lane == 0) arrived = atomicAdd(&s_waves_done, 1u);
        arrived = (uint32_t)__builtin_amdgcn_readfirstlane((int)arrived);
        if (arrived == (blockDim.x >> 6) - 1u) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (P.counters && lane == 0) {
                const uint32_t total = *(volatile uint32_t *)&s_segments;
                if (total) atomicAdd(&P.counters[0], (unsigned long long)total);
            }
            if constexpr (ADAPT) {
                // the moment plane's address is read here, behind the loop, through the opaque pointer (see the prologue)
                typedef const __attribute__((address_space(4))) BtLaunch BtLaunchK;
                BtLaunchK *C = (BtLaunchK *)__builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(C));
                sum_block<Parked, true>(P, G, bid, T, park(), lane, P.out, C->moment);
            } else {
                sum_block(P, G, bid, T, park(), lane, P.out);
            }
            if (GUIDED) {                                                 // each guide's plane, the same additions into its own frame
                const size_t at = (size_t)bid * (size_t)n_items;
                if (P.guide_out[0]) sum_block(P, G, bid, T, (const Parked *)P.guide_scratch[0] + at, lane, P.guide_out[0]);
                if (P.guide_out[1]) sum_block(P, G, bid, T, (const Parked *)P.guide_scratch[1] + at, lane, P.guide_out[1]);
                if (P.guide_out[2]) sum_block(P, G, bid, T, (const Parked1 *)P.guide_scratch[2] + at, lane, P.guide_out[2]);
            }
        }
    }
    if (P.counters) {
        if (LENS) {
            unsigned long long ls = wave_sum(lens_steps);
            if (lane == 0 && ls) atomicAdd(&P.counters[1], ls);
        }
#ifdef BT_LANESTAT
        for (int i = 0; i < 9; ++i) {
            unsigned long long v = ls_acc[i];
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(v, off, 64);
                v = o > v ? o : v;
            }
            if (lane == 0) atomicAdd(&P.counters[2 + i], v);
        }
#elif defined(BT_PROFILE)
        if (lane == 0)
            for (int i = 0; i < BT_N_COUNTERS - 2; ++i) atomicAdd(&P.counters[2 + i], prof_acc[i]);
#endif
    }
