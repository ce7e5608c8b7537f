// acas2d_step_body.inl -- the body of step_kernel, eval_stats_kernel, monte_carlo_kernel, the latter two's disturbed,
// correlated and delayed flavours and the disturbed and the correlated set collector (acas2d_kernels.hpp, where the modes and what
// each one implies are described), included inside all eleven.  It
// expects the including kernel's template parameters T, C, G, PACKED, FAST, M (or constants of those names), the constants
// STATS, MC, DIST, CORR and RESP, and the kernel's arguments a0 .. a5,
// e_n_envs, tile_elems, p_arg, rp_arg, s_arg, io_arg, k0, k1, env_offset, N_arg, n_steps, pw.
    constexpr bool AUTO_RESET = M != Mode::Latch, ROLLOUT = rollout_mode(M);
    constexpr bool POLICY = policy_mode(M), SAMPLE = sample_mode(M);
    constexpr bool ARENA = M == Mode::Arena, EVAL = M == Mode::Eval, SET = M == Mode::CollectSet;
    // the disturbed set collector is held to two waves per SIMD (256 registers) with an actor AND a critic per lane: what need not
    // be live across the two networks is formed or fetched again behind them (LEAN, below)
    constexpr bool LEAN = DIST && SET;
    static_assert(!SET || (PACKED && sizeof(T) == 4 && (G == 1 || group_policy_shape(C, G))),
                  "set collection: float32, one lane per env or the group-cooperative shapes");
    static_assert(!ROLLOUT || PACKED, "rollout modes: packed shapes");
    static_assert(!POLICY || G == 1 || (PACKED && sizeof(T) == 4 && group_policy_shape(C, G)),
                  "in-kernel policy: one lane per env, or the group-cooperative float32 shapes");
    constexpr int NS = PACKED ? C * G : 0;         // packed shapes: n_traffic is a compile-time constant
    const int N = PACKED ? NS : N_arg;
    constexpr int EPW = 64 / G;                    // envs per wavefront
    // The FIRST 14 dwords of the kernel arguments (a0 .. a5, the env count, the tile size) are preloaded into SGPRs by the
    // command processor (gfx950 kernarg preload, KFLAGS in the Makefile): loads through them leave with the wave's first
    // instructions instead of behind a scalar-load round trip to the argument segment (~0.27 us, all waves of a launch
    // miss together).  The grid size follows from the env count (geometry_for), so nothing of the launch geometry is
    // fetched either.  Six pointers do not name fourteen input arrays, so:
    //   ARENA   (launch_step found the state laid out as consecutive [k][E] rows, as the Python host allocates it)
    //           a0 = own_x (then own_y, own_psi, total_reward, steps), a1 = own_v (then goal_x, goal_y, episode),
    //           a2 = trf_x (then trf_y), a3 = trf_psi (then trf_v), a4 = actions: EVERY load leaves at once;
    //   else    a0 .. a5 = trf_x, trf_y, trf_psi, trf_v, own_x, own_y: the bulk of the bytes leaves at once, the rest
    //           behind the round trip.
    static_assert(!ARENA || (sizeof(T) == 4 && PACKED), "arena launches: float32, packed shapes");
    // A wavefront issues one instruction per four cycles whatever its kind, and every instruction in front of the first
    // load is on the launch's critical path: env indices are 32-bit here (n_envs < 2^31, geometry_for).
    const uint32_t E32 = (uint32_t)e_n_envs;
    const int lane = threadIdx.x & 63;
    const int j = lane & (G - 1), el = lane / G;   // lane in group, env in wave
    const int wib = wave_in_block();
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr uint32_t kEnvsPerBlock = EPW * kWavesPerBlock;
    // Arena launches come in whole multiples of eight workgroups (launch_step): every wave is full and the XCD remap
    // unconditional -- no bounds check, no clamped load index, no lane guards on the stores, fifteen instructions less
    // in front of the first load.
    constexpr bool FULL = ARENA;
    const uint32_t wave32 = (FULL ? (blockIdx.x & 7u) * (E32 / (kEnvsPerBlock * 8u)) + (blockIdx.x >> 3)
                                  : remap_block_of((E32 + (kEnvsPerBlock - 1u)) / kEnvsPerBlock)) * kWavesPerBlock + (uint32_t)wib;
    const uint32_t e_wave32 = wave32 * EPW;        // first env of this wave (scalar); < 2^31 + 128
    if constexpr (!FULL) { if (e_wave32 >= E32) return; }     // whole wave idle
    const int D = 5 + 3 * N;
    const int n_rows = FULL ? EPW : (int)((E32 - e_wave32) < (uint32_t)EPW ? (E32 - e_wave32) : (uint32_t)EPW);
    const bool active = FULL ? true : el < n_rows; // whole groups are active or not
    const int64_t n_envs = E32, e_wave = e_wave32, wave = wave32;
    (void)wave;
    // per wave: the observation tile, then (HANDOFF) the reset slots (SlotLayout) / one 4N+1-value scratch
    constexpr bool HANDOFF = PACKED && AUTO_RESET;   // finished envs are reset BEFORE the wave's stores
    T* tile = reinterpret_cast<T*>(lds_raw) + wib * tile_elems;
    T* row = tile + el * D;
    T* scratch = HANDOFF ? tile + (EPW * D + 3) / 4 * 4 : nullptr;     // 16-byte aligned within the tile allocation

    ACAS2D_STAMP(0, wave, lane, false);
    ACAS2D_STAMP(1, wave, lane, false);
    int32_t steps = 0;
    uint32_t episode = 0;
    T total = T(0);
    Own<T> o{};
    Traffic<T, C> tr{};
    bool frozen = false;
    T action_next = T(0);                                  // step t+1's action is fetched during step t
    // Packed shapes run loads and arithmetic on EVERY lane of the wave -- the lanes past the last env
    // (last wave only) on a copy of the wave's first env -- and predicate only the stores.  With the
    // loads and their first uses inside `if (active)`, the compiler's waitcnt model kept them pending
    // on the path around it and, vmcnt retiring in order, made every later loop and LDS read of the
    // kernel wait for all stores issued in between (s_waitcnt vmcnt(0) before the tile flush).
    const bool run = PACKED ? true : active;
    const int el_l = (PACKED && !active) ? 0 : el;         // the env a lane LOADS
    // ---- every load of this lane up front, all requests in flight at once; the loads through the preloaded pointers
    // leave in front of the wait for the other arguments ...
    State<T> s_in = s_arg;                                 // (fields nobody reads cost nothing)
    const T* act_in = io_arg.actions;
    if constexpr (ARENA) {
        act_in = a4;                                       // (the state pointers the STORES use: behind the loads, below)
    } else {
        s_in.trf_x = const_cast<T*>(a0); s_in.trf_y = const_cast<T*>(a1); s_in.trf_psi = const_cast<T*>(a2);
        s_in.trf_v = const_cast<T*>(a3); s_in.own_x = const_cast<T*>(a4); s_in.own_y = const_cast<T*>(a5);
    }
    // only the per-step auto-reset launch takes a second state generation (launch_step); elsewhere the offsets are
    // compile-time zeros and cost no registers
    if constexpr (ROLLOUT || !AUTO_RESET) { s_in.w_env = 0; s_in.w_trf = 0; }
    T ox = T(0), oy = T(0);
    if constexpr (ARENA) {
        // Unmodified preloaded bases + 32-bit per-lane byte offsets (launch_step checked that they fit): one VALU add
        // per array instead of four scalar ones.  The player's scalars and the action first, the traffic vectors (the
        // bulk) last: loads return in order, so the player-side arithmetic can start while the vectors are landing.
        if (run) {
            const uint32_t ie = e_wave32 + (uint32_t)el_l;                 // this lane's env
            const auto at = [](const T* base, uint32_t elem) {
                return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)(elem * 4u));
            };
            ox = *at(a0, ie); oy = *at(a0, ie + E32);
            o = Own<T>{ox, oy, *at(a0, ie + 2u * E32), *at(a1, ie), T(0), *at(a1, ie + E32), *at(a1, ie + 2u * E32)};
            steps = *reinterpret_cast<const int32_t*>(at(a0, ie + 4u * E32));
            total = *at(a0, ie + 3u * E32);
            episode = *reinterpret_cast<const uint32_t*>(at(a1, ie + 3u * E32));
            action_next = *at(a4, ie);
            using V = Vec<T, C>;
            const uint32_t it = ie * (uint32_t)N + (uint32_t)(j * C), EN32 = E32 * (uint32_t)N;
            tr.psi = *reinterpret_cast<const V*>(at(a3, it));
            tr.v = *reinterpret_cast<const V*>(at(a3, it + EN32));
            tr.x = *reinterpret_cast<const V*>(at(a2, it));
            tr.y = *reinterpret_cast<const V*>(at(a2, it + EN32));
        }
    } else if (run) {
        if constexpr (PACKED)
            tr = load_traffic<T, C>(s_in.trf_psi + e_wave * N, s_in.trf_v + e_wave * N, s_in.trf_x + e_wave * N,
                                    s_in.trf_y + e_wave * N, el_l * N + j * C);
        ox = (s_in.own_x + e_wave)[el_l]; oy = (s_in.own_y + e_wave)[el_l];
    }
    __builtin_amdgcn_sched_barrier(0);                     // ... and stay there: nothing below is scheduled above them
    // everything else the loads (ARENA: the stores) need from the kernel arguments, requested in ONE scalar-load round
    // trip (left alone, hipcc fetches them one by one, each behind its own s_waitcnt)
    if constexpr (ARENA)
        asm volatile("" :: "s"(s_arg.w_env), "s"(s_arg.w_trf), "s"(io_arg.obs), "s"(io_arg.reward), "s"(io_arg.done),
                     "s"(io_arg.outcome) : "memory");
    else
        asm volatile("" :: "s"(s_arg.own_psi), "s"(s_arg.own_v), "s"(s_arg.goal_x), "s"(s_arg.goal_y),
                     "s"(s_arg.steps), "s"(s_arg.total_reward), "s"(s_arg.episode), "s"(io_arg.actions),
                     "s"(s_arg.w_env), "s"(s_arg.w_trf) : "memory");
    if constexpr (ARENA) {
        const int64_t E = n_envs, EN = n_envs * N;
        T* m = const_cast<T*>(a0);
        T* c = const_cast<T*>(a1);
        s_in.own_x = m; s_in.own_y = m + E; s_in.own_psi = m + 2 * E; s_in.total_reward = m + 3 * E;
        s_in.steps = reinterpret_cast<int32_t*>(m + 4 * E);
        s_in.own_v = c; s_in.goal_x = c + E; s_in.goal_y = c + 2 * E; s_in.episode = reinterpret_cast<uint32_t*>(c + 3 * E);
        s_in.trf_x = const_cast<T*>(a2); s_in.trf_y = s_in.trf_x + EN;
        s_in.trf_psi = const_cast<T*>(a3); s_in.trf_v = s_in.trf_psi + EN;
        s_in.trace = nullptr;
    }
    const State<T> s = rebase(s_in, e_wave, N);            // everything below indexes envs by `el`
    StepIO<T> io_in = io_arg;
    io_in.actions = act_in;
    const StepIO<T> io0 = rebase(io_in, e_wave, D);
    if constexpr (!ARENA) {
        if (run) {
            o = Own<T>{ox, oy, s.own_psi[el_l], s.own_v[el_l], T(0), s.goal_x[el_l], s.goal_y[el_l]};
            steps = s.steps[el_l];
            total = s.total_reward[el_l];
            if constexpr (AUTO_RESET) episode = s.episode[el_l];
            else frozen = s.status[el_l] != 0;                             // game.py:243-245
            if constexpr (!POLICY) action_next = io0.actions[el_l];
        }
    }

    // Launch constants into VGPRs only now, AFTER the loads are in flight: pinned() is ~25 v_movs
    // behind a kernarg s_load round trip, which used to sit in front of the first global load.
    // (not for the policy rollout: its MLP needs the 25 registers more than it minds re-fetching
    // launch constants, and has to stay under 256 VGPRs to keep two waves per SIMD)
    // (float32: only the constants the formulation reads, -0.08 us per launch; float64 measured no better that way)
    const Params<T> p = POLICY ? p_arg : (sizeof(T) == 4 ? pinned_for<T, FAST>(p_arg) : pinned(p_arg));
    if constexpr (AUTO_RESET && !ROLLOUT && sizeof(T) == 4) {
        // ... and what the reset of a finished env reads, so that its wave does not start the reset
        // with a scalar-load round trip (the kernel ends with that wave).  Not in the float64 build: its 21 reset
        // constants are 42 SGPRs, and with them pinned hipcc stages the 25 launch constants through one 16-register range
        // in three batches, a scalar round trip each, in front of every wave's arithmetic (float64 FAST 10.8 -> 10.3 us per
        // launch without the request, although a finishing wave then fetches the reset constants when it needs them).
        asm volatile("" :: "s"(rp_arg.own_x0), "s"(rp_arg.own_y0), "s"(rp_arg.own_v), "s"(rp_arg.own_heading0),
                     "s"(rp_arg.own_heading_jitter), "s"(rp_arg.goal_x), "s"(rp_arg.goal_y), "s"(rp_arg.t0_x), "s"(rp_arg.t0_y_base),
                     "s"(rp_arg.t0_y_span), "s"(rp_arg.t0_heading_base), "s"(rp_arg.t0_heading_step), "s"(rp_arg.t0_heading_jitter),
                     "s"(rp_arg.tn_x_max), "s"(rp_arg.tn_y_max), "s"(rp_arg.speed_factor_min), "s"(rp_arg.speed_factor_max),
                     "s"(rp_arg.airspeed), "s"(rp_arg.d_goal0), "s"(rp_arg.h_goal0), "s"(rp_arg.d_dev0),
                     "s"(k0), "s"(k1), "s"(io_arg.term_obs), "s"(io_arg.ep_return), "s"(io_arg.ep_steps), "s"(env_offset));
    }
    const StepResetParams<T, ROLLOUT>& rp = rp_arg;
    TrigCache<T, C> trig;                                  // rollout only (a per-step launch starts cold anyway)
    const int T_steps = ROLLOUT ? n_steps : 1;
    if constexpr (POLICY) {
        // the observation the first action is taken on (reset()'s / the previous step's) into the lane's row
        const T* obs_in = static_cast<const T*>(pw.obs_in) + e_wave * D;
        if constexpr (G == 1) {
            if (active) { for (int i = 0; i < D; ++i) row[i] = obs_in[el * D + i]; }
        } else {                                           // the group shares the row: each lane a G-th of it
            if (active) { for (int i = j; i < D; i += G) row[i] = obs_in[el * D + i]; }
            wave_lds_fence();
        }
    }
    // EVAL: this wave's policy (ep_stride is a multiple of the wave, so one per wave: its weights stay SGPR operands), the
    // lane's episode, and whether it is still playing it (padding lanes past n_episodes never are)
    bool running = false;
    int64_t res_i = 0;
    if constexpr (EVAL) {
        const uint32_t kp = __builtin_amdgcn_readfirstlane(e_wave32 / (uint32_t)pw.ep_stride);
        const uint32_t ep = e_wave32 - kp * (uint32_t)pw.ep_stride + (uint32_t)el;
        running = active && ep < (uint32_t)pw.n_episodes;
        res_i = (int64_t)kp * pw.n_episodes + ep;
        constexpr int DP = 5 + 3 * NS;
        pw.w1t += (size_t)kp * (DP * kPolicyHidden); pw.b1 += (size_t)kp * kPolicyHidden;
        pw.w2t += (size_t)kp * (kPolicyHidden * kPolicyHidden); pw.b2 += (size_t)kp * kPolicyHidden;
        pw.w3 += (size_t)kp * kPolicyHidden; pw.b3 += kp;
    }
    (void)running; (void)res_i;
    // MC: the lane's RNG index is its index WITHIN its policy's block (every policy meets the same encounters), its
    // episode counter the launch's first one, and the launch's integer sums stay in registers: the four episode COUNTS
    // per wave (ballots, scalar registers), the two sums per lane
    uint64_t mc_gid_wave = 0;
    int32_t mc_n1 = 0, mc_n2 = 0, mc_n3 = 0, mc_los_eps = 0;      // wave-uniform
    int32_t mc_steps = 0, mc_los = 0;                            // per lane
    uint32_t mc_kp = 0;
    (void)mc_gid_wave; (void)mc_n1; (void)mc_n2; (void)mc_n3; (void)mc_steps; (void)mc_los_eps; (void)mc_los; (void)mc_kp;
    if constexpr (MC) {
        const PolicyMonteCarloW* const mcw = monte_carlo_args(pw);
        mc_kp = __builtin_amdgcn_readfirstlane(e_wave32 / (uint32_t)pw.ep_stride);
        mc_gid_wave = (uint64_t)env_offset + (uint64_t)(e_wave32 - mc_kp * (uint32_t)pw.ep_stride);
        episode = mcw->mc_first;
    }
    // DIST: the lane's index in the disturbance's counter -- the Monte Carlo kernel's RNG index, env_offset + the index
    // within the policy's block (the evaluator's episode index), so K policies meet the same noise
    uint64_t dist_lane = 0;
    (void)dist_lane;
    if constexpr (DIST) {
        static_assert(((EVAL && STATS) || (SET && SAMPLE)) && sizeof(T) == 4,
                      "disturbances: the float32 stats evaluator, Monte Carlo kernel and set collector");
        if constexpr (SET) {                              // the collector: the sampler's gid, the GLOBAL env index
            dist_lane = (uint64_t)env_offset + (uint64_t)(e_wave32 + (uint32_t)el);
        } else {
            const uint32_t kp = __builtin_amdgcn_readfirstlane(e_wave32 / (uint32_t)pw.ep_stride);
            dist_lane = (uint64_t)env_offset + (uint64_t)(e_wave32 - kp * (uint32_t)pw.ep_stride + (uint32_t)el);
        }
    }
    // DIST and SET (collect_set_disturbed_kernel): the member's four sigmas and the launch's noise key as the DisturbW the
    // evaluator takes by value -- filled in the SET prologue below; its episode field is not used (the lane's own counts)
    DisturbW set_dw{};
    (void)set_dw;
    // CORR: the lane's held errors e_{t-1}, at the end of the wave's LDS (CorrW) -- value i at corr_held[i * 64]: 3 k + c for
    // channel c of the lane's k-th aircraft, then the actuator's
    // (RESP: one slot more behind them, the lag's u_{s-1} -- RespW)
    constexpr int kHeldSlots = CORR ? kCorrSlots(C) + (RESP ? 1 : 0) : 0;
    float* corr_held = nullptr;
    (void)corr_held;
    // CORR and SET (collect_set_correlated_kernel): the member's four rho and four gains as the CorrW the evaluator takes by
    // value -- filled in the SET prologue below, scalar registers, so that `rho == 0` stays a wave-uniform branch
    CorrW set_cw{};
    (void)set_cw;
    if constexpr (CORR) {
        static_assert(DIST && ((EVAL && STATS) || SET),
                      "correlated errors: the disturbed stats evaluator, Monte Carlo kernel and set collector");
        corr_held = reinterpret_cast<float*>(tile) + (tile_elems - kHeldSlots * 64) + lane;
        if constexpr (SET) {
            // the state the previous launch left (CollectCorrW::held, rows of E): every process of the lane, whatever its rho --
            // a value nobody advances goes back as it came.  Lanes past the last env load nothing: they play a copy of the
            // wave's first env on whatever their slots hold, and store nothing.
            if (active) {
                const float* const hp = collect_correlation_args(pw)->held + (e_wave + el);
#pragma unroll
                for (int i = 0; i < 3 * C; ++i) corr_held[i * 64] = hp[(int64_t)(3 * (j * C) + i) * n_envs];
                corr_held[(3 * C) * 64] = hp[(int64_t)(3 * N) * n_envs];
            }
        }
    }
    // STATS: the running statistics of the lane's episode (PolicyEvalStatsW)
    T st_min = T(1) / T(0), st_a_lat = T(0), st_dev = T(0), st_sum = T(0);
    int32_t st_min_step = 0, st_los = 0;
    (void)st_min; (void)st_a_lat; (void)st_dev; (void)st_sum; (void)st_min_step; (void)st_los;
    // SET: this wave's member (member_stride is a multiple of the wave, so one per wave: its weights stay SGPR operands),
    // its slices of the stacks and its noise key -- one scalar load; everything below is Mode::Collect's step
    if constexpr (SET) {
        const uint32_t km = __builtin_amdgcn_readfirstlane(e_wave32 / pw.member_stride);
        constexpr int DP = 5 + 3 * NS;
        pw.w1t += (size_t)km * (DP * kPolicyHidden); pw.b1 += (size_t)km * kPolicyHidden;
        pw.w2t += (size_t)km * (kPolicyHidden * kPolicyHidden); pw.b2 += (size_t)km * kPolicyHidden;
        pw.w3 += (size_t)km * kPolicyHidden; pw.b3 += km;
        pw.v1t += (size_t)km * (DP * kPolicyHidden); pw.vb1 += (size_t)km * kPolicyHidden;
        pw.v2t += (size_t)km * (kPolicyHidden * kPolicyHidden); pw.vb2 += (size_t)km * kPolicyHidden;
        pw.v3 += (size_t)km * kPolicyHidden; pw.vb3 += km;
        pw.log_std += km;
        const uint64_t* keys = reinterpret_cast<const uint64_t*>((uintptr_t)pw.nk0 | ((uintptr_t)pw.nk1 << 32));
        const uint64_t key = ((const uint64_t ACAS2D_AS4*)keys)[km];
        pw.nk0 = (uint32_t)key; pw.nk1 = (uint32_t)(key >> 32);
        if constexpr (DIST) {                             // the member's row of float[K][4]: sep, cpa, closing, action
            const CollectDistW* const cw = collect_disturbance_args(pw);
            const float ACAS2D_AS4* const sg = (const float ACAS2D_AS4*)cw->sigmas + 4 * (size_t)km;
            set_dw = DisturbW{sg[0], sg[1], sg[2], sg[3], cw->dk0, cw->dk1, 0u};
        }
        if constexpr (CORR) {                             // ... and of float[K][8]: four rho, four gains
            const float ACAS2D_AS4* const cr = (const float ACAS2D_AS4*)collect_correlation_args(pw)->correlations + 8 * (size_t)km;
            set_cw = CorrW{cr[0], cr[1], cr[2], cr[3], cr[4], cr[5], cr[6], cr[7]};
        }
    }
    for (int t = 0; t < T_steps + ((DIST && SET) ? 1 : 0); ++t) {      // (DIST && SET: one pass more, for obs_read[n_steps])
        // (MC: the running minimum stays an ordinary register over the loop.  Left alone, the float64 FAST kernels at
        //  N = 2, 3, 4 keep its +inf start in an accumulation register pair and count that as a spill.)
        if constexpr (MC) asm volatile("" : "+v"(st_min));
        // outputs of step t: [t][E] / [t][E][D] slices (t == 0 for the per-step launch)
        const int64_t te = ROLLOUT ? (int64_t)t * n_envs : 0;
        const StepIO<T> io{io0.actions + te, io0.obs + te * D, io0.reward + te, io0.done + te, io0.outcome + te,
                           io0.term_obs ? io0.term_obs + te * D : nullptr,
                           io0.ep_return ? io0.ep_return + te : nullptr,
                           io0.ep_steps ? io0.ep_steps + te : nullptr};
        const bool last = !ROLLOUT || t == T_steps - 1;
        uint8_t oc = 0;
        T action = action_next;
        int el_st = el;                                   // the env index the step's STORES use
        if constexpr (POLICY) {
            constexpr int DP = 5 + 3 * NS;                // compile-time obs width (packed shapes)
            if constexpr (DIST) {
                // sensor noise: slot n + 1 of (lane, episode, steps before this step) on traffic n's three entries, IN the
                // wave's tile, by the lane that holds the aircraft in registers, fenced before the network reads the row
                // (observe() rewrites the row below; EVAL never flushes it).  In the tile at the thread-per-env shapes too:
                // perturbed in x[] below, the 5 + 3 N inputs are all live across the Philox chains where the network
                // otherwise fetches them as it goes, and the N = 8 kernels need 293 and 306 VGPRs -- one wave per SIMD
                // where their siblings (225, 252) keep two.  Through the tile they need 250 and 251.
                const DisturbW* const dw = SET ? &set_dw : disturbance_args(pw);
                if (dw->s_sep != 0.0f || dw->s_cpa != 0.0f || dw->s_closing != 0.0f) {      // (wave-uniform)
                    const uint32_t d_ep = (MC || SET) ? episode : dw->episode;
                    // CORR: the lane's first step of an episode in this launch (an in-step reset leaves steps == 1) -- SET: of
                    // an episode, reset()'s or an in-step reset's: a launch boundary is no episode boundary, the held value came
                    // in from memory.  The collector's extra pass forms e_T without committing it: what goes back to memory is
                    // the state after the last played step, and the next launch's first step forms the same e_T again.
                    const bool corr_first = CORR && (SET ? steps == 1 : (t == 0 || steps == 1));
                    const bool corr_commit = !SET || t != T_steps;         // (wave-uniform)
                    (void)corr_first; (void)corr_commit;
#pragma unroll
                    for (int k = 0; k < C; ++k) {
                        const int n = j * C + k;
                        float z0, z1, z2;
                        disturbance_normals(dw->k0, dw->k1, dist_lane, d_ep, (uint32_t)steps, (uint32_t)(n + 1), z0, z1, z2);
                        if constexpr (CORR) {             // e_t in z_t's place
                            const CorrW* const cw = SET ? &set_cw : correlation_args(pw);
                            z0 = correlated(corr_held + (3 * k) * 64, corr_first, cw->rho_sep, cw->q_sep, z0, corr_commit);
                            z1 = correlated(corr_held + (3 * k + 1) * 64, corr_first, cw->rho_cpa, cw->q_cpa, z1, corr_commit);
                            z2 = correlated(corr_held + (3 * k + 2) * 64, corr_first, cw->rho_closing, cw->q_closing, z2, corr_commit);
                        }
                        float* const e = reinterpret_cast<float*>(row) + 5 + 3 * n;
                        e[0] = disturbed(e[0], dw->s_sep, z0, 0.0f, 1.0f);
                        e[1] = disturbed(e[1], dw->s_cpa, z1, -1.0f, 1.0f);
                        e[2] = disturbed(e[2], dw->s_closing, z2, -1.0f, 1.0f);
                    }
                    wave_lds_fence();                      // the disturbed rows are complete
                }
                if constexpr (SET) {
                    // obs_read[t]: the rows both networks read at this step, as they stand in the tile (a NaN stays one:
                    // the scrub to 0 is the networks' own), with the coalesced flush of the step's end.  Row n_steps is the
                    // tile the last step left, fresh rows of just-reset envs included, under the draw the NEXT launch's
                    // first step makes from the same (episode, steps): the loop's one extra pass ends here.
                    const CollectDistW* const cw = collect_disturbance_args(pw);
                    wave_lds_fence();                      // every row of the tile is complete (zero sigmas: no fence above)
                    constexpr int kChunks = (EPW * DP * (int)sizeof(T) / 16 + 63) / 64;
                    int lane_f = lane;                     // (a fresh value: no per-lane address kept from the loop's front)
                    asm volatile("" : "+v"(lane_f));
                    flush_tile_unrolled<T, kChunks>(tile, static_cast<T*>(cw->obs_read) + ((int64_t)t * n_envs + e_wave) * D,
                                                    n_rows * D, lane_f);
                    if (t == T_steps) break;
                    wave_lds_fence();                      // the flush's reads precede observe()'s row writes
                }
            }
            float x[G == 1 ? DP : 1];
            (void)x;
            if constexpr (G == 1) {
#pragma unroll
                for (int i = 0; i < DP; ++i) x[i] = (float)row[i];
            }
            // G > 1: the group evaluates the network together (policy_mlp_group()); its hidden vector lies behind
            // the wave's tile and reset slots (geometry_for())
            float* hid = nullptr;
            if constexpr (G > 1) hid = reinterpret_cast<float*>(tile) + (tile_elems - kHeldSlots * 64 - EPW * kPolicyHidden);
            (void)hid;
            // The weights must be RE-READ every step (scalar cache hits): they are loop-invariant, and
            // hoisted out of the step loop hipcc tries to keep all 4 700 of them in SGPRs, spills them
            // to VGPR lanes and reads them back one v_readlane at a time (7x slower).  Laundering the
            // pointers through an empty asm makes the loads depend on the iteration.
            PolicyW pw_t = pw;
            asm volatile("" : "+s"(pw_t.w1t), "+s"(pw_t.b1), "+s"(pw_t.w2t), "+s"(pw_t.b2), "+s"(pw_t.w3), "+s"(pw_t.b3));
            if constexpr (SAMPLE) {
                float mean, value;
                if constexpr (G == 1) {
#pragma unroll
                    for (int i = 0; i < DP; ++i) x[i] = (x[i] == x[i] && fabsf(x[i]) < __builtin_inff()) ? x[i] : 0.0f;
                    mean = policy_mlp<DP>(pw_t.w1t, pw_t.b1, pw_t.w2t, pw_t.b2, pw_t.w3, pw_t.b3, x);
                    asm volatile("" : "+s"(pw_t.v1t), "+s"(pw_t.vb1), "+s"(pw_t.v2t), "+s"(pw_t.vb2), "+s"(pw_t.v3), "+s"(pw_t.vb3),
                                      "+s"(pw_t.log_std));
                    if constexpr (LEAN) {                 // the critic's inputs from the tile again: not live across the actor
                        const T* row_c = row;
                        asm volatile("" : "+v"(row_c));
#pragma unroll
                        for (int i = 0; i < DP; ++i) {
                            const float xi = (float)row_c[i];
                            x[i] = (xi == xi && fabsf(xi) < __builtin_inff()) ? xi : 0.0f;
                        }
                    }
                    value = policy_mlp<DP>(pw_t.v1t, pw_t.vb1, pw_t.v2t, pw_t.vb2, pw_t.v3, pw_t.vb3, x);
                } else {
                    mean = policy_mlp_shared<DP, G, true>(pw_t.w1t, pw_t.b1, pw_t.w2t, pw_t.b2, pw_t.w3, pw_t.b3,
                                                          reinterpret_cast<const float*>(tile), hid, lane);
                    asm volatile("" : "+s"(pw_t.v1t), "+s"(pw_t.vb1), "+s"(pw_t.v2t), "+s"(pw_t.vb2), "+s"(pw_t.v3), "+s"(pw_t.vb3),
                                      "+s"(pw_t.log_std));
                    value = policy_mlp_shared<DP, G, true>(pw_t.v1t, pw_t.vb1, pw_t.v2t, pw_t.vb2, pw_t.v3, pw_t.vb3,
                                                           reinterpret_cast<const float*>(tile), hid, lane);
                    wave_lds_fence();                     // the row has been read: observe() rewrites it below
                }
                // DIST: the stores' index is a fresh value behind the networks.  Left alone, hipcc forms the ~13 per-lane
                // 64-bit store addresses of a step in front of the step loop and keeps them (26 registers) across both networks.
                if constexpr (LEAN) asm volatile("" : "+v"(el_st));
                const float log_std = ((const float ACAS2D_AS4*)pw_t.log_std)[0];
                // eps ~ N(0, 1): one Philox block per (global env, noise step + t), Box-Muller on two 24-bit uniforms
                const uint64_t gid = (uint64_t)(env_offset + e_wave + el);
                const U4 w = philox4x32(U4{(uint32_t)gid, (uint32_t)(gid >> 32), pw.noise_step + (uint32_t)t, 0x6e6f6973u},
                                           pw.nk0, pw.nk1);
                const float u1 = u01f(w.x), u2 = u01f(w.y);
                const float eps = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1)) *    // -2 ln u1
                                  __builtin_amdgcn_cosf(u2);                                                    // cos(2 pi u2)
                const float raw = fmaf(__builtin_amdgcn_exp2f(log_std * 1.4426950408889634f), eps, mean);
                const float logp = fmaf(-0.5f * eps, eps, -log_std) - 0.9189385332046727f;                      // - log sqrt(2 pi)
                if (active && j == 0) {                   // (group-uniform values: the group's first lane stores them)
                    (static_cast<T*>(pw.actions_out) + e_wave + te)[el_st] = (T)raw;      // the buffer keeps the RAW action,
                    (static_cast<T*>(pw.values_out) + e_wave + te)[el_st] = (T)value;     // the env sees the clipped one
                    (static_cast<T*>(pw.logp_out) + e_wave + te)[el_st] = (T)logp;
                }
                action = (T)fminf(fmaxf(raw, -1.0f), 1.0f);
                if constexpr (DIST) {                     // actuator noise: the environment's, not the policy's -- the buffer
                    if (set_dw.s_action != 0.0f) {        // keeps raw and its logp; slot 0 on the clipped action, clipped again
                        float z0, z1, z2;                 // (wave-uniform)
                        disturbance_normals(set_dw.k0, set_dw.k1, dist_lane, episode, (uint32_t)steps, 0u, z0, z1, z2);
                        // e_t in z_t's place: the lane's last held value.  It commits: the extra pass (t == T_steps) never gets
                        // here -- it leaves the loop at the `break` behind the obs_read flush above.  A draw moved in front of
                        // that break must pass corr_commit, or the state stored behind the loop is one step ahead.
                        if constexpr (CORR)
                            z0 = correlated(corr_held + (3 * C) * 64, steps == 1, set_cw.rho_action, set_cw.q_action, z0);
                        action = (T)disturbed((float)action, set_dw.s_action, z0, -1.0f, 1.0f);
                    }
                }
            } else {
                if constexpr (G == 1) {
                    action = (T)policy_action<DP>(pw_t, x);
                } else {                                  // policy_action() with the group's network
                    const float m = policy_mlp_shared<DP, G, false>(pw_t.w1t, pw_t.b1, pw_t.w2t, pw_t.b2, pw_t.w3, pw_t.b3,
                                                                    reinterpret_cast<const float*>(tile), hid, lane);
                    wave_lds_fence();                     // the row has been read: observe() rewrites it below
                    action = (T)(m != m ? m : fminf(fmaxf(m, -1.0f), 1.0f));
                }
                if constexpr (!EVAL) { if (active && j == 0) (static_cast<T*>(pw.actions_out) + e_wave + te)[el] = action; }
                if constexpr (RESP) {
                    // the response (RespW): the clipped action a_s becomes the command c_s = a_{s - delay} of the same episode
                    // (0 while the episode is younger than that), then u_s = clamp((lam u_{s-1}) + (g c_s)) with u = 0 in front
                    // of the episode's first step; the actuator's error below acts on u_s.  Both off: wave-uniform, nothing done.
                    static_assert(CORR && EVAL && STATS, "response delay and lag: the correlated stats evaluator and Monte Carlo kernel");
                    const RespW* const rs = response_args(pw);
                    float cmd = (float)action;
                    if (rs->delay != 0) {                 // (wave-uniform)
                        // the episode's age in steps, this one not counted: t until the launch's first in-step reset (whatever
                        // `steps` the state came in with), steps - 1 from then on.  Slot steps % delay holds a_{s - delay} once the
                        // episode is `delay` steps old and is never read before.  The address is a fresh value behind the network.
                        const uint32_t age = (uint32_t)t < (uint32_t)(steps - 1) ? (uint32_t)t : (uint32_t)(steps - 1);
                        const uint32_t slot = (uint32_t)steps % (uint32_t)rs->delay;
                        int el_r = el;
                        asm volatile("" : "+v"(el_r));
                        float* const q = rs->ring + ((int64_t)slot * rs->ring_envs + (e_wave + el_r));
                        float late = 0.0f;
                        if (active && j == 0) {           // (the env's first lane: every access to an address in program order)
                            if (age >= (uint32_t)rs->delay) late = *q;
                            *q = cmd;
                        }
                        cmd = group_bcast0<G>(late);
                    }
                    if (rs->lam != 0.0f) {                // (wave-uniform)
                        float* const held = corr_held + kCorrSlots(C) * 64;
                        const float prev = (t == 0 || steps == 1) ? 0.0f : *held;
                        cmd = fminf(fmaxf(__fadd_rn(__fmul_rn(rs->lam, prev), __fmul_rn(rs->gain, cmd)), -1.0f), 1.0f);
                        *held = cmd;
                    }
                    action = (T)cmd;
                }
                if constexpr (DIST) {                     // actuator noise: slot 0 on the clipped action, clipped again
                    const DisturbW* const dw = disturbance_args(pw);
                    if (dw->s_action != 0.0f) {           // (wave-uniform)
                        float z0, z1, z2;
                        disturbance_normals(dw->k0, dw->k1, dist_lane, MC ? episode : dw->episode, (uint32_t)steps, 0u, z0, z1, z2);
                        if constexpr (CORR) {             // e_t in z_t's place: the lane's last held value
                            const CorrW* const cw = correlation_args(pw);
                            z0 = correlated(corr_held + (3 * C) * 64, t == 0 || steps == 1, cw->rho_action, cw->q_action, z0);
                        }
                        action = (T)disturbed((float)action, dw->s_action, z0, -1.0f, 1.0f);
                    }
                }
            }
        } else {
            if (ROLLOUT && active && t + 1 < T_steps) action_next = io.actions[n_envs + el];
        }
        if (run) {
            if (t == 0) ACAS2D_STAMP(2, wave, lane, true);
            if constexpr (LEAN) {
                // the traffic's headings and speeds change at a reset only, where the lane stores them: fetched again behind
                // the networks (its own stores, in program order) instead of held across them -- 2 C registers
                int el_r = el_l;
                asm volatile("" : "+v"(el_r));
                using V = Vec<T, C>;
                const int i0 = el_r * N + j * C;
                tr.psi = *reinterpret_cast<const V*>(s.trf_psi + i0);
                tr.v = *reinterpret_cast<const V*>(s.trf_v + i0);
            }

            // game.py:225 + aircraft.py:16-26 for the player
            o.a_lat = action * p.acc_lat_limit;
            if constexpr (FAST) {
                o.psi = wrap_fast(o.psi + o.a_lat * f_rcp(o.v));        // (a_lat / (v dt)) dt
                T sn, cs;
                f_sincos_rev(o.psi * Const<T>::inv360, &sn, &cs);
                const T vdt = o.v * p.dt;
                o.x = m_fma(vdt, cs, o.x);
                o.y = m_fma(vdt, sn, o.y);
            } else {
                T psi_dot = o.a_lat / (o.v * p.dt);
                o.psi = py_mod360(o.psi + (psi_dot * p.dt));
                T sn, cs;
                m_sincos(deg2rad_ref(o.psi), &sn, &cs);
                o.x = o.x + ((o.v * cs) * p.dt);
                o.y = o.y + ((o.v * sn) * p.dt);
            }
            steps += 1;                                                       // game.py:197
            // `episode` is first USED in the reset loop far below; without this use the compiler waits
            // for its load there with s_waitcnt vmcnt(0) -- i.e. for every store issued since.
            asm volatile("" : "+v"(episode));
            T d_sep = T(0);                               // record rows only
            auto before_traffic = [&](const OwnCtx<T>&) {
                if constexpr (!AUTO_RESET) { if (s.trace) d_sep = minimum_separation<T, C, G, PACKED>(s, o, tr, el, j, N); }
                if constexpr (STATS) d_sep = minimum_separation<T, C, G, PACKED>(s, o, tr, el, j, N);   // every lane: it shuffles
            };
            Seen<T> r = observe<T, C, G, PACKED, FAST>(p, s, o, el, j, N, steps, !frozen, tr, row, !EVAL && last && active,
                                                       (ROLLOUT && !LEAN) ? &trig : nullptr, before_traffic);

            // game.py:249-292 evaluate()
            T rw = step_reward_5<T, FAST>(p, r.v_closing0, o.psi, r.h_goal, r.d_cpa0, r.d_goal, r.d_dev);
            if constexpr (FAST) rw = rw * m_fma(-(T)steps, p.inv_max_steps, T(1));
            else rw = rw * (T(1) - ((T)steps / (T)p.max_steps));              // :262-263
            if constexpr (!AUTO_RESET) {                                      // :266-276, the record lists
                if (s.trace && j == 0 && active)
                    write_trace<T, FAST>(p, s.trace + el * kTraceWidth, o.psi, d_sep, o.a_lat, r.h_goal, r.d_goal, r.d_dev,
                                         r.v_closing0, r.d_cpa0, rw);
            }
            const bool at_goal = r.d_goal < p.goal_radius;                    // :191-192
            if (r.collided) rw += p.reward_collision;                         // :279-280
            if (at_goal) rw += p.reward_goal;                                 // :283-284
            // game.py:294-314 is_done(): timeout > collision > goal
            oc = (steps > p.max_steps) ? 3 : (r.collided ? 2 : (at_goal ? 1 : 0));
            total = total + rw;                                               // :287
            if (!active) oc = 0;                          // a padding lane never finishes anything
            if constexpr (STATS) {
                if (running) {                            // this step's row (the finishing step's too), in step order
                    const T ad = m_abs(r.d_dev), aa = m_abs(o.a_lat);
                    if (d_sep < st_min) { st_min = d_sep; st_min_step = t + 1; }
                    st_los += (d_sep < p.safe_distance) ? 1 : 0;
                    st_a_lat = aa > st_a_lat ? aa : st_a_lat;
                    st_dev = ad > st_dev ? ad : st_dev;
                    st_sum = st_sum + ad;
                }
            }
            if constexpr (MC) {
                if (!running) oc = 0;                     // a lane with no episode left finishes (and redraws) nothing
                const bool lead = j == 0;                 // (a group finishes together: one count per env)
                mc_n1 += __popcll(__ballot(lead && oc == 1)); mc_n2 += __popcll(__ballot(lead && oc == 2));
                mc_n3 += __popcll(__ballot(lead && oc == 3)); mc_los_eps += __popcll(__ballot(lead && oc != 0 && st_los > 0));
                if (oc != 0) {                            // an episode ends: fold it, restart the statistics, go on
                    const PolicyMonteCarloW* const mcw = monte_carlo_args(pw);
                    mc_steps += steps;
                    mc_los += st_los;
                    if (j == 0) {                         // (a group finishes together: its first lane holds its accumulators)
                        const T inv_w = sizeof(T) == 4 ? (T)mcw->mc_inv_bin_f : (T)mcw->mc_inv_bin_d;
                        const T scaled = st_min * inv_w;
                        int b = mcw->mc_n_bins - 1;         // past the last edge, +-inf, NaN (records.separation_bin())
                        if (m_abs(scaled) < T(2147483648.0)) {
                            const int q = (int)scaled;
                            if (q < mcw->mc_n_bins) b = q < 0 ? 0 : q;
                        }
                        atomicAdd(mcw->mc_sep_hist + (size_t)mc_kp * mcw->mc_n_bins + b, 1ull);
                        // the lane's own slots [k][n_lanes] (recomputed here: one per ~700 steps, not a register pair)
                        const size_t li = (size_t)mc_kp * (uint32_t)pw.n_episodes +
                                          (e_wave32 - mc_kp * (uint32_t)pw.ep_stride + (uint32_t)el);
                        const double r = (double)total;
                        mcw->mc_return_sum[li] = mcw->mc_return_sum[li] + r;
                        mcw->mc_return_sq[li] = mcw->mc_return_sq[li] + (r * r);
                        T* worst = static_cast<T*>(mcw->mc_worst_sep) + li;
                        if (st_min < *worst) { *worst = st_min; mcw->mc_worst_episode[li] = episode; }
                    }
                    st_min = T(1) / T(0); st_los = 0;
                    if (episode == mcw->mc_first + (uint32_t)mcw->mc_episodes - 1u) { running = false; oc = 0; }   // its last one
                }
            } else if constexpr (EVAL) {
                if (running && oc != 0) {                 // the first episode's result, then the lane stops for good
                    if (j == 0) {                         // (a group latches together: its first lane writes)
                        pw.res_outcome[res_i] = oc;
                        pw.res_steps[res_i] = steps;
                        static_cast<T*>(pw.res_return)[res_i] = total;
                        if constexpr (STATS) {
                            static_cast<T*>(pw.st_min_sep)[res_i] = st_min;
                            pw.st_min_sep_step[res_i] = st_min_step;
                            pw.st_los_steps[res_i] = st_los;
                            static_cast<T*>(pw.st_max_a_lat)[res_i] = st_a_lat;
                            static_cast<T*>(pw.st_max_dev)[res_i] = st_dev;
                            static_cast<T*>(pw.st_sum_dev)[res_i] = st_sum;
                        }
                    }
                    running = false;
                }
            } else if (j == 0 && active) {
                io.reward[el_st] = rw;                    // (plain stores: non-temporal measured the same, 0.6 MB)
                io.done[el_st] = (uint8_t)(oc != 0);
                io.outcome[el_st] = oc;
                if constexpr (!HANDOFF) {
                    if (last && (oc == 0 || !AUTO_RESET)) {
                        put_env(s, s.own_x, el, o.x); put_env(s, s.own_y, el, o.y); put_env(s, s.own_psi, el, o.psi);
                        put_env(s, s.steps, el, steps);
                        put_env(s, s.total_reward, el, total);
                        if constexpr (!AUTO_RESET) { if (oc) s.status[el] = oc; }
                    }
                }
            }
        }

        if (t == 0) ACAS2D_STAMP(3, wave, lane, false);
        T* const obs_wave = io.obs;
        // MC: the same resets for the lanes that go on with another episode -- nothing of them is stored (no side channels:
        // io_r's pointers are compile-time NULL; no state, no episode counter: they live in registers until the lane is done)
        const StepIO<T> io_r = MC ? StepIO<T>{} : io;
        const uint64_t gid_wave_r = MC ? mc_gid_wave : (uint64_t)(env_offset + e_wave);
        if constexpr (HANDOFF && (!EVAL || MC)) {
            // ---- finished envs (one bit per env: its group's lane 0) are reset by the whole wave NOW,
            // before anything but reward / done / outcome has been stored: the new episode's state
            // reaches the owner lanes through LDS and leaves with the coalesced state stores and the
            // ONE tile flush below.  (Resetting after the flush cost a second store round at the very
            // end of the kernel -- ~12 scattered 4-byte stores per entity lane plus a re-flush of the
            // row: 0.8 us of the 7.7 us launch at 65 536 x 8.)
            bool fresh = false, same_consts = false;
            unsigned long long dm = __ballot(oc != 0 && j == 0);
            constexpr bool SLOTTED = ResetSlots<NS>::SLOTS >= 2;      // N + 1 <= 32: several envs per pass
            if constexpr (SLOTTED) {
                using SL = SlotLayout<T, NS>;
                while (dm) {
                    wave_lds_fence();                     // every row of the tile is complete
                    const unsigned long long taken =
                        wave_reset_slots<T, FAST, NS, G, decltype(rp), MC>(p, rp, io_r, k0, k1, gid_wave_r, dm, lane,
                                                         episode, tile, scratch);
                    dm &= ~taken;
                    wave_lds_fence();                     // the fresh rows and the slots are complete
                    if ((taken >> (el * G)) & 1ull) {     // my env was reset: its owner group goes on with the new episode
                        const int k_own = __popcll(taken & ((1ull << (el * G)) - 1ull));
                        const T* scr = scratch + k_own * SL::STRIDE;
                        if (j == 0) {
                            if (io_r.ep_return) io_r.ep_return[el_st] = total;
                            if (io_r.ep_steps) io_r.ep_steps[el_st] = steps;
                        }
                        using V = Vec<T, C>;              // the slot's blocks are aligned like the live traffic block
                        tr.x = *reinterpret_cast<const V*>(scr + j * C);
                        tr.y = *reinterpret_cast<const V*>(scr + N + j * C);
                        tr.psi = *reinterpret_cast<const V*>(scr + 2 * N + j * C);
                        tr.v = *reinterpret_cast<const V*>(scr + 3 * N + j * C);
                        // own_v / goal are the configuration's: stored only where an injected state had others
                        same_consts = o.v == (T)rp.own_v && o.gx == (T)rp.goal_x && o.gy == (T)rp.goal_y;
                        o = Own<T>{(T)rp.own_x0, (T)rp.own_y0, scr[SL::OWN_PSI], (T)rp.own_v, T(0), (T)rp.goal_x, (T)rp.goal_y};
                        steps = 1;                                            // environment.py:47
                        total = T(0);
                        episode += 1u;
                        fresh = true;
                        trig.valid = false; trig.dirty = false;   // new headings (stored below)
                        if constexpr (!MC) {
                            const int i0 = el_st * N + j * C;
                            put_trf<T, C>(s, s.trf_x, i0, tr.x); put_trf<T, C>(s, s.trf_y, i0, tr.y);
                            *reinterpret_cast<V*>(s.trf_psi + i0) = tr.psi; *reinterpret_cast<V*>(s.trf_v + i0) = tr.v;
                        }
                    }
                    wave_lds_fence();                     // the slots are free for the next pass
                }
            }
            while (!SLOTTED && dm) {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)dm) - 1);   // wave-uniform
                dm &= dm - 1;
                const int el_d = src / G;
                wave_lds_fence();                         // every row of the tile is complete
                wave_reset_env<T, FAST, NS, true, decltype(rp), MC>(p, rp, s, io_r, k0, k1, gid_wave_r + (uint64_t)el_d, el_d, N,
                                                  lane, lane_value(total, src), lane_value(steps, src),
                                                  (uint32_t)lane_value((int)episode, src), tile + el_d * D, scratch);
                wave_lds_fence();                         // the fresh row and the scratch are complete
                if (el == el_d) {                         // the owner group continues with the new episode
                    if (j == 0) {
                        if (io_r.ep_return) io_r.ep_return[el_st] = total;
                        if (io_r.ep_steps) io_r.ep_steps[el_st] = steps;
                    }
#pragma unroll
                    for (int k = 0; k < C; ++k) {
                        const int n = j * C + k;
                        tr.x.v[k] = scratch[n]; tr.y.v[k] = scratch[N + n];
                        tr.psi.v[k] = scratch[2 * N + n]; tr.v.v[k] = scratch[3 * N + n];
                    }
                    o = Own<T>{(T)rp.own_x0, (T)rp.own_y0, scratch[4 * N], (T)rp.own_v, T(0), (T)rp.goal_x, (T)rp.goal_y};
                    steps = 1;                                                // environment.py:47
                    total = T(0);
                    episode += 1u;
                    fresh = true;
                    trig.valid = false; trig.dirty = false;   // new headings (stored below)
                    // the new traffic block: whole 16-byte vectors from the owner lanes
                    using V = Vec<T, C>;
                    if constexpr (!MC) {
                        const int i0 = el_st * N + j * C;
                        put_trf<T, C>(s, s.trf_x, i0, tr.x); put_trf<T, C>(s, s.trf_y, i0, tr.y);
                        *reinterpret_cast<V*>(s.trf_psi + i0) = tr.psi; *reinterpret_cast<V*>(s.trf_v + i0) = tr.v;
                    }
                }
                wave_lds_fence();                         // scratch is free for the next finished env
            }
            if (!MC && active && j == 0) {
                if (fresh) {                              // per-episode constants of the new episode
                    if constexpr (ARENA) {
                        char* c = reinterpret_cast<char*>(const_cast<T*>(a1));
                        const uint32_t ie = e_wave32 + (uint32_t)el;
                        *reinterpret_cast<uint32_t*>(c + (size_t)((ie + 3u * E32) * 4u)) = episode;
                        if (!same_consts) {
                            *reinterpret_cast<T*>(c + (size_t)(ie * 4u)) = o.v;
                            *reinterpret_cast<T*>(c + (size_t)((ie + E32) * 4u)) = o.gx;
                            *reinterpret_cast<T*>(c + (size_t)((ie + 2u * E32) * 4u)) = o.gy;
                        }
                    } else {
                        s.episode[el_st] = episode;
                        if (!same_consts) { s.own_v[el_st] = o.v; s.goal_x[el_st] = o.gx; s.goal_y[el_st] = o.gy; }
                    }
                }
                if (last || fresh) {
                    if constexpr (ARENA) {
                        // ONE base (the block's write generation) and the 32-bit per-lane offsets the loads used: hipcc
                        // otherwise re-derives five 64-bit pointers in front of these stores, ~45 scalar instructions at
                        // the end of every wave
                        char* mw = reinterpret_cast<char*>(const_cast<T*>(a0)) + (int64_t)s.w_env * 4;
                        const uint32_t ie = e_wave32 + (uint32_t)el;
                        __builtin_nontemporal_store(o.x, reinterpret_cast<T*>(mw + (size_t)(ie * 4u)));
                        __builtin_nontemporal_store(o.y, reinterpret_cast<T*>(mw + (size_t)((ie + E32) * 4u)));
                        __builtin_nontemporal_store(o.psi, reinterpret_cast<T*>(mw + (size_t)((ie + 2u * E32) * 4u)));
                        __builtin_nontemporal_store(steps, reinterpret_cast<int32_t*>(mw + (size_t)((ie + 4u * E32) * 4u)));
                        __builtin_nontemporal_store(total, reinterpret_cast<T*>(mw + (size_t)((ie + 3u * E32) * 4u)));
                    } else {
                        put_env(s, s.own_x, el_st, o.x); put_env(s, s.own_y, el_st, o.y); put_env(s, s.own_psi, el_st, o.psi);
                        put_env(s, s.steps, el_st, steps);
                        put_env(s, s.total_reward, el_st, total);
                    }
                }
            }
        }
        // Flush the tile (generic walk: now, the stores drain while finished envs are reset below).
        if constexpr (!EVAL) {
            wave_lds_fence();
            if constexpr (PACKED) {
                constexpr int kChunks = (EPW * (5 + 3 * NS) * (int)sizeof(T) / 16 + 63) / 64;
                int lane_f = lane;
                if constexpr (LEAN) asm volatile("" : "+v"(lane_f));
                flush_tile_unrolled<T, kChunks>(tile, obs_wave, n_rows * D, lane_f);
            } else {
                flush_tile<T>(tile, obs_wave, n_rows * D, lane);
            }
        }
        if (t == 0) ACAS2D_STAMP(4, wave, lane, false);
        if constexpr (AUTO_RESET && !HANDOFF) {
            // ---- generic walk: finished envs are reset by the whole wave, entity lanes store the new
            // state themselves and the row is flushed again ----
            unsigned long long dm = __ballot(oc != 0 && j == 0);
            while (dm) {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)dm) - 1);   // wave-uniform
                dm &= dm - 1;
                const int el_d = src / G;
                wave_reset_env<T, FAST, NS, false>(p, rp, s, io, k0, k1, (uint64_t)(env_offset + e_wave + el_d), el_d, N,
                                                   lane, lane_value(total, src), lane_value(steps, src),
                                                   (uint32_t)lane_value((int)episode, src), tile + el_d * D, nullptr);
                wave_lds_fence();                         // the fresh row is complete
                flush_rows<T>(tile, obs_wave, n_rows * D, el_d * D, (el_d + 1) * D, lane);
            }
        }
        if constexpr (ROLLOUT) wave_lds_fence();          // tile reads precede the next step's row writes
        // EVAL: the wave is done once every lane has latched its result (a wave-uniform exit: the loop body has no
        // workgroup barrier, only the wave's own LDS tile and fences)
        if constexpr (EVAL) { if (__ballot(running) == 0ull) break; }
    }
    if constexpr (CORR && SET) {
        // The state after the last played step goes back to memory (the extra pass above committed nothing, so these are the
        // values the last step left), through addresses formed here: none of them is live across the networks.  Every lane of
        // a group holds the actuator's value; its first lane stores it.
        int el_h = el;
        asm volatile("" : "+v"(el_h));
        if (active) {
            float* const hp = collect_correlation_args(pw)->held + (e_wave + el_h);
#pragma unroll
            for (int i = 0; i < 3 * C; ++i) hp[(int64_t)(3 * (j * C) + i) * n_envs] = corr_held[i * 64];
            if (j == 0) hp[(int64_t)(3 * N) * n_envs] = corr_held[(3 * C) * 64];
        }
    }
    if constexpr (MC) {
        // the wave's integer sums: the counts as they are, the group leaders' two sums (every other lane adds 0) summed
        // across the wave, then ONE 64-bit vector atomic per counter from lane 0.  (A lane cut short by n_steps has folded the episodes it
        // finished; the launcher refuses a budget that could cut one.)
        const PolicyMonteCarloW* const mcw = monte_carlo_args(pw);
        const bool mine = active && j == 0;
        long long v[6] = {mc_n1, mc_n2, mc_n3, mine ? mc_steps : 0, mc_los_eps, mine ? mc_los : 0};   // (64-bit: 64 lanes' int32 sums)
#pragma unroll
        for (int q = 3; q < 6; q += 2)
            for (int w = 1; w < 64; w <<= 1) v[q] += __shfl_xor(v[q], w, 64);
        if (lane == 0) {
            unsigned long long* const dst[6] = {mcw->mc_outcome_count + 4 * (size_t)mc_kp + 1, mcw->mc_outcome_count + 4 * (size_t)mc_kp + 2,
                                                mcw->mc_outcome_count + 4 * (size_t)mc_kp + 3, mcw->mc_sum_steps + mc_kp,
                                                mcw->mc_los_episodes + mc_kp, mcw->mc_sum_los_steps + mc_kp};
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (v[q] != 0) atomicAdd(dst[q], (unsigned long long)v[q]);
        }
    } else if constexpr (EVAL) {
        if (running && j == 0) {                          // no done within n_steps
            pw.res_outcome[res_i] = 0;
            pw.res_steps[res_i] = 0;
            static_cast<T*>(pw.res_return)[res_i] = T(0);
            if constexpr (STATS) {
                static_cast<T*>(pw.st_min_sep)[res_i] = T(0);
                pw.st_min_sep_step[res_i] = 0;
                pw.st_los_steps[res_i] = 0;
                static_cast<T*>(pw.st_max_a_lat)[res_i] = T(0);
                static_cast<T*>(pw.st_max_dev)[res_i] = T(0);
                static_cast<T*>(pw.st_sum_dev)[res_i] = T(0);
            }
        }
    }
    ACAS2D_STAMP(5, wave, lane, false);
    ACAS2D_STAMP(6, wave, lane, true);
    ACAS2D_STAMP(7, wave, lane, false);
