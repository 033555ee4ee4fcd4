// mppi_rollout_pc.inc — the body of the producer/consumer rollout kernel, included as the body of k_rollout_pc (MPPI_PC_BATCH 0) and
// of k_rollout_pc_batch (MPPI_PC_BATCH 1), both in mppi_kernels.hip.h. A textual body rather than a force-inlined device function: the
// single controller's instances compile to exactly the code they had (an inlined function turns the kernel's __restrict__ arguments into
// alias scopes, and the scheduler makes other choices). With MPPI_PC_BATCH 1 every per-member operand moves to member m's (C points at
// member m's DevConsts); the arithmetic of every sample (noise, model step, costs, tile soft-min, butterfly) is the same text.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int S = 2 * A;
    constexpr int NW = NP + 1;
    constexpr int CS = 4 * NP;                // steps per chunk
    constexpr int SLOT = pc_slot_floats(A);   // floats per (step, lane)
    constexpr bool PACKED = SLOT != A + 1 || A == 3; // [CS][64 lanes][SLOT], one LDS instruction per slot; else [CS][(A+1)][64 lanes] dwords
    constexpr int CH = CS * SLOT * 64;        // floats per chunk buffer
    typedef float slot_t __attribute__((ext_vector_type(SLOT == 2 ? 2 : 4)));
    constexpr int NREG = NSLOT * 4 * A;       // noise values a producer lane keeps
    constexpr bool FMA = COST == PC_COST_DIAG_FMA;
    const int H = C->H;
    const int K = C->K_local;
    const int NG = (H + 3) / 4;               // horizon groups
    const int nch = (NG + NP - 1) / NP;       // chunks
    float *buf = smem;                        // [2][CS][(A+1)][64]
    float *w_s = smem;                        // [64] weights: reuses buffer 0 once every chunk is consumed
    MPPI_TL_DECL();

    const int tid = threadIdx.x;
    // Role placement. A workgroup's waves are spread over the CU's 4 SIMDs and the 4 workgroups that share a CU
    // (observed dispatch: block b -> XCD b%8, then a CU of it; blocks b, b+256, b+512, b+768 meet on one CU) should
    // put their light consumer wave on 4 DIFFERENT SIMDs, so that every SIMD runs 1 consumer + NP producers. The
    // hardware rotates the SIMD order of successive workgroups itself (measured with HW_ID: consumers chosen by wave
    // index landed 2+2+0+0), so with one wave per SIMD the role comes from the SIMD id the wave actually runs on:
    // consumer = the wave on SIMD gen%4 (gen = b/256). Falls back to the wave index when the 4 waves are not on 4
    // distinct SIMDs, and for grids of several rounds (no fixed set of co-resident workgroups there).
    // Placement only affects speed, never results.
    const int wave_hw = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gen = (int)(blockIdx.x >> 8);
    int wave = (wave_hw + NW - gen % NW) % NW; // SGPR: scalar branches, scalar loads of U
    if (NW == 4 && balance) {
        __shared__ int simd_s[4];
        const int simd = (int)__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4); // HW_REG_HW_ID[5:4]
        if ((tid & 63) == 0) simd_s[wave_hw] = simd;
        __syncthreads();
        const int s0 = simd_s[0], s1 = simd_s[1], s2 = simd_s[2], s3 = simd_s[3];
        if (((1 << s0) | (1 << s1) | (1 << s2) | (1 << s3)) == 15) wave = (simd + 4 - (gen & 3)) & 3;
        wave = __builtin_amdgcn_readfirstlane(wave);
    }
    const int lane = tid & 63;
    unsigned blk = blockIdx.x; // the tile within its controller
#if MPPI_PC_BATCH
    // member m = blockIdx.x / nb of the batch: its own x, U, costs, records (PcBatchArgs) and constants C[m] (Philox key, goal, lambda,
    // gamma, upsilon, Sigma, Q); H and K above are shared
    const int member = (int)blockIdx.x / bt.nb;
    blk = blockIdx.x - (unsigned)(member * bt.nb);
    C += member;
    x_dev += (size_t)member * S;
    U_dev += (size_t)member * bt.u_stride;
    cost += (size_t)member * K;
    partials += (size_t)member * bt.rec_stride;
#endif
    const int k0 = blk * 64;
    const bool valid = (k0 + lane) < K;
    float *rec = partials + (size_t)record_slot(blk, rsc) * rsb; // element (b, col) at partials[b*rsb + col*rsc]
    MPPI_TL_WHERE(wave);
    float nil_range = 0.0f; // PC_PASS_WEIGHTS: -1/(lambda (max - min)) over ALL tiles
    if constexpr (PASS == PC_PASS_WEIGHTS) {
        if (tile_mm != nullptr) {
            __shared__ float mn_s[NW], mx_s[NW];
            float mn = INFINITY, mx = -INFINITY;
            for (int i = tid; i < (int)gridDim.x; i += 64 * NW) { mn = fminf(mn, tile_mm[i]); mx = fmaxf(mx, tile_mm[rsc + i]); }
            mn = wave_min(mn); mx = wave_max(mx);
            if (lane == 0) { mn_s[wave_hw] = mn; mx_s[wave_hw] = mx; }
            __syncthreads();
            mn = mn_s[0]; mx = mx_s[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) { mn = fminf(mn, mn_s[w]); mx = fmaxf(mx, mx_s[w]); }
            nil_range = C->neg_inv_lambda / (mx - mn); // k_cost_minmax's expression
            if (blockIdx.x == 0 && tid == 0) { mm_out[0] = mn; mm_out[1] = mx - mn; mm_out[2] = nil_range; } // what the finish and the weights' export read
        } else {
            nil_range = mm_out[2];
        }
    }

    if (wave != 0) {
        // ------------------------------------------------------------------ producers
        const int p = wave - 1;
        const unsigned int gk = (unsigned int)C->k_offset + (unsigned int)(k0 + lane); // the global sample index: below 2^31 + 64
        const unsigned long long base = step_ctr[0] * (unsigned long long)NG;
        const unsigned long long seed = C->seed;
        // what the Philox rounds of every group of this lane share, once (blocks base * A .. (base + NG) * A - 1)
        const PhiloxLane plane = make_philox_lane(seed, gk, base * A, (base + (unsigned long long)NG) * A - 1);
        float eps_r[NREG];
        PcProducerConsts<A> pcst; // SGPR-resident copy: no constant re-fetch after the barriers
        pcst.template load<DIAG>(C);
        const PcProducerConsts<A> *PC = &pcst;
        MPPI_STAMP(16 + 10 * p + 9);
        auto produce = [&](auto ic, auto kindc) { // kindc: the action-cost form, resolved once below
            constexpr int i = decltype(ic)::value;
            constexpr int KIND = decltype(kindc)::value;
            const int g = NP * i + p;
            if (balance) pc_set_prio(i, nch, gen, balance);
            if (PASS == PC_PASS_WEIGHTS && i < nch && g < NG) { // the noise alone: nothing is published, no chunk barrier
                float z[4 * A];
                MPPI_NORMALS_GROUP_UB(A, seed, gk, plane, base + (unsigned long long)g, z);
#pragma unroll
                for (int tl = 0; tl < 4; ++tl) {
                    float zz[A], e[A];
#pragma unroll
                    for (int j = 0; j < A; ++j) zz[j] = z[tl * A + j];
                    scale_noise<A, DIAG>(PC, zz, e);
#pragma unroll
                    for (int j = 0; j < A; ++j) eps_r[(i * 4 + tl) * A + j] = e[j];
                }
            }
            if (PASS != PC_PASS_WEIGHTS && i < nch) { // chunk i exists (wave-uniform)
                float *cb = buf + (i & 1) * CH + (size_t)(4 * p) * SLOT * 64;
                if (g < NG) {
                    // the nominal actions of the group's 4 steps: scalar loads issued ahead of the Philox rounds that
                    // hide them (mPrepareAction controller_base.cpp:205-208); steps past the horizon are never consumed
                    float ug[4][A];
#pragma unroll
                    for (int tl = 0; tl < 4; ++tl) {
                        const int tt = min(4 * g + tl, H - 1);
#pragma unroll
                        for (int j = 0; j < A; ++j) ug[tl][j] = U_dev[tt * A + j];
                    }
                    float z[4 * A];
                    MPPI_NORMALS_GROUP_UB(A, seed, gk, plane, base + (unsigned long long)g, z);
#pragma unroll
                    for (int tl = 0; tl < 4; ++tl) {
                        const int t = 4 * g + tl;
                        float zz[A], e[A], u[A];
#pragma unroll
                        for (int j = 0; j < A; ++j) zz[j] = z[tl * A + j];
                        scale_noise<A, DIAG>(PC, zz, e);
                        // steps past the horizon (ragged last group) need no mask: the butterfly sums every column on its own and the
                        // columns with t >= H are never stored (r03: the e * keep multiply that used to zero them cost 0.3 us at C3)
                        float slot[SLOT];
#pragma unroll
                        for (int j = 0; j < SLOT; ++j) slot[j] = 0.0f;
#pragma unroll
                        for (int j = 0; j < A; ++j) {
                            u[j] = ug[tl][j];
                            eps_r[(i * 4 + tl) * A + j] = e[j];
                            slot[j] = u[j] + e[j]; // to_apply, :258
                        }
                        slot[A] = action_cost<A, DIAG, PcProducerConsts<A>, FMA, KIND>(PC, u, e);
                        if constexpr (PACKED) {
                            slot_t sv;
#pragma unroll
                            for (int j = 0; j < SLOT; ++j) sv[j] = slot[j];
                            *static_cast<slot_t *>(__builtin_assume_aligned(cb + (tl * 64 + lane) * SLOT, SLOT * 4)) = sv;
                        } else {
#pragma unroll
                            for (int j = 0; j <= A; ++j) cb[(tl * (A + 1) + j) * 64 + lane] = slot[j];
                        }
                    }
                }
                MPPI_STAMP(16 + 10 * p + (i < 7 ? i : 6));
                __syncthreads(); // chunk i published
            }
            if (!(i < nch && g < NG)) {
#pragma unroll
                for (int r = 0; r < 4 * A; ++r) eps_r[i * 4 * A + r] = 0.0f;
            }
        };
        // the action-cost form (C++ reference / Python gamma-upsilon form) is decided once, around the whole horizon loop — in the instances of
        // the step's one pass with the diagonal cost (the BASELINE configurations); the others keep the per-step test (half the code to compile)
        if constexpr (PASS == PC_PASS_PLAIN && (COST == PC_COST_DIAG || COST == PC_COST_DIAG_FMA)) {
            if (MPPI_PC_KIND_ONCE(pcst.action_cost_kind == MPPI_ACTION_COST_CPP)) static_for<0, NSLOT>([&](auto ic) { produce(ic, std::integral_constant<int, MPPI_PC_KIND_OF(MPPI_ACTION_COST_CPP)>{}); });
            else static_for<0, NSLOT>([&](auto ic) { produce(ic, std::integral_constant<int, MPPI_PC_KIND_OF(MPPI_ACTION_COST_PY)>{}); });
        } else {
            static_for<0, NSLOT>([&](auto ic) { produce(ic, std::integral_constant<int, -1>{}); });
        }
        __syncthreads(); // weights published by the consumer
        MPPI_STAMP(16 + 10 * p + 7);
        // phase C from registers: V_b[t,j] = Σ_k e_k·eps[k,t,j]  (mWeightedNoise, controller_base.cpp:188-192)
        const float w = w_s[lane];
#pragma unroll
        for (int r = 0; r < NREG; ++r) eps_r[r] = w * eps_r[r];
        float tot[(NREG + 63) / 64];
        MPPI_WAVE_TRANSPOSE_SUM(NREG, eps_r, tot, lane);
        const int colbase = lane_column(lane);
#pragma unroll
        for (int m = 0; m < (NREG + 63) / 64; ++m) {
            const int n = 64 * m + colbase;        // register index this lane owns the total of
            const int i = n / (4 * A), rem = n - i * (4 * A);
            const int tl = rem / A, j = rem - tl * A;
            const int t = 4 * (NP * i + p) + tl;
            if (n < NREG && t < H) rec[(size_t)(2 + t * A + j) * rsc] = tot[m];
        }
        MPPI_STAMP(16 + 10 * p + 8);
    } else {
        // ------------------------------------------------------------------ consumer
        float x[S];
#pragma unroll
        for (int i = 0; i < S; ++i) x[i] = x_dev[i];
        PcConsumerConsts<S> ccst;
        ccst.load(C);
        const PcConsumerConsts<S> *CC = &ccst;
        PcEllipseConsts ecst;
        PcDenseQConsts<S> qcst;
        if constexpr (COST == PC_COST_ELLIPSE) ecst.load(C);
        if constexpr (COST == PC_COST_DENSE) qcst.load(C);
        auto cost_of = [&](const float (&xs)[S]) {
            if constexpr (COST == PC_COST_ELLIPSE) return state_cost_ellipse<S>(&ecst, xs);
            else if constexpr (COST == PC_COST_DENSE) return state_cost_dense<S>(&qcst, xs);
            else return state_cost<S, false, PcConsumerConsts<S>, FMA>(CC, xs);
        };
        float c = 0.0f;
        MPPI_STAMP(0);
        MPPI_STAMP_RT(62);
        if constexpr (PASS == PC_PASS_WEIGHTS) c = cost[valid ? k0 + lane : 0]; // pass 1 left this step's costs there
        if constexpr (PASS != PC_PASS_WEIGHTS) {
        __syncthreads(); // chunk 0 published
        MPPI_STAMP(1);
        for (int ch = 0; ch < nch; ++ch) {
            if (balance) pc_set_prio(ch, nch, gen, balance, MPPI_PC_CONSUMER_BOOST);
            const float *cb = buf + (ch & 1) * CH;
            const int tend = min(CS, H - ch * CS);
            for (int tl = 0; tl < MPPI_ABL_CHUNK_STEPS(tend, ch); ++tl) {
                float v[A], ac;
                if constexpr (PACKED) {
                    const slot_t sv = *static_cast<const slot_t *>(__builtin_assume_aligned(cb + (tl * 64 + lane) * SLOT, SLOT * 4));
#pragma unroll
                    for (int j = 0; j < A; ++j) v[j] = sv[j];
                    ac = sv[A];
                } else {
#pragma unroll
                    for (int j = 0; j < A; ++j) v[j] = cb[(tl * (A + 1) + j) * 64 + lane];
                    ac = cb[(tl * (A + 1) + A) * 64 + lane];
                }
                pm_step<A, PcConsumerConsts<S>, FMA>(CC, x, v);
                const float sc = cost_of(x);                  // cost on the POST-step state
                const float tmp = sc + ac;                    // Step_cost_result cost_base.cpp:49
                c = c + tmp;                                  // path_cost        controller_base.cpp:268
            }
            // barrier budget: producers run nch (one per chunk) + 1 (weights); the consumer 1 + (nch-1) + 1.
            // After the last chunk nothing is published any more: the producers already sit at the weights barrier.
            MPPI_STAMP(2 + (ch < 7 ? ch : 6));
            if (ch + 1 < nch) __syncthreads(); // chunk ch consumed / chunk ch+1 published
        }
        c = c + cost_of(x); // terminal: x_H counted a second time, :271-272
        MPPI_STORE_COST(valid, cost + k0 + lane, c);
        } // PASS != PC_PASS_WEIGHTS
        // tile-local mBeta / mExpArg / mExp / mNabla (controller_base.cpp:166-182)
        const float beta = wave_min(valid ? c : INFINITY);
        if constexpr (PASS == PC_PASS_COSTS) { // the tile's cost range for the second pass
            const float cmax = wave_max(valid ? c : -INFINITY);
            if (lane == 0) { tile_mm[blockIdx.x] = beta; tile_mm[(size_t)rsc + blockIdx.x] = cmax; }
        }
        const float arg = (PASS == PC_PASS_WEIGHTS ? nil_range : CC->neg_inv_lambda) * (c - beta);
        const float ek = valid ? expf(arg) : 0.0f;
        const float eta = wave_sum(ek);
        w_s[lane] = ek;
        if (lane == 0) { rec[0] = beta; rec[(size_t)rsc] = eta; }
        MPPI_STAMP(9);
        MPPI_STAMP_RT(63);
        __syncthreads(); // weights published
        MPPI_TL_DUMP(valid, cost + k0 + lane);
    }
