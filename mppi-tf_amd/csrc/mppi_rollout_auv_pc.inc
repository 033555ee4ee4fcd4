// mppi_rollout_auv_pc.inc — the body of the Fossen AUVModel's two-wave rollout kernel, included as the body of k_rollout_auv_pc
// (MPPI_AUV_BATCH 0) and of k_rollout_auv_pc_batch (MPPI_AUV_BATCH 1), both in mppi_gen.hip.h: the pattern of mppi_rollout_pc.inc. A
// textual body, so that the lone controller's instances compile to exactly the code they had. With MPPI_AUV_BATCH 1 every per-member
// operand moves to member m's (x, U, costs, records, and C: member m's DevConsts with its Philox key, goal, lambda, gamma, upsilon, Sigma
// and Q); the arithmetic of every sample (noise, the two waves' Runge-Kutta stages, the cost, the tile record) is the same text.
    constexpr int S = kGenS, A = kGenA;
    __shared__ float g_s[2][2][6][64];    // [tile of the workgroup][barrier parity][restoring forces g(eta) of the stage state][rollout]   A -> B
    __shared__ float vel_s[2][2][6][64];  // [tile][barrier parity][velocities of the stage state][rollout]                       B -> A
    __shared__ float act_s[2][2][7][64];  // [tile][step parity][perturbed action v, action cost][rollout]                        A -> B (v), A keeps the cost
    __shared__ float cost_s[2][64];
    __shared__ int simd_s[4];
    const int H = C->H, HA = H * A, K = C->K_local;
    const int NG = (H + 3) / 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_hw = __builtin_amdgcn_readfirstlane(tid >> 6);
    int pair = wave_hw >> 1, role = wave_hw & 1; // role 0 = velocity wave (the heavier one), 1 = pose wave
    {
        const int simd = (int)__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4); // HW_REG_HW_ID[5:4]
        if (lane == 0) simd_s[wave_hw] = simd;
        __syncthreads();
        const int s0 = simd_s[0], s1 = simd_s[1], s2 = simd_s[2], s3 = simd_s[3];
        if (balance && ((1 << s0) | (1 << s1) | (1 << s2) | (1 << s3)) == 15) {
            const int gen = (int)(blockIdx.x >> 8);
            pair = simd & 1;
            role = ((simd >> 1) ^ gen) & 1;
        }
        pair = __builtin_amdgcn_readfirstlane(pair);
        role = __builtin_amdgcn_readfirstlane(role);
    }
#if MPPI_AUV_BATCH
    // member m = blockIdx.x / W of the batch (W = (n_tiles + 1) / 2 workgroups per member): its own x, U, costs, records (PcBatchArgs) and
    // constants C[m] (H and K above are shared). tile_ok and valid below are judged against the member's own tile count and K.
    const int member = (int)blockIdx.x / ((n_tiles + 1) >> 1);
    const int tile = 2 * ((int)blockIdx.x - member * ((n_tiles + 1) >> 1)) + pair;
    C += member;
    x_dev += (size_t)member * S;
    U_dev += (size_t)member * bt.u_stride;
    cost += (size_t)member * K;
    partials += (size_t)member * bt.rec_stride;
#else
    const int tile = 2 * (int)blockIdx.x + pair;
#endif
    const bool tile_ok = tile < n_tiles; // the second tile of the last workgroup may not exist: its waves still keep every barrier
    const int k0 = tile * 64;
    const bool valid = tile_ok && (k0 + lane) < K;
    const int kk = min(k0 + lane, K - 1);
    const int rk = G->rk;
    const float dt = G->dt;
    int nbar = 0; // barriers passed so far: the parity of the stage hand-off buffers (the same sequence in both waves)

    if (role == 0) {
        // ================================================================================= wave B: velocities
        AuvLocal al;
        al.load(G);
        float vel[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) vel[i] = x_dev[7 + i];
        // stage hand-off: publish the stage state's velocities, barrier, fetch its restoring forces (the one piece of the velocity rates that
        // is a function of the quaternion alone: the pose wave evaluates it)
        auto swap_stage = [&](const float (&vs)[6], float (&gs)[6]) {
#pragma unroll
            for (int i = 0; i < 6; ++i) vel_s[pair][nbar & 1][i][lane] = vs[i];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 6; ++i) gs[i] = g_s[pair][nbar & 1][i][lane];
            ++nbar;
        };
        for (int t = 0; t < H; ++t) {
            float q[6], v[A], k1[6], tmp[6]; // (q: g(eta) of the stage state)
            swap_stage(vel, q);
#pragma unroll
            for (int i = 0; i < A; ++i) v[i] = act_s[pair][t & 1][i][lane]; // to_apply of step t (wave A prepared it a step ahead)
            auv_vel_rates_g(&al, q, vel, v, k1);
            if (rk == 2) {
                float vs[6], k2[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) vs[i] = vel[i] + dt * k1[i];
                swap_stage(vs, q);
                auv_vel_rates_g(&al, q, vs, v, k2);
#pragma unroll
                for (int i = 0; i < 6; ++i) tmp[i] = (dt / 2.0f) * (k1[i] + k2[i]);
            } else if (rk == 4) { // the reference's formula, k4*dt inside the sum (:299-300)
                float vs[6], k2[6], k3[6], k4[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) vs[i] = vel[i] + (dt * k1[i]) / 2.0f;
                swap_stage(vs, q);
                auv_vel_rates_g(&al, q, vs, v, k2);
#pragma unroll
                for (int i = 0; i < 6; ++i) vs[i] = vel[i] + (dt * k2[i]) / 2.0f;
                swap_stage(vs, q);
                auv_vel_rates_g(&al, q, vs, v, k3);
#pragma unroll
                for (int i = 0; i < 6; ++i) vs[i] = vel[i] + dt * k3[i];
                swap_stage(vs, q);
                auv_vel_rates_g(&al, q, vs, v, k4);
                const float sixth = (float)(1.0 / 6.0);
#pragma unroll
                for (int i = 0; i < 6; ++i) tmp[i] = (sixth * ((k1[i] + 2.0f * k2[i]) + (2.0f * k3[i] + k4[i] * dt))) * dt;
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i) tmp[i] = k1[i] * dt;
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) vel[i] = vel[i] + tmp[i];
        }
        float q_unused[6];
        swap_stage(vel, q_unused); // the velocities of x_H for wave A's last step cost and the terminal cost
    } else {
        // ================================================================================= wave A: pose, cost, noise
        if (balance) __builtin_amdgcn_s_setprio(3); // (one round of the grid only: beyond it the age order staggers the workgroups' phases, as in k_rollout_pc)
        // the wave a stage waits for goes first on its SIMD (measured: this one — 0.1366 ms without priorities, 0.1342 with the
                                       // velocity wave first, 0.1278 with this one first; the other kind fills the gaps)
        GenQuadConsts qc;
        const bool quad_diag = C->state_cost_kind == MPPI_STATE_COST_QUADRATIC && !C->q_full;
#pragma unroll
        for (int i = 0; i < S; ++i) { qc.goal[i] = C->goal[i]; qc.qdiag[i] = C->qdiag[i]; }
        PcProducerConsts<A> pcst; // Sigma, Sigma^-1, lambda: a kernel-local copy (no re-fetch behind the barriers)
        pcst.template load<DIAG>(C);
        const unsigned long long base = step_ctr[0] * (unsigned long long)NG;
        const unsigned long long seed = C->seed;
        const unsigned long long gk = (unsigned long long)C->k_offset + (unsigned long long)kk;
        auto cost_of = [&](const float (&xs)[S]) { return quad_diag ? state_cost<S, false>(&qc, xs) : gen_state_cost(C, G, xs); };
        float x[S], c = 0.0f, z[4 * A];
#pragma unroll
        for (int i = 0; i < S; ++i) x[i] = x_dev[i];
        // v = u + eps and the action cost of step t -> act_s[t & 1] (mPrepareAction / mPrepareNoise, controller_base.cpp:205-213, :258)
        auto prepare = [&](int t) {
            float e[A], u[A];
            if (SRC == SRC_PHILOX) {
                if ((t & 3) == 0) normals_group<A>(seed, gk, base + (unsigned long long)(t >> 2), z);
                float z1[A];
                const int tl = t & 3; // wave-uniform: four statically indexed copies instead of a dynamically indexed register array
                if (tl == 0) { _Pragma("unroll") for (int i = 0; i < A; ++i) z1[i] = z[i]; }
                else if (tl == 1) { _Pragma("unroll") for (int i = 0; i < A; ++i) z1[i] = z[A + i]; }
                else if (tl == 2) { _Pragma("unroll") for (int i = 0; i < A; ++i) z1[i] = z[2 * A + i]; }
                else { _Pragma("unroll") for (int i = 0; i < A; ++i) z1[i] = z[3 * A + i]; }
                scale_noise<A, DIAG>(&pcst, z1, e);
            } else {
#pragma unroll
                for (int i = 0; i < A; ++i) e[i] = eps_hbm[(size_t)kk * HA + t * A + i];
            }
#pragma unroll
            for (int i = 0; i < A; ++i) { u[i] = U_dev[t * A + i]; act_s[pair][t & 1][i][lane] = u[i] + e[i]; }
            act_s[pair][t & 1][6][lane] = action_cost<A, DIAG>(&pcst, u, e);
        };
        // stage hand-off: publish the restoring forces g(eta) of the stage state (auv_restoring: a function of its quaternion alone, and this
        // wave has the time the velocity wave lacks), barrier, fetch its velocities
        struct { float fng_z, fnb_z, cog[3], cob[3]; } rl;
        rl.fng_z = G->fng_z; rl.fnb_z = G->fnb_z;
#pragma unroll
        for (int i = 0; i < 3; ++i) { rl.cog[i] = G->cog[i]; rl.cob[i] = G->cob[i]; }
        auto swap_stage = [&](const float (&ps)[7], float (&vs)[6]) {
            const float q4[4] = {ps[3], ps[4], ps[5], ps[6]};
            float g6[6];
            auv_restoring(&rl, q4, g6);
#pragma unroll
            for (int i = 0; i < 6; ++i) g_s[pair][nbar & 1][i][lane] = g6[i];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 6; ++i) vs[i] = vel_s[pair][nbar & 1][i][lane];
            ++nbar;
        };
        prepare(0);
        for (int t = 0; t < H; ++t) {
            float pose[7], vel[6], k1[7], tmp[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) pose[i] = x[i];
            swap_stage(pose, vel);
            if (t >= 1) { // the state step t-1 produced is complete now: its cost, with that step's action cost
#pragma unroll
                for (int i = 0; i < 6; ++i) x[7 + i] = vel[i];
                const float sc = cost_of(x);                           // cost on the POST-step state
                const float step_c = sc + act_s[pair][(t - 1) & 1][6][lane]; // Step_cost_result cost_base.cpp:49
                c = c + step_c;                                        // path_cost        controller_base.cpp:268
            }
            const float q0[4] = {pose[3], pose[4], pose[5], pose[6]};
            auv_pose_rates(q0, vel, k1);
            if (rk == 2) {
                float ps[7], vs[6], k2[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) ps[i] = pose[i] + dt * k1[i];
                swap_stage(ps, vs);
                const float q1[4] = {ps[3], ps[4], ps[5], ps[6]};
                auv_pose_rates(q1, vs, k2);
#pragma unroll
                for (int i = 0; i < 7; ++i) tmp[i] = (dt / 2.0f) * (k1[i] + k2[i]);
            } else if (rk == 4) {
                float ps[7], vs[6], k2[7], k3[7], k4[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) ps[i] = pose[i] + (dt * k1[i]) / 2.0f;
                swap_stage(ps, vs);
                { const float qq[4] = {ps[3], ps[4], ps[5], ps[6]}; auv_pose_rates(qq, vs, k2); }
#pragma unroll
                for (int i = 0; i < 7; ++i) ps[i] = pose[i] + (dt * k2[i]) / 2.0f;
                swap_stage(ps, vs);
                { const float qq[4] = {ps[3], ps[4], ps[5], ps[6]}; auv_pose_rates(qq, vs, k3); }
#pragma unroll
                for (int i = 0; i < 7; ++i) ps[i] = pose[i] + dt * k3[i];
                swap_stage(ps, vs);
                { const float qq[4] = {ps[3], ps[4], ps[5], ps[6]}; auv_pose_rates(qq, vs, k4); }
                const float sixth = (float)(1.0 / 6.0);
#pragma unroll
                for (int i = 0; i < 7; ++i) tmp[i] = (sixth * ((k1[i] + 2.0f * k2[i]) + (2.0f * k3[i] + k4[i] * dt))) * dt;
            } else {
#pragma unroll
                for (int i = 0; i < 7; ++i) tmp[i] = k1[i] * dt;
            }
#pragma unroll
            for (int i = 0; i < 7; ++i) x[i] = x[i] + tmp[i];
            normalize_quat(x);
            if (t + 1 < H) prepare(t + 1); // a step ahead: wave B reads it right behind the next step's first barrier
        }
        float pose[7], vel[6];
#pragma unroll
        for (int i = 0; i < 7; ++i) pose[i] = x[i];
        swap_stage(pose, vel);
#pragma unroll
        for (int i = 0; i < 6; ++i) x[7 + i] = vel[i];
        const float sc = cost_of(x);
        c = c + (sc + act_s[pair][(H - 1) & 1][6][lane]);
        c = c + sc; // terminal cost: x_H counted a second time, controller_base.cpp:271-272
        cost_s[pair][lane] = c;
        if (valid) cost[k0 + lane] = c;
    }
    __syncthreads();
    if (MODE == MODE_COST_ONLY || !tile_ok) return;
    const float ct = cost_s[pair][lane];
    mlp_tile_record<A, DIAG, 2>(C, ct, valid, role, lane, kk, H, NG, SRC, eps_hbm, C->seed, (unsigned long long)C->k_offset + (unsigned long long)kk,
                                step_ctr[0] * (unsigned long long)NG, partials + (size_t)record_slot(tile, rsc) * rsb, rsc);
