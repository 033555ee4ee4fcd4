// mppi_nn_batch.hip.h — k_rollout_nn_batch: the rollouts of B learned 13-state controllers (NNAUVModel, NNAUVModelSpeed), each member with
// its OWN network, in one launch. The arithmetic is k_rollout_gen<MODEL, HID, DIAG>'s (mppi_gen.hip.h) in SRC_PHILOX / MODE_ROLLOUT: the
// same device functions in the same order (normals_group, scale_noise, action_cost, nnauv_step / nnauv_speed_step, gen_state_cost, the
// terminal re-add, mlp_tile_record), so member m's costs and record carry the bits of the lone handle's on that kernel.
//   * grid: a flat B * nb workgroups of one wave; member m = blockIdx.x / nb, tile = blockIdx.x % nb — both wave-uniform, so everything
//     indexed by m (constants, network, normalisation) stays on the scalar path;
//   * member m's operands: constants C + m (Philox key, sigma, lambda, goal, Q), x at x_dev + 13 m, U at U_dev + m * u_stride, costs at
//     cost + m K, records in the lone layout at partials + m * rec_stride (PcBatchArgs, as k_rollout_auv_pc_batch), its network: MlpDev
//     M + m (normalisation, ystd / ymean) and the padded layer pointers P[m] of a device table;
//   * the weights come through the scalar cache as in the lone kernel (the opaque zero offset keeps their loads inside the horizon loop);
//   * no flag, counter or spin across workgroups: any B runs, whether or not the grid is resident in one round of the chip.
#pragma once
#include "mppi_gen.hip.h"

namespace mppi {

template <int MODEL, int HID, bool DIAG>
__global__ __launch_bounds__(64) void k_rollout_nn_batch(
    const DevConsts *__restrict__ C, const GenConsts *__restrict__ G, const MlpDev *__restrict__ M, const MlpSmallArgs *__restrict__ P,
    const float *__restrict__ x_dev, const float *__restrict__ U_dev, const unsigned long long *__restrict__ step_ctr,
    float *__restrict__ cost, float *__restrict__ partials, const int rsb, const int rsc, const PcBatchArgs bt)
{
    static_assert(MODEL == GEN_MODEL_NNAUV || MODEL == GEN_MODEL_NNAUV_SPEED, "the learned 13-state models");
    constexpr int S = kGenS, A = kGenA;
    const int member = (int)blockIdx.x / bt.nb;
    const int tile = (int)blockIdx.x - member * bt.nb;
    C += member;
    M += member;
    P += member;
    x_dev += (size_t)member * S;
    U_dev += (size_t)member * bt.u_stride;
    cost += (size_t)member * C->K_local;
    partials += (size_t)member * bt.rec_stride;
    const int H = C->H, K = C->K_local;
    const int NG = (H + 3) / 4;
    const int lane = threadIdx.x;
    const int k0 = tile * 64;
    const bool valid = (k0 + lane) < K;
    const int kk = valid ? k0 + lane : K - 1; // lanes past K recompute the last sample, outside every sum
    const unsigned long long base = step_ctr[0] * (unsigned long long)NG;
    const unsigned long long seed = C->seed;
    const unsigned long long gk = (unsigned long long)C->k_offset + (unsigned long long)kk;
    const float *W0[kMlpSmallMaxLayers], *b0[kMlpSmallMaxLayers]; // member m's padded layers
#pragma unroll
    for (int l = 0; l < kMlpSmallMaxLayers; ++l) { W0[l] = P->W[l]; b0[l] = P->b[l]; }
    const int n_hidden = P->n_layers - 1;
    float c = 0.0f;
    float xm[kGenNin], xr[kGenNin];
#pragma unroll
    for (int i = 0; i < kGenNin; ++i) { xm[i] = M->xmean[i]; xr[i] = 1.0f / M->xstd[i]; } // (the speed model uses 15 of the 16)
    float x[S];
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = x_dev[i];
    float z[4 * A];
    for (int t = 0; t < H; ++t) {
        if ((t & 3) == 0) normals_group<A>(seed, gk, base + (unsigned long long)(t >> 2), z);
        float u[A], e[A], v[A], z1[A];
#pragma unroll
        for (int i = 0; i < A; ++i) { // z[(t & 3) * A + i] without a dynamically indexed register array
            float zi = z[i];
#pragma unroll
            for (int tl = 1; tl < 4; ++tl) zi = (t & 3) == tl ? z[tl * A + i] : zi;
            z1[i] = zi;
        }
        scale_noise<A, DIAG>(C, z1, e);
#pragma unroll
        for (int i = 0; i < A; ++i) { u[i] = U_dev[t * A + i]; v[i] = u[i] + e[i]; } // to_apply, controller_base.cpp:258
        const float ac = action_cost<A, DIAG>(C, u, e);
        int zoff; // opaque zero offset: keeps the weight loads inside the horizon loop (see k_rollout_mlp_small)
        asm("s_mov_b32 %0, 0" : "=s"(zoff) : "s"(t));
        const float *Wp[kMlpSmallMaxLayers], *bp[kMlpSmallMaxLayers];
#pragma unroll
        for (int l = 0; l < kMlpSmallMaxLayers; ++l) { Wp[l] = W0[l] + zoff; bp[l] = b0[l] + zoff; }
        if (MODEL == GEN_MODEL_NNAUV_SPEED) nnauv_speed_step<HID>(C, M, Wp, bp, n_hidden, xm, xr, x, v);
        else nnauv_step<HID>(M, Wp, bp, n_hidden, xm, xr, x, v);
        const float sc = gen_state_cost(C, G, x); // cost on the POST-step state
        const float tmp = sc + ac;                // Step_cost_result cost_base.cpp:49
        c = c + tmp;                              // path_cost        controller_base.cpp:268
    }
    c = c + gen_state_cost(C, G, x); // terminal cost, controller_base.cpp:271-272
    if (valid) cost[k0 + lane] = c;
    mlp_tile_record<A, DIAG, 1>(C, c, valid, 0, lane, kk, H, NG, SRC_PHILOX, nullptr, seed, gk, base,
                                partials + (size_t)record_slot(tile, rsc) * rsb, rsc);
}

} // namespace mppi
