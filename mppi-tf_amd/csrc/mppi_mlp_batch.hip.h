// mppi_mlp_batch.hip.h — the rollouts of B learned point-mass controllers (MPPI_MODEL_MLP), each member with its OWN network, in one
// launch (mppi_create_batch_mlp; instantiated per action dimension in mppi_launch_batch_mlp.hip).
//
// k_rollout_mlp2_batch<A, DIAG>: the [3a, 256, 256, 2a] network. k_rollout_mlp2 is weight-stationary per WORKGROUP — W2 in registers, W1 /
// W3 / b2 in LDS, loaded once before the tile walk — so a member axis is addressing only: the grid is (min(nb, n_cu), B), workgroup
// (x, m) applies member m's offsets to its operands before the first load and then runs k_rollout_mlp2's body (mppi_mlp2_body.inc, the
// very text the lone kernel includes) in SRC_PHILOX / MODE_ROLLOUT, walking member m's tiles x, x + gridDim.x, ... Member m's costs and
// records therefore carry the bits of its lone handle on the DEFAULT matrix-core kernel k_rollout_mlp2<A, DIAG, SRC_PHILOX>; the
// resources are that kernel's (one wave per SIMD, ~96 KB of LDS at a = 3).
//
// k_rollout_mlp_small_batch<A, HID>: the Dense(16|32) x 1..3 networks, k_rollout_mlp_small's arithmetic (mppi_mlp_small.hip.h) in
// SRC_PHILOX / MODE_ROLLOUT with member m's padded layer pointers from a device table, as k_rollout_nn_batch (mppi_nn_batch.hip.h):
// a flat grid of B * nb one-wave workgroups, member = blockIdx.x / nb, everything indexed by it on the scalar path — the weights too
// (mlp_gptr below: 99 s_load_dwordx16 per step at <3, 32> as in the lone kernel, no vector load of a weight).
//
// Member m's operands in both: constants C + m, network M + m (and P + m), x at x_dev + 2 a m, U at U_dev + m * u_stride, costs at
// cost + m K, records in the lone layout at partials + m * rec_stride (PcBatchArgs). No flag, counter or spin across workgroups: any B
// runs, whether or not the grid is resident in one round of the chip.
#pragma once

namespace mppi {

template <int A, bool DIAG>
__global__ __launch_bounds__(kMlp2Threads, 1) void k_rollout_mlp2_batch(
    const DevConsts *__restrict__ C, const MlpDev *__restrict__ M, const float *__restrict__ x_dev,
    const float *__restrict__ U_dev, const unsigned long long *__restrict__ step_ctr, float *__restrict__ cost,
    float *__restrict__ partials, const int rsb, const int rsc, const PcBatchArgs bt)
{
    constexpr int SRC = SRC_PHILOX, MODE = MODE_ROLLOUT;
    const float *const eps_hbm = nullptr; // (SRC_HBM's operand: no statement of the body reads it here)
    const int member = (int)blockIdx.y;
    C += member;
    M += member;
    x_dev += (size_t)member * (2 * A);
    U_dev += (size_t)member * bt.u_stride;
    cost += (size_t)member * C->K_local;
    partials += (size_t)member * bt.rec_stride;
#include "mppi_mlp2_body.inc"
}

// A layer pointer read from the member's table has lost the kernel-argument provenance that keeps k_rollout_mlp_small's weight loads
// scalar: as a generic pointer its loads become flat vector loads of one address for all lanes. Cast to the global address space, a
// wave-uniform load from memory the kernel does not write is a scalar load again (s_load_dwordx*), and the weights enter v_pk_fma_f32 as
// SGPR pairs as in the lone kernel.
typedef const float __attribute__((address_space(1))) *mlp_gptr;

// dense_pairs (mppi_mlp_small.hip.h) on global-address-space weights: the same expressions in the same order
template <int IN, int OUT2, bool RELU>
__device__ __forceinline__ void dense_pairs_g(mlp_gptr W, mlp_gptr b, const float (&in)[IN], f32x2s (&out)[OUT2])
{
    constexpr int OUT = 2 * OUT2;
#pragma unroll
    for (int i = 0; i < IN; ++i) {
        const f32x2s x2 = {in[i], in[i]};
#pragma unroll
        for (int o2 = 0; o2 < OUT2; ++o2) {
            const f32x2s w2 = {W[i * OUT + 2 * o2], W[i * OUT + 2 * o2 + 1]};
            out[o2] = i == 0 ? x2 * w2 : __builtin_elementwise_fma(x2, w2, out[o2]);
        }
    }
#pragma unroll
    for (int o2 = 0; o2 < OUT2; ++o2) {
        out[o2] = out[o2] + f32x2s{b[2 * o2], b[2 * o2 + 1]};
        if (RELU) { out[o2].x = fmaxf(out[o2].x, 0.0f); out[o2].y = fmaxf(out[o2].y, 0.0f); }
    }
}

template <int A, int HID>
__global__ __launch_bounds__(64) void k_rollout_mlp_small_batch(
    const DevConsts *__restrict__ C, const MlpDev *__restrict__ M, const MlpSmallArgs *__restrict__ P, const float *__restrict__ x_dev,
    const float *__restrict__ U_dev, const unsigned long long *__restrict__ step_ctr, float *__restrict__ cost,
    float *__restrict__ partials, const int rsb, const int rsc, const PcBatchArgs bt)
{
    constexpr int S = 2 * A, NIN = S + A, H2 = HID / 2;
    constexpr bool QFULL = false, DIAG = false;
    static_assert(HID % 2 == 0 && S % 2 == 0, "outputs are handled as pairs");
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
    mlp_gptr W0[kMlpSmallMaxLayers], b0[kMlpSmallMaxLayers]; // member m's layers
#pragma unroll
    for (int l = 0; l < kMlpSmallMaxLayers; ++l) { W0[l] = (mlp_gptr)P->W[l]; b0[l] = (mlp_gptr)P->b[l]; }
    const int n_hidden = P->n_layers - 1;

    float xm[NIN], xr[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) { xm[i] = M->xmean[i]; xr[i] = 1.0f / M->xstd[i]; }
    float x[S], c = 0.0f;
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = x_dev[i];

    float z[4 * A];
    for (int t = 0; t < H; ++t) {
        int zoff; // opaque zero offset: keeps the weight loads inside the horizon loop (see k_rollout_mlp_small)
        asm("s_mov_b32 %0, 0" : "=s"(zoff) : "s"(t));
        mlp_gptr Wp[kMlpSmallMaxLayers], bp[kMlpSmallMaxLayers];
#pragma unroll
        for (int l = 0; l < kMlpSmallMaxLayers; ++l) { Wp[l] = W0[l] + zoff; bp[l] = b0[l] + zoff; }
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
        for (int i = 0; i < A; ++i) { u[i] = U_dev[t * A + i]; v[i] = u[i] + e[i]; }
        const float ac = action_cost<A, DIAG>(C, u, e);

        float in[NIN];
#pragma unroll
        for (int i = 0; i < S; ++i) in[i] = (x[i] - xm[i]) * xr[i];
#pragma unroll
        for (int i = 0; i < A; ++i) in[S + i] = (v[i] - xm[S + i]) * xr[S + i];
        f32x2s ha[H2], hb[H2];
        float hin[HID];
        dense_pairs_g<NIN, H2, true>(Wp[0], bp[0], in, ha);
        for (int l = 1; l < n_hidden; ++l) { // wave-uniform trip count, the same code for every hidden layer
#pragma unroll
            for (int o2 = 0; o2 < H2; ++o2) { hin[2 * o2] = ha[o2].x; hin[2 * o2 + 1] = ha[o2].y; }
            const mlp_gptr Wl = l == 1 ? Wp[1] : Wp[2], bl = l == 1 ? bp[1] : bp[2];
            dense_pairs_g<HID, H2, true>(Wl, bl, hin, hb);
#pragma unroll
            for (int o2 = 0; o2 < H2; ++o2) ha[o2] = hb[o2];
        }
#pragma unroll
        for (int o2 = 0; o2 < H2; ++o2) { hin[2 * o2] = ha[o2].x; hin[2 * o2 + 1] = ha[o2].y; }
        f32x2s y[S / 2];
        const mlp_gptr Wo = n_hidden == 1 ? Wp[1] : (n_hidden == 2 ? Wp[2] : Wp[3]);
        const mlp_gptr bo = n_hidden == 1 ? bp[1] : (n_hidden == 2 ? bp[2] : bp[3]);
        dense_pairs_g<HID, S / 2, false>(Wo, bo, hin, y);
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const float yi = (i & 1) ? y[i / 2].y : y[i / 2].x;
            x[i] = x[i] + (yi * M->ystd[i] + M->ymean[i]);
        }
        const float sc = state_cost<S, QFULL>(C, x); // cost on the POST-step state
        const float tmp = sc + ac;
        c = c + tmp;
    }
    c = c + state_cost<S, QFULL>(C, x); // terminal cost, controller_base.cpp:271-272
    if (valid) cost[k0 + lane] = c;
    mlp_tile_record<A, DIAG, 1>(C, c, valid, 0, lane, kk, H, NG, SRC_PHILOX, nullptr, seed, gk, base,
                                partials + (size_t)record_slot(tile, rsc) * rsb, rsc);
}

} // namespace mppi
