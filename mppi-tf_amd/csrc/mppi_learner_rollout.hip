// mppi_learner_rollout.hip — trajectory validation of a learner batch (LearnerBase.validate_fold, learner_base.py:181-188, 211-216, 218-320):
// the B members' networks rolled open-loop along n given action sequences of T steps, ONE launch. k_lb_rollout: one LANE per trajectory,
// one wave per workgroup, grid (ceil(n / 64), B); a workgroup belongs to one member, stages that member's L tiles of P ([33][32]: rows
// 0..31 = W [in][out], row 32 = b) into LDS once, and every lane then reads the same weight address (an LDS broadcast). The step loop
// over T runs inside the kernel with the state in registers; the activations of a lane are one column of act_s [2][32][64] (no global
// scratch, and no barrier in the loop: a lane reads its own column only).
// The arithmetic is that of k_mlp_step_ref / k_nnauv_step_ref — NOT the learner's forward pass (bias first, explicit fma) — so that
// member m's trajectory is bit for bit the one a lone handle holding the member's weights returns from mppi_model_rollout:
//   inputs (x - Xmean) / Xstd, a division; acc = 0, acc = acc + cur[j] * W[j][o] for ascending j over the layer's TRUE input width
//   (the padding of the tiles is never added: acc + 0 would turn a -0 accumulator into +0), then + b[o]; relu on the hidden layers; mul
//   and add rounded separately (-ffp-contract=off). Four outputs share one pass over j (one broadcast float4 of weights per j): each
//   output's own sum is untouched, and an output past the layer's width is computed from the tile's zero padding and never read.
// Per step the lane optionally stores X[m, t+1, i, :] and accumulates e = X[t+1, i, j] - G[t+1, i, j]; sse[j] = sse[j] + e * e in fp32,
// t ascending, behind the row-0 term (X[0] - G[0])^2; the loads of V[t+1, i] and G[t+2, i] are issued before step t is computed. At the
// end each of the s sums goes through a fixed 6-level butterfly over the wave (lanes past n hold exact zeros and store nothing) and
// lane 0 writes part[m][block][j]; the host adds the blocks in order in fp64. No float atomics, no flag, no spin, nothing waits on
// another workgroup: any B x n is safe. A diverging member's NaN / Inf stays in its own workgroups.
#define MPPI_UNIT_BATCH_GEN // (mppi_gen.hip.h: its non-template kernels live in the gen unit)
#include "mppi_capi.hip.h"
#include "mppi_gen.hip.h"
#include "mppi_learner.hip.h"

using namespace mppi_lrn;

namespace {

constexpr int kTile = 33 * W32;

template <int KIND, int S, int A>
__global__ __launch_bounds__(kRollThreads) void k_lb_rollout(const LbRollout r)
{
    __shared__ __attribute__((aligned(16))) float w_s[kMaxLayers][kTile];
    __shared__ float act_s[2][W32][kRollThreads];
    const int lane = threadIdx.x, L = r.n_layers, m = blockIdx.y;
    {
        const float4 *src = reinterpret_cast<const float4 *>(r.P + (size_t)m * L * kTile); // kTile is a multiple of 4
        float4 *dst = reinterpret_cast<float4 *>(&w_s[0][0]);
        for (int e = lane; e < L * (kTile / 4); e += kRollThreads) dst[e] = src[e];
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * kRollThreads + lane, n = (size_t)r.n;
    float sse[S];
#pragma unroll
    for (int j = 0; j < S; ++j) sse[j] = 0.0f;
    if (i < n) {
        const bool has_g = r.G != nullptr;
        float *X = r.X != nullptr ? r.X + (size_t)m * ((size_t)r.T + 1) * n * S : nullptr;
        float xs[S], vn[A], gn[S];
#pragma unroll
        for (int j = 0; j < S; ++j) { xs[j] = r.x0[(r.kx == 1 ? 0 : i) * S + j]; gn[j] = 0.0f; }
#pragma unroll
        for (int j = 0; j < A; ++j) vn[j] = r.V[i * A + j];
        if (X != nullptr) {
#pragma unroll
            for (int j = 0; j < S; ++j) X[i * S + j] = xs[j];
        }
        if (has_g) {
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const float e = xs[j] - r.G[i * S + j];
                sse[j] = sse[j] + e * e;
                gn[j] = r.G[(n + i) * S + j];
            }
        }
        for (int t = 0; t < r.T; ++t) {
            float vs[A], gs[S];
#pragma unroll
            for (int j = 0; j < A; ++j) vs[j] = vn[j];
#pragma unroll
            for (int j = 0; j < S; ++j) gs[j] = gn[j];
            if (t + 1 < r.T) { // the next step's action and ground truth, in flight while this step is computed
#pragma unroll
                for (int j = 0; j < A; ++j) vn[j] = r.V[((size_t)(t + 1) * n + i) * A + j];
                if (has_g) {
#pragma unroll
                    for (int j = 0; j < S; ++j) gn[j] = r.G[((size_t)(t + 2) * n + i) * S + j];
                }
            }
            // the network's inputs into column `lane` of act_s[0]
            float *cur = &act_s[0][0][lane], *nxt = &act_s[1][0][lane];
            if constexpr (KIND == MPPI_MODEL_MLP) {
#pragma unroll
                for (int j = 0; j < S; ++j) cur[j * kRollThreads] = (xs[j] - r.xmean[j]) / r.xstd[j];
#pragma unroll
                for (int j = 0; j < A; ++j) cur[(S + j) * kRollThreads] = (vs[j] - r.xmean[S + j]) / r.xstd[S + j];
            } else if constexpr (KIND == MPPI_MODEL_NN_AUV) {
#pragma unroll
                for (int j = 0; j < S - 3; ++j) cur[j * kRollThreads] = (xs[3 + j] - r.xmean[j]) / r.xstd[j];
#pragma unroll
                for (int j = 0; j < A; ++j) cur[(S - 3 + j) * kRollThreads] = (vs[j] - r.xmean[S - 3 + j]) / r.xstd[S - 3 + j];
            } else { // NNAUVModelSpeed.prepare_data: Euler angles, velocities, forces
                const float q[4] = {xs[3], xs[4], xs[5], xs[6]};
                float eu[3];
                euler_from_quat<false>(q, eu);
#pragma unroll
                for (int j = 0; j < 3; ++j) cur[j * kRollThreads] = (eu[j] - r.xmean[j]) / r.xstd[j];
#pragma unroll
                for (int j = 0; j < 6; ++j) cur[(3 + j) * kRollThreads] = (xs[7 + j] - r.xmean[3 + j]) / r.xstd[3 + j];
#pragma unroll
                for (int j = 0; j < A; ++j) cur[(9 + j) * kRollThreads] = (vs[j] - r.xmean[9 + j]) / r.xstd[9 + j];
            }
            for (int l = 0; l < L; ++l) {
                const int width = r.width[l], out_w = r.width[l + 1];
                const bool hidden = l + 1 < L;
                const float *wl = w_s[l];
                for (int o = 0; o < out_w; o += 4) { // o + 3 <= 31: inside the tile and inside act_s
                    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 8 // eight rows' LDS reads in flight; the additions stay in ascending j
                    for (int j = 0; j < width; ++j) {
                        const float c = cur[j * kRollThreads];
                        const float4 w = *reinterpret_cast<const float4 *>(wl + j * W32 + o);
                        a0 = a0 + c * w.x; a1 = a1 + c * w.y; a2 = a2 + c * w.z; a3 = a3 + c * w.w;
                    }
                    const float4 b = *reinterpret_cast<const float4 *>(wl + W32 * W32 + o);
                    a0 = a0 + b.x; a1 = a1 + b.y; a2 = a2 + b.z; a3 = a3 + b.w;
                    nxt[(o + 0) * kRollThreads] = (hidden && a0 < 0.0f) ? 0.0f : a0; // relu on hidden layers
                    nxt[(o + 1) * kRollThreads] = (hidden && a1 < 0.0f) ? 0.0f : a1;
                    nxt[(o + 2) * kRollThreads] = (hidden && a2 < 0.0f) ? 0.0f : a2;
                    nxt[(o + 3) * kRollThreads] = (hidden && a3 < 0.0f) ? 0.0f : a3;
                }
                float *sw = cur; cur = nxt; nxt = sw;
            }
            if constexpr (KIND == MPPI_MODEL_NN_AUV_SPEED) {
                float delta[6];
#pragma unroll
                for (int o = 0; o < 6; ++o) delta[o] = cur[o * kRollThreads] * r.ystd[o] + r.ymean[o];
                nnauv_speed_next_state<false>(r.dt, xs, delta);
            } else {
#pragma unroll
                for (int o = 0; o < S; ++o) xs[o] = xs[o] + (cur[o * kRollThreads] * r.ystd[o] + r.ymean[o]);
            }
            if (X != nullptr) {
                const size_t row = (size_t)(t + 1) * n + i;
#pragma unroll
                for (int j = 0; j < S; ++j) X[row * S + j] = xs[j];
            }
            if (has_g) {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const float e = xs[j] - gs[j];
                    sse[j] = sse[j] + e * e;
                }
            }
        }
    }
    if (r.part == nullptr) return; // uniform
#pragma unroll
    for (int j = 0; j < S; ++j) {
        float v = sse[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
        if (lane == 0) r.part[((size_t)m * r.blocks + blockIdx.x) * S + j] = v;
    }
}

template <int KIND, int S, int A>
hipError_t launch(const LbRollout &r, int B, hipStream_t st)
{
    hipLaunchKernelGGL((k_lb_rollout<KIND, S, A>), dim3((unsigned)r.blocks, (unsigned)B), dim3(kRollThreads), 0, st, r);
    return hipGetLastError();
}

} // namespace

hipError_t mppi_lrn_launch_rollout(const LbRollout &r, int B, hipStream_t st)
{
    if (r.kind == MPPI_MODEL_NN_AUV && r.s == kGenS && r.a == kGenA) return launch<MPPI_MODEL_NN_AUV, kGenS, kGenA>(r, B, st);
    if (r.kind == MPPI_MODEL_NN_AUV_SPEED && r.s == kGenS && r.a == kGenA) return launch<MPPI_MODEL_NN_AUV_SPEED, kGenS, kGenA>(r, B, st);
    if (r.kind != MPPI_MODEL_MLP || r.s != 2 * r.a) return hipErrorInvalidValue;
    switch (r.a) {
    case 1: return launch<MPPI_MODEL_MLP, 2, 1>(r, B, st);
    case 2: return launch<MPPI_MODEL_MLP, 4, 2>(r, B, st);
    case 3: return launch<MPPI_MODEL_MLP, 6, 3>(r, B, st);
    case 4: return launch<MPPI_MODEL_MLP, 8, 4>(r, B, st);
    default: return hipErrorInvalidValue;
    }
}
