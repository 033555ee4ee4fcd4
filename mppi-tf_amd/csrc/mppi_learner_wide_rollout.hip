// mppi_learner_wide_rollout.hip — trajectory validation of a WIDE learner batch (LearnerBase.validate_fold, learner_base.py:181-188,
// 211-216, 218-320, for the [3a, 256, 256, 2a] network of an MPPI_MODEL_MLP controller): the B members' networks rolled open-loop along n
// given action sequences of T steps, ONE launch. What mppi_learner_rollout.hip is to the narrow batch; not that kernel with bigger
// constants, because a member's second layer is 256 KB and does not fit in LDS.
// k_wb_rollout<A>: 256 threads, one per hidden unit; grid (ceil(n / 16), B). A workgroup owns R = 16 trajectories of ONE member for all T
// steps and reads the member's weights in place from the batch's padded block P [B][kWideParams] (no copy, no repacking):
//   layer 0  thread o holds column o of W0 (3a weights and the bias) in registers for the whole call and keeps R accumulators; the R
//            normalised inputs of row j come from the LDS tile in_s [3a][R] as broadcast float4s
//   layer 1  thread o keeps R accumulators and walks j = 0..255 ascending; W1[j][o] streams from L2 (a row is 1 KB, contiguous across the
//            workgroup; the next eight rows are in flight while eight are added), the R activations of row j are broadcast float4s of
//            act_s[0][j][R]
//   layer 2  thread (r, o), r < R, o < 2a (at most 128 threads): a serial sum over the 256 rows of act_s[1] against the 2a live columns
//            of W2, staged once per workgroup as w2_s [257][2a]. The thread keeps x[r][o] in a register over the steps, writes the next
//            step's normalised input into in_s, optionally stores X[m, t+1, i, o] and accumulates its squared error
// The arithmetic is that of k_mlp_step_ref — NOT the wide learner's forward pass (matrix-core tiles round differently) — so that member
// m's trajectory is bit for bit the one a lone handle holding the member's weights returns from mppi_model_rollout:
//   inputs (x - Xmean) / Xstd, a division; acc = 0, acc = acc + cur[j] * W[j][o] for ascending j over the layer's TRUE input width (3a for
//   layer 0: the padded rows of the layout are never added, acc + 0 would turn a -0 accumulator into +0), then + b[o] (row 32 / 256 / 256
//   of the layout); relu on the two hidden layers; x' = x + (y * Ystd + Ymean); mul and add rounded separately (-ffp-contract=off).
// Squared error: e = X[t+1, i, j] - G[t+1, i, j]; sse = sse + e * e in fp32 per (trajectory, component), t ascending behind the row-0 term
// (X[0] - G[0])^2; the loads of V[t+1, i] and G[t+2, i] are issued before step t is computed. At the end the R sums of a component go
// through a fixed pairwise tree of 4 levels and one value per (member, block, component) goes to part; the host adds the blocks in order in
// fp64. Only __syncthreads() between the layers, reached by every thread: trajectories past n compute on zeros, store nothing and add
// nothing; no early return, no flag, no spin, no float atomics, nothing waits on another workgroup: any B x n is safe. A diverging member's
// NaN / Inf stays in its own workgroups.
#include <hip/hip_runtime.h>

#include "mppi_learner.hip.h"

using namespace mppi_lrn;

namespace {

constexpr int kH = kWideHidden;
constexpr int R = kWideRollR;
constexpr int kAhead = 8; // rows of W1 in flight per thread

// acc[r] = acc[r] + row[r] * w for the R trajectories of an LDS row (every lane reads the same address: a broadcast)
__device__ __forceinline__ void row_add(float (&acc)[R], const float *row, float w)
{
#pragma unroll
    for (int q = 0; q < R / 4; ++q) {
        const float4 c = *reinterpret_cast<const float4 *>(row + 4 * q);
        acc[4 * q + 0] = acc[4 * q + 0] + c.x * w;
        acc[4 * q + 1] = acc[4 * q + 1] + c.y * w;
        acc[4 * q + 2] = acc[4 * q + 2] + c.z * w;
        acc[4 * q + 3] = acc[4 * q + 3] + c.w * w;
    }
}

// + bias, relu, into row o of an activation tile
__device__ __forceinline__ void row_store(const float (&acc)[R], float b, float *row)
{
#pragma unroll
    for (int q = 0; q < R / 4; ++q) {
        float4 z;
        z.x = acc[4 * q + 0] + b; z.y = acc[4 * q + 1] + b; z.z = acc[4 * q + 2] + b; z.w = acc[4 * q + 3] + b;
        z.x = z.x < 0.0f ? 0.0f : z.x; z.y = z.y < 0.0f ? 0.0f : z.y; z.z = z.z < 0.0f ? 0.0f : z.z; z.w = z.w < 0.0f ? 0.0f : z.w;
        *reinterpret_cast<float4 *>(row + 4 * q) = z;
    }
}

template <int A>
__global__ __launch_bounds__(kH) void k_wb_rollout(const WbRollout p)
{
    constexpr int S = 2 * A, IN = 3 * A;
    __shared__ __attribute__((aligned(16))) float act_s[2][kH][R]; // 32 KB
    __shared__ __attribute__((aligned(16))) float in_s[IN][R];
    __shared__ float w2_s[(kH + 1) * S];                            // rows 0..255 = W2[:, :S], row 256 = b2[:S]
    __shared__ float red_s[R * S];
    const int tid = threadIdx.x, m = blockIdx.y;
    const float *__restrict__ P0 = p.P + (size_t)m * kWideParams, *__restrict__ P1 = P0 + kWideOff[1], *__restrict__ P2 = P0 + kWideOff[2];
    float w0[IN];
#pragma unroll
    for (int j = 0; j < IN; ++j) w0[j] = P0[j * kH + tid];
    const float b0 = P0[W32 * kH + tid], b1 = P1[kH * kH + tid];
    for (int e = tid; e < (kH + 1) * S; e += kH) w2_s[e] = P2[(e / S) * W32 + e % S];
    // the output side: thread (r, o) of the first R * S threads owns component o of trajectory i, and action component o where o < A
    const bool out_t = tid < R * S;
    const int r = out_t ? tid / S : 0, o = out_t ? tid % S : 0;
    const size_t n = (size_t)p.n, i = (size_t)blockIdx.x * R + r;
    const bool live = out_t && i < n, act_t = live && o < A, has_g = p.G != nullptr;
    float *X = p.X != nullptr ? p.X + (size_t)m * ((size_t)p.T + 1) * n * S : nullptr;
    const float xmean = p.xmean[o], xstd = p.xstd[o], vmean = p.xmean[o < A ? S + o : 0], vstd = p.xstd[o < A ? S + o : 0];
    const float ymean = p.ymean[o], ystd = p.ystd[o];
    float x = 0.0f, vn = 0.0f, gn = 0.0f, sse = 0.0f;
    if (live) {
        x = p.x0[(p.kx == 1 ? 0 : i) * S + o];
        if (X != nullptr) X[i * S + o] = x;
        if (has_g) {
            const float e = x - p.G[i * S + o];
            sse = sse + e * e;
            gn = p.G[(n + i) * S + o];
        }
    }
    if (act_t) vn = p.V[i * A + o];
    for (int t = 0; t < p.T; ++t) {
        const float v = vn, g = gn;
        if (t + 1 < p.T) { // the next step's action and ground truth, in flight while this step is computed
            if (act_t) vn = p.V[((size_t)(t + 1) * n + i) * A + o];
            if (live && has_g) gn = p.G[((size_t)(t + 2) * n + i) * S + o];
        }
        float wn[kAhead]; // the first rows of W1, in flight across layer 0
#pragma unroll
        for (int q = 0; q < kAhead; ++q) wn[q] = P1[q * kH + tid];
        if (out_t) {
            in_s[o][r] = (x - xmean) / xstd;
            if (o < A) in_s[S + o][r] = (v - vmean) / vstd;
        }
        __syncthreads(); // in_s is written (the first step: and w2_s); act_s[1] of the previous step has been read
        float acc[R];
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = 0.0f;
#pragma unroll
        for (int j = 0; j < IN; ++j) row_add(acc, in_s[j], w0[j]);
        row_store(acc, b0, act_s[0][tid]);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = 0.0f;
        for (int j0 = 0; j0 < kH; j0 += kAhead) {
            float w[kAhead];
#pragma unroll
            for (int q = 0; q < kAhead; ++q) w[q] = wn[q];
            if (j0 + kAhead < kH) {
#pragma unroll
                for (int q = 0; q < kAhead; ++q) wn[q] = P1[(j0 + kAhead + q) * kH + tid];
            }
#pragma unroll
            for (int q = 0; q < kAhead; ++q) row_add(acc, act_s[0][j0 + q], w[q]); // ascending j
        }
        row_store(acc, b1, act_s[1][tid]);
        __syncthreads();
        if (out_t) {
            float y = 0.0f;
#pragma unroll 8 // eight rows' LDS reads in flight; the additions stay in ascending j
            for (int j = 0; j < kH; ++j) y = y + act_s[1][j][r] * w2_s[j * S + o];
            y = y + w2_s[kH * S + o];
            x = x + (y * ystd + ymean);
            if (live) {
                if (X != nullptr) X[((size_t)(t + 1) * n + i) * S + o] = x;
                if (has_g) {
                    const float e = x - g;
                    sse = sse + e * e;
                }
            }
        }
    }
    if (p.part == nullptr) return; // uniform, behind the last barrier
    if (out_t) red_s[o * R + r] = sse; // a trajectory past n holds an exact zero
    __syncthreads();
    if (tid < S) {
        float s[R];
#pragma unroll
        for (int q = 0; q < R; ++q) s[q] = red_s[tid * R + q];
#pragma unroll
        for (int w = 1; w < R; w *= 2) {
#pragma unroll
            for (int q = 0; q < R; q += 2 * w) s[q] = s[q] + s[q + w];
        }
        p.part[((size_t)m * p.blocks + blockIdx.x) * S + tid] = s[0];
    }
}

template <int A>
hipError_t launch(const WbRollout &p, int B, hipStream_t st)
{
    hipLaunchKernelGGL((k_wb_rollout<A>), dim3((unsigned)p.blocks, (unsigned)B), dim3(kH), 0, st, p);
    return hipGetLastError();
}

} // namespace

hipError_t mppi_lrn_launch_wide_rollout(const WbRollout &p, int B, hipStream_t st)
{
    if (p.s != 2 * p.a || p.blocks != (p.n + R - 1) / R) return hipErrorInvalidValue;
    switch (p.a) {
    case 1: return launch<1>(p, B, st);
    case 2: return launch<2>(p, B, st);
    case 3: return launch<3>(p, B, st);
    case 4: return launch<4>(p, B, st);
    default: return hipErrorInvalidValue;
    }
}
