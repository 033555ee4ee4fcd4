// mppi_mlp2.hip.h — k_rollout_mlp2: the learned 2x256 MLP model_base in exact fp32 on the matrix cores, second design
// (BASELINE configs[3]/[4]). Included by mppi_kernels.hip.h.
//
// The fact this kernel is built around (tools/micro/mfma_f32_shadow.hip, profiles/r02_mfma_f32_shadow.json): the
// f32-input MFMA runs at the f32 vector rate and does NOT overlap with the vector ALU. Beside v_mfma_f32_32x32x2_f32
// (64 cycles) every vector instruction of the same wave adds its own 4-5 cycles, every [MFMA, MFMA, vector lump]
// excursion ~18 more, and inside a lump every instruction of the wave — an s_waitcnt, an s_nop, a ds_read — costs an
// issue slot like a v_fma; only BETWEEN back-to-back MFMAs are LDS, scalar and wait instructions free. So the bound of
// this path is (MFMA cycles + vector cycles), not the MFMA peak alone, and the design minimises vector instructions and
// excursions instead of trying to hide them:
//   * ONE wave per SIMD (4 waves, 256 threads, the unified 512-entry register file): wave w owns hidden units
//     [64w, 64w+64) of both layers = two 32-row M-tiles = 2 x 128 stationary W2 registers = exactly the accumulator
//     half (a0-a255), pinned there through inline-asm MFMAs — hipcc left alone keeps them in v0-v255 and spills; the
//     layer-2 bias is the accumulators' initial value (8 LDS reads per set and step) instead of a 129th k pair;
//   * TWO sets of 32 rollouts (one 32-column MFMA tile each: 2 x 16 accumulator registers per set), each with its own
//     h1 image in LDS (2 x 32 KB), software-pipelined against each other: while the 258 layer-2 MFMAs of one set
//     stream, the other set's step is finished and its next one prepared in ~13 LUMPS of vector work (8 of layer 3 at
//     4 accumulator registers each, partial-sum exchange, state update + costs + next inputs, relu) and 10 layer-1
//     MFMAs. Both workgroup barriers of a step fall in mid-stream with the next B operands already requested;
//   * packed math where it halves the count (v_pk_fma_f32 costs one v_fma_f32 here): layer 3 is 1 v_max + 3 v_pk_fma
//     per accumulator register; output pairs travel through LDS side by side (one 8-byte read per pair);
//   * LDS requests trickle (a few per k pair, issued between the two MFMAs and the lump — behind a lump each would
//     hold the next MFMA back), and hipcc is made to wait for a lump's operands one k pair early;
//   * the workgroup is persistent: it walks over tiles blockIdx.x, + gridDim.x, ... with the weights loaded once.
// History (r02, K=65536 H=64, fp32 peak 157.3): k_rollout_mlp 122 TFLOP/s (0.77; 8 waves in lock-step phases) -> this
// design with 64-rollout sets 108 (weight spills) -> 32-rollout sets, work spread one piece per MFMA "to hide it" 120
// (the opposite of what the hardware wants: 258 excursions) -> lumps 131 -> waits/requests out of the lumps 135 ->
// one-statement swaps, 4-register lumps 137-138 -> bias as accumulator init 141 (harness; 143 in bench.py's timing). Measured floor of the MFMAs alone: 156 (tools/micro/mlp2_bench.hip,
// ablation 2047).
// Arithmetic is k_rollout_mlp's up to the reciprocal (multiplication by 1/sigma; v_mfma_f32_32x32x2_f32 = a k-ordered
// fmaf chain; the cross-wave sum of layer 3 has 4 terms instead of 8): the parity tests hold it to the same bars.
// LDS at a_dim = 3: 2 x 32 KB images + partial sums 6 KB + W3 8 KB + noise 6 KB + W1 10 KB + U = ~96 KB.
// The kernel's body is mppi_mlp2_body.inc: k_rollout_mlp2_batch (mppi_mlp_batch.hip.h) runs the same text on one member's operands.
#pragma once

// Timing-only ablations for tools/micro/mlp2_bench.hip (results are wrong with any bit set; the product builds with 0):
// 1 no layer 3 / state update of the other set, 2 no preparation (inputs, layer 1, relu, image) of the other set,
// 4 no mid-stream barriers, 8 no noise generation; single lumps: 16 layer 3, 32 partial-sum store, 64 state update and
// cost, 128 inputs of the next step, 256 layer 1, 512 relu, 1024 the LDS requests of the lumps,
// 2048 h1 image writes.
#ifndef MPPI_MLP2_ABL
#define MPPI_MLP2_ABL 0
#endif

namespace mppi {

// (MPPI_MLP2_STAMP_AT / MPPI_MLP2_TRACE_*: the timing-study layer, mppi_ablate.hip.h — nothing in the shipped build)

constexpr int kMlp2Threads = 256;
constexpr int kMlp2R = 64; // rollouts per workgroup: two sets of 32
__host__ __device__ inline size_t mlp2_lds_floats(int S, int A, int H)
{
    return (size_t)2 * kHid * 32 + 2 * 4 * S * 32 + kHid * 8 + 2 * 2 * 4 * A * 32 + (size_t)((S + A + 2) / 2 * 2) * kHid +
           (size_t)(H * A + 3) / 4 * 4 + kHid + 64;
}

// lanes 32-63 of a <-> lanes 0-31 of b (v_permlane32_swap; asm: see the transposing butterfly in mppi_device.hip.h)
__device__ __forceinline__ void permlane32_swap(float &a, float &b)
{
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
// the odd 16-lane rows of a <-> the even 16-lane rows of b (v_permlane16_swap)
__device__ __forceinline__ void permlane16_swap(float &a, float &b)
{
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

template <int A, bool DIAG, int SRC>
__global__ __launch_bounds__(kMlp2Threads, 1) void k_rollout_mlp2(
    const DevConsts *__restrict__ C, const MlpDev *__restrict__ M, const float *__restrict__ x_dev,
    const float *__restrict__ U_dev, const float *__restrict__ eps_hbm,
    const unsigned long long *__restrict__ step_ctr, float *__restrict__ cost, float *__restrict__ partials,
    const int MODE, const int rsb, const int rsc)
{
#include "mppi_mlp2_body.inc"
}

} // namespace mppi
