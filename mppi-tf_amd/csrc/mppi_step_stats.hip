// mppi_step_stats.hip — the step statistics (include/mppi_c.h: mppi_step_stats, mppi_batch_step_stats; the episodes that log them call
// launch_step_stats from mppi_capi_step.hip): what the reference's observer logs per control step (observer_base.py:101-187) — effective
// sample size, entropy of the weights, moments and extremes of the sample costs, the best sample, two histograms — from what every
// rollout path leaves on the device: the sample costs, beta | eta, and the cost buffer and temperature MPPI_DBG_WEIGHTS weighs
// (weight_inputs, mppi_capi.hip.h). Kernel of this unit: k_step_stats. It reads those and writes its own rows: no buffer a step reads.
//
// One workgroup of 1024 threads per member. Thread t owns the 4-sample groups t, t + 1024, ... in ascending order (loaded
// four groups ahead, used in that order), whatever
// the alignment of the member's costs (16-byte loads where they are aligned, four 4-byte loads of the same samples where not): a member of
// a batch adds in the order its lone handle does. Every floating sum is fp64 — the lane's partial over its samples in index order, a
// 64-lane butterfly, then the 16 wave totals from LDS in wave order — so the result is a function of the inputs, the block size and K.
// Compiled like the rest with -ffp-contract=off: arg = t * (c' - beta) rounds twice in fp32, as in k_weights.
#include <climits>
#include <cmath>
#include <cstdint>

#include "mppi_capi.hip.h"

namespace {

constexpr int kStatThreads = 1024, kStatWaves = kStatThreads / 64, kBins = MPPI_STEP_STAT_BINS;
// a histogram in LDS: 32 copies of every bin, lane l adds to copy l & 31 — word (bin * 32 + copy) lies in bank `copy`, so the 32 lanes of
// an LDS lane group never share a bank, however many samples fall into one bin (a needle puts all K into one). Integer adds: any order.
constexpr int kCopies = 32;
// groups a thread loads before it uses the first: one workgroup has only its own waves to hide the memory latency behind
constexpr int kAhead = 4;

struct StepStatsArgs {
    const DevConsts *consts;             // member m: consts + m
    const float *cost, *cost_w;          // raw costs / the costs the weights were made from, member m: + m * K
    const float *beta_eta;               // member m: + 8 m
    const float *nil_dev;                // the step's temperature where it is not lambda, or NULL
    int K;
    float *stats;                        // [B][9]
    uint32_t *hist_cost, *hist_weight;   // [B][32] each
};

__device__ __forceinline__ double stat_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
// the block's total on every thread: wave totals through LDS, added in wave order
__device__ __forceinline__ double stat_block_sum(double v, double *red, int tid)
{
    v = stat_wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < kStatWaves; ++w) s = s + red[w];
    return s;
}
// the four samples of group g (n of them exist) from a buffer whose alignment `vec` describes
__device__ __forceinline__ void stat_load4(const float *p, bool vec, int i0, int n, float (&c)[4])
{
    if (vec && n == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p + i0);
        c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = j < n ? p[i0 + j] : 0.0f;
    }
}
// min(31, (int)v) for every finite v >= 0; defined beyond: negative -> 0, NaN and +inf -> 31
__device__ __forceinline__ int stat_bin(float v) { return v < 31.0f ? (v > 0.0f ? (int)v : 0) : kBins - 1; }

__global__ void __launch_bounds__(kStatThreads) k_step_stats(const StepStatsArgs a)
{
    __shared__ double red[kStatWaves];
    __shared__ float mn_s[kStatWaves], mx_s[kStatWaves];
    __shared__ int mi_s[kStatWaves], cnt_s[kStatWaves];
    __shared__ unsigned hc_s[kBins * kCopies], hw_s[kBins * kCopies];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.x;
    const int K = a.K, NG = (K + 3) >> 2;
    const float *cost = a.cost + (size_t)m * K, *cost_w = a.cost_w + (size_t)m * K, *be = a.beta_eta + 8 * (size_t)m;
    const bool same = a.cost_w == a.cost;
    const bool vec = (reinterpret_cast<uintptr_t>(cost) & 15) == 0, vec_w = (reinterpret_cast<uintptr_t>(cost_w) & 15) == 0;
    for (int i = tid; i < kBins * kCopies; i += kStatThreads) { hc_s[i] = 0u; hw_s[i] = 0u; }

    // ---- pass 1: how many costs are finite, their sum, maximum, and the minimum with its lowest index
    int cnt = 0, mi = INT_MAX;
    float mx = -INFINITY, mn = INFINITY;
    double sum = 0.0;
    for (int g0 = tid; g0 < NG; g0 += kAhead * kStatThreads) {
        float c[kAhead][4];
        int n[kAhead];
#pragma unroll
        for (int q = 0; q < kAhead; ++q) { // the loads of kAhead groups in flight before the first is used
            const int g = g0 + q * kStatThreads;
            n[q] = g < NG ? min(4, K - 4 * g) : 0;
            stat_load4(cost, vec, 4 * g, n[q], c[q]);
        }
#pragma unroll
        for (int q = 0; q < kAhead; ++q) {
            const int i0 = 4 * (g0 + q * kStatThreads);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n[q] && isfinite(c[q][j])) {
                    cnt += 1;
                    sum = sum + (double)c[q][j];
                    mx = fmaxf(mx, c[q][j]);
                    if (c[q][j] < mn) { mn = c[q][j]; mi = i0 + j; } // ascending indices: the first of equals stays
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        const float omn = __shfl_xor(mn, off, 64);
        const int omi = __shfl_xor(mi, off, 64);
        if (omn < mn || (omn == mn && omi < mi)) { mn = omn; mi = omi; }
    }
    if (lane == 0) { cnt_s[wave] = cnt; mx_s[wave] = mx; mn_s[wave] = mn; mi_s[wave] = mi; }
    sum = stat_block_sum(sum, red, tid); // (its barriers publish the four arrays and the zeroed histograms too)
    cnt = cnt_s[0]; mx = mx_s[0]; mn = mn_s[0]; mi = mi_s[0];
    for (int w = 1; w < kStatWaves; ++w) {
        cnt += cnt_s[w];
        mx = fmaxf(mx, mx_s[w]);
        if (mn_s[w] < mn || (mn_s[w] == mn && mi_s[w] < mi)) { mn = mn_s[w]; mi = mi_s[w]; }
    }
    const double mean = sum / (double)cnt;
    const float scale = mx == mn ? 0.0f : 32.0f / (mx - mn);

    // ---- pass 2: the weights' sums, the squared deviations, the histograms
    const float beta = be[0], t = a.nil_dev != nullptr ? a.nil_dev[0] : a.consts[m].neg_inv_lambda;
    double S1 = 0.0, S2 = 0.0, T = 0.0, V = 0.0;
    const int copy = lane & (kCopies - 1);
    for (int g0 = tid; g0 < NG; g0 += kAhead * kStatThreads) {
        float c[kAhead][4], cw[kAhead][4];
        int n[kAhead];
#pragma unroll
        for (int q = 0; q < kAhead; ++q) {
            const int g = g0 + q * kStatThreads;
            n[q] = g < NG ? min(4, K - 4 * g) : 0;
            stat_load4(cost, vec, 4 * g, n[q], c[q]);
            if (!same) stat_load4(cost_w, vec_w, 4 * g, n[q], cw[q]);
        }
#pragma unroll
        for (int q = 0; q < kAhead; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n[q] && isfinite(c[q][j])) {
                    const float arg = t * ((same ? c[q][j] : cw[q][j]) - beta);
                    const float e = expf(arg);
                    S1 = S1 + (double)e;
                    S2 = S2 + (double)e * (double)e;
                    if (e > 0.0f) T = T + (double)e * (double)arg; // e = 0: the term's limit, never 0 * -inf
                    const double d = (double)c[q][j] - mean;
                    V = V + d * d;
                    atomicAdd(&hc_s[stat_bin((c[q][j] - mn) * scale) * kCopies + copy], 1u);
                    atomicAdd(&hw_s[stat_bin(-arg * 1.442695f) * kCopies + copy], 1u);
                }
            }
        }
    }
    S1 = stat_block_sum(S1, red, tid);
    S2 = stat_block_sum(S2, red, tid);
    T = stat_block_sum(T, red, tid);
    V = stat_block_sum(V, red, tid); // (behind its barriers every histogram add is visible)

    if (tid == 0) {
        float *o = a.stats + (size_t)m * MPPI_N_STEP_STATS;
        const double nan = (double)NAN;
        o[MPPI_STAT_BETA] = be[0];
        o[MPPI_STAT_ETA] = be[1];
        o[MPPI_STAT_ESS] = (float)(cnt ? S1 * S1 / S2 : nan);
        o[MPPI_STAT_ENTROPY] = (float)(cnt ? log(S1) - T / S1 : nan);
        o[MPPI_STAT_COST_MEAN] = (float)(cnt ? mean : nan);
        o[MPPI_STAT_COST_STD] = (float)(cnt ? sqrt(V / (double)cnt) : nan);
        o[MPPI_STAT_COST_MAX] = cnt ? mx : NAN;
        o[MPPI_STAT_BEST_INDEX] = cnt ? (float)mi : -1.0f;
        o[MPPI_STAT_N_NONFINITE] = (float)(K - cnt);
    }
    if (tid < 2 * kBins) {
        const unsigned *src = (tid < kBins ? hc_s : hw_s) + (tid & (kBins - 1)) * kCopies;
        unsigned n = 0u;
        for (int k = 0; k < kCopies; ++k) n += src[(k + tid) & (kCopies - 1)]; // (rotated: the lanes read 32 different banks)
        (tid < kBins ? a.hist_cost : a.hist_weight)[(size_t)m * kBins + (tid & (kBins - 1))] = n;
    }
}

} // namespace

namespace mppi_capi {

const char *step_stats_refusal(const mppi_handle *h, mppi_status *st)
{
    *st = MPPI_ERR_UNSUPPORTED;
    if (h->shard_count != 1) return "step statistics: a sharded handle holds the costs of one rank, not the step's";
    if (h->K_local >= (1 << 24)) return "step statistics: 2^24 or more samples per member (the best sample's index would not be exact as a float)";
    *st = MPPI_OK;
    return nullptr;
}

hipError_t launch_step_stats(mppi_handle *h, hipStream_t st, float *stats, uint32_t *hist_cost, uint32_t *hist_weight)
{
    const WeightInputs w = weight_inputs(h, 0); // member m: every pointer of member 0's + m strides (a batch has no normalizeCost buffers)
    const StepStatsArgs a{w.consts, h->d_cost, w.cost_w, w.beta_eta, w.nil_dev, h->K_local, stats, hist_cost, hist_weight};
    hipLaunchKernelGGL(k_step_stats, dim3((unsigned)members(h)), dim3(kStatThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace mppi_capi

// the statistics of the last step of every member (a lone handle: one), through a scratch of B rows
static mppi_status step_stats_host(mppi_handle *h, float *stats, uint32_t *hist_cost, uint32_t *hist_weight)
{
    mppi_status why = MPPI_OK;
    if (const char *msg = step_stats_refusal(h, &why)) return fail(h, why, msg);
    if (!h->stats_step) return fail(h, MPPI_ERR_INVALID_ARG, "step statistics: no step has run yet (or mppi_update has rewritten beta and eta since)");
    MPPI_ENTER(h);
    const size_t B = (size_t)members(h), ns = B * MPPI_N_STEP_STATS, nh = B * MPPI_STEP_STAT_BINS;
    float *d = nullptr;
    HIP_TRY(h, hipMalloc((void **)&d, sizeof(float) * (ns + 2 * nh)));
    uint32_t *dhc = reinterpret_cast<uint32_t *>(d + ns), *dhw = dhc + nh;
    hipError_t e = launch_step_stats(h, h->stream, d, dhc, dhw);
    if (e == hipSuccess && stats) e = hipMemcpyAsync(stats, d, sizeof(float) * ns, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && hist_cost) e = hipMemcpyAsync(hist_cost, dhc, sizeof(uint32_t) * nh, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && hist_weight) e = hipMemcpyAsync(hist_weight, dhw, sizeof(uint32_t) * nh, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d);
    HIP_TRY(h, e);
    return MPPI_OK;
}

extern "C" mppi_status mppi_step_stats(mppi_handle *h, float *stats, uint32_t *hist_cost, uint32_t *hist_weight)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (h->batch) return fail(h, MPPI_ERR_UNSUPPORTED, "mppi_step_stats: a batched handle reports its statistics through mppi_batch_step_stats");
    return step_stats_host(h, stats, hist_cost, hist_weight);
}

extern "C" mppi_status mppi_batch_step_stats(mppi_handle *h, float *stats, uint32_t *hist_cost, uint32_t *hist_weight)
{
    MPPI_BATCH_ONLY(h);
    return step_stats_host(h, stats, hist_cost, hist_weight);
}
