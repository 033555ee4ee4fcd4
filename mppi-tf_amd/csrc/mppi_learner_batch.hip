// mppi_learner_batch.hip — B narrow learners in the launches of one (LearnerBase.k_fold_validation / grid_search,
// scripts/src/learners/learner_base.py:83-216: k copies of the network, one per fold, each with its own Adam, times a grid of rates).
// Every member is the learner of mppi_learner.hip — the same three kernels with a member axis in the grid — and is bit-identical to a
// lone mppi_learner given the member's rows: the kernels below are copies of k_learn_fwd_bwd / k_learn_grad / k_learn_adam whose
// arithmetic, and the order of every sum, is untouched (loss blocks of 256 rows and gradient chunks of 512 rows BY POSITION in the
// member's index list, four waves on interleaved sample pairs, partial tiles summed in wave order, then in chunk order).
// What differs is addressing only:
//   * one pool X [n][in], Y [n][out] for all members; member m reads row train_idx[m][i] where the lone learner reads row i
//   * weights, both Adam moments ([B][L][33][32]: rows 0..31 = W, row 32 = b), activations and deltas ([B][L][cap][32]), partial
//     tiles ([B][chunks][L][33][32]) and loss partials ([B][blocks]) at member-strided offsets
//   * members differ in n_train: the grid is sized by the largest, a workgroup past its member's range returns before any barrier
//   * per-member lr, beta1, beta2, eps from a device array; one step counter for the batch
// The held-out loss (kfold_step: _train_step, then evaluate) is a fourth launch per step, k_lb_test: the forward pass alone over the
// member's test rows with the weights the update just wrote, one partial per 256 rows; the partials are summed in block order by the
// next step's forward launch (workgroup 0 of the member) and, for the last step of a call, by one k_lb_test_sum.
// Launches per Adam step: 3, or 4 when test losses are asked for and some member has test rows. No float atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "mppi_learner.hip.h"

using namespace mppi_lrn; // W32, kMaxLayers

namespace {

constexpr int kChunk = 512;       // samples per workgroup of k_lb_grad: mppi_learner.hip's kChunk (the chunk boundaries are part of the sum's order)
constexpr int kGradThreads = 256;
constexpr int kTile = 33 * W32;   // one layer's parameters: rows 0..31 = W [in][out] padded, row 32 = b
constexpr int kMaxMembers = 1024;
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LbArgs { // by value to every kernel; device pointers
    int n_layers, width[kMaxLayers + 1];
    float *P, *M, *V;                      // [B][L][33][32]
    const float *X, *Y;                    // the pool
    const int *train_idx, *test_idx;       // [B][cap_train], [B][cap_test]: validated on the host (set_split), never out of [0, n)
    const int *n_train, *n_test;           // [B]
    int cap_train, cap_test;               // the largest n_train / n_test: strides of the index lists and of A, D
    float *A, *D;                          // [B][L][cap_train][32]
    float *part;                           // [B][chunks_max][L][33][32]
    float *loss_part, *test_part;          // [B][blocks_max], [B][tblocks_max]
    int chunks_max, blocks_max, tblocks_max;
    int *step;
};

__device__ __forceinline__ void lb_stage(const float *__restrict__ Pm, int L, float (*w_s)[W32 * W32], float (*b_s)[W32], int tid)
{
    for (int l = 0; l < L; ++l) {
        for (int i = tid; i < W32 * W32; i += 256) w_s[l][i] = Pm[(size_t)l * kTile + i];
        if (tid < W32) b_s[l][tid] = Pm[(size_t)l * kTile + W32 * W32 + tid];
    }
}

// k_learn_fwd_bwd's forward pass of one row: a[l] = input of layer l; a[L] = the prediction
__device__ __forceinline__ void lb_forward(const float (*w_s)[W32 * W32], const float (*b_s)[W32], int L, int nin, const float *__restrict__ xrow,
                                           float (&a)[kMaxLayers + 1][W32])
{
#pragma unroll
    for (int j = 0; j < W32; ++j) a[0][j] = j < nin ? xrow[j] : 0.0f;
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l) {
        if (l < L) {
#pragma unroll
            for (int o = 0; o < W32; ++o) {
                float acc = b_s[l][o];
#pragma unroll
                for (int j = 0; j < W32; ++j) acc = __builtin_fmaf(a[l][j], w_s[l][j * W32 + o], acc);
                a[l + 1][o] = (l + 1 < L && acc < 0.0f) ? 0.0f : acc; // relu on the hidden layers
            }
        }
    }
}

// the row's squared error, summed over the outputs in order; d = scale * (pred - y)
__device__ __forceinline__ float lb_error(const float (&a)[kMaxLayers + 1][W32], int L, int nout, bool valid, const float *__restrict__ yrow, float scale,
                                          float (&d)[W32])
{
    float se = 0.0f;
#pragma unroll
    for (int o = 0; o < W32; ++o) {
        float pred = 0.0f;
#pragma unroll
        for (int l = 1; l <= kMaxLayers; ++l) pred = l == L ? a[l][o] : pred;
        const float e = (o < nout && valid) ? pred - yrow[o] : 0.0f;
        se += e * e;
        d[o] = scale * e;
    }
    return se;
}

// block sum of the squared errors, fixed order (all 256 threads; red_s is free again after the caller's next barrier)
__device__ __forceinline__ float lb_block_sum(float se, float *red_s, int tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
    if ((tid & 63) == 0) red_s[tid >> 6] = se;
    __syncthreads();
    return ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
}

// member m's held-out loss from the partials k_lb_test left: block order, then the mean. No test rows: NaN, never a perfect 0.
__device__ __forceinline__ void lb_test_sum(const LbArgs &g, int m, float *__restrict__ out)
{
    const int n = g.n_test[m];
    if (n == 0) { out[m] = __builtin_nanf(""); return; }
    float s = 0.0f;
    for (int q = 0; q < (n + 255) / 256; ++q) s += g.test_part[(size_t)m * g.tblocks_max + q];
    out[m] = s / ((float)n * (float)g.width[g.n_layers]);
}

// grid (blocks_max, B). One sample per thread: forward, squared error, backward (k_learn_fwd_bwd with a member axis and a row gather).
// test_prev (or NULL): where workgroup 0 of each member leaves the previous step's held-out loss.
__global__ __launch_bounds__(256) void k_lb_fwd_bwd(const LbArgs g, float *__restrict__ test_prev, int apply)
{
    __shared__ float w_s[kMaxLayers][W32 * W32];
    __shared__ float b_s[kMaxLayers][W32];
    __shared__ float red_s[4];
    const int tid = threadIdx.x, L = g.n_layers, m = blockIdx.y;
    const int n = g.n_train[m];
    if ((int)blockIdx.x * 256 >= n) return; // uniform, before any barrier: members differ in n_train
    if (blockIdx.x == 0 && tid == 0) {
        if (test_prev != nullptr) lb_test_sum(g, m, test_prev);
        // the optimiser step this pass belongs to: advanced HERE, two launches ahead of the Adam kernel whose workgroups all read it
        if (apply && m == 0) g.step[0] = g.step[0] + 1;
    }
    lb_stage(g.P + (size_t)m * L * kTile, L, w_s, b_s, tid);
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    const int row = g.train_idx[(size_t)m * g.cap_train + ii];
    const int nin = g.width[0], nout = g.width[L];
    float a[kMaxLayers + 1][W32];
    lb_forward(w_s, b_s, L, nin, g.X + (size_t)row * nin, a);
    // loss = mean over samples and outputs of (pred - Y)^2 (tf.reduce_mean(squared_difference), learner_base.py:474-476)
    float d[W32];
    const float scale = 2.0f / ((float)n * (float)nout);
    float se = lb_error(a, L, nout, valid, g.Y + (size_t)row * nout, scale, d);
    // backward: D_l = d ; d_{l-1}[j] = (sum_o W_l[j][o] d[o]) * [a_l[j] > 0]
    float *Am = g.A + (size_t)m * L * g.cap_train * W32, *Dm = g.D + (size_t)m * L * g.cap_train * W32;
#pragma unroll
    for (int l = kMaxLayers - 1; l >= 0; --l) {
        if (l < L) {
            if (valid) {
                float4 *Dp = reinterpret_cast<float4 *>(Dm + ((size_t)l * g.cap_train + i) * W32), *Ap = reinterpret_cast<float4 *>(Am + ((size_t)l * g.cap_train + i) * W32);
#pragma unroll
                for (int q = 0; q < W32 / 4; ++q) {
                    Dp[q] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
                    Ap[q] = make_float4(a[l][4 * q], a[l][4 * q + 1], a[l][4 * q + 2], a[l][4 * q + 3]);
                }
            }
            if (l > 0) {
                float dn[W32];
#pragma unroll
                for (int j = 0; j < W32; ++j) {
                    float acc = 0.0f;
#pragma unroll
                    for (int o = 0; o < W32; ++o) acc = __builtin_fmaf(w_s[l][j * W32 + o], d[o], acc);
                    dn[j] = a[l][j] > 0.0f ? acc : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < W32; ++j) d[j] = dn[j];
            }
        }
    }
    se = lb_block_sum(se, red_s, tid);
    if (tid == 0) g.loss_part[(size_t)m * g.blocks_max + blockIdx.x] = se;
}

// grid (chunks_max, layers, B): k_learn_grad per member and chunk — dW_l = A_l^T D_l and db_l = 1^T D_l over the chunk's samples on
// v_mfma_f32_32x32x2_f32, wave w on sample pairs s0 + 2w, +8, ...; the four waves' tiles summed in wave order.
__global__ __launch_bounds__(kGradThreads) void k_lb_grad(const LbArgs g)
{
    __shared__ float tile_s[4][kTile];
    const int chunk = blockIdx.x, l = blockIdx.y, L = gridDim.y, m = blockIdx.z;
    const int n = g.n_train[m];
    if (chunk * kChunk >= n) return; // uniform, before the barrier
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, k = lane >> 5;
    const float *Al = g.A + ((size_t)m * L + l) * g.cap_train * W32, *Dl = g.D + ((size_t)m * L + l) * g.cap_train * W32;
    const int s0 = chunk * kChunk, s1 = min(n, s0 + kChunk);
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, accb = acc;
    const float one_row0 = r == 0 ? 1.0f : 0.0f; // Aop of the bias MFMA: row 0 is all ones -> row 0 of the result = column sums of D
    for (int s = s0 + 2 * w; s < s1; s += 8) {
        const int sk = s + k;
        const float av = sk < s1 ? Al[(size_t)sk * W32 + r] : 0.0f;
        const float dv = sk < s1 ? Dl[(size_t)sk * W32 + r] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, dv, acc, 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_32x32x2f32(one_row0, dv, accb, 0, 0, 0);
    }
    // accumulator register q of lane (r, k) is element [row = 8 (q >> 2) + 4 k + (q & 3)][col = r]
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = 8 * (q >> 2) + 4 * k + (q & 3);
        tile_s[w][row * W32 + r] = acc[q];
        if (row == 0) tile_s[w][32 * W32 + r] = accb[q];
    }
    __syncthreads();
    float *out = g.part + (((size_t)m * g.chunks_max + chunk) * L + l) * kTile;
    for (int e = tid; e < kTile; e += kGradThreads) out[e] = ((tile_s[0][e] + tile_s[1][e]) + tile_s[2][e]) + tile_s[3][e];
}

// grid (layers, ceil(33 * 32 / 256), B) (apply) or (1, 1, B) (loss only): k_learn_adam per member, over the member's own chunk and
// block counts, with the member's rates hp[m] = (lr, beta1, beta2, eps). loss_out[m] = the loss of THIS step's forward pass.
__global__ __launch_bounds__(256) void k_lb_adam(const LbArgs g, const float *__restrict__ hp, float *__restrict__ loss_out, int apply)
{
    const int L = g.n_layers, l = blockIdx.x, tid = threadIdx.x, e = blockIdx.y * 256 + tid, m = blockIdx.z;
    const int n = g.n_train[m], chunks = (n + kChunk - 1) / kChunk, loss_blocks = (n + 255) / 256;
    if (apply && e < kTile) {
        const float lr = hp[4 * m], b1 = hp[4 * m + 1], b2 = hp[4 * m + 2], eps = hp[4 * m + 3];
        const int t = g.step[0]; // advanced by this step's forward pass
        const float bc1 = 1.0f - powf(b1, (float)t), bc2 = 1.0f - powf(b2, (float)t);
        const float lr_t = lr * sqrtf(bc2) / bc1;
        float gr = 0.0f;
        for (int c = 0; c < chunks; ++c) gr += g.part[(((size_t)m * g.chunks_max + c) * L + l) * kTile + e]; // fixed order: deterministic
        const int row = e / W32, col = e % W32;
        const bool is_b = row == 32;
        const bool live = col < g.width[l + 1] && (is_b || row < g.width[l]); // padding stays exactly zero
        if (live) {
            const size_t at = ((size_t)m * L + l) * kTile + e;
            const float mo = g.M[at], vo = g.V[at];
            const float mn = adam_first_moment(b1, mo, gr), vn = b2 * vo + (1.0f - b2) * gr * gr;
            g.M[at] = mn; g.V[at] = vn;
            g.P[at] = g.P[at] - lr_t * mn / (sqrtf(vn) + eps);
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        float s = 0.0f;
        for (int q = 0; q < loss_blocks; ++q) s += g.loss_part[(size_t)m * g.blocks_max + q];
        loss_out[m] = s / ((float)n * (float)g.width[L]);
    }
}

// grid (tblocks_max, B): the forward pass alone over the member's test rows; test_part[m][block] = sum of squared errors
__global__ __launch_bounds__(256) void k_lb_test(const LbArgs g)
{
    __shared__ float w_s[kMaxLayers][W32 * W32];
    __shared__ float b_s[kMaxLayers][W32];
    __shared__ float red_s[4];
    const int tid = threadIdx.x, L = g.n_layers, m = blockIdx.y;
    const int n = g.n_test[m];
    if ((int)blockIdx.x * 256 >= n) return; // uniform, before any barrier (a member without test rows runs nothing)
    lb_stage(g.P + (size_t)m * L * kTile, L, w_s, b_s, tid);
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    const bool valid = i < n;
    const int row = g.test_idx[(size_t)m * g.cap_test + (valid ? i : n - 1)];
    const int nin = g.width[0], nout = g.width[L];
    float a[kMaxLayers + 1][W32], d[W32];
    lb_forward(w_s, b_s, L, nin, g.X + (size_t)row * nin, a);
    float se = lb_error(a, L, nout, valid, g.Y + (size_t)row * nout, 0.0f, d);
    se = lb_block_sum(se, red_s, tid);
    if (tid == 0) g.test_part[(size_t)m * g.tblocks_max + blockIdx.x] = se;
}

__global__ void k_lb_test_sum(const LbArgs g, int B, float *__restrict__ out)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < B) lb_test_sum(g, m, out);
}

} // namespace

struct mppi_learner_batch {
    int device = 0, B = 0;
    hipStream_t stream = nullptr;
    LbArgs g{};
    int n = 0, data_cap = 0;
    float *dX = nullptr, *dY = nullptr;
    // the splits as the host validated them; an empty train list = the default (rows 0..n-1, no test rows)
    std::vector<std::vector<int32_t>> train, test;
    bool dirty = true; // the device copies below are stale
    int *d_train_idx = nullptr, *d_test_idx = nullptr, *d_counts = nullptr; // d_counts: [2][B] = n_train, n_test
    float *d_hp = nullptr, *d_eval = nullptr, *d_hist = nullptr;            // [B][4]; [2][B]; [2][hist_cap]
    size_t hist_cap = 0;
    int max_test = 0;
    float *d_roll = nullptr; // mppi_learner_batch_rollout's inputs, trajectories and partials: one buffer, grown on demand
    size_t roll_cap = 0;
    std::string err;
};

static thread_local std::string g_lb_err;
static mppi_status bfail(mppi_learner_batch *lb, mppi_status st, const std::string &msg)
{
    if (lb) lb->err = msg; else g_lb_err = msg;
    return st;
}
#define B_TRY(lb, expr)                                                                           \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return bfail((lb), MPPI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T> static mppi_status lb_alloc(mppi_learner_batch *lb, T **p, size_t count, const char *what)
{
    *p = nullptr;
    hipError_t e = hipMalloc((void **)p, sizeof(T) * (count ? count : 1));
    if (e == hipSuccess) return MPPI_OK;
    (void)hipGetLastError();
    *p = nullptr;
    return bfail(lb, MPPI_ERR_ALLOC, std::string("learner batch: cannot allocate ") + what + " (" + std::to_string(sizeof(T) * count) + " bytes): " + hipGetErrorString(e));
}
template <typename T> static void lb_free(T **p) { if (*p) { (void)hipFree((void *)*p); *p = nullptr; } }

static void free_split_buffers(mppi_learner_batch *lb)
{
    lb_free(&lb->d_train_idx); lb_free(&lb->d_test_idx);
    lb_free(&lb->g.A); lb_free(&lb->g.D); lb_free(&lb->g.part); lb_free(&lb->g.loss_part); lb_free(&lb->g.test_part);
    lb->dirty = true;
}

// index lists, counts and everything sized by the largest split onto the device (after set_data / set_split; the stream is idle)
static mppi_status sync_splits(mppi_learner_batch *lb)
{
    if (!lb->dirty) return MPPI_OK;
    free_split_buffers(lb);
    const int B = lb->B, L = lb->g.n_layers;
    int cap = 1, tcap = 0;
    for (int m = 0; m < B; ++m) {
        cap = std::max(cap, lb->train[m].empty() ? lb->n : (int)lb->train[m].size());
        tcap = std::max(tcap, (int)lb->test[m].size());
    }
    const int chunks = (cap + kChunk - 1) / kChunk, blocks = (cap + 255) / 256, tblocks = (tcap + 255) / 256;
    std::vector<int32_t> idx((size_t)B * cap, 0), tidx((size_t)B * std::max(tcap, 1), 0), counts(2 * (size_t)B);
    for (int m = 0; m < B; ++m) {
        int32_t *row = idx.data() + (size_t)m * cap;
        if (lb->train[m].empty()) { for (int i = 0; i < lb->n; ++i) row[i] = i; counts[m] = lb->n; }
        else { memcpy(row, lb->train[m].data(), sizeof(int32_t) * lb->train[m].size()); counts[m] = (int32_t)lb->train[m].size(); }
        if (!lb->test[m].empty()) memcpy(tidx.data() + (size_t)m * tcap, lb->test[m].data(), sizeof(int32_t) * lb->test[m].size());
        counts[B + m] = (int32_t)lb->test[m].size();
    }
    auto body = [&]() -> mppi_status {
        mppi_status s;
        if ((s = lb_alloc(lb, &lb->d_train_idx, idx.size(), "the train index lists")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->d_test_idx, tidx.size(), "the test index lists")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.A, (size_t)B * L * cap * W32, "the activations [B][layers][max n_train][32]")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.D, (size_t)B * L * cap * W32, "the deltas [B][layers][max n_train][32]")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.part, (size_t)B * chunks * L * kTile, "the partial gradient tiles")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.loss_part, (size_t)B * blocks, "the loss partials")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.test_part, (size_t)B * std::max(tblocks, 1), "the test loss partials")) != MPPI_OK) return s;
        B_TRY(lb, hipMemcpy(lb->d_train_idx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice));
        B_TRY(lb, hipMemcpy(lb->d_test_idx, tidx.data(), sizeof(int32_t) * tidx.size(), hipMemcpyHostToDevice));
        B_TRY(lb, hipMemcpy(lb->d_counts, counts.data(), sizeof(int32_t) * counts.size(), hipMemcpyHostToDevice));
        return MPPI_OK;
    };
    mppi_status s = body();
    if (s != MPPI_OK) { free_split_buffers(lb); return s; }
    lb->g.train_idx = lb->d_train_idx; lb->g.test_idx = lb->d_test_idx;
    lb->g.n_train = lb->d_counts; lb->g.n_test = lb->d_counts + B;
    lb->g.cap_train = cap; lb->g.cap_test = std::max(tcap, 1);
    lb->g.chunks_max = chunks; lb->g.blocks_max = blocks; lb->g.tblocks_max = std::max(tblocks, 1);
    lb->g.X = lb->dX; lb->g.Y = lb->dY;
    lb->max_test = tcap;
    lb->dirty = false;
    return MPPI_OK;
}

extern "C" const char *mppi_learner_batch_last_error(const mppi_learner_batch *lb) { return lb ? lb->err.c_str() : g_lb_err.c_str(); }

extern "C" int mppi_learner_batch_size(const mppi_learner_batch *lb) { return lb ? lb->B : 0; }

extern "C" void mppi_learner_batch_destroy(mppi_learner_batch *lb)
{
    if (!lb) return;
    (void)hipSetDevice(lb->device);
    if (lb->stream) (void)hipStreamSynchronize(lb->stream);
    free_split_buffers(lb);
    lb_free(&lb->g.P); lb_free(&lb->g.M); lb_free(&lb->g.V); lb_free(&lb->g.step);
    lb_free(&lb->dX); lb_free(&lb->dY); lb_free(&lb->d_counts); lb_free(&lb->d_hp); lb_free(&lb->d_eval); lb_free(&lb->d_hist); lb_free(&lb->d_roll);
    if (lb->stream) (void)hipStreamDestroy(lb->stream);
    delete lb;
}

extern "C" mppi_status mppi_learner_batch_set_weights(mppi_learner_batch *lb, int member, const float *const *W, const float *const *b)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    if (!W || !b) return bfail(lb, MPPI_ERR_INVALID_ARG, "NULL weights");
    if (member < -1 || member >= lb->B) return bfail(lb, MPPI_ERR_INVALID_ARG, "member out of range (-1: every member)");
    const int L = lb->g.n_layers;
    for (int k = 0; k < L; ++k) if (!W[k] || !b[k]) return bfail(lb, MPPI_ERR_INVALID_ARG, "NULL weights");
    const size_t per = (size_t)L * kTile;
    const int copies = member < 0 ? lb->B : 1;
    std::vector<float> img(per * copies, 0.0f); // the padding is written as zero
    for (int k = 0; k < L; ++k) {
        const int in = lb->g.width[k], out = lb->g.width[k + 1];
        float *t = img.data() + (size_t)k * kTile;
        for (int i = 0; i < in; ++i) for (int o = 0; o < out; ++o) t[i * W32 + o] = W[k][(size_t)i * out + o];
        for (int o = 0; o < out; ++o) t[32 * W32 + o] = b[k][o];
    }
    for (int c = 1; c < copies; ++c) memcpy(img.data() + per * c, img.data(), sizeof(float) * per);
    B_TRY(lb, hipSetDevice(lb->device));
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    B_TRY(lb, hipMemcpy(lb->g.P + per * (member < 0 ? 0 : member), img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice));
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_get_weights(mppi_learner_batch *lb, int member, float *const *W, float *const *b)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    if (!W || !b) return bfail(lb, MPPI_ERR_INVALID_ARG, "NULL output");
    if (member < 0 || member >= lb->B) return bfail(lb, MPPI_ERR_INVALID_ARG, "member out of range");
    const int L = lb->g.n_layers;
    const size_t per = (size_t)L * kTile;
    std::vector<float> img(per);
    B_TRY(lb, hipSetDevice(lb->device));
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    B_TRY(lb, hipMemcpy(img.data(), lb->g.P + per * member, sizeof(float) * per, hipMemcpyDeviceToHost));
    for (int k = 0; k < L; ++k) {
        const int in = lb->g.width[k], out = lb->g.width[k + 1];
        const float *t = img.data() + (size_t)k * kTile;
        if (W[k]) for (int i = 0; i < in; ++i) for (int o = 0; o < out; ++o) W[k][(size_t)i * out + o] = t[i * W32 + o];
        if (b[k]) for (int o = 0; o < out; ++o) b[k][o] = t[32 * W32 + o];
    }
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_reset_optimizer(mppi_learner_batch *lb)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    const size_t all = (size_t)lb->B * lb->g.n_layers * kTile;
    B_TRY(lb, hipSetDevice(lb->device));
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    B_TRY(lb, hipMemset(lb->g.M, 0, sizeof(float) * all));
    B_TRY(lb, hipMemset(lb->g.V, 0, sizeof(float) * all));
    B_TRY(lb, hipMemset(lb->g.step, 0, sizeof(int)));
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_get_step(mppi_learner_batch *lb, int *step)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    if (!step) return bfail(lb, MPPI_ERR_INVALID_ARG, "NULL output");
    B_TRY(lb, hipSetDevice(lb->device));
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    B_TRY(lb, hipMemcpy(step, lb->g.step, sizeof(int), hipMemcpyDeviceToHost));
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_create(int n_members, int n_layers, const int32_t *widths, const float *const *W, const float *const *b,
                                                 int device, mppi_learner_batch **out)
{
    if (!out || !widths || !W || !b) return bfail(nullptr, MPPI_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    // the shape first, before the device is touched: what mppi_learner_create refuses, and the wide network it accepts
    if (n_layers < 1 || n_layers > kMaxLayers) return bfail(nullptr, MPPI_ERR_UNSUPPORTED, "learner batch: 1 to 4 Dense layers");
    for (int k = 0; k <= n_layers; ++k)
        if (widths[k] < 1 || widths[k] > W32) return bfail(nullptr, MPPI_ERR_UNSUPPORTED, "learner batch: layer widths 1..32 (the [in, 256, 256, out] learner is not batched)");
    if (n_members < 1 || n_members > kMaxMembers) return bfail(nullptr, MPPI_ERR_INVALID_ARG, "learner batch: 1 to 1024 members");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return bfail(nullptr, MPPI_ERR_NO_DEVICE, "no HIP device visible: the learner has no CPU path"); }
    if (device < 0 || device >= ndev) return bfail(nullptr, MPPI_ERR_NO_DEVICE, "device ordinal out of range");
    mppi_learner_batch *lb = new (std::nothrow) mppi_learner_batch();
    if (!lb) return bfail(nullptr, MPPI_ERR_ALLOC, "out of host memory");
    lb->device = device;
    lb->B = n_members;
    lb->g.n_layers = n_layers;
    for (int k = 0; k <= n_layers; ++k) lb->g.width[k] = widths[k];
    lb->train.resize(n_members);
    lb->test.resize(n_members);
    auto body = [&]() -> mppi_status {
        B_TRY(lb, hipSetDevice(device));
        B_TRY(lb, hipStreamCreateWithFlags(&lb->stream, hipStreamNonBlocking));
        const size_t all = (size_t)n_members * n_layers * kTile;
        mppi_status s;
        if ((s = lb_alloc(lb, &lb->g.P, all, "the weights")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.M, all, "the first Adam moments")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.V, all, "the second Adam moments")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->g.step, 1, "the step counter")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->d_counts, 2 * (size_t)n_members, "the split sizes")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->d_hp, 4 * (size_t)n_members, "the rates")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->d_eval, 2 * (size_t)n_members, "the losses")) != MPPI_OK) return s;
        if ((s = mppi_learner_batch_set_weights(lb, -1, W, b)) != MPPI_OK) return s;
        return mppi_learner_batch_reset_optimizer(lb);
    };
    mppi_status s = body();
    if (s != MPPI_OK) { g_lb_err = lb->err; mppi_learner_batch_destroy(lb); return s; }
    *out = lb;
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_set_data(mppi_learner_batch *lb, const float *X, const float *Y, int n)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    if (!X || !Y || n <= 0) return bfail(lb, MPPI_ERR_INVALID_ARG, "X is [n, in], Y is [n, out], n > 0");
    B_TRY(lb, hipSetDevice(lb->device));
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    const int nin = lb->g.width[0], nout = lb->g.width[lb->g.n_layers];
    if (n > lb->data_cap) {
        lb_free(&lb->dX); lb_free(&lb->dY);
        lb->n = 0; lb->data_cap = 0;
        mppi_status s;
        if ((s = lb_alloc(lb, &lb->dX, (size_t)n * nin, "X")) != MPPI_OK) return s;
        if ((s = lb_alloc(lb, &lb->dY, (size_t)n * nout, "Y")) != MPPI_OK) { lb_free(&lb->dX); return s; }
        lb->data_cap = n;
    }
    B_TRY(lb, hipMemcpy(lb->dX, X, sizeof(float) * (size_t)n * nin, hipMemcpyHostToDevice));
    B_TRY(lb, hipMemcpy(lb->dY, Y, sizeof(float) * (size_t)n * nout, hipMemcpyHostToDevice));
    lb->n = n;
    for (int m = 0; m < lb->B; ++m) { lb->train[m].clear(); lb->test[m].clear(); } // a new pool: every split back to rows 0..n-1, no test rows
    lb->dirty = true;
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_set_split(mppi_learner_batch *lb, int member, const int32_t *train_idx, int n_train,
                                                    const int32_t *test_idx, int n_test)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    if (lb->n <= 0) return bfail(lb, MPPI_ERR_INVALID_ARG, "no data: call mppi_learner_batch_set_data first");
    if (member < 0 || member >= lb->B) return bfail(lb, MPPI_ERR_INVALID_ARG, "member out of range");
    if (!train_idx || n_train < 1 || n_test < 0 || (n_test > 0 && !test_idx)) return bfail(lb, MPPI_ERR_INVALID_ARG, "n_train >= 1 train rows, n_test >= 0 test rows");
    // every index is checked HERE: the kernels read X[idx] unguarded
    for (int i = 0; i < n_train; ++i)
        if (train_idx[i] < 0 || train_idx[i] >= lb->n) return bfail(lb, MPPI_ERR_INVALID_ARG, "train_idx[" + std::to_string(i) + "] = " + std::to_string(train_idx[i]) + " is outside [0, " + std::to_string(lb->n) + ")");
    for (int i = 0; i < n_test; ++i)
        if (test_idx[i] < 0 || test_idx[i] >= lb->n) return bfail(lb, MPPI_ERR_INVALID_ARG, "test_idx[" + std::to_string(i) + "] = " + std::to_string(test_idx[i]) + " is outside [0, " + std::to_string(lb->n) + ")");
    lb->train[member].assign(train_idx, train_idx + n_train);
    lb->test[member].assign(test_idx, test_idx + n_test);
    lb->dirty = true;
    return MPPI_OK;
}

// forward + backward + gradient + Adam of every member [+ the held-out forward pass] onto the stream
static mppi_status enqueue_step(mppi_learner_batch *lb, float *loss_train_row, float *test_prev_row, bool test)
{
    const LbArgs &g = lb->g;
    const int L = g.n_layers, B = lb->B;
    hipLaunchKernelGGL(k_lb_fwd_bwd, dim3(g.blocks_max, B), dim3(256), 0, lb->stream, g, test_prev_row, 1);
    B_TRY(lb, hipGetLastError());
    hipLaunchKernelGGL(k_lb_grad, dim3(g.chunks_max, L, B), dim3(kGradThreads), 0, lb->stream, g);
    B_TRY(lb, hipGetLastError());
    hipLaunchKernelGGL(k_lb_adam, dim3(L, (kTile + 255) / 256, B), dim3(256), 0, lb->stream, g, (const float *)lb->d_hp, loss_train_row, 1);
    B_TRY(lb, hipGetLastError());
    if (test) {
        hipLaunchKernelGGL(k_lb_test, dim3(g.tblocks_max, B), dim3(256), 0, lb->stream, g);
        B_TRY(lb, hipGetLastError());
    }
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_train(mppi_learner_batch *lb, int steps, const float *lr, const float *beta1, const float *beta2,
                                                const float *eps, float *loss_train, float *loss_test)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    if (lb->n <= 0) return bfail(lb, MPPI_ERR_INVALID_ARG, "no data: call mppi_learner_batch_set_data first");
    const int B = lb->B;
    if (steps <= 0 || !lr || (size_t)steps * B > ((size_t)1 << 28)) return bfail(lb, MPPI_ERR_INVALID_ARG, "steps > 0 (steps * members <= 2^28), lr is [members]");
    std::vector<float> hp(4 * (size_t)B);
    for (int m = 0; m < B; ++m) {
        const float l = lr[m], b1 = beta1 ? beta1[m] : 0.9f, b2 = beta2 ? beta2[m] : 0.999f, e = eps ? eps[m] : 1e-7f;
        if (!(l > 0.0f) || !(b1 >= 0.0f && b1 < 1.0f) || !(b2 >= 0.0f && b2 < 1.0f) || !(e >= 0.0f))
            return bfail(lb, MPPI_ERR_INVALID_ARG, "member " + std::to_string(m) + ": lr > 0, 0 <= beta < 1, eps >= 0");
        hp[4 * m] = l; hp[4 * m + 1] = b1; hp[4 * m + 2] = b2; hp[4 * m + 3] = e;
    }
    B_TRY(lb, hipSetDevice(lb->device));
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    mppi_status st = sync_splits(lb);
    if (st != MPPI_OK) return st;
    const size_t cells = (size_t)steps * B;
    if (cells > lb->hist_cap) {
        lb_free(&lb->d_hist); lb->hist_cap = 0;
        if ((st = lb_alloc(lb, &lb->d_hist, 2 * cells, "the loss histories")) != MPPI_OK) return st;
        lb->hist_cap = cells;
    }
    float *h_train = lb->d_hist, *h_test = lb->d_hist + lb->hist_cap;
    const bool test = loss_test != nullptr && lb->max_test > 0;
    B_TRY(lb, hipMemcpy(lb->d_hp, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice));
    for (int s = 0; s < steps; ++s) {
        st = enqueue_step(lb, h_train + (size_t)s * B, test && s > 0 ? h_test + (size_t)(s - 1) * B : nullptr, test);
        if (st != MPPI_OK) { (void)hipStreamSynchronize(lb->stream); return st; }
    }
    if (test) {
        hipLaunchKernelGGL(k_lb_test_sum, dim3((B + 255) / 256), dim3(256), 0, lb->stream, lb->g, B, h_test + (size_t)(steps - 1) * B);
        B_TRY(lb, hipGetLastError());
    }
    // the histories were written on the device: one synchronisation, then the copies
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    if (loss_train) B_TRY(lb, hipMemcpy(loss_train, h_train, sizeof(float) * cells, hipMemcpyDeviceToHost));
    if (test) B_TRY(lb, hipMemcpy(loss_test, h_test, sizeof(float) * cells, hipMemcpyDeviceToHost));
    else if (loss_test) for (size_t i = 0; i < cells; ++i) loss_test[i] = std::numeric_limits<float>::quiet_NaN(); // no member has test rows
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_batch_evaluate(mppi_learner_batch *lb, float *loss_train, float *loss_test)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    if (lb->n <= 0) return bfail(lb, MPPI_ERR_INVALID_ARG, "no data: call mppi_learner_batch_set_data first");
    B_TRY(lb, hipSetDevice(lb->device));
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    mppi_status st = sync_splits(lb);
    if (st != MPPI_OK) return st;
    const LbArgs &g = lb->g;
    const int B = lb->B;
    const bool test = loss_test != nullptr && lb->max_test > 0;
    // the forward pass of a step without its update (the backward half's stores go to buffers the next step rewrites)
    hipLaunchKernelGGL(k_lb_fwd_bwd, dim3(g.blocks_max, B), dim3(256), 0, lb->stream, g, (float *)nullptr, 0);
    B_TRY(lb, hipGetLastError());
    hipLaunchKernelGGL(k_lb_adam, dim3(1, 1, B), dim3(256), 0, lb->stream, g, (const float *)lb->d_hp, lb->d_eval, 0);
    B_TRY(lb, hipGetLastError());
    if (test) {
        hipLaunchKernelGGL(k_lb_test, dim3(g.tblocks_max, B), dim3(256), 0, lb->stream, g);
        B_TRY(lb, hipGetLastError());
        hipLaunchKernelGGL(k_lb_test_sum, dim3((B + 255) / 256), dim3(256), 0, lb->stream, g, B, lb->d_eval + B);
        B_TRY(lb, hipGetLastError());
    }
    B_TRY(lb, hipStreamSynchronize(lb->stream));
    if (loss_train) B_TRY(lb, hipMemcpy(loss_train, lb->d_eval, sizeof(float) * B, hipMemcpyDeviceToHost));
    if (test) B_TRY(lb, hipMemcpy(loss_test, lb->d_eval + B, sizeof(float) * B, hipMemcpyDeviceToHost));
    else if (loss_test) for (int m = 0; m < B; ++m) loss_test[m] = std::numeric_limits<float>::quiet_NaN();
    return MPPI_OK;
}

// ---- trajectory validation: every member's network rolled open-loop in one launch (k_lb_rollout, mppi_learner_rollout.hip)
namespace {

// the network's first and last width the model kind asks for; 0: not one of the three kinds, -1: s_dim / a_dim do not fit the kind
int roll_widths(const mppi_learner_model *mo, int *nin, int *nout)
{
    switch (mo->model_kind) {
    case MPPI_MODEL_MLP:
        if (mo->a_dim < 1 || mo->a_dim > 4 || mo->s_dim != 2 * mo->a_dim) return -1;
        *nin = mo->s_dim + mo->a_dim; *nout = mo->s_dim;
        return 1;
    case MPPI_MODEL_NN_AUV:
    case MPPI_MODEL_NN_AUV_SPEED:
        if (mo->s_dim != 13 || mo->a_dim != 6) return -1;
        *nin = mo->model_kind == MPPI_MODEL_NN_AUV ? 16 : 15; *nout = mo->model_kind == MPPI_MODEL_NN_AUV ? 13 : 6;
        return 1;
    default:
        return 0;
    }
}

} // namespace

extern "C" mppi_status mppi_learner_batch_rollout(mppi_learner_batch *lb, const mppi_learner_model *model, const float *x0, int kx, const float *V,
                                                  const float *G, int n, int T, double *sse_out, float *X_out)
{
    if (!lb) return MPPI_ERR_INVALID_ARG;
    const std::string who = "mppi_learner_batch_rollout: ";
    // every refusal before the device is touched
    if (!model || !x0 || !V) return bfail(lb, MPPI_ERR_INVALID_ARG, who + "model, x0 [kx, s_dim] and V [T, n, a_dim] are required: NULL pointer");
    if (!sse_out && !X_out) return bfail(lb, MPPI_ERR_INVALID_ARG, who + "sse_out and X_out are both NULL");
    if (sse_out && !G) return bfail(lb, MPPI_ERR_INVALID_ARG, who + "sse_out needs the ground truth G [T+1, n, s_dim]");
    if (n < 1 || T < 1) return bfail(lb, MPPI_ERR_INVALID_ARG, who + "n and T must be >= 1");
    if ((size_t)n * (size_t)T > ((size_t)1 << 30)) return bfail(lb, MPPI_ERR_INVALID_ARG, who + "n * T must not exceed 2^30");
    if (kx != 1 && kx != n) return bfail(lb, MPPI_ERR_INVALID_ARG, who + "x0 is [kx, s_dim] with kx in {1, n}");
    int nin = 0, nout = 0;
    const int fit = roll_widths(model, &nin, &nout);
    if (fit == 0) return bfail(lb, MPPI_ERR_UNSUPPORTED, who + "model_kind must be MPPI_MODEL_MLP, MPPI_MODEL_NN_AUV or MPPI_MODEL_NN_AUV_SPEED");
    const int L = lb->g.n_layers, B = lb->B;
    if (fit < 0 || lb->g.width[0] != nin || lb->g.width[L] != nout)
        return bfail(lb, MPPI_ERR_UNSUPPORTED, who + "the batch's network is [" + std::to_string(lb->g.width[0]) + " -> " + std::to_string(lb->g.width[L]) +
            "]: MPPI_MODEL_MLP takes s_dim + a_dim -> s_dim with s_dim = 2 a_dim, a_dim <= 4; MPPI_MODEL_NN_AUV 16 -> 13 and MPPI_MODEL_NN_AUV_SPEED "
            "15 -> 6, both with s_dim = 13, a_dim = 6");
    LbRollout r{};
    for (int j = 0; j < kRollMaxIn; ++j) { r.xmean[j] = 0.0f; r.xstd[j] = 1.0f; }
    for (int j = 0; j < kRollMaxOut; ++j) { r.ymean[j] = 0.0f; r.ystd[j] = 1.0f; }
    for (int j = 0; j < nin; ++j) {
        if (model->xmean) r.xmean[j] = model->xmean[j];
        if (model->xstd) r.xstd[j] = model->xstd[j];
        if (r.xstd[j] == 0.0f) return bfail(lb, MPPI_ERR_INVALID_ARG, who + "xstd[" + std::to_string(j) + "] is 0: the inputs are divided by it");
    }
    for (int j = 0; j < nout; ++j) {
        if (model->ymean) r.ymean[j] = model->ymean[j];
        if (model->ystd) r.ystd[j] = model->ystd[j];
    }
    const size_t s = (size_t)model->s_dim, a = (size_t)model->a_dim, rows = (size_t)n * (size_t)T, blocks = ((size_t)n + kRollThreads - 1) / kRollThreads;
    r.P = lb->g.P; r.n_layers = L;
    for (int k = 0; k <= L; ++k) r.width[k] = lb->g.width[k];
    r.kind = model->model_kind; r.s = model->s_dim; r.a = model->a_dim; r.dt = model->dt;
    r.kx = kx; r.n = n; r.T = T; r.blocks = (int)blocks;
    B_TRY(lb, hipSetDevice(lb->device));
    // one buffer on the batch, carved into x0, V, G, the partials and X (each part a multiple of 64 floats: 256-byte starts)
    const auto pad = [](size_t c) { return (c + 63) & ~(size_t)63; };
    const size_t c_x = pad((size_t)kx * s), c_V = pad(rows * a), c_G = G ? pad((rows + n) * s) : 0, c_part = G ? pad((size_t)B * blocks * s) : 0,
                 c_X = X_out ? pad((size_t)B * (rows + n) * s) : 0, total = c_x + c_V + c_G + c_part + c_X;
    if (total > lb->roll_cap) {
        B_TRY(lb, hipStreamSynchronize(lb->stream));
        lb_free(&lb->d_roll); lb->roll_cap = 0;
        if (mppi_status st = lb_alloc(lb, &lb->d_roll, total, "the trajectories [B][T+1][n][s_dim] and their inputs"); st != MPPI_OK) return st;
        lb->roll_cap = total;
    }
    float *dx = lb->d_roll, *dV = dx + c_x, *dG = G ? dV + c_V : nullptr, *dpart = G ? dV + c_V + c_G : nullptr, *dX = X_out ? dV + c_V + c_G + c_part : nullptr;
    hipStream_t q = lb->stream;
    B_TRY(lb, hipMemcpyAsync(dx, x0, sizeof(float) * (size_t)kx * s, hipMemcpyHostToDevice, q));
    B_TRY(lb, hipMemcpyAsync(dV, V, sizeof(float) * rows * a, hipMemcpyHostToDevice, q));
    if (G) B_TRY(lb, hipMemcpyAsync(dG, G, sizeof(float) * (rows + n) * s, hipMemcpyHostToDevice, q));
    r.x0 = dx; r.V = dV; r.G = dG; r.X = dX; r.part = dpart;
    if (hipError_t e = mppi_lrn_launch_rollout(r, B, q); e != hipSuccess) {
        (void)hipStreamSynchronize(q);
        return bfail(lb, MPPI_ERR_HIP, who + hipGetErrorString(e));
    }
    std::vector<float> part(sse_out ? (size_t)B * blocks * s : 0);
    if (sse_out) B_TRY(lb, hipMemcpyAsync(part.data(), dpart, sizeof(float) * part.size(), hipMemcpyDeviceToHost, q));
    if (X_out) B_TRY(lb, hipMemcpyAsync(X_out, dX, sizeof(float) * (size_t)B * (rows + n) * s, hipMemcpyDeviceToHost, q));
    B_TRY(lb, hipStreamSynchronize(q));
    if (sse_out) // the blocks of a member in block order, in fp64
        for (int m = 0; m < B; ++m)
            for (size_t j = 0; j < s; ++j) {
                double acc = 0.0;
                for (size_t b = 0; b < blocks; ++b) acc += (double)part[((size_t)m * blocks + b) * s + j];
                sse_out[(size_t)m * s + j] = acc;
            }
    return MPPI_OK;
}
