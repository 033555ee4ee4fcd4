// mppi_learner_wide_batch.hip — B wide learners ([in, 256, 256, out], mppi_learner_wide.hip) in the launches of one: what
// mppi_learner_batch.hip is to the narrow learner (LearnerBase.k_fold_validation / grid_search, learner_base.py:83-216, for the network a
// MPPI_MODEL_MLP controller rolls out). Every member is bit-identical to a lone wide mppi_learner given the member's rows. k_wb_gemm is a
// COPY of k_wide_gemm's tile body and k_wb_adam of k_wide_adam's element body: 64 x 64 tile of C per workgroup, four waves with one
// 32 x 32 accumulator each on v_mfma_f32_32x32x2_f32, k in 32-wide slabs through LDS in ascending order, gradient chunks of 512 samples BY
// POSITION in the member's index list summed in ascending order by the Adam kernel, loss partials per 64-row block summed in block order,
// adam_first_moment. What differs is addressing only:
//   * a member axis in every grid: blockIdx.z of the forward / backward GEMMs (M tiles, N tiles, B); folded into blockIdx.z of the
//     gradient GEMM (chunks, N tiles, M tiles x B); blockIdx.y of Adam
//   * weights and both moments [B][kWideParams], partial tiles [B][chunks_max][kWideParams], activations and deltas [B][rows_max][256 | 32],
//     loss partials [B][blocks_max]: every operand pointer moves by member x its stride
//   * the member's rows are gathered ONCE, when the splits go to the device (k_wb_gather): X [B][max n_train][32] (padded as the lone
//     learner pads) and Y [B][max n_train][out], the same for the test rows. The GEMMs then read a member's rows as the lone learner
//     reads its data; nothing is gathered on the fly.
//   * members differ in n_train: the grids are sized by the largest, a workgroup past its member's range returns before any barrier
//   * per-member lr, beta1, beta2, eps from a device array; the loss scale 2 / (n out) per member, formed on the host as the lone
//     learner forms it; one step counter for the batch (advanced by member 0's first loss workgroup)
// The held-out loss is the forward pass alone (three GEMMs, the loss epilogue at apply = 0) over each member's test rows with the weights
// Adam just wrote, in the activation buffers the step is done with; its 64-row partials are summed in block order by the next step's
// first launch (workgroup (0, 0) of the member) and, for the last step of a call, by one k_wb_mean.
// Launches per Adam step: 9 (8 GEMMs + Adam), or 12 when test losses are asked for and some member has test rows. No float atomics.
// Trajectory validation (mppi_learner_wide_batch_validate, at the end) reads P alone and rolls every member in ONE launch of k_wb_rollout,
// which lives in mppi_learner_wide_rollout.hip: plain-order vector-ALU arithmetic, not the tiles above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "mppi_learner.hip.h"

using namespace mppi_lrn;

namespace {

constexpr int kH = kWideHidden;
constexpr int kWideChunk = 512;  // mppi_learner_wide.hip's: the chunk boundaries are part of the gradient sum's order
constexpr int kTile = 64;
constexpr int kSlab = 32;
constexpr int kLd = kTile + 1;
constexpr int kMaxMembers = 1024;
typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { EPI_BIAS_RELU = 0, EPI_LOSS = 1, EPI_MASK = 2, EPI_PART = 3 };

struct WbGemm { // k_wide_gemm's GemmArgs with a stride per member behind every pointer
    const float *A, *B;
    size_t sA, sB;
    int lda, ldb;
    const int *count;   // [B]: the member's rows (M; EPI_PART: K)
    int M, N, K;        // EPI_PART: M, N; otherwise N, K
    float *C;
    size_t sC;
    int ldc;
    const float *bias;  // member stride kWideParams
    const float *aux;   // EPI_LOSS: Y [rows][nout] ; EPI_MASK: the activation [rows][ldc]
    size_t sAux;
    int nout;           // EPI_LOSS
    const float *scale; // EPI_LOSS: [B], 2 / (n nout)
    float *loss_part;   // EPI_LOSS: [B][loss_stride]
    int loss_stride;
    int *step;          // EPI_LOSS
    int apply;          // EPI_LOSS
    int db_row;         // EPI_PART
    int mtiles;         // EPI_PART: blockIdx.z = member * mtiles + M tile
    // EPI_BIAS_RELU, the step's first launch: where workgroup (0, 0) of each member leaves the previous step's held-out loss (or NULL)
    float *test_prev;
    const float *test_part;
    const int *n_test;
    int test_stride;
};

// the mean squared error from a member's 64-row partials: block order, then the mean. No rows: NaN, never a perfect 0.
__device__ __forceinline__ float wb_mean(const float *__restrict__ part, int n, int nout)
{
    if (n == 0) return __builtin_nanf("");
    float s = 0.0f;
    for (int q = 0; q < (n + kTile - 1) / kTile; ++q) s += part[q];
    return s / ((float)n * (float)nout);
}

template <bool KC>
__device__ __forceinline__ void load_tile(const float *__restrict__ P, int ld, int mn0, int MN, int k0, int kend, float (&v)[8], int tid)
{
    if (KC) {
        const int k = k0 + (tid & 31);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int mn = mn0 + (tid >> 5) + 8 * j;
            v[j] = (mn < MN && k < kend) ? P[(size_t)mn * ld + k] : 0.0f;
        }
    } else {
        const int mn = mn0 + (tid & 63);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + (tid >> 6) + 4 * j;
            v[j] = (mn < MN && k < kend) ? P[(size_t)k * ld + mn] : 0.0f;
        }
    }
}

template <bool KC>
__device__ __forceinline__ void store_tile(float *S, const float (&v)[8], int tid)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (KC) S[(tid & 31) * kLd + (tid >> 5) + 8 * j] = v[j];
        else S[((tid >> 6) + 4 * j) * kLd + (tid & 63)] = v[j];
    }
}

// grid: EPI_PART (chunks_max, N tiles, M tiles x B), otherwise (M tiles of the largest member, N tiles, B)
template <bool A_KC, bool B_KC, int EPI>
__global__ __launch_bounds__(256) void k_wb_gemm(const WbGemm g)
{
    __shared__ float As[kSlab * kLd], Bs[kSlab * kLd];
    __shared__ float red_s[4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, kh = lane >> 5;
    const int wm = w >> 1, wn = w & 1;
    const int member = EPI == EPI_PART ? (int)blockIdx.z / g.mtiles : (int)blockIdx.z;
    const int cnt = g.count[member];
    const int chunk = EPI == EPI_PART ? (int)blockIdx.x : 0;
    const int m0 = (EPI == EPI_PART ? (int)blockIdx.z % g.mtiles : (int)blockIdx.x) * kTile, n0 = (int)blockIdx.y * kTile;
    if (EPI == EPI_PART ? chunk * kWideChunk >= cnt : m0 >= cnt) return; // uniform, before any barrier: members differ in their row counts
    const int M = EPI == EPI_PART ? g.M : cnt, N = g.N, K = EPI == EPI_PART ? cnt : g.K;
    const float *__restrict__ A = g.A + (size_t)member * g.sA, *__restrict__ B = g.B + (size_t)member * g.sB;
    float *__restrict__ C = g.C + (size_t)member * g.sC;
    if (EPI == EPI_BIAS_RELU && g.test_prev != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0)
        g.test_prev[member] = wb_mean(g.test_part + (size_t)member * g.test_stride, g.n_test[member], g.nout);
    const int kbeg = EPI == EPI_PART ? chunk * kWideChunk : 0;
    const int kend = EPI == EPI_PART ? (K - kbeg < kWideChunk ? K : kbeg + kWideChunk) : K;
    const bool live = m0 + wm * 32 < M && n0 + wn * 32 < N;
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float db = 0.0f;
    float va[8], vb[8];
    load_tile<A_KC>(A, g.lda, m0, M, kbeg, kend, va, tid);
    load_tile<B_KC>(B, g.ldb, n0, N, kbeg, kend, vb, tid);
    for (int k0 = kbeg; k0 < kend; k0 += kSlab) {
        __syncthreads(); // the previous slab has been read
        store_tile<A_KC>(As, va, tid);
        store_tile<B_KC>(Bs, vb, tid);
        __syncthreads();
        if (k0 + kSlab < kend) {
            load_tile<A_KC>(A, g.lda, m0, M, k0 + kSlab, kend, va, tid);
            load_tile<B_KC>(B, g.ldb, n0, N, k0 + kSlab, kend, vb, tid);
        }
        if (live) {
#pragma unroll
            for (int kk = 0; kk < kSlab; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + kh) * kLd + wm * 32 + r], Bs[(kk + kh) * kLd + wn * 32 + r], acc, 0, 0, 0);
        }
        if (EPI == EPI_PART && m0 == 0 && tid < kTile) { // the bias gradient: column sums of the delta, slab by slab in sample order
            float s = 0.0f;
#pragma unroll
            for (int kk = 0; kk < kSlab; ++kk) s += Bs[kk * kLd + tid];
            db += s;
        }
    }
    float se = 0.0f;
    if (live) {
        const int n = n0 + wn * 32 + r; // < N: N is a multiple of 32 and the wave is live
        const float *__restrict__ bias = (EPI == EPI_BIAS_RELU || EPI == EPI_LOSS) ? g.bias + (size_t)member * kWideParams : nullptr;
        const float *__restrict__ aux = (EPI == EPI_LOSS || EPI == EPI_MASK) ? g.aux + (size_t)member * g.sAux : nullptr;
        const float scale = EPI == EPI_LOSS ? g.scale[member] : 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = m0 + wm * 32 + 8 * (q >> 2) + 4 * kh + (q & 3);
            if (m >= M) continue;
            if (EPI == EPI_BIAS_RELU) {
                const float z = acc[q] + bias[n];
                C[(size_t)m * g.ldc + n] = z < 0.0f ? 0.0f : z;
            } else if (EPI == EPI_MASK) {
                C[(size_t)m * g.ldc + n] = aux[(size_t)m * g.ldc + n] > 0.0f ? acc[q] : 0.0f;
            } else if (EPI == EPI_LOSS) {
                const float p = acc[q] + bias[n];
                const float e = n < g.nout ? p - aux[(size_t)m * g.nout + n] : 0.0f;
                se += e * e;
                C[(size_t)m * g.ldc + n] = scale * e; // the padded columns of the delta are written as zero
            } else {
                C[(size_t)chunk * kWideParams + (size_t)m * g.ldc + n] = acc[q];
            }
        }
    }
    if (EPI == EPI_PART && m0 == 0 && tid < kTile && n0 + tid < N)
        C[(size_t)chunk * kWideParams + (size_t)g.db_row * g.ldc + n0 + tid] = db;
    if (EPI == EPI_LOSS) { // block sum of the squared errors, fixed order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
        if (lane == 0) red_s[w] = se;
        __syncthreads();
        if (tid == 0) g.loss_part[(size_t)member * g.loss_stride + blockIdx.x] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        // the optimiser step this pass belongs to: advanced HERE, launches ahead of the Adam kernel whose workgroups all read it
        if (g.apply && member == 0 && blockIdx.x == 0 && tid == 0) g.step[0] = g.step[0] + 1;
    }
}

// grid (ceil(kWideParams / 256), B): k_wide_adam per member, over the member's own chunk and block counts, with the member's rates
// hp[m] = (lr, beta1, beta2, eps). loss_out[m] = the loss of THIS step's forward pass.
__global__ __launch_bounds__(256) void k_wb_adam(float *__restrict__ P, float *__restrict__ Mo, float *__restrict__ Vo, const float *__restrict__ part,
                                                 int chunks_max, const float *__restrict__ loss_part, int blocks_max, const int *__restrict__ count,
                                                 int nin, int nout, const float *__restrict__ hp, const int *__restrict__ step, float *__restrict__ loss_out)
{
    const int e = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    const int n = count[m], chunks = (n + kWideChunk - 1) / kWideChunk;
    if (e < kWideParams) {
        constexpr int off1 = (W32 + 1) * kH, off2 = off1 + (kH + 1) * kH;
        bool live;
        if (e < off1) live = e / kH < nin || e / kH == W32;   // layer 0: rows >= in are padding, row 32 is the bias
        else if (e < off2) live = true;
        else live = (e - off2) % W32 < nout;                   // layer 2: columns >= out are padding
        if (live) { // padding: weight and moments never touched
            const float *__restrict__ pm = part + (size_t)m * chunks_max * kWideParams;
            float gsum = 0.0f; // fixed order: deterministic. Eight loads in flight, added in chunk order
            int c = 0;
            for (; c + 8 <= chunks; c += 8) {
                float t[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) t[q] = pm[(size_t)(c + q) * kWideParams + e];
#pragma unroll
                for (int q = 0; q < 8; ++q) gsum += t[q];
            }
            for (; c < chunks; ++c) gsum += pm[(size_t)c * kWideParams + e];
            const float lr = hp[4 * m], b1 = hp[4 * m + 1], b2 = hp[4 * m + 2], eps = hp[4 * m + 3];
            const size_t at = (size_t)m * kWideParams + e;
            const int t = step[0]; // advanced by this step's forward pass
            const float bc1 = 1.0f - powf(b1, (float)t), bc2 = 1.0f - powf(b2, (float)t);
            const float lr_t = lr * sqrtf(bc2) / bc1;
            const float mn = adam_first_moment(b1, Mo[at], gsum), vn = b2 * Vo[at] + (1.0f - b2) * gsum * gsum;
            Mo[at] = mn; Vo[at] = vn;
            P[at] = P[at] - lr_t * mn / (sqrtf(vn) + eps);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) loss_out[m] = wb_mean(loss_part + (size_t)m * blocks_max, n, nout);
}

__global__ void k_wb_mean(const float *__restrict__ part, int stride, const int *__restrict__ count, int nout, int B, float *__restrict__ out)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < B) out[m] = wb_mean(part + (size_t)m * stride, count[m], nout);
}

// grid (ceil(cap * 32 / 256), B): member m's rows out of the pool (Xp [n][32] padded, Yp [n][nout]) by its index list, validated on the host
__global__ __launch_bounds__(256) void k_wb_gather(const float *__restrict__ Xp, const float *__restrict__ Yp, const int *__restrict__ idx,
                                                   const int *__restrict__ count, int cap, int nout, float *__restrict__ Xo, float *__restrict__ Yo)
{
    const int m = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x, i = t / W32, c = t % W32;
    if (i >= count[m]) return;
    const int row = idx[(size_t)m * cap + i];
    Xo[((size_t)m * cap + i) * W32 + c] = Xp[(size_t)row * W32 + c];
    if (c < nout) Yo[((size_t)m * cap + i) * nout + c] = Yp[(size_t)row * nout + c];
}

} // namespace

struct mppi_learner_wide_batch {
    int device = 0, B = 0, nin = 0, nout = 0;
    hipStream_t stream = nullptr;
    float *P = nullptr, *M = nullptr, *V = nullptr; // [B][kWideParams]
    int *step = nullptr;
    int n = 0, data_cap = 0;
    float *dX = nullptr, *dY = nullptr; // the pool: [n][32] padded, [n][out]
    // the splits as the host validated them; an empty train list = the default (rows 0..n-1, no test rows)
    std::vector<std::vector<int32_t>> train, test;
    bool dirty = true; // the device copies below are stale
    int *d_counts = nullptr;                                                  // [2][B] = n_train, n_test
    float *d_scale = nullptr, *d_hp = nullptr, *d_eval = nullptr, *d_hist = nullptr; // [2][B]; [B][4]; [2][B]; [2][hist_cap]
    size_t hist_cap = 0;
    // sized by the largest split (sync_splits): the members' rows, activations, deltas, partial tiles and loss partials
    float *Xtr = nullptr, *Ytr = nullptr, *Xte = nullptr, *Yte = nullptr;     // [B][cap][32], [B][cap][out], [B][tcap][32], [B][tcap][out]
    float *A1 = nullptr, *A2 = nullptr, *D1 = nullptr, *D2 = nullptr, *D3 = nullptr; // [B][rows][256] x 4, [B][rows][32]; rows = max(cap, tcap)
    float *part = nullptr, *loss_part = nullptr, *test_part = nullptr;        // [B][chunks_max][kWideParams], [B][blocks_max], [B][tblocks_max]
    int cap = 0, tcap = 0, rows = 0, chunks_max = 0, blocks_max = 0, tblocks_max = 0, max_test = 0;
    float *d_roll = nullptr; // mppi_learner_wide_batch_validate's inputs, partials and trajectories: one buffer, grown on demand
    size_t roll_cap = 0;
    std::string err;
};

static thread_local std::string g_wb_err;
static mppi_status wfail(mppi_learner_wide_batch *wb, mppi_status st, const std::string &msg)
{
    if (wb) wb->err = msg; else g_wb_err = msg;
    return st;
}
#define W_TRY(wb, expr)                                                                           \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return wfail((wb), MPPI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T> static mppi_status wb_alloc(mppi_learner_wide_batch *wb, T **p, size_t count, const char *what)
{
    *p = nullptr;
    hipError_t e = hipMalloc((void **)p, sizeof(T) * (count ? count : 1));
    if (e == hipSuccess) return MPPI_OK;
    (void)hipGetLastError();
    *p = nullptr;
    return wfail(wb, MPPI_ERR_ALLOC, std::string("wide learner batch: cannot allocate ") + what + " (" + std::to_string(sizeof(T) * count) + " bytes): " + hipGetErrorString(e));
}
template <typename T> static void wb_free(T **p) { if (*p) { (void)hipFree((void *)*p); *p = nullptr; } }

static void free_split_buffers(mppi_learner_wide_batch *wb)
{
    float **ps[] = {&wb->Xtr, &wb->Ytr, &wb->Xte, &wb->Yte, &wb->A1, &wb->A2, &wb->D1, &wb->D2, &wb->D3, &wb->part, &wb->loss_part, &wb->test_part};
    for (float **p : ps) wb_free(p);
    wb->dirty = true;
}

// counts, loss scales, the members' gathered rows and everything sized by the largest split onto the device (after set_data / set_split;
// the stream is idle)
static mppi_status sync_splits(mppi_learner_wide_batch *wb)
{
    if (!wb->dirty) return MPPI_OK;
    free_split_buffers(wb);
    const int B = wb->B, nout = wb->nout;
    int cap = 1, tcap = 0;
    for (int m = 0; m < B; ++m) {
        cap = std::max(cap, wb->train[m].empty() ? wb->n : (int)wb->train[m].size());
        tcap = std::max(tcap, (int)wb->test[m].size());
    }
    const int rows = std::max(cap, tcap), tcap1 = std::max(tcap, 1);
    const int chunks = (cap + kWideChunk - 1) / kWideChunk, blocks = (cap + kTile - 1) / kTile, tblocks = std::max((tcap + kTile - 1) / kTile, 1);
    std::vector<int32_t> idx, tidx, counts;
    std::vector<float> scale;
    try {
        idx.assign((size_t)B * cap, 0); tidx.assign((size_t)B * tcap1, 0); counts.assign(2 * (size_t)B, 0); scale.assign(2 * (size_t)B, 0.0f);
    } catch (const std::bad_alloc &) { return wfail(wb, MPPI_ERR_ALLOC, "out of host memory"); }
    for (int m = 0; m < B; ++m) {
        int32_t *row = idx.data() + (size_t)m * cap;
        if (wb->train[m].empty()) { for (int i = 0; i < wb->n; ++i) row[i] = i; counts[m] = wb->n; }
        else { memcpy(row, wb->train[m].data(), sizeof(int32_t) * wb->train[m].size()); counts[m] = (int32_t)wb->train[m].size(); }
        if (!wb->test[m].empty()) memcpy(tidx.data() + (size_t)m * tcap1, wb->test[m].data(), sizeof(int32_t) * wb->test[m].size());
        counts[B + m] = (int32_t)wb->test[m].size();
        // the lone learner's host expression, per member
        scale[m] = 2.0f / ((float)counts[m] * (float)nout);
        scale[B + m] = counts[B + m] > 0 ? 2.0f / ((float)counts[B + m] * (float)nout) : 0.0f;
    }
    int *d_idx = nullptr, *d_tidx = nullptr;
    auto body = [&]() -> mppi_status {
        mppi_status s;
        if ((s = wb_alloc(wb, &d_idx, idx.size(), "the train index lists")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &d_tidx, tidx.size(), "the test index lists")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->Xtr, (size_t)B * cap * W32, "the members' training inputs [B][max n_train][32]")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->Ytr, (size_t)B * cap * nout, "the members' training targets")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->Xte, (size_t)B * tcap1 * W32, "the members' test inputs")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->Yte, (size_t)B * tcap1 * nout, "the members' test targets")) != MPPI_OK) return s;
        float **acts[] = {&wb->A1, &wb->A2, &wb->D1, &wb->D2};
        for (float **p : acts)
            if ((s = wb_alloc(wb, p, (size_t)B * rows * kH, "the activations and deltas [B][max rows][256]")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->D3, (size_t)B * rows * W32, "the output deltas [B][max rows][32]")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->part, (size_t)B * chunks * kWideParams, "the partial gradient tiles")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->loss_part, (size_t)B * blocks, "the loss partials")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->test_part, (size_t)B * tblocks, "the test loss partials")) != MPPI_OK) return s;
        W_TRY(wb, hipMemcpy(d_idx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice));
        W_TRY(wb, hipMemcpy(d_tidx, tidx.data(), sizeof(int32_t) * tidx.size(), hipMemcpyHostToDevice));
        W_TRY(wb, hipMemcpy(wb->d_counts, counts.data(), sizeof(int32_t) * counts.size(), hipMemcpyHostToDevice));
        W_TRY(wb, hipMemcpy(wb->d_scale, scale.data(), sizeof(float) * scale.size(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_wb_gather, dim3((unsigned)(((size_t)cap * W32 + 255) / 256), B), dim3(256), 0, wb->stream, (const float *)wb->dX,
                           (const float *)wb->dY, (const int *)d_idx, (const int *)wb->d_counts, cap, nout, wb->Xtr, wb->Ytr);
        W_TRY(wb, hipGetLastError());
        if (tcap > 0) {
            hipLaunchKernelGGL(k_wb_gather, dim3((unsigned)(((size_t)tcap * W32 + 255) / 256), B), dim3(256), 0, wb->stream, (const float *)wb->dX,
                               (const float *)wb->dY, (const int *)d_tidx, (const int *)(wb->d_counts + B), tcap1, nout, wb->Xte, wb->Yte);
            W_TRY(wb, hipGetLastError());
        }
        W_TRY(wb, hipStreamSynchronize(wb->stream));
        return MPPI_OK;
    };
    mppi_status s = body();
    if (s != MPPI_OK) (void)hipStreamSynchronize(wb->stream);
    wb_free(&d_idx); wb_free(&d_tidx);
    if (s != MPPI_OK) { free_split_buffers(wb); return s; }
    wb->cap = cap; wb->tcap = tcap1; wb->rows = rows;
    wb->chunks_max = chunks; wb->blocks_max = blocks; wb->tblocks_max = tblocks;
    wb->max_test = tcap;
    wb->dirty = false;
    return MPPI_OK;
}

extern "C" const char *mppi_learner_wide_batch_last_error(const mppi_learner_wide_batch *wb) { return wb ? wb->err.c_str() : g_wb_err.c_str(); }

extern "C" int mppi_learner_wide_batch_size(const mppi_learner_wide_batch *wb) { return wb ? wb->B : 0; }

extern "C" void mppi_learner_wide_batch_destroy(mppi_learner_wide_batch *wb)
{
    if (!wb) return;
    (void)hipSetDevice(wb->device);
    if (wb->stream) (void)hipStreamSynchronize(wb->stream);
    free_split_buffers(wb);
    wb_free(&wb->P); wb_free(&wb->M); wb_free(&wb->V); wb_free(&wb->step);
    wb_free(&wb->dX); wb_free(&wb->dY); wb_free(&wb->d_counts); wb_free(&wb->d_scale); wb_free(&wb->d_hp); wb_free(&wb->d_eval); wb_free(&wb->d_hist);
    wb_free(&wb->d_roll);
    if (wb->stream) (void)hipStreamDestroy(wb->stream);
    delete wb;
}

extern "C" mppi_status mppi_learner_wide_batch_set_weights(mppi_learner_wide_batch *wb, int member, const float *const *W, const float *const *b)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    if (!W || !b) return wfail(wb, MPPI_ERR_INVALID_ARG, "NULL weights");
    if (member < -1 || member >= wb->B) return wfail(wb, MPPI_ERR_INVALID_ARG, "member out of range (-1: every member)");
    for (int k = 0; k < kWideLayers; ++k) if (!W[k] || !b[k]) return wfail(wb, MPPI_ERR_INVALID_ARG, "NULL weights");
    const int width[kWideLayers + 1] = {wb->nin, kH, kH, wb->nout};
    std::vector<float> img;
    try { img.assign(kWideParams, 0.0f); } catch (const std::bad_alloc &) { return wfail(wb, MPPI_ERR_ALLOC, "out of host memory"); } // the padding is written as zero
    for (int q = 0; q < kWideLayers; ++q) {
        const int in = width[q], out = width[q + 1], rows = kWideRows[q], cols = kWideCols[q];
        float *t = img.data() + kWideOff[q];
        for (int i = 0; i < in; ++i) for (int o = 0; o < out; ++o) t[(size_t)i * cols + o] = W[q][(size_t)i * out + o];
        for (int o = 0; o < out; ++o) t[(size_t)rows * cols + o] = b[q][o];
    }
    W_TRY(wb, hipSetDevice(wb->device));
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    for (int m = member < 0 ? 0 : member; m < (member < 0 ? wb->B : member + 1); ++m)
        W_TRY(wb, hipMemcpy(wb->P + (size_t)m * kWideParams, img.data(), sizeof(float) * kWideParams, hipMemcpyHostToDevice));
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_get_weights(mppi_learner_wide_batch *wb, int member, float *const *W, float *const *b)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    if (!W || !b) return wfail(wb, MPPI_ERR_INVALID_ARG, "NULL output");
    if (member < 0 || member >= wb->B) return wfail(wb, MPPI_ERR_INVALID_ARG, "member out of range");
    const int width[kWideLayers + 1] = {wb->nin, kH, kH, wb->nout};
    std::vector<float> img(kWideParams);
    W_TRY(wb, hipSetDevice(wb->device));
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    W_TRY(wb, hipMemcpy(img.data(), wb->P + (size_t)member * kWideParams, sizeof(float) * kWideParams, hipMemcpyDeviceToHost));
    for (int q = 0; q < kWideLayers; ++q) {
        const int in = width[q], out = width[q + 1], rows = kWideRows[q], cols = kWideCols[q];
        const float *t = img.data() + kWideOff[q];
        if (W[q]) for (int i = 0; i < in; ++i) for (int o = 0; o < out; ++o) W[q][(size_t)i * out + o] = t[(size_t)i * cols + o];
        if (b[q]) for (int o = 0; o < out; ++o) b[q][o] = t[(size_t)rows * cols + o];
    }
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_reset_optimizer(mppi_learner_wide_batch *wb)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    const size_t all = (size_t)wb->B * kWideParams;
    W_TRY(wb, hipSetDevice(wb->device));
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    W_TRY(wb, hipMemset(wb->M, 0, sizeof(float) * all));
    W_TRY(wb, hipMemset(wb->V, 0, sizeof(float) * all));
    W_TRY(wb, hipMemset(wb->step, 0, sizeof(int)));
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_get_step(mppi_learner_wide_batch *wb, int *step)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    if (!step) return wfail(wb, MPPI_ERR_INVALID_ARG, "NULL output");
    W_TRY(wb, hipSetDevice(wb->device));
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    W_TRY(wb, hipMemcpy(step, wb->step, sizeof(int), hipMemcpyDeviceToHost));
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_create(int n_members, int n_layers, const int32_t *widths, const float *const *W, const float *const *b,
                                                      int device, mppi_learner_wide_batch **out)
{
    if (!out || !widths || !W || !b) return wfail(nullptr, MPPI_ERR_INVALID_ARG, "NULL argument");
    *out = nullptr;
    // the shape and the member count first, before the device is touched
    if (n_layers != kWideLayers || !mppi_lrn_wide_shape(n_layers, widths))
        return wfail(nullptr, MPPI_ERR_UNSUPPORTED, "wide learner batch: the network is exactly [in, 256, 256, out] with in, out in 1..32 (narrow networks: mppi_learner_batch_create)");
    if (n_members < 1 || n_members > kMaxMembers) return wfail(nullptr, MPPI_ERR_INVALID_ARG, "wide learner batch: 1 to 1024 members");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return wfail(nullptr, MPPI_ERR_NO_DEVICE, "no HIP device visible: the learner has no CPU path"); }
    if (device < 0 || device >= ndev) return wfail(nullptr, MPPI_ERR_NO_DEVICE, "device ordinal out of range");
    mppi_learner_wide_batch *wb = new (std::nothrow) mppi_learner_wide_batch();
    if (!wb) return wfail(nullptr, MPPI_ERR_ALLOC, "out of host memory");
    wb->device = device;
    wb->B = n_members;
    wb->nin = widths[0]; wb->nout = widths[kWideLayers];
    wb->train.resize(n_members);
    wb->test.resize(n_members);
    auto body = [&]() -> mppi_status {
        W_TRY(wb, hipSetDevice(device));
        W_TRY(wb, hipStreamCreateWithFlags(&wb->stream, hipStreamNonBlocking));
        const size_t all = (size_t)n_members * kWideParams;
        mppi_status s;
        if ((s = wb_alloc(wb, &wb->P, all, "the weights")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->M, all, "the first Adam moments")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->V, all, "the second Adam moments")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->step, 1, "the step counter")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->d_counts, 2 * (size_t)n_members, "the split sizes")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->d_scale, 2 * (size_t)n_members, "the loss scales")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->d_hp, 4 * (size_t)n_members, "the rates")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->d_eval, 2 * (size_t)n_members, "the losses")) != MPPI_OK) return s;
        if ((s = mppi_learner_wide_batch_set_weights(wb, -1, W, b)) != MPPI_OK) return s;
        return mppi_learner_wide_batch_reset_optimizer(wb);
    };
    mppi_status s = body();
    if (s != MPPI_OK) { g_wb_err = wb->err; mppi_learner_wide_batch_destroy(wb); return s; }
    *out = wb;
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_set_data(mppi_learner_wide_batch *wb, const float *X, const float *Y, int n)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    if (!X || !Y || n <= 0) return wfail(wb, MPPI_ERR_INVALID_ARG, "X is [n, in], Y is [n, out], n > 0");
    W_TRY(wb, hipSetDevice(wb->device));
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    const int nin = wb->nin, nout = wb->nout;
    std::vector<float> pad; // the inputs padded to 32 columns with zeros, as the lone learner holds them
    try { pad.assign((size_t)n * W32, 0.0f); } catch (const std::bad_alloc &) { return wfail(wb, MPPI_ERR_ALLOC, "out of host memory"); }
    for (size_t i = 0; i < (size_t)n; ++i) memcpy(&pad[i * W32], X + i * nin, sizeof(float) * nin);
    if (n > wb->data_cap) {
        wb_free(&wb->dX); wb_free(&wb->dY);
        wb->n = 0; wb->data_cap = 0;
        mppi_status s;
        if ((s = wb_alloc(wb, &wb->dX, (size_t)n * W32, "X")) != MPPI_OK) return s;
        if ((s = wb_alloc(wb, &wb->dY, (size_t)n * nout, "Y")) != MPPI_OK) { wb_free(&wb->dX); return s; }
        wb->data_cap = n;
    }
    W_TRY(wb, hipMemcpy(wb->dX, pad.data(), sizeof(float) * pad.size(), hipMemcpyHostToDevice));
    W_TRY(wb, hipMemcpy(wb->dY, Y, sizeof(float) * (size_t)n * nout, hipMemcpyHostToDevice));
    wb->n = n;
    for (int m = 0; m < wb->B; ++m) { wb->train[m].clear(); wb->test[m].clear(); } // a new pool: every split back to rows 0..n-1, no test rows
    wb->dirty = true;
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_set_split(mppi_learner_wide_batch *wb, int member, const int32_t *train_idx, int n_train,
                                                         const int32_t *test_idx, int n_test)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    if (wb->n <= 0) return wfail(wb, MPPI_ERR_INVALID_ARG, "no data: call mppi_learner_wide_batch_set_data first");
    if (member < 0 || member >= wb->B) return wfail(wb, MPPI_ERR_INVALID_ARG, "member out of range");
    if (!train_idx || n_train < 1 || n_test < 0 || (n_test > 0 && !test_idx)) return wfail(wb, MPPI_ERR_INVALID_ARG, "n_train >= 1 train rows, n_test >= 0 test rows");
    // every index is checked HERE: the gather reads the pool unguarded
    for (int i = 0; i < n_train; ++i)
        if (train_idx[i] < 0 || train_idx[i] >= wb->n) return wfail(wb, MPPI_ERR_INVALID_ARG, "train_idx[" + std::to_string(i) + "] = " + std::to_string(train_idx[i]) + " is outside [0, " + std::to_string(wb->n) + ")");
    for (int i = 0; i < n_test; ++i)
        if (test_idx[i] < 0 || test_idx[i] >= wb->n) return wfail(wb, MPPI_ERR_INVALID_ARG, "test_idx[" + std::to_string(i) + "] = " + std::to_string(test_idx[i]) + " is outside [0, " + std::to_string(wb->n) + ")");
    try {
        std::vector<int32_t> tr(train_idx, train_idx + n_train), te;
        if (n_test > 0) te.assign(test_idx, test_idx + n_test);
        wb->train[member].swap(tr);
        wb->test[member].swap(te);
    } catch (const std::bad_alloc &) { return wfail(wb, MPPI_ERR_ALLOC, "out of host memory"); }
    wb->dirty = true;
    return MPPI_OK;
}

// the forward pass of every member over its training rows (test = false) or its test rows: A1, A2, the output delta and the loss partials
static mppi_status enqueue_forward(mppi_learner_wide_batch *wb, bool test, int apply, float *test_prev)
{
    const int B = wb->B, nout = wb->nout;
    const float *W0 = wb->P + kWideOff[0], *W1 = wb->P + kWideOff[1], *W2 = wb->P + kWideOff[2];
    const float *b0 = W0 + W32 * kH, *b1 = W1 + kH * kH, *b2 = W2 + kH * W32;
    const int *count = wb->d_counts + (test ? B : 0);
    const size_t sAct = (size_t)wb->rows * kH;
    const unsigned mt = (unsigned)(test ? wb->tblocks_max : wb->blocks_max);
    const dim3 thr(256);
    WbGemm g{};
    g.A = test ? wb->Xte : wb->Xtr; g.sA = (size_t)(test ? wb->tcap : wb->cap) * W32; g.lda = W32; g.B = W0; g.sB = kWideParams; g.ldb = kH;
    g.count = count; g.N = kH; g.K = W32; g.C = wb->A1; g.sC = sAct; g.ldc = kH; g.bias = b0;
    g.test_prev = test_prev; g.test_part = wb->test_part; g.n_test = wb->d_counts + B; g.test_stride = wb->tblocks_max; g.nout = nout;
    hipLaunchKernelGGL((k_wb_gemm<true, false, EPI_BIAS_RELU>), dim3(mt, kH / kTile, B), thr, 0, wb->stream, g);
    W_TRY(wb, hipGetLastError());
    g.test_prev = nullptr;
    g.A = wb->A1; g.sA = sAct; g.lda = kH; g.B = W1; g.K = kH; g.C = wb->A2; g.bias = b1;
    hipLaunchKernelGGL((k_wb_gemm<true, false, EPI_BIAS_RELU>), dim3(mt, kH / kTile, B), thr, 0, wb->stream, g);
    W_TRY(wb, hipGetLastError());
    g = WbGemm{};
    g.A = wb->A2; g.sA = sAct; g.lda = kH; g.B = W2; g.sB = kWideParams; g.ldb = W32; g.count = count; g.N = W32; g.K = kH;
    g.C = wb->D3; g.sC = (size_t)wb->rows * W32; g.ldc = W32; g.bias = b2;
    g.aux = test ? wb->Yte : wb->Ytr; g.sAux = (size_t)(test ? wb->tcap : wb->cap) * nout; g.nout = nout; g.scale = wb->d_scale + (test ? B : 0);
    g.loss_part = test ? wb->test_part : wb->loss_part; g.loss_stride = test ? wb->tblocks_max : wb->blocks_max; g.step = wb->step; g.apply = apply;
    hipLaunchKernelGGL((k_wb_gemm<true, false, EPI_LOSS>), dim3(mt, 1, B), thr, 0, wb->stream, g);
    W_TRY(wb, hipGetLastError());
    return MPPI_OK;
}

// forward + backward + gradients + Adam of every member [+ the held-out forward pass] onto the stream
static mppi_status enqueue_step(mppi_learner_wide_batch *wb, float *loss_train_row, float *test_prev_row, bool test)
{
    const int B = wb->B;
    mppi_status st = enqueue_forward(wb, false, 1, test_prev_row);
    if (st != MPPI_OK) return st;
    const float *W1 = wb->P + kWideOff[1], *W2 = wb->P + kWideOff[2];
    const size_t sAct = (size_t)wb->rows * kH, sOut = (size_t)wb->rows * W32;
    const unsigned mt = (unsigned)wb->blocks_max;
    const dim3 thr(256);
    // backward: D2 = (D3 W2^T) [A2 > 0] ; D1 = (D2 W1^T) [A1 > 0]
    WbGemm g{};
    g.A = wb->D3; g.sA = sOut; g.lda = W32; g.B = W2; g.sB = kWideParams; g.ldb = W32; g.count = wb->d_counts; g.N = kH; g.K = W32;
    g.C = wb->D2; g.sC = sAct; g.ldc = kH; g.aux = wb->A2; g.sAux = sAct;
    hipLaunchKernelGGL((k_wb_gemm<true, true, EPI_MASK>), dim3(mt, kH / kTile, B), thr, 0, wb->stream, g);
    W_TRY(wb, hipGetLastError());
    g.A = wb->D2; g.sA = sAct; g.lda = kH; g.B = W1; g.ldb = kH; g.K = kH; g.C = wb->D1; g.aux = wb->A1;
    hipLaunchKernelGGL((k_wb_gemm<true, true, EPI_MASK>), dim3(mt, kH / kTile, B), thr, 0, wb->stream, g);
    W_TRY(wb, hipGetLastError());
    // weight gradients: dW_l = A_l^T D_{l+1} over chunks of samples
    const float *acts[kWideLayers] = {wb->Xtr, wb->A1, wb->A2}, *dels[kWideLayers] = {wb->D1, wb->D2, wb->D3};
    const size_t s_acts[kWideLayers] = {(size_t)wb->cap * W32, sAct, sAct}, s_dels[kWideLayers] = {sAct, sAct, sOut};
    for (int q = 0; q < kWideLayers; ++q) {
        const int mtiles = (kWideRows[q] + kTile - 1) / kTile;
        g = WbGemm{};
        g.A = acts[q]; g.sA = s_acts[q]; g.lda = kWideRows[q]; g.B = dels[q]; g.sB = s_dels[q]; g.ldb = kWideCols[q]; g.count = wb->d_counts;
        g.M = kWideRows[q]; g.N = kWideCols[q]; g.C = wb->part + kWideOff[q]; g.sC = (size_t)wb->chunks_max * kWideParams; g.ldc = kWideCols[q];
        g.db_row = kWideRows[q]; g.mtiles = mtiles;
        hipLaunchKernelGGL((k_wb_gemm<false, false, EPI_PART>), dim3(wb->chunks_max, (kWideCols[q] + kTile - 1) / kTile, mtiles * B), thr, 0, wb->stream, g);
        W_TRY(wb, hipGetLastError());
    }
    hipLaunchKernelGGL(k_wb_adam, dim3((kWideParams + 255) / 256, B), thr, 0, wb->stream, wb->P, wb->M, wb->V, (const float *)wb->part, wb->chunks_max,
                       (const float *)wb->loss_part, wb->blocks_max, (const int *)wb->d_counts, wb->nin, wb->nout, (const float *)wb->d_hp,
                       (const int *)wb->step, loss_train_row);
    W_TRY(wb, hipGetLastError());
    if (test) return enqueue_forward(wb, true, 0, nullptr);
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_train(mppi_learner_wide_batch *wb, int steps, const float *lr, const float *beta1, const float *beta2,
                                                     const float *eps, float *loss_train, float *loss_test)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    if (wb->n <= 0) return wfail(wb, MPPI_ERR_INVALID_ARG, "no data: call mppi_learner_wide_batch_set_data first");
    const int B = wb->B;
    if (steps <= 0 || !lr || (size_t)steps * B > ((size_t)1 << 28)) return wfail(wb, MPPI_ERR_INVALID_ARG, "steps > 0 (steps * members <= 2^28), lr is [members]");
    std::vector<float> hp(4 * (size_t)B);
    for (int m = 0; m < B; ++m) {
        const float l = lr[m], b1 = beta1 ? beta1[m] : 0.9f, b2 = beta2 ? beta2[m] : 0.999f, e = eps ? eps[m] : 1e-7f;
        if (!(l > 0.0f) || !(b1 >= 0.0f && b1 < 1.0f) || !(b2 >= 0.0f && b2 < 1.0f) || !(e >= 0.0f))
            return wfail(wb, MPPI_ERR_INVALID_ARG, "member " + std::to_string(m) + ": lr > 0, 0 <= beta < 1, eps >= 0");
        hp[4 * m] = l; hp[4 * m + 1] = b1; hp[4 * m + 2] = b2; hp[4 * m + 3] = e;
    }
    W_TRY(wb, hipSetDevice(wb->device));
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    mppi_status st = sync_splits(wb);
    if (st != MPPI_OK) return st;
    const size_t cells = (size_t)steps * B;
    if (cells > wb->hist_cap) {
        wb_free(&wb->d_hist); wb->hist_cap = 0;
        if ((st = wb_alloc(wb, &wb->d_hist, 2 * cells, "the loss histories")) != MPPI_OK) return st;
        wb->hist_cap = cells;
    }
    float *h_train = wb->d_hist, *h_test = wb->d_hist + wb->hist_cap;
    const bool test = loss_test != nullptr && wb->max_test > 0;
    W_TRY(wb, hipMemcpy(wb->d_hp, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice));
    for (int s = 0; s < steps; ++s) {
        st = enqueue_step(wb, h_train + (size_t)s * B, test && s > 0 ? h_test + (size_t)(s - 1) * B : nullptr, test);
        if (st != MPPI_OK) { (void)hipStreamSynchronize(wb->stream); return st; }
    }
    if (test) {
        hipLaunchKernelGGL(k_wb_mean, dim3((B + 255) / 256), dim3(256), 0, wb->stream, (const float *)wb->test_part, wb->tblocks_max,
                           (const int *)(wb->d_counts + B), wb->nout, B, h_test + (size_t)(steps - 1) * B);
        W_TRY(wb, hipGetLastError());
    }
    // the histories were written on the device: one synchronisation, then the copies
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    if (loss_train) W_TRY(wb, hipMemcpy(loss_train, h_train, sizeof(float) * cells, hipMemcpyDeviceToHost));
    if (test) W_TRY(wb, hipMemcpy(loss_test, h_test, sizeof(float) * cells, hipMemcpyDeviceToHost));
    else if (loss_test) for (size_t i = 0; i < cells; ++i) loss_test[i] = std::numeric_limits<float>::quiet_NaN(); // no member has test rows
    return MPPI_OK;
}

extern "C" mppi_status mppi_learner_wide_batch_evaluate(mppi_learner_wide_batch *wb, float *loss_train, float *loss_test)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    if (wb->n <= 0) return wfail(wb, MPPI_ERR_INVALID_ARG, "no data: call mppi_learner_wide_batch_set_data first");
    W_TRY(wb, hipSetDevice(wb->device));
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    mppi_status st = sync_splits(wb);
    if (st != MPPI_OK) return st;
    const int B = wb->B;
    const bool test = loss_test != nullptr && wb->max_test > 0;
    // the forward pass of a step without its update, over the training rows and then over the test rows
    for (int pass = 0; pass < (test ? 2 : 1); ++pass) {
        if ((st = enqueue_forward(wb, pass == 1, 0, nullptr)) != MPPI_OK) { (void)hipStreamSynchronize(wb->stream); return st; }
        hipLaunchKernelGGL(k_wb_mean, dim3((B + 255) / 256), dim3(256), 0, wb->stream, (const float *)(pass ? wb->test_part : wb->loss_part),
                           pass ? wb->tblocks_max : wb->blocks_max, (const int *)(wb->d_counts + pass * B), wb->nout, B, wb->d_eval + pass * B);
        W_TRY(wb, hipGetLastError());
    }
    W_TRY(wb, hipStreamSynchronize(wb->stream));
    if (loss_train) W_TRY(wb, hipMemcpy(loss_train, wb->d_eval, sizeof(float) * B, hipMemcpyDeviceToHost));
    if (test) W_TRY(wb, hipMemcpy(loss_test, wb->d_eval + B, sizeof(float) * B, hipMemcpyDeviceToHost));
    else if (loss_test) for (int m = 0; m < B; ++m) loss_test[m] = std::numeric_limits<float>::quiet_NaN();
    return MPPI_OK;
}

// ---- trajectory validation: every member's network rolled open-loop in one launch (k_wb_rollout, mppi_learner_wide_rollout.hip).
// mppi_learner_batch_rollout's refusals and buffer handling; it reads P only.
extern "C" mppi_status mppi_learner_wide_batch_validate(mppi_learner_wide_batch *wb, const mppi_learner_model *model, const float *x0, int kx,
                                                        const float *V, const float *G, int n, int T, double *sse_out, float *X_out)
{
    if (!wb) return MPPI_ERR_INVALID_ARG;
    const std::string who = "mppi_learner_wide_batch_validate: ";
    // every refusal before the device is touched
    if (!model || !x0 || !V) return wfail(wb, MPPI_ERR_INVALID_ARG, who + "model, x0 [kx, s_dim] and V [T, n, a_dim] are required: NULL pointer");
    if (!sse_out && !X_out) return wfail(wb, MPPI_ERR_INVALID_ARG, who + "sse_out and X_out are both NULL");
    if (sse_out && !G) return wfail(wb, MPPI_ERR_INVALID_ARG, who + "sse_out needs the ground truth G [T+1, n, s_dim]");
    if (n < 1 || T < 1) return wfail(wb, MPPI_ERR_INVALID_ARG, who + "n and T must be >= 1");
    if ((size_t)n * (size_t)T > ((size_t)1 << 30)) return wfail(wb, MPPI_ERR_INVALID_ARG, who + "n * T must not exceed 2^30");
    if (kx != 1 && kx != n) return wfail(wb, MPPI_ERR_INVALID_ARG, who + "x0 is [kx, s_dim] with kx in {1, n}");
    if (model->model_kind != MPPI_MODEL_MLP)
        return wfail(wb, MPPI_ERR_UNSUPPORTED, who + "model_kind must be MPPI_MODEL_MLP: the wide network is the point-mass controller's, no wide 13-state network exists");
    if (model->a_dim < 1 || model->a_dim > kWideRollMaxA || model->s_dim != 2 * model->a_dim)
        return wfail(wb, MPPI_ERR_UNSUPPORTED, who + "s_dim = " + std::to_string(model->s_dim) + ", a_dim = " + std::to_string(model->a_dim) +
            ": MPPI_MODEL_MLP takes s_dim = 2 a_dim with a_dim in 1..4");
    const int s_dim = model->s_dim, a_dim = model->a_dim, nin = s_dim + a_dim, B = wb->B;
    if (wb->nin != nin || wb->nout != s_dim)
        return wfail(wb, MPPI_ERR_UNSUPPORTED, who + "the batch's widths are [" + std::to_string(wb->nin) + ", 256, 256, " + std::to_string(wb->nout) +
            "]: a_dim = " + std::to_string(a_dim) + " takes [" + std::to_string(nin) + ", 256, 256, " + std::to_string(s_dim) + "] (s_dim + a_dim -> s_dim)");
    WbRollout r{};
    for (int j = 0; j < 3 * kWideRollMaxA; ++j) { r.xmean[j] = 0.0f; r.xstd[j] = 1.0f; }
    for (int j = 0; j < 2 * kWideRollMaxA; ++j) { r.ymean[j] = 0.0f; r.ystd[j] = 1.0f; }
    for (int j = 0; j < nin; ++j) {
        if (model->xmean) r.xmean[j] = model->xmean[j];
        if (model->xstd) r.xstd[j] = model->xstd[j];
        if (r.xstd[j] == 0.0f) return wfail(wb, MPPI_ERR_INVALID_ARG, who + "xstd[" + std::to_string(j) + "] is 0: the inputs are divided by it");
    }
    for (int j = 0; j < s_dim; ++j) {
        if (model->ymean) r.ymean[j] = model->ymean[j];
        if (model->ystd) r.ystd[j] = model->ystd[j];
    }
    const size_t s = (size_t)s_dim, a = (size_t)a_dim, rows = (size_t)n * (size_t)T, blocks = ((size_t)n + kWideRollR - 1) / kWideRollR;
    r.P = wb->P; r.s = s_dim; r.a = a_dim; r.kx = kx; r.n = n; r.T = T; r.blocks = (int)blocks;
    W_TRY(wb, hipSetDevice(wb->device));
    // one buffer on the batch, carved into x0, V, G, the partials and X (each part a multiple of 64 floats: 256-byte starts)
    const auto pad = [](size_t c) { return (c + 63) & ~(size_t)63; };
    const size_t c_x = pad((size_t)kx * s), c_V = pad(rows * a), c_G = G ? pad((rows + n) * s) : 0, c_part = G ? pad((size_t)B * blocks * s) : 0,
                 c_X = X_out ? pad((size_t)B * (rows + n) * s) : 0, total = c_x + c_V + c_G + c_part + c_X;
    if (total > wb->roll_cap) {
        W_TRY(wb, hipStreamSynchronize(wb->stream));
        wb_free(&wb->d_roll); wb->roll_cap = 0;
        if (mppi_status st = wb_alloc(wb, &wb->d_roll, total, "the trajectories [B][T+1][n][s_dim] and their inputs"); st != MPPI_OK) return st;
        wb->roll_cap = total;
    }
    float *dx = wb->d_roll, *dV = dx + c_x, *dG = G ? dV + c_V : nullptr, *dpart = G ? dV + c_V + c_G : nullptr, *dX = X_out ? dV + c_V + c_G + c_part : nullptr;
    hipStream_t q = wb->stream;
    W_TRY(wb, hipMemcpyAsync(dx, x0, sizeof(float) * (size_t)kx * s, hipMemcpyHostToDevice, q));
    W_TRY(wb, hipMemcpyAsync(dV, V, sizeof(float) * rows * a, hipMemcpyHostToDevice, q));
    if (G) W_TRY(wb, hipMemcpyAsync(dG, G, sizeof(float) * (rows + n) * s, hipMemcpyHostToDevice, q));
    r.x0 = dx; r.V = dV; r.G = dG; r.X = dX; r.part = dpart;
    if (hipError_t e = mppi_lrn_launch_wide_rollout(r, B, q); e != hipSuccess) {
        (void)hipStreamSynchronize(q);
        return wfail(wb, MPPI_ERR_HIP, who + hipGetErrorString(e));
    }
    std::vector<float> part(sse_out ? (size_t)B * blocks * s : 0);
    if (sse_out) W_TRY(wb, hipMemcpyAsync(part.data(), dpart, sizeof(float) * part.size(), hipMemcpyDeviceToHost, q));
    if (X_out) W_TRY(wb, hipMemcpyAsync(X_out, dX, sizeof(float) * (size_t)B * (rows + n) * s, hipMemcpyDeviceToHost, q));
    W_TRY(wb, hipStreamSynchronize(q));
    if (sse_out) // the blocks of a member in block order, in fp64
        for (int m = 0; m < B; ++m)
            for (size_t j = 0; j < s; ++j) {
                double acc = 0.0;
                for (size_t b = 0; b < blocks; ++b) acc += (double)part[((size_t)m * blocks + b) * s + j];
                sse_out[(size_t)m * s + j] = acc;
            }
    return MPPI_OK;
}
