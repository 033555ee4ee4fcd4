// mppi_learner_wide.hip — the learner of the network a MPPI_MODEL_MLP controller rolls out: [in, 256, 256, out], in / out <= 32 (padded
// to 32 with zeros), relu on the two hidden layers, full-batch Adam on the mean squared error. The semantics are mppi_learner.hip's; the
// arithmetic is GEMMs with the batch as one dimension, all on v_mfma_f32_32x32x2_f32 (exact fp32: bitwise a k-ordered fmaf chain).
// One kernel template, k_wide_gemm: a 64 x 64 tile of C per workgroup (4 waves, one 32 x 32 accumulator each), k in slabs of 32 through
// LDS, the next slab's global loads in flight while the current one is multiplied. Three operand layouts and four epilogues:
//   forward   A1 = relu(X W0 + b0), A2 = relu(A1 W1 + b1)                 X . W     bias + relu
//             P = A2 W2 + b2 ; D3 = 2 (P - Y) / (n out) ; squared error   X . W     loss (block sum, fixed order; advances the step counter)
//   backward  D2 = (D3 W2^T) [A2 > 0], D1 = (D2 W1^T) [A1 > 0]            D . W^T   mask
//   gradient  dW_l = A_l^T D_{l+1}, db_l = 1^T D_{l+1}                    A^T . D   split over chunks of kWideChunk samples: one partial
//                                                                                  tile per chunk; the column sum of D rides along
// One step = 8 GEMM launches + k_wide_adam (one thread per padded parameter: the chunks' partial tiles summed in fixed order, the Keras
// update, padding left exactly zero; one thread sums the loss). No float atomics: two learners on the same data give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mppi_learner.hip.h"

using namespace mppi_lrn;

namespace {

constexpr int kH = kWideHidden;
constexpr int kWideChunk = 512;  // samples per partial gradient tile: n = 65 536 -> 128 chunks x 82 464 floats = 42 MB
constexpr int kTile = 64;        // C tile of a workgroup (kTile x kTile), 2 x 2 waves, one 32 x 32 accumulator each
constexpr int kSlab = 32;        // k per LDS slab
constexpr int kLd = kTile + 1;   // LDS row stride (odd: the transposing writes of a k-contiguous operand hit 32 distinct banks)
typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { EPI_BIAS_RELU = 0, EPI_LOSS = 1, EPI_MASK = 2, EPI_PART = 3 };

struct GemmArgs {
    const float *A, *B; // operands; see load_tile for the two layouts
    int lda, ldb;
    int M, N, K;        // C is [M][N]; k runs over 0..K-1 (EPI_PART: over the samples of this workgroup's chunk)
    float *C;           // [M][ldc] (EPI_PART: the partial tiles, chunk stride kWideParams)
    int ldc;
    const float *bias;  // [N]   EPI_BIAS_RELU, EPI_LOSS
    const float *aux;   // EPI_LOSS: Y [M][nout] ; EPI_MASK: the activation [M][ldc]
    int nout;           // EPI_LOSS
    float scale;        // EPI_LOSS: 2 / (n nout)
    float *loss_part;   // EPI_LOSS: [gridDim.x]
    float *pred;        // EPI_LOSS: NULL or [M][nout]
    int *step;          // EPI_LOSS
    int apply;          // EPI_LOSS
    int db_row;         // EPI_PART: the row of the tile that takes the column sums of B (= M)
};

// A 64 (m or n) x 32 (k) tile of an operand into registers, then into LDS as S[k][mn]. KC: element (mn, k) is P[mn * ld + k] (k contiguous:
// a row-major activation as the left operand, W^T as the right one); otherwise P[k * ld + mn] (mn contiguous: W as the right operand, the
// sample-major activations and deltas of the gradient GEMM). Out-of-range elements read as zero. Global reads are coalesced in both forms.
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

// v_mfma_f32_32x32x2_f32: D[m][n] += sum_{k<2} Aop[m][k] Bop[k][n]; lane (r = lane & 31, kh = lane >> 5) supplies Aop[r][kh] and Bop[kh][r];
// accumulator register q of that lane is element [row = 8 (q >> 2) + 4 kh + (q & 3)][col = r].
// grid: EPI_PART (chunks, N tiles, M tiles), otherwise (M tiles, N tiles).
template <bool A_KC, bool B_KC, int EPI>
__global__ __launch_bounds__(256) void k_wide_gemm(const GemmArgs g)
{
    __shared__ float As[kSlab * kLd], Bs[kSlab * kLd];
    __shared__ float red_s[4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, kh = lane >> 5;
    const int wm = w >> 1, wn = w & 1;
    const int chunk = EPI == EPI_PART ? (int)blockIdx.x : 0;
    const int m0 = (EPI == EPI_PART ? (int)blockIdx.z : (int)blockIdx.x) * kTile, n0 = (int)blockIdx.y * kTile;
    // EPI_PART: k = the samples [kbeg, kend) of this chunk (chunk * kWideChunk < K < 2^31)
    const int kbeg = EPI == EPI_PART ? chunk * kWideChunk : 0;
    const int kend = EPI == EPI_PART ? (g.K - kbeg < kWideChunk ? g.K : kbeg + kWideChunk) : g.K;
    const bool live = m0 + wm * 32 < g.M && n0 + wn * 32 < g.N; // wave-uniform: a 32-wide edge leaves half the waves without a tile
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float db = 0.0f;
    float va[8], vb[8];
    load_tile<A_KC>(g.A, g.lda, m0, g.M, kbeg, kend, va, tid);
    load_tile<B_KC>(g.B, g.ldb, n0, g.N, kbeg, kend, vb, tid);
    for (int k0 = kbeg; k0 < kend; k0 += kSlab) {
        __syncthreads(); // the previous slab has been read
        store_tile<A_KC>(As, va, tid);
        store_tile<B_KC>(Bs, vb, tid);
        __syncthreads();
        if (k0 + kSlab < kend) { // the next slab's loads fly while this one is multiplied
            load_tile<A_KC>(g.A, g.lda, m0, g.M, k0 + kSlab, kend, va, tid);
            load_tile<B_KC>(g.B, g.ldb, n0, g.N, k0 + kSlab, kend, vb, tid);
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
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = m0 + wm * 32 + 8 * (q >> 2) + 4 * kh + (q & 3);
            if (m >= g.M) continue;
            if (EPI == EPI_BIAS_RELU) {
                const float z = acc[q] + g.bias[n];
                g.C[(size_t)m * g.ldc + n] = z < 0.0f ? 0.0f : z;
            } else if (EPI == EPI_MASK) {
                g.C[(size_t)m * g.ldc + n] = g.aux[(size_t)m * g.ldc + n] > 0.0f ? acc[q] : 0.0f;
            } else if (EPI == EPI_LOSS) {
                const float p = acc[q] + g.bias[n];
                const float e = n < g.nout ? p - g.aux[(size_t)m * g.nout + n] : 0.0f;
                se += e * e;
                g.C[(size_t)m * g.ldc + n] = g.scale * e; // the padded columns of the delta are written as zero
                if (g.pred != nullptr && n < g.nout) g.pred[(size_t)m * g.nout + n] = p;
            } else {
                g.C[(size_t)chunk * kWideParams + (size_t)m * g.ldc + n] = acc[q];
            }
        }
    }
    if (EPI == EPI_PART && m0 == 0 && tid < kTile && n0 + tid < g.N)
        g.C[(size_t)chunk * kWideParams + (size_t)g.db_row * g.ldc + n0 + tid] = db;
    if (EPI == EPI_LOSS) { // block sum of the squared errors, fixed order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
        if (lane == 0) red_s[w] = se;
        __syncthreads();
        if (tid == 0) g.loss_part[blockIdx.x] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        // the optimiser step this pass belongs to: advanced HERE, launches ahead of the Adam kernel whose workgroups all read it
        if (g.apply && blockIdx.x == 0 && tid == 0) g.step[0] = g.step[0] + 1;
    }
}

// gradient = fixed-order sum of the chunks' partial tiles; Adam as tf.keras.optimizers.Adam applies it: m = b1 m + (1-b1) g ;
// v = b2 v + (1-b2) g^2 ; w -= lr sqrt(1-b2^t)/(1-b1^t) m / (sqrt(v) + eps). One thread per element of the padded layout; an element
// outside [in][256] / [256][out] / its bias rows is padding: gradient written as zero, weight and moments never touched.
__global__ __launch_bounds__(256) void k_wide_adam(float *__restrict__ P, float *__restrict__ Mo, float *__restrict__ Vo, float *__restrict__ G,
                                                   const float *__restrict__ part, int chunks, const float *__restrict__ loss_part, int loss_blocks,
                                                   int n, int nin, int nout, float lr, float b1, float b2, float eps, const int *__restrict__ step,
                                                   float *__restrict__ loss_out, int apply)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < kWideParams) {
        constexpr int off1 = (W32 + 1) * kH, off2 = off1 + (kH + 1) * kH;
        bool live;
        if (e < off1) live = e / kH < nin || e / kH == W32;   // layer 0: rows >= in are padding, row 32 is the bias
        else if (e < off2) live = true;
        else live = (e - off2) % W32 < nout;                   // layer 2: columns >= out are padding
        float gsum = 0.0f; // fixed order: deterministic. Eight loads in flight, added in chunk order
        int c = 0;
        for (; c + 8 <= chunks; c += 8) {
            float t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = part[(size_t)(c + q) * kWideParams + e];
#pragma unroll
            for (int q = 0; q < 8; ++q) gsum += t[q];
        }
        for (; c < chunks; ++c) gsum += part[(size_t)c * kWideParams + e];
        if (!live) gsum = 0.0f;
        G[e] = gsum;
        if (apply && live) {
            const int t = step[0]; // advanced by this step's forward pass
            const float bc1 = 1.0f - powf(b1, (float)t), bc2 = 1.0f - powf(b2, (float)t);
            const float lr_t = lr * sqrtf(bc2) / bc1;
            const float mn = adam_first_moment(b1, Mo[e], gsum), vn = b2 * Vo[e] + (1.0f - b2) * gsum * gsum;
            Mo[e] = mn; Vo[e] = vn;
            P[e] = P[e] - lr_t * mn / (sqrtf(vn) + eps);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s = 0.0f;
        for (int q = 0; q < loss_blocks; ++q) s += loss_part[q];
        loss_out[0] = s / ((float)n * (float)nout);
    }
}

mppi_status alloc_fail(mppi_learner *l, size_t bytes, hipError_t e)
{
    (void)hipGetLastError();
    return mppi_lrn_fail(l, MPPI_ERR_ALLOC, "learner: cannot allocate " + std::to_string(bytes) + " bytes of device memory for the training set (" +
                                                hipGetErrorString(e) + ")");
}

} // namespace

bool mppi_lrn_wide_shape(int n_layers, const int32_t *widths)
{
    return n_layers == kWideLayers && widths[0] >= 1 && widths[0] <= W32 && widths[1] == kH && widths[2] == kH && widths[3] >= 1 && widths[3] <= W32;
}

mppi_status mppi_lrn_wide_alloc(mppi_learner *l)
{
    float **ps[] = {&l->wP, &l->wM, &l->wV, &l->wG};
    for (float **p : ps) {
        L_TRY(l, hipMalloc((void **)p, sizeof(float) * kWideParams));
        l->bufs.push_back(*p);
        L_TRY(l, hipMemset(*p, 0, sizeof(float) * kWideParams));
    }
    return MPPI_OK;
}

mppi_status mppi_lrn_wide_reset(mppi_learner *l)
{
    L_TRY(l, hipMemset(l->wM, 0, sizeof(float) * kWideParams));
    L_TRY(l, hipMemset(l->wV, 0, sizeof(float) * kWideParams));
    L_TRY(l, hipMemset(l->d_step, 0, sizeof(int)));
    return MPPI_OK;
}

mppi_status mppi_lrn_wide_put(mppi_learner *l, float *image, int k, const float *const *W, const float *const *b)
{
    for (int q = 0; q < kWideLayers; ++q) {
        if (k >= 0 && q != k) continue;
        const int in = l->net.width[q], out = l->net.width[q + 1], rows = kWideRows[q], cols = kWideCols[q];
        std::vector<float> pad((size_t)(rows + 1) * cols, 0.0f); // the padding stays exactly zero
        for (int i = 0; i < in; ++i) for (int o = 0; o < out; ++o) pad[(size_t)i * cols + o] = W[q][(size_t)i * out + o];
        for (int o = 0; o < out; ++o) pad[(size_t)rows * cols + o] = b[q][o];
        L_TRY(l, hipMemcpy(image + kWideOff[q], pad.data(), sizeof(float) * pad.size(), hipMemcpyHostToDevice));
    }
    return MPPI_OK;
}

mppi_status mppi_lrn_wide_get(mppi_learner *l, const float *image, int k, float *const *W, float *const *b)
{
    for (int q = 0; q < kWideLayers; ++q) {
        if (k >= 0 && q != k) continue;
        const int in = l->net.width[q], out = l->net.width[q + 1], rows = kWideRows[q], cols = kWideCols[q];
        std::vector<float> pad((size_t)(rows + 1) * cols);
        L_TRY(l, hipMemcpy(pad.data(), image + kWideOff[q], sizeof(float) * pad.size(), hipMemcpyDeviceToHost));
        if (W && W[q]) for (int i = 0; i < in; ++i) for (int o = 0; o < out; ++o) W[q][(size_t)i * out + o] = pad[(size_t)i * cols + o];
        if (b && b[q]) for (int o = 0; o < out; ++o) b[q][o] = pad[(size_t)rows * cols + o];
    }
    return MPPI_OK;
}

mppi_status mppi_lrn_wide_set_data(mppi_learner *l, const float *X, const float *Y, int n)
{
    const int nin = l->net.width[0], nout = l->net.width[kWideLayers];
    const int chunks = (n + kWideChunk - 1) / kWideChunk, blocks = (n + kTile - 1) / kTile;
    if (n > l->cap) {
        float **ps[] = {&l->wX, &l->dY, &l->wA1, &l->wA2, &l->wD1, &l->wD2, &l->wD3, &l->d_part, &l->d_loss_part};
        for (float **p : ps) if (*p) { L_TRY(l, hipFree(*p)); *p = nullptr; }
        l->cap = 0; l->n = 0; // nothing to train on until every buffer stands
        const size_t sz[] = {(size_t)n * W32, (size_t)n * nout, (size_t)n * kH, (size_t)n * kH, (size_t)n * kH, (size_t)n * kH, (size_t)n * W32,
                             (size_t)chunks * kWideParams, (size_t)blocks};
        for (int q = 0; q < 9; ++q) {
            const hipError_t e = hipMalloc((void **)ps[q], sizeof(float) * sz[q]);
            if (e != hipSuccess) {
                *ps[q] = nullptr;
                for (float **p : ps) if (*p) { (void)hipFree(*p); *p = nullptr; }
                return alloc_fail(l, sizeof(float) * sz[q], e);
            }
        }
        l->cap = n;
    }
    std::vector<float> pad;
    try { pad.assign((size_t)n * W32, 0.0f); } catch (const std::bad_alloc &) { return mppi_lrn_fail(l, MPPI_ERR_ALLOC, "out of host memory"); }
    for (size_t i = 0; i < (size_t)n; ++i) memcpy(&pad[i * W32], X + i * nin, sizeof(float) * nin);
    L_TRY(l, hipMemcpy(l->wX, pad.data(), sizeof(float) * pad.size(), hipMemcpyHostToDevice));
    L_TRY(l, hipMemcpy(l->dY, Y, sizeof(float) * (size_t)n * nout, hipMemcpyHostToDevice));
    l->n = n; l->chunks = chunks; l->blocks = blocks;
    return MPPI_OK;
}

mppi_status mppi_lrn_wide_enqueue_step(mppi_learner *l, float lr, float b1, float b2, float eps, int apply, float *pred_dev)
{
    const int n = l->n, nin = l->net.width[0], nout = l->net.width[kWideLayers];
    float *W0 = l->wP + kWideOff[0], *W1 = l->wP + kWideOff[1], *W2 = l->wP + kWideOff[2];
    const float *b0 = W0 + W32 * kH, *b1p = W1 + kH * kH, *b2p = W2 + kH * W32;
    const dim3 thr(256);
    const unsigned mt = (unsigned)l->blocks;
    GemmArgs g{};
    // forward
    g.A = l->wX; g.lda = W32; g.B = W0; g.ldb = kH; g.M = n; g.N = kH; g.K = W32; g.C = l->wA1; g.ldc = kH; g.bias = b0;
    hipLaunchKernelGGL((k_wide_gemm<true, false, EPI_BIAS_RELU>), dim3(mt, kH / kTile), thr, 0, l->stream, g);
    L_TRY(l, hipGetLastError());
    g.A = l->wA1; g.lda = kH; g.B = W1; g.K = kH; g.C = l->wA2; g.bias = b1p;
    hipLaunchKernelGGL((k_wide_gemm<true, false, EPI_BIAS_RELU>), dim3(mt, kH / kTile), thr, 0, l->stream, g);
    L_TRY(l, hipGetLastError());
    g = GemmArgs{};
    g.A = l->wA2; g.lda = kH; g.B = W2; g.ldb = W32; g.M = n; g.N = W32; g.K = kH; g.C = l->wD3; g.ldc = W32; g.bias = b2p; g.aux = l->dY;
    g.nout = nout; g.scale = 2.0f / ((float)n * (float)nout); g.loss_part = l->d_loss_part; g.pred = pred_dev; g.step = l->d_step; g.apply = apply;
    hipLaunchKernelGGL((k_wide_gemm<true, false, EPI_LOSS>), dim3(mt, 1), thr, 0, l->stream, g);
    L_TRY(l, hipGetLastError());
    // backward: D2 = (D3 W2^T) [A2 > 0] ; D1 = (D2 W1^T) [A1 > 0]
    g = GemmArgs{};
    g.A = l->wD3; g.lda = W32; g.B = W2; g.ldb = W32; g.M = n; g.N = kH; g.K = W32; g.C = l->wD2; g.ldc = kH; g.aux = l->wA2;
    hipLaunchKernelGGL((k_wide_gemm<true, true, EPI_MASK>), dim3(mt, kH / kTile), thr, 0, l->stream, g);
    L_TRY(l, hipGetLastError());
    g.A = l->wD2; g.lda = kH; g.B = W1; g.ldb = kH; g.K = kH; g.C = l->wD1; g.aux = l->wA1;
    hipLaunchKernelGGL((k_wide_gemm<true, true, EPI_MASK>), dim3(mt, kH / kTile), thr, 0, l->stream, g);
    L_TRY(l, hipGetLastError());
    // weight gradients: dW_l = A_l^T D_{l+1} over chunks of samples
    const float *acts[kWideLayers] = {l->wX, l->wA1, l->wA2}, *dels[kWideLayers] = {l->wD1, l->wD2, l->wD3};
    for (int q = 0; q < kWideLayers; ++q) {
        g = GemmArgs{};
        g.A = acts[q]; g.lda = kWideRows[q]; g.B = dels[q]; g.ldb = kWideCols[q]; g.M = kWideRows[q]; g.N = kWideCols[q]; g.K = n;
        g.C = l->d_part + kWideOff[q]; g.ldc = kWideCols[q]; g.db_row = kWideRows[q];
        hipLaunchKernelGGL((k_wide_gemm<false, false, EPI_PART>), dim3(l->chunks, (kWideCols[q] + kTile - 1) / kTile, (kWideRows[q] + kTile - 1) / kTile),
                           thr, 0, l->stream, g);
        L_TRY(l, hipGetLastError());
    }
    hipLaunchKernelGGL(k_wide_adam, dim3((kWideParams + 255) / 256), thr, 0, l->stream, l->wP, l->wM, l->wV, l->wG, (const float *)l->d_part, l->chunks,
                       (const float *)l->d_loss_part, l->blocks, n, nin, nout, lr, b1, b2, eps, (const int *)l->d_step, l->d_loss, apply);
    L_TRY(l, hipGetLastError());
    return MPPI_OK;
}
