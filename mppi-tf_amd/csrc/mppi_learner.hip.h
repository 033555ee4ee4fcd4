// mppi_learner.hip.h — what the two translation units of the learner share: the mppi_learner object, its error plumbing and the entry
// points of the wide path. mppi_learner.hip holds the C-ABI and the narrow learner (every layer padded to 32, one sample per lane);
// mppi_learner_wide.hip holds the learner of the [in, 256, 256, out] network a MPPI_MODEL_MLP controller rolls out (LDS-tiled GEMMs on
// v_mfma_f32_32x32x2_f32). One object serves both: `wide` says which set of buffers is alive.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "mppi_c.h"

namespace mppi_lrn {

constexpr int W32 = 32;        // padded width of every layer of the narrow learner, and of the wide learner's two edges
constexpr int kMaxLayers = 4;
constexpr int kWideHidden = 256;
constexpr int kWideLayers = 3;
// The wide learner keeps weights, both Adam moments, the gradient and every partial gradient tile in ONE padded layout of kWideParams
// floats: layer l at kWideOff[l] as [rows_l + 1][cols_l] row-major, rows 0..rows_l-1 = W ([in][out]), row rows_l = the bias.
//   layer 0: [32 + 1][256]   (inputs padded to 32 rows)     layer 1: [256 + 1][256]     layer 2: [256 + 1][32]   (outputs padded to 32 columns)
constexpr int kWideRows[kWideLayers] = {W32, kWideHidden, kWideHidden};
constexpr int kWideCols[kWideLayers] = {kWideHidden, kWideHidden, W32};
constexpr int kWideOff[kWideLayers + 1] = {0, (W32 + 1) * kWideHidden, (W32 + 1) * kWideHidden + (kWideHidden + 1) * kWideHidden,
                                           (W32 + 1) * kWideHidden + (kWideHidden + 1) * kWideHidden + (kWideHidden + 1) * W32};
constexpr int kWideParams = kWideOff[kWideLayers];

struct Net { // device pointers; weights padded: W[l] is [32][32] ([in][out]), b[l] is [32]
    float *W[kMaxLayers], *b[kMaxLayers];
    int n_layers, width[kMaxLayers + 1]; // width[0] = inputs, width[l+1] = outputs of layer l
};

struct AdamState { float *m[kMaxLayers], *v[kMaxLayers], *mb[kMaxLayers], *vb[kMaxLayers]; };

// Adam's first moment, b1 m + (1 - b1) g, for all three learners (one body: the batch stays bit for bit a lone learner). The two terms
// cancel wherever the gradient turns against its running mean, and an fp32 sum of two rounded terms is then wrong by their size, not the
// result's (measured: up to 18 700 ulp of m'). Formed in fp64 and rounded once the stored moment is the correctly rounded one.
__device__ __forceinline__ float adam_first_moment(float b1, float m, float g)
{
    return (float)((double)b1 * (double)m + (1.0 - (double)b1) * (double)g);
}

// What k_lb_rollout takes, by value (mppi_learner_rollout.hip; filled by mppi_learner_batch_rollout, which has checked every field):
// the batch's weight block, the model around the network and the trajectories. Device pointers.
constexpr int kRollThreads = 64;  // one lane per trajectory, one wave per workgroup
constexpr int kRollMaxIn = 16, kRollMaxOut = 13; // the widest network input / output of the three model kinds
struct LbRollout {
    const float *P;                       // [B][L][33][32]
    int n_layers, width[kMaxLayers + 1];
    int kind, s, a;                       // MPPI_MODEL_MLP | _NN_AUV | _NN_AUV_SPEED; the state and action widths the kind fixes
    float dt;
    float xmean[kRollMaxIn], xstd[kRollMaxIn], ymean[kRollMaxOut], ystd[kRollMaxOut];
    const float *x0, *V, *G;              // [kx][s], [T][n][a], [T+1][n][s] or NULL
    float *X, *part;                      // [B][T+1][n][s] or NULL; [B][blocks][s] (with G)
    int kx, n, T, blocks;                 // blocks = ceil(n / kRollThreads)
};

// What k_wb_rollout takes, by value (mppi_learner_wide_rollout.hip; filled by mppi_learner_wide_batch_validate, which has checked every
// field): the wide batch's weight block in its padded layout, the MPPI_MODEL_MLP normalisation and the trajectories. Device pointers.
constexpr int kWideRollR = 16;    // trajectories of one member per workgroup (256 threads: one per hidden unit)
constexpr int kWideRollMaxA = 4;  // a_dim 1..4, s_dim = 2 a_dim: the network is [3a, 256, 256, 2a]
struct WbRollout {
    const float *P;                       // [B][kWideParams]
    int s, a;
    float xmean[3 * kWideRollMaxA], xstd[3 * kWideRollMaxA], ymean[2 * kWideRollMaxA], ystd[2 * kWideRollMaxA];
    const float *x0, *V, *G;              // [kx][s], [T][n][a], [T+1][n][s] or NULL
    float *X, *part;                      // [B][T+1][n][s] or NULL; [B][blocks][s] (with G)
    int kx, n, T, blocks;                 // blocks = ceil(n / kWideRollR)
};

} // namespace mppi_lrn

// grid (blocks, B) on `st`; hipErrorInvalidValue for a (kind, s, a) no instance serves
hipError_t mppi_lrn_launch_rollout(const mppi_lrn::LbRollout &r, int B, hipStream_t st);
// grid (blocks, B) on `st`; hipErrorInvalidValue unless s = 2 a, a in 1..4
hipError_t mppi_lrn_launch_wide_rollout(const mppi_lrn::WbRollout &r, int B, hipStream_t st);

struct mppi_learner {
    int device = 0;
    hipStream_t stream = nullptr;
    mppi_lrn::Net net{};      // the wide learner uses n_layers and width[] only
    mppi_lrn::AdamState adam{};
    std::vector<float *> bufs;
    float *dX = nullptr, *dY = nullptr, *dA = nullptr, *dD = nullptr, *d_part = nullptr, *d_loss_part = nullptr, *d_loss = nullptr, *d_grads = nullptr;
    int *d_step = nullptr;
    int n = 0, cap = 0, chunks = 0, blocks = 0;
    std::string err;
    // the wide path: parameters, moments and gradient in the padded layout above (in bufs); per-sample buffers (freed by destroy):
    // wX [n][32] the padded inputs, wA1 / wA2 [n][256] the hidden activations, wD1 / wD2 [n][256] and wD3 [n][32] the deltas
    bool wide = false;
    float *wP = nullptr, *wM = nullptr, *wV = nullptr, *wG = nullptr;
    float *wX = nullptr, *wA1 = nullptr, *wA2 = nullptr, *wD1 = nullptr, *wD2 = nullptr, *wD3 = nullptr;
};

mppi_status mppi_lrn_fail(mppi_learner *l, mppi_status st, const std::string &msg);
#define L_TRY(l, expr)                                                                            \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return mppi_lrn_fail((l), MPPI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// ---- mppi_learner_wide.hip (the caller has checked its arguments, set the device and, where it matters, synchronised the stream)
bool mppi_lrn_wide_shape(int n_layers, const int32_t *widths);                 // exactly [1..32, 256, 256, 1..32]
mppi_status mppi_lrn_wide_alloc(mppi_learner *l);                              // wP, wM, wV, wG
mppi_status mppi_lrn_wide_set_data(mppi_learner *l, const float *X, const float *Y, int n);
mppi_status mppi_lrn_wide_enqueue_step(mppi_learner *l, float lr, float b1, float b2, float eps, int apply, float *pred_dev);
// compact host arrays <-> one padded device image (wP, wM, wV or wG). Layer k alone, or every layer with k = -1. Padding is written as zero.
mppi_status mppi_lrn_wide_put(mppi_learner *l, float *image, int k, const float *const *W, const float *const *b);
mppi_status mppi_lrn_wide_get(mppi_learner *l, const float *image, int k, float *const *W, float *const *b);
mppi_status mppi_lrn_wide_reset(mppi_learner *l);
