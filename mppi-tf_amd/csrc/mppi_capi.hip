// mppi_capi.hip — host side of libmppi_hip.so: the C-ABI of include/mppi_c.h over the kernels
// of mppi_kernels.hip.h.  No CPU compute path exists here: every numeric entry point launches
// HIP kernels and fails with MPPI_ERR_NO_DEVICE / MPPI_ERR_HIP when it cannot.
// This unit: version and status strings, the error text, creation and destruction of lone and batched handles, the learned model's
// upload. The other concerns are mppi_capi_{set,step,shard,log,debug}.hip; mppi_capi.hip.h is what they share.

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#define MPPI_VERSION_STRING "mppi-hip 0.1.0 (gfx950)"

#include "mppi_capi.hip.h"

static thread_local std::string g_create_err;

namespace mppi_capi {
mppi_status fail(mppi_handle *h, mppi_status st, const std::string &msg)
{
    if (h) h->err = msg; else g_create_err = msg;
    return st;
}
} // namespace mppi_capi

// see mppi_handle.hip.h: process-wide, per (kernel instance, device), only ever raised
hipError_t mppi_raise_lds_ceiling(const void *kernel, int device, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> ceiling;
    if (bytes <= 48 * 1024) return hipSuccess; // the default ceiling
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = ceiling[{kernel, device}];
    if (bytes <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}

// ----------------------------------------------------------------------------------------
extern "C" int mppi_abi_version(void) { return MPPI_ABI_VERSION; }
extern "C" const char *mppi_version(void) { return MPPI_VERSION_STRING; }

extern "C" const char *mppi_status_string(mppi_status st)
{
    switch (st) {
    case MPPI_OK: return "ok";
    case MPPI_ERR_INVALID_ARG: return "invalid argument";
    case MPPI_ERR_NO_DEVICE: return "no HIP device";
    case MPPI_ERR_HIP: return "HIP runtime error";
    case MPPI_ERR_UNSUPPORTED: return "unsupported shape or option";
    case MPPI_ERR_SINGULAR_SIGMA: return "sigma is singular";
    case MPPI_ERR_ALLOC: return "allocation failed";
    case MPPI_ERR_IO: return "i/o error";
    case MPPI_ERR_EXCHANGE: return "direct exchange deadline missed";
    }
    return "unknown status";
}

extern "C" int mppi_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

extern "C" const char *mppi_last_error(const mppi_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" mppi_status mppi_config_init(mppi_config *cfg, int k, int tau, float dt, float mass, int s_dim, int a_dim)
{
    if (!cfg) return MPPI_ERR_INVALID_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->k = k; cfg->tau = tau; cfg->s_dim = s_dim; cfg->a_dim = a_dim;
    cfg->dt = dt; cfg->mass = mass;
    cfg->lambda = 1.0f; cfg->gamma = 1.0f; cfg->upsilon = 1.0f; // controller_base.cpp:40-41
    cfg->action_cost_kind = MPPI_ACTION_COST_CPP;
    cfg->seed = 1; // RandomNormal::Seed(1.) controller_base.cpp:199
    cfg->model_kind = MPPI_MODEL_POINT_MASS;
    cfg->shard_count = 1;
    return MPPI_OK;
}

// Σ⁻¹ (cost_base.cpp:39 MatrixInverse): Gauss-Jordan with partial pivoting in double.
static bool invert(const float *S, int n, float *out)
{
    double M[kMaxA][2 * kMaxA];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) { M[i][j] = S[i * n + j]; M[i][n + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r) if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
        if (std::fabs(M[p][c]) < 1e-300) return false;
        if (p != c) for (int j = 0; j < 2 * n; ++j) std::swap(M[c][j], M[p][j]);
        const double piv = M[c][c];
        for (int j = 0; j < 2 * n; ++j) M[c][j] /= piv;
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            const double f = M[r][c];
            if (f == 0.0) continue;
            for (int j = 0; j < 2 * n; ++j) M[r][j] -= f * M[c][j];
        }
    }
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) out[i * n + j] = (float)M[i][n + j];
    return true;
}

extern "C" void mppi_destroy(mppi_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)quiesce(h);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
    if (h->pre_ev) (void)hipEventDestroy(h->pre_ev);
    if (h->pre_ev2) (void)hipEventDestroy(h->pre_ev2);
    if (h->d_ugr) (void)hipFree(h->d_ugr);
    if (h->d_cu_ctr) (void)hipFree(h->d_cu_ctr);
    if (h->d_step_recs) (void)hipFree(h->d_step_recs);
    if (h->d_xslot) (void)hipFree(h->d_xslot);
    if (h->d_decision) (void)hipFree(h->d_decision);
    if (h->h_arm) (void)hipHostFree(h->h_arm);
    float *bufs[] = {h->d_x, h->d_Ubuf[0], h->d_Ubuf[1], h->d_u, h->d_cost, h->d_cost2, h->d_part, h->d_part2, h->d_part3,
                     h->d_record, h->d_dbg, h->d_mm, h->d_eps, h->d_recs, h->d_range, h->d_tile_mm};
    for (float *p : bufs) if (p) (void)hipFree(p);
    if (h->d_step) (void)hipFree(h->d_step);
    for (float *p : {h->d_bx, h->d_bu, h->d_ep, h->d_mr}) if (p) (void)hipFree(p);
    if (h->dM) (void)hipFree(h->dM);
    if (h->d_mlp_w) (void)hipFree(h->d_mlp_w);
    if (h->d_nn_args) (void)hipFree(h->d_nn_args);
    if (h->dC) (void)hipFree(h->dC);
    if (h->h_pin) (void)hipHostFree(h->h_pin);
    if (h->d_clip) (void)hipFree(h->d_clip);
    if (h->d_sg_rows) (void)hipFree(h->d_sg_rows);
    if (h->d_sg_start) (void)hipFree(h->d_sg_start);
    for (void *p : h->xchg_opened) (void)hipIpcCloseMemHandle(p);
    if (h->xchg_inbox) (void)hipFree(h->xchg_inbox);
    if (h->h_xchg_status) (void)hipHostFree(h->h_xchg_status);
    if (h->d_xchg_dead) (void)hipFree(h->d_xchg_dead);
    if (h->d_probe_got) (void)hipFree(h->d_probe_got);
    mppi_gen_destroy(h);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// Upload a learned model's weights and normalisation (mppi_create: allocate = true; mppi_set_mlp: the same buffers again).
// member >= 0 (a learned batch, mppi_create_batch_learned / mppi_create_batch_mlp): member m's network in the same layout at d_mlp_w + m * nn_stride, its MlpDev at
// dM + m and its padded layer pointers at d_nn_args + m (allocate: all B at once, with member 0); hm / small_args mirror member 0.
static mppi_status upload_mlp(mppi_handle *h, const mppi_mlp_desc *d, bool allocate, int member = -1)
{
    const int s = h->s, a = h->a;
    const bool speed = h->hc.model_kind == MPPI_MODEL_NN_AUV_SPEED;
    const bool nnauv = h->hc.model_kind == MPPI_MODEL_NN_AUV || speed;
    // NNAUVModel.prepare_data drops the position (nn_model.py:289-293); NNAUVModelSpeed's takes Euler angles, velocities, forces (:438-461)
    const int nin = speed ? 15 : (nnauv ? s + a - 3 : s + a), nout = speed ? 6 : s;
    if (member >= 0) {
        const size_t B = (size_t)h->batch;
        if (allocate) {
            size_t total = 0;
            for (int l = 0, w_in = nin; l < d->n_layers; w_in = d->widths[l], ++l) total += (size_t)(w_in + 1) * (d->widths[l] + 1);
            h->nn_stride = (total + 3) & ~(size_t)3; // members start 16-byte aligned
            HIP_TRY(h, hipMalloc((void **)&h->d_mlp_w, sizeof(float) * h->nn_stride * B));
            HIP_TRY(h, hipMalloc((void **)&h->dM, sizeof(MlpDev) * B));
            HIP_TRY(h, hipMalloc((void **)&h->d_nn_args, sizeof(MlpSmallArgs) * B));
        }
        // the lone upload below into member m's block, on a scratch copy of the host mirrors
        MlpDev hm{};
        MlpSmallArgs sa{};
        hm.n_layers = sa.n_layers = d->n_layers;
        float *p = h->d_mlp_w + h->nn_stride * (size_t)member;
        std::vector<float> image; // one member is ~12 KB: staged whole, one copy
        for (int l = 0, w_in = nin; l < d->n_layers; w_in = d->widths[l], ++l) {
            const int ld = (d->widths[l] & 1) ? d->widths[l] + 1 : d->widths[l];
            const size_t nw = (size_t)w_in * ld, at = image.size();
            image.resize(at + nw + ld, 0.0f);
            for (int i = 0; i < w_in; ++i) for (int o = 0; o < d->widths[l]; ++o) image[at + (size_t)i * ld + o] = d->W[l][(size_t)i * d->widths[l] + o];
            for (int o = 0; o < d->widths[l]; ++o) image[at + nw + o] = d->b[l][o];
            hm.widths[l] = d->widths[l];
            hm.ld[l] = ld;
            hm.Wl[l] = sa.W[l] = p + at;
            hm.bl[l] = sa.b[l] = p + at + nw;
        }
        if (!h->mlp_small && !nnauv) { // the {256, 256, s} network of k_rollout_mlp2_batch (mppi_create_batch_mlp)
            hm.W1 = hm.Wl[0]; hm.b1 = hm.bl[0]; hm.W2 = hm.Wl[1]; hm.b2 = hm.bl[1];
            hm.W3 = hm.Wl[2]; hm.b3 = hm.bl[2];
        }
        for (int i = 0; i < kMaxS + kMaxA; ++i) { hm.xmean[i] = 0.f; hm.xstd[i] = 1.f; }
        for (int i = 0; i < nin; ++i) { hm.xmean[i] = d->xmean ? d->xmean[i] : 0.f; hm.xstd[i] = d->xstd ? d->xstd[i] : 1.f; }
        for (int i = 0; i < nout; ++i) { hm.ymean[i] = d->ymean ? d->ymean[i] : 0.f; hm.ystd[i] = d->ystd ? d->ystd[i] : 1.f; }
        HIP_TRY(h, hipMemcpyAsync(p, image.data(), sizeof(float) * image.size(), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->dM + member, &hm, sizeof(MlpDev), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_nn_args + member, &sa, sizeof(MlpSmallArgs), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream)); // (the staging is pageable host memory of this call)
        if (member == 0) { h->hm = hm; h->small_args = sa; }
        return MPPI_OK;
    }
    if (allocate) {
        size_t total = 0;
        for (int l = 0, w_in = nin; l < d->n_layers; w_in = d->widths[l], ++l) total += (size_t)(w_in + 1) * (d->widths[l] + 1);
        HIP_TRY(h, hipMalloc((void **)&h->d_mlp_w, sizeof(float) * total));
        HIP_TRY(h, hipMalloc((void **)&h->dM, sizeof(MlpDev)));
    }
    float *p = h->d_mlp_w;
    h->hm.n_layers = d->n_layers;
    h->small_args.n_layers = d->n_layers;
    std::vector<float> padded; // an odd output layer (NNAUVModel: 13) is stored with one zero column more: outputs stay pairs
    for (int l = 0, w_in = nin; l < d->n_layers; w_in = d->widths[l], ++l) {
        const int ld = (nnauv && (d->widths[l] & 1)) ? d->widths[l] + 1 : d->widths[l];
        const size_t nw = (size_t)w_in * ld, nbias = (size_t)ld;
        if (ld != d->widths[l]) {
            padded.assign(nw + nbias, 0.0f);
            for (int i = 0; i < w_in; ++i) for (int o = 0; o < d->widths[l]; ++o) padded[(size_t)i * ld +
                o] = d->W[l][(size_t)i * d->widths[l] + o];
            for (int o = 0; o < d->widths[l]; ++o) padded[nw + o] = d->b[l][o];
            HIP_TRY(h, hipMemcpyAsync(p, padded.data(), sizeof(float) * (nw + nbias), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        } else {
            HIP_TRY(h, hipMemcpyAsync(p, d->W[l], sizeof(float) * nw, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(p + nw, d->b[l], sizeof(float) * nbias, hipMemcpyHostToDevice, h->stream));
        }
        h->hm.widths[l] = d->widths[l];
        h->hm.ld[l] = ld;
        h->hm.Wl[l] = h->small_args.W[l] = p;
        h->hm.bl[l] = h->small_args.b[l] = p + nw;
        p += nw + nbias;
    }
    if (!h->mlp_small && !nnauv) {
        h->hm.W1 = h->hm.Wl[0]; h->hm.b1 = h->hm.bl[0]; h->hm.W2 = h->hm.Wl[1]; h->hm.b2 = h->hm.bl[1];
        h->hm.W3 = h->hm.Wl[2]; h->hm.b3 = h->hm.bl[2];
    }
    for (int i = 0; i < kMaxS + kMaxA; ++i) { h->hm.xmean[i] = 0.f; h->hm.xstd[i] = 1.f; }
    for (int i = 0; i < nin; ++i) { h->hm.xmean[i] = d->xmean ? d->xmean[i] : 0.f; h->hm.xstd[i] = d->xstd ? d->xstd[i] : 1.f; }
    for (int i = 0; i < nout; ++i) { h->hm.ymean[i] = d->ymean ? d->ymean[i] : 0.f; h->hm.ystd[i] = d->ystd ? d->ystd[i] : 1.f; }
    HIP_TRY(h, hipMemcpyAsync(h->dM, &h->hm, sizeof(MlpDev), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

// The constants of one controller from its config, on the geometry derive_handle set (K_local, k_offset, H, s, a): once per member
// (member_consts). sigma_diag: 1 when Σ and Σ⁻¹ are diagonal (the DIAG instances). false: Σ is singular.
static bool fill_consts(const mppi_config *cfg, const mppi_handle *h, DevConsts &c, int &sigma_diag)
{
    const int s = h->s, a = h->a;
    c.K_local = h->K_local; c.k_offset = h->k_offset; c.H = h->H; c.s = s; c.a = a;
    c.q_full = cfg->q_is_full ? 1 : 0;
    c.action_cost_kind = cfg->action_cost_kind; c.model_kind = cfg->model_kind;
    c.state_cost_kind = cfg->state_cost_kind;
    if (cfg->state_cost_kind == MPPI_STATE_COST_ELLIPSE) for (int i = 0; i < 7; ++i) c.ell[i] = cfg->ellipse[i];
    c.lambda = cfg->lambda; c.neg_inv_lambda = -1.0f / cfg->lambda;
    c.gamma = cfg->gamma; c.upsilon = cfg->upsilon;
    c.py_ncoef = cfg->lambda * (1.0f - 1.0f / cfg->upsilon);
    c.dt = cfg->dt;
    c.bp = ((cfg->dt * cfg->dt) / 2.0f) / cfg->mass; // model_base.cpp:72 then RealDiv :74-76
    c.bq = cfg->dt / cfg->mass;
    c.seed = cfg->seed;
    for (int i = 0; i < s; ++i) c.goal[i] = cfg->goal ? cfg->goal[i] : ((i & 1) ? 0.0f : 1.0f);
    float sig[kMaxA * kMaxA], inv[kMaxA * kMaxA];
    for (int i = 0; i < a; ++i) for (int j = 0; j < a; ++j) sig[i * a + j] = cfg->sigma ? cfg->sigma[i * a + j] : (i == j ? 1.0f : 0.0f);
    if (!invert(sig, a, inv)) return false;
    sigma_diag = 1;
    // the sampler's matrix: Σ (C++, controller_base.cpp:201) or υ·Σ (Py build_noise); Σ⁻¹ stays that of Σ
    const float samp = (cfg->flags & MPPI_FLAG_UPSILON_SCALES_NOISE) ? cfg->upsilon : 1.0f;
    for (int i = 0; i < a; ++i) for (int j = 0; j < a; ++j) {
        c.sigma[i * kMaxA + j] = samp * sig[i * a + j]; c.sigma_inv[i * kMaxA + j] = inv[i * a + j];
        if (i != j && (sig[i * a + j] != 0.0f || inv[i * a + j] != 0.0f)) sigma_diag = 0;
    }
    bool q_offdiag = false;
    for (int i = 0; i < s; ++i) {
        if (cfg->q_is_full) {
            for (int j = 0; j < s; ++j) {
                c.qfull[i * kMaxS + j] = cfg->Q ? cfg->Q[i * s + j] : (i == j ? 1.0f : 0.0f);
                if (i != j && c.qfull[i * kMaxS + j] != 0.0f) q_offdiag = true;
            }
            c.qdiag[i] = c.qfull[i * kMaxS + i];
        } else {
            c.qdiag[i] = cfg->Q ? cfg->Q[i] : 1.0f;
            c.qfull[i * kMaxS + i] = c.qdiag[i];
        }
    }

    // A dense Q whose off-diagonal entries are all exactly zero (the Python reference's default task files)
    // evaluates bit-identically through the diagonal instances: the dropped products are exact zeros.
    if (cfg->q_is_full && !q_offdiag) c.q_full = 0;
    return true;
}

// ---- creation: validate the config, derive the handle's geometry, fill every member's constants,
// allocate ---------------------------------
// On the host a lone handle is the one-member case of a batch's layout (mppi_handle.hip.h, `batch`): mppi_create and the batch creators
// run the same three steps and the same allocation, at members(h) = 1 and n.
static const char *const kBadTemperature = "lambda must be > 0, upsilon != 0";
static bool temperature_ok(const mppi_config *cfg) { return cfg->lambda > 0.0f && cfg->upsilon != 0.0f; }

// what a config alone tells (no handle yet), then that a device serves it
static mppi_status validate_config(const mppi_config *cfg)
{
    const int s = cfg->s_dim, a = cfg->a_dim;
    if (cfg->k <= 0 || cfg->tau <= 0 || s <= 0 || a <= 0 || s > kMaxS || a > kMaxA)
        return fail(nullptr, MPPI_ERR_INVALID_ARG, "k, tau, s_dim, a_dim out of range");
    if (!temperature_ok(cfg)) return fail(nullptr, MPPI_ERR_INVALID_ARG, kBadTemperature);
    if (cfg->shard_count < 1 || cfg->shard_rank < 0 || cfg->shard_rank >= cfg->shard_count)
        return fail(nullptr, MPPI_ERR_INVALID_ARG, "bad shard_rank/shard_count");
    if (cfg->model_kind == MPPI_MODEL_POINT_MASS && !(cfg->mass != 0.0f)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
        "mass must be non-zero");
    if (cfg->model_kind < MPPI_MODEL_POINT_MASS || cfg->model_kind > MPPI_MODEL_NN_AUV_SPEED)
        return fail(nullptr, MPPI_ERR_INVALID_ARG, "unknown model kind");
    if (cfg->state_cost_kind < MPPI_STATE_COST_QUADRATIC || cfg->state_cost_kind > MPPI_STATE_COST_ELLIPSE3D)
        return fail(nullptr, MPPI_ERR_INVALID_ARG, "unknown state cost kind");
    // the 13-state AUV family (mppi_gen.hip.h): pose with a quaternion + body velocities, 6 generalised forces
    const bool nn_speed = cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED;
    const bool gen = cfg->model_kind == MPPI_MODEL_AUV || cfg->model_kind == MPPI_MODEL_NN_AUV || nn_speed;
    const bool cost13 = cfg->state_cost_kind == MPPI_STATE_COST_QUAT || cfg->state_cost_kind == MPPI_STATE_COST_ELLIPSE3D;
    if (gen && (s != 13 || a != 6)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
        "AUVModel / NNAUVModel: s_dim = 13 (pos, quat, lin vel, ang vel), a_dim = 6");
    if (cost13 && s != 13) return fail(nullptr, MPPI_ERR_INVALID_ARG,
        "StaticQuatCost / ElipseCost3D read a 13-state (static_cost.py:141-159, elipse_cost.py:124-139)");
    if (cost13 && !gen && cfg->k * (long long)cfg->tau > 1) return fail(nullptr, MPPI_ERR_UNSUPPORTED,
        "StaticQuatCost / ElipseCost3D rollouts need a 13-state model (MPPI_MODEL_AUV / MPPI_MODEL_NN_AUV)");
    if (cfg->model_kind == MPPI_MODEL_NN_AUV || nn_speed) {
        const mppi_mlp_desc *d = cfg->mlp;
        if (!d || !d->widths || !d->W || !d->b) return fail(nullptr, MPPI_ERR_INVALID_ARG, "NNAUVModel needs cfg.mlp with widths, W, b");
        if (d->n_layers < 2 || d->n_layers > kMlpSmallMaxLayers) return fail(nullptr, MPPI_ERR_UNSUPPORTED,
            "NNAUVModel: 2 to 4 Dense layers (1 to 3 hidden + the output layer)");
        for (int l = 0; l < d->n_layers; ++l) if (!d->W[l] || !d->b[l]) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "NULL MLP weight pointer");
        if (!nn_speed && d->widths[d->n_layers - 1] != 13) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "NNAUVModel: the last layer's width must be 13 (nn_model.py:59)");
        if (nn_speed && d->widths[d->n_layers - 1] != 6) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "NNAUVModelSpeed: the last layer's width must be 6, the velocity delta (nn_model.py:345)");
        if (nn_speed && (cfg->flags & MPPI_FLAG_MLP_BF16X3)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "MPPI_FLAG_MLP_BF16X3: no split-bf16 kernel for NNAUVModelSpeed");
        const int hid = d->widths[0];
        bool same = hid == 16 || hid == 32;
        for (int l = 0; l + 1 < d->n_layers; ++l) same = same && d->widths[l] == hid;
        if (!same) return fail(nullptr, MPPI_ERR_UNSUPPORTED,
            "NNAUVModel kernels exist for 1-3 equal hidden layers of 16 or 32 (nn_model.py:54-60)");
        if (hid != 32 && (cfg->flags & MPPI_FLAG_MLP_BF16X3)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "MPPI_FLAG_MLP_BF16X3 applies to the 256-wide and the 32-wide networks");
    }
    if (cfg->state_cost_kind == MPPI_STATE_COST_ELLIPSE) {
        if (!cfg->ellipse) return fail(nullptr, MPPI_ERR_INVALID_ARG, "the elliptic cost needs cfg.ellipse[7]");
        if (s < 4) return fail(nullptr, MPPI_ERR_INVALID_ARG, "the elliptic cost reads (x, vx, y, vy): s_dim >= 4");
        if (!(cfg->ellipse[0] != 0.0f) || !(cfg->ellipse[1] != 0.0f)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "ellipse axes a, b must be non-zero");
        if (cfg->model_kind == MPPI_MODEL_MLP) return fail(nullptr, MPPI_ERR_UNSUPPORTED,
            "MLP rollouts are instantiated for the quadratic state cost");
    }
    if (cfg->model_kind == MPPI_MODEL_MLP) {
        const mppi_mlp_desc *d = cfg->mlp;
        if (!d || !d->widths || !d->W || !d->b) return fail(nullptr, MPPI_ERR_INVALID_ARG, "MLP model needs cfg.mlp with widths, W, b");
        if (d->n_layers < 2 || d->n_layers > kMlpSmallMaxLayers) return fail(nullptr, MPPI_ERR_UNSUPPORTED,
            "MLP: 2 to 4 Dense layers (1 to 3 hidden + the output layer)");
        for (int l = 0; l < d->n_layers; ++l) if (!d->W[l] || !d->b[l]) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "NULL MLP weight pointer");
        if (d->widths[d->n_layers - 1] != s) return fail(nullptr, MPPI_ERR_INVALID_ARG, "MLP: the last layer's width must be s_dim");
        const int hid = d->widths[0];
        bool same = true;
        for (int l = 0; l + 1 < d->n_layers; ++l) same = same && d->widths[l] == hid;
        const bool big = d->n_layers == 3 && same && hid == kHid, small = same && (hid == 16 || hid == 32);
        if (!big && !small)
            return fail(nullptr, MPPI_ERR_UNSUPPORTED,
                "MLP kernels exist for hidden widths {256,256} (matrix cores) and 1-3 equal hidden layers of 16 or 32 (nn_model.py:54-60)");
        if (small && hid != 32 && (cfg->flags & MPPI_FLAG_MLP_BF16X3))
            return fail(nullptr, MPPI_ERR_INVALID_ARG, "MPPI_FLAG_MLP_BF16X3 applies to the 256-wide and the 32-wide networks");
        if (s != 2 * a || a > 4) return fail(nullptr, MPPI_ERR_UNSUPPORTED,
            "MLP rollouts are instantiated for s_dim == 2*a_dim, a_dim <= 4");
        if (cfg->q_is_full) return fail(nullptr, MPPI_ERR_UNSUPPORTED, "MLP rollouts are instantiated for a diagonal Q");
    }

    int ndev = mppi_device_count();
    if (ndev <= 0) return fail(nullptr, MPPI_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, MPPI_ERR_NO_DEVICE, "device ordinal out of range");
    return MPPI_OK;
}

// the handle of cfg's geometry, kernel flags and record count: nothing on the device yet, no constants
static mppi_status derive_handle(const mppi_config *cfg, mppi_handle **out)
{
    const int s = cfg->s_dim, a = cfg->a_dim;
    const bool gen = cfg->model_kind == MPPI_MODEL_AUV || cfg->model_kind == MPPI_MODEL_NN_AUV ||
        cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED;
    mppi_handle *h = new (std::nothrow) mppi_handle();
    if (!h) return fail(nullptr, MPPI_ERR_ALLOC, "out of host memory");
    h->device = cfg->device;
    h->K_global = cfg->k; h->shard_rank = cfg->shard_rank; h->shard_count = cfg->shard_count;
    // shard g owns [g*K/G, (g+1)*K/G)  
    const long long lo = (long long)cfg->shard_rank * cfg->k / cfg->shard_count;
    const long long hi = (long long)(cfg->shard_rank + 1) * cfg->k / cfg->shard_count;
    h->k_offset = (int)lo; h->K_local = (int)(hi - lo);
    if (h->K_local <= 0) { delete h; return fail(nullptr, MPPI_ERR_INVALID_ARG, "shard owns no samples"); }
    h->H = cfg->tau; h->s = s; h->a = a; h->HA = cfg->tau * a;
    h->normalize = cfg->normalize_cost;
    // 5 producers shorten a lone tile's pipeline (15.6 vs 18.3 us at 1 tile/CU) but cost throughput once
    // >= 4 tiles share a CU (the kernel is VALU-issue bound there): pick by tiles per CU.
    h->pc_np = ((h->K_local + 63) / 64 <= 2 * 256) ? 5 : 3;

    // tile geometry: the largest R in {64,32,16} whose LDS image fits one CU (160 KiB), preferring
    // <= ~53 KiB so three workgroups share a CU.
    const size_t lds_cap = 160 * 1024;
    int R = 64;
    while (R > 16 && tile_lds_floats(h->HA, R) * 4 > lds_cap) R >>= 1;
    // CostBase and ModelBase are separate classes in the reference (cost shapes such as s=4,a=3
    // or s=13,a=6 appear in its tests): such a handle serves the cost/model helpers, and the
    // rollout entry points answer MPPI_ERR_UNSUPPORTED with this reason.
    if (gen) R = 64; // one wave per 64-rollout tile, nothing parked in LDS
    if (gen) { /* rollouts run k_rollout_gen */ }
    else if (s != 2 * a) h->no_rollout = "point-mass rollouts need s_dim == 2*a_dim (blockDiag of 2x2 / 2x1 blocks, model_base.cpp:59-82)";
    else if (a > 4) h->no_rollout = "rollout kernels are instantiated for a_dim <= 4";
    else if (tile_lds_floats(h->HA, R) * 4 > lds_cap) h->no_rollout = "tau*a_dim too large: the 16-rollout LDS tile exceeds 160 KiB";
    h->R = R; h->nb = (h->K_local + R - 1) / R; h->tile_lds = tile_lds_floats(h->HA, R) * 4;
    h->mlp_bx3 = ((cfg->model_kind == MPPI_MODEL_MLP || cfg->model_kind == MPPI_MODEL_NN_AUV) &&
        (cfg->flags & MPPI_FLAG_MLP_BF16X3)) ? 1 : 0;
    h->fp_contract = (cfg->model_kind == MPPI_MODEL_POINT_MASS && (cfg->flags & MPPI_FLAG_FP_CONTRACT)) ? 1 : 0;
    h->mlp_small = ((cfg->model_kind == MPPI_MODEL_MLP && cfg->mlp->widths[0] != kHid) || cfg->model_kind == MPPI_MODEL_NN_AUV ||
                    cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED) ? cfg->mlp->widths[0] : 0;
    h->is_gen = gen ? 1 : 0;
    // a_dim = 4: two h1 images + the rest exceed 160 KiB of LDS
    h->mlp_v2 = (cfg->model_kind == MPPI_MODEL_MLP && !h->mlp_small && !h->mlp_bx3 && a <= 3) ? 1 : 0;
    h->nb_mlp = cfg->model_kind == MPPI_MODEL_MLP ? (h->mlp_v2 ? (h->K_local + kMlp2R - 1) / kMlp2R : (h->K_local + kMlpR - 1) / kMlpR) : 0;
    h->nbp = record_pad(std::max(h->nb, h->nb_mlp));
    *out = h;
    return MPPI_OK;
}

// Member m's constants from its config, the one validation of a member: its temperature, its Sigma, and that it runs the kernel instance
// member 0 picked (sigma_diag, the effective Q form; member 0 is filled into h->hc and sets both). A failure is
// g_create_err, naming the member if `named`.
// mixed: the status of a member whose effective Sigma or Q form differs from member 0's (mppi_create_batch_mlp: MPPI_ERR_INVALID_ARG).
static mppi_status member_consts(const mppi_config *cfg, int m, bool named, mppi_handle *h, DevConsts &c, mppi_status mixed = MPPI_ERR_UNSUPPORTED)
{
    const std::string who = named ? "batched controllers: member " + std::to_string(m) + ": " : "";
    if (!temperature_ok(cfg)) return fail(nullptr, MPPI_ERR_INVALID_ARG, who + kBadTemperature);
    int diag = 0;
    if (!fill_consts(cfg, h, c, diag)) return fail(nullptr, MPPI_ERR_SINGULAR_SIGMA, who + "sigma is singular");
    if (m == 0) { h->sigma_diag = diag; return MPPI_OK; } // (c is h->hc: member 0 sets what the others are compared with)
    if (diag != h->sigma_diag)
        return fail(nullptr, mixed,
            "batched controllers: sigma must be diagonal for every member or dense for every member (member " + std::to_string(m) +
            " differs from member 0)");
    if (c.q_full != h->hc.q_full)
        return fail(nullptr, mixed,
                                                       "batched controllers: Q must be diagonal for every member or dense for every "
                                                       "member (member " + std::to_string(m) +
                                                      " differs from member 0; a dense Q without off-diagonal entries counts as diagonal)");
    return MPPI_OK;
}

// Everything mppi_create reports for cfg before it allocates: the config, the geometry, member 0's
// constants (h->hc), the 13-state constants.
// member0: the error names member 0 (mppi_create_batch_configs).
static mppi_status prepare_handle(const mppi_config *cfg, bool member0, mppi_handle **out)
{
    auto named = [&](mppi_status st) { return member0 ? fail(nullptr, st, "batched controllers: member 0: " + g_create_err) : st; };
    if (mppi_status st = validate_config(cfg); st != MPPI_OK) return named(st);
    mppi_handle *h = nullptr;
    if (mppi_status st = derive_handle(cfg, &h); st != MPPI_OK) return named(st);
    mppi_status st = member_consts(cfg, 0, member0, h, h->hc);
    if (st == MPPI_OK && (h->is_gen || cfg->state_cost_kind == MPPI_STATE_COST_QUAT || cfg->state_cost_kind == MPPI_STATE_COST_ELLIPSE3D))
        if (const char *why = mppi_gen_fill(h, cfg)) st = named(fail(nullptr, MPPI_ERR_INVALID_ARG, why));
    if (st != MPPI_OK) { mppi_destroy(h); return st; }
    *out = h;
    return MPPI_OK;
}

// The device side of a prepared handle with B = members(h) members, whose constants are consts[0..B): the per-member buffers (U, costs,
// records, dbg words, constants) at B times their stride, the rest once. On a failure the caller destroys h (h->err says why).
static mppi_status allocate_handle(mppi_handle *h, const mppi_config *cfg, int B, const DevConsts *consts)
{
    const size_t K = (size_t)h->K_local, rec = (size_t)h->nbp * (2 + h->HA), us = (size_t)h->HA + h->a;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIP_TRY(h, hipMalloc((void **)&h->dC, sizeof(DevConsts) * B));
    HIP_TRY(h, hipMalloc((void **)&h->d_x, sizeof(float) * kMaxS));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(h, hipMalloc((void **)&h->d_Ubuf[i], sizeof(float) * us * B));
        HIP_TRY(h, hipMemsetAsync(h->d_Ubuf[i], 0, sizeof(float) * us * B, h->stream)); // U0 = 0, zero tails
    }
    HIP_TRY(h, hipMalloc((void **)&h->d_u, sizeof(float) * kMaxA));
    HIP_TRY(h, hipMalloc((void **)&h->d_cost, sizeof(float) * K * B));
    HIP_TRY(h, hipMalloc((void **)&h->d_cost2, sizeof(float) * h->K_local));
    // every member's record block with its neutral pads
    const int nrec = h->nbp;
    HIP_TRY(h, hipMalloc((void **)&h->d_part, sizeof(float) * rec * B));
    for (int m = 0; m < B; ++m) fill_neutral_records(h->stream, h->d_part + rec * m, nrec, 2 + h->HA);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // steps may be enqueued on the caller's stream
    const int nrec2 = (nrec + kGroup - 1) / kGroup, nrec3 = (nrec2 + kGroup - 1) / kGroup;
    HIP_TRY(h, hipMalloc((void **)&h->d_part2, sizeof(float) * (size_t)nrec2 * (2 + h->HA)));
    HIP_TRY(h, hipMalloc((void **)&h->d_part3, sizeof(float) * (size_t)nrec3 * (2 + h->HA)));
    if (cfg->model_kind == MPPI_MODEL_MLP || cfg->model_kind == MPPI_MODEL_NN_AUV || cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED) {
        // (a learned batch: member 0's network here, with the allocation for all; the creator uploads the others)
        if (mppi_status st_ = upload_mlp(h, cfg->mlp, true, h->nn_batch ? 0 : -1); st_ != MPPI_OK) return st_;
    }
    HIP_TRY(h, hipMalloc((void **)&h->d_record, sizeof(float) * (2 + h->HA)));
    HIP_TRY(h, hipMalloc((void **)&h->d_dbg, sizeof(float) * 8 * B));
    HIP_TRY(h, hipMalloc((void **)&h->d_mm, sizeof(float) * 4));
    if (h->normalize) HIP_TRY(h, hipMalloc((void **)&h->d_tile_mm, sizeof(float) * 2 * (size_t)nrec));
    HIP_TRY(h, hipMalloc((void **)&h->d_step, sizeof(unsigned long long)));
    // mppi_shard_step's buffers: allocated here, not inside the enqueue-only step (an allocation
    // there is an implicit device sync)
    if (h->shard_count > 1) {
        HIP_TRY(h, hipMalloc((void **)&h->d_recs, sizeof(float) * (size_t)(2 + h->HA) * h->shard_count));
        HIP_TRY(h, hipMalloc((void **)&h->d_range, sizeof(float) * 2));
    }
    HIP_TRY(h, hipHostMalloc((void **)&h->h_pin, sizeof(float) * (2 * kMaxS + kMaxA), hipHostMallocMapped));
    HIP_TRY(h, hipHostGetDevicePointer((void **)&h->d_pin, h->h_pin, 0));
    HIP_TRY(h, hipMemsetAsync(h->d_step, 0, sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_dbg, 0, sizeof(float) * 8 * B, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_cost, 0, sizeof(float) * K * B, h->stream));
    if (!h->batch && !h->is_gen && cfg->model_kind == MPPI_MODEL_POINT_MASS && h->no_rollout.empty() && h->R == 64) {
        // the whole step in one launch / the armed launch (mppi_step.hip.h): record granules of a <= 128-tile grid, the verdict words,
        // and the x slot the HOST stores into — fine-grained device memory, reachable from the CPU only on a large-BAR system
        // (without one d_xslot stays NULL and MPPI_TUNE_ARMED_US answers MPPI_ERR_UNSUPPORTED)
        if (h->nb <= 128) {
            HIP_TRY(h, hipMalloc((void **)&h->d_step_recs, sizeof(unsigned long long) * (size_t)(2 + h->HA) * 128));
            HIP_TRY(h, hipMemsetAsync(h->d_step_recs, 0, sizeof(unsigned long long) * (size_t)(2 + h->HA) * 128, h->stream));
        }
        HIP_TRY(h, hipMalloc((void **)&h->d_decision, 64));
        HIP_TRY(h, hipMemsetAsync(h->d_decision, 0, 64, h->stream));
        HIP_TRY(h, hipHostMalloc((void **)&h->h_arm, 64, hipHostMallocMapped));
        HIP_TRY(h, hipHostGetDevicePointer((void **)&h->d_arm, h->h_arm, 0));
        std::memset(h->h_arm, 0, 64);
        int large_bar = 0;
        if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, h->device) != hipSuccess) { large_bar = 0;
            (void)hipGetLastError(); }
        if (large_bar && hipExtMallocWithFlags((void **)&h->d_xslot, 256, hipDeviceMallocFinegrained) == hipSuccess)
            HIP_TRY(h, hipMemsetAsync(h->d_xslot, 0, 256, h->stream));
        else { h->d_xslot = nullptr; (void)hipGetLastError(); }
    }
    if (h->gen) HIP_TRY(h, mppi_gen_upload(h));
    if (h->batch) { // a batch's x and u staging; its records are laid out once, for the batched rollout's nb tiles per member
        HIP_TRY(h, hipMalloc((void **)&h->d_bx, sizeof(float) * (size_t)B * h->s));
        HIP_TRY(h, hipMalloc((void **)&h->d_bu, sizeof(float) * (size_t)B * h->a));
        h->part_nb = h->nb;
    }
    HIP_TRY(h, hipMemcpyAsync(h->dC, consts, sizeof(DevConsts) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_create(const mppi_config *cfg, mppi_handle **out)
{
    if (!cfg || !out) return fail(nullptr, MPPI_ERR_INVALID_ARG, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != sizeof(mppi_config)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
        "mppi_config.struct_size mismatch (use mppi_config_init)");
    mppi_handle *h = nullptr;
    if (mppi_status st = prepare_handle(cfg, false, &h); st != MPPI_OK) return st;
    if (mppi_status st = allocate_handle(h, cfg, 1, &h->hc); st != MPPI_OK) { g_create_err = h->err; mppi_destroy(h); return st; }
    *out = h;
    return MPPI_OK;
}

extern "C" mppi_status mppi_set_mlp(mppi_handle *h, const mppi_mlp_desc *d)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (h->nn_batch) return fail(h, MPPI_ERR_UNSUPPORTED, "mppi_set_mlp: a batched handle takes a member's network through mppi_batch_set_mlp");
    const int mk = h->hc.model_kind;
    if (mk != MPPI_MODEL_MLP && mk != MPPI_MODEL_NN_AUV && mk != MPPI_MODEL_NN_AUV_SPEED) return fail(h, MPPI_ERR_INVALID_ARG,
        "not a learned-model handle");
    if (!d || !d->widths || !d->W || !d->b) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_set_mlp needs widths, W, b");
    if (d->n_layers != h->hm.n_layers) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_set_mlp: the layer count is fixed at creation");
    for (int l = 0; l < d->n_layers; ++l) {
        if (d->widths[l] != h->hm.widths[l]) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_set_mlp: the layer widths are fixed at creation");
        if (!d->W[l] || !d->b[l]) return fail(h, MPPI_ERR_INVALID_ARG, "NULL MLP weight pointer");
    }
    MPPI_ENTER(h);
    // steps in flight read the old weights — on the handle's stream or on the caller's (mppi_next_device / mppi_shard_*): a weight
    // push is rare, so it simply waits for the whole device (only h->stream was waited for)
    HIP_TRY(h, hipDeviceSynchronize());
    return upload_mlp(h, d, false);
}

// ---- batched controllers (mppi_create_batch_configs; kernels in mppi_launch_batch.hip and mppi_launch_batch_gen.hip) ---------------
// Member m is made from cfgs[m]: its own seed, goal, lambda, gamma, upsilon, sigma and Q (its DevConsts block dC + m), its own x and
// sequence; the rest of the config is shared. Member m is bit for bit the lone handle mppi_create(&cfgs[m]), fed the same x, goal and
// sequence, on the same step counter: the batched rollout is the text of
// k_rollout_pc (the point mass) or k_rollout_auv_pc (the Fossen AUV model) with per-member operands, with the instance that handle would
// launch, and the batched finish is k_finish_cols' column_combine on the member's records over the same padded record count.
// why cfg cannot be batched (NULL: it can, as far as the config alone tells)
static const char *batch_refusal(const mppi_config *cfg)
{
    const bool auv = cfg->model_kind == MPPI_MODEL_AUV;
    switch (cfg->model_kind) {
    case MPPI_MODEL_POINT_MASS: break;
    case MPPI_MODEL_MLP: return "batched controllers: model MLP is not supported (the point-mass and Fossen AUV models only)";
    case MPPI_MODEL_AUV:
        if (!cfg->auv) return "batched controllers: model AUV needs its mppi_auv_desc (cfg.auv)";
        break;
    case MPPI_MODEL_NN_AUV: return "batched controllers: model NNAUV is not supported (the point-mass and Fossen AUV models only)";
    case MPPI_MODEL_NN_AUV_SPEED: return "batched controllers: model NNAUVSpeed is not supported (the point-mass and Fossen AUV models "
        "only)";
    default: break; // (mppi_create reports it)
    }
    switch (cfg->state_cost_kind) {
    case MPPI_STATE_COST_QUADRATIC: break;
    case MPPI_STATE_COST_ELLIPSE: return "batched controllers: the ellipse cost (ElipseCost) is not supported (the quadratic cost, and "
        "StaticQuatCost / ElipseCost3D with the Fossen AUV model)";
    case MPPI_STATE_COST_ELLIPSE3D:
        if (!auv) return "batched controllers: the ellipse cost (ElipseCost3D) is served with the Fossen AUV model only";
        break;
    case MPPI_STATE_COST_QUAT:
        if (!auv) return "batched controllers: StaticQuatCost is served with the Fossen AUV model only";
        break;
    default: break;
    }
    if (cfg->normalize_cost) return "batched controllers: normalize_cost is not supported";
    if (cfg->flags & MPPI_FLAG_FP_CONTRACT) return "batched controllers: MPPI_FLAG_FP_CONTRACT is not supported";
    if (cfg->flags & MPPI_FLAG_MLP_BF16X3) return "batched controllers: MPPI_FLAG_MLP_BF16X3 is not supported";
    if (cfg->shard_count > 1) return "batched controllers: sharding (shard_count > 1) is not supported";
    return nullptr;
}

static bool same_bits(float x, float y) { return std::memcmp(&x, &y, sizeof(float)) == 0; }
static bool same_floats(const float *x, const float *y, int n) // NULL = zeros
{
    for (int i = 0; i < n; ++i) if (!same_bits(x ? x[i] : 0.0f, y ? y[i] : 0.0f)) return false;
    return true;
}
static bool same_auv(const mppi_auv_desc *x, const mppi_auv_desc *y)
{
    if (!x || !y) return x == y;
    return same_bits(x->mass, y->mass) && same_bits(x->volume, y->volume) && same_bits(x->density, y->density) &&
           same_bits(x->gravity, y->gravity) && same_floats(x->cog, y->cog, 3) && same_floats(x->cob, y->cob, 3) &&
           same_floats(x->inertial, y->inertial, 6) && same_floats(x->added_mass, y->added_mass, 36) &&
           same_floats(x->linear_damping, y->linear_damping, 36) &&
           same_floats(x->linear_damping_forward_speed, y->linear_damping_forward_speed, 36) &&
           same_floats(x->quad_damping, y->quad_damping, 6) && x->rk == y->rk;
}

// The first field that every member must share in which b differs from a (NULL: none). What mppi_create derives the geometry, the model,
// the cost's form and the kernel picks from is shared; seed, goal, lambda, gamma, upsilon, sigma and Q are each member's own.
// learned (mppi_create_batch_learned; every member has its cfg.mlp): also the network's shape, each member's weights being its own.
static const char *batch_shared_diff(const mppi_config *a, const mppi_config *b, bool learned = false)
{
    if (learned) {
        if (a->mlp->n_layers != b->mlp->n_layers) return "mlp.n_layers";
        if (!a->mlp->widths || !b->mlp->widths) { if (a->mlp->widths != b->mlp->widths) return "mlp.widths"; }
        else for (int l = 0; l < a->mlp->n_layers && l < kMlpSmallMaxLayers; ++l) if (a->mlp->widths[l] != b->mlp->widths[l]) return "mlp.widths";
    }
    if (a->k != b->k) return "k";
    if (a->tau != b->tau) return "tau";
    if (!same_bits(a->dt, b->dt)) return "dt";
    if (!same_bits(a->mass, b->mass)) return "mass";
    if (a->s_dim != b->s_dim) return "s_dim";
    if (a->a_dim != b->a_dim) return "a_dim";
    if (a->device != b->device) return "device";
    if (a->model_kind != b->model_kind) return "model_kind";
    if (a->model_kind == MPPI_MODEL_AUV && !same_auv(a->auv, b->auv)) return "auv";
    if (a->state_cost_kind != b->state_cost_kind) return "state_cost_kind";
    if (a->state_cost_kind == MPPI_STATE_COST_QUAT && !same_floats(a->quat_Q, b->quat_Q, 100)) return "quat_Q";
    if (a->state_cost_kind == MPPI_STATE_COST_ELLIPSE3D && !same_floats(a->ellipse3d, b->ellipse3d, 11)) return "ellipse3d";
    if (a->action_cost_kind != b->action_cost_kind) return "action_cost_kind";
    if (a->flags != b->flags) return "flags";
    if (a->q_is_full != b->q_is_full) return "q_is_full";
    if (a->normalize_cost != b->normalize_cost) return "normalize_cost";
    if (a->shard_rank != b->shard_rank) return "shard_rank";
    if (a->shard_count != b->shard_count) return "shard_count";
    return nullptr;
}

// The batch of n members cfgs[0..n) (n >= 1): the handle mppi_create(&cfgs[0]) prepares, allocated for n members, member m's DevConsts
// block filled from cfgs[m] exactly as a lone handle's. name_members: what mppi_create reports for cfgs[0] names member 0
// (mppi_create_batch_configs); mppi_create_batch keeps the messages it always gave.
// why cfg cannot be a member of a learned batch (mppi_create_batch_learned; NULL: it can, as far as the config alone tells)
static const char *learned_batch_refusal(const mppi_config *cfg)
{
    switch (cfg->model_kind) {
    case MPPI_MODEL_NN_AUV: case MPPI_MODEL_NN_AUV_SPEED: break;
    case MPPI_MODEL_MLP: return "batched learned controllers: model MLP (the learned point mass) is not supported (NNAUVModel and "
        "NNAUVModelSpeed only)";
    case MPPI_MODEL_POINT_MASS: return "batched learned controllers: model POINT_MASS has no network: mppi_create_batch_configs serves it";
    case MPPI_MODEL_AUV: return "batched learned controllers: model AUV has no network: mppi_create_batch_configs serves it";
    default: return nullptr; // (mppi_create reports it)
    }
    if (cfg->normalize_cost) return "batched learned controllers: normalize_cost is not supported";
    if (cfg->flags & MPPI_FLAG_MLP_BF16X3) return "batched learned controllers: MPPI_FLAG_MLP_BF16X3 is not supported";
    if (cfg->flags & MPPI_FLAG_FP_CONTRACT) return "batched learned controllers: MPPI_FLAG_FP_CONTRACT is not supported";
    if (cfg->shard_count > 1) return "batched learned controllers: sharding (shard_count > 1) is not supported";
    return nullptr;
}

// why cfg cannot be a member of a batch of learned point masses (mppi_create_batch_mlp; NULL: it can, as far as the config alone tells)
static const char *mlp_batch_refusal(const mppi_config *cfg)
{
    switch (cfg->model_kind) {
    case MPPI_MODEL_MLP: break;
    case MPPI_MODEL_POINT_MASS: return "batched MLP controllers: model POINT_MASS has no network: mppi_create_batch_configs serves it";
    case MPPI_MODEL_AUV: return "batched MLP controllers: model AUV has no network: mppi_create_batch_configs serves it";
    case MPPI_MODEL_NN_AUV: return "batched MLP controllers: model NNAUV is a 13-state model: mppi_create_batch_learned serves it";
    case MPPI_MODEL_NN_AUV_SPEED: return "batched MLP controllers: model NNAUVSpeed is a 13-state model: mppi_create_batch_learned serves it";
    default: return nullptr; // (mppi_create reports it)
    }
    if (cfg->normalize_cost) return "batched MLP controllers: normalize_cost is not supported";
    if (cfg->flags & MPPI_FLAG_MLP_BF16X3) return "batched MLP controllers: MPPI_FLAG_MLP_BF16X3 is not supported";
    if (cfg->flags & MPPI_FLAG_FP_CONTRACT) return "batched MLP controllers: MPPI_FLAG_FP_CONTRACT is not supported";
    if (cfg->shard_count > 1) return "batched MLP controllers: sharding (shard_count > 1) is not supported";
    if (cfg->state_cost_kind != MPPI_STATE_COST_QUADRATIC) return "batched MLP controllers: the quadratic state cost only (state_cost_kind)";
    if (cfg->q_is_full) return "batched MLP controllers: a dense Q (q_is_full) is not supported (the MLP rollouts take a diagonal Q)";
    return nullptr;
}

// learned = 1: mppi_create_batch_learned's batch — the learned 13-state models, member m with its own network cfgs[m].mlp;
// learned = 2: mppi_create_batch_mlp's — the learned point mass, likewise
static mppi_status create_batch(const mppi_config *cfgs, int n, bool name_members, mppi_handle **out, int learned = 0)
{
    for (int m = 0; m < n; ++m)
        if (cfgs[m].struct_size != sizeof(mppi_config)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
            "mppi_config.struct_size mismatch (use mppi_config_init)");
    if (learned) {
        if (const char *why = learned == 2 ? mlp_batch_refusal(&cfgs[0]) : learned_batch_refusal(&cfgs[0]))
            return fail(nullptr, MPPI_ERR_UNSUPPORTED, why);
        for (int m = 0; m < n; ++m) {
            const mppi_mlp_desc *d = cfgs[m].mlp;
            const std::string who = std::string(learned == 2 ? "batched MLP controllers: member " : "batched learned controllers: member ") +
                std::to_string(m) + ": ";
            if (!d) return fail(nullptr, MPPI_ERR_INVALID_ARG, who + "cfg.mlp is NULL (every member brings its own network)");
            if (!d->widths || !d->W || !d->b) return fail(nullptr, MPPI_ERR_INVALID_ARG, who + "cfg.mlp needs widths, W, b");
            for (int l = 0; l < d->n_layers && l < kMlpSmallMaxLayers; ++l)
                if (!d->W[l] || !d->b[l]) return fail(nullptr, MPPI_ERR_INVALID_ARG, who + "NULL MLP weight pointer");
        }
    }
    for (int m = 1; m < n; ++m)
        if (const char *f = batch_shared_diff(&cfgs[0], &cfgs[m], learned != 0))
            return fail(nullptr, MPPI_ERR_INVALID_ARG, "batched controllers: cfgs[" + std::to_string(m) + "]." + f +
                " differs from cfgs[0]." + f + " (every member shares it)");
    const mppi_config *cfg = &cfgs[0];
    if (!learned) if (const char *why = batch_refusal(cfg)) return fail(nullptr, MPPI_ERR_UNSUPPORTED, why);
    mppi_handle *h = nullptr;
    if (mppi_status st = prepare_handle(cfg, name_members, &h); st != MPPI_OK) return st;
    auto refuse = [&](mppi_status st, const std::string &why) { mppi_destroy(h); return fail(nullptr, st, why); };
    if (!learned && !h->is_gen && !pc_eligible(h)) return refuse(MPPI_ERR_UNSUPPORTED,
        "batched controllers: the producer/consumer rollout serves this shape only with s_dim = 2 a_dim, a_dim <= 4, tau <= 160 (<= 132 "
        "above 512 tiles)");
    if (!learned && h->is_gen && !auv_batch_eligible(h)) return refuse(MPPI_ERR_UNSUPPORTED,
        "batched controllers: the Fossen AUV model is batched on its two-wave rollout (k_rollout_auv_pc) only");
    if (learned == 2 && !h->mlp_small && !h->mlp_v2) return refuse(MPPI_ERR_UNSUPPORTED,
        "batched MLP controllers: the {256, 256} network at a_dim = 4 is not supported (the lone handle runs k_rollout_mlp there, which this "
        "batch does not carry; a_dim <= 3)");
    if (learned == 2 && !h->no_rollout.empty()) return refuse(MPPI_ERR_UNSUPPORTED, "batched MLP controllers: " + h->no_rollout);
    if (learned == 2 && n > 65535) return refuse(MPPI_ERR_INVALID_ARG, "batched MLP controllers: at most 65535 members");
    if (h->nbp > 1024) return refuse(MPPI_ERR_UNSUPPORTED,
        "batched controllers: at most 1024 tiles (k = 65536) per member (the finish combines a member's records in one pass)");
    if ((long long)h->nb * n > (1ll << 30) / 64) return refuse(MPPI_ERR_INVALID_ARG, "batched controllers: n * k too large");
    // every member's constants; all members must run the instance member 0's lone handle picks
    std::vector<DevConsts> consts(n);
    consts[0] = h->hc;
    for (int m = 1; m < n; ++m)
        if (mppi_status st = member_consts(&cfgs[m], m, true, h, consts[m], learned == 2 ? MPPI_ERR_INVALID_ARG : MPPI_ERR_UNSUPPORTED);
            st != MPPI_OK) { mppi_destroy(h); return st; }
    h->batch = n;
    h->nn_batch = learned;
    h->fuse_step = 0; // the two launches, always
    mppi_status st = allocate_handle(h, cfg, n, consts.data());
    for (int m = 1; learned && st == MPPI_OK && m < n; ++m) st = upload_mlp(h, cfgs[m].mlp, false, m);
    if (st != MPPI_OK) { g_create_err = h->err; mppi_destroy(h); return st; }
    *out = h;
    return MPPI_OK;
}

// ---- batched learned-model controllers (include/mppi_c.h; the kernel: mppi_nn_batch.hip.h) -------------------------------------------
extern "C" mppi_status mppi_create_batch_learned(const mppi_config *cfgs, int n, mppi_handle **out)
{
    if (!cfgs || !out) return fail(nullptr, MPPI_ERR_INVALID_ARG, "cfgs/out is NULL");
    *out = nullptr;
    if (n < 1) return fail(nullptr, MPPI_ERR_INVALID_ARG, "batched controllers: n must be >= 1");
    return create_batch(cfgs, n, true, out, 1);
}

// ---- batched learned point-mass controllers (include/mppi_c.h; the kernels: mppi_mlp_batch.hip.h) -------------------------------------
extern "C" mppi_status mppi_create_batch_mlp(const mppi_config *cfgs, int n, mppi_handle **out)
{
    if (!cfgs || !out) return fail(nullptr, MPPI_ERR_INVALID_ARG, "cfgs/out is NULL");
    *out = nullptr;
    if (n < 1) return fail(nullptr, MPPI_ERR_INVALID_ARG, "batched controllers: n must be >= 1");
    return create_batch(cfgs, n, true, out, 2);
}

extern "C" mppi_status mppi_batch_set_mlp(mppi_handle *h, int member, const mppi_mlp_desc *d)
{
    MPPI_BATCH_ONLY(h);
    if (!h->nn_batch) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_batch_set_mlp: not a batch of learned controllers (mppi_create_batch_learned / mppi_create_batch_mlp)");
    if (member < -1 || member >= h->batch) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_batch_set_mlp: member out of range");
    if (!d || !d->widths || !d->W || !d->b) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_batch_set_mlp needs widths, W, b");
    if (d->n_layers != h->hm.n_layers) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_batch_set_mlp: the layer count is fixed at creation");
    for (int l = 0; l < d->n_layers; ++l) {
        if (d->widths[l] != h->hm.widths[l]) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_batch_set_mlp: the layer widths are fixed at creation");
        if (!d->W[l] || !d->b[l]) return fail(h, MPPI_ERR_INVALID_ARG, "NULL MLP weight pointer");
    }
    MPPI_ENTER(h);
    HIP_TRY(h, hipDeviceSynchronize()); // steps in flight, on any stream, read the old weights (mppi_set_mlp)
    for (int m = member < 0 ? 0 : member; m < (member < 0 ? h->batch : member + 1); ++m)
        if (mppi_status st = upload_mlp(h, d, false, m); st != MPPI_OK) return st;
    return MPPI_OK;
}

extern "C" mppi_status mppi_create_batch_configs(const mppi_config *cfgs, int n, mppi_handle **out)
{
    if (!cfgs || !out) return fail(nullptr, MPPI_ERR_INVALID_ARG, "cfgs/out is NULL");
    *out = nullptr;
    if (n < 1) return fail(nullptr, MPPI_ERR_INVALID_ARG, "batched controllers: n must be >= 1");
    return create_batch(cfgs, n, true, out);
}

// n copies of cfg that differ in the seed
extern "C" mppi_status mppi_create_batch(const mppi_config *cfg, int n, const uint64_t *seeds, mppi_handle **out)
{
    if (!cfg || !out) return fail(nullptr, MPPI_ERR_INVALID_ARG, "cfg/out is NULL");
    *out = nullptr;
    if (n < 1) return fail(nullptr, MPPI_ERR_INVALID_ARG, "batched controllers: n must be >= 1");
    if (cfg->struct_size != sizeof(mppi_config)) return fail(nullptr, MPPI_ERR_INVALID_ARG,
        "mppi_config.struct_size mismatch (use mppi_config_init)");
    std::vector<mppi_config> cfgs;
    try {
        cfgs.assign((size_t)n, *cfg);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, MPPI_ERR_ALLOC, "out of host memory");
    }
    for (int m = 0; m < n; ++m) cfgs[m].seed = seeds ? seeds[m] : cfg->seed + (unsigned long long)m;
    return create_batch(cfgs.data(), n, false, out);
}
