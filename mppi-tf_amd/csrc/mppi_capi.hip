// mppi_capi.hip — host side of libmppi_hip.so: the C-ABI of include/mppi_c.h over the kernels
// of mppi_kernels.hip.h.  No CPU compute path exists here: every numeric entry point launches
// HIP kernels and fails with MPPI_ERR_NO_DEVICE / MPPI_ERR_HIP when it cannot.

#include <algorithm>
#include <chrono>
#include <dlfcn.h>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MPPI_VERSION_STRING "mppi-hip 0.1.0 (gfx950)"

#define MPPI_UNIT_CAPI 1
#include "mppi_handle.hip.h"
#include "mppi_step.hip.h"

#include <map>
#include <mutex>

static thread_local std::string g_create_err;

static mppi_status fail(mppi_handle *h, mppi_status st, const std::string &msg)
{
    if (h) h->err = msg; else g_create_err = msg;
    return st;
}

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e == hipErrorNotSupported && (h) && !((mppi_handle *)(h))->no_rollout.empty())       \
            return fail((h), MPPI_ERR_UNSUPPORTED, ((mppi_handle *)(h))->no_rollout);             \
        if (_e != hipSuccess)                                                                     \
            return fail((h), MPPI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)


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

// ---- roctx ranges (MPPI_TUNE_TRACE): the reference brackets its step with tf.profiler.experimental.start/stop
// (controller_base.py:241-248, 587-595). The marker library is dlopen'ed on first use — rocprofiler-sdk's (what rocprofv3
// --marker-trace records) first, the legacy libroctx64 second — so the product keeps no link dependency on a profiler.
namespace {
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false;
    bool load()
    {
        if (tried) return push != nullptr;
        tried = true;
        for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            void *lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (!lib) continue;
            push = reinterpret_cast<int (*)(const char *)>(dlsym(lib, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
            if (push && pop) return true;
            push = nullptr; pop = nullptr;
        }
        return false;
    }
} g_roctx;
// a range that lasts for the scope; free when the handle does not trace
struct TraceRange {
    bool on;
    TraceRange(const mppi_handle *h, const char *name) : on(h->trace && g_roctx.push) { if (on) g_roctx.push(name); }
    ~TraceRange() { if (on) g_roctx.pop(); }
};
} // namespace

// ---- armed launches (mppi_step.hip.h) ---------------------------------------------------------------------------------
// The host stores into fine-grained device memory directly (large BAR); the stores of one call are fenced out of the write-combining
// buffers before anything waits on their effect.
static inline void store_fence()
{
#if defined(__x86_64__)
    __builtin_ia32_sfence();
#else
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}
static inline void xslot_store(mppi_handle *h, int i, float v, unsigned tag)
{
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    __atomic_store_n(reinterpret_cast<volatile unsigned long long *>(h->d_xslot) + i, ((unsigned long long)tag << 32) | (unsigned long long)bits, __ATOMIC_RELAXED);
}
// An armed launch nobody is going to feed (any entry point other than mppi_next, a handle that changes, destroy): the host's cancel
// tag makes tile 0 abort at its next poll; every wave follows, the update is not applied, the stream drains. U, u and the Philox step
// counter are exactly what they were before the launch was armed.
// ... and the pre-launched pipeline (MPPI_TUNE_PRELAUNCH): steps are in flight on both streams; once both have drained, the plain U buffers,
// the step counter and u are what the plain path would have left. A sequence that never came (hard deadline) is in the sticky error word.
static hipError_t pre_quiesce(mppi_handle *h)
{
    if (!h->pre_active) return hipSuccess;
    h->pre_active = false;
    if (hipError_t e = hipStreamSynchronize(h->stream); e != hipSuccess) return e;
    if (hipError_t e = hipStreamSynchronize(h->stream2); e != hipSuccess) return e;
    if (h->h_arm && reinterpret_cast<volatile unsigned *>(h->h_arm + 1)[0] != 0u) {
        reinterpret_cast<volatile unsigned *>(h->h_arm + 1)[0] = 0u;
        h->err = "a pre-launched step never received its sequence (hard deadline): the controls since are invalid";
        return hipErrorLaunchTimeOut;
    }
    return hipSuccess;
}
static hipError_t quiesce(mppi_handle *h)
{
    if (hipError_t e = pre_quiesce(h); e != hipSuccess) return e;
    if (!h->arm_inflight) return hipSuccess;
    xslot_store(h, 0, 0.0f, h->arm_seq | mppi::kArmCancelBit);
    store_fence();
    h->arm_inflight = false;
    return hipStreamSynchronize(h->stream);
}
// every entry point that touches the device or the handle's stream: make the device current, retire an armed launch
#define MPPI_ENTER(h)                                \
    do {                                             \
        HIP_TRY(h, hipSetDevice((h)->device));       \
        HIP_TRY(h, quiesce(h));                      \
    } while (0)

// a batched handle (mppi_create_batch) has no single x, goal or sequence: the per-member entry points refuse it (mppi_batch_* serve it)
#define MPPI_NOT_BATCH(h, name)                                                                                                       \
    do {                                                                                                                              \
        if ((h) && (h)->batch) return fail((h), MPPI_ERR_UNSUPPORTED, std::string(name) + ": a batched handle steps through mppi_batch_*"); \
    } while (0)

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

static mppi_status upload_consts(mppi_handle *h)
{
    HIP_TRY(h, hipMemcpyAsync(h->dC, &h->hc, sizeof(DevConsts), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
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
    for (float *p : {h->d_bx, h->d_bu, h->d_ep}) if (p) (void)hipFree(p);
    if (h->dM) (void)hipFree(h->dM);
    if (h->d_mlp_w) (void)hipFree(h->d_mlp_w);
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
static mppi_status upload_mlp(mppi_handle *h, const mppi_mlp_desc *d, bool allocate)
{
    const int s = h->s, a = h->a;
    const bool speed = h->hc.model_kind == MPPI_MODEL_NN_AUV_SPEED;
    const bool nnauv = h->hc.model_kind == MPPI_MODEL_NN_AUV || speed;
    // NNAUVModel.prepare_data drops the position (nn_model.py:289-293); NNAUVModelSpeed's takes Euler angles, velocities, forces (:438-461)
    const int nin = speed ? 15 : (nnauv ? s + a - 3 : s + a), nout = speed ? 6 : s;
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
            for (int i = 0; i < w_in; ++i) for (int o = 0; o < d->widths[l]; ++o) padded[(size_t)i * ld + o] = d->W[l][(size_t)i * d->widths[l] + o];
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

// ---- creation: validate the config, derive the handle's geometry, fill every member's constants, allocate ---------------------------------
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
    if (cfg->model_kind == MPPI_MODEL_POINT_MASS && !(cfg->mass != 0.0f)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "mass must be non-zero");
    if (cfg->model_kind < MPPI_MODEL_POINT_MASS || cfg->model_kind > MPPI_MODEL_NN_AUV_SPEED)
        return fail(nullptr, MPPI_ERR_INVALID_ARG, "unknown model kind");
    if (cfg->state_cost_kind < MPPI_STATE_COST_QUADRATIC || cfg->state_cost_kind > MPPI_STATE_COST_ELLIPSE3D)
        return fail(nullptr, MPPI_ERR_INVALID_ARG, "unknown state cost kind");
    // the 13-state AUV family (mppi_gen.hip.h): pose with a quaternion + body velocities, 6 generalised forces
    const bool nn_speed = cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED;
    const bool gen = cfg->model_kind == MPPI_MODEL_AUV || cfg->model_kind == MPPI_MODEL_NN_AUV || nn_speed;
    const bool cost13 = cfg->state_cost_kind == MPPI_STATE_COST_QUAT || cfg->state_cost_kind == MPPI_STATE_COST_ELLIPSE3D;
    if (gen && (s != 13 || a != 6)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "AUVModel / NNAUVModel: s_dim = 13 (pos, quat, lin vel, ang vel), a_dim = 6");
    if (cost13 && s != 13) return fail(nullptr, MPPI_ERR_INVALID_ARG, "StaticQuatCost / ElipseCost3D read a 13-state (static_cost.py:141-159, elipse_cost.py:124-139)");
    if (cost13 && !gen && cfg->k * (long long)cfg->tau > 1) return fail(nullptr, MPPI_ERR_UNSUPPORTED, "StaticQuatCost / ElipseCost3D rollouts need a 13-state model (MPPI_MODEL_AUV / MPPI_MODEL_NN_AUV)");
    if (cfg->model_kind == MPPI_MODEL_NN_AUV || nn_speed) {
        const mppi_mlp_desc *d = cfg->mlp;
        if (!d || !d->widths || !d->W || !d->b) return fail(nullptr, MPPI_ERR_INVALID_ARG, "NNAUVModel needs cfg.mlp with widths, W, b");
        if (d->n_layers < 2 || d->n_layers > kMlpSmallMaxLayers) return fail(nullptr, MPPI_ERR_UNSUPPORTED, "NNAUVModel: 2 to 4 Dense layers (1 to 3 hidden + the output layer)");
        for (int l = 0; l < d->n_layers; ++l) if (!d->W[l] || !d->b[l]) return fail(nullptr, MPPI_ERR_INVALID_ARG, "NULL MLP weight pointer");
        if (!nn_speed && d->widths[d->n_layers - 1] != 13) return fail(nullptr, MPPI_ERR_INVALID_ARG, "NNAUVModel: the last layer's width must be 13 (nn_model.py:59)");
        if (nn_speed && d->widths[d->n_layers - 1] != 6) return fail(nullptr, MPPI_ERR_INVALID_ARG, "NNAUVModelSpeed: the last layer's width must be 6, the velocity delta (nn_model.py:345)");
        if (nn_speed && (cfg->flags & MPPI_FLAG_MLP_BF16X3)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "MPPI_FLAG_MLP_BF16X3: no split-bf16 kernel for NNAUVModelSpeed");
        const int hid = d->widths[0];
        bool same = hid == 16 || hid == 32;
        for (int l = 0; l + 1 < d->n_layers; ++l) same = same && d->widths[l] == hid;
        if (!same) return fail(nullptr, MPPI_ERR_UNSUPPORTED, "NNAUVModel kernels exist for 1-3 equal hidden layers of 16 or 32 (nn_model.py:54-60)");
        if (hid != 32 && (cfg->flags & MPPI_FLAG_MLP_BF16X3)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "MPPI_FLAG_MLP_BF16X3 applies to the 256-wide and the 32-wide networks");
    }
    if (cfg->state_cost_kind == MPPI_STATE_COST_ELLIPSE) {
        if (!cfg->ellipse) return fail(nullptr, MPPI_ERR_INVALID_ARG, "the elliptic cost needs cfg.ellipse[7]");
        if (s < 4) return fail(nullptr, MPPI_ERR_INVALID_ARG, "the elliptic cost reads (x, vx, y, vy): s_dim >= 4");
        if (!(cfg->ellipse[0] != 0.0f) || !(cfg->ellipse[1] != 0.0f)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "ellipse axes a, b must be non-zero");
        if (cfg->model_kind == MPPI_MODEL_MLP) return fail(nullptr, MPPI_ERR_UNSUPPORTED, "MLP rollouts are instantiated for the quadratic state cost");
    }
    if (cfg->model_kind == MPPI_MODEL_MLP) {
        const mppi_mlp_desc *d = cfg->mlp;
        if (!d || !d->widths || !d->W || !d->b) return fail(nullptr, MPPI_ERR_INVALID_ARG, "MLP model needs cfg.mlp with widths, W, b");
        if (d->n_layers < 2 || d->n_layers > kMlpSmallMaxLayers) return fail(nullptr, MPPI_ERR_UNSUPPORTED, "MLP: 2 to 4 Dense layers (1 to 3 hidden + the output layer)");
        for (int l = 0; l < d->n_layers; ++l) if (!d->W[l] || !d->b[l]) return fail(nullptr, MPPI_ERR_INVALID_ARG, "NULL MLP weight pointer");
        if (d->widths[d->n_layers - 1] != s) return fail(nullptr, MPPI_ERR_INVALID_ARG, "MLP: the last layer's width must be s_dim");
        const int hid = d->widths[0];
        bool same = true;
        for (int l = 0; l + 1 < d->n_layers; ++l) same = same && d->widths[l] == hid;
        const bool big = d->n_layers == 3 && same && hid == kHid, small = same && (hid == 16 || hid == 32);
        if (!big && !small)
            return fail(nullptr, MPPI_ERR_UNSUPPORTED, "MLP kernels exist for hidden widths {256,256} (matrix cores) and 1-3 equal hidden layers of 16 or 32 (nn_model.py:54-60)");
        if (small && hid != 32 && (cfg->flags & MPPI_FLAG_MLP_BF16X3))
            return fail(nullptr, MPPI_ERR_INVALID_ARG, "MPPI_FLAG_MLP_BF16X3 applies to the 256-wide and the 32-wide networks");
        if (s != 2 * a || a > 4) return fail(nullptr, MPPI_ERR_UNSUPPORTED, "MLP rollouts are instantiated for s_dim == 2*a_dim, a_dim <= 4");
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
    const bool gen = cfg->model_kind == MPPI_MODEL_AUV || cfg->model_kind == MPPI_MODEL_NN_AUV || cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED;
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
    h->mlp_bx3 = ((cfg->model_kind == MPPI_MODEL_MLP || cfg->model_kind == MPPI_MODEL_NN_AUV) && (cfg->flags & MPPI_FLAG_MLP_BF16X3)) ? 1 : 0;
    h->fp_contract = (cfg->model_kind == MPPI_MODEL_POINT_MASS && (cfg->flags & MPPI_FLAG_FP_CONTRACT)) ? 1 : 0;
    h->mlp_small = ((cfg->model_kind == MPPI_MODEL_MLP && cfg->mlp->widths[0] != kHid) || cfg->model_kind == MPPI_MODEL_NN_AUV ||
                    cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED) ? cfg->mlp->widths[0] : 0;
    h->is_gen = gen ? 1 : 0;
    h->mlp_v2 = (cfg->model_kind == MPPI_MODEL_MLP && !h->mlp_small && !h->mlp_bx3 && a <= 3) ? 1 : 0; // a_dim = 4: two h1 images + the rest exceed 160 KiB of LDS
    h->nb_mlp = cfg->model_kind == MPPI_MODEL_MLP ? (h->mlp_v2 ? (h->K_local + kMlp2R - 1) / kMlp2R : (h->K_local + kMlpR - 1) / kMlpR) : 0;
    h->nbp = record_pad(std::max(h->nb, h->nb_mlp));
    *out = h;
    return MPPI_OK;
}

// Member m's constants from its config, the one validation of a member: its temperature, its Sigma, and that it runs the kernel instance
// member 0 picked (sigma_diag, the effective Q form; member 0 is filled into h->hc and sets both). A failure is g_create_err, naming the member if `named`.
static mppi_status member_consts(const mppi_config *cfg, int m, bool named, mppi_handle *h, DevConsts &c)
{
    const std::string who = named ? "batched controllers: member " + std::to_string(m) + ": " : "";
    if (!temperature_ok(cfg)) return fail(nullptr, MPPI_ERR_INVALID_ARG, who + kBadTemperature);
    int diag = 0;
    if (!fill_consts(cfg, h, c, diag)) return fail(nullptr, MPPI_ERR_SINGULAR_SIGMA, who + "sigma is singular");
    if (m == 0) { h->sigma_diag = diag; return MPPI_OK; } // (c is h->hc: member 0 sets what the others are compared with)
    if (diag != h->sigma_diag)
        return fail(nullptr, MPPI_ERR_UNSUPPORTED, "batched controllers: sigma must be diagonal for every member or dense for every member (member " + std::to_string(m) + " differs from member 0)");
    if (c.q_full != h->hc.q_full)
        return fail(nullptr, MPPI_ERR_UNSUPPORTED, "batched controllers: Q must be diagonal for every member or dense for every member (member " + std::to_string(m) +
                                                       " differs from member 0; a dense Q without off-diagonal entries counts as diagonal)");
    return MPPI_OK;
}

// Everything mppi_create reports for cfg before it allocates: the config, the geometry, member 0's constants (h->hc), the 13-state constants.
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
    for (int m = 0; m < B; ++m)
        hipLaunchKernelGGL(k_fill_records, dim3((unsigned)((rec + 255) / 256)), dim3(256), 0, h->stream, h->d_part + rec * m, nrec, 2 + h->HA);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream)); // steps may be enqueued on the caller's stream
    const int nrec2 = (nrec + kGroup - 1) / kGroup, nrec3 = (nrec2 + kGroup - 1) / kGroup;
    HIP_TRY(h, hipMalloc((void **)&h->d_part2, sizeof(float) * (size_t)nrec2 * (2 + h->HA)));
    HIP_TRY(h, hipMalloc((void **)&h->d_part3, sizeof(float) * (size_t)nrec3 * (2 + h->HA)));
    if (cfg->model_kind == MPPI_MODEL_MLP || cfg->model_kind == MPPI_MODEL_NN_AUV || cfg->model_kind == MPPI_MODEL_NN_AUV_SPEED) {
        if (mppi_status st_ = upload_mlp(h, cfg->mlp, true); st_ != MPPI_OK) return st_;
    }
    HIP_TRY(h, hipMalloc((void **)&h->d_record, sizeof(float) * (2 + h->HA)));
    HIP_TRY(h, hipMalloc((void **)&h->d_dbg, sizeof(float) * 8 * B));
    HIP_TRY(h, hipMalloc((void **)&h->d_mm, sizeof(float) * 4));
    if (h->normalize) HIP_TRY(h, hipMalloc((void **)&h->d_tile_mm, sizeof(float) * 2 * (size_t)nrec));
    HIP_TRY(h, hipMalloc((void **)&h->d_step, sizeof(unsigned long long)));
    if (h->shard_count > 1) { // mppi_shard_step's buffers: allocated here, not inside the enqueue-only step (an allocation there is an implicit device sync)
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
        if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, h->device) != hipSuccess) { large_bar = 0; (void)hipGetLastError(); }
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
    if (cfg->struct_size != sizeof(mppi_config)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_config.struct_size mismatch (use mppi_config_init)");
    mppi_handle *h = nullptr;
    if (mppi_status st = prepare_handle(cfg, false, &h); st != MPPI_OK) return st;
    if (mppi_status st = allocate_handle(h, cfg, 1, &h->hc); st != MPPI_OK) { g_create_err = h->err; mppi_destroy(h); return st; }
    *out = h;
    return MPPI_OK;
}

// kernel dispatch: the rollout kernels are instantiated in their own translation units (mppi_launch_*.hip, one per
// kernel family and action dimension, compiled in parallel); mppi_handle.hip.h declares their entry points, one row per action dimension.
#define MPPI_UNIT_ROW(N)                                                                                                  \
    {mppi_tile_a##N, mppi_pc_a##N, mppi_mlp_a##N, mppi_step_a##N, mppi_batch_a##N, mppi_batch_finish_a##N, mppi_tile_name_a##N, \
     mppi_pc_name_a##N, mppi_mlp_name_a##N, mppi_step_name_a##N, mppi_batch_name_a##N}
static const mppi_unit_a kUnits[4] = {MPPI_UNIT_ROW(1), MPPI_UNIT_ROW(2), MPPI_UNIT_ROW(3), MPPI_UNIT_ROW(4)};
#undef MPPI_UNIT_ROW
static const mppi_unit_a *unit(const mppi_handle *h) { return h->a >= 1 && h->a <= 4 ? &kUnits[h->a - 1] : nullptr; }

// the entry point `fn` of the handle's action dimension (none above 4: such a handle runs no rollout kernel)
template <typename... P, typename... Args>
static hipError_t per_a(mppi_handle *h, hipError_t (*mppi_unit_a::*fn)(P...), Args... args)
{
    const mppi_unit_a *u = unit(h);
    return u ? (u->*fn)(h, args...) : hipErrorInvalidValue;
}

static hipError_t launch_tile(mppi_handle *h, const DevConsts *consts, hipStream_t st, int src, int mode, const float *x_dev, const float *U_dev,
                              const float *eps, float *cost, float *part, float *noise_out)
{
    if (!h->no_rollout.empty()) return hipErrorNotSupported;
    return per_a(h, &mppi_unit_a::tile, consts, st, src, mode, x_dev, U_dev, eps, cost, part, noise_out);
}

// the point-mass model with the quadratic (diagonal or dense Q) or the elliptic state cost; horizon groups per producer must fit the registers
static bool pc_eligible(const mppi_handle *h)
{
    const bool cost_ok = h->hc.state_cost_kind == MPPI_STATE_COST_QUADRATIC || (h->hc.state_cost_kind == MPPI_STATE_COST_ELLIPSE && h->s >= 4 && !h->hc.q_full);
    return !h->is_gen && h->no_rollout.empty() && h->R == 64 && !h->force_tile && h->H <= (h->pc_np == 3 ? 132 : 160) && cost_ok;
}

// What k_step_pc (mppi_step.hip.h) serves: the producer/consumer path's hot shape — point mass, diagonal quadratic cost, the step's
// one pass (no normalizeCost), no sequence filter behind the update, one shard.
static bool step_shape_ok(const mppi_handle *h)
{
    return pc_eligible(h) && h->hc.state_cost_kind == MPPI_STATE_COST_QUADRATIC && !h->hc.q_full && !h->normalize && h->shard_count == 1 &&
           h->sg_window == 0 && h->d_decision != nullptr && !h->fp_contract;
}
// the whole step in ONE launch: at most 128 tiles (K <= 8192), the 6-wave workgroup
static bool fuse_ok(const mppi_handle *h) { return h->fuse_step && step_shape_ok(h) && h->nb <= 128 && h->pc_np == 5 && h->d_step_recs != nullptr; }
// mppi_next may arm the next step (MPPI_TUNE_ARMED_US > 0, a large-BAR system)
static bool arm_ok(const mppi_handle *h) { return h->arm_us > 0 && step_shape_ok(h) && h->d_xslot != nullptr; }

// Which kernel family serves the rollout launch a profiled step brackets (ev[0] .. ev[1], mppi_c.h): the batched rollout; the fused
// k_step_pc (whole_step: the caller runs a complete control step, which may be one launch); k_rollout_pc (with normalizeCost its
// weights-only second pass); the learned-model or 13-state kernels; else the tile kernel (with normalizeCost, these three run the cost-only pass).
enum Route { ROUTE_BATCH, ROUTE_STEP, ROUTE_PC, ROUTE_TILE, ROUTE_MLP, ROUTE_GEN };
static Route rollout_route(const mppi_handle *h, int src, const float *noise_out, bool whole_step)
{
    const bool philox = src == SRC_PHILOX && noise_out == nullptr;
    if (h->batch) return ROUTE_BATCH;
    if (whole_step && philox && fuse_ok(h)) return ROUTE_STEP;
    if (h->is_gen) return ROUTE_GEN;
    if (h->hc.model_kind == MPPI_MODEL_MLP) return ROUTE_MLP;
    return philox && pc_eligible(h) ? ROUTE_PC : ROUTE_TILE;
}

// ---- the profiling slot: the one place that knows where a profiled step's events are. The slot index stays on the handle (a sharded step
// spans two C calls: mppi_shard_partial* writes the rollout events of slot prof_n, mppi_shard_finish commits it); the events of the
// launch at hand are handed to it as an argument (mppi_kev).
struct ProfSlot { // the events of the step being enqueued, or none: it is not profiled
    mppi_kev rollout, finish;
    explicit operator bool() const { return rollout.begin != nullptr; }
};
static ProfSlot prof_slot(mppi_handle *h)
{
    if (h->prof_n >= h->prof_cap) return {};
    hipEvent_t *ev = &h->ev[4 * h->prof_n];
    return {{ev[0], ev[1]}, {ev[2], ev[3]}};
}
static void prof_commit(mppi_handle *h, hipStream_t st) { h->prof_stream = st; h->prof_n++; }
// a profiled step that is one launch has no finish launch: an empty finish interval, and the step is recorded
static hipError_t prof_one_launch(mppi_handle *h, ProfSlot p, hipStream_t st)
{
    if (!p) return hipSuccess;
    if (hipError_t e = hipEventRecord(p.finish.begin, st); e != hipSuccess) return e;
    if (hipError_t e = hipEventRecord(p.finish.end, st); e != hipSuccess) return e;
    prof_commit(h, st);
    return hipSuccess;
}

// One rollout launch on `route`, through the 13-state, learned-model, producer/consumer or tile launcher, on the handle's own sequence,
// records and constants. kev: the profiled step's rollout events or none — the dispatch's own begin / end, except that the tile kernel
// takes none and gets them recorded around its launch (`around`: so does any route). pass, range_given: k_rollout_pc's (MPPI_PC_PARAMS).
static hipError_t launch_rollout(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, int mode, const float *x_dev, const float *eps,
                                 float *cost, float *noise_out, int pass = PC_PASS_PLAIN, bool range_given = false, bool around = false)
{
    const bool record = kev.begin && (around || route == ROUTE_TILE);
    const mppi_kev own = record ? mppi_kev{} : kev;
    hipError_t e = record ? hipEventRecord(kev.begin, st) : hipSuccess;
    if (e != hipSuccess) return e;
    switch (route) {
    case ROUTE_GEN: e = mppi_launch_gen(h, h->dC, st, own, src, mode, x_dev, h->U_cur(), eps, cost, h->d_part, noise_out); break;
    case ROUTE_MLP: e = per_a(h, &mppi_unit_a::mlp, st, own, src, mode, x_dev, (const float *)h->U_cur(), eps, cost); break;
    case ROUTE_PC: e = per_a(h, &mppi_unit_a::pc, st, own, x_dev, pass, range_given); break;
    case ROUTE_TILE: e = launch_tile(h, h->dC, st, src, mode, x_dev, h->U_cur(), eps, cost, h->d_part, noise_out); break;
    default: e = hipErrorInvalidValue;
    }
    // records were made: from the raw costs at the range's temperature (the weights-only pass of normalizeCost), else at lambda
    if (mode == MODE_ROLLOUT || mode == MODE_COSTS_GIVEN) h->norm_two_pass = route == ROUTE_PC && pass == PC_PASS_WEIGHTS;
    if (e == hipSuccess && record) e = hipEventRecord(kev.end, st);
    return e;
}

// What launch_finish combines and writes: n records (element (b, col) at recs[b*sb + col*sc]) and, if apply, the update:
// U' = U_in + V/eta -> U_out, u_out = U'[0].
struct Finish {
    const float *recs = nullptr;
    int sb = 1, sc = 0, n = 0;
    const float *nil_dev = nullptr; // the temperature the records were made at where it is not lambda (d_mm + 2: the weights-only pass of normalizeCost); whoever made the records fills it in
    const float *U_in = nullptr;
    float *U_out = nullptr, *u_out = nullptr, *record_out = nullptr;
    int apply = 1;
    bool xchg = false;      // the finish that exchanges the records with the peers' inboxes first (mppi_shard_p2p_step)
    unsigned armed_seq = 0; // of an armed launch: the finish obeys tile 0's verdict on it
    FinishPre pre = FinishPre{nullptr, nullptr, 0u, 0ull};
};
// the common case: the handle's own d_part (every slot: those no tile owns hold neutral records) onto its own sequence
static Finish own_records(const mppi_handle *h) { return Finish{h->d_part, 1, h->nbp, h->nbp, nullptr, h->U_cur(), h->U_other()}; }

// More than 1024 records are first folded 16:1 (k_combine_group) into row-major scratch.
static hipError_t launch_finish(mppi_handle *h, hipStream_t st, Finish f)
{
    // a profiled step = the rollout kernel + the finish that applies the update
    TraceRange tr(h, f.apply ? "mppi:finish" : "mppi:record");
    const ProfSlot p = f.apply ? prof_slot(h) : ProfSlot{};
    // The levels alternate between the two scratch buffers, so that no level reads the buffer it writes: level 1 fills d_part2
    // (ceil(nbp/16) records), level 2 d_part3 (1/16 of that), level 3 d_part2 again (1/256 of it), ...
    float *out = h->d_part2, *other = h->d_part3;
    while (f.n > 1024) {
        const int ng = (f.n + kGroup - 1) / kGroup;
        hipLaunchKernelGGL(k_combine_group, dim3(ng), dim3(kThreads), 0, st, f.recs, f.sb, f.sc, f.n, h->HA, h->hc.neg_inv_lambda, out, f.nil_dev);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        f.recs = out; f.sb = 2 + h->HA; f.sc = 1; f.n = ng;
        std::swap(out, other);
    }
    const mppi_kev kev = p.finish; // profiled: the finish kernel's own dispatch begin/end (hipExtLaunchKernel events), like the rollout kernel's
    if (f.xchg)
        hipExtLaunchKernelGGL(k_finish_cols_xchg, dim3(h->HA), dim3(kThreads), 0, st, kev.begin, kev.end, 0, f.recs, f.sb, f.sc, f.n, h->HA, h->a,
                              h->hc.neg_inv_lambda, f.U_in, f.U_out, f.u_out, h->d_step, h->d_dbg, h->xchg_peers, h->shard_count, h->shard_rank, ++h->xchg_seq,
                              h->xchg_timeout_ticks, h->d_xchg_status, h->d_xchg_dead, (const float *)h->d_clip);
    else
        hipExtLaunchKernelGGL(k_finish_cols, dim3(h->HA), dim3(kThreads), 0, st, kev.begin, kev.end, 0, f.recs, f.sb, f.sc, f.n, h->HA, h->a,
                              h->hc.neg_inv_lambda, f.U_in, f.U_out, f.u_out, f.record_out, f.apply, h->d_step, h->d_dbg, (const float *)h->d_clip, f.nil_dev,
                              f.armed_seq ? (const unsigned long long *)h->d_decision : (const unsigned long long *)nullptr, f.armed_seq, f.pre);
    hipError_t e = hipGetLastError();
    if (p && e == hipSuccess) prof_commit(h, st);
    return e;
}

// After the update: the shifted sequence becomes the warm start (a pointer offset), then the optional
// Savitzky-Golay smoothing (filterSeq) writes the filtered sequence into the other buffer.
static hipError_t advance_sequence(mppi_handle *h, hipStream_t st)
{
    h->U_advance();
    if (h->sg_window > 0) {
        hipLaunchKernelGGL(k_savgol, dim3((h->HA + 255) / 256), dim3(256), 0, st, h->U_cur(), h->U_other(), h->d_sg_rows,
                           h->d_sg_start, h->H, h->a, h->sg_window);
        h->u_cur = 1 - h->u_cur;
        h->u_off = 0;
    }
    return hipGetLastError();
}

// Savitzky-Golay weights (scipy.signal.savgol_filter, deriv=0, mode='interp'): for row t the window starts at
// s = clamp(t-h, 0, H-w) and the fitted polynomial is evaluated at x0 = t-(s+h): weights = e(x0)ᵀ(AᵀA)⁻¹Aᵀ with
// A[i][k] = ((i-h)/h')^k. Normal equations in long double with abscissae scaled to [-1,1], partial pivoting.
static bool savgol_rows(int H, int w, int p, std::vector<float> &rows, std::vector<int> &start)
{
    const int hw = w / 2, n = p + 1;
    const long double sc = hw > 0 ? (long double)hw : 1.0L;
    rows.assign((size_t)H * w, 0.f);
    start.assign(H, 0);
    std::vector<long double> A((size_t)w * n);
    for (int i = 0; i < w; ++i) {
        long double v = 1.0L;
        for (int k = 0; k < n; ++k) { A[(size_t)i * n + k] = v; v *= (long double)(i - hw) / sc; }
    }
    std::vector<long double> N((size_t)n * n);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            long double acc = 0.0L;
            for (int i = 0; i < w; ++i) acc += A[(size_t)i * n + r] * A[(size_t)i * n + c];
            N[(size_t)r * n + c] = acc;
        }
    for (int t = 0; t < H; ++t) {
        const int s0 = std::min(std::max(t - hw, 0), H - w);
        start[t] = s0;
        const long double x0 = (long double)(t - (s0 + hw)) / sc;
        std::vector<long double> M(N), y(n);
        long double v = 1.0L;
        for (int k = 0; k < n; ++k) { y[k] = v; v *= x0; }
        for (int c = 0; c < n; ++c) { // Gaussian elimination, partial pivoting
            int piv = c;
            for (int r = c + 1; r < n; ++r) if (fabsl(M[(size_t)r * n + c]) > fabsl(M[(size_t)piv * n + c])) piv = r;
            if (fabsl(M[(size_t)piv * n + c]) < 1e-300L) return false;
            if (piv != c) { for (int k = 0; k < n; ++k) std::swap(M[(size_t)piv * n + k], M[(size_t)c * n + k]); std::swap(y[piv], y[c]); }
            for (int r = c + 1; r < n; ++r) {
                const long double f = M[(size_t)r * n + c] / M[(size_t)c * n + c];
                for (int k = c; k < n; ++k) M[(size_t)r * n + k] -= f * M[(size_t)c * n + k];
                y[r] -= f * y[c];
            }
        }
        for (int r = n - 1; r >= 0; --r) {
            long double acc = y[r];
            for (int k = r + 1; k < n; ++k) acc -= M[(size_t)r * n + k] * y[k];
            y[r] = acc / M[(size_t)r * n + r];
        }
        for (int i = 0; i < w; ++i) {
            long double acc = 0.0L;
            for (int k = 0; k < n; ++k) acc += A[(size_t)i * n + k] * y[k];
            rows[(size_t)t * w + i] = (float)acc;
        }
    }
    return true;
}

extern "C" mppi_status mppi_set_action_limits(mppi_handle *h, const float *a_min, const float *a_max, int n)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!a_min && !a_max) {
        if (h->d_clip) { HIP_TRY(h, hipDeviceSynchronize()); HIP_TRY(h, hipFree(h->d_clip)); h->d_clip = nullptr; }
        return MPPI_OK;
    }
    if (!a_min || !a_max || n != h->a) return fail(h, MPPI_ERR_INVALID_ARG, "a_min and a_max must both have a_dim floats");
    std::vector<float> lim(2 * (size_t)n);
    for (int j = 0; j < n; ++j) {
        if (!(a_min[j] <= a_max[j])) return fail(h, MPPI_ERR_INVALID_ARG, "a_min must be <= a_max");
        lim[j] = a_min[j]; lim[n + j] = a_max[j];
    }
    if (!h->d_clip) HIP_TRY(h, hipMalloc((void **)&h->d_clip, sizeof(float) * 2 * n));
    HIP_TRY(h, hipMemcpy(h->d_clip, lim.data(), sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    return MPPI_OK;
}

extern "C" mppi_status mppi_set_sequence_filter(mppi_handle *h, int window, int polyorder)
{
    MPPI_NOT_BATCH(h, "mppi_set_sequence_filter");
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    HIP_TRY(h, hipDeviceSynchronize());
    if (window == 0) { h->sg_window = 0; return MPPI_OK; }
    if (window < 1 || (window & 1) == 0 || window > h->H || polyorder < 0 || polyorder >= window)
        return fail(h, MPPI_ERR_INVALID_ARG, "filter window must be odd and <= tau, 0 <= polyorder < window");
    std::vector<float> rows;
    std::vector<int> start;
    if (!savgol_rows(h->H, window, polyorder, rows, start)) return fail(h, MPPI_ERR_INVALID_ARG, "singular Savitzky-Golay system");
    if (h->d_sg_rows) { HIP_TRY(h, hipFree(h->d_sg_rows)); h->d_sg_rows = nullptr; }
    if (h->d_sg_start) { HIP_TRY(h, hipFree(h->d_sg_start)); h->d_sg_start = nullptr; }
    HIP_TRY(h, hipMalloc((void **)&h->d_sg_rows, sizeof(float) * rows.size()));
    HIP_TRY(h, hipMalloc((void **)&h->d_sg_start, sizeof(int) * start.size()));
    HIP_TRY(h, hipMemcpy(h->d_sg_rows, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_sg_start, start.data(), sizeof(int) * start.size(), hipMemcpyHostToDevice));
    h->sg_window = window;
    return MPPI_OK;
}

// The slots of d_part that hold records belong to ONE tile count at a time (the MLP kernels and the tile kernel of the same
// handle may cut K differently): when the count changes, every slot goes back to the neutral record first.
static hipError_t ensure_record_layout(mppi_handle *h, hipStream_t st, int n_tiles)
{
    if (h->part_nb == n_tiles) return hipSuccess;
    if (h->part_nb != 0)
        hipLaunchKernelGGL(k_fill_records, dim3((h->nbp * (2 + h->HA) + 255) / 256), dim3(256), 0, st, h->d_part, h->nbp, 2 + h->HA);
    h->part_nb = n_tiles;
    return hipGetLastError();
}

// ---- Py normalizeCost (controller_base.py:468-474): costs, global min/max, then the update on c' = (c-min)/(max-min) with the SAME noise
// (regenerated from the same Philox counters). Two halves, which an unsharded step (enqueue_partials) runs back to back and a K-sharded
// one as two calls with the ranks' agreement on the range between them (mppi_shard_cost_range, mppi_shard_partial_normalized).
// Fast form on the producer/consumer kernel (ROUTE_PC): exp(-(c' - min c')/lambda) = exp(-(c - min c)/(lambda (max - min))), so the normalised
// update is the plain one at another temperature. A pass at lambda for the costs; then the weights-only pass (PC_PASS_WEIGHTS, r04): no
// rollouts — the weights from the stored costs, the noise regenerated for the weighted sums; records at the range's temperature, which the
// finish reads from d_mm[2] (r03: a full second rollout pass, 42 us at C3; the tile kernel's two passes 76). Else: cost pass,
// k_cost_normalize, record pass from the normalised costs at lambda.
//  pc_eligible's horizon bound depends on pc_np, and pc_np on THIS shard's tile count (or a per-handle tuning): with
// 132 < H <= 160 and ragged shards straddling 512 tiles one rank would make raw-cost records at the range temperature and another
// normalised-cost records at lambda. A sharded handle therefore takes the fast form only below the bound that holds for every pc_np: the
// form depends on the configuration only, never on the shard's size, and all ranks make their records in the same units.
static bool norm_fast(const mppi_handle *h) { return h->hc.model_kind != MPPI_MODEL_MLP && !h->is_gen && pc_eligible(h) && (h->shard_count == 1 || h->H <= 132); }
static Route norm_route(const mppi_handle *h, int src, const float *noise_out)
{
    const Route r = rollout_route(h, src, noise_out, false);
    return r == ROUTE_PC && !norm_fast(h) ? ROUTE_TILE : r;
}

// First half: the costs into d_cost. range_out (the sharded calls): this shard's {-min, max} goes there as well. Fast form: unsharded, the
// PC_PASS_COSTS pass, every tile leaving its (min, max) in d_tile_mm; with range_out the plain pass (its records, at lambda, are overwritten
// by the second half) and k_cost_minmax. Else the cost-only pass, which a profiled step brackets (kev: the dominant launch), and k_cost_minmax.
static mppi_status norm_costs(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, const float *x_dev, const float *eps, float *noise_out, float *range_out)
{
    if (route == ROUTE_PC) HIP_TRY(h, launch_rollout(h, st, route, mppi_kev{}, src, MODE_ROLLOUT, x_dev, eps, h->d_cost, noise_out, range_out ? PC_PASS_PLAIN : PC_PASS_COSTS));
    else HIP_TRY(h, launch_rollout(h, st, route, kev, src, MODE_COST_ONLY, x_dev, eps, h->d_cost, noise_out, PC_PASS_PLAIN, false, true));
    if (route == ROUTE_PC && !range_out) return MPPI_OK;
    hipLaunchKernelGGL(k_cost_minmax, dim3(1), dim3(1024), 0, st, h->d_cost, h->K_local, h->d_mm, 0.0f, (float *)nullptr, range_out);
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

// Second half: the records from the costs of the first, and where the finish finds their temperature (made->nil_dev). Fast form: the
// weights-only pass (kev: a profiled step reports this pass, the one whose records are used); range_given: the range is in d_mm already.
// Else from the costs normalised with the range in d_mm; a learned point-mass model's records come from the tile kernel.
static mppi_status norm_records(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, const float *x_dev, const float *eps, bool range_given, Finish *made)
{
    if (route == ROUTE_PC) {
        HIP_TRY(h, launch_rollout(h, st, route, kev, src, MODE_ROLLOUT, x_dev, eps, h->d_cost, nullptr, PC_PASS_WEIGHTS, range_given));
        made->nil_dev = h->d_mm + 2; // the temperature k_rollout_pc / k_cost_minmax / k_range_apply left there
        return MPPI_OK;
    }
    hipLaunchKernelGGL(k_cost_normalize, dim3((h->K_local + 255) / 256), dim3(256), 0, st, h->d_cost, h->K_local, h->d_mm, h->d_cost2);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, launch_rollout(h, st, route == ROUTE_GEN ? ROUTE_GEN : ROUTE_TILE, mppi_kev{}, src, MODE_COSTS_GIVEN, x_dev, eps, h->d_cost2, nullptr));
    return MPPI_OK;
}

// rollouts of this shard -> partial records in d_part; *made = where they are, how many, their temperature. Handles normalizeCost.
static mppi_status enqueue_partials(mppi_handle *h, hipStream_t st, int src, const float *x_dev, const float *eps, float *noise_out, Finish *made)
{
    const Route route = rollout_route(h, src, noise_out, false);
    TraceRange tr(h, "mppi:rollout");
    *made = own_records(h);
    HIP_TRY(h, ensure_record_layout(h, st, (route == ROUTE_MLP && !h->normalize) ? h->nb_mlp : h->nb)); // (normalizeCost: the tile kernel writes the records)
    const mppi_kev kev = prof_slot(h).rollout;
    if (!h->normalize) {
        HIP_TRY(h, launch_rollout(h, st, route, kev, src, MODE_ROLLOUT, x_dev, eps, h->d_cost, noise_out));
        return MPPI_OK;
    }
    if (h->shard_count != 1) return fail(h, MPPI_ERR_UNSUPPORTED, "normalize_cost on a sharded handle: mppi_shard_cost_range, reduce the ranges over the ranks, mppi_shard_partial_normalized");
    if (mppi_status s = norm_costs(h, st, route, kev, src, x_dev, eps, noise_out, nullptr); s != MPPI_OK) return s;
    // every workgroup of the weights-only pass reduces the nb tile pairs itself: nb^2 x 8 bytes of L2 reads in all — 8 MB at 1024 tiles, too much
    // beyond a few thousand (K > 131072 on one GPU): there the range comes from ONE k_cost_minmax launch over the costs instead
    const bool many_tiles = route == ROUTE_PC && h->nb > 2048;
    if (many_tiles) {
        hipLaunchKernelGGL(k_cost_minmax, dim3(1), dim3(1024), 0, st, h->d_cost, h->K_local, h->d_mm, h->hc.neg_inv_lambda, h->d_mm + 3, (float *)nullptr);
        HIP_TRY(h, hipGetLastError());
    }
    return norm_records(h, st, route, kev, src, x_dev, eps, many_tiles, made);
}

static mppi_status ensure_eps(mppi_handle *h)
{
    if (!h->d_eps) HIP_TRY(h, hipMalloc((void **)&h->d_eps, sizeof(float) * (size_t)h->K_local * h->HA));
    return MPPI_OK;
}

// ----------------------------------------------------------------------------------------
extern "C" int mppi_record_size(const mppi_handle *h) { return h ? 2 + h->HA : 0; }
extern "C" int mppi_local_samples(const mppi_handle *h) { return h ? h->K_local : 0; }
extern "C" int mppi_sample_offset(const mppi_handle *h) { return h ? h->k_offset : 0; }

extern "C" mppi_status mppi_synchronize(mppi_handle *h)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

// The rollout kernel instance a (Philox) step of this handle launches, as rocprofv3 prints it: the route and the family's pick, no launch.
extern "C" mppi_status mppi_rollout_kernel_name(const mppi_handle *h, char *buf, size_t n)
{
    if (!h || !buf || n == 0) return MPPI_ERR_INVALID_ARG;
    const mppi_unit_a *u = unit(h);
    const char *name = nullptr;
    switch (rollout_route(h, SRC_PHILOX, nullptr, true)) {
    case ROUTE_BATCH: name = h->is_gen ? mppi_batch_auv_name(h) : u ? u->batch_name(h) : nullptr; break;
    case ROUTE_STEP: name = u ? u->step_name(h, STEP_FUSE) : nullptr; break;
    case ROUTE_PC: name = u ? u->pc_name(h, h->normalize ? PC_PASS_WEIGHTS : PC_PASS_PLAIN) : nullptr; break;
    case ROUTE_TILE: name = u ? u->tile_name(h, SRC_PHILOX, h->normalize ? MODE_COST_ONLY : MODE_ROLLOUT) : nullptr; break;
    case ROUTE_MLP: name = u ? u->mlp_name(h, SRC_PHILOX) : nullptr; break;
    case ROUTE_GEN: name = mppi_gen_name(h, h->normalize ? MODE_COST_ONLY : MODE_ROLLOUT); break;
    }
    if (!name) return MPPI_ERR_UNSUPPORTED; // (no rollout kernel serves the handle)
    std::snprintf(buf, n, "%s", name);
    return MPPI_OK;
}

extern "C" mppi_status mppi_profile_begin(mppi_handle *h, int max_steps)
{
    if (!h || max_steps <= 0 || max_steps > (1 << 20)) return h ? fail(h, MPPI_ERR_INVALID_ARG, "max_steps out of range") : MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    while ((int)h->ev.size() < 4 * max_steps) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    h->prof_n = 0;
    h->prof_cap = max_steps;
    return MPPI_OK;
}

extern "C" mppi_status mppi_profile_end(mppi_handle *h, float *rollout_ms_avg, float *finish_ms_avg, int *n_steps)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    const int n = h->prof_n;
    h->prof_cap = 0;
    double tr = 0.0, tf = 0.0;
    if (n > 0) {
        HIP_TRY(h, hipEventSynchronize(h->ev[4 * (n - 1) + 3]));
        for (int i = 0; i < n; ++i) {
            float a = 0.f, b = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&a, h->ev[4 * i + 0], h->ev[4 * i + 1]));
            HIP_TRY(h, hipEventElapsedTime(&b, h->ev[4 * i + 2], h->ev[4 * i + 3]));
            tr += a; tf += b;
        }
    }
    if (rollout_ms_avg) *rollout_ms_avg = n ? (float)(tr / n) : 0.f;
    if (finish_ms_avg) *finish_ms_avg = n ? (float)(tf / n) : 0.f;
    if (n_steps) *n_steps = n;
    h->prof_n = 0;
    return MPPI_OK;
}

// ---- state that a lone handle and a batch keep alike: each accessor serves members(h) members at the strides of mppi_handle.hip.h, and the
// public entry points (mppi_* for a lone handle, mppi_batch_* for a batch) are their argument checks plus a call.
// goals [members(h)][s] into the members' constants, the one copy the kernels read; hc mirrors member 0's. A lone handle uploads its whole
// block, so what the host changed in hc goes with the goal.
static mppi_status set_goals(mppi_handle *h, const float *goals)
{
    MPPI_ENTER(h);
    if (h->batch) {
        const size_t row = sizeof(float) * h->s;
        HIP_TRY(h, hipMemcpy2DAsync((char *)h->dC + offsetof(DevConsts, goal), sizeof(DevConsts), goals, row, row, h->batch, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    for (int i = 0; i < h->s; ++i) h->hc.goal[i] = goals[i];
    return h->batch ? MPPI_OK : upload_consts(h);
}

extern "C" mppi_status mppi_set_goal(mppi_handle *h, const float *goal, int n)
{
    MPPI_NOT_BATCH(h, "mppi_set_goal");
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!goal || n != h->s) // "Wrong goal size, it should match the state dimension" controller_base.cpp:127-130
        return fail(h, MPPI_ERR_INVALID_ARG, "wrong goal size, it should match the state dimension");
    return set_goals(h, goal);
}

extern "C" mppi_status mppi_set_mlp(mppi_handle *h, const mppi_mlp_desc *d)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    const int mk = h->hc.model_kind;
    if (mk != MPPI_MODEL_MLP && mk != MPPI_MODEL_NN_AUV && mk != MPPI_MODEL_NN_AUV_SPEED) return fail(h, MPPI_ERR_INVALID_ARG, "not a learned-model handle");
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

// One launch = one control step (k_step_pc<.., STEP_FUSE>): tiles and the column waves that finish them in the same grid.
static mppi_status fused_step(mppi_handle *h, hipStream_t st, const float *x_dev, float *u_dev)
{
    TraceRange tr(h, "mppi:rollout");
    const ProfSlot p = prof_slot(h);
    const mppi_step_launch L{STEP_FUSE, x_dev, h->U_cur(), h->U_other(), u_dev, h->next_seq()};
    HIP_TRY(h, per_a(h, &mppi_unit_a::step, st, p.rollout, &L)); // the launch's own begin / end
    HIP_TRY(h, prof_one_launch(h, p, st));
    HIP_TRY(h, advance_sequence(h, st));
    return MPPI_OK;
}

// The plain control step in two halves, which a K-sharded step runs as two calls with the record exchange between them (mppi_shard_partial,
// mppi_shard_finish): enqueue_partials makes the records; this finishes them with the update and advances the sequence.
static mppi_status finish_step(mppi_handle *h, hipStream_t st, const Finish &f)
{
    HIP_TRY(h, launch_finish(h, st, f));
    HIP_TRY(h, advance_sequence(h, st));
    return MPPI_OK;
}
// ... and both in one, on Philox noise or the noise in eps (src), xchg: with the in-kernel record exchange. ONE launch where the fused
// route serves: never with the exchange, never with injected noise (rollout_route).
static mppi_status plain_step(mppi_handle *h, hipStream_t st, int src, const float *x_dev, const float *eps, float *u_dev, bool xchg = false)
{
    if (!xchg && rollout_route(h, src, nullptr, true) == ROUTE_STEP) return fused_step(h, st, x_dev, u_dev);
    Finish f;
    if (mppi_status s = enqueue_partials(h, st, src, x_dev, eps, nullptr, &f); s != MPPI_OK) return s;
    f.u_out = u_dev; f.xchg = xchg;
    return finish_step(h, st, f);
}

// Arm a step: the launch(es) that run it as soon as mppi_next has stored x. U_in / U_out: the sequence as it stands once every step
// enqueued before this one has been applied (the caller's bookkeeping may still be one step behind).
static mppi_status arm_launch(mppi_handle *h, const float *U_in, float *U_out, unsigned seq)
{
    const int mode = STEP_ARM | (fuse_ok(h) ? STEP_FUSE : 0);
    float *u_arg = h->d_pin + 2 * kMaxS;
    if (!(mode & STEP_FUSE)) HIP_TRY(h, ensure_record_layout(h, h->stream, h->nb));
    const mppi_step_launch L{mode, nullptr, U_in, U_out, u_arg, seq};
    HIP_TRY(h, per_a(h, &mppi_unit_a::step, h->stream, mppi_kev{}, &L));
    if (!(mode & STEP_FUSE)) {
        Finish f = own_records(h);
        f.U_in = U_in; f.U_out = U_out; f.u_out = u_arg; f.armed_seq = seq;
        HIP_TRY(h, launch_finish(h, h->stream, f));
    }
    return MPPI_OK;
}

// The pre-launched pipelined step (MPPI_TUNE_PRELAUNCH; k_step_pc<.., STEP_PRE> + k_finish_cols with FinishPre). Step n goes to stream
// n & 1 of the handle: its rollout is eligible as soon as the finish of step n-2 (the launch before it on that stream) is done, i.e. while
// step n-1 still runs on the other stream; it draws its noise in the CU slots step n-1's workgroups leave and waits for step n-1's U' as
// granules. Order that keeps the two grids from competing for slots: step n-1's workgroups are all resident long before step n becomes
// eligible (that takes the finish of n-2, which takes the END of rollout n-2, whose slots rollout n-1 — eligible since finish n-3 — has
// taken). Start-up has no such history and builds it with two events: rollout 2 (second stream) behind rollout 1 — it would otherwise share
// the chip with it —, and rollout 3 (first stream, behind finish 1) behind the moment the second stream got PAST that wait: rollout 2 is
// the next packet of its queue then, and rollout 3 sees the event through the same cross-queue latency that rollout 2 has already paid
// (measured without it: rollout 3 became resident first, held every slot waiting for finish 2, and rollout 2 never ran — the deadline).
// (one round of the grid: a rollout with workgroups still undispatched while the NEXT step's waiting workgroups hold the slots would never finish)
static int pre_slots(const mppi_handle *h)
{
    const int per_cu = h->pc_np == 3 ? (mppi_pc_slots(3, h->H) == 6 && 6 * 4 * h->a <= 80 ? 4 : 2) : 3; // k_step_pc's __launch_bounds__
    return per_cu * h->n_cu;
}
static bool pre_shape_ok(const mppi_handle *h) { return step_shape_ok(h) && (fuse_ok(h) || (h->nb > 128 && h->nb <= pre_slots(h))) && h->d_arm != nullptr; }
static bool pre_ok(const mppi_handle *h) { return h->prelaunch && pre_shape_ok(h); }

static mppi_status pre_step(mppi_handle *h, const float *x_dev, float *u_dev)
{
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->arm_inflight) HIP_TRY(h, quiesce(h));
    if (!h->pre_active) { // enter: everything enqueued so far drains; the sequence as it stands becomes the first granules, the step counter the mirror
        if (!h->stream2) HIP_TRY(h, hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
        if (!h->pre_ev) HIP_TRY(h, hipEventCreateWithFlags(&h->pre_ev, hipEventDisableTiming));
        if (!h->pre_ev2) HIP_TRY(h, hipEventCreateWithFlags(&h->pre_ev2, hipEventDisableTiming));
        if (!h->d_ugr) HIP_TRY(h, hipMalloc((void **)&h->d_ugr, sizeof(unsigned long long) * 2 * (size_t)h->HA));
        if (!h->d_cu_ctr) {
            HIP_TRY(h, hipMalloc((void **)&h->d_cu_ctr, sizeof(int) * 4096));
            HIP_TRY(h, hipMemset(h->d_cu_ctr, 0, sizeof(int) * 4096));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream2));
        std::vector<float> U(h->HA);
        unsigned long long step = 0;
        HIP_TRY(h, hipMemcpy(U.data(), h->U_cur(), sizeof(float) * h->HA, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(&step, h->d_step, sizeof(step), hipMemcpyDeviceToHost));
        const unsigned tag = h->next_seq();
        std::vector<unsigned long long> g(2 * (size_t)h->HA, 0ull);
        for (int i = 0; i < h->HA; ++i) {
            uint32_t bits;
            std::memcpy(&bits, &U[i], 4);
            g[i] = ((unsigned long long)tag << 32) | bits;
        }
        HIP_TRY(h, hipMemcpy(h->d_ugr, g.data(), sizeof(unsigned long long) * g.size(), hipMemcpyHostToDevice));
        if (!fuse_ok(h)) HIP_TRY(h, ensure_record_layout(h, h->stream, h->nb));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->pre_buf = 0; h->pre_tag = tag; h->pre_step = step; h->pre_count = 0; h->pre_active = true;
    }
    hipStream_t st = (h->pre_count & 1ull) ? h->stream2 : h->stream;
    if (h->pre_count == 1) HIP_TRY(h, hipEventRecord(h->pre_ev2, h->stream2)); // (behind the wait for rollout 1, in front of rollout 2)
    const unsigned seq = h->next_seq();
    const unsigned long long *ugr_in = h->d_ugr + (size_t)h->pre_buf * h->HA;
    unsigned long long *ugr_out = h->d_ugr + (size_t)(1 - h->pre_buf) * h->HA;
    const bool fused = fuse_ok(h); // <= 128 tiles: the column waves of the same grid finish the step (and write the next step's granules)
    const ProfSlot p = prof_slot(h);
    {
        TraceRange tr(h, "mppi:rollout");
        mppi_step_launch L{STEP_PRE | (fused ? STEP_FUSE : 0), x_dev, h->U_cur(), h->U_other(), u_dev, seq};
        L.ugr = ugr_in; L.utag = h->pre_tag; L.step_index = h->pre_step; L.ugr_out = fused ? ugr_out : nullptr;
        HIP_TRY(h, per_a(h, &mppi_unit_a::step, st, p.rollout, &L));
    }
    if (h->pre_count == 0) HIP_TRY(h, hipEventRecord(h->pre_ev, st)); // (start-up: see above)
    if (!fused) {
        Finish f = own_records(h);
        f.u_out = u_dev; f.pre = FinishPre{ugr_in, ugr_out, seq, h->pre_step};
        HIP_TRY(h, launch_finish(h, st, f));
    } else HIP_TRY(h, prof_one_launch(h, p, st));
    if (h->pre_count == 0) HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->pre_ev, 0));
    if (h->pre_count == 1) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->pre_ev2, 0)); // rollout 3 behind the second stream's release
    h->U_advance(); // (no sequence filter on this path: step_shape_ok)
    h->pre_buf = 1 - h->pre_buf; h->pre_tag = seq; h->pre_step += 1ull; h->pre_count += 1ull;
    return MPPI_OK;
}

extern "C" mppi_status mppi_next_device(mppi_handle *h, const float *x_dev, float *u_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_next_device");
    if (!h || !x_dev || !u_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (h->shard_count != 1) return fail(h, MPPI_ERR_INVALID_ARG, "sharded handle: use mppi_shard_partial / mppi_shard_finish");
    if (stream == nullptr && pre_ok(h)) return pre_step(h, x_dev, u_dev);
    MPPI_ENTER(h);
    TraceRange step_range(h, "mppi:step");
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return plain_step(h, st, SRC_PHILOX, x_dev, nullptr, u_dev);
}

extern "C" mppi_status mppi_shard_partial(mppi_handle *h, const float *x_dev, float *record_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_partial");
    if (!h || !x_dev || !record_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    Finish f;
    if (mppi_status s = enqueue_partials(h, st, SRC_PHILOX, x_dev, nullptr, nullptr, &f); s != MPPI_OK) return s;
    f.u_out = h->d_u; f.record_out = record_dev; f.apply = 0;
    HIP_TRY(h, launch_finish(h, st, f));
    return MPPI_OK;
}

// ---- normalizeCost on a K-sharded controller -----------------------------------------------------
// c' = (c - min)/(max - min) needs the min and max over ALL samples (controller_base.py:468-474): each shard rolls its samples and
// reports its own {-min, max}; the ranks reduce the pairs (ONE 2-float all-reduce(MAX)); each shard then makes its record from costs
// normalised with the agreed range. The two calls are the two halves of enqueue_partials' normalizeCost (norm_costs, norm_records).
extern "C" mppi_status mppi_shard_cost_range(mppi_handle *h, const float *x_dev, float *range_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_cost_range");
    if (!h || !x_dev || !range_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (!h->normalize) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_cost_range: the handle was created without normalize_cost");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIP_TRY(h, ensure_record_layout(h, st, h->nb));
    return norm_costs(h, st, norm_route(h, SRC_PHILOX, nullptr), prof_slot(h).rollout, SRC_PHILOX, x_dev, nullptr, nullptr, range_dev);
}

extern "C" mppi_status mppi_shard_partial_normalized(mppi_handle *h, const float *x_dev, const float *range_dev, float *record_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_partial_normalized");
    if (!h || !x_dev || !range_dev || !record_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (!h->normalize) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_partial_normalized: the handle was created without normalize_cost");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    hipLaunchKernelGGL(k_range_apply, dim3(1), dim3(64), 0, st, range_dev, h->d_mm, h->hc.neg_inv_lambda, (float *)nullptr);
    HIP_TRY(h, hipGetLastError());
    // d_cost still holds this step's costs (mppi_shard_cost_range); the agreed range and its temperature are in d_mm now
    Finish f = own_records(h);
    if (mppi_status s = norm_records(h, st, norm_route(h, SRC_PHILOX, nullptr), prof_slot(h).rollout, SRC_PHILOX, x_dev, nullptr, true, &f); s != MPPI_OK) return s;
    f.u_out = h->d_u; f.record_out = record_dev; f.apply = 0;
    HIP_TRY(h, launch_finish(h, st, f));
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_finish(mppi_handle *h, const float *records_dev, int n_records, float *u_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_finish");
    if (!h || !records_dev || !u_dev || n_records <= 0) return h ? fail(h, MPPI_ERR_INVALID_ARG, "bad records/u pointer or count") : MPPI_ERR_INVALID_ARG;
    // more than 1024 records are folded 16:1 into the handle's scratch, which is sized for its own ceil(nbp/16) groups
    if (n_records > 1024 && (n_records + kGroup - 1) / kGroup > (h->nbp + kGroup - 1) / kGroup)
        return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_finish: " + std::to_string(n_records) + " records fold into more groups than this handle's scratch holds (" +
                                                 std::to_string((h->nbp + kGroup - 1) / kGroup) + "): at most 1024 records, or a handle with at least as many tiles");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    Finish f = own_records(h);
    f.recs = records_dev; f.sb = 2 + h->HA; f.sc = 1; f.n = n_records; f.u_out = u_dev;
    if (h->norm_two_pass) f.nil_dev = h->d_mm + 2; // the ranks' records are in the units of this handle's own (mppi_shard_partial_normalized)
    return finish_step(h, st, f);
}

// One call per sharded step on the collective path (include/mppi_c.h): record -> the caller's all-gather (in place) -> finish.
extern "C" mppi_status mppi_shard_step(mppi_handle *h, const float *x_dev, float *u_dev, const mppi_collectives *coll, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_step");
    if (!h || !x_dev || !u_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    const bool gather = coll && coll->all_gather;
    if (h->shard_count > 1 && !gather) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_step: shard_count > 1 needs coll->all_gather (ncclAllGather's signature)");
    if (h->normalize && gather && !coll->all_reduce) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_step: a normalize_cost handle needs coll->all_reduce (ncclAllReduce's signature)");
    MPPI_ENTER(h);
    const int n = 2 + h->HA;
    // (a sharded handle gets both buffers in mppi_create; this covers the one-shard handle that walks the sharded path. Each pointer on its
    // own: a failed second allocation must not leave a half-made pair that the next call takes for complete — ADVICE r04)
    if (!h->d_recs) HIP_TRY(h, hipMalloc((void **)&h->d_recs, sizeof(float) * (size_t)n * h->shard_count));
    if (!h->d_range) HIP_TRY(h, hipMalloc((void **)&h->d_range, sizeof(float) * 2));
    TraceRange step_range(h, "mppi:step");
    float *own = h->d_recs + (size_t)n * h->shard_rank;
    mppi_status s;
    if (h->normalize) {
        if ((s = mppi_shard_cost_range(h, x_dev, h->d_range, stream)) != MPPI_OK) return s;
        if (gather) {
            TraceRange tr(h, "mppi:exchange");
            const int rc = coll->all_reduce(h->d_range, h->d_range, 2, MPPI_COLL_FLOAT32, MPPI_COLL_MAX, coll->comm, stream ? stream : (void *)h->stream);
            if (rc != 0) return fail(h, MPPI_ERR_EXCHANGE, "mppi_shard_step: all_reduce returned " + std::to_string(rc));
        }
        if ((s = mppi_shard_partial_normalized(h, x_dev, h->d_range, own, stream)) != MPPI_OK) return s;
    } else if ((s = mppi_shard_partial(h, x_dev, own, stream)) != MPPI_OK) return s;
    if (gather) {
        TraceRange tr(h, "mppi:exchange");
        const int rc = coll->all_gather(own, h->d_recs, (size_t)n, MPPI_COLL_FLOAT32, coll->comm, stream ? stream : (void *)h->stream);
        if (rc != 0) return fail(h, MPPI_ERR_EXCHANGE, "mppi_shard_step: all_gather returned " + std::to_string(rc));
    }
    return mppi_shard_finish(h, h->d_recs, h->shard_count, u_dev, stream);
}

// ---- direct record exchange (see include/mppi_c.h) -----------------------------------------------
extern "C" mppi_status mppi_shard_p2p_export(mppi_handle *h, void *ipc_handle_out, void **inbox_dev_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_export");
    if (!h || !inbox_dev_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL inbox_dev_out") : MPPI_ERR_INVALID_ARG;
    if (h->shard_count > kMaxPeers) return fail(h, MPPI_ERR_UNSUPPORTED, "direct exchange supports at most 16 shards");
    // fault injection for the fallback tests: mppi_set_tuning(MPPI_TUNE_P2P_FAULT, 1 = export | 2 = probe)
    if (h->p2p_fault == 1) return fail(h, MPPI_ERR_HIP, "injected fault: inbox export refused");
    MPPI_ENTER(h);
    if (!h->xchg_inbox) {
        // uncached: peer stores land in memory and the local spin loads see them without any cache maintenance
        HIP_TRY(h, hipExtMallocWithFlags((void **)&h->xchg_inbox, h->xchg_inbox_bytes(), hipDeviceMallocUncached));
        HIP_TRY(h, hipMemset(h->xchg_inbox, 0, h->xchg_inbox_bytes()));
        HIP_TRY(h, hipHostMalloc((void **)&h->h_xchg_status, sizeof(unsigned), hipHostMallocMapped));
        *h->h_xchg_status = 0u;
        HIP_TRY(h, hipHostGetDevicePointer((void **)&h->d_xchg_status, h->h_xchg_status, 0));
        HIP_TRY(h, hipMalloc((void **)&h->d_xchg_dead, sizeof(unsigned)));
        HIP_TRY(h, hipMemset(h->d_xchg_dead, 0, sizeof(unsigned)));
        HIP_TRY(h, hipMalloc((void **)&h->d_probe_got, sizeof(float) * kMaxPeers));
        HIP_TRY(h, hipDeviceSynchronize());
    }
    if (ipc_handle_out) {
        static_assert(sizeof(hipIpcMemHandle_t) == MPPI_IPC_HANDLE_BYTES, "ipc handle size");
        hipIpcMemHandle_t ih;
        HIP_TRY(h, hipIpcGetMemHandle(&ih, h->xchg_inbox));
        memcpy(ipc_handle_out, &ih, sizeof(ih));
    }
    *inbox_dev_out = h->xchg_inbox;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_open(mppi_handle *h, const void *ipc_handle, void **peer_inbox_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_open");
    if (!h || !ipc_handle || !peer_inbox_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL ipc handle / output") : MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    hipIpcMemHandle_t ih;
    memcpy(&ih, ipc_handle, sizeof(ih));
    void *p = nullptr;
    HIP_TRY(h, hipIpcOpenMemHandle(&p, ih, hipIpcMemLazyEnablePeerAccess));
    h->xchg_opened.push_back(p);
    *peer_inbox_out = p;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_attach(mppi_handle *h, void *const *inboxes, int n, int timeout_ms)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_attach");
    if (!h || !inboxes) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL inbox table") : MPPI_ERR_INVALID_ARG;
    if (n != h->shard_count || n > kMaxPeers) return fail(h, MPPI_ERR_INVALID_ARG, "need exactly shard_count (<= 16) inbox pointers, rank order");
    if (!h->xchg_inbox) return fail(h, MPPI_ERR_INVALID_ARG, "call mppi_shard_p2p_export first");
    if (inboxes[h->shard_rank] != (void *)h->xchg_inbox) return fail(h, MPPI_ERR_INVALID_ARG, "entry shard_rank must be this handle's own inbox");
    if (timeout_ms <= 0 || timeout_ms > 60000) return fail(h, MPPI_ERR_INVALID_ARG, "timeout_ms must be in [1, 60000]");
    for (int g = 0; g < n; ++g) {
        if (!inboxes[g]) return fail(h, MPPI_ERR_INVALID_ARG, "NULL inbox pointer");
        h->xchg_peers.inbox[g] = (unsigned long long *)inboxes[g];
    }
    h->xchg_timeout_ticks = (long long)timeout_ms * 100000ll; // wall_clock64 ticks at 100 MHz
    h->xchg_attached = true;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_probe(mppi_handle *h, void *stream, int *ok_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_probe");
    if (!h || !ok_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL ok_out") : MPPI_ERR_INVALID_ARG;
    if (!h->xchg_attached) return fail(h, MPPI_ERR_INVALID_ARG, "inboxes not attached");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const unsigned seq = ++h->probe_seq;
    const int G = h->shard_count;
    auto payload = [&](int g) { return (float)(1000 * (int)(seq % 1000u) + g + 1); };
    hipLaunchKernelGGL(k_xchg_probe, dim3(1), dim3(64), 0, st, h->xchg_peers, h->xchg_step_slots(), G, h->shard_rank, seq,
                       payload(h->shard_rank), h->xchg_timeout_ticks, h->d_xchg_status, h->d_xchg_dead, h->d_probe_got);
    HIP_TRY(h, hipGetLastError());
    float got[kMaxPeers];
    HIP_TRY(h, hipMemcpyAsync(got, h->d_probe_got, sizeof(float) * G, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    int ok = (*(volatile unsigned *)h->h_xchg_status & 1u) ? 0 : 1;
    for (int g = 0; g < G; ++g) ok &= got[g] == payload(g);
    if (h->p2p_fault == 2) ok = 0;
    *ok_out = ok;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_step(mppi_handle *h, const float *x_dev, float *u_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_step");
    if (!h || !x_dev || !u_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (!h->xchg_attached) return fail(h, MPPI_ERR_INVALID_ARG, "inboxes not attached");
    // a deadline missed by any earlier step: refuse (the steps enqueued since then applied zero updates; U and the step
    // counter may differ between ranks until they are re-synchronised — ShardedController.resync)
    if (*(volatile unsigned *)h->h_xchg_status & 1u)
        return fail(h, MPPI_ERR_EXCHANGE, "direct exchange: a packet missed its deadline; the direct path is closed for this handle");
    MPPI_ENTER(h);
    TraceRange step_range(h, "mppi:step");
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return plain_step(h, st, SRC_PHILOX, x_dev, nullptr, u_dev, true);
}

extern "C" mppi_status mppi_shard_p2p_status(mppi_handle *h, int *timed_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_status");
    if (!h || !timed_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL timed_out") : MPPI_ERR_INVALID_ARG;
    *timed_out = h->h_xchg_status ? (int)(*(volatile unsigned *)h->h_xchg_status & 1u) : 0;
    return MPPI_OK;
}

static long long now_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// host-pointer step shared by mppi_next / mppi_next_with_noise
//
// Armed launches (MPPI_TUNE_ARMED_US > 0; mppi_step.hip.h). Once two calls have followed each other within the soft deadline, a call
// leaves the NEXT step's launch behind it — armed: resident, noise drawn, waiting for x. The next call then only stores x into the
// device's x slot and watches the pinned u slot: no launch and no dispatch between x and u. A launch whose x does not come in time
// aborts by itself (tile 0's verdict, mirrored in pinned host memory) and the call falls back to the ordinary launch; any other entry
// point retires an armed launch first (quiesce). An aborted or cancelled launch changes nothing: same U, same step counter, and the
// step that follows draws the noise it would have drawn.
static mppi_status step_host(mppi_handle *h, const float *x, int n_x, const float *eps, size_t n_eps, float *u_out, int n_u)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_NOT_BATCH(h, eps ? "mppi_next_with_noise" : "mppi_next");
    if (!x || !u_out || n_x != h->s || n_u != h->a) return fail(h, MPPI_ERR_INVALID_ARG, "x must have s_dim floats and u_out a_dim floats");
    if (h->shard_count != 1) return fail(h, MPPI_ERR_INVALID_ARG, "sharded handle: use mppi_shard_partial / mppi_shard_finish");
    HIP_TRY(h, hipSetDevice(h->device));
    TraceRange step_range(h, "mppi:step");
    const long long t_call = now_ns();
    const long long gap_ns = h->last_next_ns ? t_call - h->last_next_ns : (1ll << 62);
    h->last_next_ns = t_call;
    const bool may_arm = !eps && h->prof_cap == 0 && arm_ok(h);
    if (h->arm_inflight && !may_arm) HIP_TRY(h, quiesce(h));
    constexpr uint32_t kUSentinel = 0x7fc0deadu;
    volatile uint32_t *uslot = reinterpret_cast<volatile uint32_t *>(h->h_pin + 2 * kMaxS);
    auto u_seen = [&]() { bool seen = true; for (int j = 0; j < h->a; ++j) seen = seen && uslot[j] != kUSentinel; return seen; };
    // m_db.addX(s); m_db.addU(out_tensor[1])  controller_base.cpp:146-147 — only when a log was asked for
    // (mppi_set_transition_log): a preallocated ring, no allocation on this path
    auto hand_out = [&]() {
        std::memcpy(u_out, h->h_pin + 2 * kMaxS, sizeof(float) * h->a);
        if (h->log_cap) {
            size_t r;
            if (h->log_count < h->log_cap) r = (h->log_head + h->log_count++) % h->log_cap;
            else { r = h->log_head; h->log_head = (h->log_head + 1) % h->log_cap; h->log_dropped++; } // full: the oldest row is overwritten (counted)
            float *row = h->log_rows.data() + r * h->log_stride();
            std::memcpy(row, x, sizeof(float) * h->s);
            std::memcpy(row + h->s, u_out, sizeof(float) * h->a);
            row[2 * h->s + h->a] = 0.0f; // x_next not known yet
        }
        return MPPI_OK;
    };

    if (h->arm_inflight) {
        volatile unsigned long long *verdict = h->h_arm;
        const unsigned seq = h->arm_seq;
        auto verdict_of = [&](unsigned q) -> unsigned { const unsigned long long v = *verdict; return (unsigned)(v >> 32) == q ? (unsigned)v : 0u; };
        if (*reinterpret_cast<volatile unsigned *>(h->h_arm + 1) != 0u) { // a hard deadline passed inside an armed launch: never expected
            (void)quiesce(h);
            *reinterpret_cast<volatile unsigned *>(h->h_arm + 1) = 0u;
            return fail(h, MPPI_ERR_HIP, "armed launch: a wave waited past its hard deadline");
        }
        if (verdict_of(seq) == kArmAbort) { // the soft deadline passed before this call: the launch has left (or is leaving)
            h->arm_inflight = false;
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        } else {
            for (int j = 0; j < h->a; ++j) uslot[j] = kUSentinel;
            for (int i = 0; i < h->s; ++i) xslot_store(h, i, x[i], seq);
            store_fence();
            // arm the step after this one while this one runs (its bookkeeping is committed below, once tile 0 has accepted x)
            const unsigned seq2 = h->next_seq();
            const mppi_status as = arm_launch(h, h->d_Ubuf[1 - h->u_cur] + h->a, h->d_Ubuf[h->u_cur], seq2);
            if (as != MPPI_OK) { h->arm_seq = seq2; (void)quiesce(h); return as; }
            unsigned v = 0u;
            const long long t0 = now_ns(), limit = ((long long)h->arm_us + 100000ll) * 1000ll;
            for (unsigned it = 0; (v = verdict_of(seq)) == 0u; ++it)
                if ((it & 255u) == 255u && now_ns() - t0 > limit) break;
            if (v == kArmAccept) {
                h->U_advance();
                h->arm_seq = seq2; // (arm_inflight stays up: the launch just armed)
                bool seen = false;
                for (unsigned it = 0; !(seen = u_seen()); ++it)
                    if ((it & 1023u) == 1023u && now_ns() - t0 > 200000000ll) break;
                if (!seen) { (void)quiesce(h); return fail(h, MPPI_ERR_HIP, "armed step: no control within 200 ms of an accepted x"); }
                return hand_out();
            }
            // aborted while x was on its way (or silent): retire the launch armed behind it, then the ordinary launch below
            h->arm_seq = seq2;
            HIP_TRY(h, quiesce(h));
            if (v == 0u) return fail(h, MPPI_ERR_HIP, "armed launch: no verdict");
        }
    }

    int src = SRC_PHILOX;
    if (eps) {
        if (n_eps != (size_t)h->K_local * h->HA) return fail(h, MPPI_ERR_INVALID_ARG, "eps must hold K_local*tau*a floats");
        mppi_status s = ensure_eps(h);
        if (s != MPPI_OK) return s;
        HIP_TRY(h, hipMemcpyAsync(h->d_eps, eps, sizeof(float) * n_eps, hipMemcpyHostToDevice, h->stream));
        src = SRC_HBM;
    }
    // x goes into the pinned slot the kernels read directly (slots alternate so a step never re-reads the
    // address of the previous x); u comes back through the pinned, device-mapped u slot.
    h->pin_slot ^= 1;
    std::memcpy(h->h_pin + h->pin_slot * kMaxS, x, sizeof(float) * h->s);
    const float *x_arg = h->d_pin + h->pin_slot * kMaxS;
    float *u_arg = h->d_pin + 2 * kMaxS;
    const bool spin_u = h->sync_spin && h->sg_window == 0; // with a sequence filter the step has one more kernel after u
    if (spin_u) for (int j = 0; j < h->a; ++j) uslot[j] = kUSentinel;
    if (mppi_status s = plain_step(h, h->stream, src, x_arg, h->d_eps, u_arg); s != MPPI_OK) return s;
    // two calls within the soft deadline of each other: the host loop is fast enough for an armed launch to be fed in time
    if (may_arm && spin_u && (h->arm_always || gap_ns < (long long)h->arm_us * 1000ll)) {
        const unsigned seq = h->next_seq();
        mppi_status s = arm_launch(h, h->U_cur(), h->U_other(), seq);
        if (s != MPPI_OK) return s;
        h->arm_inflight = true;
        h->arm_seq = seq;
    }
    // u arrives in the pinned slot as `a` single 4-byte stores over PCIe: watch the slot instead of waiting for the
    // stream's completion signal (the runtime's wake-up costs several us of a ~35 us synchronous step). The slot was
    // filled with a NaN pattern the update cannot produce; if it has not changed after 2 ms (a long step, an error, a
    // genuine NaN) fall back to the ordinary wait. Later calls on this handle are stream-ordered behind the step.
    bool seen = false;
    if (spin_u) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 0; !seen; ++it) {
            seen = u_seen();
            if (!seen && (it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
    }
    if (!seen) {
        if (h->arm_inflight) HIP_TRY(h, quiesce(h)); // (the stream would only drain at the armed launch's deadline)
        else HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return hand_out();
}

extern "C" mppi_status mppi_next(mppi_handle *h, const float *x, int n_x, float *u_out, int n_u)
{
    return step_host(h, x, n_x, nullptr, 0, u_out, n_u);
}

extern "C" mppi_status mppi_next_with_noise(mppi_handle *h, const float *x, int n_x, const float *eps, size_t n_eps, float *u_out, int n_u)
{
    if (h && !eps) return fail(h, MPPI_ERR_INVALID_ARG, "eps is NULL");
    return step_host(h, x, n_x, eps, n_eps, u_out, n_u);
}

extern "C" mppi_status mppi_set_transition_log(mppi_handle *h, int max_rows)
{
    MPPI_NOT_BATCH(h, "mppi_set_transition_log");
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (max_rows < 0) return fail(h, MPPI_ERR_INVALID_ARG, "max_rows must be >= 0");
    try {
        std::vector<float> rows((size_t)max_rows * h->log_stride());
        h->log_rows.swap(rows);
    } catch (const std::bad_alloc &) {
        return fail(h, MPPI_ERR_ALLOC, "transition log: out of host memory");
    }
    h->log_cap = (size_t)max_rows; h->log_count = 0; h->log_head = 0; h->log_dropped = 0;
    return MPPI_OK;
}

extern "C" mppi_status mppi_transition_log_stats(mppi_handle *h, uint64_t *rows_held, uint64_t *rows_overwritten, uint64_t *rows_without_successor)
{
    MPPI_NOT_BATCH(h, "mppi_transition_log_stats");
    if (!h) return MPPI_ERR_INVALID_ARG;
    size_t open_rows = 0;
    for (size_t q = 0; q < h->log_count; ++q)
        if (h->log_rows[((h->log_head + q) % h->log_cap) * h->log_stride() + 2 * h->s + h->a] == 0.0f) ++open_rows;
    if (rows_held) *rows_held = h->log_count;
    if (rows_overwritten) *rows_overwritten = h->log_dropped;
    if (rows_without_successor) *rows_without_successor = open_rows;
    return MPPI_OK;
}

extern "C" mppi_status mppi_save_next(mppi_handle *h, const float *x_next, int n)
{
    MPPI_NOT_BATCH(h, "mppi_save_next");
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x_next || n != h->s) return fail(h, MPPI_ERR_INVALID_ARG, "x_next must have s_dim floats");
    if (!h->log_cap) return MPPI_OK; // logging is off
    if (!h->log_count) return fail(h, MPPI_ERR_INVALID_ARG, "saveNext before the first next()");
    // m_db.addNext controller_base.cpp:159-163: the successor of the LAST logged (x, u) — a skipped saveNext leaves that
    // row without a successor (it is then not written) instead of shifting every later row
    float *row = h->log_rows.data() + ((h->log_head + h->log_count - 1) % h->log_cap) * h->log_stride();
    std::memcpy(row + h->s + h->a, x_next, sizeof(float) * h->s);
    row[2 * h->s + h->a] = 1.0f;
    return MPPI_OK;
}

// data_base.cpp:36-71 toCSV: header x0,..,u0,..,x_next0,.. then one row per transition, columns x | u | x_next.
// MPPI_CSV_REFERENCE writes the reference's exact bytes: every header cell and every value followed by a comma
// (tensor2CSV / csvHeader append "," after each element, so lines END with a comma), values as std::to_string(float)
// = "%f" (6 decimals). MPPI_CSV_ROUNDTRIP writes "%.9g" (fp32 round-trips) without the trailing comma.
extern "C" mppi_status mppi_to_csv_format(mppi_handle *h, const char *filename, int format)
{
    MPPI_NOT_BATCH(h, "mppi_to_csv_format");
    if (!h || !filename) return h ? fail(h, MPPI_ERR_INVALID_ARG, "filename is NULL") : MPPI_ERR_INVALID_ARG;
    if (format != MPPI_CSV_REFERENCE && format != MPPI_CSV_ROUNDTRIP) return fail(h, MPPI_ERR_INVALID_ARG, "unknown CSV format");
    if (!h->log_cap) return fail(h, MPPI_ERR_INVALID_ARG, "the transition log is off: call mppi_set_transition_log first");
    FILE *f = std::fopen(filename, "w");
    if (!f) return fail(h, MPPI_ERR_IO, std::string("cannot open ") + filename);
    const bool ref = format == MPPI_CSV_REFERENCE;
    const int s = h->s, a = h->a;
    for (int i = 0; i < s; ++i) std::fprintf(f, "x%d,", i);
    for (int i = 0; i < a; ++i) std::fprintf(f, "u%d,", i);
    for (int i = 0; i < s; ++i) std::fprintf(f, (ref || i + 1 < s) ? "x_next%d," : "x_next%d", i);
    std::fputc('\n', f);
    for (size_t q = 0; q < h->log_count; ++q) {
        const float *row = h->log_rows.data() + ((h->log_head + q) % h->log_cap) * h->log_stride();
        if (row[2 * s + a] == 0.0f) continue; // no successor recorded
        const int n = 2 * s + a;
        for (int i = 0; i < n; ++i) {
            if (ref) std::fprintf(f, "%f,", (double)row[i]); // std::to_string(float)
            else std::fprintf(f, i + 1 < n ? "%.9g," : "%.9g", (double)row[i]);
        }
        std::fputc('\n', f);
    }
    if (std::fclose(f) != 0) return fail(h, MPPI_ERR_IO, std::string("write failed: ") + filename);
    return MPPI_OK;
}

// replaces ControllerBase::toCSV (controller_base.cpp:164): the reference's format
extern "C" mppi_status mppi_to_csv(mppi_handle *h, const char *filename) { return mppi_to_csv_format(h, filename, MPPI_CSV_REFERENCE); }

// diagnostic switches (A/B timing, fault injection for the fallback tests). The library reads NO environment variable:
// what a process inherits cannot change kernels or inject faults.
extern "C" mppi_status mppi_set_tuning(mppi_handle *h, int what, int value)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h); // (an armed launch was built for the handle as it was)
    if (h->batch) { // a batch always takes the two launches of mppi_launch_batch.hip
        const char *why = (what == MPPI_TUNE_FUSED_STEP && value != 0) ? "fused_step"
                        : (what == MPPI_TUNE_ARMED_US && value != 0) ? "armed_us"
                        : (what == MPPI_TUNE_PRELAUNCH && value != 0) ? "prelaunch"
                        : (what == MPPI_TUNE_FORCE_TILE_KERNEL && value != 0) ? "force_tile_kernel"
                        : (h->is_gen && what == MPPI_TUNE_GEN_ONE_WAVE && value != 0) ? "gen_one_wave"
                        : (h->is_gen && what == MPPI_TUNE_MLP32_VALU && value != 0) ? "mlp32_valu" : nullptr;
        if (why) return fail(h, MPPI_ERR_UNSUPPORTED, std::string("tuning ") + why + ": a batched handle always runs the two-launch batched step");
    }
    switch (what) {
    case MPPI_TUNE_FUSED_STEP:
        if (value < 0 || value > 2) return fail(h, MPPI_ERR_INVALID_ARG, "fused step: 0 (two launches), 1 (one launch), 2 (one launch, the six-wave workgroup at every horizon)");
        h->fuse_step = value; break;
    case MPPI_TUNE_ARMED_US:
        if (value < 0 || value > 1000000) return fail(h, MPPI_ERR_INVALID_ARG, "armed launch: soft deadline 0 (off) .. 1000000 us");
        if (value > 0 && !h->d_xslot)
            return fail(h, MPPI_ERR_UNSUPPORTED, "armed launches need the point-mass producer/consumer path and a large-BAR system (the host stores x straight into device memory)");
        h->arm_us = value; break;
    case MPPI_TUNE_ARMED_ALWAYS: h->arm_always = value != 0; break;
    case MPPI_TUNE_PRELAUNCH:
        if (value != 0 && !pre_shape_ok(h))
            return fail(h, MPPI_ERR_UNSUPPORTED, "the pre-launched step serves the point-mass producer/consumer path with the diagonal quadratic cost, at most one round of the grid, one shard");
        h->prelaunch = value != 0; break;
    case MPPI_TUNE_FORCE_TILE_KERNEL: h->force_tile = value != 0; break;
    case MPPI_TUNE_PC_PRODUCERS:
        if (value != 3 && value != 5) return fail(h, MPPI_ERR_INVALID_ARG, "producer waves per workgroup: 3 or 5");
        h->pc_np = value; break;
    case MPPI_TUNE_PC_BALANCE: // 0 off, 1 on, 0x10000 | b3 b2 b1 b0 (hex nibbles): on with these head starts of the generations
        h->pc_no_balance = value == 0;
        if (value & 0x10000) h->pc_bias = value & 0xffff;
        break;
    case MPPI_TUNE_PC_LDS_MIN:
        if (value < 0 || value > 64 * 1024) return fail(h, MPPI_ERR_INVALID_ARG, "LDS bytes out of range (0..65536)");
        h->pc_lds_min = value; break;
    case MPPI_TUNE_SYNC_SPIN: h->sync_spin = value != 0; break;
    case MPPI_TUNE_MLP_V1: // the first exact-fp32 MLP kernel (8 waves, 64 rollouts per workgroup), for A/B timing
        if (h->hc.model_kind != MPPI_MODEL_MLP || h->mlp_bx3 || h->mlp_small) return fail(h, MPPI_ERR_INVALID_ARG, "not an exact-fp32 2x256 MLP handle");
        h->mlp_v2 = (value == 0 && h->a <= 3) ? 1 : 0;
        h->nb_mlp = h->mlp_v2 ? (h->K_local + kMlp2R - 1) / kMlp2R : (h->K_local + kMlpR - 1) / kMlpR; // d_part is sized for the larger count
        break;
    case MPPI_TUNE_MLP32_VALU:
        if (!(h->mlp_small == 32 || (h->hc.model_kind == MPPI_MODEL_NN_AUV_SPEED && h->mlp_small == 16)) || h->mlp_bx3)
            return fail(h, MPPI_ERR_INVALID_ARG, "not an exact-fp32 Dense(32) MLP handle (or an NNAUVModelSpeed one)");
        if (value < 0 || value > 2)
            return fail(h, MPPI_ERR_INVALID_ARG, "0 (matrix cores, two-wave pipeline), 1 (vector-ALU kernel) or 2 (matrix cores, one wave per 32 rollouts)");
        h->mlp32_valu = value; break;
    case MPPI_TUNE_P2P_FAULT:
        if (value < 0 || value > 2) return fail(h, MPPI_ERR_INVALID_ARG, "fault: 0 none, 1 export, 2 probe");
        h->p2p_fault = value; break;
    case MPPI_TUNE_GEN_ONE_WAVE:
        if (h->hc.model_kind != MPPI_MODEL_AUV) return fail(h, MPPI_ERR_INVALID_ARG, "not an AUVModel handle");
        h->gen_one_wave = value != 0; break;
    case MPPI_TUNE_TRACE:
        if (value != 0 && !g_roctx.load()) return fail(h, MPPI_ERR_UNSUPPORTED, "MPPI_TUNE_TRACE: neither librocprofiler-sdk-roctx.so nor libroctx64.so could be loaded");
        h->trace = value != 0; break;
    default: return fail(h, MPPI_ERR_INVALID_ARG, "unknown tuning item");
    }
    return MPPI_OK;
}

// ----------------------------------------------------------------------------------------
// every member's sequence [members(h)][tau * a] out of / into its U block (HA + a floats: the sequence and its zero tail)
static mppi_status get_sequences(mppi_handle *h, float *U)
{
    MPPI_ENTER(h);
    const size_t row = sizeof(float) * h->HA, pitch = sizeof(float) * (h->HA + h->a);
    HIP_TRY(h, hipMemcpy2DAsync(U, row, h->U_cur(), pitch, row, members(h), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

static mppi_status set_sequences(mppi_handle *h, const float *U)
{
    MPPI_ENTER(h);
    const size_t row = sizeof(float) * h->HA, pitch = sizeof(float) * (h->HA + h->a);
    for (int i = 0; i < 2; ++i) HIP_TRY(h, hipMemsetAsync(h->d_Ubuf[i], 0, pitch * members(h), h->stream)); // zero tails
    h->u_cur = 0; h->u_off = 0; h->d_Uupd = nullptr;
    HIP_TRY(h, hipMemcpy2DAsync(h->d_Ubuf[0], pitch, U, row, row, members(h), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_get_action_sequence(mppi_handle *h, float *U, int n)
{
    MPPI_NOT_BATCH(h, "mppi_get_action_sequence");
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!U || n != h->HA) return fail(h, MPPI_ERR_INVALID_ARG, "U must hold tau*a floats");
    return get_sequences(h, U);
}

extern "C" mppi_status mppi_set_action_sequence(mppi_handle *h, const float *U, int n)
{
    MPPI_NOT_BATCH(h, "mppi_set_action_sequence");
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!U || n != h->HA) return fail(h, MPPI_ERR_INVALID_ARG, "U must hold tau*a floats");
    return set_sequences(h, U);
}

extern "C" mppi_status mppi_get_step_counter(mppi_handle *h, uint64_t *step)
{
    if (!h || !step) return MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    unsigned long long v = 0;
    HIP_TRY(h, hipMemcpyAsync(&v, h->d_step, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *step = v;
    return MPPI_OK;
}

extern "C" mppi_status mppi_set_step_counter(mppi_handle *h, uint64_t step)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    unsigned long long v = step;
    HIP_TRY(h, hipMemcpyAsync(h->d_step, &v, sizeof(v), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

// one debug item of member `member` (a lone handle: 0)
static mppi_status debug_get(mppi_handle *h, int member, int what, float *out, size_t n)
{
    MPPI_ENTER(h);
    const size_t K = (size_t)h->K_local;
    const float *src = nullptr;
    size_t need = 0;
    float *tmp = nullptr;
    const float *cost = h->d_cost + K * member, *dbg = h->d_dbg + 8 * (size_t)member;
    switch (what) {
    case MPPI_DBG_COSTS: src = cost; need = K; break;
    case MPPI_DBG_BETA: src = dbg; need = 1; break;
    case MPPI_DBG_ETA: src = dbg + 1; need = 1; break;
    case MPPI_DBG_AUX: src = dbg; need = 8; break; // beta, eta, and what a timing-study build left in the other words
    case MPPI_DBG_U_UPDATED: // U' of the last step = the current buffer from offset 0 (the warm start reads it from offset a)
        if (!h->d_Uupd) return fail(h, MPPI_ERR_INVALID_ARG, h->batch ? "no step has run since the action sequences were set" : "no step has run since the action sequence was set");
        src = h->d_Uupd + (size_t)(h->HA + h->a) * member; need = (size_t)h->HA; break;
    case MPPI_DBG_WEIGHTS: {
        need = K;
        if (n != need) return fail(h, MPPI_ERR_INVALID_ARG, "wrong output size");
        HIP_TRY(h, hipMalloc((void **)&tmp, sizeof(float) * K));
        // (a lone handle's two-pass normalizeCost: the raw costs at the step's temperature = the normalised costs at lambda)
        hipLaunchKernelGGL(k_weights, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, h->stream, (const DevConsts *)(h->dC + member),
                           (h->normalize && !h->norm_two_pass) ? (const float *)h->d_cost2 : cost, (int)K, dbg, (float *)nullptr, (float *)nullptr, tmp,
                           h->norm_two_pass ? (const float *)(h->d_mm + 2) : (const float *)nullptr);
        src = tmp;
        break;
    }
    case MPPI_DBG_NOISE: {
        // the member's noise of the LAST step, regenerated from its Philox key and Sigma at the previous step counter (step-1)
        need = K * (size_t)h->HA;
        if (n != need) return fail(h, MPPI_ERR_INVALID_ARG, "wrong output size");
        if (mppi_status s = ensure_eps(h); s != MPPI_OK) return s;
        unsigned long long cur = 0;
        HIP_TRY(h, hipMemcpyAsync(&cur, h->d_step, sizeof(cur), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (cur == 0) return fail(h, MPPI_ERR_INVALID_ARG, "no step has run yet");
        const unsigned long long prev = cur - 1;
        HIP_TRY(h, hipMemcpyAsync(h->d_step, &prev, sizeof(prev), hipMemcpyHostToDevice, h->stream));
        // noise-only pass of the tile kernel (the point mass) or of k_rollout_gen (the 13-state family), on the member's constants: reads
        // neither x nor any cost buffer and writes nothing but d_eps
        const DevConsts *own = h->dC + member;
        const hipError_t le = h->is_gen ? mppi_launch_gen(h, own, h->stream, mppi_kev{}, SRC_PHILOX, MODE_NOISE_ONLY, h->d_x, h->U_cur(), nullptr, nullptr, nullptr, h->d_eps)
                                        : launch_tile(h, own, h->stream, SRC_PHILOX, MODE_NOISE_ONLY, h->d_x, h->U_cur(), nullptr, nullptr, nullptr, h->d_eps);
        HIP_TRY(h, hipMemcpyAsync(h->d_step, &cur, sizeof(cur), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, le);
        src = h->d_eps;
        break;
    }
    default: return fail(h, MPPI_ERR_INVALID_ARG, "unknown debug item");
    }
    if (n != need) { if (tmp) (void)hipFree(tmp); return fail(h, MPPI_ERR_INVALID_ARG, "wrong output size"); }
    hipError_t e = hipMemcpyAsync(out, src, sizeof(float) * need, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (tmp) (void)hipFree(tmp);
    HIP_TRY(h, e);
    return MPPI_OK;
}

extern "C" mppi_status mppi_debug_get(mppi_handle *h, int what, float *out, size_t n)
{
    MPPI_NOT_BATCH(h, "mppi_debug_get");
    if (!h || !out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "out is NULL") : MPPI_ERR_INVALID_ARG;
    return debug_get(h, 0, what, out, n);
}

// ----------------------------------------------------------------------------------------
// helpers: scratch device buffers for the host-pointer helper entry points
struct DevBuf {
    float *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(float) * (n ? n : 1)); }
    hipError_t up(const float *src, size_t n, hipStream_t st) { return hipMemcpyAsync(p, src, sizeof(float) * n, hipMemcpyHostToDevice, st); }
    hipError_t down(float *dst, size_t n, hipStream_t st) const { return hipMemcpyAsync(dst, p, sizeof(float) * n, hipMemcpyDeviceToHost, st); }
};

extern "C" mppi_status mppi_model_step(mppi_handle *h, const float *x, int kx, const float *v, int k,
                                       float *out_free, float *out_action, float *out_next)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !v || k <= 0 || (kx != k && kx != 1)) return fail(h, MPPI_ERR_INVALID_ARG, "x is [kx,s] with kx in {1,k}; v is [k,a]");
    MPPI_ENTER(h);
    const int s = h->s, a = h->a;
    if (h->is_gen) {
        if (out_free || out_action) return fail(h, MPPI_ERR_UNSUPPORTED, "the free/action split exists for the point-mass model only");
        DevBuf dx, dv, dn, ds;
        HIP_TRY(h, dx.alloc((size_t)kx * s)); HIP_TRY(h, dv.alloc((size_t)k * a)); HIP_TRY(h, dn.alloc((size_t)k * s)); HIP_TRY(h, ds.alloc((size_t)k * 128));
        HIP_TRY(h, dx.up(x, (size_t)kx * s, h->stream)); HIP_TRY(h, dv.up(v, (size_t)k * a, h->stream));
        HIP_TRY(h, mppi_gen_model_step(h, h->stream, dx.p, kx, dv.p, k, ds.p, dn.p));
        if (out_next) HIP_TRY(h, dn.down(out_next, (size_t)k * s, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return MPPI_OK;
    }
    if (h->hc.model_kind == MPPI_MODEL_MLP) {
        if (out_free || out_action) return fail(h, MPPI_ERR_UNSUPPORTED, "the free/action split exists for the point-mass model only");
        DevBuf dx, dv, dn, ds;
        HIP_TRY(h, dx.alloc((size_t)kx * s)); HIP_TRY(h, dv.alloc((size_t)k * a)); HIP_TRY(h, dn.alloc((size_t)k * s)); HIP_TRY(h, ds.alloc((size_t)k * 2 * kHid));
        HIP_TRY(h, dx.up(x, (size_t)kx * s, h->stream)); HIP_TRY(h, dv.up(v, (size_t)k * a, h->stream));
        hipLaunchKernelGGL(k_mlp_step_ref, dim3((k + 63) / 64), dim3(64), 0, h->stream, h->dC, h->dM, dx.p, kx, dv.p, k, ds.p, dn.p);
        HIP_TRY(h, hipGetLastError());
        if (out_next) HIP_TRY(h, dn.down(out_next, (size_t)k * s, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return MPPI_OK;
    }
    DevBuf dx, dv, df, da, dn;
    HIP_TRY(h, dx.alloc((size_t)kx * s)); HIP_TRY(h, dv.alloc((size_t)k * a));
    HIP_TRY(h, df.alloc((size_t)kx * s)); HIP_TRY(h, da.alloc((size_t)k * s)); HIP_TRY(h, dn.alloc((size_t)k * s));
    HIP_TRY(h, dx.up(x, (size_t)kx * s, h->stream)); HIP_TRY(h, dv.up(v, (size_t)k * a, h->stream));
    const dim3 g((k + 255) / 256), b(256);
#define MPPI_MS_CASE(AA) case AA: hipLaunchKernelGGL(k_model_step<AA>, g, b, 0, h->stream, h->dC, dx.p, kx, dv.p, k, s, a, df.p, da.p, dn.p); break;
    switch (a) {
        MPPI_MS_CASE(1) MPPI_MS_CASE(2) MPPI_MS_CASE(3) MPPI_MS_CASE(4)
    default: hipLaunchKernelGGL(k_model_step<kMaxA>, g, b, 0, h->stream, h->dC, dx.p, kx, dv.p, k, s, a, df.p, da.p, dn.p); break;
    }
#undef MPPI_MS_CASE
    HIP_TRY(h, hipGetLastError());
    if (out_free) HIP_TRY(h, df.down(out_free, (size_t)kx * s, h->stream));
    if (out_action) HIP_TRY(h, da.down(out_action, (size_t)k * s, h->stream));
    if (out_next) HIP_TRY(h, dn.down(out_next, (size_t)k * s, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_auv_pieces(mppi_handle *h, const float *x, const float *u, int k, float *out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !u || !out || k <= 0) return fail(h, MPPI_ERR_INVALID_ARG, "x is [k,13], u is [k,6], out is [k,124]");
    if (h->hc.model_kind != MPPI_MODEL_AUV) return fail(h, MPPI_ERR_INVALID_ARG, "not an AUVModel handle");
    MPPI_ENTER(h);
    DevBuf dx, du, dout;
    HIP_TRY(h, dx.alloc((size_t)k * 13)); HIP_TRY(h, du.alloc((size_t)k * 6)); HIP_TRY(h, dout.alloc((size_t)k * 124));
    HIP_TRY(h, dx.up(x, (size_t)k * 13, h->stream)); HIP_TRY(h, du.up(u, (size_t)k * 6, h->stream));
    HIP_TRY(h, mppi_gen_auv_pieces(h, h->stream, dx.p, du.p, k, dout.p));
    HIP_TRY(h, dout.down(out, (size_t)k * 124, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_ellipse3d_terms(mppi_handle *h, const float *x, int k, int in_plane_frame, float *out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !out || k <= 0) return fail(h, MPPI_ERR_INVALID_ARG, "x is [k,13], out is [k,3]");
    if (h->hc.state_cost_kind != MPPI_STATE_COST_ELLIPSE3D) return fail(h, MPPI_ERR_INVALID_ARG, "not an ElipseCost3D handle");
    MPPI_ENTER(h);
    DevBuf dx, dout;
    HIP_TRY(h, dx.alloc((size_t)k * 13)); HIP_TRY(h, dout.alloc((size_t)k * 3));
    HIP_TRY(h, dx.up(x, (size_t)k * 13, h->stream));
    HIP_TRY(h, mppi_gen_e3_terms(h, h->stream, dx.p, k, in_plane_frame, dout.p));
    HIP_TRY(h, dout.down(out, (size_t)k * 3, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

template <int S, int A>
static void launch_costs_sa(mppi_handle *h, const float *x, const float *u, const float *eps, int k, float *os, float *oa, float *ot)
{
    const dim3 g((k + 255) / 256), b(256);
    if (h->hc.q_full) hipLaunchKernelGGL((k_costs<S, A, true>), g, b, 0, h->stream, h->dC, x, u, eps, k, h->s, h->a, os, oa, ot);
    else hipLaunchKernelGGL((k_costs<S, A, false>), g, b, 0, h->stream, h->dC, x, u, eps, k, h->s, h->a, os, oa, ot);
}

// state / action / step cost of k samples; x may be NULL (action cost only), u/eps may be NULL (state only)
static mppi_status costs_host(mppi_handle *h, const float *x, const float *u, const float *eps, int k,
                              float *out_state, float *out_action, float *out_step)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (k <= 0 || (!x && !u) || ((u == nullptr) != (eps == nullptr))) return fail(h, MPPI_ERR_INVALID_ARG, "bad cost arguments");
    MPPI_ENTER(h);
    const int s = h->s, a = h->a;
    DevBuf dx, du, de, ds, da, dt;
    HIP_TRY(h, dx.alloc((size_t)k * s)); HIP_TRY(h, du.alloc(a)); HIP_TRY(h, de.alloc((size_t)k * a));
    HIP_TRY(h, ds.alloc(k)); HIP_TRY(h, da.alloc(k)); HIP_TRY(h, dt.alloc(k));
    if (x) HIP_TRY(h, dx.up(x, (size_t)k * s, h->stream));
    if (u) { HIP_TRY(h, du.up(u, a, h->stream)); HIP_TRY(h, de.up(eps, (size_t)k * a, h->stream)); }
    const float *px = x ? dx.p : nullptr, *pu = u ? du.p : nullptr, *pe = u ? de.p : nullptr;
    // shapes of the reference's own tests + the point-mass family run exact instances
    if (h->gen != nullptr) HIP_TRY(h, mppi_gen_costs(h, h->stream, px, pu, pe, k, ds.p, da.p, dt.p)); // 13-state costs (quadratic, quaternion, 3D ellipse)
    else if (s == 2 && a == 1) launch_costs_sa<2, 1>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 2 && a == 2) launch_costs_sa<2, 2>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 4 && a == 2) launch_costs_sa<4, 2>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 4 && a == 3) launch_costs_sa<4, 3>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 6 && a == 3) launch_costs_sa<6, 3>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 8 && a == 4) launch_costs_sa<8, 4>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else launch_costs_sa<kMaxS, kMaxA>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    HIP_TRY(h, hipGetLastError());
    if (out_state) HIP_TRY(h, ds.down(out_state, k, h->stream));
    if (out_action) HIP_TRY(h, da.down(out_action, k, h->stream));
    if (out_step) HIP_TRY(h, dt.down(out_step, k, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_state_cost(mppi_handle *h, const float *x, int k, float *out)
{
    if (h && (!x || !out)) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    return costs_host(h, x, nullptr, nullptr, k, out, nullptr, nullptr);
}

extern "C" mppi_status mppi_action_cost(mppi_handle *h, const float *u, const float *eps, int k, float *out)
{
    if (h && (!u || !eps || !out)) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    return costs_host(h, nullptr, u, eps, k, nullptr, out, nullptr);
}

extern "C" mppi_status mppi_step_cost(mppi_handle *h, const float *x, const float *u, const float *eps, int k, float *out)
{
    if (h && (!x || !u || !eps || !out)) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    return costs_host(h, x, u, eps, k, nullptr, nullptr, out);
}

extern "C" mppi_status mppi_rollout_cost(mppi_handle *h, const float *x, const float *U, const float *eps, float *cost_out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !U || !eps || !cost_out) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    MPPI_ENTER(h);
    mppi_status s = ensure_eps(h);
    if (s != MPPI_OK) return s;
    DevBuf dx, dU, dc;
    HIP_TRY(h, dx.alloc(h->s)); HIP_TRY(h, dU.alloc(h->HA)); HIP_TRY(h, dc.alloc(h->K_local));
    HIP_TRY(h, dx.up(x, h->s, h->stream)); HIP_TRY(h, dU.up(U, h->HA, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_eps, eps, sizeof(float) * (size_t)h->K_local * h->HA, hipMemcpyHostToDevice, h->stream));
    if (h->is_gen) HIP_TRY(h, mppi_launch_gen(h, h->dC, h->stream, mppi_kev{}, SRC_HBM, MODE_COST_ONLY, dx.p, dU.p, h->d_eps, dc.p, h->d_part, nullptr));
    else if (h->hc.model_kind == MPPI_MODEL_MLP) HIP_TRY(h, per_a(h, &mppi_unit_a::mlp, h->stream, mppi_kev{}, SRC_HBM, MODE_COST_ONLY, dx.p, dU.p, h->d_eps, dc.p));
    else HIP_TRY(h, launch_tile(h, h->dC, h->stream, SRC_HBM, MODE_COST_ONLY, dx.p, dU.p, h->d_eps, dc.p, h->d_part, nullptr));
    HIP_TRY(h, dc.down(cost_out, h->K_local, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_update(mppi_handle *h, const float *cost, const float *eps, const float *U,
                                   float *beta, float *exp_arg, float *exp_out, float *nabla, float *weights,
                                   float *weighted_noise, float *U_new)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!cost || !eps || !U) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    MPPI_ENTER(h);
    mppi_status s = ensure_eps(h);
    if (s != MPPI_OK) return s;
    const int K = h->K_local, HA = h->HA;
    DevBuf dU, dc, drec, darg, dexp, dw, dUn, du;
    HIP_TRY(h, dU.alloc(HA)); HIP_TRY(h, dc.alloc(K)); HIP_TRY(h, drec.alloc(2 + HA));
    HIP_TRY(h, darg.alloc(K)); HIP_TRY(h, dexp.alloc(K)); HIP_TRY(h, dw.alloc(K)); HIP_TRY(h, dUn.alloc(HA)); HIP_TRY(h, du.alloc(kMaxA));
    HIP_TRY(h, dU.up(U, HA, h->stream)); HIP_TRY(h, dc.up(cost, K, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_eps, eps, sizeof(float) * (size_t)K * HA, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, ensure_record_layout(h, h->stream, h->nb));
    if (h->is_gen) HIP_TRY(h, mppi_launch_gen(h, h->dC, h->stream, mppi_kev{}, SRC_HBM, MODE_COSTS_GIVEN, h->d_x, dU.p, h->d_eps, dc.p, h->d_part, nullptr));
    else HIP_TRY(h, launch_tile(h, h->dC, h->stream, SRC_HBM, MODE_COSTS_GIVEN, h->d_x, dU.p, h->d_eps, dc.p, h->d_part, nullptr));
    h->norm_two_pass = 0; // records made from the GIVEN costs at lambda
    // record = (beta, eta, V); then U' on a scratch copy of U (apply shifts it, so read U_updated)
    unsigned long long step_before = 0;
    HIP_TRY(h, hipMemcpyAsync(&step_before, h->d_step, sizeof(step_before), hipMemcpyDeviceToHost, h->stream));
    Finish f = own_records(h);
    f.U_in = dU.p; f.U_out = dUn.p; f.u_out = du.p; f.record_out = drec.p;
    HIP_TRY(h, launch_finish(h, h->stream, f));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_step, &step_before, sizeof(step_before), hipMemcpyHostToDevice, h->stream)); // stateless call
    hipLaunchKernelGGL(k_weights, dim3((K + 255) / 256), dim3(256), 0, h->stream, h->dC, dc.p, K, drec.p, darg.p, dexp.p, dw.p, (const float *)nullptr);
    HIP_TRY(h, hipGetLastError());
    std::vector<float> rec(2 + HA), Un(HA);
    HIP_TRY(h, drec.down(rec.data(), 2 + HA, h->stream));
    HIP_TRY(h, dUn.down(Un.data(), HA, h->stream));
    if (exp_arg) HIP_TRY(h, darg.down(exp_arg, K, h->stream));
    if (exp_out) HIP_TRY(h, dexp.down(exp_out, K, h->stream));
    if (weights) HIP_TRY(h, dw.down(weights, K, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (beta) *beta = rec[0];
    if (nabla) *nabla = rec[1];
    if (weighted_noise) for (int c = 0; c < HA; ++c) weighted_noise[c] = (float)((double)rec[2 + c] / (double)rec[1]);
    if (U_new) std::memcpy(U_new, Un.data(), sizeof(float) * HA);
    return MPPI_OK;
}

// mGetNew (controller_base.cpp:326-329) / mShift (:314-324): pure slices, host side.
extern "C" mppi_status mppi_get_new(const float *U, int tau, int a, int nb, float *out)
{
    if (!U || (!out && nb > 0) || nb < 0 || nb > tau || a <= 0) return MPPI_ERR_INVALID_ARG;
    for (int i = 0; i < nb * a; ++i) out[i] = U[i];
    return MPPI_OK;
}

extern "C" mppi_status mppi_shift(const float *U, int tau, int a, const float *init, int nb_init, int nb, float *out)
{
    if (!U || !out || nb < 0 || nb > tau || nb_init < 0 || a <= 0) return MPPI_ERR_INVALID_ARG;
    int o = 0;
    for (int i = nb * a; i < tau * a; ++i) out[o++] = U[i];
    for (int i = 0; i < nb_init * a; ++i) out[o++] = init ? init[i] : 0.0f; // mInit0: zeros
    return MPPI_OK;
}

// ---- batched controllers (mppi_create_batch_configs; kernels in mppi_launch_batch.hip and mppi_launch_batch_gen.hip) ---------------
// Member m is made from cfgs[m]: its own seed, goal, lambda, gamma, upsilon, sigma and Q (its DevConsts block dC + m), its own x and
// sequence; the rest of the config is shared. Member m is bit for bit the lone handle mppi_create(&cfgs[m]), fed the same x, goal and
// sequence, on the same step counter: the batched rollout is the text of
// k_rollout_pc (the point mass) or k_rollout_auv_pc (the Fossen AUV model) with per-member operands, with the instance that handle would
// launch, and the batched finish is k_finish_cols' column_combine on the member's records over the same padded record count.
// the Fossen AUV model on its two-wave rollout (k_rollout_auv_pc, every horizon) with the step's one pass: what k_rollout_auv_pc_batch runs
static bool auv_batch_eligible(const mppi_handle *h)
{
    return h->is_gen && h->hc.model_kind == MPPI_MODEL_AUV && !h->gen_one_wave && !h->normalize && h->shard_count == 1;
}

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
    case MPPI_MODEL_NN_AUV_SPEED: return "batched controllers: model NNAUVSpeed is not supported (the point-mass and Fossen AUV models only)";
    default: break; // (mppi_create reports it)
    }
    switch (cfg->state_cost_kind) {
    case MPPI_STATE_COST_QUADRATIC: break;
    case MPPI_STATE_COST_ELLIPSE: return "batched controllers: the ellipse cost (ElipseCost) is not supported (the quadratic cost, and StaticQuatCost / ElipseCost3D with the Fossen AUV model)";
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
static const char *batch_shared_diff(const mppi_config *a, const mppi_config *b)
{
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
static mppi_status create_batch(const mppi_config *cfgs, int n, bool name_members, mppi_handle **out)
{
    for (int m = 0; m < n; ++m)
        if (cfgs[m].struct_size != sizeof(mppi_config)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_config.struct_size mismatch (use mppi_config_init)");
    for (int m = 1; m < n; ++m)
        if (const char *f = batch_shared_diff(&cfgs[0], &cfgs[m]))
            return fail(nullptr, MPPI_ERR_INVALID_ARG, "batched controllers: cfgs[" + std::to_string(m) + "]." + f + " differs from cfgs[0]." + f + " (every member shares it)");
    const mppi_config *cfg = &cfgs[0];
    if (const char *why = batch_refusal(cfg)) return fail(nullptr, MPPI_ERR_UNSUPPORTED, why);
    mppi_handle *h = nullptr;
    if (mppi_status st = prepare_handle(cfg, name_members, &h); st != MPPI_OK) return st;
    auto refuse = [&](mppi_status st, const std::string &why) { mppi_destroy(h); return fail(nullptr, st, why); };
    if (!h->is_gen && !pc_eligible(h)) return refuse(MPPI_ERR_UNSUPPORTED, "batched controllers: the producer/consumer rollout serves this shape only with s_dim = 2 a_dim, a_dim <= 4, tau <= 160 (<= 132 above 512 tiles)");
    if (h->is_gen && !auv_batch_eligible(h)) return refuse(MPPI_ERR_UNSUPPORTED, "batched controllers: the Fossen AUV model is batched on its two-wave rollout (k_rollout_auv_pc) only");
    if (h->nbp > 1024) return refuse(MPPI_ERR_UNSUPPORTED, "batched controllers: at most 1024 tiles (k = 65536) per member (the finish combines a member's records in one pass)");
    if ((long long)h->nb * n > (1ll << 30) / 64) return refuse(MPPI_ERR_INVALID_ARG, "batched controllers: n * k too large");
    // every member's constants; all members must run the instance member 0's lone handle picks
    std::vector<DevConsts> consts(n);
    consts[0] = h->hc;
    for (int m = 1; m < n; ++m)
        if (mppi_status st = member_consts(&cfgs[m], m, true, h, consts[m]); st != MPPI_OK) { mppi_destroy(h); return st; }
    h->batch = n;
    h->fuse_step = 0; // the two launches, always
    if (mppi_status st = allocate_handle(h, cfg, n, consts.data()); st != MPPI_OK) { g_create_err = h->err; mppi_destroy(h); return st; }
    *out = h;
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
    if (cfg->struct_size != sizeof(mppi_config)) return fail(nullptr, MPPI_ERR_INVALID_ARG, "mppi_config.struct_size mismatch (use mppi_config_init)");
    std::vector<mppi_config> cfgs;
    try {
        cfgs.assign((size_t)n, *cfg);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, MPPI_ERR_ALLOC, "out of host memory");
    }
    for (int m = 0; m < n; ++m) cfgs[m].seed = seeds ? seeds[m] : cfg->seed + (unsigned long long)m;
    return create_batch(cfgs.data(), n, false, out);
}

extern "C" int mppi_batch_size(const mppi_handle *h) { return h ? h->batch : 0; }

#define MPPI_BATCH_ONLY(h)                                                                                          \
    do {                                                                                                            \
        if (!(h)) return MPPI_ERR_INVALID_ARG;                                                                      \
        if (!(h)->batch) return fail((h), MPPI_ERR_INVALID_ARG, "not a batched handle (mppi_create_batch)");        \
    } while (0)

// rollouts of every member -> records, the finish of every member -> U', u_dev[B][a]; the sequences and the step counter advance
static mppi_status batch_step(mppi_handle *h, hipStream_t st, const float *x_dev, float *u_dev)
{
    if (h->is_gen ? !auv_batch_eligible(h) : !pc_eligible(h))
        return fail(h, MPPI_ERR_UNSUPPORTED, h->is_gen ? "batched step: the Fossen AUV model runs on k_rollout_auv_pc only"
                                                       : "batched step: the horizon exceeds what this producer count serves (tau <= 132 with 3 producers)");
    TraceRange step_range(h, "mppi:batch_step");
    const ProfSlot p = prof_slot(h); // the dispatches' own begin / end
    HIP_TRY(h, h->is_gen ? mppi_launch_batch_auv(h, st, p.rollout, x_dev) : per_a(h, &mppi_unit_a::batch, st, p.rollout, x_dev));
    HIP_TRY(h, h->is_gen ? mppi_launch_batch_finish_auv(h, st, h->U_cur(), h->U_other(), u_dev, p.finish)
                         : per_a(h, &mppi_unit_a::batch_finish, st, (const float *)h->U_cur(), h->U_other(), u_dev, p.finish));
    if (p) prof_commit(h, st);
    h->U_advance();
    return MPPI_OK;
}

extern "C" mppi_status mppi_batch_set_goals(mppi_handle *h, const float *goals, int n)
{
    MPPI_BATCH_ONLY(h);
    if (!goals || n != h->batch * h->s) return fail(h, MPPI_ERR_INVALID_ARG, "goals must hold n * s_dim floats");
    return set_goals(h, goals);
}

extern "C" mppi_status mppi_batch_next(mppi_handle *h, const float *x, int n_x, float *u_out, int n_u)
{
    MPPI_BATCH_ONLY(h);
    if (!x || !u_out || n_x != h->batch * h->s || n_u != h->batch * h->a) return fail(h, MPPI_ERR_INVALID_ARG, "x must hold n * s_dim floats and u_out n * a_dim");
    MPPI_ENTER(h);
    HIP_TRY(h, hipMemcpyAsync(h->d_bx, x, sizeof(float) * n_x, hipMemcpyHostToDevice, h->stream));
    if (mppi_status s = batch_step(h, h->stream, h->d_bx, h->d_bu); s != MPPI_OK) return s;
    HIP_TRY(h, hipMemcpyAsync(u_out, h->d_bu, sizeof(float) * n_u, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_batch_next_device(mppi_handle *h, const float *x_dev, float *u_dev, void *stream)
{
    MPPI_BATCH_ONLY(h);
    if (!x_dev || !u_dev) return fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer");
    MPPI_ENTER(h);
    return batch_step(h, stream ? (hipStream_t)stream : h->stream, x_dev, u_dev);
}

extern "C" mppi_status mppi_batch_get_action_sequences(mppi_handle *h, float *U, int n)
{
    MPPI_BATCH_ONLY(h);
    if (!U || n != h->batch * h->HA) return fail(h, MPPI_ERR_INVALID_ARG, "U must hold n * tau * a_dim floats");
    return get_sequences(h, U);
}

extern "C" mppi_status mppi_batch_set_action_sequences(mppi_handle *h, const float *U, int n)
{
    MPPI_BATCH_ONLY(h);
    if (!U || n != h->batch * h->HA) return fail(h, MPPI_ERR_INVALID_ARG, "U must hold n * tau * a_dim floats");
    return set_sequences(h, U);
}

extern "C" mppi_status mppi_batch_debug_get(mppi_handle *h, int member, int what, float *out, size_t n)
{
    MPPI_BATCH_ONLY(h);
    if (!out) return fail(h, MPPI_ERR_INVALID_ARG, "out is NULL");
    if (member < 0 || member >= h->batch) return fail(h, MPPI_ERR_INVALID_ARG, "member out of range");
    return debug_get(h, member, what, out, n);
}

// ---- closed-loop episodes (include/mppi_c.h): n_steps control steps with the handle's own model as the plant, on the handle's stream, no host
// wait between the steps. Step t is the plain step (plain_step / batch_step: never the pre-launched or an armed one — x of step t + 1 depends
// on u of step t) reading row t of the trajectory and writing row t of the control log, then ONE launch (mppi_episode.hip) that writes C[t],
// row t + 1 of the trajectory and the next goal. A learned model spends one launch more on its model-step kernel.
static mppi_status ensure_episode_staging(mppi_handle *h, size_t floats)
{
    if (floats <= h->ep_cap) return MPPI_OK;
    if (h->d_ep) { HIP_TRY(h, hipStreamSynchronize(h->stream)); HIP_TRY(h, hipFree(h->d_ep)); h->d_ep = nullptr; h->ep_cap = 0; }
    HIP_TRY(h, hipMalloc((void **)&h->d_ep, sizeof(float) * floats));
    h->ep_cap = floats;
    return MPPI_OK;
}

static mppi_status run_episode(mppi_handle *h, const char *name, const float *x0, int n_x, int n_steps, const float *goals, const float *disturbance,
                               float *X_out, float *U_out, float *C_out)
{
    const int B = members(h), s = h->s, a = h->a;
    const std::string who = std::string(name) + ": ";
    if (!x0 || n_x != B * s) return fail(h, MPPI_ERR_INVALID_ARG, who + (h->batch ? "x0 must hold n * s_dim floats" : "x0 must hold s_dim floats"));
    if (n_steps < 1 || n_steps > (1 << 24)) return fail(h, MPPI_ERR_INVALID_ARG, who + "n_steps must be in [1, 2^24]");
    if (h->shard_count != 1) return fail(h, MPPI_ERR_INVALID_ARG, "sharded handle: use mppi_shard_partial / mppi_shard_finish");
    if (!h->no_rollout.empty()) return fail(h, MPPI_ERR_UNSUPPORTED, h->no_rollout);
    if (h->batch && (h->is_gen ? !auv_batch_eligible(h) : !pc_eligible(h)))
        return fail(h, MPPI_ERR_UNSUPPORTED, h->is_gen ? "batched step: the Fossen AUV model runs on k_rollout_auv_pc only"
                                                       : "batched step: the horizon exceeds what this producer count serves (tau <= 132 with 3 producers)");
    MPPI_ENTER(h);
    const size_t n = (size_t)n_steps, xs = (size_t)B * s, us = (size_t)B * a;
    const size_t kScratch = 2 * kHid; // k_mlp_step_ref: 2 * 256 floats per sample; k_nnauv_step_ref: 128
    const size_t oX = 0, oU = oX + (n + 1) * xs, oC = oU + n * us, oG = oC + n * B, oW = oG + (goals ? n * xs : 0), oS = oW + (disturbance ? n * xs : 0);
    if (mppi_status st = ensure_episode_staging(h, oS + kScratch); st != MPPI_OK) return st;
    float *dX = h->d_ep + oX, *dU = h->d_ep + oU, *dC = h->d_ep + oC, *dG = goals ? h->d_ep + oG : nullptr, *dW = disturbance ? h->d_ep + oW : nullptr;
    float *scratch = h->d_ep + oS;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(dX, x0, sizeof(float) * xs, hipMemcpyHostToDevice, st));
    if (dW) HIP_TRY(h, hipMemcpyAsync(dW, disturbance, sizeof(float) * n * xs, hipMemcpyHostToDevice, st));
    if (dG) {
        // goal <- goals[0], as mppi_set_goal / mppi_batch_set_goals before the first step; the later rows are stored by the episode kernel
        HIP_TRY(h, hipMemcpyAsync(dG, goals, sizeof(float) * n * xs, hipMemcpyHostToDevice, st));
        const size_t row = sizeof(float) * s;
        HIP_TRY(h, hipMemcpy2DAsync((char *)h->dC + offsetof(DevConsts, goal), sizeof(DevConsts), dG, row, row, B, hipMemcpyDeviceToDevice, st));
    }
    const int mk = h->hc.model_kind;
    const bool learned = mk == MPPI_MODEL_MLP || mk == MPPI_MODEL_NN_AUV || mk == MPPI_MODEL_NN_AUV_SPEED;
    for (int t = 0; t < n_steps; ++t) {
        const float *x_t = dX + (size_t)t * xs;
        float *u_t = dU + (size_t)t * us, *x_next = dX + (size_t)(t + 1) * xs;
        if (h->batch) {
            if (mppi_status s_ = batch_step(h, st, x_t, u_t); s_ != MPPI_OK) return s_;
        } else {
            TraceRange step_range(h, "mppi:step");
            if (mppi_status s_ = plain_step(h, st, SRC_PHILOX, x_t, nullptr, u_t); s_ != MPPI_OK) return s_;
        }
        TraceRange plant_range(h, "mppi:plant");
        if (mk == MPPI_MODEL_MLP) {
            hipLaunchKernelGGL(k_mlp_step_ref, dim3(1), dim3(64), 0, st, h->dC, h->dM, x_t, 1, (const float *)u_t, 1, scratch, x_next);
            HIP_TRY(h, hipGetLastError());
        } else if (learned) HIP_TRY(h, mppi_gen_model_step(h, st, x_t, 1, u_t, 1, scratch, x_next));
        const mppi_episode_tail e{x_t, u_t, dW ? dW + (size_t)t * xs : nullptr, (dG && t + 1 < n_steps) ? dG + (size_t)(t + 1) * xs : nullptr,
                                  dC + (size_t)t * B, x_next, learned ? 0 : 1};
        HIP_TRY(h, mppi_launch_episode_tail(h, st, e));
    }
    if (X_out) HIP_TRY(h, hipMemcpyAsync(X_out, dX, sizeof(float) * (n + 1) * xs, hipMemcpyDeviceToHost, st));
    if (U_out) HIP_TRY(h, hipMemcpyAsync(U_out, dU, sizeof(float) * n * us, hipMemcpyDeviceToHost, st));
    if (C_out) HIP_TRY(h, hipMemcpyAsync(C_out, dC, sizeof(float) * n * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (goals) for (int i = 0; i < s; ++i) h->hc.goal[i] = goals[(n - 1) * xs + i]; // the host mirror (member 0's)
    return MPPI_OK;
}

extern "C" mppi_status mppi_run_episode(mppi_handle *h, const float *x0, int n_x, int n_steps, const float *goals, const float *disturbance,
                                        float *X_out, float *U_out, float *C_out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (h->batch) return fail(h, MPPI_ERR_UNSUPPORTED, "mppi_run_episode: a batched handle runs its episodes through mppi_batch_run_episode");
    return run_episode(h, "mppi_run_episode", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out);
}

extern "C" mppi_status mppi_batch_run_episode(mppi_handle *h, const float *x0, int n_x, int n_steps, const float *goals, const float *disturbance,
                                              float *X_out, float *U_out, float *C_out)
{
    MPPI_BATCH_ONLY(h);
    return run_episode(h, "mppi_batch_run_episode", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out);
}
