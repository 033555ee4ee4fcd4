// mppi_capi_set.hip — what configures or reads a handle between steps: goal, action limits, sequence filter, tuning switches,
// sequences and the step counter, profiling begin / end, the rollout kernel's name, the sizes. No kernel is launched here.

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "mppi_capi.hip.h"

// ---- roctx ranges (MPPI_TUNE_TRACE): the reference brackets its step with tf.profiler.experimental.start/stop
// (controller_base.py:241-248, 587-595). The marker library is dlopen'ed on first use — rocprofiler-sdk's (what rocprofv3
// --marker-trace records) first, the legacy libroctx64 second — so the product keeps no link dependency on a profiler.
namespace mppi_capi {
bool Roctx::load()
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
Roctx g_roctx;
} // namespace mppi_capi

static mppi_status upload_consts(mppi_handle *h)
{
    HIP_TRY(h, hipMemcpyAsync(h->dC, &h->hc, sizeof(DevConsts), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
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
    case ROUTE_BATCH: name = h->nn_batch == 2 ? (u ? u->batch_mlp_name(h) : nullptr) : h->nn_batch ? mppi_batch_nn_name(h) : h->is_gen ? mppi_batch_auv_name(h) : u ? u->batch_name(h) : nullptr; break;
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
    if (!h || max_steps <= 0 || max_steps > (1 << 20)) return h ? fail(h, MPPI_ERR_INVALID_ARG,
        "max_steps out of range") : MPPI_ERR_INVALID_ARG;
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

// ---- state that a lone handle and a batch keep alike: each accessor serves members(h) members at
// the strides of mppi_handle.hip.h, and the
// public entry points (mppi_* for a lone handle, mppi_batch_* for a batch) are their argument checks plus a call.
// goals [members(h)][s] into the members' constants, the one copy the kernels read; hc mirrors member 0's. A lone handle uploads its whole
// block, so what the host changed in hc goes with the goal.
static mppi_status set_goals(mppi_handle *h, const float *goals)
{
    MPPI_ENTER(h);
    if (h->batch) {
        const size_t row = sizeof(float) * h->s;
        HIP_TRY(h, hipMemcpy2DAsync((char *)h->dC + offsetof(DevConsts, goal), sizeof(DevConsts), goals, row, row, h->batch,
            hipMemcpyHostToDevice, h->stream));
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
                        : ((h->is_gen || h->nn_batch == 2) && what == MPPI_TUNE_MLP32_VALU && value != 0) ? "mlp32_valu"
                        : (h->nn_batch == 2 && what == MPPI_TUNE_MLP_V1 && value != 0) ? "mlp_v1" : nullptr;
        if (why) return fail(h, MPPI_ERR_UNSUPPORTED, std::string("tuning ") + why +
            ": a batched handle always runs the two-launch batched step");
    }
    switch (what) {
    case MPPI_TUNE_FUSED_STEP:
        if (value < 0 || value > 2) return fail(h, MPPI_ERR_INVALID_ARG,
            "fused step: 0 (two launches), 1 (one launch), 2 (one launch, the six-wave workgroup at every horizon)");
        h->fuse_step = value; break;
    case MPPI_TUNE_ARMED_US:
        if (value < 0 || value > 1000000) return fail(h, MPPI_ERR_INVALID_ARG, "armed launch: soft deadline 0 (off) .. 1000000 us");
        if (value > 0 && !h->d_xslot)
            return fail(h, MPPI_ERR_UNSUPPORTED,
                "armed launches need the point-mass producer/consumer path and a large-BAR system (the host stores x straight into device "
                "memory)");
        h->arm_us = value; break;
    case MPPI_TUNE_ARMED_ALWAYS: h->arm_always = value != 0; break;
    case MPPI_TUNE_PRELAUNCH:
        if (value != 0 && !pre_shape_ok(h))
            return fail(h, MPPI_ERR_UNSUPPORTED,
                "the pre-launched step serves the point-mass producer/consumer path with the diagonal quadratic cost, at most one round "
                "of the grid, one shard");
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
        if (h->hc.model_kind != MPPI_MODEL_MLP || h->mlp_bx3 || h->mlp_small) return fail(h, MPPI_ERR_INVALID_ARG,
            "not an exact-fp32 2x256 MLP handle");
        h->mlp_v2 = (value == 0 && h->a <= 3) ? 1 : 0;
        // d_part is sized for the larger count
        h->nb_mlp = h->mlp_v2 ? (h->K_local + kMlp2R - 1) / kMlp2R : (h->K_local + kMlpR - 1) / kMlpR;
        break;
    case MPPI_TUNE_MLP32_VALU:
        if (!(h->mlp_small == 32 || (h->hc.model_kind == MPPI_MODEL_NN_AUV_SPEED && h->mlp_small == 16)) || h->mlp_bx3)
            return fail(h, MPPI_ERR_INVALID_ARG, "not an exact-fp32 Dense(32) MLP handle (or an NNAUVModelSpeed one)");
        if (value < 0 || value > 2)
            return fail(h, MPPI_ERR_INVALID_ARG,
                "0 (matrix cores, two-wave pipeline), 1 (vector-ALU kernel) or 2 (matrix cores, one wave per 32 rollouts)");
        h->mlp32_valu = value; break;
    case MPPI_TUNE_P2P_FAULT:
        if (value < 0 || value > 2) return fail(h, MPPI_ERR_INVALID_ARG, "fault: 0 none, 1 export, 2 probe");
        h->p2p_fault = value; break;
    case MPPI_TUNE_GEN_ONE_WAVE:
        if (h->hc.model_kind != MPPI_MODEL_AUV) return fail(h, MPPI_ERR_INVALID_ARG, "not an AUVModel handle");
        h->gen_one_wave = value != 0; break;
    case MPPI_TUNE_FINISH_GENERIC: h->finish_generic = value != 0; break;
    case MPPI_TUNE_TRACE:
        if (value != 0 && !g_roctx.load()) return fail(h, MPPI_ERR_UNSUPPORTED,
            "MPPI_TUNE_TRACE: neither librocprofiler-sdk-roctx.so nor libroctx64.so could be loaded");
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

extern "C" int mppi_batch_size(const mppi_handle *h) { return h ? h->batch : 0; }

extern "C" mppi_status mppi_batch_set_goals(mppi_handle *h, const float *goals, int n)
{
    MPPI_BATCH_ONLY(h);
    if (!goals || n != h->batch * h->s) return fail(h, MPPI_ERR_INVALID_ARG, "goals must hold n * s_dim floats");
    return set_goals(h, goals);
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
