// mppi_model_rollout.hip — open-loop rollouts of the handle's model (mppi_model_rollout / mppi_model_rollout_device, include/mppi_c.h):
// n given action sequences of T steps each, every state and its state cost written out, in one call with no host wait inside. One LANE
// per trajectory, 64-thread workgroups, a grid of ceil(n / 64); the step loop over T runs inside the kernel with the state in registers.
// For trajectory i it
//   reads  x0[kx == 1 ? 0 : i] and V[t, i] for t = 0 .. T-1 (the load of V[t+1] is issued before step t is computed: the serial chain of a
//          trajectory does not pay a memory latency per step),
//   writes X[0, i] = x0, X[t+1, i] = model(X[t, i], V[t, i]) and C[t, i] = the state cost of X[t+1, i] under the handle's goal — the
//          POST-step state, the one the rollout kernels charge (mppi_kernels.hip.h: "cost on the POST-step state"). C = NULL: no cost
//          arithmetic.
// The step axis comes first and the trajectory axis after it (the episodes' X[n_steps+1, B, s]): the 64 lanes of a wave read V[t, i0..i0+63]
// and write X[t+1, i0..i0+63] as contiguous runs. The model and the cost are the device functions behind mppi_model_step and
// mppi_state_cost, in the expression order of k_model_step / k_costs (the point mass) and k_auv_step / k_gen_costs (the 13-state family),
// compiled like them with -ffp-contract=off: the same bits. Plain vector loads and stores; no LDS, no cross-lane operation, no flag, no
// spin, nothing waits on another workgroup: any n is safe, resident in one round of the chip or not.
// A learned model (MPPI_MODEL_MLP, NN_AUV, NN_AUV_SPEED) is stepped by its existing exactly-ordered reference kernel (k_mlp_step_ref,
// k_nnauv_step_ref), T launches from row t to row t + 1 of X; ONE launch of the kernels here then runs cost-only (model = 0): one lane per
// (t, i) pair finds X[t+1, i] in place and writes C[t, i], no recurrence (and the first n lanes store X[0]). A learned model's trajectory
// here is therefore the REFERENCE-ORDERED evaluation, as with mppi_model_step: the matrix-core rollout kernels of a control step round
// differently. The per-row scratch of the reference kernels lives on the handle (d_mr), grown on demand, freed by mppi_destroy.
// The two entry points are at the end of this file.
#define MPPI_UNIT_BATCH_GEN // (mppi_gen.hip.h: its non-template kernels live in the gen unit)
#include "mppi_capi.hip.h"
#include "mppi_gen.hip.h"
#include "mppi_model_rollout.hip.h"

namespace {

constexpr int kRolloutThreads = 64;

template <int A, bool QFULL>
__global__ void k_model_rollout_pm(const DevConsts *__restrict__ C, const mppi_model_rollout_args r)
{
    constexpr int S = 2 * A;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)r.n;
    if (!r.model) { // cost-only: lane = (t, i) pair t * n + i, whose state is row t + 1 of X
        if (i < n) {
#pragma unroll
            for (int j = 0; j < S; ++j) r.X[i * S + j] = r.x0[(r.kx == 1 ? 0 : i) * S + j];
        }
        if (r.C == nullptr || i >= n * (size_t)r.T) return;
        float xs[S];
#pragma unroll
        for (int j = 0; j < S; ++j) xs[j] = r.X[(n + i) * S + j];
        r.C[i] = state_cost_of<S, QFULL>(C, xs);
        return;
    }
    if (i >= n) return;
    float xs[S], vn[A];
#pragma unroll
    for (int j = 0; j < S; ++j) xs[j] = r.x0[(r.kx == 1 ? 0 : i) * S + j];
#pragma unroll
    for (int j = 0; j < A; ++j) vn[j] = r.V[i * A + j];
#pragma unroll
    for (int j = 0; j < S; ++j) r.X[i * S + j] = xs[j];
    for (int t = 0; t < r.T; ++t) {
        float vs[A], fr[S], ac[S];
#pragma unroll
        for (int j = 0; j < A; ++j) vs[j] = vn[j];
        if (t + 1 < r.T) { // the next step's action, in flight while this step is computed
#pragma unroll
            for (int j = 0; j < A; ++j) vn[j] = r.V[((size_t)(t + 1) * n + i) * A + j];
        }
        pm_free_step<A>(C, xs, fr);
        pm_action_step<A>(C, vs, ac);
#pragma unroll
        for (int j = 0; j < S; ++j) xs[j] = fr[j] + ac[j];
        const size_t row = (size_t)(t + 1) * n + i;
#pragma unroll
        for (int j = 0; j < S; ++j) r.X[row * S + j] = xs[j];
        if (r.C != nullptr) r.C[(size_t)t * n + i] = state_cost_of<S, QFULL>(C, xs);
    }
}

__global__ void k_model_rollout_gen(const DevConsts *__restrict__ C, const GenConsts *__restrict__ G, const mppi_model_rollout_args r)
{
    constexpr int S = kGenS, A = kGenA;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)r.n;
    if (!r.model) { // cost-only: lane = (t, i) pair t * n + i, whose state is row t + 1 of X
        if (i < n) {
#pragma unroll
            for (int j = 0; j < S; ++j) r.X[i * S + j] = r.x0[(r.kx == 1 ? 0 : i) * S + j];
        }
        if (r.C == nullptr || i >= n * (size_t)r.T) return;
        float xs[S];
#pragma unroll
        for (int j = 0; j < S; ++j) xs[j] = r.X[(n + i) * S + j];
        r.C[i] = gen_state_cost(C, G, xs);
        return;
    }
    if (i >= n) return;
    float xs[S], vn[A];
#pragma unroll
    for (int j = 0; j < S; ++j) xs[j] = r.x0[(r.kx == 1 ? 0 : i) * S + j];
#pragma unroll
    for (int j = 0; j < A; ++j) vn[j] = r.V[i * A + j];
#pragma unroll
    for (int j = 0; j < S; ++j) r.X[i * S + j] = xs[j];
    for (int t = 0; t < r.T; ++t) {
        float vs[A];
#pragma unroll
        for (int j = 0; j < A; ++j) vs[j] = vn[j];
        if (t + 1 < r.T) { // the next step's action, in flight while this step is computed
#pragma unroll
            for (int j = 0; j < A; ++j) vn[j] = r.V[((size_t)(t + 1) * n + i) * A + j];
        }
        auv_step(G, xs, vs); // xs is X[t+1, i] now
        const size_t row = (size_t)(t + 1) * n + i;
#pragma unroll
        for (int j = 0; j < S; ++j) r.X[row * S + j] = xs[j];
        if (r.C != nullptr) r.C[(size_t)t * n + i] = gen_state_cost(C, G, xs);
    }
}

template <int A>
void launch_pm(mppi_handle *h, hipStream_t st, dim3 g, const mppi_model_rollout_args &r)
{
    if (h->hc.q_full) hipLaunchKernelGGL((k_model_rollout_pm<A, true>), g, dim3(kRolloutThreads), 0, st, (const DevConsts *)h->dC, r);
    else hipLaunchKernelGGL((k_model_rollout_pm<A, false>), g, dim3(kRolloutThreads), 0, st, (const DevConsts *)h->dC, r);
}

bool learned_model(const mppi_handle *h)
{
    const int mk = h->hc.model_kind;
    return mk == MPPI_MODEL_MLP || mk == MPPI_MODEL_NN_AUV || mk == MPPI_MODEL_NN_AUV_SPEED;
}

// floats of reference-kernel scratch per row: k_mlp_step_ref 2 * kHid, k_nnauv_step_ref 128
size_t scratch_per_row(const mppi_handle *h) { return h->hc.model_kind == MPPI_MODEL_MLP ? (size_t)2 * kHid : 128; }

// the handle's scratch for n rows on the stream `st`. It is one buffer: a call on another stream than the last one's first waits for that
// stream (the two calls' step kernels would otherwise share the rows), and so does growing it, before the old buffer is freed.
mppi_status ensure_scratch(mppi_handle *h, hipStream_t st, size_t floats)
{
    if (h->d_mr != nullptr && (h->mr_stream != st || floats > h->mr_cap)) HIP_TRY(h, hipStreamSynchronize(h->mr_stream));
    if (floats > h->mr_cap) {
        if (h->d_mr) { HIP_TRY(h, hipFree(h->d_mr)); h->d_mr = nullptr; h->mr_cap = 0; }
        HIP_TRY(h, hipMalloc((void **)&h->d_mr, sizeof(float) * floats));
        h->mr_cap = floats;
    }
    h->mr_stream = st;
    return MPPI_OK;
}

// every refusal of both entry points, before anything is enqueued
mppi_status check(mppi_handle *h, const char *name, const float *x0, int kx, const float *V, int n, int T, bool has_out, const char *no_out)
{
    const std::string who = std::string(name) + ": ";
    if (h->batch) return fail(h, MPPI_ERR_UNSUPPORTED, who + "a batched handle shares one model: roll it on a lone handle");
    if (!x0 || !V) return fail(h, MPPI_ERR_INVALID_ARG, who + "x0 is [kx, s_dim] and V [T, n, a_dim]: NULL pointer");
    if (n < 1 || T < 1) return fail(h, MPPI_ERR_INVALID_ARG, who + "n and T must be >= 1");
    if ((size_t)n * (size_t)T > ((size_t)1 << 30)) return fail(h, MPPI_ERR_INVALID_ARG, who + "n * T must not exceed 2^30");
    if (kx != 1 && kx != n) return fail(h, MPPI_ERR_INVALID_ARG, who + "x0 is [kx, s_dim] with kx in {1, n}");
    if (!has_out) return fail(h, MPPI_ERR_INVALID_ARG, who + no_out);
    if (h->gen ? (h->s != kGenS || h->a != kGenA) : (h->s != 2 * h->a || h->a < 1 || h->a > 4))
        return fail(h, MPPI_ERR_UNSUPPORTED, who + "the rollout kernels serve the point-mass layout (s_dim = 2 a_dim, a_dim <= 4) and the "
            "13-state family");
    return MPPI_OK;
}

mppi_status enqueue(mppi_handle *h, hipStream_t st, const float *x0, int kx, const float *V, int n, int T, float *X, float *C)
{
    const size_t s = (size_t)h->s, a = (size_t)h->a;
    if (!learned_model(h)) {
        HIP_TRY(h, mppi_launch_model_rollout(h, st, mppi_model_rollout_args{x0, V, X, C, kx, n, T, 1}));
        return MPPI_OK;
    }
    if (mppi_status e = ensure_scratch(h, st, (size_t)n * scratch_per_row(h)); e != MPPI_OK) return e;
    for (int t = 0; t < T; ++t) { // step 0 reads x0 itself (kx rows); X[0] is stored by the cost launch behind the steps
        const float *x_t = t == 0 ? x0 : X + (size_t)t * n * s, *v_t = V + (size_t)t * n * a;
        float *x_next = X + (size_t)(t + 1) * n * s;
        if (h->hc.model_kind == MPPI_MODEL_MLP) {
            mlp_step_ref(h, st, x_t, t == 0 ? kx : n, v_t, n, h->d_mr, x_next);
            HIP_TRY(h, hipGetLastError());
        } else HIP_TRY(h, mppi_gen_model_step(h, st, x_t, t == 0 ? kx : n, v_t, n, h->d_mr, x_next));
    }
    HIP_TRY(h, mppi_launch_model_rollout(h, st, mppi_model_rollout_args{x0, V, X, C, kx, n, T, 0}));
    return MPPI_OK;
}

struct DevBuf {
    float *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(float) * (n ? n : 1)); }
};

} // namespace

hipError_t mppi_launch_model_rollout(mppi_handle *h, hipStream_t st, const mppi_model_rollout_args &r)
{
    // model = 1: a lane per trajectory; model = 0: a lane per (t, i) pair (no cost output: the n lanes that store X[0])
    const size_t lanes = r.model ? (size_t)r.n : (r.C != nullptr ? (size_t)r.n * (size_t)r.T : (size_t)r.n);
    const dim3 g((unsigned)((lanes + kRolloutThreads - 1) / kRolloutThreads));
    if (h->gen != nullptr) {
        if (h->s != kGenS || h->a != kGenA) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_model_rollout_gen, g, dim3(kRolloutThreads), 0, st, (const DevConsts *)h->dC,
                           static_cast<const GenConsts *>(mppi_gen_dev_consts(h)), r);
        return hipGetLastError();
    }
    if (h->s != 2 * h->a) return hipErrorInvalidValue;
    switch (h->a) {
    case 1: launch_pm<1>(h, st, g, r); break;
    case 2: launch_pm<2>(h, st, g, r); break;
    case 3: launch_pm<3>(h, st, g, r); break;
    case 4: launch_pm<4>(h, st, g, r); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" mppi_status mppi_model_rollout_device(mppi_handle *h, const float *x0_dev, int kx, const float *V_dev, int n, int T,
                                                 float *X_dev, float *C_dev, void *stream)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (mppi_status e = check(h, "mppi_model_rollout_device", x0_dev, kx, V_dev, n, T, X_dev != nullptr,
                              "X_dev is required (a learned model steps from row to row of it)"); e != MPPI_OK) return e;
    MPPI_ENTER(h);
    return enqueue(h, stream ? (hipStream_t)stream : h->stream, x0_dev, kx, V_dev, n, T, X_dev, C_dev);
}

extern "C" mppi_status mppi_model_rollout(mppi_handle *h, const float *x0, int kx, const float *V, int n, int T, float *X_out, float *C_out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (mppi_status e = check(h, "mppi_model_rollout", x0, kx, V, n, T, X_out != nullptr || C_out != nullptr,
                              "X_out and C_out are both NULL"); e != MPPI_OK) return e;
    MPPI_ENTER(h);
    const size_t s = (size_t)h->s, a = (size_t)h->a, rows = (size_t)n * (size_t)T;
    DevBuf dx, dV, dX, dC;
    HIP_TRY(h, dx.alloc((size_t)kx * s)); HIP_TRY(h, dV.alloc(rows * a)); HIP_TRY(h, dX.alloc((rows + (size_t)n) * s));
    if (C_out) HIP_TRY(h, dC.alloc(rows));
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(dx.p, x0, sizeof(float) * (size_t)kx * s, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(dV.p, V, sizeof(float) * rows * a, hipMemcpyHostToDevice, st));
    if (mppi_status e = mppi_model_rollout_device(h, dx.p, kx, dV.p, n, T, dX.p, dC.p, nullptr); e != MPPI_OK) {
        (void)hipStreamSynchronize(st); // (the scratch buffers are freed on return)
        return e;
    }
    if (X_out) HIP_TRY(h, hipMemcpyAsync(X_out, dX.p, sizeof(float) * (rows + (size_t)n) * s, hipMemcpyDeviceToHost, st));
    if (C_out) HIP_TRY(h, hipMemcpyAsync(C_out, dC.p, sizeof(float) * rows, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return MPPI_OK;
}
