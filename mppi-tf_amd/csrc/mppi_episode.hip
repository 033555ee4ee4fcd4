// mppi_episode.hip — the plant of a closed-loop episode (mppi_run_episode / mppi_batch_run_episode, mppi_capi_step.hip): the one launch that
// follows a control step and closes the loop on the device. One LANE per member of the handle (a lone handle: one lane). For member m it
//   reads  x_t, the step's u_t, the disturbance w_t and the goal of step t + 1,
//   writes C[t] = the state cost of x_t under the goal still in force (mppi_state_cost's value),
//          x_{t+1} = model(x_t, u_t) [+ w_t] into the next row of the trajectory, which is the next step's x_dev,
//          goal_{t+1} into the member's DevConsts.goal (what mppi_set_goal / mppi_batch_set_goals would have stored).
// The model and the cost are the device functions behind mppi_model_step and mppi_state_cost, in the expression order of k_model_step /
// k_costs (the point mass) and k_auv_step / k_gen_costs (the 13-state family), compiled like them with -ffp-contract=off: the same bits.
// A learned model is stepped by its existing reference kernel (k_mlp_step_ref, k_nnauv_step_ref) in a launch of its own; the kernel here
// then finds x_{t+1} in place (model = 0) and adds the rest. Plain vector loads and stores.
#define MPPI_UNIT_BATCH_GEN // (mppi_gen.hip.h: its non-template kernels live in the gen unit)
#include "mppi_handle.hip.h"
#include "mppi_gen.hip.h"

namespace {

constexpr int kEpisodeThreads = 64;

template <int A, bool QFULL>
__global__ void k_episode_pm(DevConsts *consts, int B, const mppi_episode_tail e)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    constexpr int S = 2 * A;
    DevConsts *C = consts + m;
    float xs[S], vs[A], xn[S];
#pragma unroll
    for (int j = 0; j < S; ++j) xs[j] = e.x[(size_t)m * S + j];
#pragma unroll
    for (int j = 0; j < A; ++j) vs[j] = e.u[(size_t)m * A + j];
    e.cost[m] = state_cost_of<S, QFULL>(C, xs);
    if (e.model) {
        float fr[S], ac[S];
        pm_free_step<A>(C, xs, fr);
        pm_action_step<A>(C, vs, ac);
#pragma unroll
        for (int j = 0; j < S; ++j) xn[j] = fr[j] + ac[j];
    } else {
#pragma unroll
        for (int j = 0; j < S; ++j) xn[j] = e.x_next[(size_t)m * S + j];
    }
    if (e.w != nullptr) {
#pragma unroll
        for (int j = 0; j < S; ++j) xn[j] = xn[j] + e.w[(size_t)m * S + j];
    }
#pragma unroll
    for (int j = 0; j < S; ++j) e.x_next[(size_t)m * S + j] = xn[j];
    if (e.goal_next != nullptr) {
#pragma unroll
        for (int j = 0; j < S; ++j) C->goal[j] = e.goal_next[(size_t)m * S + j];
    }
}

__global__ void k_episode_gen(DevConsts *consts, const GenConsts *__restrict__ G, int B, const mppi_episode_tail e)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    constexpr int S = kGenS, A = kGenA;
    DevConsts *C = consts + m;
    float xs[S], vs[A];
#pragma unroll
    for (int j = 0; j < S; ++j) xs[j] = e.x[(size_t)m * S + j];
#pragma unroll
    for (int j = 0; j < A; ++j) vs[j] = e.u[(size_t)m * A + j];
    e.cost[m] = gen_state_cost(C, G, xs);
    if (e.model) {
        auv_step(G, xs, vs); // xs is x_{t+1} now
    } else {
#pragma unroll
        for (int j = 0; j < S; ++j) xs[j] = e.x_next[(size_t)m * S + j];
    }
    if (e.w != nullptr) {
#pragma unroll
        for (int j = 0; j < S; ++j) xs[j] = xs[j] + e.w[(size_t)m * S + j];
    }
#pragma unroll
    for (int j = 0; j < S; ++j) e.x_next[(size_t)m * S + j] = xs[j];
    if (e.goal_next != nullptr) {
#pragma unroll
        for (int j = 0; j < S; ++j) C->goal[j] = e.goal_next[(size_t)m * S + j];
    }
}

template <int A>
void launch_pm(mppi_handle *h, hipStream_t st, dim3 g, int B, const mppi_episode_tail &e)
{
    if (h->hc.q_full) hipLaunchKernelGGL((k_episode_pm<A, true>), g, dim3(kEpisodeThreads), 0, st, h->dC, B, e);
    else hipLaunchKernelGGL((k_episode_pm<A, false>), g, dim3(kEpisodeThreads), 0, st, h->dC, B, e);
}

} // namespace

hipError_t mppi_launch_episode_tail(mppi_handle *h, hipStream_t st, const mppi_episode_tail &e)
{
    const int B = members(h);
    const dim3 g((B + kEpisodeThreads - 1) / kEpisodeThreads);
    if (h->gen != nullptr) {
        if (h->s != kGenS || h->a != kGenA) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_episode_gen, g, dim3(kEpisodeThreads), 0, st, h->dC, static_cast<const GenConsts *>(mppi_gen_dev_consts(h)), B, e);
        return hipGetLastError();
    }
    if (h->s != 2 * h->a) return hipErrorInvalidValue;
    switch (h->a) {
    case 1: launch_pm<1>(h, st, g, B, e); break;
    case 2: launch_pm<2>(h, st, g, B, e); break;
    case 3: launch_pm<3>(h, st, g, B, e); break;
    case 4: launch_pm<4>(h, st, g, B, e); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
