// mppi_episode_plant.hip — the plant of a closed-loop episode when it is ANOTHER handle's model (mppi_run_episode_plant /
// mppi_batch_run_episode_plant, mppi_capi_step.hip): the kernels of mppi_episode.hip with the model step taken from the member's plant
// constants. One LANE per member of the controller. For member m it
//   reads  x_t, the step's u_t, the disturbance w_t, the goal of step t + 1 and plants[m], the pointer to its plant's constants,
//   writes C[t] = the state cost of x_t under the CONTROLLER's cost and goal (mppi_state_cost's value on the controller),
//          x_{t+1} = plant_m(x_t, u_t) [+ w_t] into the next row of the trajectory,
//          goal_{t+1} into the controller member's DevConsts.goal.
// The plant's step is pm_free_step + pm_action_step (the point mass: k_model_step's expression order) or auv_step (the Fossen model:
// k_auv_step's) on the plant's constants, compiled like them with -ffp-contract=off: the bits of mppi_model_step on the plant handle.
// A plant is only read. Plain vector loads and stores.
#define MPPI_UNIT_BATCH_GEN // (mppi_gen.hip.h: its non-template kernels live in the gen unit)
#include "mppi_episode_plant.hip.h"
#include "mppi_gen.hip.h"

namespace {

constexpr int kEpisodeThreads = 64;

template <int A, bool QFULL>
__global__ void k_episode_pm_plant(DevConsts *consts, const DevConsts *const *plants, int B, const mppi_episode_tail e)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    constexpr int S = 2 * A;
    DevConsts *C = consts + m;
    const DevConsts *P = plants[m]; // (may be C itself: the controller as its own plant)
    float xs[S], vs[A], fr[S], ac[S], xn[S];
#pragma unroll
    for (int j = 0; j < S; ++j) xs[j] = e.x[(size_t)m * S + j];
#pragma unroll
    for (int j = 0; j < A; ++j) vs[j] = e.u[(size_t)m * A + j];
    e.cost[m] = state_cost_of<S, QFULL>(C, xs);
    pm_free_step<A>(P, xs, fr);
    pm_action_step<A>(P, vs, ac);
#pragma unroll
    for (int j = 0; j < S; ++j) xn[j] = fr[j] + ac[j];
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

__global__ void k_episode_gen_plant(DevConsts *consts, const GenConsts *__restrict__ G, const GenConsts *const *plants, int B,
                                    const mppi_episode_tail e)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= B) return;
    constexpr int S = kGenS, A = kGenA;
    DevConsts *C = consts + m;
    const GenConsts *P = plants[m];
    float xs[S], vs[A];
#pragma unroll
    for (int j = 0; j < S; ++j) xs[j] = e.x[(size_t)m * S + j];
#pragma unroll
    for (int j = 0; j < A; ++j) vs[j] = e.u[(size_t)m * A + j];
    e.cost[m] = gen_state_cost(C, G, xs);
    auv_step(P, xs, vs); // xs is x_{t+1} now
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
void launch_pm(mppi_handle *h, hipStream_t st, dim3 g, const DevConsts *const *plants, int B, const mppi_episode_tail &e)
{
    if (h->hc.q_full) hipLaunchKernelGGL((k_episode_pm_plant<A, true>), g, dim3(kEpisodeThreads), 0, st, h->dC, plants, B, e);
    else hipLaunchKernelGGL((k_episode_pm_plant<A, false>), g, dim3(kEpisodeThreads), 0, st, h->dC, plants, B, e);
}

} // namespace

hipError_t mppi_launch_episode_tail_plant(mppi_handle *h, hipStream_t st, const void *const *plants, const mppi_episode_tail &e)
{
    const int B = members(h);
    const dim3 g((B + kEpisodeThreads - 1) / kEpisodeThreads);
    if (plants == nullptr) return hipErrorInvalidValue;
    if (h->gen != nullptr) {
        if (h->s != kGenS || h->a != kGenA) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_episode_gen_plant, g, dim3(kEpisodeThreads), 0, st, h->dC, static_cast<const GenConsts *>(mppi_gen_dev_consts(h)),
                           reinterpret_cast<const GenConsts *const *>(plants), B, e);
        return hipGetLastError();
    }
    if (h->s != 2 * h->a) return hipErrorInvalidValue;
    const DevConsts *const *pm = reinterpret_cast<const DevConsts *const *>(plants);
    switch (h->a) {
    case 1: launch_pm<1>(h, st, g, pm, B, e); break;
    case 2: launch_pm<2>(h, st, g, pm, B, e); break;
    case 3: launch_pm<3>(h, st, g, pm, B, e); break;
    case 4: launch_pm<4>(h, st, g, pm, B, e); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
