// mppi_episode_plant.hip.h — the launch behind a control step of an episode whose plant is ANOTHER handle's analytic model
// (mppi_run_episode_plant / mppi_batch_run_episode_plant, mppi_capi_step.hip; the kernels: mppi_episode_plant.hip).
#pragma once
#include "mppi_handle.hip.h"

// mppi_launch_episode_tail with the model step taken from the plants: plants[m] is the constants block that member m's state is stepped
// with — a `const DevConsts *` (the point mass: a lone plant handle's dC) or a `const GenConsts *` (the Fossen model: mppi_gen_dev_consts
// of the plant handle), B device pointers in device memory; a shared plant repeats one pointer. The cost and the next goal stay the
// controller's. e.model is not read: a learned plant is stepped by its own kernel and closed by the plain tail (model = 0).
hipError_t mppi_launch_episode_tail_plant(mppi_handle *h, hipStream_t st, const void *const *plants, const mppi_episode_tail &e);
