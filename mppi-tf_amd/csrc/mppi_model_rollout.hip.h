// mppi_model_rollout.hip.h — the launcher of the open-loop model rollout (mppi_model_rollout.hip), declared for whoever enqueues one.
#pragma once
#include "mppi_handle.hip.h"

// One open-loop rollout of the handle's model along n action sequences (device pointers): x0 [kx, s] with kx in {1, n}, V [T, n, a] ->
// X [T+1, n, s], C [T, n] (NULL: no cost arithmetic). model = 1: the kernel steps the handle's analytic model itself, one lane per
// trajectory, the step loop inside; model = 0 (a learned model): rows 1..T of X are in place already, and the launch only adds C, one lane
// per (t, i) pair.
struct mppi_model_rollout_args {
    const float *x0, *V; // x0 [kx, s], V [T, n, a]
    float *X, *C;        // X [T+1, n, s], C [T, n] or NULL
    int kx, n, T, model;
};
hipError_t mppi_launch_model_rollout(mppi_handle *h, hipStream_t st, const mppi_model_rollout_args &r);
