// mppi_launch_batch.hip — instantiates the batched step (k_rollout_pc_batch + k_finish_cols_batch, mppi_kernels.hip.h) for ONE action
// dimension (-DMPPI_UNIT_A). B controllers that share one configuration step in the same two launches as one controller.
#include "mppi_handle.hip.h"
#ifndef MPPI_UNIT_A
#error "compile with -DMPPI_UNIT_A=<action dimension 1..4> (mppi-tf_amd/build.py)"
#endif

// The instance a member's lone handle would launch (launch_pc in mppi_launch_pc.hip): producers by the MEMBER's tile count (h->pc_np, set at
// create exactly as for a plain handle), slots by the horizon. Same NP and NSLOT = the same register layout of the noise, hence the same
// butterfly sums: the member's records are bit for bit those of its lone handle.
template <int A, int NP, int NSLOT, int COST>
static hipError_t launch_batch_inst(mppi_handle *h, hipStream_t st, const float *x_dev)
{
    const size_t lds = std::max(pc_lds_floats(A, NP) * 4, (size_t)h->pc_lds_min);
    const int nb = (h->K_local + 63) / 64;
    const int tiles = nb * h->batch;
    const dim3 g(tiles), b(64 * (NP + 1));
    // roles and head starts as launch_pc_pass, enabled by the TOTAL tile count: the whole grid must be resident in one round
    const int bias = h->pc_bias >= 0 ? h->pc_bias : ((NSLOT * 4 * A <= 80) ? 0x033a : 0x0369);
    const int balance = (tiles <= 4 * 256 && !h->pc_no_balance) ? (1 | (bias << 8)) : 0;
    const PcBatchArgs bt{h->d_seeds, h->d_goals, nb, h->HA + h->a, h->nbp * (2 + h->HA)};
    const void *fn = h->sigma_diag ? reinterpret_cast<const void *>(k_rollout_pc_batch<A, NP, NSLOT, true, COST>)
                                   : reinterpret_cast<const void *>(k_rollout_pc_batch<A, NP, NSLOT, false, COST>);
    if (hipError_t e = mppi_raise_lds_ceiling(fn, h->device, lds); e != hipSuccess) return e;
    float *const no_mm = nullptr;
    if (h->sigma_diag) hipExtLaunchKernelGGL((k_rollout_pc_batch<A, NP, NSLOT, true, COST>), g, b, (uint32_t)lds, st, h->kev0, h->kev1, 0, h->dC, x_dev, h->U_cur(), h->d_step, h->d_cost, h->d_part, 1, h->nbp, balance, no_mm, no_mm, bt);
    else hipExtLaunchKernelGGL((k_rollout_pc_batch<A, NP, NSLOT, false, COST>), g, b, (uint32_t)lds, st, h->kev0, h->kev1, 0, h->dC, x_dev, h->U_cur(), h->d_step, h->d_cost, h->d_part, 1, h->nbp, balance, no_mm, no_mm, bt);
    return hipGetLastError();
}

template <int A, int NP, int NSLOT>
static hipError_t launch_batch_cost(mppi_handle *h, hipStream_t st, const float *x_dev)
{
    if (h->hc.q_full) return launch_batch_inst<A, NP, NSLOT, PC_COST_DENSE>(h, st, x_dev);
    return launch_batch_inst<A, NP, NSLOT, PC_COST_DIAG>(h, st, x_dev);
}

hipError_t MPPI_CAT(mppi_launch_batch_a, MPPI_UNIT_A)(MPPI_PC_PARAMS)
{
    constexpr int AA = MPPI_UNIT_A;
    const int NG = (h->H + 3) / 4;
    if (h->pc_np == 3) return NG <= 18 ? launch_batch_cost<AA, 3, 6>(h, st, x_dev) : launch_batch_cost<AA, 3, 11>(h, st, x_dev);
    return NG <= 20 ? launch_batch_cost<AA, 5, 4>(h, st, x_dev) : launch_batch_cost<AA, 5, 8>(h, st, x_dev);
}

// the finish of every member: one workgroup per (member, column); reads U_in, writes U_out and u_dev [B][a]
hipError_t MPPI_CAT(mppi_launch_batch_finish_a, MPPI_UNIT_A)(MPPI_BATCH_FINISH_PARAMS)
{
    hipExtLaunchKernelGGL(k_finish_cols_batch<MPPI_UNIT_A>, dim3(h->HA * h->batch), dim3(kThreads), 0, st, ev0, ev1, 0, (const float *)h->d_part, h->nbp,
                          h->nbp, h->HA, h->nbp * (2 + h->HA), h->hc.neg_inv_lambda, U_in, U_out, h->HA + h->a, u_dev, h->d_step, h->d_dbg,
                          (const float *)h->d_clip);
    return hipGetLastError();
}
