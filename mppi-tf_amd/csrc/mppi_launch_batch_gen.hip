// mppi_launch_batch_gen.hip — instantiates the batched step of the Fossen AUV model: k_rollout_auv_pc_batch (mppi_gen.hip.h) and
// k_finish_cols_batch<6> (mppi_kernels.hip.h). B AUV controllers that share one configuration step in the same two launches as one
// controller. A unit of its own: the gen unit's object stays as it was, and the longest compile of the parallel build stays where it is.
#define MPPI_UNIT_BATCH_GEN // (mppi_gen.hip.h: its non-template kernels live in the gen unit)
#include "mppi_handle.hip.h"
#include "mppi_gen.hip.h"

static auto pick_batch_auv(const mppi_handle *h)
{
    struct Pick { decltype(&k_rollout_auv_pc_batch<false>) kern; const char *name; };
    return mppi_with_diag(h, [&](auto d) {
        static const std::string name = mppi_fmt("mppi::k_rollout_auv_pc_batch<%s>", mppi_tf(d));
        return Pick{k_rollout_auv_pc_batch<decltype(d)::value>, name.c_str()};
    });
}

// Every member's rollouts: one flat grid of B * W workgroups, W = (nb + 1) / 2 per member (two tiles per workgroup), as mppi_launch_gen's
// k_rollout_auv_pc launch per member. The SIMD-true roles are enabled by the TOTAL workgroup count, as the lone launcher decides them.
hipError_t mppi_launch_batch_auv(MPPI_BATCH_PARAMS)
{
    const int wgs = (h->nb + 1) / 2 * h->batch;
    const PcBatchArgs bt{h->nb, h->HA + h->a, h->nbp * (2 + h->HA)};
    const GenConsts *G = static_cast<const GenConsts *>(mppi_gen_dev_consts(h));
    return mppi_launch(h, kev, pick_batch_auv(h).kern, dim3(wgs), dim3(kAuvPcThreads), 0, st, h->dC, G, x_dev, h->U_cur(), h->d_step, h->d_cost,
                       h->d_part, 1, h->nbp, h->nb, mppi_two_tile_balance(h, wgs), bt);
}

const char *mppi_batch_auv_name(const mppi_handle *h) { return pick_batch_auv(h).name; }

// the finish of every member: one workgroup per (member, column); reads U_in, writes U_out and u_dev [B][6]
hipError_t mppi_launch_batch_finish_auv(MPPI_BATCH_FINISH_PARAMS)
{
    // (MPPI_TUNE_FINISH_GENERIC: the kernel as it was before the column-major fast path, A/B)
    const auto kern = h->finish_generic ? k_finish_cols_batch<kGenA, false> : k_finish_cols_batch<kGenA, true>;
    hipExtLaunchKernelGGL(kern, dim3(h->HA * h->batch), dim3(kThreads), 0, st, kev.begin, kev.end, 0, (const float *)h->d_part, h->nbp,
                          h->nbp, h->HA, h->nbp * (2 + h->HA), (const DevConsts *)h->dC, U_in, U_out, h->HA + h->a, u_dev, h->d_step, h->d_dbg,
                          (const float *)h->d_clip);
    return hipGetLastError();
}
