// mppi_launch_batch.hip — instantiates the batched step (k_rollout_pc_batch + k_finish_cols_batch, mppi_kernels.hip.h) for ONE action
// dimension (-DMPPI_UNIT_A). B controllers, each with its own constants (h->dC[m]), step in the same two launches as one controller.
#include "mppi_handle.hip.h"
#ifndef MPPI_UNIT_A
#error "compile with -DMPPI_UNIT_A=<action dimension 1..4> (mppi-tf_amd/build.py)"
#endif

struct BatchPick {
    decltype(&k_rollout_pc_batch<MPPI_UNIT_A, 5, 4, false, PC_COST_DIAG>) kern;
    const char *name;
    int np, nslot;
};

template <int A, int NP, int NSLOT, bool DIAG, int COST>
static BatchPick batch_inst()
{
    static const std::string name = mppi_fmt("mppi::k_rollout_pc_batch<%d, %d, %d, %s, %d>", A, NP, NSLOT, mppi_tf(DIAG), COST);
    return {k_rollout_pc_batch<A, NP, NSLOT, DIAG, COST>, name.c_str(), NP, NSLOT};
}

// The instance a member's lone handle would launch (mppi_launch_pc.hip): producers by the MEMBER's tile count (h->pc_np, set at create
// exactly as for a plain handle), slots by the horizon. Same NP and NSLOT = the same register layout of the noise, hence the same
// butterfly sums: the member's records are bit for bit those of its lone handle.
template <int NP>
static BatchPick pick_batch_np(const mppi_handle *h)
{
    return mppi_with_slots<NP>(h->H, [&](auto ns) {
        return mppi_with_diag(h, [&](auto d) {
            constexpr int NSLOT = decltype(ns)::value;
            constexpr bool DIAG = decltype(d)::value;
            if (h->hc.q_full) return batch_inst<MPPI_UNIT_A, NP, NSLOT, DIAG, PC_COST_DENSE>();
            return batch_inst<MPPI_UNIT_A, NP, NSLOT, DIAG, PC_COST_DIAG>();
        });
    });
}

static BatchPick pick_batch(const mppi_handle *h) { return h->pc_np == 3 ? pick_batch_np<3>(h) : pick_batch_np<5>(h); }

hipError_t MPPI_CAT(mppi_batch_a, MPPI_UNIT_A)(MPPI_BATCH_PARAMS)
{
    const BatchPick p = pick_batch(h);
    const size_t lds = std::max(pc_lds_floats(MPPI_UNIT_A, p.np) * 4, (size_t)h->pc_lds_min);
    const int nb = (h->K_local + 63) / 64;
    const int tiles = nb * h->batch;
    const PcBatchArgs bt{nb, h->HA + h->a, h->nbp * (2 + h->HA)};
    // roles and head starts as a lone handle's, enabled by the TOTAL tile count: the whole grid must be resident in one round
    return mppi_launch(h, kev, p.kern, dim3(tiles), dim3(64 * (p.np + 1)), lds, st, h->dC, x_dev, h->U_cur(), h->d_step, h->d_cost, h->d_part, 1,
                       h->nbp, mppi_pc_balance(h, MPPI_UNIT_A, p.nslot, tiles), (float *)nullptr, (float *)nullptr, bt);
}

const char *MPPI_CAT(mppi_batch_name_a, MPPI_UNIT_A)(const mppi_handle *h) { return pick_batch(h).name; }

// the finish of every member: one workgroup per (member, column); reads U_in, writes U_out and u_dev [B][a]
hipError_t MPPI_CAT(mppi_batch_finish_a, MPPI_UNIT_A)(MPPI_BATCH_FINISH_PARAMS)
{
    // (MPPI_TUNE_FINISH_GENERIC: the kernel as it was before the column-major fast path, A/B)
    const auto kern = h->finish_generic ? k_finish_cols_batch<MPPI_UNIT_A, false> : k_finish_cols_batch<MPPI_UNIT_A, true>;
    hipExtLaunchKernelGGL(kern, dim3(h->HA * h->batch), dim3(kThreads), 0, st, kev.begin, kev.end, 0, (const float *)h->d_part, h->nbp,
                          h->nbp, h->HA, h->nbp * (2 + h->HA), (const DevConsts *)h->dC, U_in, U_out, h->HA + h->a, u_dev, h->d_step, h->d_dbg,
                          (const float *)h->d_clip);
    return hipGetLastError();
}
