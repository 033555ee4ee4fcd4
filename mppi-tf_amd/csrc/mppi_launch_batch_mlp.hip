// mppi_launch_batch_mlp.hip — instantiates the batched step of the learned point mass with one network per member (mppi_create_batch_mlp;
// mppi_mlp_batch.hip.h) for ONE action dimension (-DMPPI_UNIT_A): k_rollout_mlp2_batch<A, DIAG> (a_dim <= 3: the lone handle runs
// k_rollout_mlp there) and k_rollout_mlp_small_batch<A, 16 | 32>. The finish is k_finish_cols_batch<A> (mppi_launch_batch.hip). Units of
// their own: the lone MLP units' objects stay as they were.
#include "mppi_handle.hip.h"
#include "mppi_mlp_batch.hip.h"
#ifndef MPPI_UNIT_A
#error "compile with -DMPPI_UNIT_A=<action dimension 1..4> (mppi-tf_amd/build.py)"
#endif

// the instance a batch of learned point masses runs, by argument list (exactly one pointer is set), and its geometry: the kernel member
// m's lone handle runs with a member axis — the grid's y for the tile-walking wide kernel, a flat B * nb for the one-wave kernel
struct BatchMlpPick {
    const char *name = nullptr;
    dim3 g, b;
    size_t lds = 0;
    decltype(&k_rollout_mlp2_batch<(MPPI_UNIT_A <= 3 ? MPPI_UNIT_A : 3), false>) wide = nullptr;
    decltype(&k_rollout_mlp_small_batch<MPPI_UNIT_A, 16>) small = nullptr;
};

template <int A>
static BatchMlpPick pick_batch_mlp(const mppi_handle *h)
{
    const int nb = h->nb_mlp;
    if (h->mlp_small) {
        auto small = [&](auto hid) {
            static const std::string name = mppi_fmt("mppi::k_rollout_mlp_small_batch<%d, %d>", A, decltype(hid)::value);
            return mppi_pick_in(&BatchMlpPick::small, k_rollout_mlp_small_batch<A, decltype(hid)::value>, name, dim3(nb * h->batch), dim3(64));
        };
        return h->mlp_small == 16 ? small(std::integral_constant<int, 16>{}) : small(std::integral_constant<int, 32>{});
    }
    if constexpr (A <= 3)
        if (h->mlp_v2)
            return mppi_with_diag(h, [&](auto d) {
                static const std::string name = mppi_fmt("mppi::k_rollout_mlp2_batch<%d, %s>", A, mppi_tf(d));
                return mppi_pick_in(&BatchMlpPick::wide, k_rollout_mlp2_batch<A, decltype(d)::value>, name,
                                    dim3(std::min(nb, h->n_cu), h->batch), dim3(kMlp2Threads), mlp2_lds_floats(2 * A, A, h->H) * 4);
            });
    return BatchMlpPick{};
}

// every member's rollouts in one launch; records in the lone layout per member (element (b, col) at d_part + m * rec_stride + b + col * nbp)
hipError_t MPPI_CAT(mppi_batch_mlp_a, MPPI_UNIT_A)(MPPI_BATCH_PARAMS)
{
    const BatchMlpPick p = pick_batch_mlp<MPPI_UNIT_A>(h);
    const PcBatchArgs bt{h->nb_mlp, h->HA + h->a, h->nbp * (2 + h->HA)};
    if (p.wide) return mppi_launch(h, kev, p.wide, p.g, p.b, p.lds, st, h->dC, h->dM, x_dev, h->U_cur(), h->d_step, h->d_cost, h->d_part, 1, h->nbp, bt);
    if (p.small) return mppi_launch(h, kev, p.small, p.g, p.b, p.lds, st, h->dC, h->dM, h->d_nn_args, x_dev, h->U_cur(), h->d_step, h->d_cost, h->d_part, 1,
                                    h->nbp, bt);
    return hipErrorInvalidValue;
}

const char *MPPI_CAT(mppi_batch_mlp_name_a, MPPI_UNIT_A)(const mppi_handle *h) { return pick_batch_mlp<MPPI_UNIT_A>(h).name; }
