// mppi_launch_batch_nn.hip — instantiates the batched step of the learned 13-state models with one network per member:
// k_rollout_nn_batch<MODEL, HID, DIAG> (mppi_nn_batch.hip.h), MODEL in {NNAUVModel, NNAUVModelSpeed}, HID in {16, 32}: eight instances.
// The finish is k_finish_cols_batch<6>, launched by mppi_launch_batch_finish_auv (mppi_launch_batch_gen.hip). A unit of its own: the gen
// unit's object stays as it was.
#define MPPI_UNIT_BATCH_GEN // (mppi_gen.hip.h: its non-template kernels live in the gen unit)
#include "mppi_handle.hip.h"
#include "mppi_nn_batch.hip.h"

// the instance a learned batch runs: the model and the hidden width of the handle, the sigma form of member 0 (shared by all)
static auto pick_batch_nn(const mppi_handle *h)
{
    using std::integral_constant;
    struct Pick { decltype(&k_rollout_nn_batch<GEN_MODEL_NNAUV, 32, false>) kern; const char *name; };
    auto inst = [&](auto model, auto w) {
        return mppi_with_diag(h, [&](auto d) {
            constexpr int MODEL = decltype(model)::value, W = decltype(w)::value;
            static const std::string name = mppi_fmt("mppi::k_rollout_nn_batch<%d, %d, %s>", MODEL, W, mppi_tf(d));
            return Pick{k_rollout_nn_batch<MODEL, W, decltype(d)::value>, name.c_str()};
        });
    };
    auto hid = [&](auto model) { return h->mlp_small == 16 ? inst(model, integral_constant<int, 16>{}) : inst(model, integral_constant<int, 32>{}); };
    if (h->hc.model_kind == MPPI_MODEL_NN_AUV_SPEED) return hid(integral_constant<int, GEN_MODEL_NNAUV_SPEED>{});
    return hid(integral_constant<int, GEN_MODEL_NNAUV>{});
}

// Every member's rollouts: one flat grid of B * nb one-wave workgroups, as mppi_launch_gen's k_rollout_gen launch per member.
hipError_t mppi_launch_batch_nn(MPPI_BATCH_PARAMS)
{
    const PcBatchArgs bt{h->nb, h->HA + h->a, h->nbp * (2 + h->HA)};
    const GenConsts *G = static_cast<const GenConsts *>(mppi_gen_dev_consts(h));
    return mppi_launch(h, kev, pick_batch_nn(h).kern, dim3(h->nb * h->batch), dim3(64), 0, st, h->dC, G, h->dM, h->d_nn_args, x_dev, h->U_cur(),
                       h->d_step, h->d_cost, h->d_part, 1, h->nbp, bt);
}

const char *mppi_batch_nn_name(const mppi_handle *h) { return pick_batch_nn(h).name; }
