// mppi_launch_mlp.hip — instantiates the learned-model rollout kernels (k_rollout_mlp, _mlp2, _mlp_bx3, _mlp32, _mlp_small) for
// ONE action dimension (-DMPPI_UNIT_A).
#include "mppi_handle.hip.h"
#ifndef MPPI_UNIT_A
#error "compile with -DMPPI_UNIT_A=<action dimension 1..4> (mppi-tf_amd/build.py)"
#endif

// the instance, by argument list (exactly one pointer is set), and its geometry
struct MlpPick {
    const char *name = nullptr;
    dim3 g, b;
    size_t lds = 0;
    decltype(&k_rollout_mlp<MPPI_UNIT_A, false>) plain = nullptr;              // k_rollout_mlp, _mlp32, _mlp32_bx3
    decltype(&k_rollout_mlp32_pc<MPPI_UNIT_A, false>) pipe = nullptr;          // ... + (tile count, balance): k_rollout_mlp32_pc
    decltype(&k_rollout_mlp_small<MPPI_UNIT_A, 16>) small = nullptr;           // ... + the scalar-cache weights: k_rollout_mlp_small
    decltype(&k_rollout_mlp_bx3<MPPI_UNIT_A, false, SRC_HBM>) nosrc = nullptr; // the noise source a template argument: k_rollout_mlp2, _mlp_bx3
};

template <int A>
static MlpPick pick_mlp(const mppi_handle *h, int src)
{
    const int nb = h->nb_mlp;
    if (h->mlp_small == 32 && h->mlp_bx3) { // ... on the bf16 matrix cores, every operand split in two (MPPI_FLAG_MLP_BF16X3)
        static const std::string name = mppi_fmt("mppi::k_rollout_mlp32_bx3<%d>", A);
        return mppi_pick_in(&MlpPick::plain, k_rollout_mlp32_bx3<A>, name, dim3(nb), dim3(kMlp32Threads));
    }
    if (h->mlp_small == 32 && h->mlp32_valu == 0) // default (r04): the two-wave pipeline (network wave + cost wave per tile, two tiles per workgroup)
        return mppi_with_diag(h, [&](auto d) {
            static const std::string name = mppi_fmt("mppi::k_rollout_mlp32_pc<%d, %s>", A, mppi_tf(d));
            return mppi_pick_in(&MlpPick::pipe, k_rollout_mlp32_pc<A, decltype(d)::value>, name, dim3((nb + 1) / 2), dim3(kMlp32PcThreads));
        });
    if (h->mlp_small == 32 && h->mlp32_valu == 2) { // MPPI_TUNE_MLP32_VALU = 2: one wave per 32 rollouts, 2 waves per tile (A/B timing)
        static const std::string name = mppi_fmt("mppi::k_rollout_mlp32<%d>", A);
        return mppi_pick_in(&MlpPick::plain, k_rollout_mlp32<A>, name, dim3(nb), dim3(kMlp32Threads));
    }
    if (h->mlp_small) { // one wave = one 64-rollout tile, weights through the scalar cache
        auto small = [&](auto hid) {
            static const std::string name = mppi_fmt("mppi::k_rollout_mlp_small<%d, %d>", A, decltype(hid)::value);
            return mppi_pick_in(&MlpPick::small, k_rollout_mlp_small<A, decltype(hid)::value>, name, dim3(nb), dim3(64));
        };
        return h->mlp_small == 16 ? small(std::integral_constant<int, 16>{}) : small(std::integral_constant<int, 32>{});
    }
    // the exact-fp32 2x256 network. Injected noise (API helpers, tests) runs one instance, the dense-Sigma arithmetic (exact for a
    // diagonal Sigma too: it adds 0 * z terms)
    auto by_src = [&](auto make) {
        if (src == SRC_PHILOX) return mppi_with_diag(h, [&](auto d) { return make(d, std::integral_constant<int, SRC_PHILOX>{}); });
        if (src == SRC_HBM) return make(std::false_type{}, std::integral_constant<int, SRC_HBM>{});
        return MlpPick{};
    };
    if (h->mlp_bx3) // one tile-walking workgroup of 4 waves per CU
        return by_src([&](auto d, auto s) {
            static const std::string name = mppi_fmt("mppi::k_rollout_mlp_bx3<%d, %s, %d>", A, mppi_tf(d), decltype(s)::value);
            return mppi_pick_in(&MlpPick::nosrc, k_rollout_mlp_bx3<A, decltype(d)::value, decltype(s)::value>, name, dim3(std::min(nb, h->n_cu)),
                            dim3(kBx3Threads), bx3_lds_floats(2 * A, A, h->H) * 4);
        });
    if (h->mlp_v2) {
        if constexpr (A <= 3)
            return by_src([&](auto d, auto s) {
                static const std::string name = mppi_fmt("mppi::k_rollout_mlp2<%d, %s, %d>", A, mppi_tf(d), decltype(s)::value);
                return mppi_pick_in(&MlpPick::nosrc, k_rollout_mlp2<A, decltype(d)::value, decltype(s)::value>, name, dim3(std::min(nb, h->n_cu)),
                                dim3(kMlp2Threads), mlp2_lds_floats(2 * A, A, h->H) * 4);
            });
        return MlpPick{};
    }
    return mppi_with_diag(h, [&](auto d) {
        static const std::string name = mppi_fmt("mppi::k_rollout_mlp<%d, %s>", A, mppi_tf(d));
        return mppi_pick_in(&MlpPick::plain, k_rollout_mlp<A, decltype(d)::value>, name, dim3(nb), dim3(kMlpThreads), mlp_lds_floats(2 * A, A) * 4);
    });
}

hipError_t MPPI_CAT(mppi_mlp_a, MPPI_UNIT_A)(MPPI_MLP_PARAMS)
{
    if (mode != MODE_ROLLOUT && mode != MODE_COST_ONLY) return hipErrorInvalidValue;
    const MlpPick p = pick_mlp<MPPI_UNIT_A>(h, src);
    if (p.plain) return mppi_launch(h, kev, p.plain, p.g, p.b, p.lds, st, h->dC, h->dM, x_dev, U_dev, eps, h->d_step, cost, h->d_part, src, mode, 1, h->nbp);
    if (p.pipe)
        return mppi_launch(h, kev, p.pipe, p.g, p.b, p.lds, st, h->dC, h->dM, x_dev, U_dev, eps, h->d_step, cost, h->d_part, src, mode, 1, h->nbp, h->nb_mlp,
                           mppi_two_tile_balance(h, (int)p.g.x));
    if (p.small) return mppi_launch(h, kev, p.small, p.g, p.b, p.lds, st, h->dC, h->dM, h->small_args, x_dev, U_dev, eps, h->d_step, cost, h->d_part, src, mode, 1, h->nbp);
    if (p.nosrc) return mppi_launch(h, kev, p.nosrc, p.g, p.b, p.lds, st, h->dC, h->dM, x_dev, U_dev, eps, h->d_step, cost, h->d_part, mode, 1, h->nbp);
    return hipErrorInvalidValue;
}

const char *MPPI_CAT(mppi_mlp_name_a, MPPI_UNIT_A)(const mppi_handle *h, int src) { return pick_mlp<MPPI_UNIT_A>(h, src).name; }
