// mppi_launch_pc.hip — instantiates k_rollout_pc (the hot configuration) for ONE action dimension (-DMPPI_UNIT_A).
#include "mppi_handle.hip.h"
#ifndef MPPI_UNIT_A
#error "compile with -DMPPI_UNIT_A=<action dimension 1..4> (mppi-tf_amd/build.py)"
#endif

struct PcPick {
    decltype(&k_rollout_pc<MPPI_UNIT_A, 5, 4, false, PC_COST_DIAG, PC_PASS_PLAIN>) kern;
    const char *name;
    int np, nslot;
};

template <int A, int NP, int NSLOT, bool DIAG, int COST, int PASS>
static PcPick pc_inst()
{
    static const std::string name = mppi_fmt("mppi::k_rollout_pc<%d, %d, %d, %s, %d, %d>", A, NP, NSLOT, mppi_tf(DIAG), COST, PASS);
    return {k_rollout_pc<A, NP, NSLOT, DIAG, COST, PASS>, name.c_str(), NP, NSLOT};
}

// pass: PC_PASS_PLAIN, or the two passes of normalizeCost (an argument of the launch). The weights-only pass
// evaluates no state cost: ONE instance (the diagonal-Q one) serves every cost form.
template <int A, int NP, int NSLOT, bool DIAG, int COST>
static PcPick pc_pass(int pass)
{
    if (pass == PC_PASS_WEIGHTS) return pc_inst<A, NP, NSLOT, DIAG, PC_COST_DIAG, PC_PASS_WEIGHTS>();
    if (pass == PC_PASS_COSTS) return pc_inst<A, NP, NSLOT, DIAG, COST, PC_PASS_COSTS>();
    return pc_inst<A, NP, NSLOT, DIAG, COST, PC_PASS_PLAIN>();
}

// the consumer's cost form: diagonal Q (the hot configuration), ElipseCost (elipse_cost.py:9-85; s >= 4), dense Q (static_cost.py:23-63)
template <int NP>
static PcPick pick_pc_np(const mppi_handle *h, int pass)
{
    constexpr int A = MPPI_UNIT_A;
    return mppi_with_slots<NP>(h->H, [&](auto ns) {
        return mppi_with_diag(h, [&](auto d) {
            constexpr int NSLOT = decltype(ns)::value;
            constexpr bool DIAG = decltype(d)::value;
            if constexpr (A >= 2) {
                if (h->hc.state_cost_kind == MPPI_STATE_COST_ELLIPSE) return pc_pass<A, NP, NSLOT, DIAG, PC_COST_ELLIPSE>(pass);
            }
            if (h->hc.q_full) return pc_pass<A, NP, NSLOT, DIAG, PC_COST_DENSE>(pass);
            // MPPI_FLAG_FP_CONTRACT: the step's one pass with fused multiply-adds (the two passes of normalizeCost keep the plain instances)
            if (h->fp_contract && pass == PC_PASS_PLAIN) return pc_inst<A, NP, NSLOT, DIAG, PC_COST_DIAG_FMA, PC_PASS_PLAIN>();
            return pc_pass<A, NP, NSLOT, DIAG, PC_COST_DIAG>(pass);
        });
    });
}

// MPPI_PC_PRODUCERS=3: the 4-wave variant, kept for A/B timing
static PcPick pick_pc(const mppi_handle *h, int pass) { return h->pc_np == 3 ? pick_pc_np<3>(h, pass) : pick_pc_np<5>(h, pass); }

hipError_t MPPI_CAT(mppi_pc_a, MPPI_UNIT_A)(MPPI_PC_PARAMS)
{
    const PcPick p = pick_pc(h, pass);
    const size_t lds = std::max(pc_lds_floats(MPPI_UNIT_A, p.np) * 4, (size_t)h->pc_lds_min);
    const int nb = (h->K_local + 63) / 64;
    // tile records go out column-major ([2+HA][nb]): the finish kernel reads one column per workgroup
    float *tile_mm = (pass == PC_PASS_WEIGHTS && range_given) ? nullptr : h->d_tile_mm; // (sharded: the agreed range is already in d_mm)
    return mppi_launch(h, kev, p.kern, dim3(nb), dim3(64 * (p.np + 1)), lds, st, h->dC, x_dev, h->U_cur(), h->d_step, h->d_cost, h->d_part, 1, h->nbp,
                       mppi_pc_balance(h, MPPI_UNIT_A, p.nslot, nb), tile_mm, h->d_mm);
}

const char *MPPI_CAT(mppi_pc_name_a, MPPI_UNIT_A)(const mppi_handle *h, int pass) { return pick_pc(h, pass).name; }
