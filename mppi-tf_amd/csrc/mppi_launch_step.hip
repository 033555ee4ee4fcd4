// mppi_launch_step.hip — instantiates k_step_pc (the whole step in one launch / the armed launch, mppi_step.hip.h) for ONE action
// dimension (-DMPPI_UNIT_A). Diagonal-Q quadratic cost, the step's one pass: the shapes step_shape_ok (mppi_capi.hip.h) admits.
#include "mppi_handle.hip.h"
#include "mppi_step.hip.h"
#ifndef MPPI_UNIT_A
#error "compile with -DMPPI_UNIT_A=<action dimension 1..4> (mppi-tf_amd/build.py)"
#endif

struct StepPick {
    decltype(&k_step_pc<MPPI_UNIT_A, 5, 4, false, STEP_FUSE>) kern; // nullptr: no instance serves the mode
    const char *name;
    int np, nslot;
};

template <int A, int NP, int NSLOT, bool DIAG, int MODE>
static StepPick step_inst()
{
    static const std::string name = mppi_fmt("mppi::k_step_pc<%d, %d, %d, %s, %d>", A, NP, NSLOT, mppi_tf(DIAG), MODE);
    return {k_step_pc<A, NP, NSLOT, DIAG, MODE>, name.c_str(), NP, NSLOT};
}

template <int NP, int MODE>
static StepPick step_np(const mppi_handle *h)
{
    return mppi_with_slots<NP>(h->H, [&](auto ns) { return mppi_with_diag(h, [&](auto d) { return step_inst<MPPI_UNIT_A, NP, decltype(ns)::value, decltype(d)::value, MODE>(); }); });
}

// One workgroup per CU and 3/4 of the chip empty: SEVEN producer waves (two waves on every SIMD, chunks of 28 steps) publish the horizon 1.4x
// sooner than five and the consumer's chain no longer waits for its last chunk — 9.23 -> 8.98 us per step at configs[1], 8.37 -> 8.18 at
// K = 3000 / H = 50 (r05). The pre-launched one-launch step too (two grids in flight fit side by side: at most 2 x (128 + 33) workgroups).
template <int MODE>
static StepPick step_fused(const mppi_handle *h)
{
    if (mppi_step_seven(h)) return mppi_with_diag(h, [&](auto d) { return step_inst<MPPI_UNIT_A, 7, 3, decltype(d)::value, MODE>(); });
    return step_np<5, MODE>(h);
}

static StepPick pick_step(const mppi_handle *h, int mode)
{
    switch (mode) {
    case STEP_FUSE: return step_fused<STEP_FUSE>(h); // <= 128 tiles: the 6-wave (or 8-wave) workgroup, never 3 producers
    case STEP_FUSE | STEP_PRE: return step_fused<STEP_FUSE | STEP_PRE>(h);
    case STEP_FUSE | STEP_ARM: return step_np<5, STEP_FUSE | STEP_ARM>(h);
    // the pre-launched pipelined step: more than 128 tiles (below, the fused step is one launch already)
    case STEP_PRE: return h->pc_np == 3 ? step_np<3, STEP_PRE>(h) : step_np<5, STEP_PRE>(h);
    case STEP_ARM: return h->pc_np == 3 ? step_np<3, STEP_ARM>(h) : step_np<5, STEP_ARM>(h);
    }
    return {nullptr, nullptr, 0, 0}; // (the plain rollout is k_rollout_pc)
}

hipError_t MPPI_CAT(mppi_step_a, MPPI_UNIT_A)(MPPI_STEP_PARAMS)
{
    const bool FUSE = (L->mode & STEP_FUSE) != 0, ARM = (L->mode & STEP_ARM) != 0, PRE = (L->mode & STEP_PRE) != 0;
    if (FUSE && h->pc_np != 5) return hipErrorInvalidValue;
    const StepPick p = pick_step(h, L->mode);
    if (!p.kern) return hipErrorInvalidValue;
    const int NW = p.np + 1;
    const size_t lds = std::max(pc_lds_floats(MPPI_UNIT_A, p.np) * 4 + ((ARM || PRE) ? sizeof(float) * (size_t)h->HA : 0), (size_t)h->pc_lds_min);
    const int nb = (h->K_local + 63) / 64;
    const int ncw = FUSE ? (h->HA + NW - 1) / NW : 0;
    StepArgs sa{};
    sa.recs = h->d_step_recs; sa.nb = nb; sa.nbp = 128; sa.seq = L->seq;
    sa.xslot = h->d_xslot; sa.decision = ARM ? h->d_decision : nullptr;
    sa.host_state = h->d_arm; sa.err = reinterpret_cast<unsigned *>(h->d_arm + 1);
    sa.soft_ticks = (long long)h->arm_us * 100ll;           // s_memrealtime: 100 MHz
    sa.hard_ticks = sa.soft_ticks + 50ll * 100000ll;        // + 50 ms: nothing in this kernel ever spins longer
    sa.U_in = L->U_in; sa.U_out = L->U_out; sa.u_out = L->u_out; sa.step_ctr = h->d_step; sa.dbg = h->d_dbg; sa.clip = h->d_clip;
    sa.neg_inv_lambda = h->hc.neg_inv_lambda; sa.a = h->a; sa.HA = h->HA;
    sa.ugr = L->ugr; sa.utag = L->utag; sa.step_index = L->step_index; sa.cu_ctr = h->d_cu_ctr; sa.ugr_out = L->ugr_out;
    if (PRE) sa.hard_ticks = 20ll * 100000ll; // 20 ms: a sequence that has not come by then never will (sticky error word)
    return mppi_launch(h, kev, p.kern, dim3(nb + ncw), dim3(64 * NW), lds, st, h->dC, L->x_dev, L->U_in, h->d_step, h->d_cost, h->d_part, 1, h->nbp,
                       mppi_pc_balance(h, MPPI_UNIT_A, p.nslot, nb), sa);
}

const char *MPPI_CAT(mppi_step_name_a, MPPI_UNIT_A)(const mppi_handle *h, int mode) { return pick_step(h, mode).name; }
