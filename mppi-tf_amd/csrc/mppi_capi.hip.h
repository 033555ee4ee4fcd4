// mppi_capi.hip.h — what the units of the C-ABI share (mppi_capi.hip: creation; mppi_capi_set.hip: setters and accessors;
// mppi_capi_step.hip: the control step; mppi_capi_shard.hip: the K-shard entries; mppi_capi_log.hip: the transition log;
// mppi_capi_debug.hip: debug and helper entries; mppi_step_stats.hip: the step statistics): the error and entry macros, the routing predicates, the profiling slot, what a finish
// takes, and the host functions one unit calls in another. Everything else is static in its unit. A kernel is launched only by the
// unit that defines or instantiates it; another unit calls a host function of the owner.
#pragma once
#include "mppi_handle.hip.h"
#include "mppi_step.hip.h"

#include <cstring>
#include <string>

namespace mppi_capi {

// h->err, or the thread's creation error when there is no handle (what mppi_last_error(NULL) returns): mppi_capi.hip
mppi_status fail(mppi_handle *h, mppi_status st, const std::string &msg);

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e == hipErrorNotSupported && (h) && !((mppi_handle *)(h))->no_rollout.empty())       \
            return fail((h), MPPI_ERR_UNSUPPORTED, ((mppi_handle *)(h))->no_rollout);             \
        if (_e != hipSuccess)                                                                     \
            return fail((h), MPPI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

// the roctx marker library (MPPI_TUNE_TRACE), loaded on first use: mppi_capi_set.hip
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false;
    bool load();
};
extern Roctx g_roctx;
// a range that lasts for the scope; free when the handle does not trace
struct TraceRange {
    bool on;
    TraceRange(const mppi_handle *h, const char *name) : on(h->trace && g_roctx.push) { if (on) g_roctx.push(name); }
    ~TraceRange() { if (on) g_roctx.pop(); }
};

// retire an armed launch and the pre-launched pipeline (mppi_capi_step.hip)
hipError_t quiesce(mppi_handle *h);
// every entry point that touches the device or the handle's stream: make the device current, retire an armed launch
#define MPPI_ENTER(h)                                \
    do {                                             \
        HIP_TRY(h, hipSetDevice((h)->device));       \
        HIP_TRY(h, quiesce(h));                      \
    } while (0)

// a batched handle (mppi_create_batch) has no single x, goal or sequence: the per-member entry points refuse it (mppi_batch_* serve it)
#define MPPI_NOT_BATCH(h, name)                                                                                                       \
    do {                                                                                                                              \
        if ((h) && (h)->batch) return fail((h), MPPI_ERR_UNSUPPORTED,                                                                 \
            std::string(name) + ": a batched handle steps through mppi_batch_*");                                                     \
    } while (0)

#define MPPI_BATCH_ONLY(h)                                                                                          \
    do {                                                                                                            \
        if (!(h)) return MPPI_ERR_INVALID_ARG;                                                                      \
        if (!(h)->batch) return fail((h), MPPI_ERR_INVALID_ARG, "not a batched handle (mppi_create_batch)");        \
    } while (0)

// ---- the launch units' entry points, one row per action dimension (the table: mppi_capi_step.hip)
const mppi_unit_a *unit(const mppi_handle *h);
// the entry point `fn` of the handle's action dimension (none above 4: such a handle runs no rollout kernel)
template <typename... P, typename... Args>
hipError_t per_a(mppi_handle *h, hipError_t (*mppi_unit_a::*fn)(P...), Args... args)
{
    const mppi_unit_a *u = unit(h);
    return u ? (u->*fn)(h, args...) : hipErrorInvalidValue;
}

// the point-mass model with the quadratic (diagonal or dense Q) or the elliptic state cost; horizon
// groups per producer must fit the registers
inline bool pc_eligible(const mppi_handle *h)
{
    const bool cost_ok = h->hc.state_cost_kind == MPPI_STATE_COST_QUADRATIC || (h->hc.state_cost_kind == MPPI_STATE_COST_ELLIPSE &&
        h->s >= 4 && !h->hc.q_full);
    return !h->is_gen && h->no_rollout.empty() && h->R == 64 && !h->force_tile && h->H <= (h->pc_np == 3 ? 132 : 160) && cost_ok;
}

// What k_step_pc (mppi_step.hip.h) serves: the producer/consumer path's hot shape — point mass, diagonal quadratic cost, the step's
// one pass (no normalizeCost), no sequence filter behind the update, one shard.
inline bool step_shape_ok(const mppi_handle *h)
{
    return pc_eligible(h) && h->hc.state_cost_kind == MPPI_STATE_COST_QUADRATIC && !h->hc.q_full && !h->normalize && h->shard_count == 1 &&
           h->sg_window == 0 && h->d_decision != nullptr && !h->fp_contract;
}
// the whole step in ONE launch: at most 128 tiles (K <= 8192), the 6-wave workgroup
inline bool fuse_ok(const mppi_handle *h) { return h->fuse_step && step_shape_ok(h) && h->nb <= 128 && h->pc_np == 5 &&
    h->d_step_recs != nullptr; }
// mppi_next may arm the next step (MPPI_TUNE_ARMED_US > 0, a large-BAR system)
inline bool arm_ok(const mppi_handle *h) { return h->arm_us > 0 && step_shape_ok(h) && h->d_xslot != nullptr; }

// Which kernel family serves the rollout launch a profiled step brackets (ev[0] .. ev[1], mppi_c.h): the batched rollout; the fused
// k_step_pc (whole_step: the caller runs a complete control step, which may be one launch); k_rollout_pc (with normalizeCost its
// weights-only second pass); the learned-model or 13-state kernels; else the tile kernel (with
// normalizeCost, these three run the cost-only pass).
enum Route { ROUTE_BATCH, ROUTE_STEP, ROUTE_PC, ROUTE_TILE, ROUTE_MLP, ROUTE_GEN };
inline Route rollout_route(const mppi_handle *h, int src, const float *noise_out, bool whole_step)
{
    const bool philox = src == SRC_PHILOX && noise_out == nullptr;
    if (h->batch) return ROUTE_BATCH;
    if (whole_step && philox && fuse_ok(h)) return ROUTE_STEP;
    if (h->is_gen) return ROUTE_GEN;
    if (h->hc.model_kind == MPPI_MODEL_MLP) return ROUTE_MLP;
    return philox && pc_eligible(h) ? ROUTE_PC : ROUTE_TILE;
}

// ---- the profiling slot: the one place that knows where a profiled step's events are. The slot index stays on the handle (a sharded step
// spans two C calls: mppi_shard_partial* writes the rollout events of slot prof_n, mppi_shard_finish commits it); the events of the
// launch at hand are handed to it as an argument (mppi_kev).
struct ProfSlot { // the events of the step being enqueued, or none: it is not profiled
    mppi_kev rollout, finish;
    explicit operator bool() const { return rollout.begin != nullptr; }
};
inline ProfSlot prof_slot(mppi_handle *h)
{
    if (h->prof_n >= h->prof_cap) return {};
    hipEvent_t *ev = &h->ev[4 * h->prof_n];
    return {{ev[0], ev[1]}, {ev[2], ev[3]}};
}

// What launch_finish combines and writes: n records (element (b, col) at recs[b*sb + col*sc]) and, if apply, the update:
// U' = U_in + V/eta -> U_out, u_out = U'[0].
struct Finish {
    const float *recs = nullptr;
    int sb = 1, sc = 0, n = 0;
    // the temperature the records were made at where it is not lambda (d_mm + 2: the weights-only pass of
    // normalizeCost); whoever made the records fills it in
    const float *nil_dev = nullptr;
    const float *U_in = nullptr;
    float *U_out = nullptr, *u_out = nullptr, *record_out = nullptr;
    int apply = 1;
    bool xchg = false;      // the finish that exchanges the records with the peers' inboxes first (mppi_shard_p2p_step)
    unsigned armed_seq = 0; // of an armed launch: the finish obeys tile 0's verdict on it
    FinishPre pre = FinishPre{nullptr, nullptr, 0u, 0ull};
};
// the common case: the handle's own d_part (every slot: those no tile owns hold neutral records) onto its own sequence
inline Finish own_records(const mppi_handle *h) { return Finish{h->d_part, 1, h->nbp, h->nbp, nullptr, h->U_cur(), h->U_other()}; }

// What the weights of member `member`'s last step were made from (a lone handle: member 0) — the one selection MPPI_DBG_WEIGHTS
// (mppi_capi_debug.hip) and the step statistics (mppi_step_stats.hip) share: the costs that were weighed (a lone handle's two-pass
// normalizeCost: the raw costs at the step's temperature = the normalised costs at lambda), beta | eta, the member's constants (lambda)
// and where the temperature is when it is not lambda.
struct WeightInputs { const DevConsts *consts; const float *cost_w, *beta_eta, *nil_dev; };
inline WeightInputs weight_inputs(const mppi_handle *h, int member)
{
    const float *cost = h->d_cost + (size_t)h->K_local * member;
    return {h->dC + member, (h->normalize && !h->norm_two_pass) ? (const float *)h->d_cost2 : cost, h->d_dbg + 8 * (size_t)member,
            h->norm_two_pass ? (const float *)(h->d_mm + 2) : (const float *)nullptr};
}

//  pc_eligible's horizon bound depends on pc_np, and pc_np on THIS shard's tile count (or a per-handle tuning): with
// 132 < H <= 160 and ragged shards straddling 512 tiles one rank would make raw-cost records at the range temperature and another
// normalised-cost records at lambda. A sharded handle therefore takes the fast form only below the bound that holds for every pc_np: the
// form depends on the configuration only, never on the shard's size, and all ranks make their records in the same units.
inline bool norm_fast(const mppi_handle *h) { return h->hc.model_kind != MPPI_MODEL_MLP && !h->is_gen && pc_eligible(h) &&
    (h->shard_count == 1 || h->H <= 132); }
inline Route norm_route(const mppi_handle *h, int src, const float *noise_out)
{
    const Route r = rollout_route(h, src, noise_out, false);
    return r == ROUTE_PC && !norm_fast(h) ? ROUTE_TILE : r;
}

// (one round of the grid: a rollout with workgroups still undispatched while the NEXT step's waiting
// workgroups hold the slots would never finish)
inline int pre_slots(const mppi_handle *h)
{
    const int per_cu = h->pc_np == 3 ? (mppi_pc_slots(3, h->H) == 6 && 6 * 4 * h->a <= 80 ? 4 : 2) : 3; // k_step_pc's __launch_bounds__
    return per_cu * h->n_cu;
}
inline bool pre_shape_ok(const mppi_handle *h) { return step_shape_ok(h) && (fuse_ok(h) ||
    (h->nb > 128 && h->nb <= pre_slots(h))) && h->d_arm != nullptr; }
inline bool pre_ok(const mppi_handle *h) { return h->prelaunch && pre_shape_ok(h); }

// the Fossen AUV model on its two-wave rollout (k_rollout_auv_pc, every horizon) with the step's one pass: what k_rollout_auv_pc_batch runs
inline bool auv_batch_eligible(const mppi_handle *h)
{
    return h->is_gen && h->hc.model_kind == MPPI_MODEL_AUV && !h->gen_one_wave && !h->normalize && h->shard_count == 1;
}

// a batch of learned 13-state controllers (mppi_create_batch_learned): what k_rollout_nn_batch runs
inline bool nn_batch_eligible(const mppi_handle *h)
{
    return h->is_gen && h->nn_batch == 1 && h->d_nn_args != nullptr && !h->normalize && h->shard_count == 1 && !h->mlp_bx3;
}
// a batch of learned point masses (mppi_create_batch_mlp): what k_rollout_mlp2_batch / k_rollout_mlp_small_batch run
inline bool mlp_batch_eligible(const mppi_handle *h)
{
    return !h->is_gen && h->nn_batch == 2 && h->hc.model_kind == MPPI_MODEL_MLP && h->no_rollout.empty() && (h->mlp_small ? h->d_nn_args != nullptr
        : h->mlp_v2 != 0) && !h->normalize && h->shard_count == 1 && !h->mlp_bx3;
}
// the batched step serves the handle (why not: batch_step's message)
inline bool batch_eligible(const mppi_handle *h)
{
    return h->nn_batch == 2 ? mlp_batch_eligible(h) : h->nn_batch ? nn_batch_eligible(h) : h->is_gen ? auv_batch_eligible(h) : pc_eligible(h);
}

// ---- host functions of mppi_capi_step.hip that other units call (comments at the definitions)
hipError_t launch_tile(mppi_handle *h, const DevConsts *consts, hipStream_t st, int src, int mode, const float *x_dev, const float *U_dev,
                       const float *eps, float *cost, float *part, float *noise_out);
hipError_t launch_finish(mppi_handle *h, hipStream_t st, Finish f);
hipError_t ensure_record_layout(mppi_handle *h, hipStream_t st, int n_tiles);
void fill_neutral_records(hipStream_t st, float *recs, int nbp, int ncol);
void range_apply(mppi_handle *h, hipStream_t st, const float *range_dev);
mppi_status norm_costs(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, const float *x_dev, const float *eps,
                       float *noise_out, float *range_out);
mppi_status norm_records(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, const float *x_dev, const float *eps,
                         bool range_given, Finish *made);
mppi_status enqueue_partials(mppi_handle *h, hipStream_t st, int src, const float *x_dev, const float *eps, float *noise_out, Finish *made);
mppi_status ensure_eps(mppi_handle *h);
mppi_status finish_step(mppi_handle *h, hipStream_t st, const Finish &f);
mppi_status plain_step(mppi_handle *h, hipStream_t st, int src, const float *x_dev, const float *eps, float *u_dev, bool xchg = false);
// ---- ... and of mppi_capi_debug.hip: one launch of k_mlp_step_ref, 64 samples per workgroup (the learned point-mass model as a plant).
// member_stride 0: one network (h->dM) for every row; 1: row i through the network of member i (a learned batch as its own plant)
void mlp_step_ref(mppi_handle *h, hipStream_t st, const float *x, int kx, const float *v, int k, float *scratch, float *out_next,
                  int member_stride = 0);
// ---- ... and of mppi_step_stats.hip. step_stats_refusal: why the handle's last step has no statistics (NULL: it has; *st the status) —
// a sharded handle, 2^24 or more samples per member. launch_step_stats: ONE launch of k_step_stats behind a step on `st`, a workgroup per
// member: stats [B][9], hist_cost [B][32], hist_weight [B][32], device pointers, all three required.
const char *step_stats_refusal(const mppi_handle *h, mppi_status *st);
hipError_t launch_step_stats(mppi_handle *h, hipStream_t st, float *stats, uint32_t *hist_cost, uint32_t *hist_weight);

} // namespace mppi_capi
using namespace mppi_capi;
