// mppi_capi_step.hip — everything a control step executes on the host: the launch engine (rollout, finish, record layout, the two
// passes of normalizeCost), the plain, fused, armed and pre-launched step protocols, step_host with its spin on the pinned slot,
// mppi_next*, the batched step and the closed-loop episode driver. One unit, so that the per-step path inlines as one.
// Kernels of this unit: k_fill_records, k_combine_group, k_finish_cols, k_finish_cols_xchg, k_savgol, k_cost_minmax, k_range_apply,
// k_cost_normalize.

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#define MPPI_UNIT_CAPI_STEP 1
#include "mppi_capi.hip.h"
#include "mppi_episode_plant.hip.h"

namespace mppi_capi {

// ---- armed launches (mppi_step.hip.h) ---------------------------------------------------------------------------------
// The host stores into fine-grained device memory directly (large BAR); the stores of one call are fenced out of the write-combining
// buffers before anything waits on their effect.
static inline void store_fence()
{
#if defined(__x86_64__)
    __builtin_ia32_sfence();
#else
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}
static inline void xslot_store(mppi_handle *h, int i, float v, unsigned tag)
{
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    __atomic_store_n(reinterpret_cast<volatile unsigned long long *>(h->d_xslot) + i,
        ((unsigned long long)tag << 32) | (unsigned long long)bits, __ATOMIC_RELAXED);
}
// An armed launch nobody is going to feed (any entry point other than mppi_next, a handle that changes, destroy): the host's cancel
// tag makes tile 0 abort at its next poll; every wave follows, the update is not applied, the stream drains. U, u and the Philox step
// counter are exactly what they were before the launch was armed.
// ... and the pre-launched pipeline (MPPI_TUNE_PRELAUNCH): steps are in flight on both streams; once
// both have drained, the plain U buffers,
// the step counter and u are what the plain path would have left. A sequence that never came (hard deadline) is in the sticky error word.
static hipError_t pre_quiesce(mppi_handle *h)
{
    if (!h->pre_active) return hipSuccess;
    h->pre_active = false;
    if (hipError_t e = hipStreamSynchronize(h->stream); e != hipSuccess) return e;
    if (hipError_t e = hipStreamSynchronize(h->stream2); e != hipSuccess) return e;
    if (h->h_arm && reinterpret_cast<volatile unsigned *>(h->h_arm + 1)[0] != 0u) {
        reinterpret_cast<volatile unsigned *>(h->h_arm + 1)[0] = 0u;
        h->err = "a pre-launched step never received its sequence (hard deadline): the controls since are invalid";
        return hipErrorLaunchTimeOut;
    }
    return hipSuccess;
}
hipError_t quiesce(mppi_handle *h)
{
    if (hipError_t e = pre_quiesce(h); e != hipSuccess) return e;
    if (!h->arm_inflight) return hipSuccess;
    xslot_store(h, 0, 0.0f, h->arm_seq | mppi::kArmCancelBit);
    store_fence();
    h->arm_inflight = false;
    return hipStreamSynchronize(h->stream);
}

// kernel dispatch: the rollout kernels are instantiated in their own translation units (mppi_launch_*.hip, one per
// kernel family and action dimension, compiled in parallel); mppi_handle.hip.h declares their entry points, one row per action dimension.
#define MPPI_UNIT_ROW(N)                                                                                                  \
    {mppi_tile_a##N, mppi_pc_a##N, mppi_mlp_a##N, mppi_step_a##N, mppi_batch_a##N, mppi_batch_finish_a##N, mppi_tile_name_a##N, \
     mppi_pc_name_a##N, mppi_mlp_name_a##N, mppi_step_name_a##N, mppi_batch_name_a##N, mppi_batch_mlp_a##N, mppi_batch_mlp_name_a##N}
static const mppi_unit_a kUnits[4] = {MPPI_UNIT_ROW(1), MPPI_UNIT_ROW(2), MPPI_UNIT_ROW(3), MPPI_UNIT_ROW(4)};
#undef MPPI_UNIT_ROW
const mppi_unit_a *unit(const mppi_handle *h) { return h->a >= 1 && h->a <= 4 ? &kUnits[h->a - 1] : nullptr; }

hipError_t launch_tile(mppi_handle *h, const DevConsts *consts, hipStream_t st, int src, int mode, const float *x_dev, const float *U_dev,
                              const float *eps, float *cost, float *part, float *noise_out)
{
    if (!h->no_rollout.empty()) return hipErrorNotSupported;
    return per_a(h, &mppi_unit_a::tile, consts, st, src, mode, x_dev, U_dev, eps, cost, part, noise_out);
}

static void prof_commit(mppi_handle *h, hipStream_t st) { h->prof_stream = st; h->prof_n++; }
// a profiled step that is one launch has no finish launch: an empty finish interval, and the step is recorded
static hipError_t prof_one_launch(mppi_handle *h, ProfSlot p, hipStream_t st)
{
    if (!p) return hipSuccess;
    if (hipError_t e = hipEventRecord(p.finish.begin, st); e != hipSuccess) return e;
    if (hipError_t e = hipEventRecord(p.finish.end, st); e != hipSuccess) return e;
    prof_commit(h, st);
    return hipSuccess;
}

// One rollout launch on `route`, through the 13-state, learned-model, producer/consumer or tile launcher, on the handle's own sequence,
// records and constants. kev: the profiled step's rollout events or none — the dispatch's own begin / end, except that the tile kernel
// takes none and gets them recorded around its launch (`around`: so does any route). pass, range_given: k_rollout_pc's (MPPI_PC_PARAMS).
static hipError_t launch_rollout(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, int mode,
                                 const float *x_dev, const float *eps,
                                 float *cost, float *noise_out, int pass = PC_PASS_PLAIN, bool range_given = false, bool around = false)
{
    const bool record = kev.begin && (around || route == ROUTE_TILE);
    const mppi_kev own = record ? mppi_kev{} : kev;
    hipError_t e = record ? hipEventRecord(kev.begin, st) : hipSuccess;
    if (e != hipSuccess) return e;
    switch (route) {
    case ROUTE_GEN: e = mppi_launch_gen(h, h->dC, st, own, src, mode, x_dev, h->U_cur(), eps, cost, h->d_part, noise_out); break;
    case ROUTE_MLP: e = per_a(h, &mppi_unit_a::mlp, st, own, src, mode, x_dev, (const float *)h->U_cur(), eps, cost); break;
    case ROUTE_PC: e = per_a(h, &mppi_unit_a::pc, st, own, x_dev, pass, range_given); break;
    case ROUTE_TILE: e = launch_tile(h, h->dC, st, src, mode, x_dev, h->U_cur(), eps, cost, h->d_part, noise_out); break;
    default: e = hipErrorInvalidValue;
    }
    // records were made: from the raw costs at the range's temperature (the weights-only pass of normalizeCost), else at lambda
    if (mode == MODE_ROLLOUT || mode == MODE_COSTS_GIVEN) h->norm_two_pass = route == ROUTE_PC && pass == PC_PASS_WEIGHTS;
    if (e == hipSuccess && record) e = hipEventRecord(kev.end, st);
    return e;
}

// Which instance of k_finish_cols_cm finishes these records, or -1: k_finish_cols. The fast path takes column-major records that fit a
// thread's four slots (the tile records of a step; the folded records above 1024 tiles and the gathered shard records are row-major)
// with at most one of the optional inputs: the verdict of an armed launch, the granules of a pre-launched one, a temperature on the device.
static int finish_cm_mode(const mppi_handle *h, const Finish &f)
{
    if (h->finish_generic || f.sb != 1 || f.n < 1 || f.n > 4 * kThreads || h->a < 1) return -1;
    const bool armed = f.armed_seq != 0, pre = f.pre.in != nullptr, norm = f.nil_dev != nullptr;
    if ((int)armed + (int)pre + (int)norm > 1 || (pre && f.pre.out == nullptr) || (f.pre.out != nullptr && !pre)) return -1;
    return armed ? FIN_ARMED : pre ? FIN_PRE : norm ? FIN_NORM : FIN_PLAIN;
}

// More than 1024 records are first folded 16:1 (k_combine_group) into row-major scratch.
hipError_t launch_finish(mppi_handle *h, hipStream_t st, Finish f)
{
    // a profiled step = the rollout kernel + the finish that applies the update
    TraceRange tr(h, f.apply ? "mppi:finish" : "mppi:record");
    const ProfSlot p = f.apply ? prof_slot(h) : ProfSlot{};
    // The levels alternate between the two scratch buffers, so that no level reads the buffer it writes: level 1 fills d_part2
    // (ceil(nbp/16) records), level 2 d_part3 (1/16 of that), level 3 d_part2 again (1/256 of it), ...
    float *out = h->d_part2, *other = h->d_part3;
    while (f.n > 1024) {
        const int ng = (f.n + kGroup - 1) / kGroup;
        hipLaunchKernelGGL(k_combine_group, dim3(ng), dim3(kThreads), 0, st, f.recs, f.sb, f.sc, f.n, h->HA,
            h->hc.neg_inv_lambda, out, f.nil_dev);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        f.recs = out; f.sb = 2 + h->HA; f.sc = 1; f.n = ng;
        std::swap(out, other);
    }
    // profiled: the finish kernel's own dispatch begin/end (hipExtLaunchKernel events), like the
    // rollout kernel's
    const mppi_kev kev = p.finish;
    if (f.xchg)
        hipExtLaunchKernelGGL(k_finish_cols_xchg, dim3(h->HA), dim3(kThreads), 0, st, kev.begin, kev.end, 0, f.recs,
                              f.sb, f.sc, f.n, h->HA, h->a,
                              h->hc.neg_inv_lambda, f.U_in, f.U_out, f.u_out, h->d_step, h->d_dbg, h->xchg_peers, h->shard_count,
                              h->shard_rank, ++h->xchg_seq,
                              h->xchg_timeout_ticks, h->d_xchg_status, h->d_xchg_dead, (const float *)h->d_clip);
    else if (const int mode = finish_cm_mode(h, f); mode >= 0) {
        // column-major records, one optional input at most: the instance of that protocol (k_finish_cols_cm)
        const auto kern = mode == FIN_ARMED ? k_finish_cols_cm<FIN_ARMED> : mode == FIN_PRE ? k_finish_cols_cm<FIN_PRE>
                        : mode == FIN_NORM ? k_finish_cols_cm<FIN_NORM> : k_finish_cols_cm<FIN_PLAIN>;
        hipExtLaunchKernelGGL(kern, dim3(h->HA), dim3(kThreads), 0, st, kev.begin, kev.end, 0, f.recs, f.sc, f.n, h->HA, h->a,
                              (1ull << 32) / (unsigned long long)h->a + 1ull, h->hc.neg_inv_lambda, f.U_in, f.U_out, f.u_out,
                              f.record_out, f.apply, h->d_step, h->d_dbg, (const float *)h->d_clip, f.nil_dev,
                              (const unsigned long long *)h->d_decision, f.armed_seq, f.pre);
    } else
        hipExtLaunchKernelGGL(k_finish_cols, dim3(h->HA), dim3(kThreads), 0, st, kev.begin, kev.end, 0, f.recs,
                              f.sb, f.sc, f.n, h->HA, h->a,
                              h->hc.neg_inv_lambda, f.U_in, f.U_out, f.u_out, f.record_out, f.apply, h->d_step, h->d_dbg,
                              (const float *)h->d_clip, f.nil_dev,
                              f.armed_seq ? (const unsigned long long *)h->d_decision
                                  : (const unsigned long long *)nullptr, f.armed_seq, f.pre);
    hipError_t e = hipGetLastError();
    if (p && e == hipSuccess) prof_commit(h, st);
    return e;
}

// After the update: the shifted sequence becomes the warm start (a pointer offset), then the optional
// Savitzky-Golay smoothing (filterSeq) writes the filtered sequence into the other buffer.
static hipError_t advance_sequence(mppi_handle *h, hipStream_t st)
{
    h->U_advance();
    if (h->sg_window > 0) {
        hipLaunchKernelGGL(k_savgol, dim3((h->HA + 255) / 256), dim3(256), 0, st, h->U_cur(), h->U_other(), h->d_sg_rows,
                           h->d_sg_start, h->H, h->a, h->sg_window);
        h->u_cur = 1 - h->u_cur;
        h->u_off = 0;
    }
    return hipGetLastError();
}

// The slots of d_part that hold records belong to ONE tile count at a time (the MLP kernels and the tile kernel of the same
// handle may cut K differently): when the count changes, every slot goes back to the neutral record first.
hipError_t ensure_record_layout(mppi_handle *h, hipStream_t st, int n_tiles)
{
    if (h->part_nb == n_tiles) return hipSuccess;
    if (h->part_nb != 0)
        hipLaunchKernelGGL(k_fill_records, dim3((h->nbp * (2 + h->HA) + 255) / 256), dim3(256), 0, st, h->d_part, h->nbp, 2 + h->HA);
    h->part_nb = n_tiles;
    return hipGetLastError();
}

// every slot of one record block [ncol][nbp] neutral (creation: each member's block)
void fill_neutral_records(hipStream_t st, float *recs, int nbp, int ncol)
{
    hipLaunchKernelGGL(k_fill_records, dim3((unsigned)(((size_t)nbp * ncol + 255) / 256)), dim3(256), 0, st, recs, nbp, ncol);
}

// ---- Py normalizeCost (controller_base.py:468-474): costs, global min/max, then the update on c' = (c-min)/(max-min) with the SAME noise
// (regenerated from the same Philox counters). Two halves, which an unsharded step (enqueue_partials) runs back to back and a K-sharded
// one as two calls with the ranks' agreement on the range between them (mppi_shard_cost_range, mppi_shard_partial_normalized).
// Fast form on the producer/consumer kernel (ROUTE_PC): exp(-(c' - min c')/lambda) = exp(-(c - min
// c)/(lambda (max - min))), so the normalised
// update is the plain one at another temperature. A pass at lambda for the costs; then the weights-only pass (PC_PASS_WEIGHTS, r04): no
// rollouts — the weights from the stored costs, the noise regenerated for the weighted sums; records at the range's temperature, which the
// finish reads from d_mm[2] (r03: a full second rollout pass, 42 us at C3; the tile kernel's two passes 76). Else: cost pass,
// k_cost_normalize, record pass from the normalised costs at lambda.

// First half: the costs into d_cost. range_out (the sharded calls): this shard's {-min, max} goes there as well. Fast form: unsharded, the
// PC_PASS_COSTS pass, every tile leaving its (min, max) in d_tile_mm; with range_out the plain pass
// (its records, at lambda, are overwritten
// by the second half) and k_cost_minmax. Else the cost-only pass, which a profiled step brackets (kev:
// the dominant launch), and k_cost_minmax.
mppi_status norm_costs(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, const float *x_dev, const float *eps,
    float *noise_out, float *range_out)
{
    if (route == ROUTE_PC) HIP_TRY(h, launch_rollout(h, st, route, mppi_kev{}, src, MODE_ROLLOUT, x_dev, eps, h->d_cost, noise_out,
        range_out ? PC_PASS_PLAIN : PC_PASS_COSTS));
    else HIP_TRY(h, launch_rollout(h, st, route, kev, src, MODE_COST_ONLY, x_dev, eps, h->d_cost, noise_out, PC_PASS_PLAIN, false, true));
    if (route == ROUTE_PC && !range_out) return MPPI_OK;
    hipLaunchKernelGGL(k_cost_minmax, dim3(1), dim3(1024), 0, st, h->d_cost, h->K_local, h->d_mm, 0.0f, (float *)nullptr, range_out);
    HIP_TRY(h, hipGetLastError());
    return MPPI_OK;
}

// Second half: the records from the costs of the first, and where the finish finds their temperature (made->nil_dev). Fast form: the
// weights-only pass (kev: a profiled step reports this pass, the one whose records are used); range_given: the range is in d_mm already.
// Else from the costs normalised with the range in d_mm; a learned point-mass model's records come from the tile kernel.
mppi_status norm_records(mppi_handle *h, hipStream_t st, Route route, mppi_kev kev, int src, const float *x_dev, const float *eps,
    bool range_given, Finish *made)
{
    if (route == ROUTE_PC) {
        HIP_TRY(h, launch_rollout(h, st, route, kev, src, MODE_ROLLOUT, x_dev, eps, h->d_cost, nullptr, PC_PASS_WEIGHTS, range_given));
        made->nil_dev = h->d_mm + 2; // the temperature k_rollout_pc / k_cost_minmax / k_range_apply left there
        return MPPI_OK;
    }
    hipLaunchKernelGGL(k_cost_normalize, dim3((h->K_local + 255) / 256), dim3(256), 0, st, h->d_cost, h->K_local, h->d_mm, h->d_cost2);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, launch_rollout(h, st, route == ROUTE_GEN ? ROUTE_GEN : ROUTE_TILE, mppi_kev{}, src, MODE_COSTS_GIVEN, x_dev,
        eps, h->d_cost2, nullptr));
    return MPPI_OK;
}

// rollouts of this shard -> partial records in d_part; *made = where they are, how many, their temperature. Handles normalizeCost.
mppi_status enqueue_partials(mppi_handle *h, hipStream_t st, int src, const float *x_dev, const float *eps, float *noise_out, Finish *made)
{
    const Route route = rollout_route(h, src, noise_out, false);
    TraceRange tr(h, "mppi:rollout");
    *made = own_records(h);
    // (normalizeCost: the tile kernel writes the records)
    HIP_TRY(h, ensure_record_layout(h, st, (route == ROUTE_MLP && !h->normalize) ? h->nb_mlp : h->nb));
    const mppi_kev kev = prof_slot(h).rollout;
    if (!h->normalize) {
        HIP_TRY(h, launch_rollout(h, st, route, kev, src, MODE_ROLLOUT, x_dev, eps, h->d_cost, noise_out));
        return MPPI_OK;
    }
    if (h->shard_count != 1) return fail(h, MPPI_ERR_UNSUPPORTED,
        "normalize_cost on a sharded handle: mppi_shard_cost_range, reduce the ranges over the ranks, mppi_shard_partial_normalized");
    if (mppi_status s = norm_costs(h, st, route, kev, src, x_dev, eps, noise_out, nullptr); s != MPPI_OK) return s;
    // every workgroup of the weights-only pass reduces the nb tile pairs itself: nb^2 x 8 bytes of L2
    // reads in all — 8 MB at 1024 tiles, too much
    // beyond a few thousand (K > 131072 on one GPU): there the range comes from ONE k_cost_minmax launch over the costs instead
    const bool many_tiles = route == ROUTE_PC && h->nb > 2048;
    if (many_tiles) {
        hipLaunchKernelGGL(k_cost_minmax, dim3(1), dim3(1024), 0, st, h->d_cost, h->K_local, h->d_mm, h->hc.neg_inv_lambda,
            h->d_mm + 3, (float *)nullptr);
        HIP_TRY(h, hipGetLastError());
    }
    return norm_records(h, st, route, kev, src, x_dev, eps, many_tiles, made);
}

mppi_status ensure_eps(mppi_handle *h)
{
    if (!h->d_eps) HIP_TRY(h, hipMalloc((void **)&h->d_eps, sizeof(float) * (size_t)h->K_local * h->HA));
    return MPPI_OK;
}

// K-sharded normalizeCost: the range the ranks agreed on and its temperature into d_mm (mppi_shard_partial_normalized)
void range_apply(mppi_handle *h, hipStream_t st, const float *range_dev)
{
    hipLaunchKernelGGL(k_range_apply, dim3(1), dim3(64), 0, st, range_dev, h->d_mm, h->hc.neg_inv_lambda, (float *)nullptr);
}

// One launch = one control step (k_step_pc<.., STEP_FUSE>): tiles and the column waves that finish them in the same grid.
static mppi_status fused_step(mppi_handle *h, hipStream_t st, const float *x_dev, float *u_dev)
{
    TraceRange tr(h, "mppi:rollout");
    const ProfSlot p = prof_slot(h);
    const mppi_step_launch L{STEP_FUSE, x_dev, h->U_cur(), h->U_other(), u_dev, h->next_seq()};
    HIP_TRY(h, per_a(h, &mppi_unit_a::step, st, p.rollout, &L)); // the launch's own begin / end
    HIP_TRY(h, prof_one_launch(h, p, st));
    HIP_TRY(h, advance_sequence(h, st));
    return MPPI_OK;
}

// The plain control step in two halves, which a K-sharded step runs as two calls with the record exchange between them (mppi_shard_partial,
// mppi_shard_finish): enqueue_partials makes the records; this finishes them with the update and advances the sequence.
mppi_status finish_step(mppi_handle *h, hipStream_t st, const Finish &f)
{
    HIP_TRY(h, launch_finish(h, st, f));
    HIP_TRY(h, advance_sequence(h, st));
    return MPPI_OK;
}
// ... and both in one, on Philox noise or the noise in eps (src), xchg: with the in-kernel record exchange. ONE launch where the fused
// route serves: never with the exchange, never with injected noise (rollout_route).
mppi_status plain_step(mppi_handle *h, hipStream_t st, int src, const float *x_dev, const float *eps, float *u_dev, bool xchg)
{
    if (!xchg && rollout_route(h, src, nullptr, true) == ROUTE_STEP) return fused_step(h, st, x_dev, u_dev);
    Finish f;
    if (mppi_status s = enqueue_partials(h, st, src, x_dev, eps, nullptr, &f); s != MPPI_OK) return s;
    f.u_out = u_dev; f.xchg = xchg;
    return finish_step(h, st, f);
}

// Arm a step: the launch(es) that run it as soon as mppi_next has stored x. U_in / U_out: the sequence as it stands once every step
// enqueued before this one has been applied (the caller's bookkeeping may still be one step behind).
static mppi_status arm_launch(mppi_handle *h, const float *U_in, float *U_out, unsigned seq)
{
    const int mode = STEP_ARM | (fuse_ok(h) ? STEP_FUSE : 0);
    float *u_arg = h->d_pin + 2 * kMaxS;
    if (!(mode & STEP_FUSE)) HIP_TRY(h, ensure_record_layout(h, h->stream, h->nb));
    const mppi_step_launch L{mode, nullptr, U_in, U_out, u_arg, seq};
    HIP_TRY(h, per_a(h, &mppi_unit_a::step, h->stream, mppi_kev{}, &L));
    if (!(mode & STEP_FUSE)) {
        Finish f = own_records(h);
        f.U_in = U_in; f.U_out = U_out; f.u_out = u_arg; f.armed_seq = seq;
        HIP_TRY(h, launch_finish(h, h->stream, f));
    }
    return MPPI_OK;
}

// The pre-launched pipelined step (MPPI_TUNE_PRELAUNCH; k_step_pc<.., STEP_PRE> + k_finish_cols with FinishPre). Step n goes to stream
// n & 1 of the handle: its rollout is eligible as soon as the finish of step n-2 (the launch before it on that stream) is done, i.e. while
// step n-1 still runs on the other stream; it draws its noise in the CU slots step n-1's workgroups leave and waits for step n-1's U' as
// granules. Order that keeps the two grids from competing for slots: step n-1's workgroups are all resident long before step n becomes
// eligible (that takes the finish of n-2, which takes the END of rollout n-2, whose slots rollout n-1 — eligible since finish n-3 — has
// taken). Start-up has no such history and builds it with two events: rollout 2 (second stream) behind rollout 1 — it would otherwise share
// the chip with it —, and rollout 3 (first stream, behind finish 1) behind the moment the second stream got PAST that wait: rollout 2 is
// the next packet of its queue then, and rollout 3 sees the event through the same cross-queue latency that rollout 2 has already paid
// (measured without it: rollout 3 became resident first, held every slot waiting for finish 2, and rollout 2 never ran — the deadline).
static mppi_status pre_step(mppi_handle *h, const float *x_dev, float *u_dev)
{
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->arm_inflight) HIP_TRY(h, quiesce(h));
    // enter: everything enqueued so far drains; the sequence as it stands becomes the first
    // granules, the step counter the mirror
    if (!h->pre_active) {
        if (!h->stream2) HIP_TRY(h, hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
        if (!h->pre_ev) HIP_TRY(h, hipEventCreateWithFlags(&h->pre_ev, hipEventDisableTiming));
        if (!h->pre_ev2) HIP_TRY(h, hipEventCreateWithFlags(&h->pre_ev2, hipEventDisableTiming));
        if (!h->d_ugr) HIP_TRY(h, hipMalloc((void **)&h->d_ugr, sizeof(unsigned long long) * 2 * (size_t)h->HA));
        if (!h->d_cu_ctr) {
            HIP_TRY(h, hipMalloc((void **)&h->d_cu_ctr, sizeof(int) * 4096));
            HIP_TRY(h, hipMemset(h->d_cu_ctr, 0, sizeof(int) * 4096));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream2));
        std::vector<float> U(h->HA);
        unsigned long long step = 0;
        HIP_TRY(h, hipMemcpy(U.data(), h->U_cur(), sizeof(float) * h->HA, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(&step, h->d_step, sizeof(step), hipMemcpyDeviceToHost));
        const unsigned tag = h->next_seq();
        std::vector<unsigned long long> g(2 * (size_t)h->HA, 0ull);
        for (int i = 0; i < h->HA; ++i) {
            uint32_t bits;
            std::memcpy(&bits, &U[i], 4);
            g[i] = ((unsigned long long)tag << 32) | bits;
        }
        HIP_TRY(h, hipMemcpy(h->d_ugr, g.data(), sizeof(unsigned long long) * g.size(), hipMemcpyHostToDevice));
        if (!fuse_ok(h)) HIP_TRY(h, ensure_record_layout(h, h->stream, h->nb));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->pre_buf = 0; h->pre_tag = tag; h->pre_step = step; h->pre_count = 0; h->pre_active = true;
    }
    hipStream_t st = (h->pre_count & 1ull) ? h->stream2 : h->stream;
    if (h->pre_count == 1) HIP_TRY(h, hipEventRecord(h->pre_ev2, h->stream2)); // (behind the wait for rollout 1, in front of rollout 2)
    const unsigned seq = h->next_seq();
    const unsigned long long *ugr_in = h->d_ugr + (size_t)h->pre_buf * h->HA;
    unsigned long long *ugr_out = h->d_ugr + (size_t)(1 - h->pre_buf) * h->HA;
    const bool fused = fuse_ok(h); // <= 128 tiles: the column waves of the same grid finish the step (and write the next step's granules)
    const ProfSlot p = prof_slot(h);
    {
        TraceRange tr(h, "mppi:rollout");
        mppi_step_launch L{STEP_PRE | (fused ? STEP_FUSE : 0), x_dev, h->U_cur(), h->U_other(), u_dev, seq};
        L.ugr = ugr_in; L.utag = h->pre_tag; L.step_index = h->pre_step; L.ugr_out = fused ? ugr_out : nullptr;
        HIP_TRY(h, per_a(h, &mppi_unit_a::step, st, p.rollout, &L));
    }
    if (h->pre_count == 0) HIP_TRY(h, hipEventRecord(h->pre_ev, st)); // (start-up: see above)
    if (!fused) {
        Finish f = own_records(h);
        f.u_out = u_dev; f.pre = FinishPre{ugr_in, ugr_out, seq, h->pre_step};
        HIP_TRY(h, launch_finish(h, st, f));
    } else HIP_TRY(h, prof_one_launch(h, p, st));
    if (h->pre_count == 0) HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->pre_ev, 0));
    if (h->pre_count == 1) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->pre_ev2, 0)); // rollout 3 behind the second stream's release
    h->U_advance(); // (no sequence filter on this path: step_shape_ok)
    h->pre_buf = 1 - h->pre_buf; h->pre_tag = seq; h->pre_step += 1ull; h->pre_count += 1ull;
    return MPPI_OK;
}

} // namespace mppi_capi

extern "C" mppi_status mppi_next_device(mppi_handle *h, const float *x_dev, float *u_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_next_device");
    if (!h || !x_dev || !u_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (h->shard_count != 1) return fail(h, MPPI_ERR_INVALID_ARG, "sharded handle: use mppi_shard_partial / mppi_shard_finish");
    if (stream == nullptr && pre_ok(h)) return pre_step(h, x_dev, u_dev);
    MPPI_ENTER(h);
    TraceRange step_range(h, "mppi:step");
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return plain_step(h, st, SRC_PHILOX, x_dev, nullptr, u_dev);
}

static long long now_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// host-pointer step shared by mppi_next / mppi_next_with_noise
//
// Armed launches (MPPI_TUNE_ARMED_US > 0; mppi_step.hip.h). Once two calls have followed each other within the soft deadline, a call
// leaves the NEXT step's launch behind it — armed: resident, noise drawn, waiting for x. The next call then only stores x into the
// device's x slot and watches the pinned u slot: no launch and no dispatch between x and u. A launch whose x does not come in time
// aborts by itself (tile 0's verdict, mirrored in pinned host memory) and the call falls back to the ordinary launch; any other entry
// point retires an armed launch first (quiesce). An aborted or cancelled launch changes nothing: same U, same step counter, and the
// step that follows draws the noise it would have drawn.
static mppi_status step_host(mppi_handle *h, const float *x, int n_x, const float *eps, size_t n_eps, float *u_out, int n_u)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    MPPI_NOT_BATCH(h, eps ? "mppi_next_with_noise" : "mppi_next");
    if (!x || !u_out || n_x != h->s || n_u != h->a) return fail(h, MPPI_ERR_INVALID_ARG, "x must have s_dim floats and u_out a_dim floats");
    if (h->shard_count != 1) return fail(h, MPPI_ERR_INVALID_ARG, "sharded handle: use mppi_shard_partial / mppi_shard_finish");
    HIP_TRY(h, hipSetDevice(h->device));
    TraceRange step_range(h, "mppi:step");
    const long long t_call = now_ns();
    const long long gap_ns = h->last_next_ns ? t_call - h->last_next_ns : (1ll << 62);
    h->last_next_ns = t_call;
    const bool may_arm = !eps && h->prof_cap == 0 && arm_ok(h);
    if (h->arm_inflight && !may_arm) HIP_TRY(h, quiesce(h));
    constexpr uint32_t kUSentinel = 0x7fc0deadu;
    volatile uint32_t *uslot = reinterpret_cast<volatile uint32_t *>(h->h_pin + 2 * kMaxS);
    auto u_seen = [&]() { bool seen = true; for (int j = 0; j < h->a; ++j) seen = seen && uslot[j] != kUSentinel; return seen; };
    // m_db.addX(s); m_db.addU(out_tensor[1])  controller_base.cpp:146-147 — only when a log was asked for
    // (mppi_set_transition_log): a preallocated ring, no allocation on this path
    auto hand_out = [&]() {
        std::memcpy(u_out, h->h_pin + 2 * kMaxS, sizeof(float) * h->a);
        if (h->log_cap) {
            size_t r;
            if (h->log_count < h->log_cap) r = (h->log_head + h->log_count++) % h->log_cap;
            // full: the oldest row is overwritten (counted)
            else { r = h->log_head; h->log_head = (h->log_head + 1) % h->log_cap; h->log_dropped++; }
            float *row = h->log_rows.data() + r * h->log_stride();
            std::memcpy(row, x, sizeof(float) * h->s);
            std::memcpy(row + h->s, u_out, sizeof(float) * h->a);
            row[2 * h->s + h->a] = 0.0f; // x_next not known yet
        }
        return MPPI_OK;
    };

    if (h->arm_inflight) {
        volatile unsigned long long *verdict = h->h_arm;
        const unsigned seq = h->arm_seq;
        auto verdict_of = [&](unsigned q) -> unsigned { const unsigned long long v = *verdict;
            return (unsigned)(v >> 32) == q ? (unsigned)v : 0u; };
        if (*reinterpret_cast<volatile unsigned *>(h->h_arm + 1) != 0u) { // a hard deadline passed inside an armed launch: never expected
            (void)quiesce(h);
            *reinterpret_cast<volatile unsigned *>(h->h_arm + 1) = 0u;
            return fail(h, MPPI_ERR_HIP, "armed launch: a wave waited past its hard deadline");
        }
        if (verdict_of(seq) == kArmAbort) { // the soft deadline passed before this call: the launch has left (or is leaving)
            h->arm_inflight = false;
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        } else {
            for (int j = 0; j < h->a; ++j) uslot[j] = kUSentinel;
            for (int i = 0; i < h->s; ++i) xslot_store(h, i, x[i], seq);
            store_fence();
            // arm the step after this one while this one runs (its bookkeeping is committed below, once tile 0 has accepted x)
            const unsigned seq2 = h->next_seq();
            const mppi_status as = arm_launch(h, h->d_Ubuf[1 - h->u_cur] + h->a, h->d_Ubuf[h->u_cur], seq2);
            if (as != MPPI_OK) { h->arm_seq = seq2; (void)quiesce(h); return as; }
            unsigned v = 0u;
            const long long t0 = now_ns(), limit = ((long long)h->arm_us + 100000ll) * 1000ll;
            for (unsigned it = 0; (v = verdict_of(seq)) == 0u; ++it)
                if ((it & 255u) == 255u && now_ns() - t0 > limit) break;
            if (v == kArmAccept) {
                h->U_advance();
                h->arm_seq = seq2; // (arm_inflight stays up: the launch just armed)
                bool seen = false;
                for (unsigned it = 0; !(seen = u_seen()); ++it)
                    if ((it & 1023u) == 1023u && now_ns() - t0 > 200000000ll) break;
                if (!seen) { (void)quiesce(h); return fail(h, MPPI_ERR_HIP, "armed step: no control within 200 ms of an accepted x"); }
                return hand_out();
            }
            // aborted while x was on its way (or silent): retire the launch armed behind it, then the ordinary launch below
            h->arm_seq = seq2;
            HIP_TRY(h, quiesce(h));
            if (v == 0u) return fail(h, MPPI_ERR_HIP, "armed launch: no verdict");
        }
    }

    int src = SRC_PHILOX;
    if (eps) {
        if (n_eps != (size_t)h->K_local * h->HA) return fail(h, MPPI_ERR_INVALID_ARG, "eps must hold K_local*tau*a floats");
        mppi_status s = ensure_eps(h);
        if (s != MPPI_OK) return s;
        HIP_TRY(h, hipMemcpyAsync(h->d_eps, eps, sizeof(float) * n_eps, hipMemcpyHostToDevice, h->stream));
        src = SRC_HBM;
    }
    // x goes into the pinned slot the kernels read directly (slots alternate so a step never re-reads the
    // address of the previous x); u comes back through the pinned, device-mapped u slot.
    h->pin_slot ^= 1;
    std::memcpy(h->h_pin + h->pin_slot * kMaxS, x, sizeof(float) * h->s);
    const float *x_arg = h->d_pin + h->pin_slot * kMaxS;
    float *u_arg = h->d_pin + 2 * kMaxS;
    const bool spin_u = h->sync_spin && h->sg_window == 0; // with a sequence filter the step has one more kernel after u
    if (spin_u) for (int j = 0; j < h->a; ++j) uslot[j] = kUSentinel;
    if (mppi_status s = plain_step(h, h->stream, src, x_arg, h->d_eps, u_arg); s != MPPI_OK) return s;
    // two calls within the soft deadline of each other: the host loop is fast enough for an armed launch to be fed in time
    if (may_arm && spin_u && (h->arm_always || gap_ns < (long long)h->arm_us * 1000ll)) {
        const unsigned seq = h->next_seq();
        mppi_status s = arm_launch(h, h->U_cur(), h->U_other(), seq);
        if (s != MPPI_OK) return s;
        h->arm_inflight = true;
        h->arm_seq = seq;
    }
    // u arrives in the pinned slot as `a` single 4-byte stores over PCIe: watch the slot instead of waiting for the
    // stream's completion signal (the runtime's wake-up costs several us of a ~35 us synchronous step). The slot was
    // filled with a NaN pattern the update cannot produce; if it has not changed after 2 ms (a long step, an error, a
    // genuine NaN) fall back to the ordinary wait. Later calls on this handle are stream-ordered behind the step.
    bool seen = false;
    if (spin_u) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 0; !seen; ++it) {
            seen = u_seen();
            if (!seen && (it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
    }
    if (!seen) {
        if (h->arm_inflight) HIP_TRY(h, quiesce(h)); // (the stream would only drain at the armed launch's deadline)
        else HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return hand_out();
}

extern "C" mppi_status mppi_next(mppi_handle *h, const float *x, int n_x, float *u_out, int n_u)
{
    return step_host(h, x, n_x, nullptr, 0, u_out, n_u);
}

extern "C" mppi_status mppi_next_with_noise(mppi_handle *h, const float *x, int n_x, const float *eps, size_t n_eps, float *u_out, int n_u)
{
    if (h && !eps) return fail(h, MPPI_ERR_INVALID_ARG, "eps is NULL");
    return step_host(h, x, n_x, eps, n_eps, u_out, n_u);
}

// why the batched step does not serve the handle as it stands (batch_eligible)
static const char *kBatchStepRefusal(const mppi_handle *h)
{
    return h->nn_batch == 2 ? "batched step: the learned point mass runs on k_rollout_mlp2_batch / k_rollout_mlp_small_batch only"
         : h->nn_batch ? "batched step: the learned 13-state models run on k_rollout_nn_batch only"
         : h->is_gen   ? "batched step: the Fossen AUV model runs on k_rollout_auv_pc only"
                       : "batched step: the horizon exceeds what this producer count serves (tau <= 132 with 3 producers)";
}

// rollouts of every member -> records, the finish of every member -> U', u_dev[B][a]; the sequences and the step counter advance
static mppi_status batch_step(mppi_handle *h, hipStream_t st, const float *x_dev, float *u_dev)
{
    if (!batch_eligible(h)) return fail(h, MPPI_ERR_UNSUPPORTED, kBatchStepRefusal(h));
    TraceRange step_range(h, "mppi:batch_step");
    const ProfSlot p = prof_slot(h); // the dispatches' own begin / end
    HIP_TRY(h, h->nn_batch == 2 ? per_a(h, &mppi_unit_a::batch_mlp, st, p.rollout, x_dev)
             : h->nn_batch ? mppi_launch_batch_nn(h, st, p.rollout, x_dev)
             : h->is_gen ? mppi_launch_batch_auv(h, st, p.rollout, x_dev) : per_a(h, &mppi_unit_a::batch, st, p.rollout, x_dev));
    HIP_TRY(h, h->is_gen ? mppi_launch_batch_finish_auv(h, st, h->U_cur(), h->U_other(), u_dev, p.finish)
                         : per_a(h, &mppi_unit_a::batch_finish, st, (const float *)h->U_cur(), h->U_other(), u_dev, p.finish));
    if (p) prof_commit(h, st);
    h->U_advance();
    return MPPI_OK;
}

extern "C" mppi_status mppi_batch_next(mppi_handle *h, const float *x, int n_x, float *u_out, int n_u)
{
    MPPI_BATCH_ONLY(h);
    if (!x || !u_out || n_x != h->batch * h->s || n_u != h->batch * h->a) return fail(h, MPPI_ERR_INVALID_ARG,
        "x must hold n * s_dim floats and u_out n * a_dim");
    MPPI_ENTER(h);
    HIP_TRY(h, hipMemcpyAsync(h->d_bx, x, sizeof(float) * n_x, hipMemcpyHostToDevice, h->stream));
    if (mppi_status s = batch_step(h, h->stream, h->d_bx, h->d_bu); s != MPPI_OK) return s;
    HIP_TRY(h, hipMemcpyAsync(u_out, h->d_bu, sizeof(float) * n_u, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_batch_next_device(mppi_handle *h, const float *x_dev, float *u_dev, void *stream)
{
    MPPI_BATCH_ONLY(h);
    if (!x_dev || !u_dev) return fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer");
    MPPI_ENTER(h);
    return batch_step(h, stream ? (hipStream_t)stream : h->stream, x_dev, u_dev);
}

// ---- closed-loop episodes (include/mppi_c.h): n_steps control steps with the handle's own model as
// the plant, on the handle's stream, no host
// wait between the steps. Step t is the plain step (plain_step / batch_step: never the pre-launched
// or an armed one — x of step t + 1 depends
// on u of step t) reading row t of the trajectory and writing row t of the control log, then ONE
// launch (mppi_episode.hip) that writes C[t],
// row t + 1 of the trajectory and the next goal. A learned model spends one launch more on its model-step kernel.
static mppi_status ensure_episode_staging(mppi_handle *h, size_t floats)
{
    if (floats <= h->ep_cap) return MPPI_OK;
    if (h->d_ep) { HIP_TRY(h, hipStreamSynchronize(h->stream)); HIP_TRY(h, hipFree(h->d_ep)); h->d_ep = nullptr; h->ep_cap = 0; }
    HIP_TRY(h, hipMalloc((void **)&h->d_ep, sizeof(float) * floats));
    h->ep_cap = floats;
    return MPPI_OK;
}

static bool learned_model(const mppi_handle *h)
{
    const int mk = h->hc.model_kind;
    return mk == MPPI_MODEL_MLP || mk == MPPI_MODEL_NN_AUV || mk == MPPI_MODEL_NN_AUV_SPEED;
}

// ---- ... against a separate plant (mppi_run_episode_plant / mppi_batch_run_episode_plant): step 4 runs the model of ANOTHER handle, a
// lone unsharded one on the controller's device with its s_dim and a_dim. Only the plant's model is read: an analytic one (the point mass,
// the Fossen model) through its constants block on the device, whose address goes into a table of B pointers in the episode staging
// (member m's plant at [m]; a shared plant repeats one pointer; written once per call) that the plant variant of the episode kernel
// reads (mppi_episode_plant.hip); a learned one through its own model-step kernel, ONE launch over the B rows on the controller's
// stream, closed by the plain episode kernel — which is why a learned plant is shared by all members. The launches per step are the
// plain episode's.
struct EpisodePlant {
    mppi_handle *learned = nullptr;  // the shared learned plant, or none
    std::vector<const void *> table; // else: the B constants pointers (empty: the controller's own model, the plain episode)
};

// every refusal of a plant list, before anything is enqueued; fills `out`
static mppi_status check_plants(mppi_handle *h, const std::string &who, mppi_handle *const *plants, int n_plants, EpisodePlant *out)
{
    const int B = members(h);
    if (!plants) return fail(h, MPPI_ERR_INVALID_ARG, who + "plants is NULL");
    if (n_plants != 1 && n_plants != B) return fail(h, MPPI_ERR_INVALID_ARG, who + (h->batch ? "n_plants must be 1 or the member count"
        : "n_plants must be 1 for a lone controller"));
    for (int i = 0; i < n_plants; ++i) {
        const mppi_handle *p = plants[i];
        const std::string which = who + "plant " + std::to_string(i);
        if (!p) return fail(h, MPPI_ERR_INVALID_ARG, which + " is NULL");
        if (p->batch) return fail(h, MPPI_ERR_INVALID_ARG, which + " is a batched handle: a plant is a lone handle");
        if (p->shard_count != 1) return fail(h, MPPI_ERR_INVALID_ARG, which + " is a sharded handle: a plant is an unsharded handle");
        if (p->s != h->s || p->a != h->a) return fail(h, MPPI_ERR_INVALID_ARG, which + ": its s_dim and a_dim differ from the controller's");
        if (p->device != h->device) return fail(h, MPPI_ERR_INVALID_ARG, which + " lives on another device than the controller");
    }
    if (h->gen ? (h->s != 13 || h->a != 6) : (h->s != 2 * h->a || h->a < 1 || h->a > 4))
        return fail(h, MPPI_ERR_UNSUPPORTED, who + "the episode kernels serve the point-mass layout (s_dim = 2 a_dim, a_dim <= 4) and the "
            "13-state family");
    for (int i = 0; i < n_plants; ++i) {
        const mppi_handle *p = plants[i];
        if (learned_model(p)) {
            if (n_plants > 1) return fail(h, MPPI_ERR_UNSUPPORTED, who + "per-member learned plants: a learned plant is shared by all "
                "members (n_plants = 1)");
            if (p->hc.model_kind != MPPI_MODEL_MLP && !h->gen) return fail(h, MPPI_ERR_UNSUPPORTED, who + "a 13-state learned plant "
                "needs a controller of the 13-state family");
            out->learned = plants[i];
            return MPPI_OK;
        }
        if ((p->hc.model_kind == MPPI_MODEL_AUV) != (h->gen != nullptr)) return fail(h, MPPI_ERR_UNSUPPORTED, who + "plant " +
            std::to_string(i) + ": its model does not step the controller's state layout");
    }
    out->table.resize(B);
    for (int m = 0; m < B; ++m) {
        const mppi_handle *p = plants[n_plants == 1 ? 0 : m];
        out->table[m] = h->gen ? mppi_gen_dev_consts(p) : static_cast<const void *>(p->dC);
    }
    return MPPI_OK;
}

// ---- ... with the statistics of every step logged (mppi_run_episode_stats / mppi_batch_run_episode_stats): ONE launch of k_step_stats
// (mppi_step_stats.hip) right behind each control step, in front of the episode tail, writing row t of three more blocks of the staging
// (S [n][B][9] | Hc [n][B][32] | Hw [n][B][32]: 73 words per step and member), copied out with X, U and C. Outputs may be NULL.
struct EpisodeStats { float *S; uint32_t *Hc, *Hw; };

static mppi_status run_episode(mppi_handle *h, const char *name, const float *x0, int n_x, int n_steps, const float *goals,
                               const float *disturbance,
                               float *X_out, float *U_out, float *C_out, mppi_handle *const *plants = nullptr, int n_plants = 0,
                               bool with_plant = false, const EpisodeStats *stats = nullptr)
{
    const int B = members(h), s = h->s, a = h->a;
    const std::string who = std::string(name) + ": ";
    if (!x0 || n_x != B * s) return fail(h, MPPI_ERR_INVALID_ARG, who + (h->batch ? "x0 must hold n * s_dim floats"
        : "x0 must hold s_dim floats"));
    if (n_steps < 1 || n_steps > (1 << 24)) return fail(h, MPPI_ERR_INVALID_ARG, who + "n_steps must be in [1, 2^24]");
    if (stats) {
        mppi_status why = MPPI_OK;
        if (const char *msg = step_stats_refusal(h, &why)) return fail(h, why, who + msg);
    }
    if (h->shard_count != 1) return fail(h, MPPI_ERR_INVALID_ARG, "sharded handle: use mppi_shard_partial / mppi_shard_finish");
    if (!h->no_rollout.empty()) return fail(h, MPPI_ERR_UNSUPPORTED, h->no_rollout);
    if (h->batch && !batch_eligible(h)) return fail(h, MPPI_ERR_UNSUPPORTED, kBatchStepRefusal(h));
    EpisodePlant plant;
    if (with_plant)
        if (mppi_status st = check_plants(h, who, plants, n_plants, &plant); st != MPPI_OK) return st;
    MPPI_ENTER(h);
    // a plant's stream is drained once, here: an mppi_set_mlp in flight on it is complete before its weights are read (an armed launch of
    // a plant is retired as any entry point of that handle retires it). Plants are only read from here on.
    for (int i = 0; with_plant && i < n_plants; ++i) {
        mppi_handle *p = plants[i];
        if (p == h || (i > 0 && p == plants[i - 1])) continue;
        HIP_TRY(h, quiesce(p));
        HIP_TRY(h, hipStreamSynchronize(p->stream));
    }
    const size_t n = (size_t)n_steps, xs = (size_t)B * s, us = (size_t)B * a;
    // k_mlp_step_ref: 2 * 256 floats per sample; k_nnauv_step_ref: 128. The handle's own model steps one sample, a learned plant B.
    // ... and a learned batch as its own plant its B rows, row m through member m's network
    const size_t kScratch = 2 * kHid * ((plant.learned || h->nn_batch) ? (size_t)B : 1);
    const size_t oX = 0, oU = oX + (n + 1) * xs, oC = oU + n * us, oG = oC + n * B, oW = oG + (goals ? n * xs : 0), oS = oW +
        (disturbance ? n * xs : 0);
    const size_t oP = (oS + kScratch + 1) & ~(size_t)1; // the plant table: B pointers, 8-byte aligned
    const size_t oT = plant.table.empty() ? oS + kScratch : oP + 2 * (size_t)B; // the statistics, behind everything the plain episode stages
    const size_t nS = n * B * MPPI_N_STEP_STATS, nH = n * B * MPPI_STEP_STAT_BINS;
    if (mppi_status st = ensure_episode_staging(h, oT + (stats ? nS + 2 * nH : 0)); st != MPPI_OK) return st;
    float *dS = h->d_ep + oT;
    uint32_t *dHc = reinterpret_cast<uint32_t *>(dS + nS), *dHw = dHc + nH;
    float *dX = h->d_ep + oX, *dU = h->d_ep + oU, *dC = h->d_ep + oC, *dG = goals ? h->d_ep + oG : nullptr, *dW = disturbance
        ? h->d_ep + oW : nullptr;
    float *scratch = h->d_ep + oS;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(dX, x0, sizeof(float) * xs, hipMemcpyHostToDevice, st));
    if (dW) HIP_TRY(h, hipMemcpyAsync(dW, disturbance, sizeof(float) * n * xs, hipMemcpyHostToDevice, st));
    if (dG) {
        // goal <- goals[0], as mppi_set_goal / mppi_batch_set_goals before the first step; the later rows are stored by the episode kernel
        HIP_TRY(h, hipMemcpyAsync(dG, goals, sizeof(float) * n * xs, hipMemcpyHostToDevice, st));
        const size_t row = sizeof(float) * s;
        HIP_TRY(h, hipMemcpy2DAsync((char *)h->dC + offsetof(DevConsts, goal), sizeof(DevConsts), dG, row, row, B,
            hipMemcpyDeviceToDevice, st));
    }
    static_assert(sizeof(void *) == 2 * sizeof(float), "the plant table takes two floats of staging per pointer");
    const void *const *dP = plant.table.empty() ? nullptr : reinterpret_cast<const void *const *>(h->d_ep + oP);
    if (dP) HIP_TRY(h, hipMemcpyAsync(h->d_ep + oP, plant.table.data(), sizeof(void *) * (size_t)B, hipMemcpyHostToDevice, st));
    // whose model steps the state: a learned plant's kernel over the B rows, else the handle's own learned model on its one row, else
    // the episode kernel itself (the handle's analytic model, or the plants' through dP)
    mppi_handle *stepper = plant.learned ? plant.learned : (!with_plant && learned_model(h)) ? h : nullptr;
    const bool learned = stepper != nullptr;
    const int mk = learned ? stepper->hc.model_kind : h->hc.model_kind;
    for (int t = 0; t < n_steps; ++t) {
        const float *x_t = dX + (size_t)t * xs;
        float *u_t = dU + (size_t)t * us, *x_next = dX + (size_t)(t + 1) * xs;
        if (h->batch) {
            if (mppi_status s_ = batch_step(h, st, x_t, u_t); s_ != MPPI_OK) return s_;
        } else {
            TraceRange step_range(h, "mppi:step");
            if (mppi_status s_ = plain_step(h, st, SRC_PHILOX, x_t, nullptr, u_t); s_ != MPPI_OK) return s_;
        }
        if (stats) {
            const size_t r = (size_t)t * B;
            HIP_TRY(h, launch_step_stats(h, st, dS + r * MPPI_N_STEP_STATS, dHc + r * MPPI_STEP_STAT_BINS, dHw + r * MPPI_STEP_STAT_BINS));
        }
        TraceRange plant_range(h, "mppi:plant");
        if (learned && mk == MPPI_MODEL_MLP) {
            mlp_step_ref(stepper, st, x_t, B, u_t, B, scratch, x_next, (stepper == h && h->nn_batch) ? 1 : 0);
            HIP_TRY(h, hipGetLastError());
        } else if (learned && stepper == h && h->nn_batch) HIP_TRY(h, mppi_gen_model_step_members(h, st, x_t, u_t, B, scratch, x_next));
        else if (learned) HIP_TRY(h, mppi_gen_model_step(stepper, st, x_t, B, u_t, B, scratch, x_next));
        const mppi_episode_tail e{x_t, u_t, dW ? dW + (size_t)t * xs : nullptr, (dG && t + 1 < n_steps) ? dG +
                                  (size_t)(t + 1) * xs : nullptr,
                                  dC + (size_t)t * B, x_next, learned ? 0 : 1};
        HIP_TRY(h, dP ? mppi_launch_episode_tail_plant(h, st, dP, e) : mppi_launch_episode_tail(h, st, e));
    }
    if (X_out) HIP_TRY(h, hipMemcpyAsync(X_out, dX, sizeof(float) * (n + 1) * xs, hipMemcpyDeviceToHost, st));
    if (U_out) HIP_TRY(h, hipMemcpyAsync(U_out, dU, sizeof(float) * n * us, hipMemcpyDeviceToHost, st));
    if (C_out) HIP_TRY(h, hipMemcpyAsync(C_out, dC, sizeof(float) * n * B, hipMemcpyDeviceToHost, st));
    if (stats && stats->S) HIP_TRY(h, hipMemcpyAsync(stats->S, dS, sizeof(float) * nS, hipMemcpyDeviceToHost, st));
    if (stats && stats->Hc) HIP_TRY(h, hipMemcpyAsync(stats->Hc, dHc, sizeof(uint32_t) * nH, hipMemcpyDeviceToHost, st));
    if (stats && stats->Hw) HIP_TRY(h, hipMemcpyAsync(stats->Hw, dHw, sizeof(uint32_t) * nH, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (goals) for (int i = 0; i < s; ++i) h->hc.goal[i] = goals[(n - 1) * xs + i]; // the host mirror (member 0's)
    return MPPI_OK;
}

extern "C" mppi_status mppi_run_episode(mppi_handle *h, const float *x0, int n_x, int n_steps, const float *goals, const float *disturbance,
                                        float *X_out, float *U_out, float *C_out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (h->batch) return fail(h, MPPI_ERR_UNSUPPORTED,
        "mppi_run_episode: a batched handle runs its episodes through mppi_batch_run_episode");
    return run_episode(h, "mppi_run_episode", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out);
}

extern "C" mppi_status mppi_batch_run_episode(mppi_handle *h, const float *x0, int n_x, int n_steps, const float *goals,
                                              const float *disturbance,
                                              float *X_out, float *U_out, float *C_out)
{
    MPPI_BATCH_ONLY(h);
    return run_episode(h, "mppi_batch_run_episode", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out);
}

extern "C" mppi_status mppi_run_episode_plant(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x, int n_steps,
                                              const float *goals, const float *disturbance, float *X_out, float *U_out, float *C_out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (h->batch) return fail(h, MPPI_ERR_UNSUPPORTED,
        "mppi_run_episode_plant: a batched handle runs its episodes through mppi_batch_run_episode_plant");
    return run_episode(h, "mppi_run_episode_plant", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out, plants, n_plants, true);
}

extern "C" mppi_status mppi_batch_run_episode_plant(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x,
                                                    int n_steps, const float *goals, const float *disturbance, float *X_out, float *U_out,
                                                    float *C_out)
{
    MPPI_BATCH_ONLY(h);
    return run_episode(h, "mppi_batch_run_episode_plant", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out, plants, n_plants, true);
}

extern "C" mppi_status mppi_run_episode_stats(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x, int n_steps,
                                              const float *goals, const float *disturbance, float *X_out, float *U_out, float *C_out,
                                              float *S_out, uint32_t *Hc_out, uint32_t *Hw_out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (h->batch) return fail(h, MPPI_ERR_UNSUPPORTED,
        "mppi_run_episode_stats: a batched handle runs its episodes through mppi_batch_run_episode_stats");
    const EpisodeStats stats{S_out, Hc_out, Hw_out};
    return run_episode(h, "mppi_run_episode_stats", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out, plants, n_plants,
        plants != nullptr || n_plants != 0, &stats);
}

extern "C" mppi_status mppi_batch_run_episode_stats(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x,
                                                    int n_steps, const float *goals, const float *disturbance, float *X_out, float *U_out,
                                                    float *C_out, float *S_out, uint32_t *Hc_out, uint32_t *Hw_out)
{
    MPPI_BATCH_ONLY(h);
    const EpisodeStats stats{S_out, Hc_out, Hw_out};
    return run_episode(h, "mppi_batch_run_episode_stats", x0, n_x, n_steps, goals, disturbance, X_out, U_out, C_out, plants, n_plants,
        plants != nullptr || n_plants != 0, &stats);
}
