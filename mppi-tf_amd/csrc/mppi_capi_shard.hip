// mppi_capi_shard.hip — the K-shard entry points (a step in two or three calls with the ranks' exchange between them) and the
// direct peer exchange. Kernel of this unit: k_xchg_probe; the rollouts, the finish and the range go through mppi_capi_step.hip.

#include <cstring>
#include <string>

#define MPPI_UNIT_CAPI_SHARD 1
#include "mppi_capi.hip.h"

extern "C" mppi_status mppi_shard_partial(mppi_handle *h, const float *x_dev, float *record_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_partial");
    if (!h || !x_dev || !record_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    Finish f;
    if (mppi_status s = enqueue_partials(h, st, SRC_PHILOX, x_dev, nullptr, nullptr, &f); s != MPPI_OK) return s;
    f.u_out = h->d_u; f.record_out = record_dev; f.apply = 0;
    HIP_TRY(h, launch_finish(h, st, f));
    return MPPI_OK;
}

// ---- normalizeCost on a K-sharded controller -----------------------------------------------------
// c' = (c - min)/(max - min) needs the min and max over ALL samples (controller_base.py:468-474): each shard rolls its samples and
// reports its own {-min, max}; the ranks reduce the pairs (ONE 2-float all-reduce(MAX)); each shard then makes its record from costs
// normalised with the agreed range. The two calls are the two halves of enqueue_partials' normalizeCost (norm_costs, norm_records).
extern "C" mppi_status mppi_shard_cost_range(mppi_handle *h, const float *x_dev, float *range_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_cost_range");
    if (!h || !x_dev || !range_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (!h->normalize) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_cost_range: the handle was created without normalize_cost");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIP_TRY(h, ensure_record_layout(h, st, h->nb));
    return norm_costs(h, st, norm_route(h, SRC_PHILOX, nullptr), prof_slot(h).rollout, SRC_PHILOX, x_dev, nullptr, nullptr, range_dev);
}

extern "C" mppi_status mppi_shard_partial_normalized(mppi_handle *h, const float *x_dev, const float *range_dev,
    float *record_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_partial_normalized");
    if (!h || !x_dev || !range_dev || !record_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (!h->normalize) return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_partial_normalized: the handle was created without normalize_cost");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    range_apply(h, st, range_dev);
    HIP_TRY(h, hipGetLastError());
    // d_cost still holds this step's costs (mppi_shard_cost_range); the agreed range and its temperature are in d_mm now
    Finish f = own_records(h);
    if (mppi_status s = norm_records(h, st, norm_route(h, SRC_PHILOX, nullptr), prof_slot(h).rollout, SRC_PHILOX, x_dev, nullptr, true,
        &f); s != MPPI_OK) return s;
    f.u_out = h->d_u; f.record_out = record_dev; f.apply = 0;
    HIP_TRY(h, launch_finish(h, st, f));
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_finish(mppi_handle *h, const float *records_dev, int n_records, float *u_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_finish");
    if (!h || !records_dev || !u_dev || n_records <= 0) return h ? fail(h, MPPI_ERR_INVALID_ARG,
        "bad records/u pointer or count") : MPPI_ERR_INVALID_ARG;
    // more than 1024 records are folded 16:1 into the handle's scratch, which is sized for its own ceil(nbp/16) groups
    if (n_records > 1024 && (n_records + kGroup - 1) / kGroup > (h->nbp + kGroup - 1) / kGroup)
        return fail(h, MPPI_ERR_INVALID_ARG, "mppi_shard_finish: " + std::to_string(n_records) +
                                                 " records fold into more groups than this handle's scratch holds (" +
                                                 std::to_string((h->nbp + kGroup - 1) / kGroup) +
                                                 "): at most 1024 records, or a handle with at least as many tiles");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    Finish f = own_records(h);
    f.recs = records_dev; f.sb = 2 + h->HA; f.sc = 1; f.n = n_records; f.u_out = u_dev;
    // the ranks' records are in the units of this handle's own (mppi_shard_partial_normalized)
    if (h->norm_two_pass) f.nil_dev = h->d_mm + 2;
    return finish_step(h, st, f);
}

// One call per sharded step on the collective path (include/mppi_c.h): record -> the caller's all-gather (in place) -> finish.
extern "C" mppi_status mppi_shard_step(mppi_handle *h, const float *x_dev, float *u_dev, const mppi_collectives *coll, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_step");
    if (!h || !x_dev || !u_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    const bool gather = coll && coll->all_gather;
    if (h->shard_count > 1 && !gather) return fail(h, MPPI_ERR_INVALID_ARG,
        "mppi_shard_step: shard_count > 1 needs coll->all_gather (ncclAllGather's signature)");
    if (h->normalize && gather && !coll->all_reduce) return fail(h, MPPI_ERR_INVALID_ARG,
        "mppi_shard_step: a normalize_cost handle needs coll->all_reduce (ncclAllReduce's signature)");
    MPPI_ENTER(h);
    const int n = 2 + h->HA;
    // (a sharded handle gets both buffers in mppi_create; this covers the one-shard handle that walks the sharded path. Each pointer on its
    // own: a failed second allocation must not leave a half-made pair that the next call takes for complete — ADVICE r04)
    if (!h->d_recs) HIP_TRY(h, hipMalloc((void **)&h->d_recs, sizeof(float) * (size_t)n * h->shard_count));
    if (!h->d_range) HIP_TRY(h, hipMalloc((void **)&h->d_range, sizeof(float) * 2));
    TraceRange step_range(h, "mppi:step");
    float *own = h->d_recs + (size_t)n * h->shard_rank;
    mppi_status s;
    if (h->normalize) {
        if ((s = mppi_shard_cost_range(h, x_dev, h->d_range, stream)) != MPPI_OK) return s;
        if (gather) {
            TraceRange tr(h, "mppi:exchange");
            const int rc = coll->all_reduce(h->d_range, h->d_range, 2, MPPI_COLL_FLOAT32, MPPI_COLL_MAX, coll->comm, stream
                ? stream : (void *)h->stream);
            if (rc != 0) return fail(h, MPPI_ERR_EXCHANGE, "mppi_shard_step: all_reduce returned " + std::to_string(rc));
        }
        if ((s = mppi_shard_partial_normalized(h, x_dev, h->d_range, own, stream)) != MPPI_OK) return s;
    } else if ((s = mppi_shard_partial(h, x_dev, own, stream)) != MPPI_OK) return s;
    if (gather) {
        TraceRange tr(h, "mppi:exchange");
        const int rc = coll->all_gather(own, h->d_recs, (size_t)n, MPPI_COLL_FLOAT32, coll->comm, stream ? stream : (void *)h->stream);
        if (rc != 0) return fail(h, MPPI_ERR_EXCHANGE, "mppi_shard_step: all_gather returned " + std::to_string(rc));
    }
    return mppi_shard_finish(h, h->d_recs, h->shard_count, u_dev, stream);
}

// ---- direct record exchange (see include/mppi_c.h) -----------------------------------------------
extern "C" mppi_status mppi_shard_p2p_export(mppi_handle *h, void *ipc_handle_out, void **inbox_dev_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_export");
    if (!h || !inbox_dev_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL inbox_dev_out") : MPPI_ERR_INVALID_ARG;
    if (h->shard_count > kMaxPeers) return fail(h, MPPI_ERR_UNSUPPORTED, "direct exchange supports at most 16 shards");
    // fault injection for the fallback tests: mppi_set_tuning(MPPI_TUNE_P2P_FAULT, 1 = export | 2 = probe)
    if (h->p2p_fault == 1) return fail(h, MPPI_ERR_HIP, "injected fault: inbox export refused");
    MPPI_ENTER(h);
    if (!h->xchg_inbox) {
        // uncached: peer stores land in memory and the local spin loads see them without any cache maintenance
        HIP_TRY(h, hipExtMallocWithFlags((void **)&h->xchg_inbox, h->xchg_inbox_bytes(), hipDeviceMallocUncached));
        HIP_TRY(h, hipMemset(h->xchg_inbox, 0, h->xchg_inbox_bytes()));
        HIP_TRY(h, hipHostMalloc((void **)&h->h_xchg_status, sizeof(unsigned), hipHostMallocMapped));
        *h->h_xchg_status = 0u;
        HIP_TRY(h, hipHostGetDevicePointer((void **)&h->d_xchg_status, h->h_xchg_status, 0));
        HIP_TRY(h, hipMalloc((void **)&h->d_xchg_dead, sizeof(unsigned)));
        HIP_TRY(h, hipMemset(h->d_xchg_dead, 0, sizeof(unsigned)));
        HIP_TRY(h, hipMalloc((void **)&h->d_probe_got, sizeof(float) * kMaxPeers));
        HIP_TRY(h, hipDeviceSynchronize());
    }
    if (ipc_handle_out) {
        static_assert(sizeof(hipIpcMemHandle_t) == MPPI_IPC_HANDLE_BYTES, "ipc handle size");
        hipIpcMemHandle_t ih;
        HIP_TRY(h, hipIpcGetMemHandle(&ih, h->xchg_inbox));
        memcpy(ipc_handle_out, &ih, sizeof(ih));
    }
    *inbox_dev_out = h->xchg_inbox;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_open(mppi_handle *h, const void *ipc_handle, void **peer_inbox_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_open");
    if (!h || !ipc_handle || !peer_inbox_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL ipc handle / output") : MPPI_ERR_INVALID_ARG;
    MPPI_ENTER(h);
    hipIpcMemHandle_t ih;
    memcpy(&ih, ipc_handle, sizeof(ih));
    void *p = nullptr;
    HIP_TRY(h, hipIpcOpenMemHandle(&p, ih, hipIpcMemLazyEnablePeerAccess));
    h->xchg_opened.push_back(p);
    *peer_inbox_out = p;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_attach(mppi_handle *h, void *const *inboxes, int n, int timeout_ms)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_attach");
    if (!h || !inboxes) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL inbox table") : MPPI_ERR_INVALID_ARG;
    if (n != h->shard_count || n > kMaxPeers) return fail(h, MPPI_ERR_INVALID_ARG,
        "need exactly shard_count (<= 16) inbox pointers, rank order");
    if (!h->xchg_inbox) return fail(h, MPPI_ERR_INVALID_ARG, "call mppi_shard_p2p_export first");
    if (inboxes[h->shard_rank] != (void *)h->xchg_inbox) return fail(h, MPPI_ERR_INVALID_ARG,
        "entry shard_rank must be this handle's own inbox");
    if (timeout_ms <= 0 || timeout_ms > 60000) return fail(h, MPPI_ERR_INVALID_ARG, "timeout_ms must be in [1, 60000]");
    for (int g = 0; g < n; ++g) {
        if (!inboxes[g]) return fail(h, MPPI_ERR_INVALID_ARG, "NULL inbox pointer");
        h->xchg_peers.inbox[g] = (unsigned long long *)inboxes[g];
    }
    h->xchg_timeout_ticks = (long long)timeout_ms * 100000ll; // wall_clock64 ticks at 100 MHz
    h->xchg_attached = true;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_probe(mppi_handle *h, void *stream, int *ok_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_probe");
    if (!h || !ok_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL ok_out") : MPPI_ERR_INVALID_ARG;
    if (!h->xchg_attached) return fail(h, MPPI_ERR_INVALID_ARG, "inboxes not attached");
    MPPI_ENTER(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const unsigned seq = ++h->probe_seq;
    const int G = h->shard_count;
    auto payload = [&](int g) { return (float)(1000 * (int)(seq % 1000u) + g + 1); };
    hipLaunchKernelGGL(k_xchg_probe, dim3(1), dim3(64), 0, st, h->xchg_peers, h->xchg_step_slots(), G, h->shard_rank, seq,
                       payload(h->shard_rank), h->xchg_timeout_ticks, h->d_xchg_status, h->d_xchg_dead, h->d_probe_got);
    HIP_TRY(h, hipGetLastError());
    float got[kMaxPeers];
    HIP_TRY(h, hipMemcpyAsync(got, h->d_probe_got, sizeof(float) * G, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    int ok = (*(volatile unsigned *)h->h_xchg_status & 1u) ? 0 : 1;
    for (int g = 0; g < G; ++g) ok &= got[g] == payload(g);
    if (h->p2p_fault == 2) ok = 0;
    *ok_out = ok;
    return MPPI_OK;
}

extern "C" mppi_status mppi_shard_p2p_step(mppi_handle *h, const float *x_dev, float *u_dev, void *stream)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_step");
    if (!h || !x_dev || !u_dev) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL device pointer") : MPPI_ERR_INVALID_ARG;
    if (!h->xchg_attached) return fail(h, MPPI_ERR_INVALID_ARG, "inboxes not attached");
    // a deadline missed by any earlier step: refuse (the steps enqueued since then applied zero updates; U and the step
    // counter may differ between ranks until they are re-synchronised — ShardedController.resync)
    if (*(volatile unsigned *)h->h_xchg_status & 1u)
        return fail(h, MPPI_ERR_EXCHANGE, "direct exchange: a packet missed its deadline; the direct path is closed for this handle");
    MPPI_ENTER(h);
    TraceRange step_range(h, "mppi:step");
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    return plain_step(h, st, SRC_PHILOX, x_dev, nullptr, u_dev, true);
}

extern "C" mppi_status mppi_shard_p2p_status(mppi_handle *h, int *timed_out)
{
    MPPI_NOT_BATCH(h, "mppi_shard_p2p_status");
    if (!h || !timed_out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "NULL timed_out") : MPPI_ERR_INVALID_ARG;
    *timed_out = h->h_xchg_status ? (int)(*(volatile unsigned *)h->h_xchg_status & 1u) : 0;
    return MPPI_OK;
}
