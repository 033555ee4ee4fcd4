// mppi_capi_debug.hip — debug items and the reference's public graph helpers as entry points (model step, costs, rollout cost, update,
// slices): host-pointer calls that allocate scratch, launch, copy back and wait. Kernels of this unit: k_weights, k_mlp_step_ref and every
// instance of k_model_step and k_costs.

#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#define MPPI_UNIT_CAPI_DEBUG 1
#include "mppi_capi.hip.h"

// one debug item of member `member` (a lone handle: 0)
static mppi_status debug_get(mppi_handle *h, int member, int what, float *out, size_t n)
{
    MPPI_ENTER(h);
    const size_t K = (size_t)h->K_local;
    const float *src = nullptr;
    size_t need = 0;
    float *tmp = nullptr;
    const float *cost = h->d_cost + K * member, *dbg = h->d_dbg + 8 * (size_t)member;
    switch (what) {
    case MPPI_DBG_COSTS: src = cost; need = K; break;
    case MPPI_DBG_BETA: src = dbg; need = 1; break;
    case MPPI_DBG_ETA: src = dbg + 1; need = 1; break;
    case MPPI_DBG_AUX: src = dbg; need = 8; break; // beta, eta, and what a timing-study build left in the other words
    case MPPI_DBG_U_UPDATED: // U' of the last step = the current buffer from offset 0 (the warm start reads it from offset a)
        if (!h->d_Uupd) return fail(h, MPPI_ERR_INVALID_ARG, h->batch ? "no step has run since the action sequences were set"
            : "no step has run since the action sequence was set");
        src = h->d_Uupd + (size_t)(h->HA + h->a) * member; need = (size_t)h->HA; break;
    case MPPI_DBG_WEIGHTS: {
        need = K;
        if (n != need) return fail(h, MPPI_ERR_INVALID_ARG, "wrong output size");
        HIP_TRY(h, hipMalloc((void **)&tmp, sizeof(float) * K));
        const WeightInputs w = weight_inputs(h, member);
        hipLaunchKernelGGL(k_weights, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, h->stream, w.consts, w.cost_w, (int)K, w.beta_eta,
                           (float *)nullptr, (float *)nullptr, tmp, w.nil_dev);
        src = tmp;
        break;
    }
    case MPPI_DBG_NOISE: {
        // the member's noise of the LAST step, regenerated from its Philox key and Sigma at the previous step counter (step-1)
        need = K * (size_t)h->HA;
        if (n != need) return fail(h, MPPI_ERR_INVALID_ARG, "wrong output size");
        if (mppi_status s = ensure_eps(h); s != MPPI_OK) return s;
        unsigned long long cur = 0;
        HIP_TRY(h, hipMemcpyAsync(&cur, h->d_step, sizeof(cur), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (cur == 0) return fail(h, MPPI_ERR_INVALID_ARG, "no step has run yet");
        const unsigned long long prev = cur - 1;
        HIP_TRY(h, hipMemcpyAsync(h->d_step, &prev, sizeof(prev), hipMemcpyHostToDevice, h->stream));
        // noise-only pass of the tile kernel (the point mass) or of k_rollout_gen (the 13-state family), on the member's constants: reads
        // neither x nor any cost buffer and writes nothing but d_eps
        const DevConsts *own = h->dC + member;
        const hipError_t le = h->is_gen ? mppi_launch_gen(h, own, h->stream, mppi_kev{}, SRC_PHILOX, MODE_NOISE_ONLY, h->d_x, h->U_cur(),
            nullptr, nullptr, nullptr, h->d_eps)
                                        : launch_tile(h, own, h->stream, SRC_PHILOX, MODE_NOISE_ONLY, h->d_x, h->U_cur(), nullptr,
                                            nullptr, nullptr, h->d_eps);
        HIP_TRY(h, hipMemcpyAsync(h->d_step, &cur, sizeof(cur), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, le);
        src = h->d_eps;
        break;
    }
    default: return fail(h, MPPI_ERR_INVALID_ARG, "unknown debug item");
    }
    if (n != need) { if (tmp) (void)hipFree(tmp); return fail(h, MPPI_ERR_INVALID_ARG, "wrong output size"); }
    hipError_t e = hipMemcpyAsync(out, src, sizeof(float) * need, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (tmp) (void)hipFree(tmp);
    HIP_TRY(h, e);
    return MPPI_OK;
}

extern "C" mppi_status mppi_debug_get(mppi_handle *h, int what, float *out, size_t n)
{
    MPPI_NOT_BATCH(h, "mppi_debug_get");
    if (!h || !out) return h ? fail(h, MPPI_ERR_INVALID_ARG, "out is NULL") : MPPI_ERR_INVALID_ARG;
    return debug_get(h, 0, what, out, n);
}

// ----------------------------------------------------------------------------------------
// helpers: scratch device buffers for the host-pointer helper entry points
struct DevBuf {
    float *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(float) * (n ? n : 1)); }
    hipError_t up(const float *src, size_t n, hipStream_t st) { return hipMemcpyAsync(p, src, sizeof(float) * n,
        hipMemcpyHostToDevice, st); }
    hipError_t down(float *dst, size_t n, hipStream_t st) const { return hipMemcpyAsync(dst, p, sizeof(float) * n,
        hipMemcpyDeviceToHost, st); }
};

namespace mppi_capi {
void mlp_step_ref(mppi_handle *h, hipStream_t st, const float *x, int kx, const float *v, int k, float *scratch, float *out_next,
                  int member_stride)
{
    hipLaunchKernelGGL(k_mlp_step_ref, dim3((k + 63) / 64), dim3(64), 0, st, h->dC, h->dM, x, kx, v, k, scratch, out_next, member_stride);
}
} // namespace mppi_capi

extern "C" mppi_status mppi_model_step(mppi_handle *h, const float *x, int kx, const float *v, int k,
                                       float *out_free, float *out_action, float *out_next)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !v || k <= 0 || (kx != k && kx != 1)) return fail(h, MPPI_ERR_INVALID_ARG, "x is [kx,s] with kx in {1,k}; v is [k,a]");
    MPPI_ENTER(h);
    const int s = h->s, a = h->a;
    if (h->is_gen) {
        if (out_free || out_action) return fail(h, MPPI_ERR_UNSUPPORTED, "the free/action split exists for the point-mass model only");
        DevBuf dx, dv, dn, ds;
        HIP_TRY(h, dx.alloc((size_t)kx * s)); HIP_TRY(h, dv.alloc((size_t)k * a)); HIP_TRY(h, dn.alloc((size_t)k * s)); HIP_TRY(h,
            ds.alloc((size_t)k * 128));
        HIP_TRY(h, dx.up(x, (size_t)kx * s, h->stream)); HIP_TRY(h, dv.up(v, (size_t)k * a, h->stream));
        HIP_TRY(h, mppi_gen_model_step(h, h->stream, dx.p, kx, dv.p, k, ds.p, dn.p));
        if (out_next) HIP_TRY(h, dn.down(out_next, (size_t)k * s, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return MPPI_OK;
    }
    if (h->hc.model_kind == MPPI_MODEL_MLP) {
        if (out_free || out_action) return fail(h, MPPI_ERR_UNSUPPORTED, "the free/action split exists for the point-mass model only");
        DevBuf dx, dv, dn, ds;
        HIP_TRY(h, dx.alloc((size_t)kx * s)); HIP_TRY(h, dv.alloc((size_t)k * a)); HIP_TRY(h, dn.alloc((size_t)k * s)); HIP_TRY(h,
            ds.alloc((size_t)k * 2 * kHid));
        HIP_TRY(h, dx.up(x, (size_t)kx * s, h->stream)); HIP_TRY(h, dv.up(v, (size_t)k * a, h->stream));
        mlp_step_ref(h, h->stream, dx.p, kx, dv.p, k, ds.p, dn.p);
        HIP_TRY(h, hipGetLastError());
        if (out_next) HIP_TRY(h, dn.down(out_next, (size_t)k * s, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return MPPI_OK;
    }
    DevBuf dx, dv, df, da, dn;
    HIP_TRY(h, dx.alloc((size_t)kx * s)); HIP_TRY(h, dv.alloc((size_t)k * a));
    HIP_TRY(h, df.alloc((size_t)kx * s)); HIP_TRY(h, da.alloc((size_t)k * s)); HIP_TRY(h, dn.alloc((size_t)k * s));
    HIP_TRY(h, dx.up(x, (size_t)kx * s, h->stream)); HIP_TRY(h, dv.up(v, (size_t)k * a, h->stream));
    const dim3 g((k + 255) / 256), b(256);
#define MPPI_MS_CASE(AA) case AA: hipLaunchKernelGGL(k_model_step<AA>, g, b, 0, h->stream, h->dC, dx.p, kx, dv.p, k, s, a, \
    df.p, da.p, dn.p); break;
    switch (a) {
        MPPI_MS_CASE(1) MPPI_MS_CASE(2) MPPI_MS_CASE(3) MPPI_MS_CASE(4)
    default: hipLaunchKernelGGL(k_model_step<kMaxA>, g, b, 0, h->stream, h->dC, dx.p, kx, dv.p, k, s, a, df.p, da.p, dn.p); break;
    }
#undef MPPI_MS_CASE
    HIP_TRY(h, hipGetLastError());
    if (out_free) HIP_TRY(h, df.down(out_free, (size_t)kx * s, h->stream));
    if (out_action) HIP_TRY(h, da.down(out_action, (size_t)k * s, h->stream));
    if (out_next) HIP_TRY(h, dn.down(out_next, (size_t)k * s, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_auv_pieces(mppi_handle *h, const float *x, const float *u, int k, float *out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !u || !out || k <= 0) return fail(h, MPPI_ERR_INVALID_ARG, "x is [k,13], u is [k,6], out is [k,124]");
    if (h->hc.model_kind != MPPI_MODEL_AUV) return fail(h, MPPI_ERR_INVALID_ARG, "not an AUVModel handle");
    MPPI_ENTER(h);
    DevBuf dx, du, dout;
    HIP_TRY(h, dx.alloc((size_t)k * 13)); HIP_TRY(h, du.alloc((size_t)k * 6)); HIP_TRY(h, dout.alloc((size_t)k * 124));
    HIP_TRY(h, dx.up(x, (size_t)k * 13, h->stream)); HIP_TRY(h, du.up(u, (size_t)k * 6, h->stream));
    HIP_TRY(h, mppi_gen_auv_pieces(h, h->stream, dx.p, du.p, k, dout.p));
    HIP_TRY(h, dout.down(out, (size_t)k * 124, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_ellipse3d_terms(mppi_handle *h, const float *x, int k, int in_plane_frame, float *out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !out || k <= 0) return fail(h, MPPI_ERR_INVALID_ARG, "x is [k,13], out is [k,3]");
    if (h->hc.state_cost_kind != MPPI_STATE_COST_ELLIPSE3D) return fail(h, MPPI_ERR_INVALID_ARG, "not an ElipseCost3D handle");
    MPPI_ENTER(h);
    DevBuf dx, dout;
    HIP_TRY(h, dx.alloc((size_t)k * 13)); HIP_TRY(h, dout.alloc((size_t)k * 3));
    HIP_TRY(h, dx.up(x, (size_t)k * 13, h->stream));
    HIP_TRY(h, mppi_gen_e3_terms(h, h->stream, dx.p, k, in_plane_frame, dout.p));
    HIP_TRY(h, dout.down(out, (size_t)k * 3, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

template <int S, int A>
static void launch_costs_sa(mppi_handle *h, const float *x, const float *u, const float *eps, int k, float *os, float *oa, float *ot)
{
    const dim3 g((k + 255) / 256), b(256);
    if (h->hc.q_full) hipLaunchKernelGGL((k_costs<S, A, true>), g, b, 0, h->stream, h->dC, x, u, eps, k, h->s, h->a, os, oa, ot);
    else hipLaunchKernelGGL((k_costs<S, A, false>), g, b, 0, h->stream, h->dC, x, u, eps, k, h->s, h->a, os, oa, ot);
}

// state / action / step cost of k samples; x may be NULL (action cost only), u/eps may be NULL (state only)
static mppi_status costs_host(mppi_handle *h, const float *x, const float *u, const float *eps, int k,
                              float *out_state, float *out_action, float *out_step)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (k <= 0 || (!x && !u) || ((u == nullptr) != (eps == nullptr))) return fail(h, MPPI_ERR_INVALID_ARG, "bad cost arguments");
    MPPI_ENTER(h);
    const int s = h->s, a = h->a;
    DevBuf dx, du, de, ds, da, dt;
    HIP_TRY(h, dx.alloc((size_t)k * s)); HIP_TRY(h, du.alloc(a)); HIP_TRY(h, de.alloc((size_t)k * a));
    HIP_TRY(h, ds.alloc(k)); HIP_TRY(h, da.alloc(k)); HIP_TRY(h, dt.alloc(k));
    if (x) HIP_TRY(h, dx.up(x, (size_t)k * s, h->stream));
    if (u) { HIP_TRY(h, du.up(u, a, h->stream)); HIP_TRY(h, de.up(eps, (size_t)k * a, h->stream)); }
    const float *px = x ? dx.p : nullptr, *pu = u ? du.p : nullptr, *pe = u ? de.p : nullptr;
    // shapes of the reference's own tests + the point-mass family run exact instances
    // 13-state costs (quadratic, quaternion, 3D ellipse)
    if (h->gen != nullptr) HIP_TRY(h, mppi_gen_costs(h, h->stream, px, pu, pe, k, ds.p, da.p, dt.p));
    else if (s == 2 && a == 1) launch_costs_sa<2, 1>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 2 && a == 2) launch_costs_sa<2, 2>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 4 && a == 2) launch_costs_sa<4, 2>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 4 && a == 3) launch_costs_sa<4, 3>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 6 && a == 3) launch_costs_sa<6, 3>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else if (s == 8 && a == 4) launch_costs_sa<8, 4>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    else launch_costs_sa<kMaxS, kMaxA>(h, px, pu, pe, k, ds.p, da.p, dt.p);
    HIP_TRY(h, hipGetLastError());
    if (out_state) HIP_TRY(h, ds.down(out_state, k, h->stream));
    if (out_action) HIP_TRY(h, da.down(out_action, k, h->stream));
    if (out_step) HIP_TRY(h, dt.down(out_step, k, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_state_cost(mppi_handle *h, const float *x, int k, float *out)
{
    if (h && (!x || !out)) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    return costs_host(h, x, nullptr, nullptr, k, out, nullptr, nullptr);
}

extern "C" mppi_status mppi_action_cost(mppi_handle *h, const float *u, const float *eps, int k, float *out)
{
    if (h && (!u || !eps || !out)) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    return costs_host(h, nullptr, u, eps, k, nullptr, out, nullptr);
}

extern "C" mppi_status mppi_step_cost(mppi_handle *h, const float *x, const float *u, const float *eps, int k, float *out)
{
    if (h && (!x || !u || !eps || !out)) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    return costs_host(h, x, u, eps, k, nullptr, nullptr, out);
}

extern "C" mppi_status mppi_rollout_cost(mppi_handle *h, const float *x, const float *U, const float *eps, float *cost_out)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!x || !U || !eps || !cost_out) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    MPPI_ENTER(h);
    mppi_status s = ensure_eps(h);
    if (s != MPPI_OK) return s;
    DevBuf dx, dU, dc;
    HIP_TRY(h, dx.alloc(h->s)); HIP_TRY(h, dU.alloc(h->HA)); HIP_TRY(h, dc.alloc(h->K_local));
    HIP_TRY(h, dx.up(x, h->s, h->stream)); HIP_TRY(h, dU.up(U, h->HA, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_eps, eps, sizeof(float) * (size_t)h->K_local * h->HA, hipMemcpyHostToDevice, h->stream));
    if (h->is_gen) HIP_TRY(h, mppi_launch_gen(h, h->dC, h->stream, mppi_kev{}, SRC_HBM, MODE_COST_ONLY, dx.p, dU.p, h->d_eps,
        dc.p, h->d_part, nullptr));
    else if (h->hc.model_kind == MPPI_MODEL_MLP) HIP_TRY(h, per_a(h, &mppi_unit_a::mlp, h->stream, mppi_kev{}, SRC_HBM, MODE_COST_ONLY,
        dx.p, dU.p, h->d_eps, dc.p));
    else HIP_TRY(h, launch_tile(h, h->dC, h->stream, SRC_HBM, MODE_COST_ONLY, dx.p, dU.p, h->d_eps, dc.p, h->d_part, nullptr));
    HIP_TRY(h, dc.down(cost_out, h->K_local, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return MPPI_OK;
}

extern "C" mppi_status mppi_update(mppi_handle *h, const float *cost, const float *eps, const float *U,
                                   float *beta, float *exp_arg, float *exp_out, float *nabla, float *weights,
                                   float *weighted_noise, float *U_new)
{
    if (!h) return MPPI_ERR_INVALID_ARG;
    if (!cost || !eps || !U) return fail(h, MPPI_ERR_INVALID_ARG, "NULL pointer");
    MPPI_ENTER(h);
    mppi_status s = ensure_eps(h);
    if (s != MPPI_OK) return s;
    const int K = h->K_local, HA = h->HA;
    DevBuf dU, dc, drec, darg, dexp, dw, dUn, du;
    HIP_TRY(h, dU.alloc(HA)); HIP_TRY(h, dc.alloc(K)); HIP_TRY(h, drec.alloc(2 + HA));
    HIP_TRY(h, darg.alloc(K)); HIP_TRY(h, dexp.alloc(K)); HIP_TRY(h, dw.alloc(K)); HIP_TRY(h, dUn.alloc(HA)); HIP_TRY(h, du.alloc(kMaxA));
    HIP_TRY(h, dU.up(U, HA, h->stream)); HIP_TRY(h, dc.up(cost, K, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_eps, eps, sizeof(float) * (size_t)K * HA, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, ensure_record_layout(h, h->stream, h->nb));
    if (h->is_gen) HIP_TRY(h, mppi_launch_gen(h, h->dC, h->stream, mppi_kev{}, SRC_HBM, MODE_COSTS_GIVEN, h->d_x, dU.p, h->d_eps,
        dc.p, h->d_part, nullptr));
    else HIP_TRY(h, launch_tile(h, h->dC, h->stream, SRC_HBM, MODE_COSTS_GIVEN, h->d_x, dU.p, h->d_eps, dc.p, h->d_part, nullptr));
    h->norm_two_pass = 0; // records made from the GIVEN costs at lambda
    h->stats_step = false; // ... whose beta and eta the finish below leaves in d_dbg, beside the last step's costs in d_cost
    // record = (beta, eta, V); then U' on a scratch copy of U (apply shifts it, so read U_updated)
    unsigned long long step_before = 0;
    HIP_TRY(h, hipMemcpyAsync(&step_before, h->d_step, sizeof(step_before), hipMemcpyDeviceToHost, h->stream));
    Finish f = own_records(h);
    f.U_in = dU.p; f.U_out = dUn.p; f.u_out = du.p; f.record_out = drec.p;
    HIP_TRY(h, launch_finish(h, h->stream, f));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_step, &step_before, sizeof(step_before), hipMemcpyHostToDevice, h->stream)); // stateless call
    hipLaunchKernelGGL(k_weights, dim3((K + 255) / 256), dim3(256), 0, h->stream, h->dC, dc.p, K, drec.p, darg.p, dexp.p, dw.p,
        (const float *)nullptr);
    HIP_TRY(h, hipGetLastError());
    std::vector<float> rec(2 + HA), Un(HA);
    HIP_TRY(h, drec.down(rec.data(), 2 + HA, h->stream));
    HIP_TRY(h, dUn.down(Un.data(), HA, h->stream));
    if (exp_arg) HIP_TRY(h, darg.down(exp_arg, K, h->stream));
    if (exp_out) HIP_TRY(h, dexp.down(exp_out, K, h->stream));
    if (weights) HIP_TRY(h, dw.down(weights, K, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (beta) *beta = rec[0];
    if (nabla) *nabla = rec[1];
    if (weighted_noise) for (int c = 0; c < HA; ++c) weighted_noise[c] = (float)((double)rec[2 + c] / (double)rec[1]);
    if (U_new) std::memcpy(U_new, Un.data(), sizeof(float) * HA);
    return MPPI_OK;
}

// mGetNew (controller_base.cpp:326-329) / mShift (:314-324): pure slices, host side.
extern "C" mppi_status mppi_get_new(const float *U, int tau, int a, int nb, float *out)
{
    if (!U || (!out && nb > 0) || nb < 0 || nb > tau || a <= 0) return MPPI_ERR_INVALID_ARG;
    for (int i = 0; i < nb * a; ++i) out[i] = U[i];
    return MPPI_OK;
}

extern "C" mppi_status mppi_shift(const float *U, int tau, int a, const float *init, int nb_init, int nb, float *out)
{
    if (!U || !out || nb < 0 || nb > tau || nb_init < 0 || a <= 0) return MPPI_ERR_INVALID_ARG;
    int o = 0;
    for (int i = nb * a; i < tau * a; ++i) out[o++] = U[i];
    for (int i = 0; i < nb_init * a; ++i) out[o++] = init ? init[i] : 0.0f; // mInit0: zeros
    return MPPI_OK;
}

extern "C" mppi_status mppi_batch_debug_get(mppi_handle *h, int member, int what, float *out, size_t n)
{
    MPPI_BATCH_ONLY(h);
    if (!out) return fail(h, MPPI_ERR_INVALID_ARG, "out is NULL");
    if (member < 0 || member >= h->batch) return fail(h, MPPI_ERR_INVALID_ARG, "member out of range");
    return debug_get(h, member, what, out, n);
}
