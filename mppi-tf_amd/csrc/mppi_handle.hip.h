// mppi_handle.hip.h — host-side state of one controller (mppi_handle) and the launchers of the rollout kernels.
// The library is several translation units compiled in parallel (mppi-tf_amd/build.py): the C-ABI is split by concern — mppi_capi.hip
// (creation), mppi_capi_set.hip (setters, accessors), mppi_capi_step.hip (the control step), mppi_capi_shard.hip, mppi_capi_log.hip,
// mppi_capi_debug.hip — behind one internal header, mppi_capi.hip.h;
// mppi_launch_tile.hip / _pc.hip / _mlp.hip / _batch.hip instantiate one kernel family each for ONE action dimension per object
// (-DMPPI_UNIT_A=1..4), mppi_launch_gen.hip the generic-model kernels, mppi_launch_batch_gen.hip the batched AUV step, mppi_launch_batch_nn.hip the batched step of the learned 13-state models, mppi_launch_batch_mlp.hip that of the learned point mass (per action dimension), mppi_episode.hip the plant of a closed-loop
// episode, mppi_episode_plant.hip the same with another handle's model as the plant, mppi_model_rollout.hip the open-loop rollout of the
// handle's model (kernels and entry points). This header is what they share.
#pragma once
#include "mppi_kernels.hip.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

using namespace mppi;

// ----------------------------------------------------------------------------------------
struct mppi_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    DevConsts hc{};
    DevConsts *dC = nullptr;
    int norm_two_pass = 0;    // how the last records were made: 1 = from the raw costs at the temperature in d_mm[2] (the weights-only pass of normalizeCost), 0 = at lambda. Written where records are made; read by MPPI_DBG_WEIGHTS and by mppi_shard_finish (the ranks' records)
    int K_global = 0, K_local = 0, k_offset = 0, shard_rank = 0, shard_count = 1;
    int H = 0, s = 0, a = 0, HA = 0;
    int R = 64, nb = 0;   // tile size / record count of the point-mass tile kernels
    int nb_mlp = 0;       // record count of the MLP rollout kernel (64 rollouts per workgroup)
    int nbp = 0;          // record slots in d_part: record_pad(max(nb, nb_mlp)), the column stride of every rollout launch
    int part_nb = 0;      // tile count whose slots currently hold records (0: all slots neutral)
    int fp_contract = 0;  // MPPI_FLAG_FP_CONTRACT: the point-mass producer/consumer rollout with fused multiply-adds (PC_COST_DIAG_FMA)
    int mlp_bx3 = 0;      // MPPI_FLAG_MLP_BF16X3: split-bf16 matrix-core variant of the MLP rollout
    int mlp_small = 0;    // hidden width (16 or 32) of a small learned model served by k_rollout_mlp_small, else 0
    MlpSmallArgs small_args{};
    int mlp32_valu = 0;   // tuning: a Dense(32) network on 1 = the vector-ALU kernel, 2 = the one-wave-per-32-rollouts matrix-core kernel, instead of the two-wave pipeline
    int n_cu = 256;       // compute units of the device (k_rollout_mlp2 runs one tile-walking workgroup per CU)
    int mlp_v2 = 0;       // exact-fp32 MLP rollouts run k_rollout_mlp2 (one wave per SIMD, two pipelined sets; a_dim <= 3)
    MlpDev hm{};          // learned model: device pointers + normalisation (host copy)
    MlpDev *dM = nullptr;
    float *d_mlp_w = nullptr; // one allocation holding W1,b1,W2,b2,W3,b3
    size_t tile_lds = 0;
    int normalize = 0;
    int sigma_diag = 0; // Σ and Σ⁻¹ are exactly diagonal (the DIAG kernel instances are bit-identical then)
    int pc_np = 5;      // producer waves per workgroup of k_rollout_pc (chosen by tiles per CU; MPPI_TUNE_PC_PRODUCERS overrides)
    float *d_tile_mm = nullptr; // normalize_cost: every tile's (min, max) cost of the first pass, [2][nbp]
    // diagnostic switches, set only through mppi_set_tuning (the library reads no environment variable)
    int force_tile = 0;   // MPPI_TUNE_FORCE_TILE_KERNEL: the LDS-tile kernel instead of the producer/consumer one (A/B timing)
    int pc_no_balance = 0; // MPPI_TUNE_PC_BALANCE = 0: no SIMD-true roles / progress priorities
    int pc_bias = -1;      // head start (quarter chunks) of the four generations of workgroups on a CU, gen 0 in the low nibble (pc_set_prio); -1: the launcher's choice; MPPI_TUNE_PC_BALANCE = 0x10000 | biases
    int pc_lds_min = 0;   // MPPI_TUNE_PC_LDS_MIN: pad the dynamic LDS (caps workgroups per CU)
    int sync_spin = 1;    // MPPI_TUNE_SYNC_SPIN: the synchronous step watches the pinned u slot (0: waits for the stream)
    int p2p_fault = 0;    // MPPI_TUNE_P2P_FAULT: 1 = inbox export refused, 2 = probe reports failure (fallback tests)
    int trace = 0;        // MPPI_TUNE_TRACE: roctx ranges around what a step enqueues
    int gen_one_wave = 0; // MPPI_TUNE_GEN_ONE_WAVE: the Fossen AUVModel on k_rollout_gen<0> (one wave per tile) instead of k_rollout_auv_pc
    int finish_generic = 0; // MPPI_TUNE_FINISH_GENERIC: k_finish_cols / k_finish_cols_batch<A, false> instead of the column-major fast path (A/B timing)
    float *d_x = nullptr, *d_u = nullptr, *d_cost = nullptr, *d_cost2 = nullptr;
    // The nominal sequence lives in one of two buffers of tau*a + a floats whose last a floats stay zero. A step
    // reads U from ubuf[u_cur] + u_off and writes U' to the other buffer at offset 0; the shifted sequence
    // (mShift + mInit0, controller_base.cpp:310-324) is then simply that buffer read from offset a_dim.
    float *d_Ubuf[2] = {nullptr, nullptr};
    int u_cur = 0, u_off = 0;
    float *U_cur() const { return d_Ubuf[u_cur] + u_off; }
    float *U_other() const { return d_Ubuf[1 - u_cur]; }
    float *d_Uupd = nullptr; // U' of the last step (MPPI_DBG_U_UPDATED)
    bool stats_step = false; // d_cost and d_dbg are those of ONE control step (mppi_step_stats): up with every step, down when mppi_update rewrites d_dbg
    void U_advance() { u_cur = 1 - u_cur; u_off = a; d_Uupd = d_Ubuf[u_cur]; stats_step = true; }
    // options of the Python reference's update: clip_act limits [a_min | a_max] and the Savitzky-Golay filter
    float *d_clip = nullptr;
    int sg_window = 0;
    float *d_sg_rows = nullptr;
    int *d_sg_start = nullptr;
    float *d_part = nullptr, *d_part2 = nullptr, *d_part3 = nullptr, *d_record = nullptr, *d_dbg = nullptr, *d_mm = nullptr;
    float *d_eps = nullptr; // lazily allocated [K_local, H, a] for injected noise / debug export
    float *d_recs = nullptr, *d_range = nullptr; // mppi_shard_step: all shards' records (the own one in place) and the {-min, max} pair, lazily
    unsigned long long *d_step = nullptr;
    // pinned, device-mapped host staging for the synchronous path: x slot 0 | x slot 1 | u. The kernels read
    // x and write u straight through these (zero-copy over PCIe, 24 B / 12 B): no H2D / D2H copy nodes per step.
    float *h_pin = nullptr, *d_pin = nullptr;
    int pin_slot = 0;
    std::string err;
    // profiling: event pairs around the rollout / finish kernels (mppi_profile_begin/end)
    std::vector<hipEvent_t> ev;   // 4 events per step: rollout begin/end, finish begin/end
    int prof_cap = 0, prof_n = 0; // steps that can be / have been recorded
    hipStream_t prof_stream = nullptr;
    std::string no_rollout; // non-empty: why this handle cannot run rollouts (helpers still work)
    int is_gen = 0;         // model_base is AUVModel / NNAUVModel: rollouts run k_rollout_gen
    void *gen = nullptr;    // 13-state AUV family (model AUV / NN_AUV; mppi_launch_gen.hip owns it): constants + device copy
    // transition log (m_db of the reference: addX/addU/addNext/toCSV, data_base.cpp:29-71): off until
    // mppi_set_transition_log gives it a capacity; a ring of rows (x | u | x_next | has_next), allocated once there
    std::vector<float> log_rows;
    size_t log_cap = 0, log_count = 0, log_head = 0; // capacity in rows, rows held, index of the oldest row
    unsigned long long log_dropped = 0;               // rows overwritten since the log was (re)sized: the ring was full
    size_t log_stride() const { return (size_t)2 * s + a + 1; }
    // direct record exchange (mppi_shard_p2p_*): own inbox, the peers' mapped inboxes, call sequence number
    unsigned long long *xchg_inbox = nullptr;
    XchgPeers xchg_peers{};
    std::vector<void *> xchg_opened; // hipIpcOpenMemHandle mappings to close
    bool xchg_attached = false;
    unsigned xchg_seq = 0, probe_seq = 0;
    long long xchg_timeout_ticks = 0;
    unsigned *h_xchg_status = nullptr, *d_xchg_status = nullptr; // pinned, device-mapped: deadline flag for the host
    unsigned *d_xchg_dead = nullptr;                             // the same flag in device memory, read by every launch
    float *d_probe_got = nullptr;
    // r05: the whole step in one launch / the armed launch (mppi_step.hip.h, mppi_launch_step.hip)
    int fuse_step = 1;          // MPPI_TUNE_FUSED_STEP: 1 = a handle of <= 128 tiles runs its device-resident step as ONE launch (0: rollout + finish; 2: ONE launch, five producer waves at every horizon)
    int arm_us = 0;             // MPPI_TUNE_ARMED_US: soft deadline of an armed launch in microseconds, 0 = mppi_next never arms
    int arm_always = 0;         // MPPI_TUNE_ARMED_ALWAYS: arm after every mppi_next, whatever the gap between the last two calls was
    unsigned long long *d_step_recs = nullptr; // record granules of the fused step [(2 + HA)][128]
    unsigned long long *d_xslot = nullptr;     // x granules, stored by the HOST straight into fine-grained device memory (large BAR); NULL: no armed launches
    unsigned long long *d_decision = nullptr;  // tile 0's verdict on an armed launch (device)
    unsigned long long *h_arm = nullptr, *d_arm = nullptr; // pinned, device-mapped: [0] the verdict for the host, [1] the sticky error word
    unsigned step_seq = 0;      // launch sequence numbers of fused / armed launches: 31 bits, never 0, never reused
    bool arm_inflight = false;  // an armed launch of sequence number arm_seq sits in the stream, waiting for x
    unsigned arm_seq = 0;
    long long last_next_ns = 0; // steady-clock time of the previous mppi_next (the arming rule looks at the gap)
    // the pre-launched pipelined step (MPPI_TUNE_PRELAUNCH; k_step_pc<.., STEP_PRE>): steps alternate between `stream` and `stream2`
    int prelaunch = 0;            // tuning: mppi_next_device on the handle's own stream pre-launches (0: off)
    hipStream_t stream2 = nullptr;
    hipEvent_t pre_ev = nullptr, pre_ev2 = nullptr; // start-up order (pre_step, mppi_capi_step.hip)
    unsigned long long *d_ugr = nullptr; // [2][HA] sequence granules {value, tag}
    int *d_cu_ctr = nullptr;             // [4096] workgroup arrivals per CU (role placement of a pre-launched grid)
    bool pre_active = false;      // steps are in flight on both streams; the plain U buffers / step counter are valid again after pre_quiesce
    int pre_buf = 0;              // which half of d_ugr holds the sequence the NEXT launch reads
    unsigned pre_tag = 0;         // ... and its tag
    unsigned long long pre_step = 0; // host mirror of the Philox step counter
    unsigned long long pre_count = 0; // launches since the mode was entered (parity = stream)
    unsigned next_seq() { step_seq = (step_seq + 1u) & 0x7fffffffu; if (step_seq == 0u) step_seq = 1u; return step_seq; }
    // The host-side layout: a handle holds members(h) controllers that share this geometry, and a lone handle is the one-member case.
    // Member m's x is at d_bx + m*s (a batch's staging), its U in d_Ubuf[i] + m*(HA + a) (the sequence and its zero tail), its costs at
    // d_cost + m*K_local, its records at d_part + m*nbp*(2 + HA), beta/eta/aux at d_dbg + 8m, its constants (Philox key, goal, lambda, gamma,
    // upsilon, Sigma, Q) at dC + m; hc is member 0's constants. Everything else exists once.
    // batch = 0: a plain handle (mppi_create), on the lone kernels; batch = n >= 1: a batched handle (mppi_create_batch_configs), stepped by
    // the two batched launches (mppi_launch_batch.hip; the Fossen AUV model: mppi_launch_batch_gen.hip).
    int batch = 0;
    float *d_bx = nullptr, *d_bu = nullptr;
    // a batch of learned controllers, one network per member — 1: the 13-state models (mppi_create_batch_learned; mppi_launch_batch_nn.hip),
    // 2: the learned point mass (mppi_create_batch_mlp; mppi_launch_batch_mlp.hip): member m's network is the lone upload
    // layout at d_mlp_w + m * nn_stride, its MlpDev at dM + m, its padded layer pointers at d_nn_args + m (hm / small_args: member 0's)
    int nn_batch = 0;
    size_t nn_stride = 0; // floats
    MlpSmallArgs *d_nn_args = nullptr;
    // a closed-loop episode's staging (mppi_run_episode / mppi_batch_run_episode): X | U | C | goals | disturbance | model-step scratch
    // [| the plants' constants pointers: mppi_run_episode_plant], one allocation that grows on demand
    float *d_ep = nullptr;
    size_t ep_cap = 0; // floats
    // mppi_model_rollout of a learned model (mppi_model_rollout.hip): the per-row scratch of its reference step kernel, grown on demand,
    // and the stream the last such call was enqueued on
    float *d_mr = nullptr;
    size_t mr_cap = 0; // floats
    hipStream_t mr_stream = nullptr;
    size_t xchg_step_slots() const { return (size_t)2 * HA * shard_count * 3; }
    size_t xchg_inbox_bytes() const { return sizeof(unsigned long long) * (xchg_step_slots() + (size_t)2 * shard_count); }
};

inline int members(const mppi_handle *h) { return h->batch ? h->batch : 1; }

// The dynamic-LDS ceiling (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to the (kernel instance, device) pair,
// not to a handle: several handles, devices and host threads share one template instance. It is kept process-wide and
// only ever RAISED (mppi_capi.hip), so a handle that needs less never lowers it under one that needs more.
hipError_t mppi_raise_lds_ceiling(const void *kernel, int device, size_t bytes);

// ---- launch policy shared by the launch units (each rule defined once) ---------------------------------------------------
// slots per producer wave of k_rollout_pc / k_rollout_pc_batch / k_step_pc: the horizon's 4-step groups, spread over NP producers
inline int mppi_pc_slots(int np, int H) { const int NG = (H + 3) / 4; return np == 3 ? (NG <= 18 ? 6 : 11) : (NG <= 20 ? 4 : 8); }
// f(NSLOT) with NSLOT as a std::integral_constant: the slot count of the NP-producer instances that serves the horizon H
template <int NP, typename F>
auto mppi_with_slots(int H, F &&f)
{
    using std::integral_constant;
    if constexpr (NP == 3) return mppi_pc_slots(3, H) == 6 ? f(integral_constant<int, 6>{}) : f(integral_constant<int, 11>{});
    else return mppi_pc_slots(5, H) == 4 ? f(integral_constant<int, 4>{}) : f(integral_constant<int, 8>{});
}
// The balance word of k_rollout_pc / k_rollout_pc_batch / k_step_pc over a grid of `tiles` workgroups: one round of workgroups (<= 4 per
// CU, all resident from the start) gets SIMD-true roles + progress priorities. Bit 0: on; bits 8..23: the generations' head starts
// (pc_set_prio). Four workgroups per CU (the small-NSLOT instances): 10, 3, 3, 0 quarter chunks — r05's sweep on three boxes
// (tools/tune_prio.py, profiles/r05_tune_prio.txt): kernel 15.05 -> 14.68 us at configs[2], 14.1 -> 13.4 at K = 49152, against r04's 9, 6,
// 3, 0; two per CU (H > 80 at a = 3) keep r04's: the new ones cost 10 % there.
inline int mppi_pc_balance(const mppi_handle *h, int A, int NSLOT, int tiles)
{
    const int bias = h->pc_bias >= 0 ? h->pc_bias : ((NSLOT * 4 * A <= 80) ? 0x033a : 0x0369);
    return (tiles <= 4 * 256 && !h->pc_no_balance) ? (1 | (bias << 8)) : 0;
}
// SIMD-true roles of the two-tile workgroups (a network / pose wave and a cost / velocity wave per tile) while the whole grid of `wgs`
// workgroups is resident in one round (MPPI_TUNE_PC_BALANCE = 0: roles by wave index, A/B)
inline int mppi_two_tile_balance(const mppi_handle *h, int wgs) { return (wgs <= 2 * h->n_cu && !h->pc_no_balance) ? 1 : 0; }
// the one-launch step on SEVEN producer waves (k_step_pc<A, 7, 3, ..>): H <= 84, unless MPPI_TUNE_FUSED_STEP = 2 keeps the six-wave workgroup
inline bool mppi_step_seven(const mppi_handle *h) { return h->fuse_step != 2 && (h->H + 3) / 4 <= 21; }

// ---- picks and launches -----------------------------------------------------------------------------------------------------------
// A pick (one per kernel family, in the family's launch unit) is a pure function of the handle that returns the kernel instance a launch
// serves, its name as rocprofv3 prints it and the geometry the template arguments decide; the launcher then launches exactly that.
// The name is formatted once per instance from the template arguments that instantiate it (a function-local static of the instance's pick).
template <typename... V>
std::string mppi_fmt(const char *fmt, V... v) { char b[128]; std::snprintf(b, sizeof b, fmt, v...); return b; }
inline const char *mppi_tf(bool b) { return b ? "true" : "false"; }
// a pick of a family whose kernels take different argument lists: P holds one kernel pointer per list, and `slot` is set
template <typename P, typename K>
P mppi_pick_in(K P::*slot, K kern, const std::string &name, dim3 g, dim3 b, size_t lds = 0)
{
    P p; p.*slot = kern; p.name = name.c_str(); p.g = g; p.b = b; p.lds = lds; return p;
}
// f(DIAG) with DIAG as a std::bool_constant: the instance for an exactly diagonal Sigma or the one for a dense Sigma
template <typename F>
auto mppi_with_diag(const mppi_handle *h, F &&f) { return h->sigma_diag ? f(std::true_type{}) : f(std::false_type{}); }

// The events of ONE dispatch. When a step is being profiled its dominant kernel is launched with hipExtLaunchKernel, whose start / stop
// events carry the dispatch's own begin / end timestamps (what rocprofv3 reports), not the stream-level gaps around it; else both are null.
struct mppi_kev { hipEvent_t begin = nullptr, end = nullptr; };
// One launch of a rollout kernel on the events `kev`, after raising the instance's dynamic-LDS ceiling if it needs more than the default.
template <typename... P, typename... Args>
hipError_t mppi_launch(const mppi_handle *h, mppi_kev kev, void (*kern)(P...), dim3 g, dim3 b, size_t lds, hipStream_t st, Args... args)
{
    if (hipError_t e = mppi_raise_lds_ceiling(reinterpret_cast<const void *>(kern), h->device, lds); e != hipSuccess) return e;
    hipExtLaunchKernelGGL(kern, g, b, (uint32_t)lds, st, kev.begin, kev.end, 0, args...);
    return hipGetLastError();
}

// What holds for one launch is an argument: `kev`; `consts`, the DevConsts block to run on (h->dC, or a batch member's: mppi_debug_get);
// `pass` of k_rollout_pc (PC_PASS_PLAIN the step's one pass, PC_PASS_COSTS / _WEIGHTS the two of normalizeCost) and `range_given`: the weights-only
// pass takes its temperature from d_mm[2] (a K-sharded handle: the ranks agreed on the range; many tiles) instead of reducing d_tile_mm.
#define MPPI_TILE_PARAMS mppi_handle *h, const DevConsts *consts, hipStream_t st, int src, int mode, const float *x_dev, const float *U_dev, \
                         const float *eps, float *cost, float *part, float *noise_out
#define MPPI_MLP_PARAMS mppi_handle *h, hipStream_t st, mppi_kev kev, int src, int mode, const float *x_dev, const float *U_dev, \
                        const float *eps, float *cost
#define MPPI_PC_PARAMS mppi_handle *h, hipStream_t st, mppi_kev kev, const float *x_dev, int pass, bool range_given
#define MPPI_BATCH_PARAMS mppi_handle *h, hipStream_t st, mppi_kev kev, const float *x_dev
// one launch of k_step_pc (mppi_step.hip.h): mode = STEP_FUSE | STEP_ARM bits; the sequence it reads / writes is given explicitly
// (an armed launch for step n+1 is enqueued before step n's bookkeeping is committed)
struct mppi_step_launch {
    int mode; const float *x_dev, *U_in; float *U_out, *u_out; unsigned seq;
    const unsigned long long *ugr = nullptr; unsigned utag = 0; unsigned long long step_index = 0; // STEP_PRE: this step's sequence as granules, their tag, the Philox step index
    unsigned long long *ugr_out = nullptr; // STEP_PRE | STEP_FUSE: the next step's granules (the column waves write them)
};
#define MPPI_STEP_PARAMS mppi_handle *h, hipStream_t st, mppi_kev kev, const mppi_step_launch *L
#define MPPI_BATCH_FINISH_PARAMS mppi_handle *h, hipStream_t st, const float *U_in, float *U_out, float *u_dev, mppi_kev kev
// The entry points of the per-a launch units (mppi_launch_{tile,pc,mlp,step,batch}.hip): X(NAME, result, parameters) is defined as
// mppi_NAME_a1 .. mppi_NAME_a4, one per action dimension, each in its own object file; the *_name entries name what the launch would run.
// The batched step (mppi_launch_batch.hip): every member's rollout in one launch, every member's finish in another; batch_mlp: the
// rollouts of a batch of learned point masses, one network per member (mppi_launch_batch_mlp.hip), finished by batch_finish.
#define MPPI_UNIT_ENTRIES(X)                                                                                                         \
    X(tile, hipError_t, MPPI_TILE_PARAMS) X(pc, hipError_t, MPPI_PC_PARAMS) X(mlp, hipError_t, MPPI_MLP_PARAMS)                       \
    X(step, hipError_t, MPPI_STEP_PARAMS) X(batch, hipError_t, MPPI_BATCH_PARAMS) X(batch_finish, hipError_t, MPPI_BATCH_FINISH_PARAMS) \
    X(tile_name, const char *, const mppi_handle *h, int src, int mode) X(pc_name, const char *, const mppi_handle *h, int pass)      \
    X(mlp_name, const char *, const mppi_handle *h, int src) X(step_name, const char *, const mppi_handle *h, int mode)               \
    X(batch_name, const char *, const mppi_handle *h) X(batch_mlp, hipError_t, MPPI_BATCH_PARAMS)                                     \
    X(batch_mlp_name, const char *, const mppi_handle *h)
#define MPPI_DECL_A(NAME, R, ...) R mppi_##NAME##_a1(__VA_ARGS__); R mppi_##NAME##_a2(__VA_ARGS__); R mppi_##NAME##_a3(__VA_ARGS__); R mppi_##NAME##_a4(__VA_ARGS__);
#define MPPI_MEMBER(NAME, R, ...) R (*NAME)(__VA_ARGS__);
MPPI_UNIT_ENTRIES(MPPI_DECL_A)
struct mppi_unit_a { MPPI_UNIT_ENTRIES(MPPI_MEMBER) }; // one row per action dimension (mppi_capi_step.hip holds the table)
#undef MPPI_DECL_A
#undef MPPI_MEMBER
// the 13-state AUV family (mppi_launch_gen.hip)
const char *mppi_gen_fill(mppi_handle *h, const mppi_config *cfg); // NULL = ok, else why the config is invalid
hipError_t mppi_gen_upload(mppi_handle *h);
void mppi_gen_destroy(mppi_handle *h);
hipError_t mppi_launch_gen(mppi_handle *h, const DevConsts *consts, hipStream_t st, mppi_kev kev, int src, int mode, const float *x_dev,
                           const float *U_dev, const float *eps, float *cost, float *part, float *noise_out);
const char *mppi_gen_name(const mppi_handle *h, int mode); // the instance mppi_launch_gen runs for `mode` without a noise export
hipError_t mppi_gen_model_step(mppi_handle *h, hipStream_t st, const float *x, int kx, const float *v, int k, float *scratch, float *out_next);
hipError_t mppi_gen_costs(mppi_handle *h, hipStream_t st, const float *x, const float *u, const float *eps, int k, float *os, float *oa, float *ot);
hipError_t mppi_gen_auv_pieces(mppi_handle *h, hipStream_t st, const float *x, const float *u, int k, float *out);
hipError_t mppi_gen_e3_terms(mppi_handle *h, hipStream_t st, const float *x, int k, int in_plane, float *out);
const void *mppi_gen_dev_consts(const mppi_handle *h); // the handle's GenConsts on the device
// the batched step of the Fossen AUV model (mppi_launch_batch_gen.hip): every member's rollout in one launch (k_rollout_auv_pc_batch),
// every member's finish in another (k_finish_cols_batch<6>)
hipError_t mppi_launch_batch_auv(MPPI_BATCH_PARAMS);
hipError_t mppi_launch_batch_finish_auv(MPPI_BATCH_FINISH_PARAMS);
const char *mppi_batch_auv_name(const mppi_handle *h);
// the batched step of the learned 13-state models, one network per member (mppi_launch_batch_nn.hip): every member's rollout in one launch
// (k_rollout_nn_batch); the finish is mppi_launch_batch_finish_auv's
hipError_t mppi_launch_batch_nn(MPPI_BATCH_PARAMS);
const char *mppi_batch_nn_name(const mppi_handle *h);
// mppi_gen_model_step with row i stepped by the network at dM + i (a learned batch as its own plant): x [k,13], v [k,6] -> next [k,13]
hipError_t mppi_gen_model_step_members(mppi_handle *h, hipStream_t st, const float *x, const float *v, int k, float *scratch, float *out_next);
// The plant of a closed-loop episode (mppi_episode.hip): ONE launch behind a control step serves every member. Member m: C[t] = the state
// cost of x_t under the goal in force; x_{t+1} = model(x_t, u_t) (+ w_t) into the trajectory's next row, which is the next step's x_dev; the
// goal of step t + 1 into the member's DevConsts.goal. model = 0 (a learned model): an existing model-step kernel has written x_next already.
struct mppi_episode_tail {
    const float *x, *u;         // x_t [B][s], u_t [B][a]
    const float *w, *goal_next; // w_t [B][s] / goal_{t+1} [B][s], or NULL
    float *cost, *x_next;       // C[t] [B], x_{t+1} [B][s]
    int model;
};
hipError_t mppi_launch_episode_tail(mppi_handle *h, hipStream_t st, const mppi_episode_tail &e);
#define MPPI_CAT_(a, b) a##b
#define MPPI_CAT(a, b) MPPI_CAT_(a, b)
