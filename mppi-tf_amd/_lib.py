"""ctypes binding of libmppi_hip.so (include/mppi_c.h) — the only way Python reaches the kernels.

There is no CPU fallback: a missing library or a missing GPU raises (MppiError / OSError).
torch is imported before the library is loaded on purpose: torch's wheel bundles its own
libamdhip64.so.7; loading it first makes our library bind to that same HIP runtime instance
(same soname) instead of bringing a second runtime into the process.
"""
import collections
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MPPI_SO_PATH selects a variant build of the SAME library (tools/ablate.py); never a different backend.
SO_PATH = os.environ.get("MPPI_SO_PATH") or os.path.join(HERE, "libmppi_hip.so")

OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_SINGULAR_SIGMA, ERR_ALLOC, ERR_IO, ERR_EXCHANGE = range(9)
MODEL_POINT_MASS, MODEL_MLP, MODEL_AUV, MODEL_NN_AUV, MODEL_NN_AUV_SPEED = 0, 1, 2, 3, 4
STATE_COST_QUADRATIC, STATE_COST_ELLIPSE, STATE_COST_QUAT, STATE_COST_ELLIPSE3D = 0, 1, 2, 3
ACTION_COST_CPP, ACTION_COST_PY = 0, 1
DBG_COSTS, DBG_BETA, DBG_ETA, DBG_WEIGHTS, DBG_NOISE, DBG_U_UPDATED, DBG_AUX = range(7)
CSV_REFERENCE, CSV_ROUNDTRIP = 0, 1
# mppi_set_tuning items (diagnostics; the library reads no environment variable)
TUNING = {"force_tile_kernel": 0, "pc_producers": 1, "pc_balance": 2, "pc_lds_min": 3, "sync_spin": 4, "p2p_fault": 5, "mlp_v1": 6, "mlp32_valu": 7,
          "trace": 8, "gen_one_wave": 9, "fused_step": 10, "armed_us": 11, "armed_always": 12, "prelaunch": 13,
          "finish_generic": 14}
P2P_FAULTS = {"": 0, "export": 1, "probe": 2}

FP = C.POINTER(C.c_float)
DP = C.POINTER(C.c_double)
UP = C.POINTER(C.c_uint32)
N_STEP_STATS, STEP_STAT_BINS = 9, 32  # MPPI_N_STEP_STATS, MPPI_STEP_STAT_BINS


class MppiError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("mppi status %d: %s" % (status, text))
        self.status = status


class MlpDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("widths", C.POINTER(C.c_int32)),
                ("W", C.POINTER(FP)), ("b", C.POINTER(FP)),
                ("xmean", FP), ("xstd", FP), ("ymean", FP), ("ystd", FP)]


class AuvDesc(C.Structure):
    _fields_ = [("mass", C.c_float), ("volume", C.c_float), ("density", C.c_float), ("gravity", C.c_float),
                ("cog", C.c_float * 3), ("cob", C.c_float * 3), ("inertial", C.c_float * 6),
                ("added_mass", FP), ("linear_damping", FP), ("linear_damping_forward_speed", FP), ("quad_damping", FP),
                ("rk", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_int32), ("tau", C.c_int32),
                ("s_dim", C.c_int32), ("a_dim", C.c_int32), ("dt", C.c_float), ("mass", C.c_float),
                ("lam", C.c_float), ("gamma", C.c_float), ("upsilon", C.c_float),
                ("action_cost_kind", C.c_int32), ("normalize_cost", C.c_int32),
                ("sigma", FP), ("goal", FP), ("Q", FP), ("q_is_full", C.c_int32),
                ("seed", C.c_uint64), ("model_kind", C.c_int32), ("mlp", C.POINTER(MlpDesc)),
                ("device", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("flags", C.c_int32), ("state_cost_kind", C.c_int32), ("ellipse", FP),
                ("auv", C.POINTER(AuvDesc)), ("quat_Q", FP), ("ellipse3d", FP)]


class LearnerModel(C.Structure):
    """mppi_learner_model: the learned model around a batch's network (mppi_learner_batch_rollout)"""
    _fields_ = [("model_kind", C.c_int32), ("s_dim", C.c_int32), ("a_dim", C.c_int32), ("dt", C.c_float),
                ("xmean", FP), ("xstd", FP), ("ymean", FP), ("ystd", FP)]


class Collectives(C.Structure):
    """mppi_collectives: the caller's all-gather / all-reduce with ncclAllGather's / ncclAllReduce's signatures + the communicator"""
    _fields_ = [("all_gather", C.c_void_p), ("all_reduce", C.c_void_p), ("comm", C.c_void_p)]


# name -> (restype, argtypes); must list EVERY symbol include/mppi_c.h declares
# (tests/test_capi_symbols.py parses the header and compares).
_H = C.c_void_p
SIGNATURES = {
    "mppi_abi_version": (C.c_int, []),
    "mppi_version": (C.c_char_p, []),
    "mppi_status_string": (C.c_char_p, [C.c_int]),
    "mppi_device_count": (C.c_int, []),
    "mppi_config_init": (C.c_int, [C.POINTER(Config), C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]),
    "mppi_create": (C.c_int, [C.POINTER(Config), C.POINTER(_H)]),
    "mppi_destroy": (None, [_H]),
    "mppi_last_error": (C.c_char_p, [_H]),
    "mppi_set_goal": (C.c_int, [_H, FP, C.c_int]),
    "mppi_set_mlp": (C.c_int, [_H, C.POINTER(MlpDesc)]),
    "mppi_next": (C.c_int, [_H, FP, C.c_int, FP, C.c_int]),
    "mppi_next_with_noise": (C.c_int, [_H, FP, C.c_int, FP, C.c_size_t, FP, C.c_int]),
    "mppi_save_next": (C.c_int, [_H, FP, C.c_int]),
    "mppi_to_csv": (C.c_int, [_H, C.c_char_p]),
    "mppi_to_csv_format": (C.c_int, [_H, C.c_char_p, C.c_int]),
    "mppi_set_transition_log": (C.c_int, [_H, C.c_int]),
    "mppi_transition_log_stats": (C.c_int, [_H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mppi_set_tuning": (C.c_int, [_H, C.c_int, C.c_int]),
    "mppi_get_action_sequence": (C.c_int, [_H, FP, C.c_int]),
    "mppi_set_action_sequence": (C.c_int, [_H, FP, C.c_int]),
    "mppi_get_step_counter": (C.c_int, [_H, C.POINTER(C.c_uint64)]),
    "mppi_set_step_counter": (C.c_int, [_H, C.c_uint64]),
    "mppi_debug_get": (C.c_int, [_H, C.c_int, FP, C.c_size_t]),
    "mppi_model_step": (C.c_int, [_H, FP, C.c_int, FP, C.c_int, FP, FP, FP]),
    "mppi_auv_pieces": (C.c_int, [_H, FP, FP, C.c_int, FP]),
    "mppi_ellipse3d_terms": (C.c_int, [_H, FP, C.c_int, C.c_int, FP]),
    "mppi_state_cost": (C.c_int, [_H, FP, C.c_int, FP]),
    "mppi_action_cost": (C.c_int, [_H, FP, FP, C.c_int, FP]),
    "mppi_step_cost": (C.c_int, [_H, FP, FP, FP, C.c_int, FP]),
    "mppi_rollout_cost": (C.c_int, [_H, FP, FP, FP, FP]),
    "mppi_update": (C.c_int, [_H, FP, FP, FP, FP, FP, FP, FP, FP, FP, FP]),
    "mppi_get_new": (C.c_int, [FP, C.c_int, C.c_int, C.c_int, FP]),
    "mppi_shift": (C.c_int, [FP, C.c_int, C.c_int, FP, C.c_int, C.c_int, FP]),
    "mppi_record_size": (C.c_int, [_H]),
    "mppi_local_samples": (C.c_int, [_H]),
    "mppi_sample_offset": (C.c_int, [_H]),
    "mppi_next_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mppi_shard_partial": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mppi_shard_finish": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mppi_shard_cost_range": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mppi_shard_partial_normalized": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mppi_shard_step": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(Collectives), C.c_void_p]),
    "mppi_synchronize": (C.c_int, [_H]),
    "mppi_set_action_limits": (C.c_int, [_H, FP, FP, C.c_int]),
    "mppi_set_sequence_filter": (C.c_int, [_H, C.c_int, C.c_int]),
    "mppi_shard_p2p_export": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mppi_shard_p2p_open": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mppi_shard_p2p_attach": (C.c_int, [_H, C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "mppi_shard_p2p_probe": (C.c_int, [_H, C.c_void_p, C.POINTER(C.c_int)]),
    "mppi_shard_p2p_step": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mppi_shard_p2p_status": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "mppi_profile_begin": (C.c_int, [_H, C.c_int]),
    "mppi_profile_end": (C.c_int, [_H, FP, FP, C.POINTER(C.c_int)]),
    "mppi_rollout_kernel_name": (C.c_int, [_H, C.c_char_p, C.c_size_t]),
    # batched controllers (BatchHandle)
    "mppi_create_batch": (C.c_int, [C.POINTER(Config), C.c_int, C.POINTER(C.c_uint64), C.POINTER(_H)]),
    "mppi_create_batch_configs": (C.c_int, [C.POINTER(Config), C.c_int, C.POINTER(_H)]),
    "mppi_batch_size": (C.c_int, [_H]),
    "mppi_batch_set_goals": (C.c_int, [_H, FP, C.c_int]),
    "mppi_batch_next": (C.c_int, [_H, FP, C.c_int, FP, C.c_int]),
    "mppi_batch_next_device": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mppi_batch_get_action_sequences": (C.c_int, [_H, FP, C.c_int]),
    "mppi_batch_set_action_sequences": (C.c_int, [_H, FP, C.c_int]),
    "mppi_batch_debug_get": (C.c_int, [_H, C.c_int, C.c_int, FP, C.c_size_t]),
    # ... of the learned 13-state models, one network per member (BatchHandle.learned, BatchHandle.set_mlp)
    "mppi_create_batch_learned": (C.c_int, [C.POINTER(Config), C.c_int, C.POINTER(_H)]),
    "mppi_batch_set_mlp": (C.c_int, [_H, C.c_int, C.POINTER(MlpDesc)]),
    # ... of the learned point mass, one network per member (BatchHandle.learned(model="mlp"))
    "mppi_create_batch_mlp": (C.c_int, [C.POINTER(Config), C.c_int, C.POINTER(_H)]),
    # closed-loop episodes on the device (Handle.run_episode, BatchHandle.run_episode)
    "mppi_run_episode": (C.c_int, [_H, FP, C.c_int, C.c_int, FP, FP, FP, FP, FP]),
    "mppi_batch_run_episode": (C.c_int, [_H, FP, C.c_int, C.c_int, FP, FP, FP, FP, FP]),
    # ... against a separate plant: another handle's model (run_episode(..., plant=))
    "mppi_run_episode_plant": (C.c_int, [_H, C.POINTER(_H), C.c_int, FP, C.c_int, C.c_int, FP, FP, FP, FP, FP]),
    "mppi_batch_run_episode_plant": (C.c_int, [_H, C.POINTER(_H), C.c_int, FP, C.c_int, C.c_int, FP, FP, FP, FP, FP]),
    # step statistics (Handle.step_stats, BatchHandle.step_stats) and the episodes that log them per step (run_episode(..., stats=True))
    "mppi_step_stats": (C.c_int, [_H, FP, UP, UP]),
    "mppi_batch_step_stats": (C.c_int, [_H, FP, UP, UP]),
    "mppi_run_episode_stats": (C.c_int, [_H, C.POINTER(_H), C.c_int, FP, C.c_int, C.c_int, FP, FP, FP, FP, FP, FP, UP, UP]),
    "mppi_batch_run_episode_stats": (C.c_int, [_H, C.POINTER(_H), C.c_int, FP, C.c_int, C.c_int, FP, FP, FP, FP, FP, FP, UP, UP]),
    # open-loop rollouts of the handle's model (Handle.model_rollout, model_rollout_device)
    "mppi_model_rollout": (C.c_int, [_H, FP, C.c_int, FP, C.c_int, C.c_int, FP, FP]),
    "mppi_model_rollout_device": (C.c_int, [_H, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the learner (LearnerBase.train / _train_step)
    "mppi_learner_create": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(FP), C.POINTER(FP), C.c_int, C.POINTER(_H)]),
    "mppi_learner_destroy": (None, [_H]),
    "mppi_learner_last_error": (C.c_char_p, [_H]),
    "mppi_learner_set_data": (C.c_int, [_H, FP, FP, C.c_int]),
    "mppi_learner_train": (C.c_int, [_H, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, FP, FP]),
    "mppi_learner_evaluate": (C.c_int, [_H, FP, FP, FP]),
    "mppi_learner_gradients": (C.c_int, [_H, FP, C.POINTER(FP), C.POINTER(FP)]),
    "mppi_learner_get_weights": (C.c_int, [_H, C.POINTER(FP), C.POINTER(FP)]),
    "mppi_learner_set_weights": (C.c_int, [_H, C.POINTER(FP), C.POINTER(FP)]),
    "mppi_learner_reset_optimizer": (C.c_int, [_H]),
    "mppi_learner_get_step": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "mppi_learner_save": (C.c_int, [_H, C.c_char_p, DP, DP, DP, DP]),
    "mppi_learner_load": (C.c_int, [_H, C.c_char_p, DP, DP, DP, DP, C.POINTER(C.c_int)]),
    "mppi_learner_peek": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int32)]),
    # batched learners (LearnerBase.k_fold_validation / grid_search)
    "mppi_learner_batch_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(FP), C.POINTER(FP), C.c_int, C.POINTER(_H)]),
    "mppi_learner_batch_destroy": (None, [_H]),
    "mppi_learner_batch_last_error": (C.c_char_p, [_H]),
    "mppi_learner_batch_size": (C.c_int, [_H]),
    "mppi_learner_batch_set_data": (C.c_int, [_H, FP, FP, C.c_int]),
    "mppi_learner_batch_set_split": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "mppi_learner_batch_set_weights": (C.c_int, [_H, C.c_int, C.POINTER(FP), C.POINTER(FP)]),
    "mppi_learner_batch_get_weights": (C.c_int, [_H, C.c_int, C.POINTER(FP), C.POINTER(FP)]),
    "mppi_learner_batch_reset_optimizer": (C.c_int, [_H]),
    "mppi_learner_batch_get_step": (C.c_int, [_H, C.POINTER(C.c_int)]),
    "mppi_learner_batch_train": (C.c_int, [_H, C.c_int, FP, FP, FP, FP, FP, FP]),
    "mppi_learner_batch_evaluate": (C.c_int, [_H, FP, FP]),
    # ... their trajectory validation (LearnerBatch.rollout, LearnerBase.validate_fold)
    "mppi_learner_batch_rollout": (C.c_int, [_H, C.POINTER(LearnerModel), FP, C.c_int, FP, FP, C.c_int, C.c_int, DP, FP]),
}
# batched wide learners ([in, 256, 256, out]): the narrow batch's twelve signatures under another prefix
SIGNATURES.update({"mppi_learner_wide_batch_" + e: SIGNATURES["mppi_learner_batch_" + e] for e in (
    "create", "destroy", "last_error", "size", "set_data", "set_split", "set_weights", "get_weights", "reset_optimizer", "get_step", "train",
    "evaluate")})
# ... and their trajectory validation: mppi_learner_batch_rollout's signature under a name of its own (WideLearnerBatch.validate)
SIGNATURES["mppi_learner_wide_batch_validate"] = SIGNATURES["mppi_learner_batch_rollout"]

_lib = None


def load():
    """Load libmppi_hip.so (built in-tree by build.py). Raises OSError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (one HIP runtime per process — see module docstring)
    if not os.path.exists(SO_PATH):
        raise OSError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950). There is no CPU fallback." % SO_PATH)
    lib = C.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.mppi_abi_version() != 5:
        raise OSError("libmppi_hip.so ABI version mismatch")
    _lib = lib
    return lib


def f32(x, shape=None):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    return a.reshape(shape) if shape is not None else a


def fp(a):
    return a.ctypes.data_as(FP) if a is not None else None


def _mlp_desc(mlp, n_in, n_out):
    """mppi_mlp_desc of an mlp dict(W, b[, xmean, xstd, ymean, ystd]) -> (desc, objects that must outlive its use)"""
    Ws = [f32(w) for w in mlp["W"]]
    bs = [f32(b).ravel() for b in mlp["b"]]
    held = Ws + bs
    desc = MlpDesc()
    desc.n_layers = len(Ws)
    widths = (C.c_int32 * len(Ws))(*[w.shape[1] for w in Ws])
    Wp = (FP * len(Ws))(*[fp(w) for w in Ws])
    bp = (FP * len(bs))(*[fp(b) for b in bs])
    desc.widths, desc.W, desc.b = widths, Wp, bp
    for name, n in (("xmean", n_in), ("xstd", n_in), ("ymean", n_out), ("ystd", n_out)):
        if mlp.get(name) is not None:
            held.append(f32(mlp[name], (n,)))
            setattr(desc, name, fp(held[-1]))
    return desc, held + [desc, widths, Wp, bp]


def _fill_13state(cfg, keep, auv, quat_cost, ellipse3d, Q):
    """the Fossen AUV model (auv: the reference's AUVModel `parameters` dict), StaticQuatCost (quat_cost, with Q [10,10] or its 10 diagonal
    entries) and ElipseCost3D (ellipse3d dict) into cfg, as Handle and BatchHandle take them; the arrays cfg points to are appended to
    `keep`. Returns the Q that is left for the quadratic cost (None once StaticQuatCost took it)."""
    if auv is not None:
        d = AuvDesc()
        d.mass, d.volume, d.density, d.gravity = auv["mass"], auv["volume"], auv["density"], auv.get("gravity", 0.0)
        d.rk = int(auv.get("rk", 1))  # auv_model.py:111-114: rk defaults to 1 when the parameters do not carry it
        for i in range(3):
            d.cog[i], d.cob[i] = auv["cog"][i], auv["cob"][i]
        for i, key in enumerate(("ixx", "iyy", "izz", "ixy", "ixz", "iyz")):
            d.inertial[i] = auv["inertial"][key]

        def mat6(key):  # a 6-vector is the diagonal (auv_model.py:186-195)
            if auv.get(key) is None:
                return None
            m6 = np.asarray(auv[key], np.float32)
            keep.append(f32(np.diag(m6) if m6.shape == (6,) else m6, (36,)))
            return fp(keep[-1])
        d.added_mass, d.linear_damping = mat6("Ma"), mat6("linear_damping")
        d.linear_damping_forward_speed = mat6("linear_damping_forward_speed")
        if auv.get("quad_damping") is not None:
            keep.append(f32(auv["quad_damping"], (6,)))
            d.quad_damping = fp(keep[-1])
        keep.append(d)
        cfg.model_kind, cfg.auv = MODEL_AUV, C.pointer(d)
    if quat_cost:
        q = f32(Q if Q is not None else np.ones(10))
        keep.append(f32(np.diag(q) if q.ndim == 1 else q, (100,)))
        cfg.state_cost_kind, cfg.quat_Q = STATE_COST_QUAT, fp(keep[-1])
        Q = None
    if ellipse3d is not None:
        e = ellipse3d
        keep.append(f32(list(np.ravel(e["normal"])) + list(np.ravel(e["aVec"])) + list(np.ravel(e["axis"])) + [e["speed"], e["m_state"], e["m_vel"]], (11,)))
        cfg.state_cost_kind, cfg.ellipse3d = STATE_COST_ELLIPSE3D, fp(keep[-1])
    return Q


def _fill_config(lib, keep, k, tau, s_dim, a_dim, dt=0.1, mass=1.0, lam=1.0, gamma=1.0, upsilon=1.0, sigma=None, goal=None, Q=None,
                 q_is_full=None, action_cost=ACTION_COST_CPP, seed=1, device=0, upsilon_scales_noise=False, mlp_bf16x3=False,
                 fp_contract=False, ellipse=None, auv=None, quat_cost=False, ellipse3d=None):
    """one mppi_config from the keywords Handle and BatchHandle share (a lone controller's, or one member's of a batch); the arrays it
    points to are appended to `keep`"""
    cfg = Config()
    st = lib.mppi_config_init(C.byref(cfg), k, tau, dt, mass, s_dim, a_dim)
    if st != OK:
        raise MppiError(st, "%s (%s)" % ((lib.mppi_last_error(None) or b"").decode(), lib.mppi_status_string(st).decode()))
    cfg.lam, cfg.gamma, cfg.upsilon, cfg.action_cost_kind = lam, gamma, upsilon, action_cost
    cfg.seed, cfg.device = seed, device
    cfg.flags = (1 if upsilon_scales_noise else 0) | (2 if mlp_bf16x3 else 0) | (4 if fp_contract else 0)  # MPPI_FLAG_UPSILON_SCALES_NOISE | _MLP_BF16X3 | _FP_CONTRACT
    if ellipse is not None:  # ElipseCost (elipse_cost.py:9-85): dict or the 7 numbers a, b, cx, cy, speed, m_state, m_vel
        e = [ellipse[key] for key in ("a", "b", "cx", "cy", "speed", "m_state", "m_vel")] if isinstance(ellipse, dict) else ellipse
        keep.append(f32(e, (7,)))
        cfg.state_cost_kind, cfg.ellipse = STATE_COST_ELLIPSE, fp(keep[-1])
    Q = _fill_13state(cfg, keep, auv, quat_cost, ellipse3d, Q)
    if sigma is not None:
        keep.append(f32(sigma, (a_dim, a_dim)))
        cfg.sigma = fp(keep[-1])
    if goal is not None:
        keep.append(f32(goal, (s_dim,)))
        cfg.goal = fp(keep[-1])
    if Q is not None:
        q = f32(Q)
        full = q.ndim == 2 if q_is_full is None else q_is_full
        keep.append(f32(q, (s_dim, s_dim) if full else (s_dim,)))
        cfg.Q, cfg.q_is_full = fp(keep[-1]), int(full)
    return cfg


class StepStats(collections.namedtuple("StepStats", "beta eta ess entropy cost_mean cost_std cost_max best_index n_nonfinite hist_cost "
                                                  "hist_weight k")):
    """The statistics of control steps (include/mppi_c.h, MPPI_STAT_*): every field but k is an array over the leading axes of the call
    ([] for a lone handle's last step, [n] for a batch's, a step axis in front for an episode); hist_cost and hist_weight have 32 bins as
    their last axis; best_index and n_nonfinite are integers; k is the sample count per member, so ess / k is the observer's scale."""
    __slots__ = ()

    @classmethod
    def from_rows(cls, S, Hc, Hw, k):
        """S [..., 9] float32 rows as the library wrote them, Hc / Hw [..., 32] uint32"""
        cols = [S[..., i] for i in range(N_STEP_STATS)]
        cols[7], cols[8] = cols[7].astype(np.int64), cols[8].astype(np.int64)
        return cls(*cols, Hc, Hw, int(k))


class _HandleBase:
    """What a lone controller (Handle) and a batch (BatchHandle) share: one mppi_handle `h` of `lib`, owned until close()."""

    def _check(self, st, h=True):
        if st != OK:
            txt = self.lib.mppi_last_error(self.h if (h and self.h) else None) or b""
            raise MppiError(st, "%s (%s)" % (txt.decode(), self.lib.mppi_status_string(st).decode()))

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.mppi_destroy(h)

    def __del__(self):
        # At interpreter shutdown the module globals and the ctypes function objects may already be torn down (VERDICT r02:
        # "TypeError: 'NoneType' object is not callable" from __del__ = close): a finaliser must never raise.
        try:
            self.close()
        except Exception:
            pass

    def set_tuning(self, key, value):
        self._check(self.lib.mppi_set_tuning(self.h, TUNING[key], int(value)))

    def get_step_counter(self):
        v = C.c_uint64(0)
        self._check(self.lib.mppi_get_step_counter(self.h, C.byref(v)))
        return int(v.value)

    def set_step_counter(self, step):
        self._check(self.lib.mppi_set_step_counter(self.h, step))

    def _debug_get(self, what, call):
        """one debug item (a member's, of a batch) through call(what, out, n), in the item's shape"""
        n = {DBG_COSTS: self.k_local, DBG_BETA: 1, DBG_ETA: 1, DBG_WEIGHTS: self.k_local,
             DBG_NOISE: self.k_local * self.tau * self.a, DBG_U_UPDATED: self.tau * self.a, DBG_AUX: 8}[what]
        out = np.zeros(n, np.float32)
        self._check(call(what, fp(out), n))
        if what == DBG_NOISE:
            return out.reshape(self.k_local, self.tau, self.a)
        if what == DBG_U_UPDATED:
            return out.reshape(self.tau, self.a)
        return out if n > 1 else out[0]

    @staticmethod
    def _stream(stream):
        """The C-ABI's `void *stream` from what a Python caller holds. None = the handle's own stream (NULL in C). A torch stream object or its
        `.cuda_stream` integer names that stream — and torch's DEFAULT stream, whose handle is 0, is passed as hipStreamLegacy (1): a raw 0 that
        came out of torch must never select the handle's own non-blocking stream, which nothing of torch's is ordered against (the stale-record
        race of r04; ADVICE r04: mapped once, here, for every caller)."""
        if stream is None:
            return 0
        v = getattr(stream, "cuda_stream", stream)
        return int(v) or 1

    def set_action_limits(self, a_min=None, a_max=None):
        """clip_act (controller_base.py:500-504): clamp U' rows to [a_min, a_max] (a batch: every member's, the limits are shared);
        None, None = off"""
        if a_min is None and a_max is None:
            self._check(self.lib.mppi_set_action_limits(self.h, None, None, 0))
            return
        lo, hi = f32(a_min, (self.a,)), f32(a_max, (self.a,))
        self._check(self.lib.mppi_set_action_limits(self.h, fp(lo), fp(hi), self.a))

    def synchronize(self):
        self._check(self.lib.mppi_synchronize(self.h))

    def _step_stats(self, name, lead):
        """the statistics of the last step through the entry point `name`; lead as in _run_episode"""
        S = np.zeros((*lead, N_STEP_STATS), np.float32)
        Hc, Hw = np.zeros((*lead, STEP_STAT_BINS), np.uint32), np.zeros((*lead, STEP_STAT_BINS), np.uint32)
        self._check(getattr(self.lib, name)(self.h, fp(S), Hc.ctypes.data_as(UP), Hw.ctypes.data_as(UP)))
        return StepStats.from_rows(S, Hc, Hw, self.k_local)

    def _run_episode(self, name, lead, x0, n_steps, goals, disturbance, plant=None, stats=False):
        """n_steps closed-loop steps through the entry point `name` (mppi_run_episode / mppi_batch_run_episode); lead = () for a lone handle, (n,) for a batch:
        x0 [*lead, s], goals / disturbance [n_steps, *lead, s] or None -> (X [n_steps+1, *lead, s], U [n_steps, *lead, a], C [n_steps, *lead]).
        plant: None (the handle's own model, through `name`), a Handle, or for a batch a sequence of n Handles (through `name`_plant).
        stats: True -> (X, U, C, StepStats) through `name`_stats, the statistics of every step with a leading step axis.
        Shapes and the plant count are checked here, before the library is called: a bad one raises ValueError."""
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1, not %d" % n_steps)
        plants = None
        if plant is not None:
            plants = [plant] if isinstance(plant, Handle) else (list(plant) if isinstance(plant, (list, tuple)) else None)
            if plants is None or not all(isinstance(p, Handle) for p in plants):
                raise ValueError("plant must be a Handle%s" % (" or a sequence of %d Handles" % lead[0] if lead else ""))
            if len(plants) != 1 and (not lead or len(plants) != lead[0]):
                raise ValueError("plant must be one Handle%s, not %d" % (" or %d of them" % lead[0] if lead else "", len(plants)))

        def shaped(name, v, shape):
            v = np.asarray(v, dtype=np.float32)
            if v.shape != shape:
                raise ValueError("%s must have shape %s, not %s" % (name, shape, v.shape))
            return np.ascontiguousarray(v)
        x0 = shaped("x0", x0, (*lead, self.s))
        goals = None if goals is None else shaped("goals", goals, (n_steps, *lead, self.s))
        disturbance = None if disturbance is None else shaped("disturbance", disturbance, (n_steps, *lead, self.s))
        X = np.zeros((n_steps + 1, *lead, self.s), np.float32)
        U = np.zeros((n_steps, *lead, self.a), np.float32)
        Cs = np.zeros((n_steps, *lead), np.float32)
        if stats:
            S = np.zeros((n_steps, *lead, N_STEP_STATS), np.float32)
            Hc, Hw = np.zeros((n_steps, *lead, STEP_STAT_BINS), np.uint32), np.zeros((n_steps, *lead, STEP_STAT_BINS), np.uint32)
            ph = None if plants is None else (_H * len(plants))(*[p.h for p in plants])
            self._check(getattr(self.lib, name + "_stats")(self.h, ph, len(plants or ()), fp(x0), x0.size, n_steps, fp(goals), fp(disturbance),
                                                           fp(X), fp(U), fp(Cs), fp(S), Hc.ctypes.data_as(UP), Hw.ctypes.data_as(UP)))
            return X, U, Cs, StepStats.from_rows(S, Hc, Hw, self.k_local)
        if plants is None:
            self._check(getattr(self.lib, name)(self.h, fp(x0), x0.size, n_steps, fp(goals), fp(disturbance), fp(X), fp(U), fp(Cs)))
            return X, U, Cs
        ph = (_H * len(plants))(*[p.h for p in plants])
        self._check(getattr(self.lib, name + "_plant")(self.h, ph, len(plants), fp(x0), x0.size, n_steps, fp(goals), fp(disturbance), fp(X), fp(U),
                                                       fp(Cs)))
        return X, U, Cs

    def rollout_kernel_name(self):
        buf = C.create_string_buffer(128)
        self._check(self.lib.mppi_rollout_kernel_name(self.h, buf, 128))
        return buf.value.decode()

    def profile_begin(self, max_steps):
        self._check(self.lib.mppi_profile_begin(self.h, max_steps))

    def profile_end(self):
        """-> (rollout kernel ms avg, finish kernel ms avg, steps recorded); HIP events on the launch stream."""
        r, f, n = C.c_float(0), C.c_float(0), C.c_int(0)
        self._check(self.lib.mppi_profile_end(self.h, C.byref(r), C.byref(f), C.byref(n)))
        return r.value, f.value, n.value


class Handle(_HandleBase):
    """RAII wrapper of one mppi_handle (one controller on one GPU)."""

    def __init__(self, k, tau, s_dim, a_dim, dt=0.1, mass=1.0, lam=1.0, gamma=1.0, upsilon=1.0,
                 sigma=None, goal=None, Q=None, q_is_full=None, action_cost=ACTION_COST_CPP,
                 normalize_cost=False, seed=1, device=0, shard_rank=0, shard_count=1, mlp=None,
                 upsilon_scales_noise=False, mlp_bf16x3=False, fp_contract=False, tuning=None, log_rows=0, ellipse=None,
                 auv=None, nnauv=None, quat_cost=False, ellipse3d=None, nnauv_speed=None):
        """mlp: dict(W=[W1,W2,W3], b=[b1,b2,b3], xmean=, xstd=, ymean=, ystd=) selects the learned
        model_base (Dense(256,relu) x2 + Dense(s_dim); Keras [in x out] kernels).
        tuning: dict of diagnostic switches (keys of TUNING) applied with mppi_set_tuning right after creation.
        log_rows: capacity of the transition log (mppi_set_transition_log); 0 = off.
        auv: the reference's AUVModel `parameters` dict (auv_model.py:85-245: mass, volume, density, cog, cob, Ma, linear_damping,
        quad_damping, linear_damping_forward_speed, inertial{ixx..iyz}, rk) selects the Fossen model (s_dim 13, a_dim 6);
        nnauv: an mlp dict whose first kernel has s+a-3 = 16 rows selects NNAUVModel (nn_model.py:179-304);
        nnauv_speed: an mlp dict with 15 input rows (Euler angles, velocities, forces) and 6 outputs selects NNAUVModelSpeed (nn_model.py:307-588);
        quat_cost: StaticQuatCost (static_cost.py:73-159) with goal [13] and Q [10,10] (or its 10 diagonal entries);
        ellipse3d: dict(normal, aVec, axis, speed, m_state, m_vel) selects ElipseCost3D (elipse_cost.py:101-246)."""
        lib = self.lib = load()
        keep = []
        cfg = _fill_config(lib, keep, k, tau, s_dim, a_dim, dt=dt, mass=mass, lam=lam, gamma=gamma, upsilon=upsilon, sigma=sigma, goal=goal, Q=Q,
                           q_is_full=q_is_full, action_cost=action_cost, seed=seed, device=device, upsilon_scales_noise=upsilon_scales_noise,
                           mlp_bf16x3=mlp_bf16x3, fp_contract=fp_contract, ellipse=ellipse, auv=auv, quat_cost=quat_cost, ellipse3d=ellipse3d)
        cfg.normalize_cost, cfg.shard_rank, cfg.shard_count = int(bool(normalize_cost)), shard_rank, shard_count
        if nnauv is not None:
            mlp = nnauv
        if nnauv_speed is not None:
            mlp = nnauv_speed
        self._mlp_io = None
        if mlp is not None:
            n_in = 15 if nnauv_speed is not None else s_dim + a_dim - (3 if nnauv is not None else 0)
            self._mlp_io = (n_in, 6 if nnauv_speed is not None else s_dim)
            desc, held = _mlp_desc(mlp, *self._mlp_io)
            keep += held
            cfg.model_kind = MODEL_NN_AUV_SPEED if nnauv_speed is not None else (MODEL_NN_AUV if nnauv is not None else MODEL_MLP)
            cfg.mlp = C.pointer(desc)
        self.h = _H()
        self.k, self.tau, self.s, self.a = k, tau, s_dim, a_dim
        st = lib.mppi_create(C.byref(cfg), C.byref(self.h))
        if st != OK:
            self.h = _H()
            self._check(st, None)
        self.k_local = lib.mppi_local_samples(self.h)
        self._stage = None
        self.k_offset = lib.mppi_sample_offset(self.h)
        self.record_size = lib.mppi_record_size(self.h)
        for key, val in (tuning or {}).items():
            self.set_tuning(key, val)
        if log_rows:
            self.set_transition_log(log_rows)

    def set_tuning(self, key, value):
        if key == "p2p_fault" and isinstance(value, str):
            value = P2P_FAULTS[value]
        super().set_tuning(key, value)

    def set_transition_log(self, max_rows):
        self._check(self.lib.mppi_set_transition_log(self.h, int(max_rows)))

    # ---- host loop -------------------------------------------------------------------
    def set_goal(self, goal):
        g = f32(goal).ravel()
        self._check(self.lib.mppi_set_goal(self.h, fp(g), g.size))

    def set_mlp(self, mlp):
        """mppi_set_mlp: new weights / normalisation for a learned-model handle (same layer widths), from the next step on"""
        if self._mlp_io is None:
            raise MppiError(1, "not a learned-model handle")
        desc, held = _mlp_desc(mlp, *self._mlp_io)
        self._check(self.lib.mppi_set_mlp(self.h, C.byref(desc)))
        del held

    def next(self, x):
        # persistent staging arrays with ready-made ctypes pointers: building them per call costs more host time
        # (~5 us) than the launch of the step itself
        if self._stage is None:
            xs, us = np.zeros(self.s, np.float32), np.zeros(self.a, np.float32)
            self._stage = (xs, us, fp(xs), fp(us))
        xs, us, xp, up = self._stage
        xin = np.asarray(x).reshape(-1)
        if xin.size != self.s:  # let the C-ABI report it (MPPI_ERR_INVALID_ARG, as the reference's size checks)
            xin = f32(xin)
            self._check(self.lib.mppi_next(self.h, fp(xin), xin.size, up, self.a))
        xs[:] = xin
        st = self.lib.mppi_next(self.h, xp, self.s, up, self.a)
        if st != OK:
            self._check(st)
        return us.copy()

    def next_with_noise(self, x, eps):
        x, eps = f32(x).ravel(), f32(eps).ravel()
        u = np.zeros(self.a, np.float32)
        self._check(self.lib.mppi_next_with_noise(self.h, fp(x), x.size, fp(eps), eps.size, fp(u), u.size))
        return u

    def step_stats(self):
        """mppi_step_stats: the StepStats of the last step (effective sample size, entropy, cost moments, best sample, histograms),
        computed on the device from what the step left there; refused before the first step and on a sharded handle"""
        return self._step_stats("mppi_step_stats", ())

    def run_episode(self, x0, n_steps, goals=None, disturbance=None, *, plant=None, stats=False):
        """mppi_run_episode: n_steps control steps on the device with the handle's own model as the plant, no host round trip between them.
        x0 [s]; goals [n_steps, s]: the goal in force at step t; disturbance [n_steps, s]: w_t added to the plant's x'
        -> (X [n_steps+1, s] the realised trajectory, U [n_steps, a] the controls, C [n_steps] the state cost of x_t under step t's goal).
        The handle ends where the host loop set_goal, next, model_next leaves it.
        plant: another Handle (lone, unsharded, same device, s_dim and a_dim) whose model steps the state instead (mppi_run_episode_plant):
        x' is plant.model_next(x, u); nothing else of the plant is read, and nothing of it is written.
        stats=True (mppi_run_episode_stats): -> (X, U, C, StepStats), every field of the StepStats with a leading [n_steps] axis: what
        step_stats() would return after each step, logged on the device; X, U and C are bit for bit those of stats=False."""
        return self._run_episode("mppi_run_episode", (), x0, n_steps, goals, disturbance, plant, stats)

    def save_next(self, x_next):
        x = f32(x_next).ravel()
        self._check(self.lib.mppi_save_next(self.h, fp(x), x.size))

    def transition_log_stats(self):
        """-> dict(held, overwritten, without_successor): what to_csv will and will not write"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.mppi_transition_log_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(held=int(a.value), overwritten=int(b.value), without_successor=int(c.value))

    def to_csv(self, filename, fmt=CSV_REFERENCE):
        """DataBase::toCSV; fmt = CSV_REFERENCE (the reference's bytes) or CSV_ROUNDTRIP (%.9g, no trailing commas)"""
        self._check(self.lib.mppi_to_csv_format(self.h, os.fsencode(filename), fmt))

    # ---- state -----------------------------------------------------------------------
    def get_action_sequence(self):
        U = np.zeros((self.tau, self.a), np.float32)
        self._check(self.lib.mppi_get_action_sequence(self.h, fp(U), U.size))
        return U

    def set_action_sequence(self, U):
        U = f32(U).ravel()
        self._check(self.lib.mppi_set_action_sequence(self.h, fp(U), U.size))

    def debug_get(self, what):
        return self._debug_get(what, lambda *args: self.lib.mppi_debug_get(self.h, *args))

    # ---- graph helpers ---------------------------------------------------------------
    def model_next(self, x, v):
        """next state only (works for the learned model too) -> [k,s]"""
        x, v = f32(x, (-1, self.s)), f32(v, (-1, self.a))
        nx = np.zeros((v.shape[0], self.s), np.float32)
        self._check(self.lib.mppi_model_step(self.h, fp(x), x.shape[0], fp(v), v.shape[0], None, None, fp(nx)))
        return nx

    def model_step(self, x, v):
        """-> (free [kx,s], action [k,s], next [k,s])"""
        x, v = f32(x, (-1, self.s)), f32(v, (-1, self.a))
        kx, k = x.shape[0], v.shape[0]
        fr, ac, nx = np.zeros((kx, self.s), np.float32), np.zeros((k, self.s), np.float32), np.zeros((k, self.s), np.float32)
        self._check(self.lib.mppi_model_step(self.h, fp(x), kx, fp(v), k, fp(fr), fp(ac), fp(nx)))
        return fr, ac, nx

    def auv_pieces(self, x, u):
        """AUVModel's intermediates for k (state, action) pairs -> dict(rot [k,3,3], T [k,4,3], Cv, Dv, g [k,6], xdot [k,13])"""
        x, u = f32(x, (-1, 13)), f32(u, (-1, 6))
        k = x.shape[0]
        out = np.zeros((k, 124), np.float32)
        self._check(self.lib.mppi_auv_pieces(self.h, fp(x), fp(u), k, fp(out)))
        return dict(rot=out[:, :9].reshape(k, 3, 3), T=out[:, 9:21].reshape(k, 4, 3), Cv=out[:, 21:27], Dv=out[:, 27:33], g=out[:, 33:39],
                    xdot=out[:, 39:52], D=out[:, 52:88].reshape(k, 6, 6), C=out[:, 88:124].reshape(k, 6, 6))

    def ellipse3d_terms(self, x, in_plane_frame=False):
        """ElipseCost3D's (position, orientation, velocity) errors of k states -> [k,3]"""
        x = f32(x, (-1, 13))
        out = np.zeros((x.shape[0], 3), np.float32)
        self._check(self.lib.mppi_ellipse3d_terms(self.h, fp(x), x.shape[0], int(bool(in_plane_frame)), fp(out)))
        return out

    def state_cost(self, x):
        x = f32(x, (-1, self.s))
        out = np.zeros(x.shape[0], np.float32)
        self._check(self.lib.mppi_state_cost(self.h, fp(x), x.shape[0], fp(out)))
        return out

    def action_cost(self, u, eps):
        u, eps = f32(u, (self.a,)), f32(eps, (-1, self.a))
        out = np.zeros(eps.shape[0], np.float32)
        self._check(self.lib.mppi_action_cost(self.h, fp(u), fp(eps), eps.shape[0], fp(out)))
        return out

    def step_cost(self, x, u, eps):
        x, u, eps = f32(x, (-1, self.s)), f32(u, (self.a,)), f32(eps, (-1, self.a))
        out = np.zeros(x.shape[0], np.float32)
        self._check(self.lib.mppi_step_cost(self.h, fp(x), fp(u), fp(eps), x.shape[0], fp(out)))
        return out

    def rollout_cost(self, x, U, eps):
        x, U = f32(x, (self.s,)), f32(U, (self.tau, self.a))
        eps = f32(eps, (self.k_local, self.tau, self.a))
        out = np.zeros(self.k_local, np.float32)
        self._check(self.lib.mppi_rollout_cost(self.h, fp(x), fp(U), fp(eps), fp(out)))
        return out

    def update(self, cost, eps, U):
        """-> dict(beta, arg, exp, nabla, w, wn, Unew) (exp_arg is 'arg', weights 'w', weighted noise 'wn')"""
        K = self.k_local
        cost, U = f32(cost, (K,)), f32(U, (self.tau, self.a))
        eps = f32(eps, (K, self.tau, self.a))
        beta, nabla = np.zeros(1, np.float32), np.zeros(1, np.float32)
        arg, e, w = (np.zeros(K, np.float32) for _ in range(3))
        wn, Un = np.zeros((self.tau, self.a), np.float32), np.zeros((self.tau, self.a), np.float32)
        self._check(self.lib.mppi_update(self.h, fp(cost), fp(eps), fp(U), fp(beta), fp(arg), fp(e), fp(nabla),
                                         fp(w), fp(wn), fp(Un)))
        return dict(beta=beta[0], arg=arg, exp=e, nabla=nabla[0], w=w, wn=wn, Unew=Un)

    # ---- open-loop rollouts (mppi_model_rollout, include/mppi_c.h) -------------------------------
    def model_rollout(self, x0, V, costs=True):
        """The handle's model rolled along given action sequences, in ONE call: V [T, a] -> (X [T+1, s], C [T]); V [T, n, a] ->
        (X [T+1, n, s], C [T, n]), the step axis first. x0 is [s] (shared by every trajectory) or [n, s]. X[0] = x0, X[t+1] =
        model_next(X[t], V[t]) and C[t] = state_cost(X[t+1]) under the current goal, bit for bit those helpers' values; T is free of tau.
        costs=False: no cost arithmetic, C is None. Nothing of the handle changes. A learned model's trajectory is the reference-ordered
        evaluation model_next gives, not the rounding of a control step's matrix-core rollouts.
        Shapes are checked here, before the library is called: a bad one raises ValueError."""
        V = np.asarray(V, dtype=np.float32)
        x0 = np.asarray(x0, dtype=np.float32)
        if V.ndim not in (2, 3) or V.shape[-1] != self.a:
            raise ValueError("V must have shape (T, %d) or (T, n, %d), not %s" % (self.a, self.a, V.shape))
        lone = V.ndim == 2
        T, n = V.shape[0], 1 if lone else V.shape[1]
        if T < 1 or n < 1:
            raise ValueError("V must hold T >= 1 steps of n >= 1 trajectories, not %s" % (V.shape,))
        good = [(self.s,), (1, self.s)] + ([] if lone else [(n, self.s)])
        if x0.shape not in good:
            raise ValueError("x0 must have shape %s, not %s" % (" or ".join(str(g) for g in good), x0.shape))
        x0, V = np.ascontiguousarray(x0).reshape(-1, self.s), np.ascontiguousarray(V).reshape(T, n, self.a)
        X = np.zeros((T + 1, n, self.s), np.float32)
        Cs = np.zeros((T, n), np.float32) if costs else None
        self._check(self.lib.mppi_model_rollout(self.h, fp(x0), x0.shape[0], fp(V), n, T, fp(X), fp(Cs)))
        if lone:
            return X[:, 0], (Cs[:, 0] if costs else None)
        return X, Cs

    def model_rollout_device(self, x0_ptr, kx, V_ptr, n, T, X_ptr, C_ptr=0, stream=None):
        """mppi_model_rollout_device: the same on device pointers (ints: tensor.data_ptr()), enqueue only. x0 [kx, s] with kx in {1, n},
        V [T, n, a] -> X [T+1, n, s] (required), C [T, n] (0: none). stream: next_device's convention."""
        self._check(self.lib.mppi_model_rollout_device(self.h, x0_ptr, int(kx), V_ptr, int(n), int(T), X_ptr, C_ptr or None,
                                                       self._stream(stream)))

    def sample_trajectories(self, x, U_before, ks):
        """What the controller planned in the LAST step, read out on the host side: the trajectories of the samples `ks` (indices into the
        handle's k_local samples). x: the state the step ran from; U_before [tau, a]: the sequence the step started from, read with
        get_action_sequence() BEFORE next(). -> (X [tau+1, m, s], C [tau, m], eps [m, tau, a]) with m = len(ks): the noise rows of those
        samples, and model_rollout of V = U_before + eps[k] (an fp32 add: the kernels' v = u + e, without action limits).
        A diagnostic: it regenerates and copies the whole noise array of the step (debug_get(DBG_NOISE)) to take m rows of it."""
        ks = np.asarray(ks, dtype=np.int64).reshape(-1)
        if ks.size < 1 or ks.min() < 0 or ks.max() >= self.k_local:
            raise ValueError("ks must hold sample indices in [0, %d)" % self.k_local)
        U = np.asarray(U_before, dtype=np.float32)
        if U.shape != (self.tau, self.a):
            raise ValueError("U_before must have shape %s, not %s" % ((self.tau, self.a), U.shape))
        eps = np.ascontiguousarray(self.debug_get(DBG_NOISE)[ks])
        V = (U[None] + eps).astype(np.float32)
        X, Cs = self.model_rollout(np.asarray(x, dtype=np.float32).reshape(self.s), np.ascontiguousarray(V.transpose(1, 0, 2)))
        return X, Cs, eps

    # ---- device-resident step (pointers are ints: tensor.data_ptr()) -----
    def next_device(self, x_ptr, u_ptr, stream=None):
        self._check(self.lib.mppi_next_device(self.h, x_ptr, u_ptr, self._stream(stream)))

    def shard_partial(self, x_ptr, record_ptr, stream=None):
        self._check(self.lib.mppi_shard_partial(self.h, x_ptr, record_ptr, self._stream(stream)))

    def shard_finish(self, records_ptr, n_records, u_ptr, stream=None):
        self._check(self.lib.mppi_shard_finish(self.h, records_ptr, n_records, u_ptr, self._stream(stream)))

    def shard_cost_range(self, x_ptr, range_ptr, stream=None):
        """normalize_cost on a sharded handle, first half: {-min, max} of this shard's sample costs -> range_ptr[2]"""
        self._check(self.lib.mppi_shard_cost_range(self.h, x_ptr, range_ptr, self._stream(stream)))

    def shard_partial_normalized(self, x_ptr, range_ptr, record_ptr, stream=None):
        """... second half: range_ptr[2] = the {-min, max} all ranks agreed on (all-reduce MAX) -> this shard's record"""
        self._check(self.lib.mppi_shard_partial_normalized(self.h, x_ptr, range_ptr, record_ptr, self._stream(stream)))

    # ---- options of the Python reference's update ---------------------------------------------
    def shard_step(self, x_ptr, u_ptr, coll=None, stream=None):
        """mppi_shard_step: the whole sharded step in ONE call; coll = a Collectives (or None on an unsharded handle: record -> finish)"""
        self._check(self.lib.mppi_shard_step(self.h, x_ptr, u_ptr, C.byref(coll) if coll is not None else None, self._stream(stream)))

    def set_sequence_filter(self, window, polyorder=3):
        """filterSeq (controller_base.py:277-291): Savitzky-Golay smoothing of the stored sequence; window 0 = off"""
        self._check(self.lib.mppi_set_sequence_filter(self.h, int(window), int(polyorder)))

    # ---- direct record exchange (mppi_shard_p2p_*, include/mppi_c.h) -------------------------
    def p2p_export(self, want_ipc=True):
        """-> (inbox device pointer, 64-byte hipIpcMemHandle_t as bytes or None)"""
        buf = C.create_string_buffer(64) if want_ipc else None
        ptr = C.c_void_p()
        self._check(self.lib.mppi_shard_p2p_export(self.h, buf, C.byref(ptr)))
        return ptr.value, (buf.raw if want_ipc else None)

    def p2p_open(self, ipc_handle):
        """map another process's inbox -> device pointer valid here"""
        ptr = C.c_void_p()
        self._check(self.lib.mppi_shard_p2p_open(self.h, C.create_string_buffer(ipc_handle, 64), C.byref(ptr)))
        return ptr.value

    def p2p_attach(self, inbox_ptrs, timeout_ms=2000):
        arr = (C.c_void_p * len(inbox_ptrs))(*inbox_ptrs)
        self._check(self.lib.mppi_shard_p2p_attach(self.h, arr, len(inbox_ptrs), timeout_ms))

    def p2p_probe(self, stream=None):
        ok = C.c_int(0)
        self._check(self.lib.mppi_shard_p2p_probe(self.h, self._stream(stream), C.byref(ok)))
        return bool(ok.value)

    def p2p_step(self, x_ptr, u_ptr, stream=None):
        self._check(self.lib.mppi_shard_p2p_step(self.h, x_ptr, u_ptr, self._stream(stream)))

    def p2p_timed_out(self):
        t = C.c_int(0)
        self._check(self.lib.mppi_shard_p2p_status(self.h, C.byref(t)))
        return bool(t.value)


# BatchHandle's per-member keywords: each replaces the shared keyword of the same name without the plural s
BATCH_PER_MEMBER = {"lams": "lam", "gammas": "gamma", "upsilons": "upsilon", "sigmas": "sigma", "Qs": "Q"}


def batch_configs(n, k, tau, s_dim, a_dim, dt=0.1, mass=1.0, lam=1.0, gamma=1.0, upsilon=1.0, sigma=None, goal=None, Q=None,
                  q_is_full=None, action_cost=ACTION_COST_CPP, seed=1, seeds=None, device=0, upsilon_scales_noise=False, auv=None,
                  quat_cost=False, ellipse3d=None, lams=None, gammas=None, upsilons=None, sigmas=None, Qs=None):
    """-> (Config array [n] for mppi_create_batch_configs, objects that must outlive its use). Member m's config is the shared keywords'
    with lam, gamma, upsilon, sigma and Q replaced by lams[m], gammas[m], upsilons[m], sigmas[m] ([a, a]) and Qs[m] ([s] or [s, s]) where
    those are given, and seed = seeds[m] (None: seed + m, as mppi_create_batch). A list of the wrong length raises MppiError(ERR_INVALID_ARG)."""
    lib = load()
    per = dict(lams=lams, gammas=gammas, upsilons=upsilons, sigmas=sigmas, Qs=Qs, seeds=seeds)
    for name, v in per.items():
        if v is not None and len(v) != n:
            raise MppiError(ERR_INVALID_ARG, "%s must hold n = %d entries, not %d" % (name, n, len(v)))
    shared = dict(lam=lam, gamma=gamma, upsilon=upsilon, sigma=sigma, Q=Q)
    cfgs, keep = (Config * n)(), []
    for m in range(n):
        own = {one: (shared[one] if per[many] is None else per[many][m]) for many, one in BATCH_PER_MEMBER.items()}
        cfgs[m] = _fill_config(lib, keep, k, tau, s_dim, a_dim, dt=dt, mass=mass, goal=goal, q_is_full=q_is_full, action_cost=action_cost,
                               seed=int(seeds[m]) if seeds is not None else seed + m, device=device, upsilon_scales_noise=upsilon_scales_noise,
                               auv=auv, quat_cost=quat_cost, ellipse3d=ellipse3d, **own)
    return cfgs, keep


class BatchHandle(_HandleBase):
    """RAII wrapper of a batched mppi_handle (mppi_create_batch / mppi_create_batch_configs): n independent controllers that step in the
    same two launches. Member m is bit for bit Handle(..., seed=seeds[m]) fed the same x, goal and sequence, with lams[m], gammas[m],
    upsilons[m], sigmas[m] and Qs[m] where those are given (include/mppi_c.h)."""

    def __init__(self, n, k, tau, s_dim, a_dim, dt=0.1, mass=1.0, lam=1.0, gamma=1.0, upsilon=1.0, sigma=None, goal=None, goals=None,
                 Q=None, q_is_full=None, action_cost=ACTION_COST_CPP, seed=1, seeds=None, device=0, upsilon_scales_noise=False, tuning=None,
                 auv=None, quat_cost=False, ellipse3d=None, lams=None, gammas=None, upsilons=None, sigmas=None, Qs=None):
        """n members; seeds: n Philox keys (None: seed + m); goal: every member's goal, goals: [n, s_dim] per member (after goal);
        the other keywords as Handle's. tuning: dict of diagnostic switches (keys of TUNING) that a batch takes.
        auv, quat_cost, ellipse3d: as Handle's (the Fossen AUV model, s_dim 13, a_dim 6; StaticQuatCost; ElipseCost3D); goals is then
        [n, 13], next / next_device take x [n, 13] and give u [n, 6].
        lams, gammas, upsilons: n values; sigmas: [n, a_dim, a_dim]; Qs: [n, s_dim] or [n, s_dim, s_dim] — each member's own lambda, gamma,
        upsilon, sigma and quadratic-cost Q (None: the shared keyword). Every member's sigma must be diagonal, or every one dense; so must Q."""
        lib = self.lib = load()
        self.h = _H()
        keep = []
        self.n, self.k, self.tau, self.s, self.a = n, k, tau, s_dim, a_dim
        if all(v is None for v in (lams, gammas, upsilons, sigmas, Qs)):
            cfg = _fill_config(lib, keep, k, tau, s_dim, a_dim, dt=dt, mass=mass, lam=lam, gamma=gamma, upsilon=upsilon, sigma=sigma, goal=goal,
                               Q=Q, q_is_full=q_is_full, action_cost=action_cost, seed=seed, device=device,
                               upsilon_scales_noise=upsilon_scales_noise, auv=auv, quat_cost=quat_cost, ellipse3d=ellipse3d)
            sp = None
            if seeds is not None:
                sv = np.ascontiguousarray(seeds, np.uint64).ravel()
                if sv.size != n:
                    raise MppiError(ERR_INVALID_ARG, "seeds must hold n values")
                keep.append(sv)
                sp = sv.ctypes.data_as(C.POINTER(C.c_uint64))
            st = lib.mppi_create_batch(C.byref(cfg), int(n), sp, C.byref(self.h))
        else:
            cfgs, keep = batch_configs(n, k, tau, s_dim, a_dim, dt=dt, mass=mass, lam=lam, gamma=gamma, upsilon=upsilon, sigma=sigma,
                                       goal=goal, Q=Q, q_is_full=q_is_full, action_cost=action_cost, seed=seed, seeds=seeds, device=device,
                                       upsilon_scales_noise=upsilon_scales_noise, auv=auv, quat_cost=quat_cost, ellipse3d=ellipse3d,
                                       lams=lams, gammas=gammas, upsilons=upsilons, sigmas=sigmas, Qs=Qs)
            st = lib.mppi_create_batch_configs(cfgs, int(n), C.byref(self.h))
        if st != OK:
            self.h = _H()
            self._check(st, None)
        self.k_local = lib.mppi_local_samples(self.h)
        for key, val in (tuning or {}).items():
            self.set_tuning(key, val)
        if goals is not None:
            self.set_goals(goals)

    _LEARNED = {"nnauv": (MODEL_NN_AUV, 16, 13), "nnauv_speed": (MODEL_NN_AUV_SPEED, 15, 6)}  # kind, network inputs, outputs

    @classmethod
    def learned(cls, n, nets, model="nnauv", *, k, tau, a_dim=None, goals=None, tuning=None, normalize_cost=False, shard_count=1,
                mlp_bf16x3=False, fp_contract=False, **cfg):
        """mppi_create_batch_learned: n controllers of a learned 13-state model ("nnauv": NNAUVModel, "nnauv_speed": NNAUVModelSpeed), member m
        with its OWN network. nets: one dict in the `nnauv=` format of Handle (every member gets it) or n of them, all of one shape;
        k, tau and the other keywords as batch_configs' (seeds, goal, lam(s), gamma(s), upsilon(s), sigma(s), Q(s), quat_cost, ellipse3d, ...).
        Member m is bit for bit the lone Handle of its config and network on k_rollout_gen (include/mppi_c.h).
        model="mlp" with a_dim (mppi_create_batch_mlp): n controllers of the learned point mass (s_dim = 2 a_dim), nets in the `mlp=` format
        of Handle: [3a, 256, 256, 2a] (a_dim <= 3) or 1-3 hidden layers of 16 or 32. Member m is bit for bit Handle(..., mlp=nets[m]) on its
        default kernel (Dense(32): the Handle tuned mlp32_valu = 1). A network of the wrong shape raises ValueError before the library is
        called."""
        if model == "mlp":
            if a_dim is None or int(a_dim) < 1:
                raise ValueError('model="mlp" needs a_dim >= 1 (s_dim = 2 a_dim)')
            a, kind = int(a_dim), MODEL_MLP
            s, n_in, n_out = 2 * a, 3 * a, 2 * a
        elif model in cls._LEARNED:
            if a_dim is not None and int(a_dim) != 6:
                raise ValueError("the learned 13-state models have a_dim = 6")
            (kind, n_in, n_out), s, a = cls._LEARNED[model], 13, 6
        else:
            raise ValueError('model must be "nnauv", "nnauv_speed" or "mlp", not %r' % (model,))
        nets = [nets] * n if isinstance(nets, dict) else list(nets)
        if len(nets) != n:
            raise MppiError(ERR_INVALID_ARG, "nets must hold n = %d networks (or be one dict), not %d" % (n, len(nets)))
        if model == "mlp":  # the shapes, before any device work
            shapes = [None if net is None else [tuple(np.shape(w)) for w in net["W"]] for net in nets]
            for m, sh in enumerate(shapes):
                if sh is None:
                    continue
                chain = all(len(x) == 2 for x in sh) and all(sh[l][1] == sh[l + 1][0] for l in range(len(sh) - 1))
                if not sh or not chain or sh[0][0] != n_in or sh[-1][1] != n_out:
                    raise ValueError("nets[%d]: the kernels must chain from %d inputs (s_dim + a_dim) to %d outputs (s_dim), not %s"
                                     % (m, n_in, n_out, sh))
                if [np.size(b) for b in nets[m]["b"]] != [x[1] for x in sh]:
                    raise ValueError("nets[%d]: one bias vector per layer, of the layer's width" % m)
                first = next(x for x in shapes if x is not None)
                if sh != first:
                    raise ValueError("nets[%d]: every member's network has the shape of the first (%s), not %s" % (m, first, sh))
        self = cls.__new__(cls)
        lib = self.lib = load()
        self.h = _H()
        self.n, self.k, self.tau, self.s, self.a = n, k, tau, s, a
        self._mlp_io = (n_in, n_out)
        cfgs, keep = batch_configs(n, k, tau, s, a, **cfg)
        for m in range(n):
            cfgs[m].model_kind = kind
            cfgs[m].normalize_cost, cfgs[m].shard_count = int(bool(normalize_cost)), shard_count
            cfgs[m].flags |= (2 if mlp_bf16x3 else 0) | (4 if fp_contract else 0)
            if nets[m] is not None:
                desc, held = _mlp_desc(nets[m], n_in, n_out)
                keep += held
                cfgs[m].mlp = C.pointer(desc)
        st = (lib.mppi_create_batch_mlp if model == "mlp" else lib.mppi_create_batch_learned)(cfgs, int(n), C.byref(self.h))
        if st != OK:
            self.h = _H()
            self._check(st, None)
        self.k_local = lib.mppi_local_samples(self.h)
        for key, val in (tuning or {}).items():
            self.set_tuning(key, val)
        if goals is not None:
            self.set_goals(goals)
        return self

    def set_mlp(self, member, net):
        """mppi_batch_set_mlp: member's network <- net (member = -1: every member's); the shape is fixed at creation"""
        if getattr(self, "_mlp_io", None) is None:
            raise MppiError(ERR_INVALID_ARG, "not a batch of learned controllers (BatchHandle.learned)")
        desc, held = _mlp_desc(net, *self._mlp_io)
        self._check(self.lib.mppi_batch_set_mlp(self.h, int(member), C.byref(desc)))
        del held

    def load_learners(self, batch, model):
        """Every member's weights of the LearnerBatch or WideLearnerBatch `batch` (as many members as this handle; what is read of it is
        .B and .get_weights(m)), with the normalisation of `model` (LearnerBatch.model_desc: a model object or a dict with xmean, xstd,
        ymean, ystd), into the controllers, through the host."""
        if batch.B != self.n:
            raise MppiError(ERR_INVALID_ARG, "load_learners: the learner batch has %d members, the controllers %d" % (batch.B, self.n))
        d = LearnerBatch.model_desc(model)
        norm = {key: d.get(key) for key in ("xmean", "xstd", "ymean", "ystd")}
        for m in range(self.n):
            self.set_mlp(m, dict(batch.get_weights(m), **norm))

    def set_goals(self, goals):
        g = f32(goals).ravel()
        self._check(self.lib.mppi_batch_set_goals(self.h, fp(g), g.size))

    def next(self, X):
        """X [n, s_dim] -> u [n, a_dim] (synchronous)"""
        x = f32(X).ravel()
        u = np.zeros((self.n, self.a), np.float32)
        self._check(self.lib.mppi_batch_next(self.h, fp(x), x.size, fp(u), u.size))
        return u

    def next_device(self, x_ptr, u_ptr, stream=None):
        """x_ptr [n, s_dim] -> u_ptr [n, a_dim], device pointers; enqueue only (stream: Handle.next_device's convention)"""
        self._check(self.lib.mppi_batch_next_device(self.h, x_ptr, u_ptr, self._stream(stream)))

    def step_stats(self):
        """mppi_batch_step_stats: the StepStats of every member's last step, fields [n] (histograms [n, 32]); row m has the bits of the
        lone handle m's step_stats()"""
        return self._step_stats("mppi_batch_step_stats", (self.n,))

    def run_episode(self, X0, n_steps, goals=None, disturbance=None, *, plant=None, stats=False):
        """mppi_batch_run_episode: Handle.run_episode for every member at once. X0 [n, s]; goals / disturbance [n_steps, n, s]
        -> (X [n_steps+1, n, s], U [n_steps, n, a], C [n_steps, n]); member m's slices are its lone handle's episode.
        plant: a Handle every member's state is stepped with, or a sequence of n Handles, member m's at [m] (mppi_batch_run_episode_plant;
        a learned plant is shared: a sequence of n > 1 learned plants is refused).
        stats=True (mppi_batch_run_episode_stats): -> (X, U, C, StepStats) with fields [n_steps, n]."""
        return self._run_episode("mppi_batch_run_episode", (self.n,), X0, n_steps, goals, disturbance, plant, stats)

    def model_rollout(self, *args, **kwargs):
        """refused: the members of a batch share one model, so an open-loop rollout is a lone handle's business (Handle.model_rollout)"""
        raise MppiError(ERR_UNSUPPORTED, "BatchHandle.model_rollout: the members of a batch share one model; roll it on a lone Handle of "
                                         "the same model and cost (Handle.model_rollout)")

    def get_action_sequences(self):
        U = np.zeros((self.n, self.tau, self.a), np.float32)
        self._check(self.lib.mppi_batch_get_action_sequences(self.h, fp(U), U.size))
        return U

    def set_action_sequences(self, U):
        U = f32(U).ravel()
        self._check(self.lib.mppi_batch_set_action_sequences(self.h, fp(U), U.size))

    def debug_get(self, member, what):
        return self._debug_get(what, lambda *args: self.lib.mppi_batch_debug_get(self.h, int(member), *args))


def get_new(U, nb):
    lib = load()
    U = f32(U)
    tau, a = U.shape
    out = np.zeros((nb, a), np.float32)
    st = lib.mppi_get_new(fp(U), tau, a, nb, fp(out))
    if st != OK:
        raise MppiError(st, "mppi_get_new")
    return out


def shift(U, init, nb):
    lib = load()
    U = f32(U)
    tau, a = U.shape
    init = f32(init, (-1, a))
    out = np.zeros((tau - nb + init.shape[0], a), np.float32)
    st = lib.mppi_shift(fp(U), tau, a, fp(init), init.shape[0], nb, fp(out))
    if st != OK:
        raise MppiError(st, "mppi_shift")
    return out


class Learner:
    """RAII wrapper of one mppi_learner: full-batch Adam on the MSE of a small Dense network, on the GPU (mppi_learner.hip,
    mppi_learner_wide.hip). weights: dict(W=[...], b=[...]) (Keras [in x out] kernels); widths <= 32 and 1-4 layers, or exactly
    [in, 256, 256, out] with in, out <= 32 (the network of an MPPI_MODEL_MLP controller)."""

    def __init__(self, weights, device=0):
        lib = self.lib = load()
        self.Ws = [f32(w) for w in weights["W"]]
        self.bs = [f32(b).ravel() for b in weights["b"]]
        self.widths = [self.Ws[0].shape[0]] + [w.shape[1] for w in self.Ws]
        wd = (C.c_int32 * len(self.widths))(*self.widths)
        self.h = _H()
        st = lib.mppi_learner_create(len(self.Ws), wd, self._ptrs(self.Ws), self._ptrs(self.bs), device, C.byref(self.h))
        if st != OK:
            self.h = _H()
            raise MppiError(st, (lib.mppi_learner_last_error(None) or b"").decode())
        self.n = 0

    @staticmethod
    def _ptrs(arrs):
        return (FP * len(arrs))(*[fp(a) for a in arrs])

    def _check(self, st):
        if st != OK:
            raise MppiError(st, (self.lib.mppi_learner_last_error(self.h) or b"").decode())

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.mppi_learner_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, X, Y):
        X, Y = f32(X, (-1, self.widths[0])), f32(Y, (-1, self.widths[-1]))
        assert X.shape[0] == Y.shape[0]
        self.n = X.shape[0]
        self._check(self.lib.mppi_learner_set_data(self.h, fp(X), fp(Y), self.n))

    def train(self, steps, lr, beta1=0.9, beta2=0.999, eps=1e-7):
        """`steps` Adam steps (Keras defaults) -> (loss of the first step's forward pass, loss of the last step's)"""
        first, last = np.zeros(1, np.float32), np.zeros(1, np.float32)
        self._check(self.lib.mppi_learner_train(self.h, int(steps), lr, beta1, beta2, eps, fp(first), fp(last)))
        return float(first[0]), float(last[0])

    def evaluate(self, grads=False, pred=False):
        """loss of the current weights on the training set [, gradients as dict(W=[...], b=[...])] [, predictions]"""
        loss = np.zeros(1, np.float32)
        p = np.zeros((self.n, self.widths[-1]), np.float32) if pred else None
        if pred or not grads:
            self._check(self.lib.mppi_learner_evaluate(self.h, fp(loss), None, fp(p)))
        out = [float(loss[0])]
        if grads:  # mppi_learner_gradients: the compact layout of get_weights, for every learner
            gW, gb = [np.zeros_like(w) for w in self.Ws], [np.zeros_like(b) for b in self.bs]
            self._check(self.lib.mppi_learner_gradients(self.h, fp(loss), self._ptrs(gW), self._ptrs(gb)))
            out = [float(loss[0]), dict(W=gW, b=gb)]
        if pred:
            out.append(p)
        return out[0] if len(out) == 1 else tuple(out)

    def get_weights(self):
        Ws = [np.zeros_like(w) for w in self.Ws]
        bs = [np.zeros_like(b) for b in self.bs]
        self._check(self.lib.mppi_learner_get_weights(self.h, self._ptrs(Ws), self._ptrs(bs)))
        return dict(W=Ws, b=bs)

    def set_weights(self, weights):
        Ws, bs = [f32(w) for w in weights["W"]], [f32(b).ravel() for b in weights["b"]]
        self._check(self.lib.mppi_learner_set_weights(self.h, self._ptrs(Ws), self._ptrs(bs)))

    def reset_optimizer(self):
        self._check(self.lib.mppi_learner_reset_optimizer(self.h))

    # persistence (mppi_learner_save / _load / _peek): weights, both Adam moments, the step count and — the model's, handed through —
    # the normalisation, in the flat format include/mppi_c.h documents
    def save(self, filename, norm=None):
        """norm: dict(xmean, xstd, ymean, ystd) or None"""
        held = [None] * 4
        if norm is not None:
            n_in, n_out = self.widths[0], self.widths[-1]
            held = [np.ascontiguousarray(np.asarray(norm[k], np.float64).reshape(n)) for k, n in
                    (("xmean", n_in), ("xstd", n_in), ("ymean", n_out), ("ystd", n_out))]
        self._check(self.lib.mppi_learner_save(self.h, os.fsencode(filename), *[a.ctypes.data_as(DP) if a is not None else None for a in held]))

    def load(self, filename):
        """-> the file's normalisation dict(xmean, xstd, ymean, ystd), or None when it holds none"""
        n_in, n_out = self.widths[0], self.widths[-1]
        out = [np.zeros(n_in), np.zeros(n_in), np.zeros(n_out), np.zeros(n_out)]
        has = C.c_int(0)
        self._check(self.lib.mppi_learner_load(self.h, os.fsencode(filename), *[a.ctypes.data_as(DP) for a in out], C.byref(has)))
        return dict(zip(("xmean", "xstd", "ymean", "ystd"), out)) if has.value else None

    @classmethod
    def from_file(cls, filename, device=0):
        """a learner of the file's network with the file's weights, Adam moments and step count -> (learner, normalisation or None)"""
        lib = load()
        n, w = C.c_int(0), (C.c_int32 * 5)()
        st = lib.mppi_learner_peek(os.fsencode(filename), C.byref(n), w)
        if st != OK:
            raise MppiError(st, (lib.mppi_learner_last_error(None) or b"").decode())
        widths = [int(w[i]) for i in range(n.value + 1)]
        zero = dict(W=[np.zeros((widths[i], widths[i + 1]), np.float32) for i in range(n.value)],
                    b=[np.zeros(widths[i + 1], np.float32) for i in range(n.value)])
        lrn = cls(zero, device=device)
        return lrn, lrn.load(filename)

    def step_count(self):
        v = C.c_int(0)
        self._check(self.lib.mppi_learner_get_step(self.h, C.byref(v)))
        return int(v.value)


class _LearnerBatchBase:
    """What LearnerBatch and WideLearnerBatch share: the two objects' entry points are namesakes with one signature each, _PREFIX apart."""
    _PREFIX = None

    def _f(self, name):
        return getattr(self.lib, self._PREFIX + name)

    def __init__(self, weights, n_members, device=0):
        self.lib = load()
        self.Ws = [f32(w) for w in weights["W"]]
        self.bs = [f32(b).ravel() for b in weights["b"]]
        self.widths = [self.Ws[0].shape[0]] + [w.shape[1] for w in self.Ws]
        wd = (C.c_int32 * len(self.widths))(*self.widths)
        self.h = _H()
        st = self._f("create")(int(n_members), len(self.Ws), wd, Learner._ptrs(self.Ws), Learner._ptrs(self.bs), device, C.byref(self.h))
        if st != OK:
            self.h = _H()
            raise MppiError(st, (self._f("last_error")(None) or b"").decode())
        self.B = int(self._f("size")(self.h))
        self.n = 0

    def _check(self, st):
        if st != OK:
            raise MppiError(st, (self._f("last_error")(self.h) or b"").decode())

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self._f("destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, X, Y):
        """the pool every member draws its rows from; resets every split (train on all rows, no test rows)"""
        X, Y = f32(X, (-1, self.widths[0])), f32(Y, (-1, self.widths[-1]))
        assert X.shape[0] == Y.shape[0]
        self._check(self._f("set_data")(self.h, fp(X), fp(Y), X.shape[0]))
        self.n = X.shape[0]

    @staticmethod
    def _idx(idx):
        a = np.asarray([] if idx is None else idx)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise MppiError(ERR_INVALID_ARG, "row indices must be integers")
        a = a.astype(np.int64).ravel()
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise MppiError(ERR_INVALID_ARG, "row index outside int32")
        return np.ascontiguousarray(a, dtype=np.int32)

    def set_split(self, member, train_idx, test_idx=None):
        """member trains on pool rows train_idx (in that order, repeats allowed) and reports its held-out loss on test_idx"""
        tr, te = self._idx(train_idx), self._idx(test_idx)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else None
        self._check(self._f("set_split")(self.h, int(member), ip(tr), tr.size, ip(te), te.size))

    def set_weights(self, weights, member=-1):
        Ws, bs = [f32(w) for w in weights["W"]], [f32(b).ravel() for b in weights["b"]]
        if [w.shape for w in Ws] != [w.shape for w in self.Ws] or [b.shape for b in bs] != [b.shape for b in self.bs]:
            raise MppiError(ERR_INVALID_ARG, "weights of another shape than the batch's network")
        self._check(self._f("set_weights")(self.h, int(member), Learner._ptrs(Ws), Learner._ptrs(bs)))

    def get_weights(self, member):
        Ws, bs = [np.zeros_like(w) for w in self.Ws], [np.zeros_like(b) for b in self.bs]
        self._check(self._f("get_weights")(self.h, int(member), Learner._ptrs(Ws), Learner._ptrs(bs)))
        return dict(W=Ws, b=bs)

    def _per_member(self, v, name):
        if v is None:
            return None
        a = np.asarray(v, np.float32)
        if a.ndim == 0:
            return np.full(self.B, a, np.float32)
        if a.shape != (self.B,):
            raise MppiError(ERR_INVALID_ARG, "%s: a scalar or %d values, one per member (got shape %s)" % (name, self.B, a.shape))
        return np.ascontiguousarray(a)

    def train(self, steps, lr, beta1=None, beta2=None, eps=None):
        """`steps` Adam steps of every member; lr, beta1, beta2, eps: a scalar for all members or one value each (None: Keras' 0.9 /
        0.999 / 1e-7) -> (loss_train [steps, B]: each step's forward pass before its update, loss_test [steps, B]: the updated weights on
        the member's test rows, NaN where a member has none)"""
        steps = int(steps)
        hp = [self._per_member(v, k) for v, k in ((lr, "lr"), (beta1, "beta1"), (beta2, "beta2"), (eps, "eps"))]
        if hp[0] is None:
            raise MppiError(ERR_INVALID_ARG, "lr is required")
        tr, te = np.zeros((max(steps, 0), self.B), np.float32), np.zeros((max(steps, 0), self.B), np.float32)
        self._check(self._f("train")(self.h, steps, *[fp(a) for a in hp], fp(tr), fp(te)))
        return tr, te

    def evaluate(self):
        """(loss_train [B], loss_test [B]) of the current weights; no update"""
        tr, te = np.zeros(self.B, np.float32), np.zeros(self.B, np.float32)
        self._check(self._f("evaluate")(self.h, fp(tr), fp(te)))
        return tr, te

    def reset_optimizer(self):
        self._check(self._f("reset_optimizer")(self.h))

    def step_count(self):
        v = C.c_int(0)
        self._check(self._f("get_step")(self.h, C.byref(v)))
        return int(v.value)


    # ---- trajectory validation (mppi_learner_batch_rollout / mppi_learner_wide_batch_validate, include/mppi_c.h): one body, two entry points
    _KINDS = {"mlp": MODEL_MLP, "nnauv": MODEL_NN_AUV, "nnauv_speed": MODEL_NN_AUV_SPEED}

    @classmethod
    def model_desc(cls, model):
        """dict(kind, s_dim, a_dim[, dt, xmean, xstd, ymean, ystd]) of `model`: such a dict itself (kind: MPPI_MODEL_* or "mlp" / "nnauv" /
        "nnauv_speed"), or a model object — NNAUVModel, NNAUVModelSpeed, NNPointMassModel — from which these are read"""
        if isinstance(model, dict):
            d = dict(model)
        else:
            speed = hasattr(model, "to_euler")
            s, a = int(model.get_state_dim()), int(model.get_action_dim())
            kind = MODEL_NN_AUV_SPEED if speed else (MODEL_NN_AUV if s == 13 else MODEL_MLP)
            d = dict(kind=kind, s_dim=s, a_dim=a, dt=float(getattr(model, "_dt", 0.1)), **model.normalisation())
        d["kind"] = cls._KINDS.get(d["kind"], d["kind"])
        return d

    def _roll(self, entry, who, model, x0, V, gt, trajectories):
        """what LearnerBatch.rollout and WideLearnerBatch.validate do: the shape checks (ValueError), the call of `entry`, dict(sse[, X])"""
        d = self.model_desc(model)
        s, a = int(d["s_dim"]), int(d["a_dim"])
        V, x0 = np.asarray(V, dtype=np.float32), np.asarray(x0, dtype=np.float32)
        if V.ndim != 3 or V.shape[2] != a or V.shape[0] < 1 or V.shape[1] < 1:
            raise ValueError("V must have shape (T, n, %d) with T, n >= 1, not %s" % (a, V.shape))
        T, n = V.shape[0], V.shape[1]
        if x0.shape not in [(s,), (1, s), (n, s)]:
            raise ValueError("x0 must have shape (%d,), (1, %d) or (%d, %d), not %s" % (s, s, n, s, x0.shape))
        if gt is None and not trajectories:
            raise ValueError("%s: nothing to return without gt and without trajectories" % who)
        x0, V = np.ascontiguousarray(x0).reshape(-1, s), np.ascontiguousarray(V)
        G = None
        if gt is not None:
            G = np.ascontiguousarray(np.asarray(gt, dtype=np.float32))
            if G.shape != (T + 1, n, s):
                raise ValueError("gt must have shape (%d, %d, %d), not %s" % (T + 1, n, s, G.shape))
        held = {k: (f32(d[k]).ravel() if d.get(k) is not None else None) for k in ("xmean", "xstd", "ymean", "ystd")}
        for k, v in held.items():  # the library reads widths[0] / widths[-1] entries: the network's own widths, which it holds the kind to
            if v is not None and v.size != (self.widths[0] if k[0] == "x" else self.widths[-1]):
                raise ValueError("%s must have %d entries, not %d" % (k, self.widths[0] if k[0] == "x" else self.widths[-1], v.size))
        desc = LearnerModel(int(d["kind"]), s, a, float(d.get("dt") or 0.0), *[fp(held[k]) for k in ("xmean", "xstd", "ymean", "ystd")])
        sse = np.zeros((self.B, s), np.float64) if G is not None else None
        X = np.zeros((self.B, T + 1, n, s), np.float32) if trajectories else None
        self._check(entry(self.h, C.byref(desc), fp(x0), x0.shape[0], fp(V), fp(G), n, T, sse.ctypes.data_as(DP) if sse is not None else None, fp(X)))
        out = dict(sse=sse)
        if trajectories:
            out["X"] = X
        return out


class WideLearnerBatch(_LearnerBatchBase):
    """RAII wrapper of one mppi_learner_wide_batch: n_members learners of the [in, 256, 256, out] network (in, out <= 32) that share one
    data pool and step in the same launches (mppi_learner_wide_batch.hip). LearnerBatch's methods and meaning, member for member
    bit-identical to a lone wide Learner given the member's rows. LearnerBatch.rollout is `validate` here (mppi_learner_wide_batch_validate,
    an entry point of its own): the members of a [3a, 256, 256, 2a] batch rolled open-loop in one launch (mppi_learner_wide_rollout.hip)."""
    _PREFIX = "mppi_learner_wide_batch_"

    def validate(self, model, x0, V, gt=None, trajectories=False):
        """LearnerBatch.rollout for the wide members: every member's network rolled open-loop as the learned point-mass model `model`
        (model_desc; MPPI_MODEL_MLP with s = 2a, a <= 4, the batch's widths [3a, 256, 256, 2a]) along the action sequences V [T, n, a] from
        x0 [s] or [n, s], in ONE launch -> dict(sse [B, s] float64: the summed squared error against the ground truth gt [T+1, n, s], row 0
        included (None without gt); X [B, T+1, n, s] float32 with trajectories=True: member m's is bit for bit
        Handle(mlp=member m's weights).model_rollout(x0, V)). The batch itself does not change. Shapes are checked here: ValueError."""
        return self._roll(self.lib.mppi_learner_wide_batch_validate, "validate", model, x0, V, gt, trajectories)


class LearnerBatch(_LearnerBatchBase):
    """RAII wrapper of one mppi_learner_batch: n_members narrow learners (widths <= 32, 1-4 layers) that share one data pool and
    step in the same launches (mppi_learner_batch.hip). Every member starts from `weights`, trains on its own rows of the pool
    (set_split) with its own Adam rates, and is bit-identical to a lone Learner given those rows."""
    _PREFIX = "mppi_learner_batch_"

    def rollout(self, model, x0, V, gt=None, trajectories=False):
        """Every member's network rolled open-loop as the learned model `model` (model_desc) along the action sequences V [T, n, a] from
        x0 [s] or [n, s], in ONE launch -> dict(sse [B, s] float64: the summed squared error against the ground truth gt [T+1, n, s], row 0
        included (None without gt); X [B, T+1, n, s] float32 with trajectories=True: member m's is bit for bit
        Handle(member m's weights).model_rollout(x0, V)). The batch itself does not change. Shapes are checked here: ValueError."""
        return self._roll(self.lib.mppi_learner_batch_rollout, "rollout", model, x0, V, gt, trajectories)
