"""What the batched-controller GPU tests share (test_batch_gpu.py, test_batch_auv_gpu.py, test_batch_params_gpu.py): the point-mass plant,
the members' states / goals / sequences, the rexrov2 task, raw mppi_config batches, the lone handles a batch is compared with and that
comparison. A plain module: `m` is the mppi_tf_amd package each test file's fixture gives."""
import ctypes as C

import numpy as np

F32 = np.float32
Q10 = np.diag([100.0] * 3 + [10.0] + [1.0] * 6) + 0.01
E3 = dict(normal=[0.0, np.sin(0.3), np.cos(0.3)], aVec=[1.0, 0.0, 0.0], axis=[2.0, 1.5], speed=1.0, m_state=50.0, m_vel=5.0)
AUV_PC = "mppi::k_rollout_auv_pc<"


def plant(x, u, a, dt=0.1):
    x = x.copy()
    for j in range(a):
        x[2 * j] = x[2 * j] + F32(dt) * x[2 * j + 1] + F32(dt * dt / 2) * u[j]
        x[2 * j + 1] = x[2 * j + 1] + F32(dt) * u[j]
    return x


def pm_members(B, a, H, seed=0):
    """distinct x, goal and initial U per member of a point-mass batch"""
    rng = np.random.default_rng(100 + seed)
    s = 2 * a
    X = rng.uniform(-1, 1, (B, s)).astype(F32)
    G = np.zeros((B, s), F32)
    G[:, 0::2] = rng.uniform(-1, 1, (B, a))
    U0 = rng.uniform(-0.2, 0.2, (B, H, a)).astype(F32)
    return X, G, U0


def auv_members(B, H, seed=0):
    """distinct x (unit quaternions), goals and initial sequences per member of an AUV batch"""
    rng = np.random.default_rng(200 + seed)
    X = np.zeros((B, 13), F32)
    X[:, :3] = rng.uniform(-1, 1, (B, 3))
    q = rng.standard_normal((B, 4))
    X[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    X[:, 7:] = rng.uniform(-0.3, 0.3, (B, 6))
    G = np.zeros((B, 13), F32)
    G[:, :3] = rng.uniform(-3, 3, (B, 3))
    qg = rng.standard_normal((B, 4))
    G[:, 3:7] = qg / np.linalg.norm(qg, axis=1, keepdims=True)
    U0 = (50.0 * rng.standard_normal((B, H, 6))).astype(F32)
    return X, G, U0


def rexrov2(rk=2):
    from mppi_tf_amd.auv import auv_task
    return dict(auv_task(8)["auv"], rk=rk)


# ---- raw mppi_configs ----------------------------------------------------------------------------------------------------------------
def raw_configs(n, s_dim=4, a_dim=2, k=256, tau=16, each=None, **fields):
    """n raw mppi_configs (point mass a = 2 unless `fields` say otherwise); each(m, cfg, keep) edits member m -> (array, keep)"""
    from mppi_tf_amd import _lib
    lib = _lib.load()
    arr, keep = (_lib.Config * n)(), []
    for i in range(n):
        assert lib.mppi_config_init(C.byref(arr[i]), k, tau, 0.1, 1.0, s_dim, a_dim) == 0
        for key, v in fields.items():
            setattr(arr[i], key, v)
        if each:
            each(i, arr[i], keep)
    return arr, keep


def ptr(keep, a):
    from mppi_tf_amd import _lib
    keep.append(np.ascontiguousarray(a, F32).ravel())
    return keep[-1].ctypes.data_as(_lib.FP)


def create_batch_configs(arr, n=None):
    """mppi_create_batch_configs on raw configs -> (status, the creation error, whether a handle came back); the handle is destroyed"""
    from mppi_tf_amd import _lib
    lib = _lib.load()
    h = _lib._H()
    st = lib.mppi_create_batch_configs(arr, len(arr) if n is None else n, C.byref(h))
    if h:
        lib.mppi_destroy(h)
    return st, lib.mppi_last_error(None).decode(), bool(h)


def create_batch(n=2, s_dim=4, a_dim=2, **fields):
    """mppi_create_batch on a raw mppi_config (K = 256, tau = 16, point mass a = 2 unless told otherwise) -> (status, handle)"""
    from mppi_tf_amd import _lib
    arr, _ = raw_configs(1, s_dim, a_dim, **fields)
    h = _lib._H()
    return _lib.load().mppi_create_batch(C.byref(arr[0]), n, None, C.byref(h)), h


def batch_of(m, each):
    """a batch of two from one raw 13-state config that each(cfg, keep) filled; raises MppiError with the creation error"""
    from mppi_tf_amd import _lib
    lib = _lib.load()
    arr, keep = raw_configs(1, 13, 6, each=lambda i, cfg, kp: each(cfg, kp))
    h = _lib._H()
    st = lib.mppi_create_batch(C.byref(arr[0]), 2, None, C.byref(h))
    if st != _lib.OK:
        raise m.MppiError(st, lib.mppi_last_error(None).decode())
    lib.mppi_destroy(h)


def batch_with_mlp(m, kw):
    """a batch of a learned 13-state model through the Python binding's config path (Handle's keywords on a raw mppi_create_batch)"""
    from mppi_tf_amd import _lib
    name, mlp = next(iter(kw.items()))
    speed = name == "nnauv_speed"

    def each(cfg, keep):
        desc, held = _lib._mlp_desc(mlp, 15 if speed else 16, 6 if speed else 13)
        keep += held
        cfg.model_kind, cfg.mlp = (_lib.MODEL_NN_AUV_SPEED if speed else _lib.MODEL_NN_AUV), C.pointer(desc)
    batch_of(m, each)


def batch_with(m, **fields):
    """an AUV batch (rexrov2) with raw config fields set on top"""
    from mppi_tf_amd import _lib

    def each(cfg, keep):
        _lib._fill_13state(cfg, keep, rexrov2(), False, None, None)
        for k, v in fields.items():
            setattr(cfg, k, v)
    batch_of(m, each)


# ---- a batch against its members' lone handles ------------------------------------------------------------------------------------------
def lone_handles(m, kws, seeds, G, U0, prefix):
    """member i's lone Handle(seed=seeds[i], goal=G[i], **kws[i]) on the sequence U0[i]; its rollout kernel's name starts with `prefix`"""
    hs = []
    for i, kw in enumerate(kws):
        h = m.Handle(seed=seeds[i], **dict(kw, goal=G[i]))
        assert h.rollout_kernel_name().startswith(prefix), h.rollout_kernel_name()
        h.set_action_sequence(U0[i])
        hs.append(h)
    return hs


def lone(m, c, seeds, G, U0, lim=None):
    """the lone AUV handles of a batch whose members share the keywords c"""
    hs = lone_handles(m, [c] * len(seeds), seeds, G, U0, AUV_PC)
    for h in hs:
        if lim:
            h.set_action_limits(*lim)
    return hs


def make(m, shared, per, lone_kw, seeds, G, U0, lone_prefix):
    hb = m.BatchHandle(n=len(seeds), seeds=seeds, goals=G, **shared, **per)
    hb.set_action_sequences(U0)
    return hb, lone_handles(m, lone_kw, seeds, G, U0, lone_prefix)


def assert_members_equal(m, hb, hs, ub, us, tag):
    Ub = hb.get_action_sequences()
    for i, h in enumerate(hs):
        msg = "member %d %s" % (i, tag)
        np.testing.assert_array_equal(hb.debug_get(i, m.DBG_COSTS), h.debug_get(m.DBG_COSTS), err_msg=msg)
        np.testing.assert_array_equal(hb.debug_get(i, m.DBG_BETA), h.debug_get(m.DBG_BETA), err_msg=msg)
        np.testing.assert_array_equal(hb.debug_get(i, m.DBG_ETA), h.debug_get(m.DBG_ETA), err_msg=msg)
        np.testing.assert_array_equal(ub[i], us[i], err_msg=msg)
        np.testing.assert_array_equal(Ub[i], h.get_action_sequence(), err_msg=msg)


def close(hb, hs):
    for h in hs:
        h.close()
    hb.close()
