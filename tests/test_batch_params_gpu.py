"""Batched controllers with per-member lambda, gamma, upsilon, Sigma and Q (mppi_create_batch_configs / BatchHandle(lams=, gammas=,
upsilons=, sigmas=, Qs=)). Needs an MI355X: every test is marked `gpu`.

The contract (include/mppi_c.h): member m of the batch made from cfgs[0..n) is BIT-IDENTICAL to the lone handle mppi_create(&cfgs[m]) on
its default path, fed the same x and sequence on the same step counter: sample costs, beta, eta, U' and u.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from batch_util import (E3, Q10, assert_members_equal, auv_members, close, create_batch_configs as _create, make, plant, pm_members, ptr as _ptr,
                        raw_configs as _cfgs)

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def spd(rng, n, scale, off):
    """a symmetric matrix scale * I + a symmetric perturbation of size `off` (non-zero off-diagonal entries)"""
    S = rng.uniform(-off, off, (n, n))
    return (scale * np.eye(n) + (S + S.T) / 2).astype(F32)


def pm_sweep(B, K, H, a, dense_sigma=False, dense_q=False, py=False, scales=False, seed=0):
    """-> (shared keywords, per-member keywords of BatchHandle, the Handle keywords of each member): lambda log-spaced over two decades,
    each member's own Sigma and Q, with the Python action-cost form each member's own gamma and upsilon"""
    rng = np.random.default_rng(300 + seed)
    s = 2 * a
    shared = dict(k=K, tau=H, s_dim=s, a_dim=a, dt=0.1, mass=1.0, goal=rng.uniform(-1, 1, s).astype(F32))
    if py:
        shared.update(action_cost=1, upsilon_scales_noise=scales)
    per = dict(lams=list(np.logspace(-1, 1, B)))
    if dense_sigma:
        per["sigmas"] = [spd(rng, a, rng.uniform(0.15, 0.5), 0.06) for _ in range(B)]
    else:
        per["sigmas"] = [np.diag(rng.uniform(0.1, 0.6, a)).astype(F32) for _ in range(B)]
    if dense_q:
        per["Qs"] = [(lambda L: (L @ L.T).astype(F32))(rng.uniform(-0.3, 0.3, (s, s)) + np.eye(s) * rng.uniform(0.7, 1.5)) for _ in range(B)]
    else:
        per["Qs"] = [rng.uniform(0.3, 3.0, s).astype(F32) for _ in range(B)]
    if py:
        per["gammas"] = list(rng.uniform(0.05, 0.9, B))
        per["upsilons"] = list(rng.uniform(1.0, 3.0, B))
    names = dict(lams="lam", gammas="gamma", upsilons="upsilon", sigmas="sigma", Qs="Q")
    lone = [dict(shared, **{names[k]: v[i] for k, v in per.items()}) for i in range(B)]
    return shared, per, lone


def auv_sweep(B, K, H, cost, rk, seed=0):
    from mppi_tf_amd.auv import auv_task
    rng = np.random.default_rng(400 + seed)
    t = auv_task(H)
    shared = dict(k=K, tau=H, s_dim=13, a_dim=6, dt=0.1, auv=dict(t["auv"], rk=rk))
    per = dict(lams=list(np.logspace(-1, 1, B)), sigmas=[(f * t["sigma"]).astype(F32) for f in np.linspace(0.5, 2.0, B)])
    if cost == "quadratic":
        per["Qs"] = [(t["Q"] * rng.uniform(0.5, 2.0, 13)).astype(F32) for _ in range(B)]
    elif cost == "dense":
        per["Qs"] = [(np.diag(t["Q"] * rng.uniform(0.5, 2.0, 13)) + rng.uniform(0.01, 0.1)).astype(F32) for _ in range(B)]
    elif cost == "quat":
        shared.update(Q=Q10, quat_cost=True)
    else:
        shared.update(ellipse3d=E3)
    names = dict(lams="lam", sigmas="sigma", Qs="Q")
    lone = [dict(shared, **{names[k]: v[i] for k, v in per.items()}) for i in range(B)]
    return shared, per, lone


# (B, K, H, a, dense_sigma, dense_q, py, upsilon_scales_noise, the lone handle's kernel)
PM = [(4, 4096, 64, 2, False, False, False, False, "mppi::k_step_pc<"),      # the lone handle runs its fused step
      (5, 3000, 50, 3, False, True, True, True, "mppi::k_rollout_pc<"),      # ragged K; dense Q; gamma / upsilon scaling the noise
      (2, 65536, 64, 3, True, False, True, False, "mppi::k_rollout_pc<3, 3"),  # the NP = 3 instance; dense Sigma
      (3, 128, 32, 1, False, True, False, False, "mppi::k_")]


@pytest.mark.parametrize("B,K,H,a,dense_sigma,dense_q,py,scales,kern", PM)
def test_point_mass_sweep_equals_lone_handles(m, B, K, H, a, dense_sigma, dense_q, py, scales, kern):
    """Every member, every step: costs, beta, eta, U' and u are the bits of Handle(**cfg_m) on its default path."""
    shared, per, lone_kw = pm_sweep(B, K, H, a, dense_sigma, dense_q, py, scales)
    X, G, U0 = pm_members(B, a, H)
    seeds = [11 + 7 * i for i in range(B)]
    hb, hs = make(m, shared, per, lone_kw, seeds, G, U0, kern)
    assert "k_rollout_pc_batch<%d, %d" % (a, 3 if K > 512 * 64 else 5) in hb.rollout_kernel_name()
    assert ("true" if not dense_sigma else "false") in hb.rollout_kernel_name()
    for step in range(3):
        ub = hb.next(X)
        us = [h.next(X[i]) for i, h in enumerate(hs)]
        assert_members_equal(m, hb, hs, ub, us, "step %d" % step)
        X = np.stack([plant(X[i], ub[i], a) for i in range(B)])
    close(hb, hs)


AUV = [(3, 1000, 16, "quadratic", 1), (3, 2048, 20, "dense", 2), (2, 1000, 12, "quat", 2), (2, 1000, 12, "ellipse3d", 1)]


@pytest.mark.parametrize("B,K,H,cost,rk", AUV)
def test_auv_sweep_equals_lone_handles(m, B, K, H, cost, rk):
    """The Fossen AUV model with per-member lambda and Sigma (and Q of the quadratic cost): every member is its lone k_rollout_auv_pc."""
    shared, per, lone_kw = auv_sweep(B, K, H, cost, rk)
    X, G, U0 = auv_members(B, H)
    seeds = [5 + 13 * i for i in range(B)]
    hb, hs = make(m, shared, per, lone_kw, seeds, G, U0, "mppi::k_rollout_auv_pc<")
    assert hb.rollout_kernel_name() == "mppi::k_rollout_auv_pc_batch<true>"
    for step in range(3):
        ub = hb.next(X)
        us = [h.next(X[i]) for i, h in enumerate(hs)]
        assert_members_equal(m, hb, hs, ub, us, "step %d" % step)
        X = hs[0].model_next(X, ub)
    close(hb, hs)


@pytest.mark.parametrize("model", ["pm", "auv"])
def test_members_are_independent_of_each_others_parameters(m, model):
    """Two batches that differ only in member j's lambda and Sigma: member j differs, every other member is bit-identical."""
    B, j = 4, 1
    if model == "pm":
        shared, per, _ = pm_sweep(B, 4096, 64, 2)
        X, G, U0 = pm_members(B, 2, 64, seed=2)
    else:
        shared, per, _ = auv_sweep(B, 2048, 16, "quadratic", 2)
        X, G, U0 = auv_members(B, 16, seed=2)
    per2 = {k: list(v) for k, v in per.items()}
    per2["lams"][j] = per["lams"][j] * 7.0
    per2["sigmas"][j] = per["sigmas"][j] * 1.5
    h1 = m.BatchHandle(n=B, goals=G, **shared, **per)
    h2 = m.BatchHandle(n=B, goals=G, **shared, **per2)
    for h in (h1, h2):
        h.set_action_sequences(U0)
    others = [i for i in range(B) if i != j]
    for _ in range(3):
        u1, u2 = h1.next(X), h2.next(X)
        assert not np.array_equal(u1[j], u2[j])
        assert not np.array_equal(h1.debug_get(j, m.DBG_COSTS), h2.debug_get(j, m.DBG_COSTS))
        np.testing.assert_array_equal(u1[others], u2[others])
        np.testing.assert_array_equal(h1.get_action_sequences()[others], h2.get_action_sequences()[others])
        for i in others:
            np.testing.assert_array_equal(h1.debug_get(i, m.DBG_COSTS), h2.debug_get(i, m.DBG_COSTS))
    h1.close(); h2.close()


@pytest.mark.parametrize("model", ["pm", "auv"])
def test_equal_configs_equal_the_uniform_batch(m, model):
    """mppi_create_batch_configs with n equal configs (seeds aside) is mppi_create_batch, bit for bit."""
    if model == "pm":
        B, H, a = 5, 50, 3
        c = dict(k=3000, tau=H, s_dim=6, a_dim=a, dt=0.1, lam=0.7, sigma=np.diag([0.2, 0.3, 0.25]), Q=np.arange(1, 7, dtype=F32),
                 action_cost=1, gamma=0.3, upsilon=2.0)
        X, G, U0 = pm_members(B, a, H, seed=4)
    else:
        from mppi_tf_amd.auv import auv_task
        B, H, a = 3, 16, 6
        t = auv_task(H)
        c = dict(k=2048, tau=H, s_dim=13, a_dim=6, dt=0.1, lam=0.5, sigma=t["sigma"], Q=t["Q"], auv=t["auv"])
        X, G, U0 = auv_members(B, H, seed=4)
    seeds = [3 + 2 * i for i in range(B)]
    hu = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hc = m.BatchHandle(n=B, seeds=seeds, goals=G, lams=[c["lam"]] * B, **c)  # the per-member path, every member alike
    for h in (hu, hc):
        h.set_action_sequences(U0)
    for _ in range(3):
        uu, uc = hu.next(X), hc.next(X)
        np.testing.assert_array_equal(uu, uc)
        np.testing.assert_array_equal(hu.get_action_sequences(), hc.get_action_sequences())
        for i in range(B):
            np.testing.assert_array_equal(hu.debug_get(i, m.DBG_COSTS), hc.debug_get(i, m.DBG_COSTS))
        X = np.stack([plant(X[i], uu[i], a) for i in range(B)]) if model == "pm" else X
    assert hu.rollout_kernel_name() == hc.rollout_kernel_name()
    hu.close(); hc.close()


@pytest.mark.parametrize("model", ["pm", "auv"])
def test_debug_items_are_the_members_own(m, model):
    """DBG_WEIGHTS (at the member's lambda), DBG_NOISE (its key and Sigma), DBG_BETA and DBG_ETA equal the lone handle's."""
    if model == "pm":
        B, H = 3, 32
        shared, per, lone_kw = pm_sweep(B, 2000, H, 2, py=True, scales=True, seed=5)
        X, G, U0 = pm_members(B, 2, H, seed=5)
        kern = "mppi::k_"
    else:
        B, H = 2, 12
        shared, per, lone_kw = auv_sweep(B, 1000, H, "quadratic", 2, seed=5)
        X, G, U0 = auv_members(B, H, seed=5)
        kern = "mppi::k_rollout_auv_pc<"
    seeds = [21 + i for i in range(B)]
    hb, hs = make(m, shared, per, lone_kw, seeds, G, U0, kern)
    for step in range(2):
        ub = hb.next(X)
        for i, h in enumerate(hs):
            h.next(X[i])
            for what in (m.DBG_WEIGHTS, m.DBG_NOISE, m.DBG_BETA, m.DBG_ETA):
                np.testing.assert_array_equal(hb.debug_get(i, what), h.debug_get(what), err_msg="member %d step %d item %d" % (i, step, what))
        # the members' weights and noise really differ (lambda, Sigma, key)
        assert not np.array_equal(hb.debug_get(0, m.DBG_NOISE), hb.debug_get(1, m.DBG_NOISE))
        X = np.stack([plant(X[i], ub[i], 2) for i in range(B)]) if model == "pm" else hs[0].model_next(X, ub)
    close(hb, hs)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(m):
    from mppi_tf_amd import _lib
    lib = _lib.load()
    UNSUP, INVAL, SING = _lib.ERR_UNSUPPORTED, _lib.ERR_INVALID_ARG, _lib.ERR_SINGULAR_SIGMA
    # a batch that is valid: the baseline every case below breaks in one field of one member
    arr, keep = _cfgs(3, each=lambda i, c, kp: setattr(c, "lam", 0.1 * 10 ** i))
    assert _create(arr)[0] == 0
    # every shared field: INVALID_ARG naming the field and the first member that differs
    for field, val in [("k", 512), ("tau", 8), ("dt", 0.05), ("mass", 2.0), ("device", 1), ("action_cost_kind", 1), ("flags", 1),
                       ("q_is_full", 1), ("normalize_cost", 1), ("shard_rank", 1), ("shard_count", 2), ("model_kind", _lib.MODEL_MLP),
                       ("state_cost_kind", _lib.STATE_COST_ELLIPSE), ("s_dim", 6), ("a_dim", 3)]:
        arr, keep = _cfgs(3, each=lambda i, c, kp, f=field, v=val: setattr(c, f, v) if i == 2 else None)
        st, msg, ok = _create(arr)
        assert st == INVAL and not ok, (field, st, msg)
        assert "cfgs[2].%s" % field in msg, (field, msg)
    # the 13-state model and costs: the contents of auv, quat_Q and ellipse3d are shared
    from mppi_tf_amd.auv import auv_task
    par = auv_task(8)["auv"]

    def auv(i, c, kp, mass=None, q=None, e3=None):
        _lib._fill_13state(c, kp, dict(par, mass=par["mass"] + (1.0 if mass and i == 1 else 0.0)), q is not None,
                           None if e3 is None else dict(E3, speed=E3["speed"] + (0.5 if e3 and i == 1 else 0.0)),
                           None if q is None else Q10 + (1.0 if q and i == 1 else 0.0))
        c.sigma = _ptr(kp, 1500.0 * np.eye(6))
    for kw, field in [(dict(mass=True), "auv"), (dict(q=True), "quat_Q"), (dict(e3=True), "ellipse3d")]:
        arr, keep = _cfgs(2, 13, 6, each=lambda i, c, kp, kw=kw: auv(i, c, kp, **kw))
        st, msg, _ = _create(arr)
        assert st == INVAL and "cfgs[1].%s" % field in msg, (field, msg)
    for kw in (dict(mass=False), dict(q=False), dict(e3=False)):  # the same contents through different pointers: accepted
        arr, keep = _cfgs(2, 13, 6, each=lambda i, c, kp, kw=kw: auv(i, c, kp, **kw))
        assert _create(arr)[0] == 0, kw
    # one kernel instance for every member: Sigma all diagonal or all dense, Q all diagonal or all dense
    arr, keep = _cfgs(3, each=lambda i, c, kp: setattr(c, "sigma", _ptr(kp, [[0.3, 0.05 * (i == 1)], [0.05 * (i == 1), 0.3]])))
    st, msg, _ = _create(arr)
    assert st == UNSUP and "sigma" in msg and "member 1" in msg, msg

    def dense_q(off_member):
        def f(i, c, kp):
            Q = np.eye(4) * 2.0
            if i == off_member:
                Q[0, 1] = Q[1, 0] = 0.3
            c.Q, c.q_is_full = _ptr(kp, Q), 1
        return f
    st, msg, _ = _create(_cfgs(3, each=dense_q(2))[0])
    assert st == UNSUP and "Q" in msg and "member 2" in msg, msg
    assert _create(_cfgs(3, each=dense_q(-1))[0])[0] == 0  # dense Q without off-diagonal entries everywhere: diagonal for all
    # a singular Sigma names the member (member 0 too)
    for j in (0, 2):
        arr, keep = _cfgs(3, each=lambda i, c, kp, j=j: setattr(c, "sigma", _ptr(kp, np.zeros((2, 2)) if i == j else np.eye(2))))
        st, msg, _ = _create(arr)
        assert st == SING and "member %d" % j in msg, (j, msg)
    arr, keep = _cfgs(3, each=lambda i, c, kp: setattr(c, "lam", -1.0 if i == 1 else 1.0))
    st, msg, _ = _create(arr)
    assert st == INVAL and "member 1" in msg and "lambda" in msg, msg
    # n < 1, NULL
    arr, keep = _cfgs(2)
    assert _create(arr, n=0)[0] == INVAL
    h = _lib._H()
    assert lib.mppi_create_batch_configs(None, 2, C.byref(h)) == INVAL and not h
    assert lib.mppi_create_batch_configs(arr, 2, None) == INVAL
    # what mppi_create_batch refuses is refused here, with the same message
    for fields in [dict(model_kind=_lib.MODEL_MLP), dict(model_kind=_lib.MODEL_AUV, s_dim=13, a_dim=6),
                   dict(model_kind=_lib.MODEL_NN_AUV, s_dim=13, a_dim=6), dict(state_cost_kind=_lib.STATE_COST_ELLIPSE),
                   dict(state_cost_kind=_lib.STATE_COST_QUAT, s_dim=13, a_dim=6), dict(normalize_cost=1), dict(flags=4), dict(flags=2),
                   dict(shard_count=2), dict(tau=200)]:
        arr, keep = _cfgs(2, **fields)
        hh = _lib._H()
        st0 = lib.mppi_create_batch(C.byref(arr[0]), 2, None, C.byref(hh))
        msg0 = lib.mppi_last_error(None).decode()
        st, msg, ok = _create(arr)
        assert st0 != 0 and st == st0 and msg == msg0 and not ok, (fields, st0, st, msg0, msg)
    # BatchHandle: a per-member list of the wrong length
    for kw in (dict(lams=[1.0, 2.0]), dict(sigmas=[np.eye(2)] * 4), dict(Qs=[np.ones(4)]), dict(gammas=[0.5] * 2), dict(upsilons=[1.0] * 5)):
        with pytest.raises(m.MppiError) as e:
            m.BatchHandle(n=3, k=256, tau=16, s_dim=4, a_dim=2, **kw)
        assert e.value.status == INVAL, kw


def test_singular_member_after_member_zero_then_repaired(m):
    """K = 256, H = 16, a = 2, n = 3 through mppi_create_batch_configs. Member 2's singular Sigma is found after member 0 passed every
    check, where the batch's one allocation follows: MPPI_ERR_SINGULAR_SIGMA naming member 2, no handle. The same configs with that Sigma
    repaired create, step once and equal the three lone handles mppi_create(&cfgs[i]) bit for bit (u, U', costs, beta, eta)."""
    from mppi_tf_amd import _lib
    lib = _lib.load()
    n, K, H, a = 3, 256, 16, 2
    sig = [np.diag([0.2, 0.3]), np.diag([0.4, 0.25]), np.diag([0.15, 0.5])]

    def each(bad):
        def f(i, c, kp):
            c.sigma, c.lam, c.seed = _ptr(kp, np.zeros((a, a)) if (bad and i == 2) else sig[i]), 0.5 * (i + 1), 31 + i
        return f
    arr, keep = _cfgs(n, 2 * a, a, K, H, each=each(True))
    hb = _lib._H()
    st = lib.mppi_create_batch_configs(arr, n, C.byref(hb))
    msg = lib.mppi_last_error(None).decode()
    assert st == _lib.ERR_SINGULAR_SIGMA and "member 2" in msg and "sigma is singular" in msg and not hb, (st, msg)
    arr, keep = _cfgs(n, 2 * a, a, K, H, each=each(False))
    assert lib.mppi_create_batch_configs(arr, n, C.byref(hb)) == 0 and hb, lib.mppi_last_error(None)
    assert lib.mppi_batch_size(hb) == n
    X = np.random.default_rng(12).uniform(-1, 1, (n, 2 * a)).astype(F32)
    fp = lambda x: x.ctypes.data_as(_lib.FP)
    ub, Ub = np.zeros((n, a), F32), np.zeros((n, H, a), F32)
    assert lib.mppi_batch_next(hb, fp(X), X.size, fp(ub), ub.size) == 0, lib.mppi_last_error(hb)
    assert lib.mppi_batch_get_action_sequences(hb, fp(Ub), Ub.size) == 0
    for i in range(n):
        h = _lib._H()
        assert lib.mppi_create(C.byref(arr[i]), C.byref(h)) == 0, lib.mppi_last_error(None)
        u, U = np.zeros(a, F32), np.zeros((H, a), F32)
        assert lib.mppi_next(h, fp(X[i]), 2 * a, fp(u), a) == 0 and lib.mppi_get_action_sequence(h, fp(U), U.size) == 0
        np.testing.assert_array_equal(ub[i], u, err_msg="member %d" % i)
        np.testing.assert_array_equal(Ub[i], U, err_msg="member %d" % i)
        for what, size in ((m.DBG_COSTS, K), (m.DBG_BETA, 1), (m.DBG_ETA, 1)):
            cb, cl = np.zeros(size, F32), np.zeros(size, F32)
            assert lib.mppi_batch_debug_get(hb, i, what, fp(cb), size) == 0 and lib.mppi_debug_get(h, what, fp(cl), size) == 0
            np.testing.assert_array_equal(cb, cl, err_msg="member %d item %d" % (i, what))
        lib.mppi_destroy(h)
    assert len({tuple(r) for r in ub}) == n  # the members' controls differ
    lib.mppi_destroy(hb)


# ---- device path, closed loop, the example ------------------------------------------------------------------------------------------
def test_device_path_and_closed_loop(m):
    """next_device on torch tensors = next; then 30 closed-loop steps of a lambda / Sigma sweep on the point-mass plant, every member's
    trajectory the bits of its lone handle's."""
    import torch
    B, K, H, a = 4, 2048, 40, 2
    shared, per, lone_kw = pm_sweep(B, K, H, a, seed=7)
    X, G, U0 = pm_members(B, a, H, seed=7)
    hd = m.BatchHandle(n=B, goals=G, **shared, **per)
    hh = m.BatchHandle(n=B, goals=G, **shared, **per)
    for h in (hd, hh):
        h.set_action_sequences(U0)
    x = torch.from_numpy(X).cuda()
    u = torch.zeros((B, a), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    for _ in range(10):
        hd.next_device(x.data_ptr(), u.data_ptr(), st)
    for _ in range(10):
        uh = hh.next(X)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u.cpu().numpy(), uh)
    np.testing.assert_array_equal(hd.get_action_sequences(), hh.get_action_sequences())
    hd.close(); hh.close()
    hb = m.BatchHandle(n=B, goals=G, seeds=[1 + i for i in range(B)], **shared, **per)
    hs = [m.Handle(seed=1 + i, **dict(kw, goal=G[i])) for i, kw in enumerate(lone_kw)]
    Xb, Xs = X.copy(), X.copy()
    for _ in range(30):
        ub = hb.next(Xb)
        us = np.stack([h.next(Xs[i]) for i, h in enumerate(hs)])
        np.testing.assert_array_equal(ub, us)
        Xb = np.stack([plant(Xb[i], ub[i], a) for i in range(B)])
        Xs = np.stack([plant(Xs[i], us[i], a) for i in range(B)])
    np.testing.assert_array_equal(Xb, Xs)
    assert len({tuple(r) for r in Xb}) == B  # the members went their own ways
    close(hb, hs)


def test_sweep_example_runs(m):
    """examples/sweep.py at a 2 x 2 x 1 x 2 grid for 5 steps: 8 grid points, a finite distance each."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "sweep.py"), "--lams", "0.05", "0.2", "--upsilons", "1", "2", "--gammas", "0.1",
           "--noises", "0.1", "0.2", "-s", "5", "--samples", "4096"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()[1:] if ln.strip() and ln.split()[0][0].isdigit() and len(ln.split()) == 5]
    assert len(rows) == 8, r.stdout
    assert all(np.isfinite(float(row[4])) for row in rows), r.stdout
    assert "8 grid points, 5 steps in one batch" in r.stdout, r.stdout
