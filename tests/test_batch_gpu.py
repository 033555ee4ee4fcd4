"""Batched controllers (mppi_create_batch / BatchHandle): B independent MPPI problems stepped in the same two launches as one. Needs an
MI355X: every test is marked `gpu`.

The contract (include/mppi_c.h): member m is BIT-IDENTICAL to a lone Handle made from the same configuration with seed = seeds[m], fed the
same x, goal and action sequence on the same step counter — sample costs, U' and u; members never interact. Through that, every member
inherits the lone handle's parity with the oracle; a direct oracle check is here as well.
"""
import ctypes as C

import numpy as np
import pytest

from batch_util import create_batch, plant, pm_members as members
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32
U_TOL = 1e-5


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def common(K, H, a, dense=False):
    s = 2 * a
    d = dict(k=K, tau=H, s_dim=s, a_dim=a, dt=0.1, mass=1.0, lam=1.0, sigma=np.eye(a) * 0.25, Q=np.ones(s))
    if dense:
        rng = np.random.default_rng(7)
        L = rng.uniform(-0.3, 0.3, (s, s)) + np.eye(s)
        d["Q"] = (L @ L.T).astype(F32)  # symmetric positive definite, off-diagonal entries non-zero: the dense-Q instance
        S = rng.uniform(-0.05, 0.05, (a, a))
        d["sigma"] = (0.25 * np.eye(a) + (S + S.T) / 2).astype(F32)
    return d


EQUIV = [(4, 4096, 64, 2, False), (5, 3000, 50, 2, False), (3, 1000, 20, 1, False), (16, 4096, 64, 3, False), (2, 65536, 64, 3, False),
         (1, 512, 32, 4, False), (3, 4096, 64, 2, True)]


@pytest.mark.parametrize("B,K,H,a,dense", EQUIV)
def test_batch_equals_standalone_handles(m, B, K, H, a, dense):
    """Every member, every step: u, the member's sequence and its sample costs are the bits of Handle(seed=seeds[m]) on its default
    (fused where it applies) path and on the two-launch path."""
    c = common(K, H, a, dense)
    X, G, U0 = members(B, a, H)
    seeds = [11 + 7 * i for i in range(B)]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    assert hb.lib.mppi_batch_size(hb.h) == B and "k_rollout_pc_batch" in hb.rollout_kernel_name()
    hb.set_action_sequences(U0)
    lone = []
    for i in range(B):
        pair = (m.Handle(seed=seeds[i], goal=G[i], **c), m.Handle(seed=seeds[i], goal=G[i], tuning={"fused_step": 0}, **c))
        for h in pair:
            h.set_action_sequence(U0[i])
        lone.append(pair)
    # the batch runs the instance each member's lone handle runs on its two-launch path (k_rollout_pc<.., PASS = 0>), spelled in full
    assert hb.rollout_kernel_name() == lone[0][1].rollout_kernel_name().replace("k_rollout_pc<", "k_rollout_pc_batch<")[:-len(", 0>")] + ">"
    if dense:
        lim = ([-0.3, -0.25][:a], [0.2, 0.35][:a])
        hb.set_action_limits(*lim)
        for pair in lone:
            for h in pair:
                h.set_action_limits(*lim)
    for step in range(5):
        ub = hb.next(X)
        Ub = hb.get_action_sequences()
        for i, pair in enumerate(lone):
            cb = hb.debug_get(i, m.DBG_COSTS)
            for h in pair:
                u = h.next(X[i])
                np.testing.assert_array_equal(ub[i], u, err_msg="member %d step %d (%s)" % (i, step, h.rollout_kernel_name()))
                np.testing.assert_array_equal(Ub[i], h.get_action_sequence(), err_msg="member %d step %d" % (i, step))
                np.testing.assert_array_equal(cb, h.debug_get(m.DBG_COSTS), err_msg="member %d step %d" % (i, step))
        X = np.stack([plant(X[i], ub[i], a) for i in range(B)])
    assert hb.get_step_counter() == 5
    for pair in lone:
        for h in pair:
            h.close()
    hb.close()


@pytest.mark.parametrize("B,K,H,a", [(3, 3000, 50, 2), (2, 4096, 64, 3)])
def test_batch_against_oracle(m, B, K, H, a):
    """Per member: the noise is the Philox restatement at seeds[m] (5e-6), the costs are the oracle's on that noise bit for bit, u and U'
    within 1e-5."""
    c = common(K, H, a)
    X, G, _ = members(B, a, H, seed=1)
    seeds = [3, 40, 500][:B]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    probs = [orc.Problem(tau=H, s=2 * a, a=a, dt=0.1, mass=1.0, lam=1.0, sigma=c["sigma"], goal=G[i], Q=c["Q"], threads=0) for i in range(B)]
    U = [np.zeros((H, a), F32) for _ in range(B)]
    for step in range(3):
        ub = hb.next(X)
        Ub = hb.get_action_sequences()
        for i in range(B):
            eps = hb.debug_get(i, m.DBG_NOISE)
            np.testing.assert_allclose(eps, orc.noise(seeds[i], step, 0, K, H, a, c["sigma"]), rtol=0, atol=5e-6)
            u_ref, U_ref, c_ref = probs[i].next_with_noise(X[i], U[i], eps)
            np.testing.assert_array_equal(hb.debug_get(i, m.DBG_COSTS), c_ref)
            np.testing.assert_allclose(ub[i], u_ref, rtol=0, atol=U_TOL)
            np.testing.assert_allclose(Ub[i], U_ref, rtol=0, atol=U_TOL)
            U[i] = Ub[i]
        X = np.stack([plant(X[i], ub[i], a) for i in range(B)])
    hb.close()


def test_members_are_independent(m):
    """Changing member j's x, goal and sequence changes no bit of any other member's u, U' or costs."""
    B, K, H, a, j = 6, 4096, 64, 2, 2
    c = common(K, H, a)
    X, G, U0 = members(B, a, H, seed=2)
    X2, G2, U2 = X.copy(), G.copy(), U0.copy()
    X2[j] += 0.5
    G2[j, 0] -= 0.7
    U2[j] = -U2[j]
    h1, h2 = m.BatchHandle(n=B, goals=G, **c), m.BatchHandle(n=B, goals=G2, **c)
    h1.set_action_sequences(U0)
    h2.set_action_sequences(U2)
    others = [i for i in range(B) if i != j]
    for step in range(3):
        u1, u2 = h1.next(X), h2.next(X2)
        assert not np.array_equal(u1[j], u2[j])
        np.testing.assert_array_equal(u1[others], u2[others])
        np.testing.assert_array_equal(h1.get_action_sequences()[others], h2.get_action_sequences()[others])
        for i in others:
            np.testing.assert_array_equal(h1.debug_get(i, m.DBG_COSTS), h2.debug_get(i, m.DBG_COSTS))
            np.testing.assert_array_equal(h1.debug_get(i, m.DBG_U_UPDATED), h2.debug_get(i, m.DBG_U_UPDATED))
    h1.close(); h2.close()


def test_device_path_equals_host_path(m):
    """25 pipelined batched steps from torch tensors (no host in between) = 25 host-synchronous steps; the step counter is 25."""
    import torch
    B, K, H, a = 4, 4096, 64, 2
    c = common(K, H, a)
    X, G, U0 = members(B, a, H, seed=3)
    hd, hh = m.BatchHandle(n=B, goals=G, **c), m.BatchHandle(n=B, goals=G, **c)
    for h in (hd, hh):
        h.set_action_sequences(U0)
        h.set_action_limits([-0.4, -0.3], [0.35, 0.3])
    x = torch.from_numpy(X).cuda()
    u = torch.zeros((B, a), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    for _ in range(25):
        hd.next_device(x.data_ptr(), u.data_ptr(), st)
    for _ in range(25):
        uh = hh.next(X)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u.cpu().numpy(), uh)
    np.testing.assert_array_equal(hd.get_action_sequences(), hh.get_action_sequences())
    assert hd.get_step_counter() == hh.get_step_counter() == 25
    hd.close(); hh.close()


def test_refusals(m):
    from mppi_tf_amd import _lib
    lib = _lib.load()
    UNSUP, INVAL = _lib.ERR_UNSUPPORTED, _lib.ERR_INVALID_ARG
    # options outside the batched kernels: refused before anything is allocated, with a message that names the option
    for fields, word in [(dict(model_kind=_lib.MODEL_MLP), "MLP"), (dict(model_kind=_lib.MODEL_AUV, s_dim=13, a_dim=6), "AUV"),
                         (dict(model_kind=_lib.MODEL_NN_AUV, s_dim=13, a_dim=6), "NNAUV"),
                         (dict(model_kind=_lib.MODEL_NN_AUV_SPEED, s_dim=13, a_dim=6), "NNAUVSpeed"),
                         (dict(state_cost_kind=_lib.STATE_COST_ELLIPSE), "ellipse"), (dict(state_cost_kind=_lib.STATE_COST_ELLIPSE3D, s_dim=13, a_dim=6), "ellipse"),
                         (dict(state_cost_kind=_lib.STATE_COST_QUAT, s_dim=13, a_dim=6), "StaticQuatCost"), (dict(normalize_cost=1), "normalize_cost"),
                         (dict(flags=4), "FP_CONTRACT"), (dict(flags=2), "BF16X3"), (dict(shard_count=2), "shard")]:
        st, h = create_batch(**fields)
        assert st == UNSUP and not h, fields
        assert word in lib.mppi_last_error(None).decode(), (fields, lib.mppi_last_error(None))
    st, h = create_batch(n=0)
    assert st == INVAL and not h
    hb = m.BatchHandle(n=3, k=256, tau=16, s_dim=4, a_dim=2)
    assert lib.mppi_batch_size(hb.h) == 3
    # tunings a batch does not take (the two-launch batched step, always); fused_step = 0 is what it runs
    for key, val in (("fused_step", 1), ("armed_us", 100), ("prelaunch", 1), ("force_tile_kernel", 1)):
        with pytest.raises(m.MppiError) as e:
            hb.set_tuning(key, val)
        assert e.value.status == UNSUP and key in str(e.value)
    hb.set_tuning("fused_step", 0)
    # per-member single-handle entry points
    f = np.zeros(4096, F32)
    p = f.ctypes.data_as(_lib.FP)
    dev = 0x1000  # never dereferenced: the refusal comes first
    calls = [lambda: lib.mppi_next(hb.h, p, 4, p, 2), lambda: lib.mppi_next_with_noise(hb.h, p, 4, p, 256 * 32, p, 2),
             lambda: lib.mppi_next_device(hb.h, dev, dev, None), lambda: lib.mppi_set_goal(hb.h, p, 4),
             lambda: lib.mppi_get_action_sequence(hb.h, p, 32), lambda: lib.mppi_set_action_sequence(hb.h, p, 32),
             lambda: lib.mppi_debug_get(hb.h, 0, p, 256), lambda: lib.mppi_shard_partial(hb.h, dev, dev, None),
             lambda: lib.mppi_shard_finish(hb.h, dev, 1, dev, None), lambda: lib.mppi_shard_cost_range(hb.h, dev, dev, None),
             lambda: lib.mppi_shard_partial_normalized(hb.h, dev, dev, dev, None), lambda: lib.mppi_shard_step(hb.h, dev, dev, None, None),
             lambda: lib.mppi_shard_p2p_export(hb.h, None, C.byref(C.c_void_p())),
             lambda: lib.mppi_shard_p2p_open(hb.h, C.create_string_buffer(64), C.byref(C.c_void_p())),
             lambda: lib.mppi_shard_p2p_attach(hb.h, (C.c_void_p * 1)(dev), 1, 100), lambda: lib.mppi_shard_p2p_probe(hb.h, None, C.byref(C.c_int())),
             lambda: lib.mppi_shard_p2p_step(hb.h, dev, dev, None), lambda: lib.mppi_shard_p2p_status(hb.h, C.byref(C.c_int())),
             lambda: lib.mppi_set_transition_log(hb.h, 10), lambda: lib.mppi_transition_log_stats(hb.h, None, None, None),
             lambda: lib.mppi_save_next(hb.h, p, 4), lambda: lib.mppi_to_csv(hb.h, b"/nonexistent/x.csv"),
             lambda: lib.mppi_to_csv_format(hb.h, b"/nonexistent/x.csv", 0), lambda: lib.mppi_set_sequence_filter(hb.h, 5, 2)]
    for i, call in enumerate(calls):
        assert call() == UNSUP, i
    # sizes, member range; the batched calls on a plain handle
    assert lib.mppi_batch_next(hb.h, p, 4 * 3 - 1, p, 6) == INVAL
    assert lib.mppi_batch_next(hb.h, p, 12, p, 5) == INVAL
    assert lib.mppi_batch_set_goals(hb.h, p, 4) == INVAL
    assert lib.mppi_batch_get_action_sequences(hb.h, p, 32) == INVAL
    assert lib.mppi_batch_set_action_sequences(hb.h, p, 3 * 32 + 1) == INVAL
    assert lib.mppi_batch_debug_get(hb.h, 3, m.DBG_COSTS, p, 256) == INVAL
    assert lib.mppi_batch_debug_get(hb.h, -1, m.DBG_COSTS, p, 256) == INVAL
    assert lib.mppi_batch_debug_get(hb.h, 0, m.DBG_COSTS, p, 255) == INVAL
    h1 = m.Handle(k=256, tau=16, s_dim=4, a_dim=2)
    assert lib.mppi_batch_size(h1.h) == 0
    assert lib.mppi_batch_next(h1.h, p, 4, p, 2) == INVAL
    assert lib.mppi_batch_debug_get(h1.h, 0, m.DBG_COSTS, p, 256) == INVAL
    # what a batch shares and still serves
    hb.next(np.zeros((3, 4), F32))
    hb.set_step_counter(7)
    assert hb.get_step_counter() == 7
    hb.synchronize()
    h1.close(); hb.close()


def test_closed_loop_every_plant_approaches_its_goal(m):
    """B = 8 point-mass plants with distinct starts and goals, 100 batched steps: each ends closer to ITS goal than it started."""
    B, K, H, a = 8, 2048, 40, 2
    c = common(K, H, a)
    rng = np.random.default_rng(5)
    X = np.zeros((B, 4), F32)
    X[:, 0::2] = rng.uniform(-1.5, 1.5, (B, 2))
    G = np.zeros((B, 4), F32)
    G[:, 0::2] = rng.uniform(-1.5, 1.5, (B, 2))
    hb = m.BatchHandle(n=B, goals=G, **c)
    d0 = np.linalg.norm(X - G, axis=1)
    for _ in range(100):
        u = hb.next(X)
        X = np.stack([plant(X[i], u[i], a) for i in range(B)])
    d1 = np.linalg.norm(X - G, axis=1)
    assert np.all(d1 < d0), (d0, d1)
    hb.close()
