"""Batched controllers of the Fossen AUV model (mppi_create_batch with MPPI_MODEL_AUV / BatchHandle(auv=...)): B independent AUV controllers
stepped in the same two launches as one (k_rollout_auv_pc_batch + k_finish_cols_batch<6>). Needs an MI355X: every test is marked `gpu`.

The contract (include/mppi_c.h): member m is BIT-IDENTICAL to a lone Handle made from the same configuration with seed = seeds[m], on its
default k_rollout_auv_pc path, fed the same x, goal and action sequence on the same step counter: sample costs, U' and u; members never
interact. Through that, every member inherits the lone handle's parity with the oracle; a direct oracle check is here as well.
"""
import numpy as np
import pytest

from batch_util import (E3, Q10, auv_members as members, batch_with as _batch_with, batch_with_mlp as _batch_with_mlp, create_batch, lone,
                        rexrov2)
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32
U_TOL = 1e-5


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def config(K, H, cost="quadratic", rk=2, dense_sigma=False):
    """the keywords of Handle / BatchHandle (without seeds and goals): rexrov2 at `rk`, Sigma = 1500 I (or a dense one), the state cost"""
    from mppi_tf_amd.auv import auv_task
    t = auv_task(H)
    d = dict(k=K, tau=H, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=t["sigma"], auv=rexrov2(rk))
    if dense_sigma:
        rng = np.random.default_rng(11)
        S = rng.uniform(-100.0, 100.0, (6, 6))
        d["sigma"] = (1500.0 * np.eye(6) + (S + S.T) / 2).astype(F32)
    if cost == "quadratic":
        d["Q"] = t["Q"]
    elif cost == "dense":
        d["Q"], d["q_is_full"] = (np.diag(t["Q"]) + 0.05).astype(F32), True
    elif cost == "quat":
        d["Q"], d["quat_cost"] = Q10, True
    else:
        d["ellipse3d"] = E3
    return d


EQUIV = [(4, 4096, 40, "quadratic", 2, False), (3, 1000, 20, "quat", 4, False), (5, 3000, 16, "dense", 1, True),
         (16, 4096, 40, "ellipse3d", 2, False), (2, 65536, 64, "quadratic", 2, False), (1, 64, 8, "quadratic", 2, False)]


@pytest.mark.parametrize("B,K,H,cost,rk,dense_sigma", EQUIV)
def test_auv_batch_equals_standalone_handles(m, B, K, H, cost, rk, dense_sigma):
    """Every member, every step: u, the member's sequence and its sample costs are the bits of Handle(seed=seeds[m]) on k_rollout_auv_pc."""
    c = config(K, H, cost, rk, dense_sigma)
    X, G, U0 = members(B, H)
    seeds = [5 + 13 * i for i in range(B)]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    assert hb.lib.mppi_batch_size(hb.h) == B
    assert hb.rollout_kernel_name() == "mppi::k_rollout_auv_pc_batch<%s>" % ("false" if dense_sigma else "true")
    hb.set_action_sequences(U0)
    hs = lone(m, c, seeds, G, U0)
    plant = hs[0]
    for step in range(3):
        ub = hb.next(X)
        Ub = hb.get_action_sequences()
        for i, h in enumerate(hs):
            u = h.next(X[i])
            np.testing.assert_array_equal(hb.debug_get(i, m.DBG_COSTS), h.debug_get(m.DBG_COSTS), err_msg="member %d step %d" % (i, step))
            np.testing.assert_array_equal(ub[i], u, err_msg="member %d step %d" % (i, step))
            np.testing.assert_array_equal(Ub[i], h.get_action_sequence(), err_msg="member %d step %d" % (i, step))
        X = plant.model_next(X, ub)
    assert hb.get_step_counter() == 3
    for h in hs:
        h.close()
    hb.close()


def test_auv_batch_against_oracle(m):
    """One member at K = 1000: its noise is the Philox restatement at its key, its costs the fp32 oracle's on that noise bit for bit, U'
    and u within 1e-5 of the noise scale."""
    B, K, H, j = 3, 1000, 12, 1
    c = config(K, H)
    X, G, _ = members(B, H, seed=1)
    seeds = [3, 40, 500]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    p = orc.Problem(tau=H, s=13, a=6, dt=0.1, lam=1.0, sigma=c["sigma"], goal=G[j], Q=c["Q"], auv=c["auv"], threads=0, dtype=F32)
    U = np.zeros((H, 6), F32)
    for step in range(2):
        ub = hb.next(X)
        eps = hb.debug_get(j, m.DBG_NOISE)
        np.testing.assert_allclose(eps / 1500.0, orc.noise(seeds[j], step, 0, K, H, 6, c["sigma"]) / 1500.0, rtol=0, atol=5e-6)
        u_ref, U_ref, c_ref = p.next_with_noise(X[j], U, eps)
        np.testing.assert_array_equal(hb.debug_get(j, m.DBG_COSTS), c_ref)
        Ub = hb.get_action_sequences()[j]
        np.testing.assert_allclose(Ub / 1500.0, U_ref / 1500.0, rtol=0, atol=U_TOL)
        np.testing.assert_allclose(ub[j] / 1500.0, u_ref / 1500.0, rtol=0, atol=U_TOL)
        U = Ub
        X = X.copy()
        X[:, 7:] *= 0.5
    hb.close()


def test_auv_members_are_independent(m):
    """Changing member j's x, goal and sequence changes no bit of any other member's u, U' or costs."""
    B, K, H, j = 6, 2048, 20, 2
    c = config(K, H, "quat")
    X, G, U0 = members(B, H, seed=2)
    X2, G2, U2 = X.copy(), G.copy(), U0.copy()
    X2[j, :3] += 0.5
    G2[j, 0] -= 0.7
    G2[j, 3:7] = [0.0, 0.0, 0.0, 1.0]
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


def test_auv_device_path_equals_host_path(m):
    """10 pipelined batched steps from torch tensors (no host in between), action limits set = 10 host-synchronous steps."""
    import torch
    B, K, H = 4, 4096, 40
    c = config(K, H)
    X, G, U0 = members(B, H, seed=3)
    lim = ([-900.0, -800.0, -700.0, -600.0, -500.0, -400.0], [400.0, 500.0, 600.0, 700.0, 800.0, 900.0])
    hd, hh = m.BatchHandle(n=B, goals=G, **c), m.BatchHandle(n=B, goals=G, **c)
    for h in (hd, hh):
        h.set_action_sequences(U0)
        h.set_action_limits(*lim)
    x = torch.from_numpy(X).cuda()
    u = torch.zeros((B, 6), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    for _ in range(10):
        hd.next_device(x.data_ptr(), u.data_ptr(), st)
    for _ in range(10):
        uh = hh.next(X)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u.cpu().numpy(), uh)
    np.testing.assert_array_equal(hd.get_action_sequences(), hh.get_action_sequences())
    assert np.all(uh >= np.array(lim[0], F32)) and np.all(uh <= np.array(lim[1], F32))
    assert hd.get_step_counter() == hh.get_step_counter() == 10
    hd.close(); hh.close()


def test_auv_debug_items_equal_lone_handles(m):
    """DBG_NOISE (regenerated from the member's key through the 13-state noise-only pass) and DBG_WEIGHTS of member m are the lone handle's."""
    B, K, H = 3, 1000, 12
    c = config(K, H, "ellipse3d")
    X, G, U0 = members(B, H, seed=4)
    seeds = [7, 8, 99]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hb.set_action_sequences(U0)
    hs = lone(m, c, seeds, G, U0)
    for step in range(2):
        ub = hb.next(X)
        for i, h in enumerate(hs):
            h.next(X[i])
            np.testing.assert_array_equal(hb.debug_get(i, m.DBG_NOISE), h.debug_get(m.DBG_NOISE), err_msg="member %d" % i)
            np.testing.assert_array_equal(hb.debug_get(i, m.DBG_WEIGHTS), h.debug_get(m.DBG_WEIGHTS), err_msg="member %d" % i)
            assert hb.debug_get(i, m.DBG_BETA) == h.debug_get(m.DBG_BETA) and hb.debug_get(i, m.DBG_ETA) == h.debug_get(m.DBG_ETA)
        X = hs[0].model_next(X, ub)
    for h in hs:
        h.close()
    hb.close()


def test_auv_batch_refusals(m):
    from mppi_tf_amd import _lib
    lib = _lib.load()
    UNSUP = _lib.ERR_UNSUPPORTED
    nn = dict(W=[np.zeros((16, 32), F32), np.zeros((32, 13), F32)], b=[np.zeros(32, F32), np.zeros(13, F32)])
    nns = dict(W=[np.zeros((15, 32), F32), np.zeros((32, 6), F32)], b=[np.zeros(32, F32), np.zeros(6, F32)])
    for kw, word in [(dict(nnauv=nn), "NNAUV"), (dict(nnauv_speed=nns), "NNAUVSpeed")]:
        with pytest.raises(m.MppiError) as e:
            _batch_with_mlp(m, kw)
        assert e.value.status == UNSUP and word in str(e.value), str(e.value)
    st, h = create_batch(s_dim=13, a_dim=6, model_kind=_lib.MODEL_AUV)
    assert st == UNSUP and not h and "AUV" in lib.mppi_last_error(None).decode()
    with pytest.raises(m.MppiError) as e:
        _batch_with(m, normalize_cost=1)
    assert e.value.status == UNSUP and "normalize_cost" in str(e.value)
    hb = m.BatchHandle(n=2, **config(256, 16))
    for key in ("gen_one_wave", "mlp32_valu"):
        with pytest.raises(m.MppiError) as e:
            hb.set_tuning(key, 1)
        assert e.value.status == UNSUP and key in str(e.value)
    hb.set_tuning("gen_one_wave", 0)
    f = np.zeros(4096, F32)
    p = f.ctypes.data_as(_lib.FP)
    assert lib.mppi_next(hb.h, p, 13, p, 6) == UNSUP
    assert "mppi_next" in lib.mppi_last_error(hb.h).decode()
    assert hb.rollout_kernel_name() == "mppi::k_rollout_auv_pc_batch<true>"
    hb.next(members(2, 16)[0])  # still serves its own steps
    hb.close()


def test_auv_closed_loop_equals_lone_handles(m):
    """B = 4 AUVs with different goals, 20 steps, the plant stepped on the device (a lone AUV handle's model step on the B states): the
    batch's trajectories are the bits of B lone handles' in the same loop, and the vehicles end closer to their goal positions."""
    B, K, H = 4, 2048, 20
    c = config(K, H)
    rng = np.random.default_rng(9)
    X0 = np.zeros((B, 13), F32)
    X0[:, 6] = 1.0
    G = np.zeros((B, 13), F32)
    G[:, :3] = rng.uniform(-2, 2, (B, 3))
    G[:, 6] = 1.0
    seeds = [21, 22, 23, 24]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hs = lone(m, c, seeds, G, np.zeros((B, H, 6), F32))
    plant = m.Handle(k=B, tau=1, s_dim=13, a_dim=6, dt=0.1, sigma=np.eye(6), auv=rexrov2())
    Xb, Xl = X0.copy(), X0.copy()
    for _ in range(20):
        ub = hb.next(Xb)
        ul = np.stack([h.next(Xl[i]) for i, h in enumerate(hs)])
        np.testing.assert_array_equal(ub, ul)
        Xb, Xl = plant.model_next(Xb, ub), plant.model_next(Xl, ul)
        np.testing.assert_array_equal(Xb, Xl)
    d0 = np.linalg.norm(X0[:, :3] - G[:, :3], axis=1)
    d1 = np.linalg.norm(Xb[:, :3] - G[:, :3], axis=1)
    assert d1.mean() < d0.mean(), (d0, d1)
    for h in hs + [plant]:
        h.close()
    hb.close()
