"""Closed-loop episodes against a separate plant (mppi_run_episode_plant / mppi_batch_run_episode_plant; run_episode(..., plant=)): the
controller plans with its own model, the state is stepped by ANOTHER handle's model. Needs an MI355X: every test is marked `gpu`.

The contract (include/mppi_c.h): such an episode equals, bit for bit, the host loop set_goal, state_cost and next on the controller,
model_next on the plant handle, fp32 add of w (episode_plant_util.host_loop_plant) in X, U, C, the controller's final sequence and its
step counter; member m of a batched episode equals its lone controller on its lone plant; a plant is left as it was. Every comparison
is assert_array_equal: there are no tolerances in this file. Each case runs 6 steps as two calls (2 + 4) with a goal per step and a
non-zero disturbance (13 states: off the quaternion)."""
import os
import sys

import numpy as np
import pytest

from batch_util import E3, Q10, auv_members, lone_handles, pm_members, rexrov2
from conftest import ROOT
from episode_plant_util import (assert_plant_untouched, auv_plant, check_lone_plant, heavier, host_loop_plant, plant_state, pm_plant,
                                pm_rollout_plant)
from episode_util import auv_cfg, make_nnauv, pm_cfg, pm_x0, signals

pytestmark = pytest.mark.gpu
F32 = np.float32
CALLS = [2, 4]
N = sum(CALLS)
VEL = list(range(7, 13))  # the 13-state disturbance: on the velocities only


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def close(*hs):
    for h in hs:
        h.close()


def _dense_q():
    rng = np.random.default_rng(7)
    L = rng.uniform(-0.3, 0.3, (4, 4)) + np.eye(4)
    return (L @ L.T).astype(F32)


def _plant_was_used(m, make, x0, goals, dist, X):
    """the plain episode of a twin controller (its own model as the plant) leaves x0 for another x_1"""
    h = make()
    Xp = h.run_episode(x0, CALLS[0], goals[:CALLS[0]], dist[:CALLS[0]])[0]
    assert np.isfinite(Xp).all() and not np.array_equal(Xp[1], X[1]), "the plant episode's x_1 is the controller's own model's"
    h.close()


# ---- point mass, lone controller ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_point_mass_on_a_heavier_plant(m, a):
    """K = 200 (ragged, the one-launch step), H = 12; the controller's mass 1.0 and dt 0.1, the plant's 1.5 and 0.05. The plant is a
    controller in its own right (a = 2: and the plain episode differs), left untouched."""
    c = pm_cfg(200, 12, a)
    G, W = signals(N, 2 * a, seed=20 + a)
    make = lambda: m.Handle(**c)  # noqa: E731
    X, hs = check_lone_plant(make, lambda: pm_rollout_plant(m, a), pm_x0(a), CALLS, G, W, tag="a=%d" % a)
    assert np.isfinite(X).all()
    assert hs[0].rollout_kernel_name().startswith("mppi::k_step_pc<")
    if a == 2:
        _plant_was_used(m, make, pm_x0(a), G, W, X)
    close(*hs)


def test_point_mass_dense_q(m):
    c = pm_cfg(200, 12, 2, Q=_dense_q())
    G, W = signals(N, 4, seed=31)
    X, hs = check_lone_plant(lambda: m.Handle(**c), lambda: pm_plant(m, 2), pm_x0(2), CALLS, G, W, tag="dense Q")
    assert np.isfinite(X).all()
    close(*hs)


def test_point_mass_two_launch_step(m):
    """K = 8256 = 129 tiles: above the one-launch step's 128, rollout + finish"""
    c = pm_cfg(8256, 8, 2)
    G, W = signals(N, 4, seed=32)
    X, hs = check_lone_plant(lambda: m.Handle(**c), lambda: pm_plant(m, 2), pm_x0(2), CALLS, G, W, tag="129 tiles")
    assert hs[0].rollout_kernel_name().startswith("mppi::k_rollout_pc<")
    close(*hs)


def test_the_controller_as_its_own_plant(m):
    """plant = h itself: the plain episode of a twin"""
    c = pm_cfg(200, 12, 3)
    G, W = signals(N, 6, seed=33)
    he, ht = m.Handle(**c), m.Handle(**c)
    for e, t in zip(he.run_episode(pm_x0(3), N, G, W, plant=he), ht.run_episode(pm_x0(3), N, G, W)):
        np.testing.assert_array_equal(e, t)
    np.testing.assert_array_equal(he.get_action_sequence(), ht.get_action_sequence())
    assert he.get_step_counter() == ht.get_step_counter() == N
    close(he, ht)


# ---- the 13-state family -------------------------------------------------------------------------------------------------------------
def _auv_signals(seed):
    X0, G, U0 = auv_members(1, 8, seed=seed)
    goals = np.repeat(G, N, axis=0)
    goals[:, :3] += np.random.default_rng(seed).uniform(-0.5, 0.5, (N, 3)).astype(F32)  # the position moves, the attitude stays a unit quaternion
    _, W = signals(N, 13, seed=seed, scale=0.02, cols=VEL)
    return X0[0], goals, W, U0[0]


def _nn_controller(m, cost, speed, seed=9):
    """keywords of a learned 13-state controller: NNAUVModel or NNAUVModelSpeed (hid 16, one hidden layer), K = 128, H = 8"""
    mlp = make_nnauv(3, 16, 1, n_in=15, n_out=6) if speed else make_nnauv(3, 16, 1)
    c = dict(k=128, tau=8, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=np.eye(6, dtype=F32), seed=seed)
    c["nnauv_speed" if speed else "nnauv"] = mlp
    if cost == "quat":
        c["Q"], c["quat_cost"] = Q10, True
    else:
        c["ellipse3d"] = E3
    return c


def _nn_plant_weights(seed):
    """NNAUVModel weights for a plant driven by a Fossen controller: the forces (columns 10..15 of the input) in their own units"""
    mlp = make_nnauv(seed, 16, 1)
    mlp["xstd"][10:] = F32(1500.0)
    return mlp


def _nn_plant(m, mlp):
    return m.Handle(k=1, tau=1, s_dim=13, a_dim=6, dt=0.1, sigma=np.eye(6, dtype=F32), goal=np.zeros(13, F32), nnauv=mlp)


@pytest.mark.parametrize("cost,speed", [("quat", False), ("ellipse3d", True)])
def test_learned_controller_on_the_fossen_plant(m, cost, speed):
    """NNAUVModel with StaticQuatCost / NNAUVModelSpeed with ElipseCost3D plan, the rexrov2 Fossen model (rk 2) is the vehicle"""
    c = _nn_controller(m, cost, speed)
    x0, G, W, _ = _auv_signals(40 + speed)
    make = lambda: m.Handle(goal=G[0], **c)  # noqa: E731
    X, hs = check_lone_plant(make, lambda: auv_plant(m, rexrov2(2)), x0, CALLS, G, W, tag="%s speed=%d" % (cost, speed))
    assert np.isfinite(X).all()
    if not speed:
        _plant_was_used(m, make, x0, G, W, X)
    close(*hs)


def test_fossen_controller_on_a_learned_plant(m):
    """a learned plant, shared: its model-step kernel in a launch of its own behind the control step"""
    c = auv_cfg(128, 8, "quat")
    x0, G, W, U0 = _auv_signals(42)
    mlp = _nn_plant_weights(6)

    def make():
        h = m.Handle(goal=G[0], seed=4, **c)
        h.set_action_sequence(U0)
        return h
    X, hs = check_lone_plant(make, lambda: _nn_plant(m, mlp), x0, CALLS, G, W, tag="nnauv plant")
    assert np.isfinite(X).all()
    assert hs[0].rollout_kernel_name().startswith("mppi::k_rollout_auv_pc<")
    close(*hs)


def test_replaced_plant_weights_take_effect(m):
    """mppi_set_mlp on the plant between two calls: the second call runs the new network, as the host loop with the new weights does"""
    c = auv_cfg(128, 8, "quat")
    x0, G, W, U0 = _auv_signals(43)
    old, new = _nn_plant_weights(6), _nn_plant_weights(11)

    def make():
        h = m.Handle(goal=G[0], seed=4, **c)
        h.set_action_sequence(U0)
        return h
    X, hs = check_lone_plant(make, lambda: _nn_plant(m, old), x0, CALLS, G, W, tag="new weights", between=lambda p: p.set_mlp(new))
    assert np.isfinite(X).all()
    # ... and they did change the trajectory: the same episode on the old weights throughout leaves another x behind the second call
    h, p = make(), _nn_plant(m, old)
    Xo = h.run_episode(x0, N, G, W, plant=p)[0]
    np.testing.assert_array_equal(Xo[:CALLS[0] + 1], X[:CALLS[0] + 1])
    assert not np.array_equal(Xo[CALLS[0] + 1], X[CALLS[0] + 1])
    close(h, p, *hs)


# ---- a twin plant is the plain episode ---------------------------------------------------------------------------------------------
def _twin(m, make, make_plant, x0, G, W, tag):
    he, ht, p = make(), make(), make_plant()
    for name, e, t in zip("XUC", he.run_episode(x0, N, G, W, plant=p), ht.run_episode(x0, N, G, W)):
        assert np.isfinite(e).all()
        np.testing.assert_array_equal(e, t, err_msg="%s %s" % (name, tag))
    np.testing.assert_array_equal(he.get_action_sequence(), ht.get_action_sequence())
    close(he, ht, p)


def test_twin_plant_point_mass(m):
    c = pm_cfg(200, 12, 2)
    G, W = signals(N, 4, seed=50)
    _twin(m, lambda: m.Handle(**c), lambda: pm_plant(m, 2, mass=c["mass"], dt=c["dt"]), pm_x0(2), G, W, "point mass")


def test_twin_plant_fossen(m):
    c = auv_cfg(128, 8, "quat")
    x0, G, W, U0 = _auv_signals(51)

    def make():
        h = m.Handle(goal=G[0], seed=4, **c)
        h.set_action_sequence(U0)
        return h
    _twin(m, make, lambda: auv_plant(m, rexrov2(2)), x0, G, W, "fossen")


def test_twin_plant_nnauv(m):
    c = _nn_controller(m, "quat", False)
    x0, G, W, _ = _auv_signals(52)
    _twin(m, lambda: m.Handle(goal=G[0], **c), lambda: _nn_plant(m, c["nnauv"]), x0, G, W, "nnauv")


# ---- the learned point mass --------------------------------------------------------------------------------------------------------
def test_learned_point_mass_controller_on_an_analytic_plant(m):
    mlp = make_nnauv(5, 32, 1, n_in=6, n_out=4)
    c = pm_cfg(64, 4, 2, mlp=mlp)
    G, W = signals(N, 4, seed=60)
    make = lambda: m.Handle(**c)  # noqa: E731
    X, hs = check_lone_plant(make, lambda: pm_plant(m, 2), pm_x0(2), CALLS, G, W, tag="mlp controller")
    assert np.isfinite(X).all()
    _plant_was_used(m, make, pm_x0(2), G, W, X)
    close(*hs)


def test_point_mass_controller_on_a_learned_plant(m):
    mlp = make_nnauv(5, 32, 1, n_in=6, n_out=4)
    c = pm_cfg(200, 12, 2)
    G, W = signals(N, 4, seed=61)
    X, hs = check_lone_plant(lambda: m.Handle(**c), lambda: m.Handle(**pm_cfg(64, 4, 2, mlp=mlp)), pm_x0(2), CALLS, G, W, tag="mlp plant")
    assert np.isfinite(X).all()
    close(*hs)


# ---- batches -----------------------------------------------------------------------------------------------------------------------
def _assert_members_on_plants(hb, hs, plants_b, plants_h, X0, goals, dist, tag, members=None):
    """the batch hb on plants_b (one Handle or a list) in two calls against the host loops of the lone controllers hs[i] on plants_h[i]"""
    B = hb.n
    X, t, got = X0, 0, []
    for c in CALLS:
        got.append(hb.run_episode(X, c, goals[t:t + c], dist[t:t + c], plant=plants_b))
        assert got[-1][0].shape == (c + 1, B, hb.s) and got[-1][1].shape == (c, B, hb.a) and got[-1][2].shape == (c, B)
        X, t = got[-1][0][-1], t + c
    Xb = np.concatenate([got[0][0]] + [g[0][1:] for g in got[1:]])
    Ub, Cb = np.concatenate([g[1] for g in got]), np.concatenate([g[2] for g in got])
    assert np.isfinite(Xb).all()
    Useq = hb.get_action_sequences()
    for i in (range(B) if members is None else members):
        Xh, Uh, Ch = host_loop_plant(hs[i], plants_h[i], X0[i], N, goals[:, i], dist[:, i])
        msg = "member %d %s" % (i, tag)
        np.testing.assert_array_equal(Ub[:, i], Uh, err_msg="U " + msg)
        np.testing.assert_array_equal(Xb[:, i], Xh, err_msg="X " + msg)
        np.testing.assert_array_equal(Cb[:, i], Ch, err_msg="C " + msg)
        np.testing.assert_array_equal(Useq[i], hs[i].get_action_sequence(), err_msg="sequence " + msg)
        assert hs[i].get_step_counter() == hb.get_step_counter() == N
    return Xb


def _batch_pm(m, B):
    shared = dict(k=256, tau=16, s_dim=4, a_dim=2, dt=0.1, mass=1.0, Q=np.ones(4, F32))
    lams = [0.5, 1.0, 2.0][:B]
    seeds = [11 + 7 * i for i in range(B)]
    X0, G, U0 = pm_members(B, 2, 16)
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, lams=lams, **shared)
    hb.set_action_sequences(U0)
    twin = lambda i: lone_handles(m, [dict(shared, lam=lams[i])], seeds[i:i + 1], G[i:i + 1], U0[i:i + 1], "mppi::k_step_pc<")[0]  # noqa: E731
    hs = [twin(i) for i in range(B)]
    rng = np.random.default_rng(21)
    goals = np.zeros((N, B, 4), F32)
    goals[:, :, 0::2] = rng.uniform(-1, 1, (N, B, 2))
    dist = rng.uniform(-0.05, 0.05, (N, B, 4)).astype(F32)
    return hb, hs, X0, goals, dist, twin


@pytest.mark.parametrize("plants", ["shared", "members"])
def test_batched_point_mass(m, plants):
    """B = 3 with per-member lambda on one shared plant (mass 1.5) and on per-member plants of mass 0.8 / 1.0 / 1.5: member m's slices
    are its lone controller's host loop on its lone plant; the plants are left as they were"""
    B = 3
    hb, hs, X0, goals, dist, twin = _batch_pm(m, B)
    masses = [1.5] * B if plants == "shared" else [0.8, 1.0, 1.5]
    pb = [pm_rollout_plant(m, 2, mass=v, dt=0.1) for v in (masses[:1] if plants == "shared" else masses)]
    ph = [pm_plant(m, 2, mass=v, dt=0.1) for v in masses]
    probe = np.full(4, 0.3, F32)
    before = [plant_state(p, probe) for p in pb]
    Xb = _assert_members_on_plants(hb, hs, pb[0] if plants == "shared" else pb, ph, X0, goals, dist, plants)
    for p, b in zip(pb, before):
        assert_plant_untouched(p, b, probe, plants)
    # the plant was used: the plain episode of member 0's twin (its own mass 1.0; the plant's is 1.5 or 0.8) leaves x0 for another x_1
    h = twin(0)
    Xo = h.run_episode(X0[0], CALLS[0], goals[:CALLS[0], 0], dist[:CALLS[0], 0])[0]
    assert np.isfinite(Xo).all() and not np.array_equal(Xo[1], Xb[1, 0])
    h.close()
    close(hb, *hs, *pb, *ph)


def test_batched_members_on_both_sides_of_a_workgroup(m):
    """B = 65, K = 64, H = 4, a plant per member (masses 0.8 .. 1.44): the episode kernel's first workgroup of 64 lanes is full, the
    second holds member 64. Members 0, 63 and 64 against their lone controllers on their lone plants."""
    B, a = 65, 2
    c = pm_cfg(64, 4, a)
    del c["seed"], c["goal"]
    seeds = [50 + i for i in range(B)]
    masses = [0.8 + 0.01 * i for i in range(B)]
    X0, G, U0 = pm_members(B, a, 4, seed=5)
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hb.set_action_sequences(U0)
    pick = (0, 63, 64)
    hs = dict(zip(pick, lone_handles(m, [c] * 3, [seeds[i] for i in pick], G[list(pick)], U0[list(pick)], "mppi::k_")))
    plants = [pm_plant(m, a, mass=v, dt=0.1) for v in masses]
    rng = np.random.default_rng(34)
    goals = np.zeros((N, B, 2 * a), F32)
    goals[:, :, 0::2] = rng.uniform(-1, 1, (N, B, a))
    dist = rng.uniform(-0.05, 0.05, (N, B, 2 * a)).astype(F32)
    Xb = _assert_members_on_plants(hb, hs, plants, plants, X0, goals, dist, "B=65", members=pick)
    assert len({Xb[1, i].tobytes() for i in pick}) == 3
    close(hb, *hs.values(), *plants)


def test_batched_fossen_on_per_member_plants(m):
    """B = 2 Fossen controllers (StaticQuatCost), K = 128, H = 8; member 1's vehicle is heavier and drags more"""
    B = 2
    c = auv_cfg(128, 8, "quat")
    X0, G, U0 = auv_members(B, 8, seed=3)
    seeds = [5, 18]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hb.set_action_sequences(U0)
    hs = lone_handles(m, [c] * B, seeds, G, U0, "mppi::k_rollout_auv_pc<")
    plants = [auv_plant(m, rexrov2(2)), auv_plant(m, heavier(rexrov2(2)))]
    goals = np.repeat(G[None], N, axis=0)
    goals[:, :, :3] += np.random.default_rng(8).uniform(-0.5, 0.5, (N, B, 3)).astype(F32)
    dist = np.zeros((N, B, 13), F32)
    dist[:, :, 7:] = np.random.default_rng(4).uniform(-0.02, 0.02, (N, B, 6))
    Xb = _assert_members_on_plants(hb, hs, plants, plants, X0, goals, dist, "auv")
    # the heavier vehicle is another vehicle: the plain episode of member 1's twin (the nominal model) leaves x0 for another x_1
    h = lone_handles(m, [c], seeds[1:], G[1:], U0[1:], "mppi::k_rollout_auv_pc<")[0]
    Xo = h.run_episode(X0[1], CALLS[0], goals[:CALLS[0], 1], dist[:CALLS[0], 1])[0]
    assert np.isfinite(Xo).all() and not np.array_equal(Xo[1], Xb[1, 1])
    close(hb, h, *hs, *plants)


def test_batched_point_mass_on_a_shared_learned_plant(m):
    """one launch of the learned plant's step kernel over the B rows: member m is its lone controller on the same plant"""
    B = 3
    hb, hs, X0, goals, dist, _ = _batch_pm(m, B)
    p = m.Handle(**pm_cfg(64, 4, 2, mlp=make_nnauv(5, 32, 1, n_in=6, n_out=4)))
    _assert_members_on_plants(hb, hs, p, [p] * B, X0, goals, dist, "shared mlp plant")
    close(hb, p, *hs)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(m):
    """every refusal: its status, a message naming the cause, and nothing enqueued (the controller's step counter stands)"""
    import torch
    from mppi_tf_amd import _lib
    lib = _lib.load()
    c = pm_cfg(256, 8, 2)
    x = np.zeros(8, F32)
    out = np.zeros(64, F32)
    fp, H = _lib.fp, _lib._H

    def arr(*ps):
        return (H * len(ps))(*[p.h if p is not None else None for p in ps])

    def refused(h, fn, status, word, plants, n_plants, *args):
        st = fn(h.h, plants, n_plants, *args)
        assert st == status, (fn.__name__, st, lib.mppi_last_error(h.h))
        assert word in lib.mppi_last_error(h.h).decode(), lib.mppi_last_error(h.h)
        assert h.get_step_counter() == 0

    h = m.Handle(**c)
    hb = m.BatchHandle(n=2, **{k: v for k, v in c.items() if k != "seed"})
    p, p2 = pm_plant(m, 2), pm_plant(m, 2, mass=0.8)
    lone, batch = lib.mppi_run_episode_plant, lib.mppi_batch_run_episode_plant
    good = (2, None, None, fp(out), None, None)
    for hh, fn, nx in ((h, lone, 4), (hb, batch, 8)):
        ok = (fp(x), nx, *good)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "plants is NULL", None, 1, *ok)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "is NULL", arr(None), 1, *ok)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "n_plants", arr(p), 0, *ok)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "n_plants", arr(p, p2, p), 3, *ok)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "batched", arr(hb), 1, *ok)
        # ... and those of the plain entry points
        refused(hh, fn, _lib.ERR_INVALID_ARG, "n_steps", arr(p), 1, fp(x), nx, 0, None, None, fp(out), None, None)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "x0", arr(p), 1, fp(x), nx - 1, *good)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "x0", arr(p), 1, None, nx, *good)
    refused(h, lone, _lib.ERR_INVALID_ARG, "n_plants", arr(p, p2), 2, fp(x), 4, *good)  # a lone controller has one plant
    refused(hb, batch, _lib.ERR_INVALID_ARG, "is NULL", arr(p, None), 2, fp(x), 8, *good)
    refused(hb, lone, _lib.ERR_UNSUPPORTED, "mppi_batch_run_episode_plant", arr(p), 1, fp(x), 4, *good)
    refused(h, batch, _lib.ERR_INVALID_ARG, "not a batched handle", arr(p), 1, fp(x), 4, *good)
    sharded = m.Handle(shard_rank=0, shard_count=2, **c)
    refused(h, lone, _lib.ERR_INVALID_ARG, "sharded", arr(sharded), 1, fp(x), 4, *good)
    refused(sharded, lone, _lib.ERR_INVALID_ARG, "sharded handle", arr(p), 1, fp(x), 4, *good)
    other = pm_plant(m, 3)
    refused(h, lone, _lib.ERR_INVALID_ARG, "s_dim", arr(other), 1, fp(x), 4, *good)
    refused(hb, batch, _lib.ERR_INVALID_ARG, "s_dim", arr(p, other), 2, fp(x), 8, *good)
    learned = [m.Handle(**pm_cfg(64, 4, 2, mlp=make_nnauv(5, 16, 1, n_in=6, n_out=4))) for _ in range(2)]
    refused(hb, batch, _lib.ERR_UNSUPPORTED, "per-member learned plants", arr(*learned), 2, fp(x), 8, *good)
    refused(hb, batch, _lib.ERR_UNSUPPORTED, "per-member learned plants", arr(p, learned[0]), 2, fp(x), 8, *good)
    with pytest.raises(ValueError):
        hb.run_episode(np.zeros((2, 4), F32), 2, plant=[p, p2, p])
    with pytest.raises(m.MppiError, match="per-member learned plants"):
        hb.run_episode(np.zeros((2, 4), F32), 2, plant=learned)
    if torch.cuda.device_count() > 1:
        far = pm_plant(m, 2, device=1)
        refused(h, lone, _lib.ERR_INVALID_ARG, "device", arr(far), 1, fp(x), 4, *good)
        far.close()
    close(h, hb, p, p2, sharded, other, *learned)


# ---- examples/learn_loop.py --------------------------------------------------------------------------------------------------------
def test_learn_loop_runs_to_the_end(m, capsys):
    """two rounds at K = 128, H = 8, 8 steps, 3 epochs: finite numbers, and the learner was handed exactly the episodes' rows"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import learn_loop
    finally:
        sys.path.pop(0)
    learner, episodes, figures = learn_loop.main(["--rounds", "2", "--samples", "128", "--horizon", "8", "--steps", "8", "--epochs", "3",
                                                  "--hidden", "16", "--layers", "1"])
    printed = capsys.readouterr().out.strip().splitlines()
    assert len(printed) == 2 and printed[0].startswith("round 1:") and printed[1].startswith("round 2:")
    assert len(figures) == 2 and np.isfinite(np.asarray(figures, np.float64)).all()
    rb = learner.rb_trans()
    X = np.concatenate([e[0][:-1] for e in episodes]).astype(np.float64)
    U = np.concatenate([e[1] for e in episodes]).astype(np.float64)
    Xn = np.concatenate([e[0][1:] for e in episodes]).astype(np.float64)
    assert X.shape == (16, 13) and np.isfinite(X).all() and np.isfinite(U).all()
    np.testing.assert_array_equal(rb["obs"][..., 0], X)
    np.testing.assert_array_equal(rb["act"][..., 0], U)
    np.testing.assert_array_equal(rb["next_obs"][..., 0], Xn)
