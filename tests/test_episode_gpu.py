"""Closed-loop episodes on the device (mppi_run_episode / mppi_batch_run_episode; Handle.run_episode, BatchHandle.run_episode): n control
steps with the handle's own model as the plant, a goal signal, a disturbance, the realised trajectory logged — no host round trip between
the steps. Needs an MI355X: every test is marked `gpu`.

The contract (include/mppi_c.h): an episode equals, bit for bit, the host loop set_goal, state_cost, next, model_next, fp32 add of w
(episode_util.host_loop) in X, U, C, the final sequence and the step counter; member m of a batched episode equals its lone handle's.
"""
import ctypes as C

import numpy as np
import pytest

from batch_util import auv_members, lone_handles, pm_members
from episode_util import assert_same_state, auv_cfg, check_lone, host_loop, make_nnauv, pm_cfg, pm_x0, signals

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def close(*hs):
    for h in hs:
        h.close()


@pytest.mark.parametrize("a", [2, 3])
def test_point_mass_one_launch_step(m, a):
    """K = 256: the step is one launch (k_step_pc). 5 steps (odd: the two sequence buffers end swapped), then a second call of 2 that
    continues where the first stopped, against a host loop of 7."""
    c = pm_cfg(256, 8, a)
    he, hh = check_lone(lambda: m.Handle(**c), pm_x0(a), [5, 2], tag="a=%d" % a)
    assert he.rollout_kernel_name().startswith("mppi::k_step_pc<")
    close(he, hh)


def test_point_mass_two_launch_step(m):
    """K = 8256 = 129 tiles: above the one-launch step's 128, rollout + finish"""
    c = pm_cfg(8256, 8, 2)
    he, hh = check_lone(lambda: m.Handle(**c), pm_x0(2), [3])
    assert he.rollout_kernel_name().startswith("mppi::k_rollout_pc<")
    close(he, hh)


def _dense_q():
    rng = np.random.default_rng(7)
    L = rng.uniform(-0.3, 0.3, (4, 4)) + np.eye(4)
    return (L @ L.T).astype(F32)


def _with_filter(h):
    h.set_sequence_filter(5, 2)
    return h


def _with_limits(h):
    h.set_action_limits(*LIMITS)
    return h


LIMITS = ([-0.005, -0.002], [0.003, 0.004])  # far inside the update's size at K = 256 (noise of variance 0.25 averaged over 256 samples)


OPTIONS = {
    "filter": lambda m: _with_filter(m.Handle(**pm_cfg(256, 8, 2))),
    "limits": lambda m: _with_limits(m.Handle(**pm_cfg(256, 8, 2))),
    "normalize": lambda m: m.Handle(normalize_cost=True, **pm_cfg(256, 8, 2)),
    "dense_q": lambda m: m.Handle(**pm_cfg(256, 8, 2, Q=_dense_q())),
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_options_behind_the_update(m, opt):
    """the sequence filter (window 5, order 2), action limits tight enough to clip, normalize_cost and a dense Q: whatever the plain step
    runs, the episode's step runs"""
    he, hh = check_lone(lambda: OPTIONS[opt](m), pm_x0(2), [3], tag=opt)
    if opt == "limits":
        U = he.get_action_sequence()
        lo, hi = np.asarray(LIMITS[0], F32), np.asarray(LIMITS[1], F32)
        assert ((U == lo) | (U == hi)).any(), "the limits never clipped"
    close(he, hh)


@pytest.mark.parametrize("which", ["both", "goals", "disturbance"])
def test_goal_signal_and_disturbance(m, which):
    """a different goal row per step, a non-zero disturbance; afterwards the goal in force is the last row: one more plain step agrees"""
    c, n = pm_cfg(256, 8, 2), 4
    G, W = signals(n, 4, seed=5)
    assert len({tuple(g) for g in G}) == n and np.all(W != 0)
    goals, dist = (G if which != "disturbance" else None), (W if which != "goals" else None)
    he, hh = check_lone(lambda: m.Handle(**c), pm_x0(2), [3, 1], goals, dist, tag=which)
    x = np.array([0.3, -0.1, 0.2, 0.05], F32)
    np.testing.assert_array_equal(he.state_cost(x), hh.state_cost(x))
    np.testing.assert_array_equal(he.next(x), hh.next(x), err_msg="the step after the episode (goal = the last row)")
    np.testing.assert_array_equal(he.get_action_sequence(), hh.get_action_sequence())
    hh.set_goal(c["goal"])
    he.set_goal(c["goal"])  # the host mirror went with the device's goal: a later upload of the constants changes nothing else
    np.testing.assert_array_equal(he.next(x), hh.next(x))
    close(he, hh)


def test_fossen_auv(m):
    """rk2 Fossen model, StaticQuatCost; the disturbance on the velocity entries only (the quaternion stays the model's)"""
    c, n = auv_cfg(128, 6, "quat"), 3
    X0, G, U0 = auv_members(1, 6)
    _, W = signals(n, 13, seed=9, scale=0.02, cols=list(range(7, 13)))

    def make():
        h = m.Handle(goal=G[0], seed=4, **c)
        h.set_action_sequence(U0[0])
        return h
    he, hh = check_lone(make, X0[0], [n], None, W, tag="auv")
    assert he.rollout_kernel_name().startswith("mppi::k_rollout_auv_pc<")
    close(he, hh)


def test_learned_model(m):
    """NNAUVModel, one Dense(16) hidden layer, random weights: the plant is the model's reference evaluation (mppi_model_step's)"""
    mlp = make_nnauv(3, 16, 1)
    X0, G, _ = auv_members(1, 4, seed=2)
    c = dict(k=64, tau=4, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=np.eye(6, dtype=F32), goal=G[0], Q=np.ones(13, F32), nnauv=mlp, seed=9)
    Gs = np.repeat(G, 2, axis=0)
    Gs[1, :3] += F32(0.5)
    he, hh = check_lone(lambda: m.Handle(**c), X0[0], [2], Gs, None, tag="nnauv")
    close(he, hh)


def test_learned_point_mass_model(m):
    """the learned model in the point mass's shape (s = 4, a = 2, one Dense(16) hidden layer): the other model-step kernel behind
    mppi_model_step, with a goal signal and a disturbance"""
    mlp = make_nnauv(5, 16, 1, n_in=6, n_out=4)
    c = pm_cfg(64, 4, 2, mlp=mlp)
    G, W = signals(2, 4, seed=8)
    he, hh = check_lone(lambda: m.Handle(**c), pm_x0(2), [2], G, W, tag="mlp")
    close(he, hh)


def test_profiling_sees_the_episodes_steps(m):
    """mppi_profile_begin / _end count an episode's steps as they count any step: one-launch, two-launch and batched"""
    lone1, lone2 = m.Handle(**pm_cfg(256, 8, 2)), m.Handle(**pm_cfg(8256, 8, 2))
    hb = m.BatchHandle(n=2, **pm_cfg(256, 8, 2))
    for h, x0 in ((lone1, pm_x0(2)), (lone2, pm_x0(2)), (hb, np.stack([pm_x0(2)] * 2))):
        h.profile_begin(8)
        h.run_episode(x0, 3)
        rollout_ms, _, n = h.profile_end()
        assert n == 3 and rollout_ms > 0.0
    close(lone1, lone2, hb)


def test_prelaunch_tuning_never_prelaunches_an_episode(m):
    """x of step t + 1 depends on u of step t: a handle with MPPI_TUNE_PRELAUNCH drains its two streams and runs the plain step. After a few
    pre-launched next_device calls the episode equals the host loop of a handle without the tuning."""
    import torch
    c = pm_cfg(256, 8, 2)
    x0 = pm_x0(2)

    def before(h):
        xd, ud = torch.tensor(x0, device="cuda"), torch.zeros(2, device="cuda")
        torch.cuda.synchronize()
        for _ in range(3):
            h.next_device(xd.data_ptr(), ud.data_ptr(), None)
        h.synchronize()
        return 3
    made = []

    def make():  # the first handle (the episode's) carries the tuning, its host-loop twin does not
        made.append(m.Handle(tuning={"prelaunch": 1} if not made else None, **c))
        return made[-1]
    he, hh = check_lone(make, x0, [3], before=before, tag="prelaunch")
    close(he, hh)


def _batch_pm(m, B, n):
    shared = dict(k=256, tau=16, s_dim=4, a_dim=2, dt=0.1, mass=1.0, Q=np.ones(4, F32))
    lams = [0.5, 1.0, 2.0][:B]
    sigmas = [np.eye(2, dtype=F32) * F32(v) for v in (0.1, 0.25, 0.4)][:B]
    seeds = [11 + 7 * i for i in range(B)]
    X0, G, U0 = pm_members(B, 2, 16)
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, lams=lams, sigmas=sigmas, **shared)
    hb.set_action_sequences(U0)
    hs = lone_handles(m, [dict(shared, lam=lams[i], sigma=sigmas[i]) for i in range(B)], seeds, G, U0, "mppi::k_step_pc<")
    rng = np.random.default_rng(21)
    goals = np.zeros((n, B, 4), F32)
    goals[:, :, 0::2] = rng.uniform(-1, 1, (n, B, 2))
    dist = rng.uniform(-0.05, 0.05, (n, B, 4)).astype(F32)
    return hb, hs, X0, goals, dist


def _assert_members(hb, hs, X0, n, goals, dist, tag):
    X, U, Cs = hb.run_episode(X0, n, goals, dist)
    B = len(hs)
    assert X.shape == (n + 1, B, hb.s) and U.shape == (n, B, hb.a) and Cs.shape == (n, B)
    Ub = hb.get_action_sequences()
    for i, h in enumerate(hs):
        Xi, Ui, Ci = h.run_episode(X0[i], n, None if goals is None else goals[:, i], None if dist is None else dist[:, i])
        msg = "member %d %s" % (i, tag)
        np.testing.assert_array_equal(U[:, i], Ui, err_msg="U " + msg)
        np.testing.assert_array_equal(X[:, i], Xi, err_msg="X " + msg)
        np.testing.assert_array_equal(Cs[:, i], Ci, err_msg="C " + msg)
        np.testing.assert_array_equal(Ub[i], h.get_action_sequence(), err_msg="sequence " + msg)
        assert h.get_step_counter() == hb.get_step_counter()
    return X


@pytest.mark.parametrize("B", [3, 1])
def test_batched_point_mass(m, B):
    """per-member lambda, Sigma, goal, seed, goal signal and disturbance: member m's X, U, C and final sequence are its lone handle's
    episode's; a second episode continues the first; member 0 against the host loop as well"""
    n = 3
    hb, hs, X0, goals, dist = _batch_pm(m, B, 2 * n)
    X = _assert_members(hb, hs, X0, n, goals[:n], dist[:n], "first")
    _assert_members(hb, hs, X[-1], n, goals[n:], dist[n:], "second")
    assert hb.get_step_counter() == 2 * n
    for h in hs:
        h.close()
    hb.close()
    # the lone episode is itself the host loop (the tests above), so the batch is; one direct check keeps that chain honest
    hb, hs, X0, goals, dist = _batch_pm(m, B, n)
    Xb, Ub, Cb = hb.run_episode(X0, n, goals, dist)
    Xh, Uh, Ch = host_loop(hs[0], X0[0], n, goals[:, 0], dist[:, 0])
    np.testing.assert_array_equal(Xb[:, 0], Xh)
    np.testing.assert_array_equal(Ub[:, 0], Uh)
    np.testing.assert_array_equal(Cb[:, 0], Ch)
    for h in hs:
        h.close()
    hb.close()


def test_batched_more_members_than_one_workgroup(m):
    """B = 70 members: the episode kernel runs two workgroups of 64 lanes, the second ragged. a = 3, the Python action-cost form with
    upsilon scaling the noise and per-member lambda (examples/sweep.py's kind of grid), against the host loop of batched steps:
    hb.next, then the model step and the state cost of all members at once through one lone handle (the model and the goal are shared)."""
    B, n, a = 70, 3, 3
    c = pm_cfg(64, 8, a, action_cost=m.ACTION_COST_PY, upsilon_scales_noise=True, gamma=0.1, upsilon=1.4)
    del c["lam"], c["seed"]
    lams = list(np.linspace(0.05, 0.5, B))
    rng = np.random.default_rng(33)
    X0 = rng.uniform(-1, 1, (B, 2 * a)).astype(F32)
    G, _ = signals(n, 2 * a, seed=12)
    dist = rng.uniform(-0.05, 0.05, (n, B, 2 * a)).astype(F32)
    goals = np.repeat(G[:, None, :], B, axis=1)
    he, hh = (m.BatchHandle(n=B, lams=lams, seeds=range(50, 50 + B), **c) for _ in range(2))
    h1 = m.Handle(lam=1.0, **c)
    Xe, Ue, Ce = he.run_episode(X0, n, goals, dist)
    X = X0
    for t in range(n):
        hh.set_goals(goals[t])
        h1.set_goal(G[t])
        np.testing.assert_array_equal(Ce[t], h1.state_cost(X), err_msg="C step %d" % t)
        U = hh.next(X)
        np.testing.assert_array_equal(Ue[t], U, err_msg="U step %d" % t)
        X = h1.model_next(X, U) + dist[t]
        np.testing.assert_array_equal(Xe[t + 1], X, err_msg="X step %d" % t)
    np.testing.assert_array_equal(he.get_action_sequences(), hh.get_action_sequences())
    assert he.get_step_counter() == hh.get_step_counter() == n
    np.testing.assert_array_equal(he.next(X), hh.next(X), err_msg="the goals after the episode are the last rows")
    close(he, hh, h1)


def test_batched_auv(m):
    """B = 2 Fossen AUV controllers with ElipseCost3D against their lone handles"""
    B, n = 2, 3
    c = auv_cfg(128, 6, "ellipse3d")
    X0, G, U0 = auv_members(B, 6, seed=3)
    seeds = [5, 18]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hb.set_action_sequences(U0)
    hs = lone_handles(m, [c] * B, seeds, G, U0, "mppi::k_rollout_auv_pc<")
    dist = np.zeros((n, B, 13), F32)
    dist[:, :, 7:] = np.random.default_rng(4).uniform(-0.02, 0.02, (n, B, 6))
    _assert_members(hb, hs, X0, n, None, dist, "auv")
    for h in hs:
        h.close()
    hb.close()


def test_refusals(m):
    """every refusal: its status, a message naming the cause, and nothing enqueued (the step counter stands)"""
    from mppi_tf_amd import _lib
    lib = _lib.load()
    c = pm_cfg(256, 8, 2)
    x = np.zeros(8, F32)
    out = np.zeros(64, F32)
    fp = _lib.fp

    def refused(h, fn, status, word, *args):
        st = fn(h.h, *args)
        assert st == status, (fn.__name__, st, lib.mppi_last_error(h.h))
        assert word in lib.mppi_last_error(h.h).decode(), lib.mppi_last_error(h.h)
        assert h.get_step_counter() == 0

    h = m.Handle(**c)
    hb = m.BatchHandle(n=2, **{k: v for k, v in c.items() if k != "seed"})
    good = (2, None, None, fp(out), None, None)
    refused(hb, lib.mppi_run_episode, _lib.ERR_UNSUPPORTED, "mppi_batch_run_episode", fp(x), 4, *good)
    refused(h, lib.mppi_batch_run_episode, _lib.ERR_INVALID_ARG, "not a batched handle", fp(x), 4, *good)
    for hh, fn, nx in ((h, lib.mppi_run_episode, 4), (hb, lib.mppi_batch_run_episode, 8)):
        refused(hh, fn, _lib.ERR_INVALID_ARG, "n_steps", fp(x), nx, 0, None, None, fp(out), None, None)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "n_steps", fp(x), nx, -3, None, None, fp(out), None, None)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "x0", fp(x), nx - 1, *good)
        refused(hh, fn, _lib.ERR_INVALID_ARG, "x0", None, nx, *good)
    hs = m.Handle(shard_rank=0, shard_count=2, **c)
    assert lib.mppi_next_device(hs.h, C.c_void_p(8), C.c_void_p(8), None) == _lib.ERR_INVALID_ARG  # (refused before the pointers are looked at)
    as_next_device = lib.mppi_last_error(hs.h).decode()
    refused(hs, lib.mppi_run_episode, _lib.ERR_INVALID_ARG, "sharded handle", fp(x), 4, *good)
    assert lib.mppi_last_error(hs.h).decode() == as_next_device
    with pytest.raises(ValueError):
        h.run_episode(np.zeros(5, F32), 2)
    close(h, hb, hs)
