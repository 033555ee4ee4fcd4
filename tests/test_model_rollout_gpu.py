"""Open-loop model rollouts on the device (mppi_model_rollout / mppi_model_rollout_device; Handle.model_rollout, model_rollout_device,
sample_trajectories; ControllerBase.predict_trajectories). Needs an MI355X: every test is marked `gpu`.

The contract (include/mppi_c.h): X and C of one call equal, bit for bit, the host loop of T model_next and state_cost calls
(model_rollout_util.host_rollout), both pinned to the golden vectors and the oracle elsewhere; the handle is left as it was. Every
comparison is assert_array_equal: there are no tolerances in this file."""
import ctypes

import numpy as np
import pytest

from model_rollout_util import (F32, auv_inputs, auv_kw, check_rollout, host_rollout, learned_inputs, learned_kw, pm_inputs, pm_kw,
                                readout_case, rollout_cost_from)

pytestmark = pytest.mark.gpu
NS, TS = (1, 64, 65), (1, 3)  # 65: one lane in a second workgroup


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def _fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _pm_matrix(h, a, seed):
    for n in NS:
        for T in TS:
            x0, V = pm_inputs(a, n, T, seed)
            check_rollout(h, x0, V, "n=%d T=%d kx=n" % (n, T))
            X, _ = check_rollout(h, x0[0], V, "n=%d T=%d kx=1" % (n, T))
            np.testing.assert_array_equal(X[0], np.broadcast_to(x0[0], (n, 2 * a)))


# ---- the analytic models ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", ["diag", "dense"])
@pytest.mark.parametrize("a", [1, 2, 3, 4])
def test_point_mass(m, a, q):
    """every a, diagonal and dense Q, n in {1, 64, 65}, T in {1, 3}, one start for all and one each"""
    h = m.Handle(**pm_kw(a, q))
    _pm_matrix(h, a, seed=a)
    h.close()


def test_point_mass_ellipse_cost(m):
    h = m.Handle(**pm_kw(2, "ellipse"))
    _pm_matrix(h, 2, seed=9)
    h.close()


@pytest.mark.parametrize("cost", ["quad", "quat", "e3"])
@pytest.mark.parametrize("rk", [1, 2, 4])
def test_fossen(m, rk, cost):
    h = m.Handle(**auv_kw(cost, rk))
    for n, T in ((1, 1), (65, 3)):
        x0, V = auv_inputs(n, T, seed=rk)
        X, Cs = check_rollout(h, x0, V, "n=%d T=%d kx=n" % (n, T))
        check_rollout(h, x0[0], V, "n=%d T=%d kx=1" % (n, T))
        assert not np.array_equal(X[1], X[0]) and (Cs > 0).all()
    h.close()


# ---- the learned models: the reference-ordered step kernels, row to row ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mlp", "nnauv", "nnauv_speed"])
def test_learned(m, kind):
    h = m.Handle(**learned_kw(kind))
    for n in (5, 65):
        x0, V = learned_inputs(kind, n, 3, seed=4)
        X, _ = check_rollout(h, x0, V, "%s n=%d kx=n" % (kind, n))
        check_rollout(h, x0[0], V, "%s n=%d kx=1" % (kind, n))
        assert not np.array_equal(X[2], X[1])
    h.close()


# ---- T is not tau ------------------------------------------------------------------------------------------------------------------------
def test_T_is_free_of_tau(m):
    h = m.Handle(**pm_kw(2, K=64, H=4))
    x0, V = pm_inputs(2, 3, 9, seed=1)
    check_rollout(h, x0, V, "tau=4 T=9")
    h.close()
    # plants: handles that run no rollouts
    p = m.Handle(k=1, tau=1, s_dim=6, a_dim=3, dt=0.05, mass=1.5)
    x0, V = pm_inputs(3, 7, 5, seed=2)
    check_rollout(p, x0, V, "plant T=5")
    p.close()
    from batch_util import rexrov2
    p = m.Handle(k=1, tau=1, s_dim=13, a_dim=6, dt=0.1, sigma=np.eye(6, dtype=F32), goal=np.zeros(13, F32), auv=rexrov2(2))
    x0, V = auv_inputs(7, 5, seed=2)
    check_rollout(p, x0, V, "Fossen plant T=5")
    p.close()


def test_one_sequence_form(m):
    """V [T, a] -> X [T+1, s], C [T]: trajectory 0 of the n = 1 form"""
    h = m.Handle(**pm_kw(2))
    x0, V = pm_inputs(2, 1, 3, seed=5)
    X, Cs = h.model_rollout(x0[0], V[:, 0])
    Xh, Ch = host_rollout(h, x0, V)
    assert X.shape == (4, 4) and Cs.shape == (3,)
    np.testing.assert_array_equal(X, Xh[:, 0])
    np.testing.assert_array_equal(Cs, Ch[:, 0])
    h.close()


# ---- optional outputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pm", "auv", "mlp"])
def test_optional_outputs(m, kind):
    h = m.Handle(**(pm_kw(2, "dense") if kind == "pm" else auv_kw("quat", 2) if kind == "auv" else learned_kw("mlp")))
    n, T = 65, 3
    x0, V = auv_inputs(n, T, seed=6) if kind == "auv" else pm_inputs(2, n, T, seed=6)
    X, Cs = h.model_rollout(x0, V)
    X2, none = h.model_rollout(x0, V, costs=False)
    assert none is None
    np.testing.assert_array_equal(X2, X)
    lib = m.load()
    # C only, and both: outputs pre-filled with NaN, every entry written
    Cn = np.full((T, n), np.nan, F32)
    assert lib.mppi_model_rollout(h.h, _fp(x0), n, _fp(V), n, T, None, _fp(Cn)) == 0
    np.testing.assert_array_equal(Cn, Cs)
    Xn, Cn = np.full((T + 1, n, h.s), np.nan, F32), np.full((T, n), np.nan, F32)
    assert lib.mppi_model_rollout(h.h, _fp(x0), n, _fp(V), n, T, _fp(Xn), _fp(Cn)) == 0
    assert not np.isnan(Xn).any() and not np.isnan(Cn).any()
    np.testing.assert_array_equal(Xn, X)
    np.testing.assert_array_equal(Cn, Cs)
    Xn = np.full((T + 1, n, h.s), np.nan, F32)
    assert lib.mppi_model_rollout(h.h, _fp(x0), n, _fp(V), n, T, _fp(Xn), None) == 0
    np.testing.assert_array_equal(Xn, X)
    h.close()


# ---- the handle is left as it was ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pm", "auv", "mlp"])
def test_handle_untouched(m, kind):
    kw = pm_kw(2, K=200, H=6) if kind == "pm" else auv_kw("quat", 2) if kind == "auv" else learned_kw("mlp")
    h, twin = m.Handle(**kw), m.Handle(**kw)
    x = (auv_inputs(1, 1)[0] if kind == "auv" else pm_inputs(2, 1, 1)[0])[0]
    U0 = np.random.default_rng(3).uniform(-0.3, 0.3, (h.tau, h.a)).astype(F32)
    for g in (h, twin):
        g.set_action_sequence(U0)
        g.next(x)
    probe = x + F32(0.125)
    before = h.get_action_sequence(), h.get_step_counter(), h.state_cost(probe)
    x0, V = auv_inputs(65, 5, seed=8) if kind == "auv" else pm_inputs(2, 65, 5, seed=8)
    h.model_rollout(x0, V)
    h.model_rollout(x0[0], V, costs=False)
    np.testing.assert_array_equal(h.get_action_sequence(), before[0])
    assert h.get_step_counter() == before[1] == twin.get_step_counter()
    np.testing.assert_array_equal(h.state_cost(probe), before[2])
    for _ in range(2):
        np.testing.assert_array_equal(h.next(x), twin.next(x))
    np.testing.assert_array_equal(h.get_action_sequence(), twin.get_action_sequence())
    np.testing.assert_array_equal(h.debug_get(m.DBG_COSTS), twin.debug_get(m.DBG_COSTS))
    h.close()
    twin.close()


# ---- the device entry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pm", "auv", "mlp", "nnauv"])
def test_device_entry(m, kind):
    import torch
    kw = pm_kw(2) if kind == "pm" else auv_kw("e3", 2) if kind == "auv" else learned_kw(kind)
    h = m.Handle(**kw)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    # the second and third calls take more rows than the first: a learned handle's scratch regrows, once per stream it is used on
    for n, T, st, kx1 in ((5, 3, None, False), (65, 3, stream, False), (130, 2, None, True), (65, 3, stream, True)):
        x0, V = (pm_inputs(2, n, T, seed=n) if kind in ("pm", "mlp") else auv_inputs(n, T, seed=n, force=100.0 if kind == "auv" else 1.0))
        if kx1:
            x0 = x0[:1]
        Xh, Ch = h.model_rollout(x0, V)
        dx, dV = torch.from_numpy(x0).to(dev), torch.from_numpy(V).to(dev)
        dX = torch.full((T + 1, n, h.s), float("nan"), dtype=torch.float32, device=dev)
        dC = torch.full((T, n), float("nan"), dtype=torch.float32, device=dev)
        dX2 = torch.full((T + 1, n, h.s), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        h.model_rollout_device(dx.data_ptr(), x0.shape[0], dV.data_ptr(), n, T, dX.data_ptr(), dC.data_ptr(), stream=st)
        h.model_rollout_device(dx.data_ptr(), x0.shape[0], dV.data_ptr(), n, T, dX2.data_ptr(), 0, stream=st)
        if st is None:
            h.synchronize()
        else:
            st.synchronize()
        tag = "%s n=%d stream=%s" % (kind, n, "own" if st is None else "torch")
        np.testing.assert_array_equal(dX.cpu().numpy(), Xh, err_msg="X " + tag)
        np.testing.assert_array_equal(dC.cpu().numpy(), Ch, err_msg="C " + tag)
        np.testing.assert_array_equal(dX2.cpu().numpy(), Xh, err_msg="X without C " + tag)
    h.close()


# ---- the readout: what the controller planned -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pm", "auv"])
def test_readout_needle(m, name):
    """One control step; the trajectories of chosen samples are read out, and each sample's rollout cost is rebuilt from the state costs
    of ITS trajectory, the action costs of ITS noise and the fp32 recurrence of the rollouts (test_model_rollout_oracle.py proves the
    identity on the CPU). It must equal the cost the step computed for that sample bit for bit: a trajectory of the wrong sample, step or
    row moves it by O(sigma)."""
    case = readout_case(name)
    h = m.Handle(**case["handle"])
    h.set_action_sequence(case["U"])
    U_before = h.get_action_sequence()
    np.testing.assert_array_equal(U_before, case["U"])
    h.next(case["x"])
    costs = h.debug_get(m.DBG_COSTS)
    ks = list(dict.fromkeys(case["ks"] + [int(np.argmin(costs))]))  # 0, 63, 64 (K = 128), K - 1, the best sample
    X, Cs, eps = h.sample_trajectories(case["x"], U_before, ks)
    H, s, a = case["H"], case["s"], case["a"]
    assert X.shape == (H + 1, len(ks), s) and Cs.shape == (H, len(ks)) and eps.shape == (len(ks), H, a)
    np.testing.assert_array_equal(eps, h.debug_get(m.DBG_NOISE)[ks])
    np.testing.assert_array_equal(X[0], np.broadcast_to(case["x"], (len(ks), s)))
    rebuilt = []
    for j, k in enumerate(ks):
        ac = np.asarray([h.action_cost(U_before[t], eps[j, t])[0] for t in range(H)], F32)
        rebuilt.append(rollout_cost_from(Cs[:, j], ac))
    print("readout %s: ks %s rebuilt %s costs %s" % (name, ks, rebuilt, costs[ks]))
    np.testing.assert_array_equal(np.asarray(rebuilt, F32), costs[ks])
    # ... and the identity discriminates: the state costs of the neighbouring column do not rebuild a sample's cost
    ac0 = np.asarray([h.action_cost(U_before[t], eps[0, t])[0] for t in range(H)], F32)
    assert rollout_cost_from(Cs[:, 1], ac0) != costs[ks[0]]
    h.close()


# ---- ControllerBase.predict_trajectories ------------------------------------------------------------------------------------------------
def test_predict_trajectories(m):
    s, a, H = 4, 2, 6
    sigma = np.eye(a) * 0.5
    goal = np.asarray([1.0, 0.0, 0.5, 0.0])[:, None]
    model = m.PointMassModel(1.25, 0.1, s, a)
    cost = m.StaticCost(1.0, 1.0, 1.0, sigma, goal, np.diag([1.0, 0.5, 2.0, 0.25]))
    ctl = m.ControllerBase(model=model, cost=cost, k=64, tau=H, sDim=s, aDim=a, lam=1.0, sigma=sigma, seed=3)
    x = np.asarray([0.2, -0.1, -0.3, 0.15], F32)
    ctl.next(x[:, None])
    traj1, cost1 = ctl.predict_trajectory(x[:, None])
    traj, c = ctl.predict_trajectories(x[:, None])
    assert traj.shape == (H, s) and np.abs(traj1).max() > 0
    np.testing.assert_array_equal(traj, traj1)
    assert c == cost1
    seqs = np.random.default_rng(5).uniform(-1, 1, (3, H, a)).astype(F32)
    trajs, cs = ctl.predict_trajectories(x, seqs)
    assert trajs.shape == (H, 3, s) and cs.shape == (3,)
    for i in range(3):
        ti, ci = ctl.predict_trajectory(x, seqs[i])
        np.testing.assert_array_equal(trajs[:, i], ti)
        assert cs[i] == ci
        tj, cj = ctl.predict_trajectories(x, seqs[i])
        np.testing.assert_array_equal(tj, ti)
        assert cj == ci
    np.testing.assert_array_equal(ctl.predict_trajectories(x, seqs[..., None])[0], trajs)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(m):
    from mppi_tf_amd import _lib
    lib = m.load()
    kw = pm_kw(2, K=200, H=6)
    h, twin = m.Handle(**kw), m.Handle(**kw)
    n, T = 5, 3
    x0, V = pm_inputs(2, n, T)
    X, Cs = np.zeros((T + 1, n, 4), F32), np.zeros((T, n), F32)
    x = x0[0]
    for g in (h, twin):
        g.next(x)
    bad = ((_fp(x0), n, _fp(V), 0, T, _fp(X), _fp(Cs)), (_fp(x0), n, _fp(V), -1, T, _fp(X), _fp(Cs)), (_fp(x0), n, _fp(V), n, 0, _fp(X), _fp(Cs)),
           (_fp(x0), 2, _fp(V), n, T, _fp(X), _fp(Cs)), (_fp(x0), 0, _fp(V), n, T, _fp(X), _fp(Cs)), (None, n, _fp(V), n, T, _fp(X), _fp(Cs)),
           (_fp(x0), n, None, n, T, _fp(X), _fp(Cs)), (_fp(x0), n, _fp(V), n, T, None, None))
    for args in bad:
        assert lib.mppi_model_rollout(h.h, *args) == _lib.ERR_INVALID_ARG, args[1:5]
        assert b"mppi_model_rollout" in lib.mppi_last_error(h.h)
    # the device entry: the same refusals, and X_dev is required (p: a device buffer that would hold every argument of the good call)
    import torch
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    for args in ((p, n, p, 0, T, p, p), (p, n, p, n, 0, p, p), (p, 2, p, n, T, p, p), (None, n, p, n, T, p, p), (p, n, None, n, T, p, p),
                 (p, n, p, n, T, None, p)):
        assert lib.mppi_model_rollout_device(h.h, *args, None) == _lib.ERR_INVALID_ARG, args[1:5]
    with pytest.raises(m.MppiError) as e:
        h.model_rollout_device(p, n, p, n, T, 0)
    assert e.value.status == _lib.ERR_INVALID_ARG
    # a batched handle; a point mass with a_dim > 4
    hb = m.BatchHandle(n=2, **pm_kw(2, K=128, H=4))
    assert lib.mppi_model_rollout(hb.h, _fp(x0), n, _fp(V), n, T, _fp(X), _fp(Cs)) == _lib.ERR_UNSUPPORTED
    assert lib.mppi_model_rollout_device(hb.h, p, n, p, n, T, p, p, None) == _lib.ERR_UNSUPPORTED
    with pytest.raises(m.MppiError) as e:
        hb.model_rollout(x0, V)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    hb.close()
    h5 = m.Handle(k=1, tau=1, s_dim=10, a_dim=5)
    x5, V5 = np.zeros((1, 10), F32), np.zeros((T, 1, 5), F32)
    with pytest.raises(m.MppiError) as e:
        h5.model_rollout(x5, V5)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    h5.close()
    assert lib.mppi_model_rollout(None, _fp(x0), n, _fp(V), n, T, _fp(X), _fp(Cs)) == _lib.ERR_INVALID_ARG
    # afterwards the handle still steps, and its next control equals its twin's
    np.testing.assert_array_equal(h.next(x), twin.next(x))
    np.testing.assert_array_equal(h.get_action_sequence(), twin.get_action_sequence())
    check_rollout(h, x0, V, "after the refusals")
    h.close()
    twin.close()
