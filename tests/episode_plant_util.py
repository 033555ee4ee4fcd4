"""What the tests of the closed-loop episode against a separate plant share (test_episode_plant_gpu.py), on top of episode_util.py: the
host loop such an episode must equal bit for bit, written with calls that exist without the plant entry points (set_goal, state_cost and
next on the controller, model_next on the PLANT handle, an fp32 add of the disturbance), the lone comparison, and the plants. A plain
module: `m` is the mppi_tf_amd package."""
import numpy as np

from episode_util import assert_same_state, pm_cfg

F32 = np.float32


def host_loop_plant(h, plant, x0, n_steps, goals=None, disturbance=None):
    """-> (X [n+1, s], U [n, a], C [n]) of the loop set goal, state cost, next (the controller h), model step (the plant), add w"""
    x = np.asarray(x0, F32).copy()
    X, U, Cs = [x], [], []
    for t in range(n_steps):
        if goals is not None:
            h.set_goal(goals[t])
        Cs.append(h.state_cost(x)[0])
        u = h.next(x)
        x = plant.model_next(x, u)[0]
        if disturbance is not None:
            x = x + np.asarray(disturbance[t], F32)  # fp32 + fp32, rounded once per component
            assert x.dtype == F32
        X.append(x)
        U.append(u)
    return np.stack(X), np.stack(U), np.asarray(Cs, F32)


def plant_state(p, x_probe):
    """what of a plant a call must leave alone: its sequence, its step counter and its goal (seen through the state cost of a probe)"""
    return p.get_action_sequence(), p.get_step_counter(), p.state_cost(x_probe)


def assert_plant_untouched(p, before, x_probe, tag=""):
    U, step, cost = plant_state(p, x_probe)
    np.testing.assert_array_equal(U, before[0], err_msg="the plant's sequence " + tag)
    assert step == before[1], "the plant's step counter " + tag
    np.testing.assert_array_equal(cost, before[2], err_msg="the plant's goal " + tag)


def check_lone_plant(make, make_plant, x0, calls, goals, disturbance, tag="", between=None):
    """make() twice, make_plant() twice: one controller runs run_episode(plant=) once per entry of `calls` (step counts), its twin the
    host loop of sum(calls) steps against the second plant; X, U, C of every call, the controller's final sequence and step counter
    must agree bit for bit, and the episode's plant must be left as it was. between(plant): run on both plants between the first call
    and the rest (new weights). Returns (the episode's X [sum(calls)+1, s], the four handles: controllers, plants), open."""
    he, hh = make(), make()
    pe, ph = make_plant(), make_plant()
    probe = np.asarray(x0, F32)
    x, t, Xs = np.asarray(x0, F32), 0, [np.asarray(x0, F32)[None]]
    for i, c in enumerate(calls):
        if i == 1 and between is not None:
            between(pe)
            between(ph)
        sl = slice(t, t + c)
        g, w = None if goals is None else goals[sl], None if disturbance is None else disturbance[sl]
        Xh, Uh, Ch = host_loop_plant(hh, ph, x, c, g, w)
        before = plant_state(pe, probe)
        X, U, Cs = he.run_episode(x, c, g, w, plant=pe)
        assert X.shape == (c + 1, he.s) and U.shape == (c, he.a) and Cs.shape == (c,)
        msg = "%s steps %d..%d" % (tag, t, t + c)
        np.testing.assert_array_equal(U, Uh, err_msg="U " + msg)
        np.testing.assert_array_equal(X, Xh, err_msg="X " + msg)
        np.testing.assert_array_equal(Cs, Ch, err_msg="C " + msg)
        assert_plant_untouched(pe, before, probe, msg)
        x, t = X[-1], t + c
        Xs.append(X[1:])
    assert_same_state(he, hh, sum(calls), tag)
    return np.concatenate(Xs), (he, hh, pe, ph)


def pm_plant(m, a, mass=1.5, dt=0.05, **kw):
    """a point-mass plant: a handle that runs no rollouts (k = 1, tau = 1), only its mass and dt matter"""
    return m.Handle(**dict(k=1, tau=1, s_dim=2 * a, a_dim=a, dt=dt, mass=mass), **kw)


def pm_rollout_plant(m, a, mass=1.5, dt=0.05):
    """a point-mass plant that is a controller in its own right: a sequence, a step counter and a goal of its own to leave alone"""
    p = m.Handle(**pm_cfg(64, 4, a, mass=mass, dt=dt, seed=17))
    p.set_action_sequence(np.linspace(-0.3, 0.4, 4 * a, dtype=F32).reshape(4, a))
    p.next(np.full(2 * a, 0.2, F32))
    return p


def auv_plant(m, auv):
    """a Fossen plant: a handle that runs no rollouts with the parameters dict `auv`"""
    return m.Handle(k=1, tau=1, s_dim=13, a_dim=6, dt=0.1, sigma=np.eye(6, dtype=F32), goal=np.zeros(13, F32), auv=auv)


def heavier(auv, mass=1.25, quad=1.4):
    """the parameters of a vehicle `mass` times heavier with `quad` times the quadratic damping"""
    d = dict(auv)
    d["mass"] = float(auv["mass"]) * mass
    d["quad_damping"] = (np.asarray(auv["quad_damping"], np.float64) * quad).tolist()
    return d
