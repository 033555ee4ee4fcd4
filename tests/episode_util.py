"""What the closed-loop episode tests share (test_episode_gpu.py): the host loop an episode must equal bit for bit, written with calls that
exist without the episode entry points (set_goal, next, model_next, state_cost, an fp32 add of the disturbance), the comparison of a handle
that ran episodes with one that ran the host loop, and the configurations. A plain module: `m` is the mppi_tf_amd package."""
import numpy as np

F32 = np.float32


def host_loop(h, x0, n_steps, goals=None, disturbance=None):
    """-> (X [n+1, s], U [n, a], C [n]) of the loop set goal, state cost, next, model step, add w"""
    x = np.asarray(x0, F32).copy()
    X, U, Cs = [x], [], []
    for t in range(n_steps):
        if goals is not None:
            h.set_goal(goals[t])
        Cs.append(h.state_cost(x)[0])
        u = h.next(x)
        x = h.model_next(x, u)[0]
        if disturbance is not None:
            x = x + np.asarray(disturbance[t], F32)  # fp32 + fp32, rounded once per component
            assert x.dtype == F32
        X.append(x)
        U.append(u)
    return np.stack(X), np.stack(U), np.asarray(Cs, F32)


def assert_same_state(he, hh, steps, tag=""):
    """the handle that ran episodes (he) is where the host loop left its twin (hh)"""
    np.testing.assert_array_equal(he.get_action_sequence(), hh.get_action_sequence(), err_msg="final sequence " + tag)
    assert he.get_step_counter() == hh.get_step_counter() == steps, tag


def check_lone(make, x0, calls, goals=None, disturbance=None, tag="", before=None):
    """make() twice: one handle runs run_episode once per entry of `calls` (step counts), its twin the host loop of sum(calls) steps; X, U,
    C of every call, the final sequence and the step counter must agree bit for bit. goals / disturbance: [sum(calls), s] or None.
    before(h): run on both handles first. Returns (episode handle, host-loop handle), open."""
    he, hh = make(), make()
    done = 0
    if before is not None:
        done = before(he)
        assert before(hh) == done
    n = sum(calls)
    Xh, Uh, Ch = host_loop(hh, x0, n, goals, disturbance)
    x, t = np.asarray(x0, F32), 0
    for c in calls:
        sl = slice(t, t + c)
        X, U, Cs = he.run_episode(x, c, None if goals is None else goals[sl], None if disturbance is None else disturbance[sl])
        assert X.shape == (c + 1, he.s) and U.shape == (c, he.a) and Cs.shape == (c,)
        msg = "%s steps %d..%d" % (tag, t, t + c)
        np.testing.assert_array_equal(U, Uh[sl], err_msg="U " + msg)
        np.testing.assert_array_equal(X, Xh[t:t + c + 1], err_msg="X " + msg)
        np.testing.assert_array_equal(Cs, Ch[sl], err_msg="C " + msg)
        x, t = X[-1], t + c
    assert_same_state(he, hh, done + n, tag)
    return he, hh


def pm_cfg(K, H, a, **kw):
    s = 2 * a
    goal = np.zeros(s, F32)
    goal[0::2] = [1.0, 0.5, 0.75, -0.5][:a]
    return dict(dict(k=K, tau=H, s_dim=s, a_dim=a, dt=0.1, mass=1.0, lam=1.0, sigma=np.eye(a, dtype=F32) * F32(0.25), goal=goal, Q=np.ones(s, F32), seed=3), **kw)


def pm_x0(a):
    return ((np.arange(2 * a) % 3 - 1) * 0.1).astype(F32)


def signals(n, s, seed, scale=0.05, cols=None):
    """a goal per step (positions move, velocities zero) and a non-zero disturbance per step (on the columns `cols`: default all)"""
    rng = np.random.default_rng(seed)
    G = np.zeros((n, s), F32)
    G[:, 0::2] = rng.uniform(-1, 1, (n, (s + 1) // 2))
    W = np.zeros((n, s), F32)
    cols = list(range(s)) if cols is None else cols
    W[:, cols] = rng.uniform(-scale, scale, (n, len(cols)))
    return G, W


def auv_cfg(K, H, cost, rk=2):
    """Handle / BatchHandle keywords (without goal and seed) of the rexrov2 Fossen model with StaticQuatCost ("quat") or ElipseCost3D"""
    from batch_util import E3, Q10, rexrov2
    from mppi_tf_amd.auv import auv_task
    d = dict(k=K, tau=H, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=auv_task(H)["sigma"], auv=rexrov2(rk))
    if cost == "quat":
        d["Q"], d["quat_cost"] = Q10, True
    else:
        d["ellipse3d"] = E3
    return d


def make_nnauv(seed=0, hid=16, n_hidden=1, n_in=16, n_out=13):
    """NNAUVModel weights as the learned-model tests make them: Dense(hid, relu) x n_hidden + Dense(13), random, with a normalisation
    (n_in = s + a, n_out = s: the learned point-mass model's)"""
    rng = np.random.default_rng(seed)
    dims = [n_in] + [hid] * n_hidden + [n_out]
    W = [(rng.uniform(-1, 1, (dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(F32) for i in range(n_hidden + 1)]
    b = [(rng.uniform(-1, 1, dims[i + 1]) / np.sqrt(dims[i])).astype(F32) for i in range(n_hidden + 1)]
    W[-1] *= 0.1
    b[-1] *= 0.1
    return dict(W=W, b=b, xmean=rng.uniform(-0.1, 0.1, n_in).astype(F32), xstd=rng.uniform(0.8, 1.2, n_in).astype(F32),
                ymean=rng.uniform(-0.01, 0.01, n_out).astype(F32), ystd=rng.uniform(0.8, 1.2, n_out).astype(F32))
