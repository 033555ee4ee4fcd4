"""What the open-loop rollout tests share (test_model_rollout_oracle.py on the CPU, test_model_rollout_gpu.py on the GPU): the host loop
a rollout must equal bit for bit, written with calls that exist without the rollout entry points (model_next and state_cost, one call per
step), the inputs, the handle configurations, the two readout cases on both sides (handle keywords and oracle problem) and the fp32
recurrence that rebuilds a sample's rollout cost from its state costs. A plain module: `m` is the mppi_tf_amd package."""
import numpy as np

F32 = np.float32
ELLIPSE2D = dict(a=2.0, b=1.5, cx=0.25, cy=-0.5, speed=1.0, m_state=5.0, m_vel=2.0)


# ---- the reference: T host round trips ---------------------------------------------------------------------------------------------
def host_rollout(h, x0, V):
    """x0 [s] or [n, s], V [T, n, a] -> (X [T+1, n, s], C [T, n]) of the loop model_next, state_cost (mppi_model_step / mppi_state_cost)"""
    V = np.asarray(V, F32)
    T, n, _ = V.shape
    x = np.broadcast_to(np.asarray(x0, F32).reshape(-1, h.s), (n, h.s)).copy()
    X, Cs = [x], []
    for t in range(T):
        x = h.model_next(x, V[t])
        X.append(x)
        Cs.append(h.state_cost(x))
    return np.stack(X), np.stack(Cs)


def check_rollout(h, x0, V, tag=""):
    """model_rollout against the host loop, bit for bit; -> (X, C)"""
    Xh, Ch = host_rollout(h, x0, V)
    X, Cs = h.model_rollout(x0, V)
    assert X.shape == Xh.shape and Cs.shape == Ch.shape, tag
    assert np.isfinite(Xh).all() and np.isfinite(Ch).all(), "the reference is not finite " + tag
    np.testing.assert_array_equal(X, Xh, err_msg="X " + tag)
    np.testing.assert_array_equal(Cs, Ch, err_msg="C " + tag)
    return X, Cs


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def pm_inputs(a, n, T, seed=0):
    """-> (x0 [n, 2a], V [T, n, a]): distinct starts and actions per trajectory and step"""
    rng = np.random.default_rng(1000 + 17 * seed + n + 7 * T)
    return rng.uniform(-1, 1, (n, 2 * a)).astype(F32), rng.uniform(-2, 2, (T, n, a)).astype(F32)


def auv_inputs(n, T, seed=0, force=100.0):
    """-> (x0 [n, 13] with unit quaternions, V [T, n, 6] forces and torques)"""
    rng = np.random.default_rng(2000 + 17 * seed + n + 7 * T)
    X = np.zeros((n, 13), F32)
    X[:, :3] = rng.uniform(-1, 1, (n, 3))
    q = rng.standard_normal((n, 4))
    X[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    X[:, 7:] = rng.uniform(-0.3, 0.3, (n, 6))
    return X, (force * rng.standard_normal((T, n, 6))).astype(F32)


def auv_goal():
    g = np.zeros(13, F32)
    g[:3] = [1.0, -0.5, 0.25]
    g[3:7] = np.asarray([0.1, -0.2, 0.3, 0.9], F32) / F32(np.linalg.norm([0.1, -0.2, 0.3, 0.9]))
    return g


# ---- handle configurations -------------------------------------------------------------------------------------------------------------
def dense_q(s, seed=7):
    """a symmetric positive definite Q [s, s] with non-zero off-diagonal entries"""
    L = np.random.default_rng(seed).uniform(-0.3, 0.3, (s, s)) + np.eye(s)
    Q = (L @ L.T).astype(F32)
    assert np.count_nonzero(Q - np.diag(np.diag(Q))) > 0
    return Q


def pm_kw(a, q="diag", K=64, H=4, **kw):
    """keywords of a point-mass handle: q = "diag", "dense" or "ellipse" (the 2D ellipse cost; a >= 2)"""
    s = 2 * a
    goal = np.zeros(s, F32)
    goal[0::2] = [1.0, 0.5, 0.75, -0.5][:a]
    c = dict(k=K, tau=H, s_dim=s, a_dim=a, dt=0.1, mass=1.25, lam=1.0, sigma=np.eye(a, dtype=F32) * F32(0.25), goal=goal, seed=3)
    if q == "ellipse":
        c["ellipse"] = ELLIPSE2D
    else:
        c["Q"] = dense_q(s) if q == "dense" else np.linspace(0.5, 2.0, s).astype(F32)
    return dict(c, **kw)


def auv_kw(cost, rk, K=64, H=4, **kw):
    """keywords of a rexrov2 Fossen handle with the quadratic cost ("quad"), StaticQuatCost ("quat") or ElipseCost3D ("e3")"""
    from batch_util import E3, Q10, rexrov2
    c = dict(k=K, tau=H, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=np.eye(6, dtype=F32) * F32(50.0), auv=rexrov2(rk), goal=auv_goal(), seed=5)
    if cost == "quat":
        c["Q"], c["quat_cost"] = Q10, True
    elif cost == "e3":
        c["ellipse3d"] = E3
    else:
        c["Q"] = np.linspace(0.5, 2.0, 13).astype(F32)
    return dict(c, **kw)


def make_mlp(s, a, hid=32, seed=0):
    """a Dense(hid, relu) + Dense(s) learned point-mass model with a normalisation"""
    from episode_util import make_nnauv
    return make_nnauv(seed, hid, 1, n_in=s + a, n_out=s)


def learned_kw(kind):
    """keywords of the three learned handles: "mlp" (Dense(32) point mass, a = 2), "nnauv", "nnauv_speed" """
    from batch_util import Q10
    from episode_util import make_nnauv
    if kind == "mlp":
        return dict(pm_kw(2, K=64, H=4), mlp=make_mlp(4, 2))
    c = dict(k=64, tau=4, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=np.eye(6, dtype=F32), goal=auv_goal(), Q=Q10, quat_cost=True, seed=9)
    if kind == "nnauv":
        return dict(c, nnauv=make_nnauv(3, 16, 1))
    return dict(c, nnauv_speed=make_nnauv(3, 16, 1, n_in=15, n_out=6))


def learned_inputs(kind, n, T, seed=0):
    return pm_inputs(2, n, T, seed) if kind == "mlp" else auv_inputs(n, T, seed, force=1.0)


# ---- the readout cases: one control step whose samples' costs are rebuilt from their trajectories ---------------------------------------
# The C++ action-cost form (lambda u' Sigma^-1 eps), no action limits, a non-zero nominal sequence.
def readout_case(name):
    """-> dict(K, H, s, a, sigma, x, U, seed, ks_extra, handle = Handle keywords, problem = oracle Problem keywords)"""
    if name == "pm":
        K, H, a = 128, 8, 2
        sigma = np.eye(a) * 0.5
        goal = np.asarray([1.0, 0.0, 0.5, 0.0], F32)
        Q = np.asarray([1.0, 0.5, 2.0, 0.25], F32)
        rng = np.random.default_rng(41)
        case = dict(K=K, H=H, s=4, a=a, sigma=sigma, seed=11, ks=[0, 63, 64, K - 1], x=np.asarray([0.2, -0.1, -0.3, 0.15], F32),
                    U=rng.uniform(-0.5, 0.5, (H, a)).astype(F32))
        case["handle"] = dict(k=K, tau=H, s_dim=4, a_dim=a, dt=0.1, mass=1.0, lam=1.0, sigma=sigma, goal=goal, Q=Q, seed=11)
        case["problem"] = dict(tau=H, s=4, a=a, dt=0.1, mass=1.0, lam=1.0, sigma=sigma, goal=goal, Q=Q)
        return case
    from batch_util import rexrov2
    K, H = 64, 4
    sigma = np.eye(6) * 50.0
    goal, Q = auv_goal(), np.linspace(0.5, 2.0, 13).astype(F32)
    x0, V = auv_inputs(1, H, seed=3, force=80.0)
    case = dict(K=K, H=H, s=13, a=6, sigma=sigma, seed=12, ks=[0, K - 1], x=x0[0], U=np.ascontiguousarray(V[:, 0]))
    case["handle"] = dict(k=K, tau=H, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=sigma, auv=rexrov2(2), goal=goal, Q=Q, seed=12)
    case["problem"] = dict(tau=H, s=13, a=6, dt=0.1, lam=1.0, sigma=sigma, auv=rexrov2(2), goal=goal, Q=Q)
    return case


def rollout_cost_from(Cs, ac):
    """the sequential fp32 recurrence of a rollout's cost (orc_rollout_cost, the kernels): c = c + (C[t] + ac[t]) for t = 0 .. H-1, then
    c = c + C[H-1] — Cs [H] the state costs of the states the steps produced, ac [H] the action costs"""
    Cs, ac = np.asarray(Cs, F32), np.asarray(ac, F32)
    c = F32(0.0)
    for t in range(Cs.shape[0]):
        c = F32(c + F32(Cs[t] + ac[t]))
    return F32(c + Cs[-1])
