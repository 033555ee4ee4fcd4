"""What the trajectory-validation tests of a learner batch share (test_learner_rollout_oracle.py on the CPU, test_learner_rollout_gpu.py on
the GPU): the cases, and a numpy restatement of the plain-order model step (k_mlp_step_ref / k_nnauv_step_ref) for the `mlp` and `nnauv`
kinds — in float32, where every operation is a single IEEE + - x / and numpy reproduces the kernel's bits, and in float64, the reference
of the squared-error sums. The speed model's Euler angles are NOT restated: that kind is compared with the lone handle only.
A plain module."""
import numpy as np

F32 = np.float32
MLP, NN_AUV, NN_AUV_SPEED = 1, 3, 4  # MPPI_MODEL_* of include/mppi_c.h
EPS = 2.0 ** -23
N_SSE, T_SSE = 129, 7  # the squared-error cases: three blocks of 64 with a ragged last one


def sse_bar(T):
    """the relative bound of an fp32 sse against fp64 over the same trajectories: (T + 16) * 2^-23 (derived in test_learner_rollout_gpu.py)"""
    return (T + 16) * EPS


# ---- networks -----------------------------------------------------------------------------------------------------------------------
def make_net(dims, seed, scale=1.0, dead=None):
    """Dense layers dims[0] -> ... -> dims[-1], random; the output layer small (a state moves a little per step). dead = (layer, unit):
    that hidden unit has zero incoming weights and a negative bias — relu kills it for every input"""
    rng = np.random.default_rng(seed)
    L = len(dims) - 1
    W = [(scale * rng.uniform(-1, 1, (dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(F32) for i in range(L)]
    b = [(scale * rng.uniform(-1, 1, dims[i + 1]) / np.sqrt(dims[i])).astype(F32) for i in range(L)]
    W[-1] *= F32(0.1)
    b[-1] *= F32(0.1)
    if dead is not None:
        W[dead[0]][:, dead[1]] = 0.0
        b[dead[0]][dead[1]] = -0.5
    return dict(W=W, b=b)


def make_norm(n_in, n_out, seed):
    rng = np.random.default_rng(seed)
    return dict(xmean=rng.uniform(-0.2, 0.2, n_in).astype(F32), xstd=rng.uniform(0.7, 1.4, n_in).astype(F32),
                ymean=rng.uniform(-0.01, 0.01, n_out).astype(F32), ystd=rng.uniform(0.7, 1.4, n_out).astype(F32))


# ---- the plain-order step ------------------------------------------------------------------------------------------------------------
def net_inputs(kind, x, v):
    return np.concatenate([x, v], axis=1) if kind == MLP else np.concatenate([x[:, 3:], v], axis=1)


def step(kind, net, norm, x, v, dt=F32):
    """x [n, s], v [n, a] -> x' [n, s] in `dt` arithmetic, operation by operation in the reference kernels' order: inputs (x - Xmean) / Xstd,
    acc = 0, acc = acc + cur[j] * W[j][o] for ascending j, + b[o], relu on the hidden layers, x' = x + (y * Ystd + Ymean)"""
    assert kind in (MLP, NN_AUV)
    c = lambda a: np.asarray(a, F32).astype(dt)  # the fp32 values, widened exactly
    cur = (net_inputs(kind, x, v).astype(dt) - c(norm["xmean"])) / c(norm["xstd"])
    L = len(net["W"])
    for l in range(L):
        W, b = c(net["W"][l]), c(net["b"][l])
        acc = np.zeros((cur.shape[0], W.shape[1]), dt)
        for j in range(W.shape[0]):
            acc = acc + cur[:, j:j + 1] * W[j][None, :]
        acc = acc + b[None, :]
        cur = np.where(acc < 0, dt(0.0), acc) if l + 1 < L else acc
    return x.astype(dt) + (cur * c(norm["ystd"]) + c(norm["ymean"]))


def rollout(kind, net, norm, x0, V, dt=F32):
    """x0 [n, s] or [1, s] or [s], V [T, n, a] -> X [T+1, n, s] in `dt`"""
    V = np.asarray(V, F32)
    T, n, _ = V.shape
    x = np.broadcast_to(np.asarray(x0, F32).reshape(-1, np.asarray(x0).shape[-1]), (n, np.asarray(x0).shape[-1])).astype(dt)
    X = [x]
    for t in range(T):
        x = step(kind, net, norm, x, V[t], dt)
        X.append(x)
    return np.stack(X)


def sse64(X, G):
    """sum over steps and trajectories of (X - G)^2 in float64: X [T+1, n, s] (or [B, T+1, n, s]), G [T+1, n, s] -> [s] (or [B, s])"""
    d = np.asarray(X, np.float64) - np.asarray(G, np.float64)
    return (d * d).sum(axis=(-3, -2))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def inputs(kind, n, T, seed=0):
    """-> (x0 [n, s], V [T, n, a]): distinct per trajectory and step; 13-state x0 with unit quaternions"""
    rng = np.random.default_rng(7000 + 31 * seed + n + 11 * T)
    if kind == MLP:
        return rng.uniform(-1, 1, (n, 4)).astype(F32), rng.uniform(-2, 2, (T, n, 2)).astype(F32)
    x = np.zeros((n, 13), F32)
    x[:, :3] = rng.uniform(-1, 1, (n, 3))
    q = rng.standard_normal((n, 4))
    x[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x[:, 7:] = rng.uniform(-0.3, 0.3, (n, 6))
    return x, rng.standard_normal((T, n, 6)).astype(F32)


CASES = {  # name -> (kind, s, a, layer widths, the dead hidden unit)
    "mlp_6_7_5_4": (MLP, 4, 2, [6, 7, 5, 4], (1, 2)),
    "nnauv_16_13": (NN_AUV, 13, 6, [16, 13], None),
    "nnauv_16_32_32_32_13": (NN_AUV, 13, 6, [16, 32, 32, 32, 13], (0, 5)),
}
_cache = {}


def case(name, B=3):
    """-> dict(kind, s, a, dims, norm, nets [B]: the members' weights, truth: another network's): built once, never modified"""
    if (name, B) not in _cache:
        kind, s, a, dims, dead = CASES[name]
        seed = sorted(CASES).index(name)
        _cache[(name, B)] = dict(kind=kind, s=s, a=a, dims=dims, dead=dead, norm=make_norm(dims[0], dims[-1], 40 + seed),
                                 nets=[make_net(dims, 100 * seed + m, dead=dead) for m in range(B)], truth=make_net(dims, 100 * seed + 99))
    return _cache[(name, B)]


def model_desc(c):
    return dict(kind=c["kind"], s_dim=c["s"], a_dim=c["a"], dt=0.1, **c["norm"])


def ground_truth(c, x0, V):
    """what the members are judged against: the fp64 trajectory of the case's `truth` network plus a little noise, as fp32 [T+1, n, s]"""
    G = rollout(c["kind"], c["truth"], c["norm"], x0, V, np.float64)
    return (G + 0.01 * np.random.default_rng(5).standard_normal(G.shape)).astype(F32)


def sse_case(name):
    """the squared-error case of `name`: n = 129, T = 7 -> (case, x0, V, G)"""
    key = ("sse", name)
    if key not in _cache:
        c = case(name)
        x0, V = inputs(c["kind"], N_SSE, T_SSE)
        _cache[key] = (c, x0, V, ground_truth(c, x0, V))
    return _cache[key]


def batch_of(m, c, nets=None):
    """a LearnerBatch of the case's members"""
    nets = c["nets"] if nets is None else nets
    lb = m.LearnerBatch(nets[0], len(nets))
    for i, net in enumerate(nets):
        lb.set_weights(net, member=i)
    return lb
