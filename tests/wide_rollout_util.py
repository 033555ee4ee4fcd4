"""What the trajectory-validation tests of a WIDE learner batch share (test_learner_wide_rollout_oracle.py on the CPU,
test_learner_wide_rollout_gpu.py on the GPU): the cases, one per action width a = 1..4 of the [3a, 256, 256, 2a] point-mass network, built on
learner_rollout_util's networks and its numpy restatement of the plain-order step (k_mlp_step_ref), and two WRONG steps — layer sums taken
in descending j, and each product and add rounded once (an emulated fused multiply-add) — that a kernel of the wrong arithmetic would
compute. A plain module."""
import numpy as np

import learner_rollout_util as L

F32 = np.float32
MLP = L.MLP
R = 16                      # trajectories per workgroup of k_wb_rollout (kWideRollR)
N_SSE, T_SSE = 129, 7       # the squared-error case: nine blocks of 16 with a single live trajectory in the last
TREE = 4                    # fp32 additions on a term's path across a block's 16 trajectories: a pairwise tree
DEAD = (1, 5)               # hidden unit 5 of layer 1: zero incoming weights, negative bias
A_DIMS = (1, 2, 3, 4)
_cache = {}


def sse_bar(T):
    """the relative bound of an fp32 sse against fp64 over the same trajectories: 2 (T + 6 + d) 2^-24 with d = TREE (derived in
    test_learner_wide_rollout_gpu.py)"""
    return 2.0 * (T + 6 + TREE) * 2.0 ** -24


def dims(a):
    return [3 * a, 256, 256, 2 * a]


def case(a, B=3):
    """-> dict(kind, s, a, dims, norm, nets [B]: the members' weights, truth: another network's): built once, never modified"""
    if (a, B) not in _cache:
        d = dims(a)
        _cache[(a, B)] = dict(kind=MLP, s=2 * a, a=a, dims=d, dead=DEAD, norm=L.make_norm(d[0], d[-1], 40 + a),
                              nets=[L.make_net(d, 500 + 10 * a + m, dead=DEAD) for m in range(B)], truth=L.make_net(d, 500 + 10 * a + 9))
    return _cache[(a, B)]


def inputs(a, n, T, seed=0):
    """-> (x0 [n, 2a] uniform in [-1, 1], V [T, n, a] uniform in [-2, 2]): distinct per trajectory and step"""
    rng = np.random.default_rng(9000 + 31 * seed + 101 * a + n + 11 * T)
    return rng.uniform(-1, 1, (n, 2 * a)).astype(F32), rng.uniform(-2, 2, (T, n, a)).astype(F32)


def model_desc(c):
    return dict(kind=MLP, s_dim=c["s"], a_dim=c["a"], dt=0.1, **c["norm"])


def rollout(c, net, x0, V, dt=F32):
    return L.rollout(MLP, net, c["norm"], x0, V, dt)


def ground_truth(c, x0, V):
    return L.ground_truth(c, x0, V)


def sse_case(a):
    """the squared-error case of width a: n = 129, T = 7 -> (case, x0, V, G)"""
    key = ("sse", a)
    if key not in _cache:
        c = case(a)
        x0, V = inputs(a, N_SSE, T_SSE)
        _cache[key] = (c, x0, V, ground_truth(c, x0, V))
    return _cache[key]


def batch_of(m, c, nets=None):
    """a WideLearnerBatch of the case's members"""
    nets = c["nets"] if nets is None else nets
    wb = m.WideLearnerBatch(nets[0], len(nets))
    for i, net in enumerate(nets):
        wb.set_weights(net, member=i)
    return wb


def lone_handle(m, c, net):
    """the lone MPPI_MODEL_MLP handle holding `net` and the case's normalisation: what a member is held to, bit for bit"""
    a = c["a"]
    return m.Handle(k=1, tau=1, s_dim=2 * a, a_dim=a, dt=0.1, lam=1.0, sigma=np.eye(a, dtype=F32), goal=np.zeros(2 * a, F32),
                    Q=np.ones(2 * a, F32), seed=1, mlp=dict(net, **c["norm"]))


# ---- two wrong steps: what a kernel of another arithmetic computes ------------------------------------------------------------------
def wrong_step(c, net, x, v, how):
    """one fp32 step as L.step, but how = "descending": the layer sums taken for descending j; how = "fma": acc = fl(acc + cur[j] * W[j][o])
    with ONE rounding (the product of two fp32 numbers is exact in fp64; the sum is formed there and rounded to fp32)"""
    norm = c["norm"]
    cur = (np.concatenate([x, v], axis=1).astype(F32) - norm["xmean"]) / norm["xstd"]
    n_layers = len(net["W"])
    for l in range(n_layers):
        W, b = net["W"][l], net["b"][l]
        acc = np.zeros((cur.shape[0], W.shape[1]), F32)
        order = range(W.shape[0] - 1, -1, -1) if how == "descending" else range(W.shape[0])
        for j in order:
            if how == "fma":
                acc = (acc.astype(np.float64) + cur[:, j:j + 1].astype(np.float64) * W[j][None, :].astype(np.float64)).astype(F32)
            else:
                acc = acc + cur[:, j:j + 1] * W[j][None, :]
        acc = acc + b[None, :]
        cur = np.where(acc < 0, F32(0.0), acc) if l + 1 < n_layers else acc
    return x.astype(F32) + (cur * norm["ystd"] + norm["ymean"])
