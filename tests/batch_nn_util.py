"""What the tests of the batched learned-model controllers share (test_batch_nn_oracle.py on the CPU, test_batch_nn_gpu.py on the GPU): the
case matrix, every member's network / seed / goal / lambda / x / sequence, the oracle problems and the bars. A plain module: `m` is the
mppi_tf_amd package the GPU file's fixture gives.

The shapes are the smallest at which k_rollout_nn_batch can still go wrong: a ragged last tile (K = 100, 130, 65), a lone tile (K = 64), a
partial 4-step Philox group (H = 5, 9), B = 1, and more workgroups than the chip has CUs (B = 300)."""
import functools

import numpy as np

from batch_util import E3, Q10
from episode_util import make_nnauv
from oracle import oracle as orc

F32 = np.float32
MODELS = {"nnauv": (1, 16, 13), "nnspeed": (2, 15, 6)}  # GEN_MODEL_* of the kernel names, network inputs, outputs
CASES = [
    dict(id="nnauv-32x3-diag-quadratic", model="nnauv", hid=32, nh=3, dense=False, cost="quadratic", K=100, H=5, B=3),
    dict(id="nnauv-16x1-dense-quat", model="nnauv", hid=16, nh=1, dense=True, cost="quat", K=64, H=4, B=1),
    dict(id="nnauv-32x2-diag-ellipse3d", model="nnauv", hid=32, nh=2, dense=False, cost="ellipse3d", K=130, H=9, B=4, net_seed=164, spread=0.1),
    dict(id="nnspeed-16x3-diag-quadratic", model="nnspeed", hid=16, nh=3, dense=False, cost="quadratic", K=100, H=5, B=3),
    dict(id="nnspeed-32x1-dense-quat", model="nnspeed", hid=32, nh=1, dense=True, cost="quat", K=65, H=8, B=2),
    dict(id="nnauv-16x2-diag-quadratic-B300", model="nnauv", hid=16, nh=2, dense=False, cost="quadratic", K=64, H=4, B=300, check=(0, 150, 299)),
]
IDS = [c["id"] for c in CASES]
GOAL13 = np.array([1.0, 2.0, -3.0, 0.0, 0.0, np.sin(0.2), np.cos(0.2)] + [0.0] * 6)
X0 = np.array([0.5, -0.5, 0.2, 0.0, 0.0, 0.0, 1.0, 0.3, 0.0, -0.1, 0.0, 0.05, 0.0])
# the bars the project holds these models to (tests/test_auv_gpu.py): costs relative to fp64, U' absolute on noise of scale 0.5
COST_BAR, COST_FAC, U_BAR, U_FAC = 2e-5, 4, 1e-5, 4


def checked(case):
    return list(case.get("check", range(case["B"])))


def make_net(case, seed):
    """a network of the case's shape, as make_nnauv / make_nnauv_speed of the lone tests make them; the cases whose cost takes acos of a raw
    quaternion dot product (StaticQuatCost, ElipseCost3D; NNAUVModel does not renormalise the attitude) scale the output layer by 0.2, so
    that the product stays inside (-1, 1) over the horizon"""
    _, n_in, n_out = MODELS[case["model"]]
    net = make_nnauv(seed, case["hid"], case["nh"], n_in, n_out)
    if case["cost"] in ("quat", "ellipse3d"):
        net["W"][-1] = (0.2 * net["W"][-1]).astype(F32)
        net["b"][-1] = (0.2 * net["b"][-1]).astype(F32)
    return net


def sigma_of(case):
    s = 0.25 * np.eye(6)
    return (s + 0.02 * (1 - np.eye(6))) if case["dense"] else s


def cost_kw(case):
    """the shared cost keywords (Handle's and the oracle's alike)"""
    if case["cost"] == "quat":
        return dict(Q=Q10 / 10, quat_cost=True)
    if case["cost"] == "ellipse3d":
        return dict(ellipse3d=E3)
    return dict(Q=np.array([10.0] * 3 + [5.0] * 4 + [1.0] * 6))


@functools.lru_cache(maxsize=None)
def members(ci):
    """case CASES[ci] -> dict(nets, seeds, lams, G, X, U0): every member its own network, Philox key, goal, lambda, x and sequence"""
    case = CASES[ci]
    B, H = case["B"], case["H"]
    rng = np.random.default_rng(1000 + ci)
    G = np.tile(GOAL13, (B, 1))
    G[:, :3] += rng.uniform(-1, 1, (B, 3))
    if case["cost"] == "quat":  # a goal attitude a radian away from the start
        G[:, 3:7] = [0.0, 0.0, np.sin(0.5), np.cos(0.5)]
    X = np.tile(X0, (B, 1))
    X[:, :3] += rng.uniform(-1, 1, (B, 3)) * case.get("spread", 0.5)
    X[:, 7:] += rng.uniform(-0.1, 0.1, (B, 6))
    return dict(nets=[make_net(case, case.get("net_seed", 50 + 7 * ci) + m) for m in range(B)], seeds=[11 + 3 * m for m in range(B)],
                lams=[0.8 + 0.1 * (m % 5) for m in range(B)], G=G.astype(F32), X=X.astype(F32),
                U0=(0.1 * rng.standard_normal((B, H, 6))).astype(F32))


def problem(case, mem, m, dtype, net=None):
    """the oracle problem of member m (net: another member's network in its place)"""
    kind = "nnauv" if case["model"] == "nnauv" else "nnauv_speed"
    return orc.Problem(tau=case["H"], s=13, a=6, dt=0.1, lam=mem["lams"][m], sigma=sigma_of(case), goal=mem["G"][m], threads=0, dtype=dtype,
                       **{kind: mem["nets"][m] if net is None else net}, **cost_kw(case))


def oracle_step(case, mem, m, U, eps, net=None):
    """one update of member m on the noise eps -> dict(c64, c32, U64, U32, rel32, eu32, u_bar): the fp64 and fp32 CPU results, the fp32
    CPU's own errors against fp64 and the U' bar that follows from them"""
    _, U64, c64 = problem(case, mem, m, np.float64, net).next_with_noise(mem["X"][m], U, eps)
    _, U32, c32 = problem(case, mem, m, F32, net).next_with_noise(mem["X"][m], U, eps)
    c64 = np.asarray(c64, np.float64)
    rel32 = float((np.abs(c32.astype(np.float64) - c64) / np.abs(c64)).max())
    eu32 = float(np.abs(np.asarray(U32, np.float64) - U64).max())
    return dict(c64=c64, c32=c32, U64=np.asarray(U64, np.float64), U32=U32, rel32=rel32, eu32=eu32, u_bar=max(U_BAR, U_FAC * eu32))


def first_noise(case, mem, m):
    """member m's noise of step 0 from its Philox key, on the CPU"""
    return orc.noise(mem["seeds"][m], 0, 0, case["K"], case["H"], 6, sigma_of(case).astype(F32))


# ---- the handles (GPU) ---------------------------------------------------------------------------------------------------------------
def kernel_names(case):
    """(the batch's rollout kernel, the lone handle's) as rocprofv3 prints them"""
    args = "<%d, %d, %s>" % (MODELS[case["model"]][0], case["hid"], "false" if case["dense"] else "true")
    return "mppi::k_rollout_nn_batch" + args, "mppi::k_rollout_gen" + args


def lone_kw(case, mem, i, net=None):
    """Handle keywords of member i's lone controller on k_rollout_gen: that kernel is the default for NNAUVModel Dense(16), else the handle
    is tuned onto it with MPPI_TUNE_MLP32_VALU = 1"""
    kind = "nnauv" if case["model"] == "nnauv" else "nnauv_speed"
    tuned = not (case["model"] == "nnauv" and case["hid"] == 16)
    return dict(k=case["K"], tau=case["H"], s_dim=13, a_dim=6, dt=0.1, lam=mem["lams"][i], sigma=sigma_of(case), goal=mem["G"][i],
                seed=mem["seeds"][i], tuning={"mlp32_valu": 1} if tuned else None, **{kind: mem["nets"][i] if net is None else net},
                **cost_kw(case))


def make_batch(m, case, mem, nets=None, **kw):
    model = "nnauv" if case["model"] == "nnauv" else "nnauv_speed"
    hb = m.BatchHandle.learned(case["B"], mem["nets"] if nets is None else nets, model, k=case["K"], tau=case["H"], dt=0.1, sigma=sigma_of(case),
                               seeds=mem["seeds"], lams=mem["lams"], goals=mem["G"], **cost_kw(case), **kw)
    hb.set_action_sequences(mem["U0"])
    return hb


def make_lone(m, case, mem, i, net=None):
    h = m.Handle(**lone_kw(case, mem, i, net))
    assert h.rollout_kernel_name() == kernel_names(case)[1], h.rollout_kernel_name()
    h.set_action_sequence(mem["U0"][i])
    return h
