"""What the tests of the batched learned point-mass controllers share (test_batch_mlp_oracle.py on the CPU, test_batch_mlp_gpu.py on the
GPU): the case matrix, every member's network / normalisation / seed / goal / lambda / gamma / upsilon / sigma / Q / x / sequence, the
oracle problems and the bars. A plain module: `m` is the mppi_tf_amd package the GPU file's fixture gives.

The shapes are the smallest at which the two kernels can still go wrong. k_rollout_mlp2_batch owns 64 rollouts per workgroup as two sets
of 32: K = 33 leaves set A full and set B one lane, 64 is one full tile, 65 a ragged second tile whose set B is all clamped lanes, 129
three tiles; H = 1 is no loop iteration at all, 4 a whole Philox group, 5 and 9 ragged groups. k_rollout_mlp_small_batch owns 64 per
one-wave workgroup: K = 1, 64, 65."""
import functools

import numpy as np

from episode_util import make_nnauv
from oracle import oracle as orc

F32 = np.float32
WIDE_KH = [(33, 1), (64, 4), (65, 5), (129, 9)]
NARROW_KH = [(1, 1), (64, 4), (65, 5)]
# wide: a in {1, 2, 3} x WIDE_KH; sigma dense where it can be (a >= 2) on every other shape, so both DIAG instances of a = 2 and 3 run
WIDE = [dict(id="wide-a%d-K%d-H%d-%s" % (a, K, H, "dense" if dense else "diag"), hid=256, nh=2, a=a, K=K, H=H, dense=dense, B=3)
        for a in (1, 2, 3) for i, (K, H) in enumerate(WIDE_KH) for dense in [a >= 2 and (i + a) % 2 == 0]]
NARROW = [dict(id="dense%dx%d-a%d-K%d-H%d" % (hid, nh, a, K, H), hid=hid, nh=nh, a=a, K=K, H=H, dense=(a == 4 and nh == 3), B=3)
          for hid in (16, 32) for nh in (1, 3) for a in (1, 4) for (K, H) in NARROW_KH]
# more workgroups than the chip holds at once: B = 300 (members 0, 149, 299 are compared)
MANY = [dict(id="wide-a2-B300", hid=256, nh=2, a=2, K=64, H=2, dense=False, B=300, check=(0, 149, 299)),
        dict(id="dense16x2-a2-B300", hid=16, nh=2, a=2, K=64, H=2, dense=False, B=300, check=(0, 149, 299))]
# the direct check against the oracle: one wide and one narrow member set at (K, H) = (129, 9)
ORACLE = [dict(id="oracle-wide-a3", hid=256, nh=2, a=3, K=129, H=9, dense=True, B=3),
          dict(id="oracle-dense32x3-a2", hid=32, nh=3, a=2, K=129, H=9, dense=False, B=3)]
CASES = WIDE + NARROW + MANY + ORACLE
IDS = [c["id"] for c in CASES]
INDEX = {c["id"]: i for i, c in enumerate(CASES)}
# the bars DESIGN section 3 states for learned models: costs relative to fp64, U' absolute
COST_BAR, COST_FAC, U_BAR, U_FAC = 2e-5, 4, 1e-5, 4


def ids_of(cases):
    return [INDEX[c["id"]] for c in cases]


def checked(case):
    return list(case.get("check", range(case["B"])))


def make_net(case, seed):
    a = case["a"]
    return make_nnauv(seed, case["hid"], case["nh"], 3 * a, 2 * a)


def sigma_of(case, i):
    """member i's sigma: its own scale; dense for every member or diagonal for every member"""
    a = case["a"]
    s = (0.25 + 0.05 * (i % 4)) * np.eye(a)
    return (s + 0.02 * (1 - np.eye(a))) if case["dense"] else s


@functools.lru_cache(maxsize=None)
def members(ci):
    """case CASES[ci] -> build_members of it, made once"""
    return build_members(CASES[ci], ci)


def build_members(case, ci):
    """every member its own network and normalisation, Philox key, goal, lambda, gamma, upsilon, sigma, Q, x and sequence (ci: the salt)"""
    B, H, a = case["B"], case["H"], case["a"]
    s = 2 * a
    rng = np.random.default_rng(2000 + ci)
    G = np.zeros((B, s))
    G[:, 0::2] = rng.uniform(-1, 1, (B, a))
    X = 0.2 * rng.standard_normal((B, s))
    return dict(nets=[make_net(case, 70 + 11 * ci + i) for i in range(B)], seeds=[11 + 3 * i for i in range(B)],
                lams=[0.8 + 0.1 * (i % 5) for i in range(B)], gammas=[1.0 - 0.1 * (i % 3) for i in range(B)],
                upsilons=[1.0 + 0.5 * (i % 3) for i in range(B)], sigmas=[sigma_of(case, i).astype(F32) for i in range(B)],
                Qs=[(np.array([10.0, 1.0] * a) * (1.0 + 0.25 * (i % 4))).astype(F32) for i in range(B)],
                G=G.astype(F32), X=X.astype(F32), U0=(0.1 * rng.standard_normal((B, H, a))).astype(F32))


def problem(case, mem, i, dtype, net=None):
    """the oracle problem of member i (net: another member's network in its place)"""
    a = case["a"]
    return orc.Problem(tau=case["H"], s=2 * a, a=a, dt=0.1, lam=mem["lams"][i], gamma=mem["gammas"][i], upsilon=mem["upsilons"][i],
                       sigma=mem["sigmas"][i], goal=mem["G"][i], Q=mem["Qs"][i], threads=0, dtype=dtype,
                       mlp=mem["nets"][i] if net is None else net)


def oracle_step(case, mem, i, U, eps, net=None):
    """one update of member i on the noise eps -> the fp64 and fp32 CPU results, the fp32 CPU's own errors against fp64"""
    _, U64, c64 = problem(case, mem, i, np.float64, net).next_with_noise(mem["X"][i], U, eps)
    _, U32, c32 = problem(case, mem, i, F32, net).next_with_noise(mem["X"][i], U, eps)
    c64 = np.asarray(c64, np.float64)
    rel32 = float((np.abs(np.asarray(c32, np.float64) - c64) / np.abs(c64)).max())
    eu32 = float(np.abs(np.asarray(U32, np.float64) - U64).max())
    return dict(c64=c64, U64=np.asarray(U64, np.float64), rel32=rel32, eu32=eu32)


def first_noise(case, mem, i):
    """member i's noise of step 0 from its Philox key, on the CPU"""
    return orc.noise(mem["seeds"][i], 0, 0, case["K"], case["H"], case["a"], mem["sigmas"][i])


# ---- the handles (GPU) ---------------------------------------------------------------------------------------------------------------
def kernel_names(case):
    """(the batch's rollout kernel, what the lone handle's starts with) as rocprofv3 prints them"""
    a = case["a"]
    if case["hid"] == 256:
        diag = "false" if (case["dense"] and a > 1) else "true"
        return "mppi::k_rollout_mlp2_batch<%d, %s>" % (a, diag), "mppi::k_rollout_mlp2<%d, %s, " % (a, diag)
    return "mppi::k_rollout_mlp_small_batch<%d, %d>" % (a, case["hid"]), "mppi::k_rollout_mlp_small<%d, %d>" % (a, case["hid"])


def lone_kw(case, mem, i, net=None):
    """Handle keywords of member i's lone controller: its default kernel, except Dense(32), tuned onto the vector-ALU kernel"""
    a = case["a"]
    return dict(k=case["K"], tau=case["H"], s_dim=2 * a, a_dim=a, dt=0.1, lam=mem["lams"][i], gamma=mem["gammas"][i],
                upsilon=mem["upsilons"][i], sigma=mem["sigmas"][i], goal=mem["G"][i], Q=mem["Qs"][i], seed=mem["seeds"][i],
                tuning={"mlp32_valu": 1} if case["hid"] == 32 else None, mlp=mem["nets"][i] if net is None else net)


def make_batch(m, case, mem, nets=None, **kw):
    hb = m.BatchHandle.learned(case["B"], mem["nets"] if nets is None else nets, "mlp", a_dim=case["a"], k=case["K"], tau=case["H"], dt=0.1,
                               seeds=mem["seeds"], lams=mem["lams"], gammas=mem["gammas"], upsilons=mem["upsilons"], sigmas=mem["sigmas"],
                               Qs=mem["Qs"], goals=mem["G"], **kw)
    hb.set_action_sequences(mem["U0"])
    return hb


def make_lone(m, case, mem, i, net=None):
    h = m.Handle(**lone_kw(case, mem, i, net))
    assert h.rollout_kernel_name().startswith(kernel_names(case)[1]), h.rollout_kernel_name()
    h.set_action_sequence(mem["U0"][i])
    return h
