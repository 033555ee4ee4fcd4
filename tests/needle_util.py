"""What the needle tests share (test_needle_oracle.py on the CPU, test_needle_gpu.py on the GPU): the case matrix, the three-call
protocol that turns one chosen sample k* of a control step into a needle, the fp64 reference and the checks. A plain module: `m` is the
mppi_tf_amd package each GPU test file's fixture gives.

A needle: x sits on the goal at rest and the nominal sequence is U = -eps[k*], so sample k* applies U + eps[k*] = 0 exactly, stays on the
goal and costs nothing, while every other sample applies eps[k] - eps[k*] != 0 and leaves it. With a large Q and a small lambda the
soft-min puts (nearly) all weight on k*, and U' = U + sum_k w_k eps_k ~ 0 whatever K is — unless the update drops, mis-weights or misplaces
that one sample's contribution, in which case U' moves by O(sigma) = 1e4 x U_TOL. Whether a case IS a needle depends on the reference
only: conditions (a) w_ref[k*] >= W_MIN, (b) |U'_ref - U'_ref without k*| >= LOO_MIN and (c) the fp32 oracle's update within COND_MAX of
the fp64 oracle's, proven on the CPU for the oracle's restated noise and recomputed on the GPU for the noise the step drew.

No action cost: the cases use the gamma / upsilon action-cost form with gamma = 0 and upsilon = 1, whose every term is multiplied by an
exact zero. (The C++ form's lambda u' Sigma^-1 eps is not zero once U = -eps[k*]: it gives k* the cost
-lambda sum_t eps*' Sigma^-1 eps* < 0; the case `fused7_K8192_cpp_form` keeps that form and holds beta to that cost instead of to 0.)
The form is a run-time branch of the same kernel instances (mppi_rollout_pc.inc), so the records and their combine are the same code.
"""
import numpy as np

from oracle import oracle as orc

F32 = np.float32
U_TOL = 1e-5            # tests/test_parity_gpu.py: stated fp32 tolerance on the control update (absolute, on U' and u; x the noise scale)
W_MIN = 0.999           # (a) the reference weight of the needle
LOO_MIN = 100 * U_TOL   # (b) what losing the needle moves the reference update by, at least
COND_MAX = U_TOL / 4    # (c) the reference's own fp32 evaluation of the update is this close to its fp64 one: 1/lambda amplifies the fp32 rounding of the
#                         runner-up costs, and a case where that alone comes near U_TOL would test the case, not the kernel
ETA_RTOL = 1e-5         # eta against the fp64 sum of exp(-(c - beta)/lambda) over the pinned fp32 costs: the finish accumulates in double; what
#                         remains is the fp32 rounding of the argument (<= ~17 * 2^-23 for any weight above 4e-8), expf at a few ulp and a
#                         64-term fp32 tile sum: together <= ~7e-6
W_RTOL = 2e-4           # DBG_WEIGHTS[k*] (test_normalize_cost_on_the_fused_path's tolerance)
GOAL3 = [1, 0, .5, 0, .75, 0]
DENSE_SIGMA3 = np.array([[0.3, 0.05, 0.0], [0.02, 0.2, -0.04], [0.0, 0.03, 0.25]])
Q10 = np.diag([100.0] * 3 + [10.0] + [1.0] * 6) + 0.01
AUV_SIGMA = 200.0       # the noise scale tests/test_auv_gpu.py uses; the AUV update is held to U_TOL x this
AUV_TILE = 64           # rollouts per tile of k_rollout_auv_pc and k_rollout_gen


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------
# Each case's lambda is about a ninth of the smallest gap between cost[k*] = 0 and the next-best sample over the case's k* (fp64 oracle on
# the restated noise, Q scale 1e4; tests/test_needle_oracle.py holds the result to W_MIN): the needle keeps >= 0.9999 of the weight, and
# the other samples still carry enough of it (up to ~7e-5, tens of U_TOL in U') that eta, w[k*] and U' are not trivially 1, 1 and 0.
def pm(id, K, ks, kernel, H=4, a=3, lam=1.0, q=1e4, sigma=0.5, seed=1, dense_q=False, normalize=False, tuning=None, inject=False,
       cpp_form=False, group="", goal=None):
    """one point-mass case: `kernel` is what rollout_kernel_name() must contain (a tuple: start, end), `ks` the needles to loop over"""
    return dict(id=id, model="pm", K=K, ks=list(ks), kernel=kernel, H=H, a=a, lam=lam, q=q, seed=seed, dense_q=dense_q, normalize=normalize,
                sigma=np.asarray(sigma * np.eye(a) if np.isscalar(sigma) else sigma, np.float64), tuning=tuning, inject=inject, cpp_form=cpp_form,
                group=group, goal=goal, scale=1.0)


def auv(id, K, kernel, lam, q, tuning=None, seed=1, goal=None, ks=None, group="auv"):
    """one Fossen-AUV case (rexrov2 made neutrally buoyant, StaticQuatCost, H = 2): needles in the first tile, across the first tile
    boundary and in the ragged last tile"""
    ks = [0, AUV_TILE - 1, AUV_TILE, K - 1] if ks is None else ks
    return dict(id=id, model="auv", K=K, ks=list(ks), kernel=kernel, H=2, a=6, lam=lam, q=q, seed=seed, dense_q=False, normalize=False,
                sigma=AUV_SIGMA * np.eye(6), tuning=tuning, inject=False, cpp_form=False, group=group, goal=goal, scale=AUV_SIGMA)


FOLD_KS = [64 * b for b in range(8)] + [1023, 1024, 65535, 65536]  # a needle per XCD-class slot; the last tile of fold group 0, the first of group 1; the last full tile; alone in the last group
FUSED = [pm("%s_K%d" % (name, K), K, ks, (kern, ""), tuning=tun, lam=lam, group="fused")
         for name, tun, kern in (("fused7", None, "mppi::k_step_pc<3, 7, 3, true"), ("fused5", {"fused_step": 2}, "mppi::k_step_pc<3, 5, "))
         for K, ks, lam in ((65, [0, 63, 64], 20.0), (8191, [8190], 20.0), (8192, [0, 63, 64, 4095, 8128, 8191], 7.0))]
FUSED += [pm("two_launch_K8192", 8192, [0, 63, 64, 4095, 8128, 8191], ("mppi::k_rollout_pc<3, 5, ", ", 0, 0>"), tuning={"fused_step": 0}, lam=7.0, group="fused"),
          pm("fused7_K8192_cpp_form", 8192, [0, 4095, 8191], ("mppi::k_step_pc<3, 7, 3, true", ""), cpp_form=True, lam=6.0, group="fused")]
FINISH = [pm("cols_K8193", 8193, [0, 8191, 8192], ("mppi::k_rollout_pc<3, 5, ", ", 0, 0>"), lam=7.0, group="finish_cols"),
          pm("cols_K32768", 32768, [32767], ("mppi::k_rollout_pc<3, 5, ", ", 0, 0>"), lam=12.0, group="finish_cols"),
          pm("cols_K32769", 32769, [0, 32767, 32768], ("mppi::k_rollout_pc<3, 3, ", ", 0, 0>"), lam=4.0, group="finish_cols"),
          pm("cols_K65536", 65536, [0, 65535], ("mppi::k_rollout_pc<3, 3, ", ", 0, 0>"), lam=4.0, group="finish_cols")]
FOLD = [pm("fold_K65537", 65537, FOLD_KS, ("mppi::k_rollout_pc<3, 3, ", ", 0, 0>"), lam=2.5, group="fold"),
        pm("fold_K131073", 131073, [0, 131071, 131072], ("mppi::k_rollout_pc<3, 3, ", ", 0, 0>"), lam=4.0, group="fold")]
NORMALIZE = [pm("norm_K8193", 8193, [0, 8191, 8192], ("mppi::k_rollout_pc<3, 5, ", ""), normalize=True, lam=6e-4, group="normalize"),
             pm("norm_K131073", 131073, [0, 131071, 131072], ("mppi::k_rollout_pc<3, 3, ", ""), normalize=True, lam=2.5e-4, group="normalize")]
INSTANCES = [pm("dense_sigma", 4097, [0, 4095, 4096], ("mppi::k_step_pc<3, 7, 3, false", ""), sigma=2.0 * DENSE_SIGMA3, lam=10.0, group="instances"),
             pm("dense_q", 4097, [0, 4095, 4096], ("mppi::k_rollout_pc<3, 5, ", ", 2, 0>"), dense_q=True, lam=10.0, group="instances"),
             pm("a1_H8", 4097, [0, 4095, 4096], ("mppi::k_step_pc<1, ", ""), H=8, a=1, lam=2.0, group="instances"),
             pm("a2", 4097, [0, 4095, 4096], ("mppi::k_step_pc<2, ", ""), a=2, lam=2.0, group="instances"),
             pm("a4", 4097, [0, 4095, 4096], ("mppi::k_step_pc<4, ", ""), a=4, lam=20.0, group="instances")]
TILE = [pm("tile_K8193", 8193, [0, 8191, 8192], ("mppi::k_rollout_tile<3, 64, ", ""), tuning={"force_tile_kernel": 1}, lam=7.0, group="tile"),
        pm("tile_R32_inject", 300, [31, 32, 299], ("mppi::k_rollout_tile<3, 32, ", ""), H=256, inject=True, q=1.0, lam=200.0, group="tile"),
        pm("tile_R16_inject", 100, [15, 16, 99], ("mppi::k_rollout_tile<4, 16, ", ""), H=500, a=4, inject=True, q=1.0, lam=2500.0, group="tile")]
LONE = FUSED + FINISH + FOLD + NORMALIZE + INSTANCES + TILE

# K-sharded: k* at 0, K-1 and on both sides of every shard boundary
SHARD_KERNEL = ("mppi::k_rollout_pc<3, 5, ", ", 0, 0>")


def shard_offsets(K, shards):
    return [g * K // shards for g in range(shards)]


def shard_ks(K, shards):
    return sorted({0, K - 1} | {o - d for o in shard_offsets(K, shards)[1:] for d in (0, 1)})


SHARDED = [dict(pm("shard%d_K%d" % (n, K), K, shard_ks(K, n), SHARD_KERNEL, seed=21, lam=lam, group="sharded"), shards=n)
           for K, n, lam in ((8192, 2, 8.0), (8192, 8, 5.0), (8191, 3, 7.0))]

# batched: member i has its own goal, seed, lambda and needle
BATCH_K, BATCH_H, BATCH_A = 3000, 4, 3
BATCH_KS = [0, 2999, 2944]          # first sample; last sample of the ragged last tile; first sample of that tile
BATCH_KS_MOVED = [1500, 64, 2944]   # the others' needles moved, member 2's kept
BATCH_KS_MOVED2 = [0, 64, 100]      # member 0's as in the first step, member 1's as in the second, member 2's moved
BATCH_MOVES = [BATCH_KS, BATCH_KS_MOVED, BATCH_KS_MOVED2]
BATCH_LAMS = [4.5, 9.0, 10.0]
BATCH_SEEDS = [11, 12, 13]
BATCH_GOALS = [[1, 0, .5, 0, .75, 0], [-.5, 0, .25, 0, 1, 0], [.3, 0, -.8, 0, .1, 0]]
BATCH_KERNEL = ("mppi::k_rollout_pc_batch<3, 5, ", "")
BATCH = [pm("batch_m%d" % i, BATCH_K, sorted({ks[i] for ks in BATCH_MOVES}), BATCH_KERNEL, H=BATCH_H, a=BATCH_A, lam=BATCH_LAMS[i],
            seed=BATCH_SEEDS[i], goal=BATCH_GOALS[i], group="batched") for i in range(3)]

AUV_PC, AUV_GEN, AUV_BATCH = ("mppi::k_rollout_auv_pc<true>", ""), ("mppi::k_rollout_gen<0, 32, true>", ""), ("mppi::k_rollout_auv_pc_batch<true>", "")
# StaticQuatCost is ill-conditioned in fp32 next to the goal attitude (acos of a dot product within a few ulp of 1: a sample 1e-3 rad off has
# its attitude term wrong by percents), and a needle's 1/lambda turns 3 % of a runner-up's cost into 40 % of its weight — the fp32 reference's
# own error, not a kernel's. So the AUV cases run colder (the smallest gap is >= 14 lambda: runner-up weights <= 1e-6, condition (c)) and keep
# the goal positions at and near the origin, where x - goal loses nothing to the fp32 spacing of x.
AUV_GOALS = [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0] + [0.0] * 6, [0.5, -0.25, 0.125, 0.0, 0.0, 0.0, 1.0] + [0.0] * 6]
AUV_BATCH_MAX_K = 1024 * AUV_TILE  # a batch takes at most 1024 tiles per member (its finish combines a member's records in one pass): K = 65537 is refused
AUV_LAM, AUV_Q = {2 * AUV_TILE + 1: 0.6, AUV_BATCH_MAX_K: 0.18, 65537: 0.25}, 1e4
AUV_LONE = [auv("auv_%s_K%d" % (name, K), K, kern, AUV_LAM[K], AUV_Q, tuning=tun, goal=AUV_GOALS[0])
            for name, kern, tun in (("pc", AUV_PC, None), ("onewave", AUV_GEN, {"gen_one_wave": 1})) for K in (2 * AUV_TILE + 1, 65537)]
AUV_BATCH_SEEDS = [5, 6]
AUV_BATCHED = [[auv("auv_batch_K%d_m%d" % (K, i), K, AUV_BATCH, AUV_LAM[K], AUV_Q, seed=AUV_BATCH_SEEDS[i], goal=AUV_GOALS[i],
                    ks=[0, AUV_TILE - 1, AUV_TILE, K - 1][::1 - 2 * i], group="auv") for i in range(2)] for K in (2 * AUV_TILE + 1, AUV_BATCH_MAX_K)]

MODES = [pm("armed_K8192", 8192, [0, 8191], ("mppi::k_step_pc<3, 7, 3, true", ""), tuning={"armed_us": 20000, "armed_always": 1}, lam=10.0, group="modes"),
         pm("prelaunched_K8192", 8192, [0, 8191], ("mppi::k_step_pc<3, 7, 3, true", ""), tuning={"prelaunch": 1}, lam=10.0, group="modes")]

EVERY_CASE = LONE + SHARDED + BATCH + AUV_LONE + [c for pair in AUV_BATCHED for c in pair] + MODES


def ids(cases):
    return [c["id"] for c in cases]


# ---- a case's configuration on both sides -----------------------------------------------------------------------------------------------
def neutral_rexrov2():
    """rexrov2 with W = B in fp32 (density x volume = mass exactly) and no righting moment: at rest with no force nothing moves"""
    from mppi_tf_amd.auv import auv_task
    P = dict(auv_task(8)["auv"])
    P.update(volume=1.0, density=P["mass"], cob=list(P["cog"]))
    return P


def goal_of(case):
    if case["goal"] is not None:
        return np.asarray(case["goal"], F32)
    return np.asarray((GOAL3 + [0.25, 0])[:2 * case["a"]], F32)


def q_of(case):
    if case["model"] == "auv":
        return case["q"] * Q10
    s = 2 * case["a"]
    if not case["dense_q"]:
        return case["q"] * np.ones(s)
    B = np.random.default_rng(4).standard_normal((s, s))
    return (case["q"] * (np.eye(s) + 0.05 * (B + B.T))).astype(F32)


def config(case):
    """the keywords m.Handle and m.BatchHandle share for this case (no k, seed, goal, lam: a batch gives those per member)"""
    if case["model"] == "auv":
        return dict(tau=case["H"], s_dim=13, a_dim=6, dt=0.1, sigma=case["sigma"], auv=neutral_rexrov2(), Q=q_of(case), quat_cost=True,
                    action_cost=1, gamma=0.0, upsilon=1.0)
    a = case["a"]
    kw = dict(tau=case["H"], s_dim=2 * a, a_dim=a, dt=0.1, mass=1.0, sigma=case["sigma"], Q=q_of(case))
    if case["dense_q"]:
        kw["q_is_full"] = True
    if not case["cpp_form"]:
        kw.update(action_cost=1, gamma=0.0, upsilon=1.0)
    return kw


def handle(m, case, **kw):
    c = dict(config(case), k=case["K"], seed=case["seed"], goal=goal_of(case), lam=case["lam"], tuning=case["tuning"])
    if case["normalize"]:
        c["normalize_cost"] = True
    c.update(kw)
    h = m.Handle(**c)
    assert_kernel(h, case)
    return h


def assert_kernel(h, case):
    name, (start, end) = h.rollout_kernel_name(), case["kernel"]
    assert name.startswith(start) and name.endswith(end), "%s runs %s, not %s...%s" % (case["id"], name, start, end)
    return name


def problems(case):
    """-> (fp32, fp64) oracle problems of the case"""
    lam = float(F32(case["lam"]))  # the temperature the C-ABI carries
    if case["model"] == "auv":
        kw = dict(tau=case["H"], s=13, a=6, dt=0.1, lam=lam, sigma=case["sigma"], auv=neutral_rexrov2(), goal=goal_of(case), Q=q_of(case),
                  quat_cost=True, threads=0, action_cost=orc.ACTION_COST_PY, gamma=0.0, upsilon=1.0)
    else:
        a = case["a"]
        kw = dict(tau=case["H"], s=2 * a, a=a, dt=0.1, mass=1.0, lam=lam, sigma=case["sigma"], goal=goal_of(case), Q=q_of(case), threads=0)
        if not case["cpp_form"]:
            kw.update(action_cost=orc.ACTION_COST_PY, gamma=0.0, upsilon=1.0)
    return orc.Problem(**kw), orc.Problem(dtype=np.float64, **kw)


def oracle_noise(case, step=0):
    """the noise the case's step draws, as the oracle restates it (the CPU proof); an injected-noise case's own noise"""
    K, H, a = case["K"], case["H"], case["a"]
    if case["inject"]:
        return (np.random.default_rng(case["seed"]).standard_normal((K, H, a)) @ np.asarray(case["sigma"]).T).astype(F32)
    return orc.noise(case["seed"], step, 0, K, H, a, case["sigma"])


# ---- the fp64 reference -----------------------------------------------------------------------------------------------------------------
def softmin(c, lam, normalize):
    """-> (exp(-(c - beta)/lambda) [K], their sum) in fp64; normalize: (c - beta)/(max - beta) first (controller_base.py:468-474)"""
    d = np.asarray(c, np.float64) - np.min(c)
    if normalize:
        d = d / d.max()
    e = np.exp(-d / lam)
    return e, e.sum()


def reference(case, p32, p64, x, eps, k):
    """the step with U = -eps[k] on the noise eps [K, H, a]: the fp64 oracle's u, U' and shifted sequence, the needle's reference weight,
    the distance to the fp64 update without sample k, eta over the fp32 oracle's costs"""
    lam, nrm = float(F32(case["lam"])), case["normalize"]
    U = (-eps[k]).astype(F32)
    u, Ushift, c64 = p64.next_with_noise(x, U, eps, normalize=nrm)
    Uupd = np.vstack([u[None], Ushift[:-1]])
    e, eta = softmin(c64, lam, nrm)
    rest = np.delete(np.arange(eps.shape[0]), k)
    el, etal = softmin(c64[rest], lam, nrm)
    Uloo = U.astype(np.float64) + np.tensordot(el / etal, eps[rest].astype(np.float64), axes=(0, 0))
    u32, Ushift32, c32 = p32.next_with_noise(x, U, eps, normalize=nrm)
    cond = max(np.abs(u32 - u).max(), np.abs(Ushift32 - Ushift).max()) / case["scale"]  # how far the reference's own fp32 evaluation is from its fp64 one
    return dict(U=U, u=u, Uupd=Uupd, Ushift=Ushift, c64=c64, c32=c32, w=e[k] / eta, loo=np.abs(Uloo - Uupd).max() / case["scale"],
                eta=softmin(c32, lam, nrm)[1], cond=cond)


def assert_is_needle(case, k, ref):
    assert ref["w"] >= W_MIN, "case is no needle: %s k* = %d has reference weight %.6f < %g" % (case["id"], k, ref["w"], W_MIN)
    assert ref["cond"] <= COND_MAX, "case is no needle: %s k* = %d is ill-conditioned: the fp32 oracle's own update is %.3g from the fp64 one" % (case["id"], k, ref["cond"])
    assert ref["loo"] >= LOO_MIN, "case is no needle: %s k* = %d: losing it moves the reference update by %.3g < %g" % (case["id"], k, ref["loo"], LOO_MIN)


# ---- the GPU side -----------------------------------------------------------------------------------------------------------------------
class Lone:
    """debug items, sequence and stepping of a lone handle"""

    def __init__(self, m, h):
        self.m, self.h = m, h

    def dbg(self, what):
        return self.h.debug_get(what)

    def sequence(self):
        return self.h.get_action_sequence()


class Member:
    """... of member i of a batch"""

    def __init__(self, m, hb, i):
        self.m, self.hb, self.i = m, hb, i

    def dbg(self, what):
        return self.hb.debug_get(self.i, what)

    def sequence(self):
        return self.hb.get_action_sequences()[self.i]


def check(view, case, k, ref, u, seen):
    """everything the needle tests assert of one step (view: Lone / Member) that ran with U = ref["U"] on the noise ref was made of;
    `seen` collects the measured extremes"""
    m, tag, tol = view.m, "%s k* = %d" % (case["id"], k), U_TOL * case["scale"]
    c = view.dbg(m.DBG_COSTS)
    beta, eta = float(view.dbg(m.DBG_BETA)), float(view.dbg(m.DBG_ETA))
    if case["model"] == "auv":  # StaticQuatCost's bar (tests/test_auv_gpu.py): device acosf against libm
        np.testing.assert_allclose(c, ref["c32"], rtol=3e-6, atol=0, err_msg=tag)
    else:
        np.testing.assert_array_equal(c, ref["c32"], err_msg=tag)
        if case["cpp_form"]:
            assert c[k] == ref["c32"].min() and beta == c[k] and c[k] < 0, (tag, c[k], beta)
        else:
            assert c[k] == 0.0 and beta == 0.0, (tag, c[k], beta)
    assert_is_needle(case, k, ref)
    np.testing.assert_allclose(u, ref["u"], rtol=0, atol=tol, err_msg=tag + " u")
    np.testing.assert_allclose(view.dbg(m.DBG_U_UPDATED), ref["Uupd"], rtol=0, atol=tol, err_msg=tag + " U'")
    np.testing.assert_allclose(view.sequence(), ref["Ushift"], rtol=0, atol=tol, err_msg=tag + " shifted sequence")
    eta_err = abs(eta - ref["eta"]) / ref["eta"]
    print("%s: w_ref %.9f loo %.3g eta %.9g (rel err %.3g) max|dU'| %.3g" % (tag, ref["w"], ref["loo"], eta, eta_err,
                                                                               np.abs(view.dbg(m.DBG_U_UPDATED) - ref["Uupd"]).max() / case["scale"]))
    assert eta_err <= ETA_RTOL, "%s: eta %.9g against %.9g: %.3g relative" % (tag, eta, ref["eta"], eta_err)
    w = float(view.dbg(m.DBG_WEIGHTS)[k])
    assert abs(w - ref["w"]) <= W_RTOL * ref["w"], "%s: weight %.9g against %.9g" % (tag, w, ref["w"])
    seen["w"], seen["loo"], seen["eta"] = min(seen.get("w", 1.0), ref["w"]), min(seen.get("loo", np.inf), ref["loo"]), max(seen.get("eta", 0.0), eta_err)


def run_lone(m, case, step=None):
    """the three-call protocol for every needle of a lone-handle case; step(h, x) -> u runs one control step (default h.next)"""
    step = step or (lambda h, x: h.next(x))
    h = handle(m, case)
    p32, p64 = problems(case)
    x, seen = goal_of(case), {}
    if case["inject"]:
        eps0 = oracle_noise(case)
    else:
        s = h.get_step_counter()
        step(h, x)
        eps0 = h.debug_get(m.DBG_NOISE)
    for k in case["ks"]:
        h.set_action_sequence(-eps0[k])
        if case["inject"]:
            u = h.next_with_noise(x, eps0)
        else:
            h.set_step_counter(s)
            u = step(h, x)
            np.testing.assert_array_equal(h.debug_get(m.DBG_NOISE), eps0, err_msg="%s: the replayed step drew other noise" % case["id"])
        check(Lone(m, h), case, k, reference(case, p32, p64, x, eps0, k), u, seen)
    return h, seen
