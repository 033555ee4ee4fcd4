"""What the attitude-matrix tests share (test_attitude_oracle.py on the CPU, test_attitude_gpu.py on the GPU): start attitudes away from the
identity quaternion for the 13-state rollout kernels, the cases that launch every such kernel from them, and the oracle-side measures
(Euler angles of the visited states, octants, straddled folds) that prove the cases reach what they claim. A plain module in the manner
of learned_matrix_util.py, whose cases, rules and oracle side it reuses through spec(start=); nothing here touches a GPU.

Start attitudes (ATTITUDES): eight unit quaternions (fp32) named by the Euler angles (roll, pitch, yaw) that the oracle's own
orc.euler_from_quaternion gives for them (test_attitude_oracle.py asserts it), each with body rates of order 1 rad/s. The yaw angles are
the centres of the eight octants of atan2_pose (+-pi/8, +-3pi/8, +-5pi/8, +-7pi/8: sign x (|angle| > pi/2: the x < 0 fold) x (pi/4 <
|angle| < 3pi/4: the ay > ax fold)), except +-3.0 in place of +-7pi/8, whose trajectories cross the +-pi cut between steps; the roll
angles are a permutation of the same set (+3.0 and -1.75 among them), the pitch angles reach +-1.3.

NNAUVModelSpeed: the matrix's network moves the angular rates by ~3e-2 rad/s per step, so the 160 samples of a step stay within ~3e-3 rad
of each other and a wave diverges at a fold of atan2_pose only when the cloud sits on it. For every instance and every continuous fold
(|y| = |x|, x = 0, y = 0) there is therefore one AIMED case: its start yaw is bisected on the fp64 oracle (aim(): 40 halvings of a 1.2 rad
bracket) until the median yaw of the first tile's 64 samples at horizon step AIM_T of the first control step lies on the fold (yaw -3pi/4:
the ay > ax fold where x < 0 folds too; +pi/2; 0). The network is the matrix's own, unscaled: zeroing its three Euler rows moves more than
half of every case's costs (test_attitude_oracle.py), so no row is scaled either.

NNAUVModel: two attitudes (INVERTED: roll near pi; SKEW: ~120 degrees about a skew axis) whose four quaternion components are all larger
than 0.2 in magnitude, with both signs.

The Fossen model: every start attitude on k_rollout_auv_pc<DIAG>, k_rollout_gen<0, 32, DIAG> and, as the members of a batch,
k_rollout_auv_pc_batch<DIAG>; K = 129, H = 5, tests/golden's model_auv parameters and Sigma = 200 I (dense: 200 x DENSE_SIGMA6), as
tests/test_auv_gpu.py's auv_case; rk and the cost cycle over the attitudes (fossen_rk_cost), the quaternion cost's goal attitude on the far
hemisphere of every start.

The lock case: a unit quaternion never reaches the gimbal-lock branch of euler_from_quat (|r20| <= (1 - 4 eps)^2 < 1 - 1e-6), a caller's
x0 of norm ~1 + 1e-6 at pitch -+90 degrees does, at t = 0 only (the step normalises). lock_x0() gives such an x0 per sign: its two non-zero
components are the fp32 number in the middle of the twelve for which r20 lands in the branch, five ulp or more from either end, so the branch is taken
robustly (test_attitude_oracle.py moves both components by +-1 ulp). The fp64 oracle's branch is 1.8e-15 wide and its asin gives NaN here,
so these cases (H = 1) are held to the fp32 oracle alone.
"""
import functools

import numpy as np

import learned_matrix_util as lm
from oracle import oracle as orc

F32 = np.float32
PI = np.pi
PITCH_MAX = PI / 2 - 0.05
CUT_MARGIN = 1e-3
OCTANT_MIN = 64         # (sample, step) states per octant and kernel instance
SIDE_MIN = 16           # samples of one tile on each side of a fold
MOVED = 10 * 2e-5       # "matters": a quarter of the costs move by more than ten times the costs' bar
FOLDS = ("|y| = |x|", "x = 0", "y = 0")
K_FOSSEN, H_FOSSEN = 129, 5


def quat_of(roll, pitch, yaw):
    """(x, y, z, w) of R = Rz(yaw) Ry(pitch) Rx(roll), fp32: a construction only — what names an attitude is the oracle's Euler angles of it"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    q = np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])
    return (q / np.linalg.norm(q)).astype(F32)


# name -> ((roll, pitch, yaw), body rates (p, q, r) [rad/s])
ATTITUDES = {
    "yaw+3.0": ((PI / 8, 0.3, 3.0), (0.8, -0.6, 1.0)),           # yaw crosses +pi between steps
    "yaw-3.0": ((-PI / 8, -0.3, -3.0), (-0.8, 0.6, -1.0)),       # ... and -pi
    "roll+3.0": ((3.0, 0.5, 3 * PI / 8), (1.0, 0.6, -0.8)),      # roll crosses +pi
    "roll-1.75": ((-1.75, -0.6, -3 * PI / 8), (-1.0, 0.8, 0.6)),
    "pitch+1.3": ((3 * PI / 8, 1.3, 5 * PI / 8), (0.8, 0.3, 1.0)),
    "pitch-1.3": ((-3 * PI / 8, -1.3, -5 * PI / 8), (-0.8, -0.3, -1.0)),
    "inverted": ((-3.0, 0.7, PI / 8), (-1.0, 0.5, 0.8)),         # roll crosses -pi
    "skew120": ((5 * PI / 8, -0.5, -PI / 8), (0.6, -1.0, -0.8)),
}
NAMES = tuple(ATTITUDES)
INVERTED = np.array([0.93, 0.22, -0.21, -0.2])                    # roll near pi, every component beyond 0.2
SKEW = np.array([0.6, -0.5, 0.62, 0.0])                           # the axis of the 120 degree turn


def quaternion(name):
    if name == "nnauv_inverted":
        return (INVERTED / np.linalg.norm(INVERTED)).astype(F32)
    if name == "nnauv_skew120":
        ax = SKEW[:3] / np.linalg.norm(SKEW[:3])
        return np.r_[np.sin(PI / 3) * ax, np.cos(PI / 3)].astype(F32)
    return quat_of(*ATTITUDES[name][0])


def rates(name):
    return {"nnauv_inverted": (0.8, -0.6, 1.0), "nnauv_skew120": (-1.0, 0.8, 0.6)}.get(name) or ATTITUDES[name][1]


def start(name):
    """the `start` of learned_matrix_util.spec: the matrix's X13 with this attitude and these body rates"""
    x = lm.X13.copy()
    x[3:7], x[10:13] = quaternion(name), rates(name)
    return name, tuple(float(v) for v in x.astype(F32))


# a case that broke a condition gets another seed or multiplier here (never another bar): problem key -> dict(seed=, mult=)
ADJUST = {}


def spec(kind, hid, H, name, state=None, **kw):
    c = lm.spec(kind, hid, lm.depth(H), H=H, start=start(name) if state is None else (name, state), **kw)
    c.update(ADJUST.get(c["key"], {}))
    return c


# ---- NNAUVModelSpeed -----------------------------------------------------------------------------------------------------------------------
SPEED_FAMILIES = ("nnspeed_pc", "nnspeed32", "gen_nnspeed")
SPEED_H = (5, 9)


def speed_h(i):
    return SPEED_H[i % 2]


AIM_T = 3                                                      # the horizon step at which an aimed case's cloud sits on its fold
AIM_H = 5
AIMS = {"|y| = |x|": ("aim_diag", -3 * PI / 4), "x = 0": ("aim_x0", PI / 2), "y = 0": ("aim_y0", 0.0)}   # fold -> (name, the yaw of the fold)
AIM_ROLL_PITCH, AIM_RATES = (0.4, -0.3), (0.8, -0.6, 1.0)


def _aim_state(yaw):
    x = lm.X13.copy()
    x[3:7], x[10:13] = quat_of(AIM_ROLL_PITCH[0], AIM_ROLL_PITCH[1], yaw), AIM_RATES
    return tuple(float(v) for v in x.astype(F32))


@functools.lru_cache(None)
def aim(hid, dense, member, fold):
    """the start state whose first tile's median yaw at horizon step AIM_T of the first control step is the fold's, by bisection of the
    start yaw on the fp64 oracle (the trajectories depend on neither lambda nor the tuning)"""
    name, target = AIMS[fold]
    c = spec("nnspeed", hid, AIM_H, name, state=_aim_state(target), dense=dense, member=member)
    p64 = orc.Problem(dtype=np.float64, **lm.problem_kw(c, 1.0))
    U, eps = lm.inputs(c)[1], lm.noise(c, 0)[:lm.TILE]

    def miss(yaw0):
        x = np.array(_aim_state(yaw0), F32)
        states = np.concatenate([np.broadcast_to(x.astype(np.float64), (lm.TILE, 1, 13)), p64.rollout_cost(x, U, eps, traj=True)[1]], axis=1)
        return float(np.median(euler(states[:, AIM_T])[:, 2])) - target

    lo, hi = target - 0.9, target + 0.3   # (a yaw rate of 1 rad/s: ~0.3 rad in three steps)
    assert miss(lo) < 0.0 < miss(hi), (hid, dense, member, fold, miss(lo), miss(hi))
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if miss(mid) < 0.0 else (lo, mid)
    return _aim_state(lo)


def aimed(hid, dense, member, fold, **kw):
    return spec("nnspeed", hid, AIM_H, AIMS[fold][0], state=aim(hid, bool(dense), member, fold), dense=dense, member=member, **kw)


def speed_cases(fam, hid, dense):
    """one lone instance: every start attitude, H = 5 and 9 in turn; then the three aimed cases"""
    tuning = lm.lone_tuning(fam, "nnspeed", hid)
    return [spec("nnspeed", hid, speed_h(i), name, dense=dense, tuning=tuning) for i, name in enumerate(NAMES)] + [aimed(hid, dense, 0, f, tuning=tuning) for f in FOLDS]


def speed_instances():
    return [(fam, hid, dense) for fam in SPEED_FAMILIES for hid in (16, 32) for dense in (False, True)]


def batches(kind, hid, dense, names):
    """batches of lm.B members, each member at another start attitude (its own network, key, goal, lambda and Sigma scale, as the matrix's);
    the names in threes, the last batch filled from the front"""
    out = []
    for j, i0 in enumerate(range(0, len(names), lm.B)):
        H = speed_h(j) if kind == "nnspeed" else lm.EDGE_H
        tuning = {"mlp32_valu": 1} if (hid == 32 or kind == "nnspeed") else {}  # the lone kernel the batch mirrors
        out.append([spec(kind, hid, H, names[(i0 + i) % len(names)], dense=dense, tuning=tuning, member=i) for i in range(lm.B)])
    return out


def speed_batches(hid, dense):
    """... and one batch whose members are aimed at the three folds"""
    return batches("nnspeed", hid, dense, NAMES) + [[aimed(hid, dense, i, f, tuning={"mlp32_valu": 1}) for i, f in enumerate(FOLDS)]]


# ---- NNAUVModel ----------------------------------------------------------------------------------------------------------------------------
NNAUV_NAMES = ("nnauv_inverted", "nnauv_skew120")
NNAUV_FAMILIES = ("nnauv_pc", "nnauv32", "nnauv32_bx3", "gen_nnauv")


def nnauv_cases(fam):
    kind, hids, bx3, _, _ = lm.LONE[fam]
    return [spec(kind, hid, lm.EDGE_H, name, dense=dense, bx3=bx3, tuning=lm.lone_tuning(fam, kind, hid))
            for hid in hids for dense in (False, True) for name in NNAUV_NAMES]


def nnauv_batches():
    return [b for hid in (16, 32) for dense in (False, True) for b in batches("nnauv", hid, dense, NNAUV_NAMES + ("roll+3.0",))]


def learned_cases():
    """every learned case of this matrix, once per oracle problem: {problem key: case}"""
    every = [c for inst in speed_instances() for c in speed_cases(*inst)] + [c for fam in NNAUV_FAMILIES for c in nnauv_cases(fam)]
    every += [c for hid in (16, 32) for dense in (False, True) for b in speed_batches(hid, dense) for c in b] + [c for b in nnauv_batches() for c in b]
    out = {}
    for c in every:
        out.setdefault(c["key"], c)
    return out


# ---- the oracle's view of a case -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _visited(key):
    c = learned_cases()[key]
    mk = lm.make_case(c)
    p32, p64 = lm.problems(mk)
    x, U, out = mk["x"], mk["U"], []
    for step in range(lm.STEPS + (0 if c["member"] else 1)):
        eps = lm.noise(c, step)
        _, traj = p64.rollout_cost(x, U, eps, traj=True)
        out.append(np.concatenate([np.broadcast_to(np.asarray(x, np.float64), (c["K"], 1, 13)), traj], axis=1))
        U = p32.next_with_noise(x, U, eps)[1]
    return np.stack(out)


def visited(c):
    """the fp64 oracle's states of the case's steps, [step, K, H + 1, 13]: x0, then the state after each horizon step (the kernel takes the
    Euler angles of [:, :, :H])"""
    return _visited(c["key"])


def euler(states):
    """the oracle's Euler angles (roll, pitch, yaw) of states [..., 13], fp64"""
    q = np.asarray(states, np.float64)[..., 3:7]
    return orc.euler_from_quaternion(q.reshape(-1, 4)).reshape(q.shape[:-1] + (3,))


def sides(angle):
    """on which side of each fold of atan2_pose an angle lies: [3, ...] bools in the order of FOLDS (ay > ax, x < 0, y > 0)"""
    a = np.abs(angle)
    return np.stack([(a > PI / 4) & (a < 3 * PI / 4), a > PI / 2, angle > 0])


def octant(angle):
    s = sides(angle)
    return 4 * s[2].astype(int) + 2 * s[1].astype(int) + s[0].astype(int)


def straddles(angle):
    """angle [step, K, H] -> {fold: [(step, t, tile, samples on the smaller side)]} over t >= 1 and the tiles of 64 rollouts"""
    out = {f: [] for f in FOLDS}
    s = sides(angle)
    for f, fold in enumerate(FOLDS):
        for step in range(angle.shape[0]):
            for t in range(1, angle.shape[2]):
                for tile in range(lm.tiles(angle.shape[1])):
                    side = s[f, step, tile * lm.TILE:(tile + 1) * lm.TILE, t]
                    n = int(min(side.sum(), (~side).sum()))
                    if n >= SIDE_MIN:
                        out[fold].append((step, t, tile, n))
    return out


def moved(c, change):
    """the share of the samples whose fp64 cost moves by more than MOVED relative when the first layer is changed (change(W0) -> W0)"""
    mk = lm.make_case(c)
    net = mk["problem"][lm.model_kw(c)]
    other = dict(net, W=[change(np.array(net["W"][0]))] + list(net["W"][1:]))
    eps = lm.noise(c, 0)
    c64 = orc.Problem(dtype=np.float64, **mk["problem"]).rollout_cost(mk["x"], mk["U"], eps)
    d64 = orc.Problem(dtype=np.float64, **dict(mk["problem"], **{lm.model_kw(c): other})).rollout_cost(mk["x"], mk["U"], eps)
    return float((np.abs(d64 - c64) / np.abs(c64) > MOVED).mean())


def without_euler_rows(W0):
    W0[:3] = 0.0
    return W0


def with_qx_qy_swapped(W0):
    W0[[0, 1]] = W0[[1, 0]]   # NNAUVModel's input is x[3:]: rows 0..3 are the quaternion's
    return W0


# ---- the lock case -------------------------------------------------------------------------------------------------------------------------
LOCK_COMPONENT = F32(0.7071075)   # w and |y| of the x0 (y = w: pitch +90 degrees, y = -w: -90): the 7th of the 12 fp32 numbers (0.7071071 .. 0.7071078) that take the branch


def lock_x0(sign):
    """pitch = sign x pi/2 at norm 1 + 1.0e-6"""
    x = lm.X13.copy()
    x[3:7] = [0.0, sign * LOCK_COMPONENT, 0.0, LOCK_COMPONENT]
    x[10:13] = (0.8, -0.6, 1.0)
    return x.astype(F32)


def lock_case(fam, hid, sign):
    """-> the case and its make_case with lambda from the fp32 oracle (learned_matrix_util.lam_of's rule; the fp64 oracle gives NaN)"""
    c = lm.spec("nnspeed", hid, 1, H=1, tuning=lm.lone_tuning(fam, "nnspeed", hid), start=("lock%+d" % sign, tuple(float(v) for v in lock_x0(sign))))
    x, U = lm.inputs(c)
    c32 = np.sort(orc.Problem(dtype=F32, **lm.problem_kw(c, 1.0)).next_with_noise(x, U, lm.noise(c, 0))[2].astype(np.float64))
    lam = float(F32(c["mult"] * (c32[8] - c32[0])))
    h = dict(k=c["K"], tau=1, s_dim=13, a_dim=6, dt=0.1, lam=lam, sigma=lm.sigma_of(c), goal=lm.goal_of(c), Q=lm.q_of(c), seed=c["seed"],
             tuning=dict(c["tuning"]) or None, nnauv_speed=lm.net_of(c))
    return c, dict(handle=h, problem=lm.problem_kw(c, lam), x=x, U=U, lam=lam)


# ---- the Fossen model ----------------------------------------------------------------------------------------------------------------------
FOSSEN_RK = (1, 2, 4)
FOSSEN_COSTS = ("quadratic", "quat", "ellipse3d")
FOSSEN_KERNELS = {("pc", True): "mppi::k_rollout_auv_pc<true>", ("pc", False): "mppi::k_rollout_auv_pc<false>",
                  ("gen", True): "mppi::k_rollout_gen<0, 32, true>", ("gen", False): "mppi::k_rollout_gen<0, 32, false>",
                  ("batch", True): "mppi::k_rollout_auv_pc_batch<true>", ("batch", False): "mppi::k_rollout_auv_pc_batch<false>"}
SIGMA_SCALE = 200.0
GOAL_POS = (1.0, 2.0, -3.0)   # tests/test_auv_gpu.py's GOAL13
Q13 = np.array([100.0] * 3 + [10.0] * 4 + [1.0] * 6)
Q10 = np.diag([100.0] * 3 + [10.0] + [1.0] * 6) + 0.01
E3 = dict(normal=[0.0, np.sin(0.3), np.cos(0.3)], aVec=[1.0, 0.0, 0.0], axis=[2.0, 1.5], speed=1.0, m_state=50.0, m_vel=5.0)


# the nominal sequence is U_SCALE x randn: auv_case's 50, but 5 under the 3D-ellipse cost. That cost is ~100 per step here and the signed action
# cost lambda u' Sigma^-1 eps reaches +-300 at 50: sample costs then land near zero (10 of the 40 ellipse cases had one whose fp32 oracle
# value was 1.6e-6 .. 1.2e-5 relative from the fp64 oracle's), and a relative bar judges the case, not the kernel.
U_SCALE = {"quadratic": 50.0, "quat": 50.0, "ellipse3d": 5.0}
# the fp32 oracle's quat / ellipse3d costs within half their bar (rtol 3e-6 to the fp32 oracle) of the fp64 oracle's, relative: the kernel differs
# from the fp32 oracle by the rounding of acosf and sqrtf only, a fraction of the fp32 oracle's own distance (measured: at most 1.2e-6, at pitch 1.3)
FOSSEN_COND = 3e-6 / 2
# ONE control step (step counter 0): at auv_case's lambda = 1 the best sample holds the weight (costs of 1e3 .. 1e4), so U' = U + its noise, of
# scale 200, and a second step's action cost (+-1e4) throws the sample costs across zero. (For the same reason U' says little here, as in
# tests/test_auv_gpu.py: what judges these kernels is every sample's cost.)
FOSSEN_STEPS = 1


def fossen_rk_cost(i):
    """attitude i's (rk, cost): the nine pairs in turn, so eight attitudes see every rk and every cost"""
    return FOSSEN_RK[i % 3], FOSSEN_COSTS[(i + i // 3) % 3]


def fossen_sigma(diag):
    return (SIGMA_SCALE * (np.eye(6) if diag else lm.DENSE_SIGMA6)).astype(F32)


def fossen_goal(name):
    """the position of auv_case's goal; the attitude: the start turned by 0.9 rad about (1, 2, -2) / 3, NEGATED — the same rotation on the far
    hemisphere, <q, g_q> = -cos(0.45) < 0"""
    q = quaternion(name).astype(np.float64)
    d = np.r_[np.sin(0.45) * np.array([1.0, 2.0, -2.0]) / 3.0, np.cos(0.45)]
    g = -orc.quat_multiply(q, d)
    return np.r_[GOAL_POS, g / np.linalg.norm(g), np.zeros(6)].astype(F32)


def fossen_x0(name):
    x = np.array([0.5, -0.5, 0.2, 0.0, 0.0, 0.0, 1.0, 0.3, 0.0, -0.1, 0.0, 0.0, 0.0])
    x[3:7], x[10:13] = quaternion(name), rates(name)
    return x.astype(F32)


def fossen_cost_kw(cost, name):
    """-> (the handle's keywords, the oracle's) of the state cost, as tests/test_auv_gpu.py's auv_case"""
    if cost == "quadratic":
        kw = dict(goal=fossen_goal(name), Q=Q13)
        return kw, dict(kw)
    if cost == "quat":
        kw = dict(goal=fossen_goal(name), Q=Q10, quat_cost=True)
        return kw, dict(kw)
    kw = dict(ellipse3d=E3, goal=np.zeros(13, F32))   # (ElipseCost3D reads no goal; a batch takes one per member)
    return kw, dict(kw)


def fossen_case(params, i, diag, rk=None, cost=None):
    """start attitude i -> dict(name, rk, cost, seed, x, U, handle keywords (no tuning), oracle keywords (no dtype))"""
    name = NAMES[i]
    rk_i, cost_i = fossen_rk_cost(i)
    rk, cost = rk or rk_i, cost or cost_i
    hk, ok = fossen_cost_kw(cost, name)
    P = dict(params, rk=rk)
    seed = 700 + 10 * i + rk
    shared = dict(tau=H_FOSSEN, dt=0.1, lam=1.0, sigma=fossen_sigma(diag), auv=P)
    U = (U_SCALE[cost] * np.random.default_rng(seed).standard_normal((H_FOSSEN, 6))).astype(F32)
    return dict(name=name, rk=rk, cost=cost, seed=seed, x=fossen_x0(name), U=U, goal=np.asarray(hk["goal"], F32),
                handle=dict(shared, k=K_FOSSEN, s_dim=13, a_dim=6, seed=seed, **hk), problem=dict(shared, s=13, a=6, threads=0, **ok))


def fossen_batches():
    """(rk, cost) of the batches whose members are the eight start attitudes: a batch shares its model and its cost, so three batches
    show every rk and every cost to k_rollout_auv_pc_batch"""
    return list(zip(FOSSEN_RK, FOSSEN_COSTS))
