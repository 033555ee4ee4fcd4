"""What the tests of the soft-min update on GIVEN costs share (test_update_given_oracle.py on the CPU, test_update_given_gpu.py on the GPU):
mppi_update (Handle.update(cost, eps, U)) is the one entry point where the caller chooses every sample cost and every noise value, and it
ends in the finish kernels (k_finish_cols_cm by default, k_finish_cols with MPPI_TUNE_FINISH_GENERIC, k_combine_group above 1024 tiles).
A plain module: `m` is the mppi_tf_amd package each GPU test file's fixture gives.

The finish's record count is always nbp = record_pad(nb), a multiple of 128: tile b's record sits in slot record_slot(b, nbp), the slots
no tile owns hold pads (kPadBeta, eta 0, V 0) BETWEEN the real records. A thread of the finish takes slots t, t + 256, t + 512, t + 768.

Shapes. Point mass, H = 4, a in {1, 2, 3, 4}; for every j = 1..8 (nbp = 128 j) a full count K = 64 * 128 j (every slot a real tile) and a
ragged one K = 64 * (128 (j - 1) + 1) - 63 (the first tile of a new block of 128 slots holds ONE valid sample, every other slot of that
block is a pad). The action dimension walks 1..4 with j, two apart between full and ragged, so each a meets both. Three more: one fold
(K = 64 * 1025: k_combine_group, then the generic kernel), one wide (a = 4, H = 40: 160 finish workgroups, j = 3 ragged) and one 13-state
a = 6 handle (needle_util.auv, H = 3, j = 3 ragged: the records come from k_rollout_gen).

Cost families (finite fp32; lambda in {0.05, 1, 20}; U = update_tail_util.tree_U; eps N(0, 0.5^2), seeded per shape):
  spread:  1000 + U[0, 6 lambda): every sample carries comparable weight behind a large common offset;
  ties:    every cost 3.25: beta is everybody's, every weight 1 / K;
  stairs:  sample k costs (k // 64) * 10 lambda + U[0, lambda): tile t weighs e^-10t, from tile 9 on below 1e-38;
  needle:  cost 0 at k*, every other cost in [14 + ln K, 16 + ln K) * lambda, eps[k*] = +-1 alternating (update_tail_util.tree_records'
           numbers): all others together weigh e^-14, so losing, mis-weighting or misplacing k*'s record moves U' by O(1).
           k* is chosen by SLOT: a sample of the tile whose record sits in slot 0, 255, 256, 511, 512, 767, 768 and nbp - 1 wherever that
           slot exists and belongs to a real tile; and samples 0, 63, 64 and K - 1 (alone in the ragged tile).
Every shape gets spread and all its needles at lambda = 1; the other families and lambdas (and two needles at each other lambda) run at
j in {1, 3, 5, 7, 8}. K = 1 (j = 1 ragged) has neither a needle (nothing is left without it) nor stairs (one tile).

The bars of arg, exp and w (section `bars`) are derived from the fp32 operations that make them, not from what a GPU returned.
"""
import functools

import numpy as np

import needle_util as nu
import update_tail_util as ut
from needle_util import F32, U_TOL, ETA_RTOL
from oracle import oracle as orc

H = 4
LAMS = (0.05, 1.0, 20.0)
J_ALL = tuple(range(1, 9))
J_MORE = (1, 3, 5, 7, 8)
SLOT_TARGETS = (0, 255, 256, 511, 512, 767, 768)  # ... and nbp - 1: the edges of a thread's four slot blocks
TINY = 1e-30        # exp and w are compared where the fp64 value is at least this, and must be at most this elsewhere (stairs only)
STAIRS_MIN_NB = 16  # stairs needs tiles that underflow: tile 9 on weighs less than 1e-38
record_pad, slot_tile = ut.record_pad, ut.slot_tile


def record_slot(b, nbp):
    """mppi_device.hip.h: the slot of tile b's record among nbp"""
    return (b & 7) * (nbp >> 3) + (b >> 3)


# ---- the shapes -----------------------------------------------------------------------------------------------------------------------------
def shape(id, K, a, Hs=H, model="pm", j=None, ragged=False, more=False):
    nb = (K + 63) // 64
    return dict(id=id, K=K, H=Hs, a=a, model=model, j=j, ragged=ragged, more=more, nb=nb, nbp=record_pad(nb))


def k_full(j):
    return 64 * 128 * j


def k_ragged(j):
    return 64 * (128 * (j - 1) + 1) - 63


def a_of(j, ragged):
    return (j - 1 + 2 * int(ragged)) % 4 + 1


MATRIX = [shape("j%d_%s_a%d" % (j, "ragged" if r else "full", a_of(j, r)), k_ragged(j) if r else k_full(j), a_of(j, r), j=j, ragged=r, more=j in J_MORE)
          for j in J_ALL for r in (False, True)]
FOLD = shape("fold_1025_tiles_a3", 64 * 1025, 3)
WIDE = shape("wide_H40_a4_j3_ragged", k_ragged(3), 4, Hs=40, j=3, ragged=True)
AUV = shape("auv_H3_a6_j3_ragged", k_ragged(3), 6, Hs=3, model="auv", j=3, ragged=True)
SHAPES = MATRIX + [FOLD, WIDE, AUV]
SHAPE_IDS = [s["id"] for s in SHAPES]


def needles(sh):
    """-> [(k*, slot of its tile)]: by slot first, then samples 0, 63, 64 and K - 1; none at K = 1"""
    K, nb, nbp = sh["K"], sh["nb"], sh["nbp"]
    if K == 1:
        return []
    out = []
    for s in SLOT_TARGETS + (nbp - 1,):
        b = slot_tile(s, nbp) if s < nbp else nb
        if b < nb:  # a real tile: one of its valid samples (the ragged tile has one)
            out.append(min(64 * b + s % 64, K - 1))
    out += [k for k in (0, 63, 64, K - 1) if k < K]
    ks = sorted(set(out), key=out.index)
    return [(k, record_slot(k // 64, nbp)) for k in ks]


def cases(sh):
    """the (family, lambda, k*) of a shape"""
    out = [("spread", 1.0, None)] + [("needle", 1.0, k) for k, _ in needles(sh)]
    if sh["more"]:
        nd = needles(sh)
        for lam in LAMS:
            out += [("ties", lam, None)] + ([("stairs", lam, None)] if sh["nb"] >= STAIRS_MIN_NB else [])
            if lam != 1.0:
                out += [("spread", lam, None)] + [("needle", lam, k) for k, _ in (nd[:1] + nd[-1:])]
    return out


def case_id(case):
    return "%s lambda %g%s" % (case[0], case[1], "" if case[2] is None else " k* = %d" % case[2])


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def noise(K, Hs, a):
    """eps [K, H, a] ~ N(0, 0.5^2), the same for every case of a shape (the needle overwrites row k*)"""
    eps = (0.5 * np.random.default_rng(31 * K + 7 * Hs + a).standard_normal((K, Hs, a))).astype(F32)
    eps.setflags(write=False)
    return eps


def inputs(sh, case):
    """-> (cost [K], eps [K, H, a], U [H, a], lambda as the C-ABI carries it); eps is shared and read-only unless the case is a needle"""
    family, lam, k = case
    K, Hs, a = sh["K"], sh["H"], sh["a"]
    lam32 = float(F32(lam))
    rng = np.random.default_rng([K, Hs * a, int(1000 * lam), 0 if k is None else k + 1, ("spread", "ties", "stairs", "needle").index(family)])
    eps = noise(K, Hs, a)
    if family == "spread":
        cost = 1000.0 + rng.uniform(0.0, 6.0 * lam32, K)
    elif family == "ties":
        cost = np.full(K, 3.25)
    elif family == "stairs":
        cost = (np.arange(K) // 64) * 10.0 * lam32 + rng.uniform(0.0, lam32, K)
    else:
        cost = rng.uniform(14.0 + np.log(K), 16.0 + np.log(K), K) * lam32
        cost[k] = 0.0
        eps = eps.copy()
        eps[k] = np.where(np.arange(Hs * a) % 2 == 0, 1.0, -1.0).reshape(Hs, a)
    cost = cost.astype(F32)
    assert np.isfinite(cost).all()
    return cost, eps, ut.tree_U(Hs, a), lam32


def reference(cost, eps, U, lam32, dtype=np.float64, without=None):
    """orc.update in `dtype`; without: leave that sample out"""
    if without is not None:
        cost, eps = np.delete(cost, without), np.delete(eps, without, axis=0)
    return orc.update(cost, eps, U, lam32, dtype=dtype)


# ---- the bars -------------------------------------------------------------------------------------------------------------------------------
# The device makes arg = fl(fl(-1 / lambda) * fl(c - beta)) (k_weights): three fp32 roundings of relative size u = 2^-24 each on the exact
# -(c - beta) / lambda, so |arg - arg64| <= ((1 + u)^3 - 1) |arg64|: the bar grows with |arg|. exp = expf(arg): the error of the argument
# passes through exp as expm1(that), and expf itself is held to EXP_ULPS ulp (HIP documents 1 ulp for expf; glibc's is below 1).
# w = fl(exp / eta): the same, the bar the tests hold eta to (ETA_RTOL), and one more rounding.
U32 = 2.0 ** -24
EXP_ULPS = 3


def arg_bar(arg64):
    """absolute, per sample"""
    return ((1.0 + U32) ** 3 - 1.0) * np.abs(arg64) * (1.0 + 1e-9)


def exp_rbar(arg64):
    """relative, per sample"""
    return np.expm1(arg_bar(arg64)) + EXP_ULPS * 2.0 * U32


def w_rbar(arg64):
    return exp_rbar(arg64) + ETA_RTOL + U32


def unew_bar(wn, Unew):
    """|Unew - (U + wn)| per element: Unew = fl(U + fl(V / eta)) from the kernel's double quotient, wn = fl(fl(V) / fl(eta)) from the rounded
    record: the roundings of V, of eta and of the two quotients act on wn, the rounding of the sum on Unew"""
    return U32 * (4.0 * np.abs(wn) + np.abs(Unew)) * (1.0 + 1e-6)


def distances(got, ref):
    """what the docstrings record: got (fp32 oracle or GPU) against the fp64 reference; exp where the reference is at least TINY"""
    arg64, e64 = ref["arg"], ref["exp"]
    big = e64 >= TINY
    nz = arg64 != 0
    return dict(Unew=np.abs(got["Unew"] - ref["Unew"]).max(), nabla=abs(float(got["nabla"]) - ref["nabla"]) / ref["nabla"],
                arg=(np.abs(got["arg"][nz] - arg64[nz]) / np.abs(arg64[nz])).max() if nz.any() else 0.0,
                exp=(np.abs(got["exp"][big] - e64[big]) / e64[big]).max(),
                arg_of_bar=(np.abs(got["arg"] - arg64)[nz] / arg_bar(arg64)[nz]).max() if nz.any() else 0.0,
                exp_of_bar=(np.abs(got["exp"][big] - e64[big]) / e64[big] / exp_rbar(arg64[big])).max())


def worse(seen, d):
    for key, v in d.items():
        seen[key] = max(seen.get(key, 0.0), float(v))
    seen["n"] = seen.get("n", 0) + 1


def limits(a):
    """a band of its own per action dimension, narrow enough that every element of U' is clamped: a limit read at the wrong index shows"""
    lo = np.array([0.01, -0.02, 0.03, -0.04, 0.05, -0.06][:a], F32)
    return lo, lo + F32(0.001)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------------
KEYS_BITS = ("beta", "nabla", "wn", "Unew", "arg", "exp", "w")
AUV_POSE = np.array([0.5, -0.4, 0.3] + list(nu.AUV_GOALS[0][3:]), F32)


def auv_case(K, Hs, lam=1.0, seed=1):
    return dict(nu.auv("update_given_auv", K, ("", ""), lam, 1.0, seed=seed, goal=nu.AUV_GOALS[0], ks=[]), H=Hs)


def handle(m, sh, lam, **tuning):
    """the shape's handle at temperature lam, one control step behind it: the sequence and the step counter an update must leave alone"""
    K, Hs, a = sh["K"], sh["H"], sh["a"]
    if sh["model"] == "auv":
        h = nu.handle(m, auv_case(K, Hs, lam), tuning=tuning or None)
        x = AUV_POSE
    else:
        goal = (nu.GOAL3 + [0.25, 0])[:2 * a]
        h = m.Handle(k=K, tau=Hs, s_dim=2 * a, a_dim=a, dt=0.1, mass=1.0, lam=lam, sigma=0.25 * np.eye(a), goal=goal, seed=3, tuning=tuning or None)
        x = np.zeros(2 * a, F32)
    h.next(x)
    return h


def held(h):
    return h.get_step_counter(), h.get_action_sequence()


def assert_held(h, before, tag):
    step, seq = held(h)
    assert step == before[0], "%s: update() moved the step counter from %d to %d" % (tag, before[0], step)
    np.testing.assert_array_equal(seq, before[1], err_msg=tag + ": update() changed the stored sequence")


def check_update(sh, case, rf, rg, inp, ref, seen):
    """one update() of the default handle (rf) and of its finish_generic twin (rg) against each other and against the fp64 oracle (ref)"""
    tag = "%s %s" % (sh["id"], case_id(case))
    cost, eps, U, lam32 = inp
    for key in KEYS_BITS:
        np.testing.assert_array_equal(rf[key], rg[key], err_msg="%s: %s of the fast path against the generic kernel" % (tag, key))
    d = distances(rf, ref)
    d["Unew_wn"] = np.abs(U.astype(np.float64) + rf["wn"] - ref["Unew"]).max()
    d["split_of_bar"] = (np.abs(rf["Unew"].astype(np.float64) - (U.astype(np.float64) + rf["wn"])) / unew_bar(rf["wn"], rf["Unew"])).max()
    print("%s: beta %.9g | nabla rel %.3g | max|dUnew| %.3g | max|d(U + wn)| %.3g | Unew - (U + wn) %.2f of its bar | arg rel %.3g (%.2f of its bar) "
          "| exp rel %.3g (%.2f of its bar)" % (tag, rf["beta"], d["nabla"], d["Unew"], d["Unew_wn"], d["split_of_bar"], d["arg"], d["arg_of_bar"],
                                                d["exp"], d["exp_of_bar"]))
    worse(seen, d)
    assert rf["beta"] == F32(ref["beta"]) == cost.min(), "%s: beta %.9g against %.9g" % (tag, rf["beta"], ref["beta"])
    assert d["nabla"] <= ETA_RTOL, "%s: nabla %.9g against %.9g: %.3g relative" % (tag, rf["nabla"], ref["nabla"], d["nabla"])
    np.testing.assert_allclose(rf["Unew"], ref["Unew"], rtol=0, atol=U_TOL, err_msg=tag + " Unew")
    np.testing.assert_allclose(U.astype(np.float64) + rf["wn"], ref["Unew"], rtol=0, atol=U_TOL, err_msg=tag + " U + wn")
    assert d["split_of_bar"] <= 1.0, "%s: Unew is %.2f bars from U + wn" % (tag, d["split_of_bar"])
    # arg everywhere; exp and w where the fp64 value is at least TINY, at most TINY elsewhere — and only stairs has such samples
    arg64 = ref["arg"]
    bad = np.flatnonzero(np.abs(rf["arg"] - arg64) > arg_bar(arg64))
    assert bad.size == 0, "%s: arg of sample %d is %.9g against %.12g, bar %.3g" % (tag, bad[0], rf["arg"][bad[0]], arg64[bad[0]], arg_bar(arg64)[bad[0]])
    for key, rbar in (("exp", exp_rbar(arg64)), ("w", w_rbar(arg64))):
        v64, got = ref[key], rf[key].astype(np.float64)
        big = v64 >= TINY
        assert case[0] == "stairs" or big.all(), "%s: %d samples have an fp64 %s below %g" % (tag, (~big).sum(), key, TINY)
        bad = np.flatnonzero(big & (np.abs(got - v64) > rbar * v64))
        assert bad.size == 0, "%s: %s of sample %d is %.9g against %.12g (%.3g relative, bar %.3g)" % (
            tag, key, bad[0], got[bad[0]], v64[bad[0]], abs(got[bad[0]] - v64[bad[0]]) / v64[bad[0]], rbar[bad[0]])
        assert (got[~big] <= TINY).all() and (got >= 0).all(), "%s: %s where the reference is below %g" % (tag, key, TINY)
