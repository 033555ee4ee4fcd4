"""What the update-tail tests share (test_update_tail_oracle.py on the CPU, test_update_tail_gpu.py on the GPU): what runs after the
tile records — the record tree at every fold depth, and the options of the update (action limits, sequence filter) on the paths that apply
it. A plain module: `m` is the mppi_tf_amd package each GPU test file's fixture gives.

A. The record tree. mppi_shard_finish combines n row-major records (beta_b, eta_b, V_b[HA]); above 1024 it folds them 16:1 per level
(k_combine_group) until at most 1024 remain (column_combine in k_finish_cols). Synthetic records reach every depth without a rollout:
  plain:   beta_b uniform in [0, 2 lambda), eta_b in [1, 64], |V_b| <= 1, V_b leaning on beta_b a different way in each column — every
           record carries comparable weight and U' - U is O(0.1) per column at every n, so a wrong stride, weight or column shows;
  needle:  record b* has beta = 0, eta = 1, V = v* (entries +-1); every other record has beta_b >= (14 + ln n) lambda, so all of them
           together weigh <= 64 e^-14 = 5e-5 — losing, mis-weighting or misplacing b* moves U' by O(1).
The reference is the formula in fp64: beta = min beta_b, r_b = exp(-(beta_b - beta)/lambda), eta = sum r_b eta_b, U' = U + sum r_b V_b / eta.

B. Limits and filter. Three control steps per case; the reference is clip(U'_raw, lo, hi) per action column on the fp64 oracle's unclipped
U'_raw for the noise the step drew, u = U'[0], and the stored sequence savgol_filter(shift(U')) in fp64 (not re-clipped: controller_base.py
filters after _next). The limits are distinct per action and asymmetric; each case's x, lo and hi are chosen here so that the conditions of
`option_conditions` hold — then a clip left out, indexed c // H, or applied after the filter is 100 bars away from the reference.
"""
import numpy as np

import needle_util as nu
from needle_util import F32, U_TOL, ETA_RTOL
from oracle import oracle as orc

# ---- A1: synthetic records ------------------------------------------------------------------------------------------------------------------
TREE_LAM = 0.7
TREE_LEVELS = {1: 0, 1023: 0, 1024: 0, 1025: 1, 16384: 1, 16385: 2, 262145: 3}  # n -> fold levels before the finish
TREE_N = sorted(TREE_LEVELS)
TREE_LOO_MIN = 100 * U_TOL
TREE_COND_MAX = U_TOL / 4
kGroup, kOnePass = 16, 1024


def tree_levels(n):
    """fold levels launch_finish runs for n records: 16:1 while more than 1024 remain"""
    lv = 0
    while n > kOnePass:
        n, lv = (n + kGroup - 1) // kGroup, lv + 1
    return lv


def record_pad(nb):
    """record slots of a handle with nb tiles (mppi_device.hip.h): a multiple of 128"""
    return (nb + 127) // 128 * 128


def tree_handle_shape(n):
    """-> (K, H, a) of the point-mass handle that finishes n records: its scratch holds ceil(nbp/16) folded records for its own
    nbp = record_pad(ceil(K/64)) slots, so K grows with n; the three-level handle is only created and finished, so it is as thin as can be"""
    if n == 262145:
        return 2 ** 24 + 1, 1, 1
    return (192 if n <= kOnePass else 64 * n), 2, 2


def tree_fits(n, K):
    """mppi_shard_finish's rule: n <= 1024, or ceil(n/16) <= ceil(nbp/16)"""
    nbp = record_pad((K + 63) // 64)
    return n <= kOnePass or (n + kGroup - 1) // kGroup <= (nbp + kGroup - 1) // kGroup


def tree_needles(n):
    """b*: first and last record; the last and first index of a level-1, level-2 and level-3 group"""
    return sorted({b for b in (0, n - 1, 15, 16, 255, 256, 4095, 4096) if 0 <= b < n}) if n > 1 else []


def tree_U(H, a):
    """the non-zero nominal sequence the records update"""
    return (0.25 + 0.125 * np.arange(H * a).reshape(H, a) * (-1.0) ** np.arange(a)).astype(F32)


def tree_records(n, HA, bstar=None):
    """[n, 2 + HA] fp32 records: the plain population, or the needle population around record bstar"""
    rng = np.random.default_rng(1000 + n if bstar is None else 7 * n + bstar)
    lam = float(F32(TREE_LAM))
    rec = np.empty((n, 2 + HA), F32)
    rec[:, 1] = 1.0 + 63.0 * rng.uniform(0.0, 1.0, n) ** 16  # in [1, 64], mostly small: U' - U = sum r V / sum r eta stays O(0.1)
    rec[:, 2:] = rng.uniform(-1.0, 1.0, (n, HA))
    if bstar is None:
        rec[:, 0] = rng.uniform(0.0, 2.0 * lam, n)
        # V leans on beta, each column its own way: the weighted mean stays O(0.1) however many records average, and differs per column
        lean = (-1.0) ** np.arange(HA) * (1.0 - 0.5 * np.arange(HA) / HA)
        rec[:, 2:] = 0.5 * rec[:, 2:] + 0.5 * lean * (1.0 - rec[:, :1] / lam)
    else:
        rec[:, 0] = rng.uniform(14.0 + np.log(n), 16.0 + np.log(n), n) * lam
        rec[bstar, 0], rec[bstar, 1] = 0.0, 1.0
        rec[bstar, 2:] = np.where(np.arange(HA) % 2 == 0, 1.0, -1.0)
    return rec


def tree_reference(rec, U, dtype=np.float64, without=None):
    """the combine + update of the records in `dtype` -> (beta, eta, U'); without: leave that record out"""
    lam = dtype(F32(TREE_LAM))  # the temperature the C-ABI carries
    r = np.asarray(rec, dtype)
    if without is not None:
        r = np.delete(r, without, axis=0)
    beta = r[:, 0].min()
    w = np.exp(-(r[:, 0] - beta) / lam).astype(dtype)
    eta = (w * r[:, 1]).sum(dtype=dtype)
    V = (w[:, None] * r[:, 2:]).sum(axis=0, dtype=dtype)
    return beta, eta, np.asarray(U, dtype) + (V / eta).reshape(np.shape(U))


def tree_proof(n, bstar, rec, U):
    """the CPU conditions of one (n, b*): -> (leave-one-out distance, fp32 / fp64 distance, the needle's weight)"""
    _, eta, Uu = tree_reference(rec, U)
    loo = np.abs(tree_reference(rec, U, without=bstar)[2] - Uu).max()
    cond = np.abs(tree_reference(rec, U, dtype=np.float32)[2].astype(np.float64) - Uu).max()
    return loo, cond, 1.0 / eta


def assert_tree_case(n, bstar, rec, U):
    loo, cond, w = tree_proof(n, bstar, rec, U)
    assert loo >= TREE_LOO_MIN, "n = %d b* = %d: losing the needle record moves U' by %.3g < %g" % (n, bstar, loo, TREE_LOO_MIN)
    assert cond <= TREE_COND_MAX, "n = %d b* = %d: the fp32 evaluation is %.3g from the fp64 one" % (n, bstar, cond)
    return loo, cond, w


def shifted(Uupd):
    """mShift + mInit0: drop row 0, append a zero row"""
    return np.concatenate([Uupd[1:], np.zeros((1, Uupd.shape[1]), Uupd.dtype)])


def tree_handle(m, n):
    K, H, a = tree_handle_shape(n)
    assert tree_fits(n, K)
    goal = (nu.GOAL3 + [0.25, 0])[:2 * a]
    return m.Handle(k=K, tau=H, s_dim=2 * a, a_dim=a, dt=0.1, mass=1.0, lam=TREE_LAM, sigma=0.5 * np.eye(a), goal=goal, seed=1), H, a


def run_tree(m, h, H, a, n, bstar, seen):
    """one mppi_shard_finish of n synthetic records on handle h, against the fp64 formula"""
    import torch
    rec, U = tree_records(n, H * a, bstar), tree_U(H, a)
    if bstar is not None:
        assert_tree_case(n, bstar, rec, U)
    beta, eta, Uu = tree_reference(rec, U)
    h.set_action_sequence(U)
    recs, u = torch.tensor(rec.ravel(), device="cuda"), torch.zeros(a, device="cuda")
    torch.cuda.synchronize()  # the upload ran on torch's stream, the finish runs on the handle's
    h.shard_finish(recs.data_ptr(), n, u.data_ptr())
    h.synchronize()
    u, Ud, seq = u.cpu().numpy(), h.debug_get(m.DBG_U_UPDATED), h.get_action_sequence()
    tag = "n = %d (%d levels) %s" % (n, tree_levels(n), "plain" if bstar is None else "b* = %d" % bstar)
    eta_err, dU = abs(float(h.debug_get(m.DBG_ETA)) - eta) / eta, max(np.abs(Ud - Uu).max(), np.abs(u - Uu[0]).max())
    print("%s: eta rel err %.3g max|dU'| %.3g" % (tag, eta_err, dU))
    assert float(h.debug_get(m.DBG_BETA)) == beta, (tag, h.debug_get(m.DBG_BETA), beta)
    assert eta_err <= ETA_RTOL, "%s: eta %.9g against %.9g" % (tag, h.debug_get(m.DBG_ETA), eta)
    np.testing.assert_allclose(Ud, Uu, rtol=0, atol=U_TOL, err_msg=tag + " U'")
    np.testing.assert_allclose(u, Uu[0], rtol=0, atol=U_TOL, err_msg=tag + " u")
    np.testing.assert_array_equal(u, Ud[0], err_msg=tag + " u is U'[0]")
    np.testing.assert_array_equal(seq, shifted(Ud), err_msg=tag + " the stored sequence is the shift of U'")
    seen["eta"], seen["dU"] = max(seen.get("eta", 0.0), eta_err), max(seen.get("dU", 0.0), dU)


# ---- B: limits and filter ---------------------------------------------------------------------------------------------------------------------
STEPS = 3
MARGIN = 100  # how many bars every condition holds by


def savgol_rows(H, window, order):
    """the fp64 Savitzky-Golay coefficient rows of savgol_filter(mode='interp'): row t weighs the window [start[t], start[t] + window);
    the edge rows evaluate the edge window's polynomial off its centre (scipy's `pos`)"""
    from scipy.signal import savgol_coeffs
    hw = window // 2
    start = np.clip(np.arange(H) - hw, 0, H - window)
    rows = np.stack([savgol_coeffs(window, order, pos=int(t - start[t]), use="dot") for t in range(H)])
    return rows, start


def savgol(seq, window, order):
    from scipy.signal import savgol_filter
    return savgol_filter(np.asarray(seq, np.float64), window, order, deriv=0, delta=1.0, axis=0)


def filter_bar(H, window, order, Uupd):
    """the fp32 rounding of the weights and of the inputs of the filter's sum: 4 * 2^-24 * max_t sum_i |r[t, i]| * max|U'|, at least 2e-6"""
    rows, _ = savgol_rows(H, window, order)
    return max(2e-6, 4 * 2.0 ** -24 * np.abs(rows).sum(axis=1).max() * np.abs(Uupd).max())


def clip_cols(Uraw, lo, hi):
    """clip_act: action column j of U' [H, a] to [lo[j], hi[j]]"""
    return np.clip(Uraw, np.asarray(lo, np.float64), np.asarray(hi, np.float64))


def clip_transposed(Uraw, lo, hi):
    """the wrong clip: flat column c limited by action c // H instead of c % a"""
    H, a = Uraw.shape
    j = (np.arange(H * a) // H).reshape(H, a)
    return np.clip(Uraw, np.asarray(lo, np.float64)[j], np.asarray(hi, np.float64)[j])


def option_reference(case, Uraw):
    """-> (U', the stored sequence) in fp64 for the unclipped update Uraw: clip, then shift, then filter (never re-clipped)"""
    Uu = clip_cols(Uraw, case["lo"], case["hi"]) if case["limits"] else np.asarray(Uraw, np.float64)
    seq = shifted(Uu)
    return Uu, (savgol(seq, *case["filter"]) if case["filter"] else seq)


def option_conditions(case, Uraw, tag=""):
    """the conditions that make a step of the case a test of its options, on the fp64 unclipped update Uraw; -> the margins, in bars"""
    H, a = Uraw.shape
    tol = U_TOL * case["scale"]
    Uu, seq = option_reference(case, Uraw)
    out = {}
    if case["limits"]:
        lo, hi = np.asarray(case["lo"], np.float64), np.asarray(case["hi"], np.float64)
        assert len(set(np.abs(np.concatenate([lo, hi])))) == 2 * a, "the limits are distinct per action and asymmetric"
        above, below = (Uraw - hi).max(axis=0), (lo - Uraw).max(axis=0)
        inside = np.minimum(Uraw - lo, hi - Uraw).max(axis=0)
        out["above"], out["below"], out["inside"] = above.min() / tol, below.min() / tol, inside.min() / tol
        for name in ("above", "below", "inside"):
            assert out[name] >= MARGIN, "%s: an action column of U'_raw has no entry %s the limits by %d bars (%.3g)" % (tag, name, MARGIN, out[name])
    wrong = {}
    if case["filter"]:
        bar = filter_bar(H, *case["filter"], Uu)
        out["filter"] = np.abs(seq - shifted(Uu)).max() / bar
        assert out["filter"] >= MARGIN, "%s: the filter moves the sequence by %.3g bars only" % (tag, out["filter"])
        wrong["no filter"] = np.abs(seq - shifted(Uu)).max() / bar
        if case["limits"]:
            out["outside"] = max((seq - hi).max(), (lo - seq).max()) / bar
            assert out["outside"] >= MARGIN, "%s: no filtered entry lies outside the limits (%.3g bars): the order of clip and filter would not show" % (tag, out["outside"])
            wrong["no clip"] = np.abs(savgol(shifted(Uraw), *case["filter"]) - seq).max() / bar
            wrong["filter before clip"] = np.abs(clip_cols(savgol(shifted(Uraw), *case["filter"]), lo, hi) - seq).max() / bar
            if a > 1:
                wrong["clip by c // H"] = np.abs(savgol(shifted(clip_transposed(Uraw, lo, hi)), *case["filter"]) - seq).max() / bar
    elif case["limits"]:
        wrong["no clip"] = np.abs(Uraw - Uu).max() / tol
        if a > 1:
            wrong["clip by c // H"] = np.abs(clip_transposed(Uraw, lo, hi) - Uu).max() / tol
    for name, d in wrong.items():
        assert d >= MARGIN, "%s: the wrong reference '%s' is only %.3g bars away" % (tag, name, d)
        out["wrong: " + name] = d
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# Every row runs warm (lambda = 1 against cost differences of a few units) and quiet (sigma = 0.1): the update is a smooth pull towards the
# goal that is strongest in row 0 and fades towards the end of the horizon, the same way in every step. Both limits of an action lie on the
# side the pull goes to, at fixed fractions of the first step's range: row 0 ends beyond the far limit in every step, the fresh last row
# (0 + a small pull) stays short of the near one, and the row that was clipped to the near limit one step earlier has moved just inside.
def mlp_weights(s, a, hid, n_hidden, seed):
    """synthetic weights of a learned model (tests/test_parity_gpu.py: U(-1/sqrt(fan_in), 1/sqrt(fan_in)), last layer x0.1)"""
    rng = np.random.default_rng(seed)
    dims = [s + a] + [hid] * n_hidden + [s]
    W = [rng.uniform(-1, 1, (dims[i], dims[i + 1])) / np.sqrt(dims[i]) for i in range(n_hidden + 1)]
    b = [rng.uniform(-1, 1, dims[i + 1]) / np.sqrt(dims[i]) for i in range(n_hidden + 1)]
    W[-1] *= 0.1
    b[-1] *= 0.1
    return dict(W=[w.astype(F32) for w in W], b=[v.astype(F32) for v in b],
                xmean=rng.uniform(-0.1, 0.1, s + a).astype(F32), xstd=rng.uniform(0.8, 1.2, s + a).astype(F32),
                ymean=rng.uniform(-0.01, 0.01, s).astype(F32), ystd=rng.uniform(0.8, 1.2, s).astype(F32))


PM_OFF = [1.0, 0.0, -0.8, 0.0, 0.6, 0.0, -0.5, 0.0]  # x - goal of the point-mass rows: at rest, away from the goal a different way per axis
LIMITS, FILTER = "limits", "filter"


def option_sets(base, *sets):
    """the cases of one row: (LIMITS,), (FILTER, w, p) or (LIMITS, FILTER, w, p) per set, on the row's handle, x and limits"""
    out = []
    for st in sets:
        flt = tuple(st[-2:]) if FILTER in st else None
        name = "+".join((["limits"] if LIMITS in st else []) + (["filter%d_%d" % flt] if flt else []))
        out.append(dict(base, id="%s_%s" % (base["id"], name), limits=LIMITS in st, filter=flt))
    return out


def pm_row(id, K, H, a, kernel, lo, hi, path="lone", counts=(1, 1, 1), **kw):
    kw = dict(dict(lam=1.0, q=10.0, sigma=0.1), **kw)
    c = nu.pm(id, K, [], kernel, H=H, a=a, **kw)
    c.update(path=path, lo=lo, hi=hi, x=(nu.goal_of(c) + np.asarray(PM_OFF[:2 * a], F32)).astype(F32), counts=counts, mlp=None)
    return c


def mlp_row(id, K, H, a, kernel, hid, n_hidden, lo, hi, lam=1.0, sigma=0.1, seed=1, q=1.0):
    c = pm_row(id, K, H, a, kernel, lo, hi, lam=lam, sigma=sigma, seed=seed, q=q)
    c.update(model="mlp", mlp=mlp_weights(2 * a, a, hid, n_hidden, 40 + a), x=(0.2 * np.random.default_rng(a).standard_normal(2 * a)).astype(F32))
    return c


def auv_row(id, K, H, kernel, lo, hi, tuning=None, lam=1.0, q=1.0, seed=1):
    c = nu.auv(id, K, kernel, lam, q, tuning=tuning, seed=seed, goal=nu.AUV_GOALS[0], ks=[])
    x = np.array(nu.AUV_GOALS[0], F32)
    x[:3] = [0.5, -0.4, 0.3]
    c.update(H=H, path="lone", lo=lo, hi=hi, x=x, counts=(1, 1, 1), mlp=None)
    return c



def option_problems(case):
    """-> (fp32, fp64) oracle problems of the case"""
    if case["model"] != "mlp":
        return nu.problems(case)
    a = case["a"]
    kw = dict(tau=case["H"], s=2 * a, a=a, lam=float(F32(case["lam"])), sigma=case["sigma"], goal=nu.goal_of(case), Q=nu.q_of(case), mlp=case["mlp"], threads=0)
    return orc.Problem(**kw), orc.Problem(dtype=np.float64, **kw)


def step_noise(case, step):
    """the noise of control step `step` as the CPU knows it: the oracle's restatement of the Philox draw, or the case's own injected noise"""
    K, H, a = case["K"], case["H"], case["a"]
    if case["inject"]:  # antithetic pairs: the sample mean of the noise is zero, so what these few samples move U' by is the pull alone
        z = np.random.default_rng(100 * case["seed"] + step).standard_normal(((K + 1) // 2, H, a))
        if case["inject"] == "axes":  # ... each pair along one horizon-action axis, 1 to 1.5 sqrt(HA) long: the pull without sampling noise
            p = np.arange((K + 1) // 2)
            z = np.zeros(((K + 1) // 2, H * a))
            z[p, p % (H * a)] = np.sqrt(H * a) * (1.0 + 0.25 * ((p // (H * a) + step) % 3))
            z = z.reshape(-1, H, a)
        return (np.concatenate([z, -z])[:K] @ np.asarray(case["sigma"]).T).astype(F32)
    return orc.noise(case["seed"], step, 0, K, H, a, case["sigma"])


def raw_update(case, p64, U, eps):
    """the fp64 oracle's unclipped U' [H, a] of one step from the sequence U on the noise eps"""
    u, Ushift, _ = p64.next_with_noise(case["x"], U, eps, normalize=case["normalize"])
    return np.vstack([u[None], Ushift[:-1]])


def first_sequence(case):
    """the nominal sequence of the first step: zeros, or the case's own warm start"""
    U0 = case.get("U0")
    return np.zeros((case["H"], case["a"]), F32) if U0 is None else np.asarray(U0, F32).reshape(case["H"], case["a"])


def checked_steps(case):
    """the steps that are held to the reference: every one of three single steps; of runs of several device steps the last of each run"""
    return set(np.cumsum(case["counts"]) - 1)


def cpu_steps(case, check=True):
    """the case's control steps on the CPU's noise with the fp64 references, the stored sequence rounded to fp32 between the steps as the
    handle holds it; -> per step (U'_raw, the margins of option_conditions)"""
    _, p64 = option_problems(case)
    U, out = first_sequence(case), []
    for s in range(sum(case["counts"])):
        Uraw = raw_update(case, p64, U, step_noise(case, s))
        held = check and s in checked_steps(case)
        out.append((Uraw, option_conditions(case, Uraw, "%s step %d" % (case["id"], s)) if held else None))
        U = option_reference(case, Uraw)[1].astype(F32)
    return out


L, F53, B53 = (LIMITS,), (FILTER, 5, 3), (LIMITS, FILTER, 5, 3)
PC2, PC3_5, PC3_3 = ("mppi::k_rollout_pc<2, 5, ", ", 0, 0>"), ("mppi::k_rollout_pc<3, 5, ", ", 0, 0>"), ("mppi::k_rollout_pc<3, 3, ", ", 0, 0>")
LIM_192 = dict(lo=[-0.08132, 0.01461], hi=[-0.01653, 0.04913])
LIM_NORM = dict(lo=[-0.04436, 0.01225, -0.02114], hi=[-0.01854, 0.03177, -0.00855])
LIM_AUV = dict(lo=[-32.01, 9.77, -19.64, -7.6, -12.56, -10.29], hi=[-10.99, 22.99, -4.8, 10.57, -3.39, 2.85])
AUV_KW = dict(lam=30.0, seed=3)  # noise-led (sigma = 200 on 129 samples): twelve entries per column scatter over both limits in every step
OPTION_CASES = (
    option_sets(pm_row("r01_column_waves", 192, 8, 2, ("mppi::k_step_pc<2, ", ""), **LIM_192), L)
    + option_sets(pm_row("r02_finish_cols_3_tiles", 192, 8, 2, PC2, tuning={"fused_step": 0}, **LIM_192), L, F53, B53)
    + option_sets(pm_row("r03_finish_cols_129_tiles", 8256, 8, 3, PC3_5, [-0.05608, 0.01536, -0.02674], [-0.02298, 0.0406, -0.01109]), L, B53)
    + option_sets(pm_row("r04_one_fold_level", 65600, 4, 3, PC3_3, [-0.01827, 0.00458, -0.01136], [-0.00582, 0.01461, -0.00352]), L)
    + option_sets(pm_row("r05_normalize_two_pass", 8256, 8, 3, ("mppi::k_rollout_pc<3, 5, ", ""), normalize=True, lam=0.1, **LIM_NORM), L, B53)
    + option_sets(pm_row("r05_normalize_tile", 8256, 8, 3, ("mppi::k_rollout_tile<3, 64, ", ""), normalize=True, lam=0.1, tuning={"force_tile_kernel": 1},
                         **LIM_NORM), L, B53)
    + option_sets(pm_row("r06_tile_R64_inject", 130, 5, 4, ("mppi::k_rollout_tile<4, 64, ", ""), [-0.05961, 0.00843, -0.02529, 0.00441],
                         [-0.01236, 0.0394, -0.00557, 0.01978], inject="axes", tuning={"force_tile_kernel": 1}), B53)  # window 5 = H: every row an edge row
    + option_sets(pm_row("r07_tile_R32_inject", 70, 207, 3, ("mppi::k_rollout_tile<3, 32, ", ""), [-0.1396, -0.1094, -0.1562], [0.099, 0.2007, 0.0942],
                         inject=True), L)
    + option_sets(pm_row("r08_three_shards", 8191, 8, 3, PC3_5, [-0.05889, 0.01737, -0.03097], [-0.01908, 0.04844, -0.01051], path="shards3", seed=21), L, B53)
    + option_sets(pm_row("r09_direct_exchange", 8192, 8, 3, PC3_5, [-0.06337, 0.01106, -0.03667], [-0.01504, 0.04576, -0.00833], path="p2p2", seed=33), L)
    + option_sets(pm_row("r10_prelaunched_fused", 512, 8, 2, ("mppi::k_step_pc<2, ", ""), [-0.06055, 0.01604], [-0.01306, 0.04774], path="pre",
                         counts=(1, 2, 3, 9), tuning={"prelaunch": 1}), L)
    + option_sets(pm_row("r11_prelaunched_129_tiles", 8256, 8, 2, PC2, [-0.05826, 0.01167], [-0.01683, 0.04631], path="pre", counts=(1, 2, 3, 9),
                         tuning={"prelaunch": 1}), L)
    + option_sets(mlp_row("r12_mlp_small_dense16", 130, 6, 2, ("mppi::k_rollout_mlp_small<2, 16>", ""), 16, 3, [-0.0064, -0.0161], [0.0175, 0.0513],
                          sigma=0.5, seed=2), B53)
    # (the learned models pull weakly, so sigma = 0.5 and the noise leads; with four entries per column the three steps meet the conditions
    # for few seeds: 1065 is the first that does)
    + option_sets(mlp_row("r13_mlp2", 65, 4, 3, ("mppi::k_rollout_mlp2<3, ", ""), 256, 2, [-0.02492, -0.0808, -0.07482], [0.06745, 0.00378, -0.03532],
                          sigma=0.5, seed=1065), (LIMITS, FILTER, 3, 1))
    + option_sets(auv_row("r14_auv_pc", 129, 12, nu.AUV_PC, **LIM_AUV, **AUV_KW), L, F53, B53, (LIMITS, FILTER, 11, 2))
    + option_sets(auv_row("r15_auv_one_wave", 129, 12, nu.AUV_GEN, tuning={"gen_one_wave": 1}, **LIM_AUV, **AUV_KW), B53)
    + option_sets(pm_row("r16_a1", 192, 9, 1, ("mppi::k_rollout_pc<1, ", ""), None, None), (FILTER, 9, 2)))
OPTION_LONE = [c for c in OPTION_CASES if c["path"] == "lone"]
OPTION_BY_PATH = {p: [c for c in OPTION_CASES if c["path"] == p] for p in ("shards3", "p2p2", "pre")}


# ---- the GPU side -----------------------------------------------------------------------------------------------------------------------------
def option_handle(m, case, **kw):
    """the case's handle with its options set; the kernel name is asserted with the options in place (a filter takes the one-launch step away)"""
    if case["model"] == "mlp":
        a = case["a"]
        h = m.Handle(k=case["K"], tau=case["H"], s_dim=2 * a, a_dim=a, lam=case["lam"], sigma=case["sigma"], goal=nu.goal_of(case), Q=nu.q_of(case),
                     mlp=case["mlp"], seed=case["seed"], tuning=case["tuning"], **kw)
    else:
        h = nu.handle(m, dict(case, kernel=("", "")), **kw)
    set_options(h, case)
    nu.assert_kernel(h, case)
    if case.get("U0") is not None:
        h.set_action_sequence(first_sequence(case))
    return h


def set_options(h, case):
    if case["limits"]:
        h.set_action_limits(case["lo"], case["hi"])
    if case["filter"]:
        h.set_sequence_filter(*case["filter"])


def check_step(m, case, h, p64, U, eps, u, step, seen):
    """one control step of handle h that started from the sequence U and ran on the noise eps, against the fp64 reference; the conditions
    that make the step a test are recomputed on that noise first"""
    tag, tol, H = "%s step %d" % (case["id"], step), U_TOL * case["scale"], case["H"]
    if not case["inject"]:
        np.testing.assert_allclose(eps, step_noise(case, step), rtol=0, atol=5e-6 * case["scale"], err_msg=tag + ": the noise is not the one the CPU proof ran on")
    Uraw = raw_update(case, p64, U, eps)
    margins = option_conditions(case, Uraw, tag)
    Uu, _ = option_reference(case, Uraw)
    Ud, seq = h.debug_get(m.DBG_U_UPDATED), h.get_action_sequence()
    dU = max(np.abs(Ud - Uu).max(), np.abs(u - Uu[0]).max()) / case["scale"]
    seen["dU"] = max(seen.get("dU", 0.0), dU)
    np.testing.assert_array_equal(u, Ud[0], err_msg=tag + " u is U'[0]")
    if case["filter"]:
        want, bar = savgol(shifted(Ud.astype(np.float64)), *case["filter"]), filter_bar(H, *case["filter"], Ud)
        dS = np.abs(seq - want).max()
        seen["dS"] = max(seen.get("dS", 0.0), dS / bar)
        print("%s: max|dU'| %.3g (x scale) | filtered sequence off by %.3g, bar %.3g | least margin %.0f bars" % (tag, dU, dS, bar, min(margins.values())))
        assert dS <= bar, "%s: the stored sequence is %.3g from the filter of the device's U', bar %.3g" % (tag, dS, bar)
    else:
        print("%s: max|dU'| %.3g (x scale) | least margin %.0f bars" % (tag, dU, min(margins.values())))
        np.testing.assert_array_equal(seq, shifted(Ud), err_msg=tag + " the stored sequence is the shift of U'")
    np.testing.assert_allclose(Ud, Uu, rtol=0, atol=tol, err_msg=tag + " U'")
    np.testing.assert_allclose(u, Uu[0], rtol=0, atol=tol, err_msg=tag + " u")


def run_lone_options(m, case):
    """three control steps of a lone handle, each from the sequence the handle stored"""
    h, (_, p64), seen = option_handle(m, case), option_problems(case), {}
    for s in range(STEPS):
        U = h.get_action_sequence()
        if case["inject"]:
            eps = step_noise(case, s)
            u = h.next_with_noise(case["x"], eps)
        else:
            u = h.next(case["x"])
            eps = h.debug_get(m.DBG_NOISE)
        check_step(m, case, h, p64, U, eps, u, s, seen)
    assert h.get_step_counter() == STEPS
    h.close()
    return seen


def device_steps(h, x, n, a):
    """n enqueue-only steps on the handle's own stream (where the pre-launched route serves), then drain"""
    import torch
    xd, ud = torch.tensor(np.asarray(x, F32), device="cuda"), torch.zeros(a, device="cuda")
    torch.cuda.synchronize()
    for _ in range(n):
        h.next_device(xd.data_ptr(), ud.data_ptr(), None)
    h.synchronize()
    torch.cuda.synchronize()
    return ud.cpu().numpy()


def assert_same_state(m, ha, hb, tag, costs=True):
    """two handles that received the same calls hold the same bits"""
    np.testing.assert_array_equal(ha.get_action_sequence(), hb.get_action_sequence(), err_msg=tag + " sequence")
    np.testing.assert_array_equal(ha.debug_get(m.DBG_U_UPDATED), hb.debug_get(m.DBG_U_UPDATED), err_msg=tag + " U'")
    if costs:
        np.testing.assert_array_equal(ha.debug_get(m.DBG_COSTS), hb.debug_get(m.DBG_COSTS), err_msg=tag + " costs")
    assert ha.get_step_counter() == hb.get_step_counter(), tag


# ---- A2: the second fold level end to end ----------------------------------------------------------------------------------------------------
K20 = 2 ** 20 + 1
K20_NB, K20_NBP = (K20 + 63) // 64, record_pad((K20 + 63) // 64)
K20_SLOTS = [0, 255, 256, 4095, 4096, 16383, 16384, 16495]  # first / last slot of a level-1 and a level-2 group; 16495: the highest owned slot, in the partial last level-2 group


def slot_tile(slot, nbp):
    """record_slot's inverse: the tile whose record sits in `slot` of nbp"""
    q = nbp // 8
    return (slot % q) * 8 + slot // q


K20_KS = [64 * slot_tile(s, K20_NBP) + s % 64 for s in K20_SLOTS] + [K20 - 1]  # a sample of each of those tiles; the lone sample of the last tile
# lambda: about a ninth of the smallest gap over the case's needles (fp64 oracle, restated noise; the gaps are 18.2 .. 61.2, normalised 2.1e-3 .. 2.7e-3)
TWO_LEVEL = [nu.pm("two_levels_K%d_%s" % (K20, n), K20, ks, PC3_3, lam=lam, group="two_levels")
             for n, ks, lam in (("a", K20_KS[0:3], 2.0), ("b", K20_KS[3:6], 3.9), ("c", K20_KS[6:9], 4.3))]
TWO_LEVEL += [nu.pm("two_levels_K%d_normalize" % K20, K20, [K20_KS[0], K20_KS[2], K20_KS[-1]], ("mppi::k_rollout_pc<3, 3, ", ""), normalize=True,
                    lam=2.3e-4, group="two_levels")]
