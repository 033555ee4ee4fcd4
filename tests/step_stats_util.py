"""What the step-statistics tests share (test_step_stats_oracle.py on the CPU, test_step_stats_gpu.py on the device): the numpy reference of
mppi_step_stats (include/mppi_c.h), the bar of every statistic derived per case, the comparison, and the cost draws of the CPU oracle.
A plain module.

The reference restates the kernel's per-sample quantities op by op in float32 — arg = t * (c' - beta): one subtraction, one product — takes
e = exp(arg) in float64, and evaluates every sum and final expression in float64. What the device does differently is one thing only: its
e is expf's float32 value. The bars say how far that can move a statistic."""
import numpy as np

F32, F64 = np.float32, np.float64
BINS = 32
NAMES = ("beta", "eta", "ess", "entropy", "cost_mean", "cost_std", "cost_max", "best_index", "n_nonfinite")
# the two regimes a user tunes lambda between, as the GPU cases make them (point mass, K = 256, tau = 8, x0 = pm_x0, Sigma = 0.25 I): the
# sample costs there have this mean and standard deviation; `lam` spreads the weight over many samples or leaves it with one
SPREAD = dict(lam=0.3, mean=12.5, std=0.3)
NEEDLE = dict(lam=0.02, mean=12.5, std=0.3)


def ulp32(x):
    """the spacing of the float32 line at x (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def _bin(v):
    """the kernel's stat_bin on a float32 array: min(31, (int)v) for finite v >= 0; negative -> 0, NaN and +inf -> 31"""
    v = np.asarray(v, F32)
    low = v < F32(31.0)
    with np.errstate(invalid="ignore"):
        i = np.where(low & (v > 0), v, F32(0.0)).astype(np.int32)
    return np.where(low, i, BINS - 1)


def cost_bins(c, cmin, cmax):
    """hist_cost's bin of every finite raw cost, op by op in float32"""
    c, cmin, cmax = np.asarray(c, F32), F32(cmin), F32(cmax)
    with np.errstate(all="ignore"):
        scale = F32(0.0) if cmax == cmin else F32(32.0) / F32(cmax - cmin)
        v = ((c - cmin).astype(F32) * scale).astype(F32)
    return _bin(v)


def weight_bins(arg):
    """hist_weight's bin from the exponent's argument, op by op in float32"""
    with np.errstate(all="ignore"):
        v = ((-np.asarray(arg, F32)).astype(F32) * F32(1.442695)).astype(F32)
    return _bin(v)


def args_of(costs_w, beta, t):
    """arg_k = t * (c'_k - beta) in float32, k_weights' expression"""
    with np.errstate(all="ignore"):
        d = (np.asarray(costs_w, F32) - F32(beta)).astype(F32)
        return (F32(t) * d).astype(F32)


def sums(arg, e):
    """S1, S2, T in float64 from the arguments and ANY e (float64 values); a term with e = 0 is its limit, never 0 * -inf"""
    e = np.asarray(e, F64)
    pos = e > 0
    return e.sum(), (e * e).sum(), (e[pos] * np.asarray(arg, F64)[pos]).sum()


def weight_stats(S1, S2, T):
    return S1 * S1 / S2, np.log(S1) - T / S1


@np.errstate(all="ignore")  # (a wrong implementation under test may leave no weight at all: NaN, which compare() reports)
def reference(costs, costs_w, beta, eta, t, e_of=None):
    """-> dict: the nine statistics (float64 / int), hist_cost, hist_weight, and `bar`: how far the device's value of ess, entropy,
    cost_mean and cost_std may lie from these (everything else is exact). costs: the raw sample costs (MPPI_DBG_COSTS); costs_w, beta, t:
    what the weights were made from (MPPI_DBG_WEIGHTS' selection); eta is passed through. e_of(arg) replaces e = exp(float64(arg))."""
    c, cw = np.asarray(costs, F32).ravel(), np.asarray(costs_w, F32).ravel()
    fin = np.isfinite(c)
    cf = c[fin]
    out = dict(beta=F32(beta), eta=F32(eta), n_nonfinite=int(c.size - cf.size), k=int(c.size))
    if cf.size == 0:
        out.update(ess=np.nan, entropy=np.nan, cost_mean=np.nan, cost_std=np.nan, cost_max=np.nan, best_index=-1,
                   hist_cost=np.zeros(BINS, np.int64), hist_weight=np.zeros(BINS, np.int64), bar={})
        return out
    arg = args_of(cw[fin], beta, t)
    e = np.exp(arg.astype(F64)) if e_of is None else np.asarray(e_of(arg), F64)
    S1, S2, T = sums(arg, e)
    ess, ent = weight_stats(S1, S2, T)
    c64 = cf.astype(F64)
    mean = c64.sum() / cf.size
    std = np.sqrt(((c64 - mean) ** 2).sum() / cf.size)
    cmax, cmin = cf.max(), cf.min()
    out.update(ess=ess, entropy=ent, cost_mean=mean, cost_std=std, cost_max=cmax, best_index=int(np.flatnonzero(fin)[np.argmin(cf)]),
               hist_cost=np.bincount(cost_bins(cf, cmin, cmax), minlength=BINS), hist_weight=np.bincount(weight_bins(arg), minlength=BINS))
    # ---- the bars. expf is documented to 1 ulp; every e_k is allowed max(2 ulp32(e_k), 2^-126) (the floor: a flushed denormal) in the
    # worst direction for the statistic at hand: |delta f| <= sum_k |df/de_k| d_k, with
    #   ESS = S1^2 / S2:              dESS/de_k = 2 S1 / S2 - 2 S1^2 e_k / S2^2
    #   ENT = ln S1 - T / S1:         dENT/de_k = (1 - arg_k + T / S1) / S1     (arg_k = -inf has e_k = 0 on both sides: no term)
    # (the second-order remainder is below 1e-12 of the bar: d_k / e_k <= 2.4e-7), then 2 float32 ulps of the value for the one cast.
    d = np.maximum(2.0 * ulp32(e), 2.0 ** -126)
    g_ess = np.abs(2.0 * S1 / S2 - 2.0 * S1 * S1 * e / (S2 * S2))
    a64 = np.where(np.isfinite(arg), arg.astype(F64), 0.0)
    g_ent = np.where(np.isfinite(arg), np.abs(1.0 - a64 + T / S1) / S1, 0.0)
    out["bar"] = dict(ess=(g_ess * d).sum() * (1 + 1e-9) + 2 * ulp32(ess), entropy=(g_ent * d).sum() * (1 + 1e-9) + 2 * ulp32(ent),
                      cost_mean=2 * ulp32(mean), cost_std=2 * ulp32(std))
    return out


def e_float32(arg):
    """e as a float32 evaluation has it: exp correctly rounded to float32"""
    return np.exp(np.asarray(arg, F32).astype(F64)).astype(F32).astype(F64)


def compare(ref, got):
    """got: a dict or StepStats-like with the reference's names -> (exact, ratio): the names of the exact checks that fail, and for every
    barred statistic |got - ref| / bar"""
    g = (lambda n: got[n]) if isinstance(got, dict) else (lambda n: getattr(got, n))
    exact = []
    for n in ("beta", "eta", "cost_max"):
        if np.asarray(g(n), F32).tobytes() != np.asarray(ref[n], F32).tobytes():
            exact.append(n)
    for n in ("best_index", "n_nonfinite"):
        if int(g(n)) != int(ref[n]):
            exact.append(n)
    for n in ("hist_cost", "hist_weight"):
        h = np.asarray(g(n)).astype(np.int64)
        if not np.array_equal(h, ref[n]):
            exact.append(n)
        if int(h.sum()) != ref["k"] - ref["n_nonfinite"]:
            exact.append(n + " sum")
    ratio = {}
    for n, bar in ref["bar"].items():
        v, r = F64(g(n)), F64(ref[n])
        ratio[n] = (abs(v - r) / bar) if np.isfinite(v) and np.isfinite(r) else (0.0 if (np.isnan(v) and np.isnan(r)) or v == r else np.inf)
    return exact, ratio


def assert_matches(ref, got, tag="", log=print):
    """every exact check, and every barred statistic inside its bar; prints the distance found beside the bar first"""
    exact, ratio = compare(ref, got)
    g = (lambda n: got[n]) if isinstance(got, dict) else (lambda n: getattr(got, n))
    for n, bar in ref["bar"].items():
        log("%s %-9s got %.9g ref %.17g |diff| %.3g bar %.3g (%.3g rel)" % (tag, n, F64(g(n)), ref[n], abs(F64(g(n)) - ref[n]), bar,
                                                                           bar / abs(ref[n]) if ref[n] else np.inf))
    assert not exact, "%s: exact checks failed: %s" % (tag, exact)
    bad = {n: r for n, r in ratio.items() if not r <= 1.0}
    assert not bad, "%s: outside the bar (|diff| / bar): %s" % (tag, bad)


def draw(kind, K, seed):
    """sample costs as a GPU case of this regime has them -> (costs float32 [K], beta, eta, t): Gaussian about the case's mean"""
    rng = np.random.default_rng(seed)
    c = (kind["mean"] + kind["std"] * rng.standard_normal(K)).astype(F32)
    t = F32(-1.0) / F32(kind["lam"])
    beta = c.min()
    eta = F32(np.exp(args_of(c, beta, t).astype(F64)).sum())
    return c, beta, eta, t
