"""The step statistics' reference and bars mean something (step_stats_util.py; no GPU): on costs drawn with the lambda and the scales of
the GPU cases, one spread over many samples and one a needle, the bars are tight, a float32 evaluation of the same formulas stays inside
them, and each plausible wrong implementation lies at least ten bars outside or breaks an exact check."""
import numpy as np
import pytest

import step_stats_util as su
from step_stats_util import F32, F64

K = 8256  # a GPU case's: 129 tiles, eight 4-sample groups per thread and a ragged ninth at 1024 threads
CASES = {"spread": su.SPREAD, "needle": su.NEEDLE}


def case(name, seed=1):
    c, beta, eta, t = su.draw(CASES[name], K, seed)
    return c, beta, eta, t, su.reference(c, c, beta, eta, t)


def as_got(ref, **over):
    got = {n: ref[n] for n in su.NAMES + ("hist_cost", "hist_weight")}
    got.update(over)
    return got


def far_outside(ref, got, bars=10.0):
    exact, ratio = su.compare(ref, got)
    return bool(exact) or max(ratio.values()) >= bars


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_cases_are_what_they_are_called(name):
    c, beta, eta, t, ref = case(name)
    frac = ref["ess"] / K
    if name == "spread":
        assert 0.05 <= frac <= 0.9, frac
        assert 0.5 * np.log(K) < ref["entropy"] <= np.log(K)
    else:
        assert 1.0 <= ref["ess"] < 2.0, ref["ess"]
        assert ref["hist_weight"][-1] > K // 2  # nearly every sample is more than 31 octaves below the best
    assert ref["best_index"] == int(np.argmin(c)) and c[ref["best_index"]].tobytes() == F32(beta).tobytes()
    assert ref["hist_cost"].sum() == ref["hist_weight"].sum() == K and ref["n_nonfinite"] == 0
    assert ref["hist_weight"][0] >= 1  # the best sample: arg = 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_bars_are_tight_and_float32_stays_inside(name):
    c, beta, eta, t, ref = case(name)
    assert ref["bar"]["ess"] < 1e-5 * ref["ess"], ref["bar"]
    assert ref["bar"]["entropy"] < 1e-5 * max(ref["entropy"], 1.0)
    got = su.reference(c, c, beta, eta, t, e_of=su.e_float32)
    assert (got["ess"], got["entropy"]) != (ref["ess"], ref["entropy"])  # (it IS another evaluation)
    got32 = as_got(got, **{n: F32(got[n]) for n in ("ess", "entropy", "cost_mean", "cost_std")})
    su.assert_matches(ref, got32, name)
    # e moved by one float32 ulp per sample in the worst direction for the ESS is inside as well, and by twenty ulps is not
    e = np.exp(su.args_of(c, beta, t).astype(F64))
    S1, S2, _ = su.sums(su.args_of(c, beta, t), e)
    sign = np.sign(2.0 * S1 / S2 - 2.0 * S1 * S1 * e / (S2 * S2))
    # (a needle's ESS has no first-order term to speak of: 1 + 2 sum of the small e; its bar is the cast's two ulps)
    for ulps, inside in ((1.0, True),) + (((20.0, False),) if name == "spread" else ()):
        moved = su.reference(c, c, beta, eta, t, e_of=lambda arg: e + sign * ulps * su.ulp32(e))
        _, ratio = su.compare(ref, as_got(moved))
        assert (ratio["ess"] <= 1.0) == inside, (ulps, ratio)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("where", ["first", "last", "63", "64", "block_last"])
def test_a_dropped_sample_is_seen(name, where):
    """a kernel that skips one position: the first, the last, either side of a wave's edge, the last thread's of a block"""
    c, beta, eta, t, ref = case(name)
    i = {"first": 0, "last": K - 1, "63": 63, "64": 64, "block_last": 1023}[where]
    keep = np.ones(K, bool)
    keep[i] = False
    got = su.reference(c[keep], c[keep], beta, eta, t)
    assert far_outside(ref, as_got(got))
    # ... also when the dropped one is the best sample
    j = ref["best_index"]
    c2 = c.copy()
    c2[[i, j]] = c2[[j, i]]
    ref2 = su.reference(c2, c2, beta, eta, t)
    got2 = su.reference(c2[keep], c2[keep], beta, eta, t)
    exact, ratio = su.compare(ref2, as_got(got2))
    assert "best_index" in exact or "hist_weight" in exact


def test_lambda_instead_of_the_steps_temperature():
    """normalize_cost: the weights are made at t = -1 / (lambda (max - min)); a kernel that takes -1 / lambda is far outside"""
    c, beta, eta, _, _ = case("spread")
    lam = F32(su.SPREAD["lam"])
    t_step = (F32(-1.0) / lam) / F32(c.max() - c.min())
    ref = su.reference(c, c, beta, eta, t_step)
    got = su.reference(c, c, beta, eta, F32(-1.0) / lam)
    exact, ratio = su.compare(ref, as_got(got))
    assert ratio["ess"] >= 10.0 and ratio["entropy"] >= 10.0, ratio


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_stale_eta(name):
    """ESS = eta^2 / S2 with the eta of the step before (other costs): far outside; the kernel's own S1 is what the reference uses"""
    c, beta, eta, t, ref = case(name)
    c_prev, beta_prev, eta_prev, _ = su.draw(CASES[name], K, seed=2)
    e = np.exp(su.args_of(c, beta, t).astype(F64))
    S2 = (e * e).sum()
    assert far_outside(ref, as_got(ref, ess=F64(eta_prev) ** 2 / S2))
    # (with this step's eta, a float32 of S1, it is a legitimate evaluation: inside)
    _, ratio = su.compare(ref, as_got(ref, ess=F64(eta) ** 2 / S2))
    assert ratio["ess"] <= 1.0


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_nonfinite_cost_is_counted_and_left_out(bad):
    c, beta, eta, t, _ = case("spread")
    c = c.copy()
    hit = [5, 64, K - 1]
    c[hit] = bad
    ref = su.reference(c, c, beta, eta, t)
    clean = su.reference(np.delete(c, hit), np.delete(c, hit), beta, eta, t)
    assert ref["n_nonfinite"] == 3 and ref["hist_cost"].sum() == ref["hist_weight"].sum() == K - 3
    for n in ("ess", "entropy", "cost_mean", "cost_std", "cost_max"):
        assert ref[n] == clean[n] and np.isfinite(ref[n]), n
    assert ref["best_index"] == int(np.argmin(np.where(np.isfinite(c), c, np.inf)))
    # a kernel that lets it into the sums
    with np.errstate(all="ignore"):
        c64 = c.astype(F64)
        wrong = as_got(ref, cost_mean=c64.sum() / K, cost_std=np.sqrt(((c64 - c64.sum() / K) ** 2).sum() / K))
    assert far_outside(ref, wrong)
    # nothing finite at all
    none = su.reference(np.full(7, bad, F32), np.full(7, bad, F32), beta, eta, t)
    assert none["n_nonfinite"] == 7 and none["best_index"] == -1 and np.isnan(none["ess"]) and none["hist_cost"].sum() == 0


def test_histogram_edges():
    c = np.linspace(1.0, 3.0, 1000).astype(F32)
    b = su.cost_bins(c, c.min(), c.max())
    assert b[-1] == 31 and b[0] == 0 and np.all(np.diff(b) >= 0) and set(b) == set(range(32))  # c = COST_MAX: (int)32.0 clamps to 31
    assert np.all(su.cost_bins(np.full(9, 2.5, F32), 2.5, 2.5) == 0)  # a constant array: scale = 0
    big = np.array([-3e38, 0.0, 3e38], F32)  # max - min overflows: scale = 32 / inf = 0, and the maximum's inf * 0 = NaN has a bin
    assert list(su.cost_bins(big, big.min(), big.max())) == [0, 0, 31]
    arg = -np.log(2.0) * np.array([0.0, 0.5, 1.5, 30.5, 31.5, 200.0], F64)
    assert list(su.weight_bins(arg.astype(F32))) == [0, 0, 1, 30, 31, 31]
    assert list(su.weight_bins(np.array([-np.inf, np.nan, 1.0], F32))) == [31, 31, 0]  # arg > 0 (a cost below beta) stays in range
    # bin j holds the weights in (2^-(j+1), 2^-j] of the best one's
    w = np.exp(arg)
    assert np.all(w[[2, 3]] <= 2.0 ** -np.array([1, 30])) and np.all(w[[2, 3]] > 2.0 ** -np.array([2, 31]))


def test_zero_weight_terms_never_form_zero_times_inf():
    c = np.array([1.0, 2.0, 3e38], F32)
    ref = su.reference(c, c, F32(1.0), F32(1.0), F32(-3e5))  # arg of the last: -inf, e = 0
    assert np.isfinite(ref["entropy"]) and np.isfinite(ref["ess"]) and ref["hist_weight"][31] == 2
