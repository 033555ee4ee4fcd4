"""Step statistics on the device (mppi_step_stats / mppi_batch_step_stats / mppi_run_episode_stats; Handle.step_stats,
BatchHandle.step_stats, run_episode(..., stats=True)). Needs an MI355X: every test is marked `gpu`.

The contract (include/mppi_c.h): the statistics of the last step equal the numpy reference (step_stats_util.reference) on the costs, beta
and eta that debug_get reads back — bit or integer equality for BETA, ETA, COST_MAX, BEST_INDEX, N_NONFINITE and both histograms, two
float32 ulps for the cost moments, and for ESS and ENTROPY the bar the util derives per case from expf's accuracy (printed beside the
distance found). They only observe; a batch's row m has the bits of lone handle m's; an episode with stats=True is the plain episode in
X, U, C and where the handle ends, and its rows are step_stats() after each step of the host loop."""
import numpy as np
import pytest

import step_stats_util as su
from batch_util import auv_members, lone_handles, pm_members
from episode_util import auv_cfg, make_nnauv, pm_cfg, pm_x0, signals

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FIELDS = su.NAMES + ("hist_cost", "hist_weight")


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def close(*hs):
    for h in hs:
        h.close()


def temperature(lam, costs=None):
    """-1 / lambda as the library forms it; with `costs` the step's temperature under normalize_cost, k_cost_minmax's expression"""
    t = F32(-1.0) / F32(lam)
    return t if costs is None else t / F32(costs.max() - costs.min())


def check_last_step(m, h, lam, tag, normalized=False, dbg=None, st=None):
    """the statistics of the last step against the reference on what debug_get reads back -> (StepStats, reference)"""
    dbg = dbg or h.debug_get
    costs, beta, eta = dbg(m.DBG_COSTS), dbg(m.DBG_BETA), dbg(m.DBG_ETA)
    t = temperature(lam, costs[np.isfinite(costs)] if normalized else None)
    ref = su.reference(costs, costs, beta, eta, t)
    st = h.step_stats() if st is None else st
    assert st.k == costs.size
    su.assert_matches(ref, st, tag)
    assert int(st.hist_cost.sum()) == int(st.hist_weight.sum()) == costs.size - ref["n_nonfinite"]
    if ref["n_nonfinite"] == 0:
        assert int(st.best_index) == int(np.argmin(costs)) and costs[int(st.best_index)].tobytes() == F32(beta).tobytes(), tag
    # the temperature the test assumed is the device's: MPPI_DBG_WEIGHTS' w = e / eta gives eta^2 / S2 = 1 / sum w^2, the ESS up to eta's
    # float32 rounding
    w = dbg(m.DBG_WEIGHTS).astype(F64)[np.isfinite(costs)]
    assert abs(1.0 / (w * w).sum() - F64(st.ess)) <= 1e-4 * F64(st.ess), (tag, 1.0 / (w * w).sum(), st.ess)
    return st, ref


def same_bits(a, b, tag=""):
    for n in FIELDS:
        x, y = np.asarray(getattr(a, n)), np.asarray(getattr(b, n))
        assert x.shape == y.shape and x.tobytes() == y.astype(x.dtype).tobytes(), "%s: %s differs: %r != %r" % (tag, n, x, y)


def _pm(m, K, **kw):
    return m.Handle(**pm_cfg(K, 8, 2, **kw))


def _auv(m):
    X0, G, U0 = auv_members(1, 6)
    h = m.Handle(goal=G[0], seed=4, **auv_cfg(128, 6, "quat"))
    h.set_action_sequence(U0[0])
    return h, X0[0]


def _nnauv(m):
    X0, G, _ = auv_members(1, 4, seed=2)
    return m.Handle(k=64, tau=4, s_dim=13, a_dim=6, dt=0.1, lam=1.0, sigma=np.eye(6, dtype=F32), goal=G[0], Q=np.ones(13, F32),
                    nnauv=make_nnauv(3, 16, 1), seed=9), X0[0]


# name -> (make(m) -> handle or (handle, x), lambda, the rollout kernel's name starts with, normalize_cost)
CASES = {
    "pm_k64_one_wave": (lambda m: _pm(m, 64), 1.0, "mppi::k_step_pc<", False),
    "pm_k256_one_launch": (lambda m: _pm(m, 256), 1.0, "mppi::k_step_pc<", False),
    "pm_k8256_two_launches": (lambda m: _pm(m, 8256), 1.0, "mppi::k_rollout_pc<", False),
    "force_tile_kernel": (lambda m: _pm(m, 256, tuning={"force_tile_kernel": 1}), 1.0, "", False),
    "normalize_cost": (lambda m: _pm(m, 256, normalize_cost=True), 1.0, "mppi::k_rollout_pc<", True),
    "action_cost_py": (lambda m: _pm(m, 256, action_cost=m.ACTION_COST_PY, upsilon_scales_noise=True, gamma=0.1, upsilon=1.4, lam=0.3), 0.3,
                       "", False),
    "fossen_k128": (_auv, 1.0, "mppi::k_rollout_auv_pc<", False),
    "nnauv_dense16_k64": (_nnauv, 1.0, "", False),
    "learned_pm_dense32_k64": (lambda m: m.Handle(**pm_cfg(64, 4, 2, mlp=make_nnauv(5, 32, 1, n_in=6, n_out=4))), 1.0, "", False),
    "spread": (lambda m: _pm(m, 256, lam=su.SPREAD["lam"]), su.SPREAD["lam"], "", False),
    "needle": (lambda m: _pm(m, 256, lam=su.NEEDLE["lam"]), su.NEEDLE["lam"], "", False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_last_step_against_the_reference(m, name):
    """two steps (the second on a warm-started sequence), then step_stats() against the reference on that step's costs"""
    make, lam, kernel, normalized = CASES[name]
    made = make(m)
    h, x = made if isinstance(made, tuple) else (made, pm_x0(2))
    assert h.rollout_kernel_name().startswith(kernel), h.rollout_kernel_name()
    if name == "force_tile_kernel":
        assert "k_rollout_pc" not in h.rollout_kernel_name() and "k_step_pc" not in h.rollout_kernel_name(), h.rollout_kernel_name()
    h.next(x)
    h.next(x)
    st, ref = check_last_step(m, h, lam, name, normalized)
    K = st.k
    print("%s: K %d ess %.6g (%.3g of K) entropy %.6g eta %.6g" % (name, K, st.ess, st.ess / K, st.entropy, st.eta))
    if name == "spread":
        assert 0.05 <= st.ess / K <= 0.9, st.ess / K
    if name == "needle":
        assert st.ess < 2.0, st.ess
    if name == "normalize_cost":  # lambda itself would be far off: the case tells the two temperatures apart
        costs = h.debug_get(m.DBG_COSTS)
        _, ratio = su.compare(su.reference(costs, costs, ref["beta"], ref["eta"], temperature(lam)), st)
        assert ratio["ess"] >= 10.0, ratio
    close(h)


def test_statistics_only_observe(m):
    """two calls in a row return the same bits; a step, step_stats(), and the next step agree with a handle that never asked"""
    for K in (256, 8256):
        h1, h2 = _pm(m, K), _pm(m, K)
        x = pm_x0(2)
        np.testing.assert_array_equal(h1.next(x), h2.next(x))
        a, b = h1.step_stats(), h1.step_stats()
        same_bits(a, b, "two calls")
        np.testing.assert_array_equal(h1.next(x), h2.next(x))
        for what in (m.DBG_COSTS, m.DBG_BETA, m.DBG_ETA, m.DBG_WEIGHTS):
            np.testing.assert_array_equal(h1.debug_get(what), h2.debug_get(what))
        np.testing.assert_array_equal(h1.get_action_sequence(), h2.get_action_sequence())
        assert h1.get_step_counter() == h2.get_step_counter() == 2
        same_bits(h1.step_stats(), h2.step_stats(), "after the next step")
        close(h1, h2)


def test_nonfinite_costs_are_counted_and_left_out(m):
    """Which way was taken: injected noise (next_with_noise). A Q and goal that overflow for a known subset only would depend on how the
    horizon's terms are added up; instead the noise rows of a chosen subset are 1e22: their positions reach 5e19, whose square is not a
    float32. Their costs are +inf; they are counted, and every sum, maximum and histogram is that of the other samples."""
    K, H, a = 256, 8, 2
    h = m.Handle(**pm_cfg(K, H, a))
    rng = np.random.default_rng(5)
    eps = (0.25 * rng.standard_normal((K, H, a))).astype(F32)
    hit = [0, 63, 64, 200, 255]
    eps[hit] = F32(1e22)
    h.next_with_noise(pm_x0(a), eps)
    costs = h.debug_get(m.DBG_COSTS)
    assert sorted(np.flatnonzero(~np.isfinite(costs))) == hit, np.flatnonzero(~np.isfinite(costs))
    st, ref = check_last_step(m, h, 1.0, "nonfinite")
    assert int(st.n_nonfinite) == len(hit) and int(st.hist_cost.sum()) == K - len(hit)
    assert np.isfinite([st.ess, st.entropy, st.cost_mean, st.cost_std, st.cost_max]).all()
    fin = np.isfinite(costs)
    assert st.cost_max == costs[fin].max() and int(st.best_index) == int(np.flatnonzero(fin)[np.argmin(costs[fin])])
    close(h)


def _batch_pm(m, B=3):
    shared = dict(k=256, tau=8, s_dim=4, a_dim=2, dt=0.1, mass=1.0, Q=np.ones(4, F32))
    lams = [0.05, 1.0, 0.2][:B]
    sigmas = [np.eye(2, dtype=F32) * F32(v) for v in (0.1, 0.25, 0.4)][:B]
    seeds = [11 + 7 * i for i in range(B)]
    X0, G, U0 = pm_members(B, 2, 8)
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, lams=lams, sigmas=sigmas, **shared)
    hb.set_action_sequences(U0)
    hs = lone_handles(m, [dict(shared, lam=lams[i], sigma=sigmas[i]) for i in range(B)], seeds, G, U0, "mppi::k_step_pc<")
    return hb, hs, X0, lams


def _rows_equal_lone(m, hb, hs, X0, lams, tag):
    hb.next(X0)
    sb = hb.step_stats()
    assert sb.ess.shape == (len(hs),) and sb.hist_cost.shape == (len(hs), 32)
    for i, h in enumerate(hs):
        h.next(X0[i])
        sl = h.step_stats()
        row = type(sb)(*[np.asarray(getattr(sb, n))[i] for n in FIELDS], sb.k)
        same_bits(row, sl, "%s member %d" % (tag, i))
        check_last_step(m, hb, lams[i], "%s member %d" % (tag, i), dbg=lambda what, i=i: hb.debug_get(i, what), st=row)


def test_batched_point_mass_rows_are_the_lone_handles(m):
    """B = 3 members with their own lambda, Sigma, seed and goal: row m has the bits of lone handle m's step_stats(), step after step"""
    hb, hs, X0, lams = _batch_pm(m)
    _rows_equal_lone(m, hb, hs, X0, lams, "first")
    _rows_equal_lone(m, hb, hs, X0, lams, "second")
    close(hb, *hs)


def test_batched_auv_rows_are_the_lone_handles(m):
    B = 2
    c = auv_cfg(128, 6, "ellipse3d")
    X0, G, U0 = auv_members(B, 6, seed=3)
    seeds = [5, 18]
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hb.set_action_sequences(U0)
    hs = lone_handles(m, [c] * B, seeds, G, U0, "mppi::k_rollout_auv_pc<")
    _rows_equal_lone(m, hb, hs, X0, [1.0] * B, "auv")
    close(hb, *hs)


def _host_loop_with_stats(h, x0, n_steps, goals, disturbance, plant=None):
    """episode_util.host_loop's order with step_stats() taken after every step"""
    x = np.asarray(x0, F32).copy()
    out = []
    for t in range(n_steps):
        h.set_goal(goals[t])
        h.state_cost(x)
        u = h.next(x)
        out.append(h.step_stats())
        x = (plant or h).model_next(x, u)[0] + np.asarray(disturbance[t], F32)
    return out


@pytest.mark.parametrize("case", ["one_launch", "two_launches", "plant"])
def test_lone_episode_logs_every_step(m, case):
    """4 + 2 steps in two calls, a goal per step and a disturbance: X, U, C, the final sequence and the step counter are the plain
    episode's; row t of the statistics is step_stats() after step t of the host loop"""
    K = 8256 if case == "two_launches" else 256
    c, calls = pm_cfg(K, 8, 2), (4, 2)
    n = sum(calls)
    G, W = signals(n, 4, seed=5)
    he, hp, hh = (m.Handle(**c) for _ in range(3))
    plant = m.Handle(k=1, tau=1, s_dim=4, a_dim=2, dt=0.1, mass=1.7) if case == "plant" else None
    x, t = pm_x0(2), 0
    host = _host_loop_with_stats(hh, x, n, G, W, plant)
    for k in calls:
        sl = slice(t, t + k)
        X, U, Cs, st = he.run_episode(x, k, G[sl], W[sl], plant=plant, stats=True)
        Xp, Up, Cp = hp.run_episode(x, k, G[sl], W[sl], plant=plant)
        for got, want, what in ((X, Xp, "X"), (U, Up, "U"), (Cs, Cp, "C")):
            np.testing.assert_array_equal(got, want, err_msg="%s steps %d..%d" % (what, t, t + k))
        assert st.k == K and st.ess.shape == (k,) and st.hist_weight.shape == (k, 32) and st.best_index.dtype.kind == "i"
        for j in range(k):
            row = type(st)(*[np.asarray(getattr(st, f))[j] for f in FIELDS], st.k)
            same_bits(row, host[t + j], "%s step %d" % (case, t + j))
        x, t = X[-1], t + k
    for other in (hp, hh):
        np.testing.assert_array_equal(he.get_action_sequence(), other.get_action_sequence())
        assert he.get_step_counter() == other.get_step_counter() == n
    same_bits(he.step_stats(), host[-1], "the last step, asked afterwards")
    close(he, hp, hh, *([plant] if plant else []))


def test_batched_episode_logs_every_step(m):
    """B = 3, 4 + 2 steps in two calls with goals and a disturbance per member: the plain batched episode in X, U, C and where the handle
    ends; row [t, m] is the batched host loop's step_stats() after step t (fed the episode's own states, which are the plain episode's)"""
    B, calls = 3, (4, 2)
    n = sum(calls)
    he, hs, X0, _ = _batch_pm(m, B)
    hp, hs2, _, _ = _batch_pm(m, B)
    hh, hs3, _, _ = _batch_pm(m, B)
    close(*hs, *hs2, *hs3)
    rng = np.random.default_rng(21)
    goals = np.zeros((n, B, 4), F32)
    goals[:, :, 0::2] = rng.uniform(-1, 1, (n, B, 2))
    dist = rng.uniform(-0.05, 0.05, (n, B, 4)).astype(F32)
    x, t = X0, 0
    for k in calls:
        sl = slice(t, t + k)
        X, U, Cs, st = he.run_episode(x, k, goals[sl], dist[sl], stats=True)
        Xp, Up, Cp = hp.run_episode(x, k, goals[sl], dist[sl])
        for got, want, what in ((X, Xp, "X"), (U, Up, "U"), (Cs, Cp, "C")):
            np.testing.assert_array_equal(got, want, err_msg="%s steps %d..%d" % (what, t, t + k))
        assert st.ess.shape == (k, B) and st.hist_cost.shape == (k, B, 32)
        for j in range(k):
            hh.set_goals(goals[t + j])
            np.testing.assert_array_equal(hh.next(X[j]), U[j])
            row = type(st)(*[np.asarray(getattr(st, f))[j] for f in FIELDS], st.k)
            same_bits(row, hh.step_stats(), "batched step %d" % (t + j))
        x, t = X[-1], t + k
    for other in (hp, hh):
        np.testing.assert_array_equal(he.get_action_sequences(), other.get_action_sequences())
        assert he.get_step_counter() == other.get_step_counter() == n
    close(he, hp, hh)


def test_refusals(m):
    """each refusal has its status, names its cause, enqueues nothing and leaves the handle usable"""
    from mppi_tf_amd import _lib
    c = pm_cfg(256, 8, 2)
    x = pm_x0(2)

    def refused(fn, status, word):
        with pytest.raises(m.MppiError) as e:
            fn()
        assert e.value.status == status and word in str(e.value), str(e.value)

    h = m.Handle(**c)
    refused(h.step_stats, _lib.ERR_INVALID_ARG, "no step has run")
    assert h.get_step_counter() == 0
    h.next(x)
    check_last_step(m, h, 1.0, "after a refusal")
    hb = m.BatchHandle(n=2, **{k: v for k, v in c.items() if k != "seed"})
    refused(hb.step_stats, _lib.ERR_INVALID_ARG, "no step has run")
    refused(lambda: hb._step_stats("mppi_step_stats", (2,)), _lib.ERR_UNSUPPORTED, "mppi_batch_step_stats")
    refused(lambda: h._step_stats("mppi_batch_step_stats", ()), _lib.ERR_INVALID_ARG, "not a batched handle")
    refused(lambda: hb._run_episode("mppi_run_episode", (2,), np.stack([x, x]), 2, None, None, stats=True), _lib.ERR_UNSUPPORTED,
            "mppi_batch_run_episode_stats")
    refused(lambda: h._run_episode("mppi_batch_run_episode", (), x, 2, None, None, stats=True), _lib.ERR_INVALID_ARG, "not a batched handle")
    assert hb.get_step_counter() == 0 and h.get_step_counter() == 1
    hb.next(np.stack([x, x]))
    assert hb.step_stats().ess.shape == (2,)
    same_bits(h.step_stats(), h.step_stats(), "the lone handle after the refusals")
    hs = m.Handle(shard_rank=0, shard_count=2, **c)  # nothing is ever launched on it
    refused(hs.step_stats, _lib.ERR_UNSUPPORTED, "sharded")
    refused(lambda: hs.run_episode(x, 2, stats=True), _lib.ERR_UNSUPPORTED, "sharded")
    assert hs.get_step_counter() == 0
    # mppi_update leaves its own beta and eta beside the last step's costs: refused until the next step
    K = 256
    h.update(np.linspace(1, 2, K).astype(F32), np.zeros((K, 8, 2), F32), np.zeros((8, 2), F32))
    refused(h.step_stats, _lib.ERR_INVALID_ARG, "mppi_update")
    h.next(x)
    check_last_step(m, h, 1.0, "after mppi_update and a step")
    close(h, hb, hs)
