"""The instance matrix on the GPU: every reachable k_rollout_pc / k_step_pc<.., STEP_FUSE> / k_rollout_pc_batch instance is launched at its
geometry's edge horizons (tests/pc_matrix_util.py) at K = 160 for two control steps and held to the CPU oracle; that every case is fit to
judge a kernel is proven on the CPU by tests/test_pc_matrix_oracle.py. Needs an MI355X: every test is marked `gpu`.

Bars, each the suite's own: the noise the step drew within 5e-6 of the oracle's restatement; sample costs BIT-IDENTICAL to the fp32 oracle's
on that noise (COST 0, 1, 2 in the plain pass); u, U' and the shifted sequence within U_TOL = 1e-5; the weights sum to 1 within 1e-5;
beta is the smallest cost. normalizeCost (the cost pass + the weights pass): test_normalize_cost_on_the_fused_path's bars against the fp64
oracle — costs rtol 2e-6, U' U_TOL, weights rtol 2e-4. fp_contract (COST 3): test_contracted_instance_against_fp64's — costs within
max(2e-6, 1.25 x the unfused fp32 evaluation's own distance) of the fp64 evaluation, U' U_TOL. The one-launch step and every batch member
are also the two-launch lone handle bit for bit (u, U', costs, beta, eta, the sequence).

Measured on an MI355X over the 293 instances (largest distance per bar): noise 5.4e-7; u, U', sequence 2.4e-7 (normalizeCost 8.7e-7,
fp_contract 7.4e-7); sum of the weights 1.3e-7; normalizeCost costs 9.1e-7 and weights 3.1e-5 relative; contracted costs 0.38 x their bar
(7.6e-7 relative); every bit-for-bit comparison holds.

The two bars that are relative to a sample's own cost have a test of their own (test_relative_cost_bars, 288 steps), and their cases aim at
a goal 100 x as far (an ellipse of 10 x the axes) than the other cases. Next to the near goal these bars judged the case, not the kernel:
  fp_contract: the C++ action cost's lambda u' Sigma^-1 eps (lambda in the hundreds to thousands by the matrix's rule) cancels against the
  state cost: single samples cost 3.4 among costs of 6.7e3, the unfused fp32 oracle is itself 1e-5 .. 4e-5 from the fp64 one, and the
  contracted kernel missed max(2e-6, 1.25 x unfused) in 16 steps, at worst 5.8 x (2.3e-4 relative = 1.6 ulp of the sums that sample is made
  of), while u and U' held to 3.0e-7;
  normalizeCost: 4 steps of 3 cases at H = 160 missed rtol 2e-6 (2.01e-6 .. 2.34e-6) where the fp32 ORACLE's own costs are 1.3e-6 .. 3.5e-6
  from the fp64 ones whatever the seed (ten tried per case): the point mass passes the goal, or crosses the ellipse, within the horizon.
No seed or multiplier mends either (pc_matrix_util.cost_conditioning). At the far goal the CPU file proves, as condition (d), that the
fp32 oracle's costs are within 1e-6 of the fp64 ones for every one of these cases (worst 8.3e-7), and every step meets its bar.

The library names one kernel per handle (rollout_kernel_name): for a normalizeCost step that is the weights pass; the cost pass that the
same call launches before it is named from the restated pick rule.
"""
import numpy as np
import pytest

import pc_matrix_util as pm

pytestmark = pytest.mark.gpu
F32 = np.float32
U_TOL = pm.U_TOL
NOISE_TOL = 5e-6
RAN = set()       # the names that ran
ENTERED = set()   # the matrix tests that ran
SEEN = {}         # bar -> the largest distance observed
RELATIVE = {}     # group -> [(case and step, relative distance of the costs, its bar)]: measured by the group's test, asserted by test_relative_cost_bars


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def see(bar, value):
    SEEN[bar] = max(SEEN.get(bar, 0.0), float(value))


class Lone:
    def __init__(self, h):
        self.h = h

    def dbg(self, what):
        return self.h.debug_get(what)

    def sequence(self):
        return self.h.get_action_sequence()


class Member:
    def __init__(self, hb, i):
        self.hb, self.i = hb, i

    def dbg(self, what):
        return self.hb.debug_get(self.i, what)

    def sequence(self):
        return self.hb.get_action_sequences()[self.i]


def snapshot(m, view, u):
    """what one step left: the bits the one-launch step, a batch member and the two-launch lone handle must share"""
    return dict(u=np.array(u), costs=view.dbg(m.DBG_COSTS), beta=float(view.dbg(m.DBG_BETA)), eta=float(view.dbg(m.DBG_ETA)),
                Uupd=view.dbg(m.DBG_U_UPDATED), seq=view.sequence())


def assert_same_bits(got, want, tag):
    for key in ("u", "costs", "Uupd", "seq"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (tag, key))
    assert got["beta"] == want["beta"] and got["eta"] == want["eta"], (tag, got["beta"], want["beta"], got["eta"], want["eta"])


def check_step(m, view, c, mk, p32, p64, U_in, step, snap, relative):
    """one step of case c (it read the sequence U_in) against the oracle on the noise the step drew; the two bars that are relative to a
    sample's cost (normalizeCost, fp_contract) are measured into `relative` and asserted by test_relative_cost_bars"""
    tag, x, nrm = "%s step %d" % (c["id"], step), mk["x"], c["normalize"]
    eps = view.dbg(m.DBG_NOISE)
    d_noise = np.abs(eps - pm.noise(c, step)).max()
    see("noise", d_noise)
    assert d_noise <= NOISE_TOL, "%s: the noise is %.3g from the oracle's restatement" % (tag, d_noise)
    costs = snap["costs"]
    if nrm:
        u_ref, Us_ref, c_ref = p64.next_with_noise(x, U_in, eps, normalize=True)
        rel = np.abs(costs - c_ref) / np.abs(c_ref)
        see("normalize: costs (rtol 2e-6)", rel.max())
        relative.append((tag, float(rel.max()), 2e-6))
        cn = (c_ref - c_ref.min()) / (c_ref.max() - c_ref.min())
        w_ref = np.exp(-cn / mk["lam"])
        w_ref /= w_ref.sum()
        w = view.dbg(m.DBG_WEIGHTS).astype(np.float64)
        see("normalize: weights (rtol 2e-4)", (np.abs(w - w_ref) / np.maximum(w_ref, 1e-5)).max())
        np.testing.assert_allclose(w, w_ref, rtol=2e-4, atol=1e-9, err_msg=tag)
        bar = "normalize: "
    elif c["fp_contract"]:
        c64 = np.asarray(p64.rollout_cost(x.astype(np.float64), U_in.astype(np.float64), eps.astype(np.float64)), np.float64)
        u_ref, Us_ref, c32 = p32.next_with_noise(x, U_in, eps)
        rel = np.abs(costs.astype(np.float64) - c64) / np.maximum(np.abs(c64), 1e-30)
        rel32 = np.abs(c32.astype(np.float64) - c64) / np.maximum(np.abs(c64), 1e-30)
        see("fp_contract: costs / max(2e-6, 1.25 x unfused)", rel.max() / max(2e-6, 1.25 * rel32.max()))
        relative.append((tag, float(rel.max()), float(max(2e-6, 1.25 * rel32.max()))))
        bar = "fp_contract: "
    else:
        u_ref, Us_ref, c_ref = p32.next_with_noise(x, U_in, eps)
        np.testing.assert_array_equal(costs, c_ref, err_msg=tag + ": costs")
        assert snap["beta"] == float(costs.min()), (tag, snap["beta"], costs.min())
        bar = ""
    Uupd_ref = pm.updated(u_ref, Us_ref)
    d = max(np.abs(snap["u"] - u_ref).max(), np.abs(snap["Uupd"] - Uupd_ref).max(), np.abs(snap["seq"] - Us_ref).max())
    see(bar + "u, U', sequence (1e-5)", d)
    np.testing.assert_allclose(snap["u"], u_ref, rtol=0, atol=U_TOL, err_msg=tag + ": u")
    np.testing.assert_allclose(snap["Uupd"], Uupd_ref, rtol=0, atol=U_TOL, err_msg=tag + ": U'")
    np.testing.assert_allclose(snap["seq"], Us_ref, rtol=0, atol=U_TOL, err_msg=tag + ": shifted sequence")
    wsum = float(view.dbg(m.DBG_WEIGHTS).astype(np.float64).sum())
    see("sum of the weights (1e-5)", abs(wsum - 1.0))
    assert abs(wsum - 1.0) <= 1e-5, (tag, wsum)


def named(h, c, tag):
    """the handle runs the instance the restated rules give; -> the names one step of it launches"""
    name, want = h.rollout_kernel_name(), pm.expected_name(c)
    assert pm.name_matches(name, want), "%s runs %s, not %s" % (tag, name, want)
    return [pm.fmt(i) for i in pm.route(c)[:-1]] + [name]


def run_lone(m, c, memo):
    """case c on a lone handle for STEPS steps, each against the oracle; -> the steps' snapshots (memo: by case id, within one test)"""
    if c["id"] in memo:
        return memo[c["id"]]
    mk = pm.make_case(c)
    h = m.Handle(**mk["handle"])
    names = named(h, c, c["id"])
    p32, p64 = pm.problems(mk)
    h.set_action_sequence(mk["U"])
    U_in, snaps = mk["U"], []
    for step in range(pm.STEPS):
        u = h.next(mk["x"])
        snaps.append(snapshot(m, Lone(h), u))
        check_step(m, Lone(h), c, mk, p32, p64, U_in, step, snaps[-1], memo.setdefault("relative", []))
        U_in = snaps[-1]["seq"]
    assert h.get_step_counter() == pm.STEPS
    h.close()
    RAN.update(n for n in names if "k_rollout_tile" not in n)
    memo[c["id"]] = snaps
    return snaps


def run_batch(m, pair, memo):
    """two members with their own seed, goal and lambda in one k_rollout_pc_batch launch: each the lone handle bit for bit, member 1 also
    against the oracle"""
    c0, mks = pair[0], [pm.make_case(c) for c in pair]
    kw = {k: v for k, v in mks[0]["handle"].items() if k not in ("lam", "goal", "seed", "tuning")}
    tuning = {"pc_producers": 3} if c0["producers"] == 3 else None
    hb = m.BatchHandle(2, seeds=[c["seed"] for c in pair], lams=[mk["lam"] for mk in mks], goals=[mk["handle"]["goal"] for mk in mks], tuning=tuning, **kw)
    names = named(hb, pm.batch_cfg(pair), "batch of " + c0["id"])
    lone = [run_lone(m, c, memo) for c in pair]
    hb.set_action_sequences(np.stack([mk["U"] for mk in mks]))
    p32, p64 = pm.problems(mks[1])
    U_in = mks[1]["U"]
    for step in range(pm.STEPS):
        u = hb.next(np.stack([mk["x"] for mk in mks]))
        for i in range(2):
            snap = snapshot(m, Member(hb, i), u[i])
            assert_same_bits(snap, lone[i][step], "batch of %s member %d step %d" % (c0["id"], i, step))
            if i == 1:
                check_step(m, Member(hb, 1), pair[1], mks[1], p32, p64, U_in, step, snap, memo.setdefault("relative", []))
                U_in = snap["seq"]
    hb.close()
    RAN.update(names)


@pytest.mark.parametrize("group", pm.groups(), ids=pm.group_id)
def test_instances_of_the_geometry_against_the_oracle(m, group):
    memo = {}
    for c in pm.lone_cases(*group):
        run_lone(m, c, memo)
    for fused, two in pm.fused_cases(*group):
        f, t = run_lone(m, fused, memo), run_lone(m, two, memo)
        for step in range(pm.STEPS):
            assert_same_bits(f[step], t[step], "%s against the two launches, step %d" % (fused["id"], step))
    for pair in pm.batch_cases(*group):
        run_batch(m, pair, memo)
    RELATIVE[group] = memo.get("relative", [])
    ENTERED.add(group)


@pytest.mark.parametrize("group", [g for g in pm.groups() if g[1][0] != 7], ids=pm.group_id)
def test_relative_cost_bars(m, group):
    """the two bars that are relative to a sample's own cost, on the group's normalizeCost and fp_contract cases: costs within rtol 2e-6 of
    the fp64 oracle's; contracted costs within max(2e-6, 1.25 x the unfused fp32 evaluation's distance) of the fp64 evaluation"""
    if group not in RELATIVE:  # (this test alone: measure now)
        memo = {}
        for c in pm.lone_cases(*group):
            if c["normalize"] or c["fp_contract"]:
                run_lone(m, c, memo)
        RELATIVE[group] = memo["relative"]
    assert len(RELATIVE[group]) > 0
    for tag, rel, bar in RELATIVE[group]:
        print("%s: costs %.3g relative, bar %.3g%s" % (tag, rel, bar, "" if rel <= bar else "  MISSED"))
    missed = ["%s: %.3g > %.3g" % t for t in RELATIVE[group] if t[1] > t[2]]
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("a", pm.A_DIMS)
def test_routing_edges_by_name(m, a):
    """H = 161, and H = 133 on three producers, run k_rollout_tile; H = 84 / 85 with the default tuning the seven- and the five-producer
    one-launch step; the horizons whose 64-rollout LDS image no longer fits (a = 4: H >= 155) the tile kernel — each still against the oracle"""
    for c, inst in pm.routing_cases(a):
        assert pm.route(c) == [inst], (c["id"], pm.route(c), inst)
        run_lone(m, c, {})
    ENTERED.add(a)


def test_the_names_that_ran_are_the_reachable_set():
    print("\n".join(sorted(RAN)))
    print("%d instances ran; largest distances observed:" % len(RAN))
    for bar in sorted(SEEN):
        print("  %-50s %.3g" % (bar, SEEN[bar]))
    reachable = {pm.fmt(i) for i in pm.reachable_instances()}
    assert RAN <= reachable, sorted(RAN - reachable)
    if ENTERED >= set(pm.groups()) | set(pm.A_DIMS):  # (a run of part of this file has launched part of the set)
        assert RAN == reachable, "reachable, but never launched: %s" % sorted(reachable - RAN)
        assert len(RAN) == 216 + 21 + 56
