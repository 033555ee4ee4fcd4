"""The instance matrix of the point-mass producer/consumer kernels (tests/pc_matrix_util.py, run on the GPU by tests/test_pc_matrix_gpu.py),
proven on the CPU before a GPU sees it.

Completeness: every k_rollout_pc / k_step_pc / k_rollout_pc_batch instance in libmppi_hip.so (read from the library's mangled names) is
launched by a case of the matrix or stands in the exclusion table with its reason; the matrix launches exactly what the restated pick
rules can reach. A new instance with neither a case nor an entry fails here.

Conditions: every case the GPU file compares with the oracle is, over both of its steps and on the oracle's restatement of the noise
(orc.noise), (a) well conditioned: the fp32 oracle's U' within U_TOL / 4 = 2.5e-6 of the fp64 oracle's, so the GPU bar tests the kernel and
not the case; (b) not blind: no sample holds more than 0.9 of the weight (at lambda = 1, K = 160 and H >= 80 one sample holds all of it
and the update sees no other lane); (c) in need of every tile: leaving out any one of the three tiles moves the fp64 U' by at least
50 x U_TOL = 5e-4. Each case's lambda is float32(3 x (c_sorted[8] - c_min)) from the fp64 oracle's costs at lambda = 1 (pc_matrix_util.lam_of).

(d), for the fp_contract and normalizeCost cases, whose costs are held to a bar relative to each sample's own cost: the fp32 oracle's costs within 1e-6
relative of the fp64 oracle's (pc_matrix_util.cost_conditioning: why these cases aim at a far goal).

Measured over the 510 oracle problems of the matrix (two steps each): worst (a) 1.81e-6, worst (b) 0.834, worst (c) 1.69e-3, worst (d)
8.3e-7. Eight problems broke a condition with their first seed or multiplier and got another (pc_matrix_util.ADJUST, each with its figures).
"""
import numpy as np
import pytest

import pc_matrix_util as pm

WORST = {"a": 0.0, "b": 0.0, "c": np.inf, "d": 0.0, "n": 0}
FAMILIES = (("pc", "k_rollout_pc"), ("step", "k_step_pc"), ("batch", "k_rollout_pc_batch"))


@pytest.fixture(scope="module")
def compiled():
    import __graft_entry__
    so = __graft_entry__.build()
    with open(so, "rb") as fh:
        return pm.compiled_instances(fh.read())


def test_every_compiled_instance_has_a_case_or_a_reason(compiled):
    covered, reachable = pm.matrix_instances(), set(pm.reachable_instances())
    excluded = {i: pm.exclusion(i) for i in compiled if pm.exclusion(i) is not None}  # the exclusion table: instance -> reason
    for fam, kernel in FAMILIES:
        n = lambda s: sum(1 for i in s if i[0] == fam)
        reasons = sorted({r.split(":")[0] for i, r in excluded.items() if i[0] == fam})
        print("%s: compiled %d, covered %d, reachable %d, excluded %d (%s)" % (kernel, n(compiled), n(covered), n(reachable), n(excluded), ", ".join(reasons)))
    assert len(compiled) > 0 and {f for f, _ in FAMILIES} == {i[0] for i in compiled}, "no instance names found in the library"
    assert not covered & set(excluded), "excluded and covered: %s" % sorted(covered & set(excluded))
    missing = compiled - covered - set(excluded)
    assert not missing, "compiled, but neither launched by the matrix nor excluded with a reason: %s" % sorted(pm.fmt(i) for i in missing)
    assert covered <= compiled, "the matrix expects instances the library does not hold: %s" % sorted(pm.fmt(i) for i in covered - compiled)
    assert covered == reachable, (sorted(pm.fmt(i) for i in covered - reachable), sorted(pm.fmt(i) for i in reachable - covered))
    # the counts the pick rules give: 8 instances per (geometry, DIAG) of k_rollout_pc (6 at a = 1: no ellipse), 3 fused geometries, 4 x 2 batched
    count = lambda fam: sum(1 for i in covered if i[0] == fam)
    assert (count("pc"), count("step"), count("batch")) == (216, 21, 56)
    assert sum(1 for i in compiled if i[0] == "pc") == 240


def test_restated_rules_at_their_thresholds():
    """the rules as the code states them, at every threshold"""
    assert [pm.pc_slots(5, H) for H in (1, 80, 81, 160)] == [4, 4, 8, 8] and [pm.pc_slots(3, H) for H in (1, 72, 73, 132)] == [6, 6, 11, 11]
    assert [pm.reach(a, 5) for a in pm.A_DIMS] == [160, 160, 160, 154] and [pm.reach(a, 3) for a in pm.A_DIMS] == [132] * 4
    assert pm.edge_horizons(4, (5, 8)) == [81, 153, 154] and pm.edge_horizons(3, (5, 8)) == [81, 157, 160]
    name = lambda **kw: pm.expected_name(dict(dict(a=3, H=64, fused_step=0), **kw))
    assert name() == "mppi::k_rollout_pc<3, 5, 4, true, 0, 0>" and name(fused_step=1) == "mppi::k_step_pc<3, 7, 3, true, 1>"
    assert name(H=84, fused_step=1) == "mppi::k_step_pc<3, 7, 3, true, 1>" and name(H=85, fused_step=1) == "mppi::k_step_pc<3, 5, 8, true, 1>"
    assert name(H=80, fused_step=2) == "mppi::k_step_pc<3, 5, 4, true, 1>" and name(H=161) == "mppi::k_rollout_tile<3, 64, "
    assert name(H=133, producers=3) == "mppi::k_rollout_tile<3, 64, " and name(H=132, producers=3, dense_sigma=True) == "mppi::k_rollout_pc<3, 3, 11, false, 0, 0>"
    assert name(normalize=True, cost="dense") == "mppi::k_rollout_pc<3, 5, 4, true, 0, 2>" and name(fp_contract=True) == "mppi::k_rollout_pc<3, 5, 4, true, 3, 0>"
    assert pm.route(dict(a=2, H=64, fused_step=0, normalize=True, cost="ellipse"))[0] == ("pc", 2, 5, 4, True, 1, 1)
    assert name(a=4, H=155) == "mppi::k_rollout_tile<4, 32, " and name(a=1, dense_sigma=True) == "mppi::k_rollout_pc<1, 5, 4, true, 0, 0>"
    assert name(batch=True, cost="dense", producers=3, H=73) == "mppi::k_rollout_pc_batch<3, 3, 11, true, 2>"
    ids = [c["id"] for g in pm.groups() for c in pm.lone_cases(*g)]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("a", pm.A_DIMS)
def test_every_case_meets_the_conditions(a):
    cases = [c for c in pm.oracle_cases().values() if c["a"] == a]
    assert len(cases) > 50
    bad = []
    for c in cases:
        cond, wmax, loo = pm.conditions(c)
        WORST.update(a=max(WORST["a"], cond), b=max(WORST["b"], wmax), c=min(WORST["c"], loo), n=WORST["n"] + 1)
        rel = pm.cost_conditioning(c) if (c["fp_contract"] or c["normalize"]) else 0.0
        WORST["d"] = max(WORST["d"], rel)
        if not (cond <= pm.COND_MAX and wmax <= pm.W_MAX and loo >= pm.TILE_MIN and rel <= pm.COST_COND_MAX):
            bad.append("%s (seed %d, lambda %.4g): (a) %.3g (b) %.4f (c) %.3g (d) %.3g" % (pm.problem_key(c), c["seed"], pm.lam_of(c), cond, wmax, loo, rel))
    print("a = %d: %d oracle problems; worst so far over %d: (a) %.3g (b) %.4f (c) %.3g (d) %.3g" % (a, len(cases), WORST["n"], WORST["a"], WORST["b"], WORST["c"], WORST["d"]))
    assert not bad, "cases that break a condition (give them another seed or multiplier in pc_matrix_util.ADJUST):\n" + "\n".join(bad)
