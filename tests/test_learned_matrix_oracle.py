"""The instance matrix of the learned-model rollout kernels (tests/learned_matrix_util.py, run on the GPU by tests/test_learned_matrix_gpu.py),
proven on the CPU before a GPU sees it.

Completeness: every instance of the learned families in libmppi_hip.so (k_rollout_mlp, _mlp2, _mlp_bx3, _mlp32, _mlp32_bx3, _mlp32_pc,
_mlp_small, _mlp2_batch, _mlp_small_batch, _nnauv32, _nnauv32_bx3, _nnauv_pc, _nnspeed32, _nnspeed_pc, _gen, _nn_batch; read from the
library's mangled names) is launched by a case of the matrix or stands in the exclusion table with its reason; the matrix launches exactly
what the restated creation, tuning and pick rules can reach. A new instance with neither a case nor an entry fails here.

Conditions: every K = 160 case the GPU file compares with the oracle is, over its two Philox steps and its injected-noise step and on the
oracle's restatement of the noise (orc.noise), (a) well conditioned: the fp32 oracle's U' within a quarter of the case's U' bar (1e-5;
split-bf16 2e-5) of the fp64 oracle's; (b) not blind: no sample holds more than 0.9 of the weight; (c) in need of every tile: leaving out
any one of the three tiles moves the fp64 U' by at least 50 x 1e-5. Each case's lambda is float32(3 x (c_sorted[8] - c_min)) from the fp64
oracle's costs at lambda = 1 (learned_matrix_util.lam_of). The cases of every other K (1, 33, 64, 65, the tile walkers' 64 n_cu + 1, the
pipelines' 32768 + 65 and 65536 + 1) cannot meet (c) and are held to (a), (b) (K = 1: its one sample holds the weight) and (d).

(d), which the first run of the matrix added: the fp32 oracle's sample costs within 2e-5 / 4 (split-bf16: 2e-5 / 8) relative of the fp64 oracle's,
so that of the two bars on a sample's cost the one relative to the fp32 oracle's own distance is the one that binds (the C++ action cost is
signed, and one sample's cost can land next to zero: learned_matrix_util.cost_cond_max).

Measured over the 432 oracle problems of the matrix (93 of them at another K): worst (a) 0.129 of the case's bar (the bound: 0.25), worst (b)
0.108, worst (c) 5.57e-4, worst (d) 7.9e-7. Three problems broke a condition with their first seed and got another
(learned_matrix_util.ADJUST, each with its figures). The 13-state cases aim at a goal half a metre from the start: at the four metres of
tests/test_auv_gpu.py's goal 39 of the 99 13-state problems broke (a) whatever the seed (learned_matrix_util.GOAL13).
"""
import numpy as np
import pytest

import learned_matrix_util as lm

WORST = {"a": 0.0, "b": 0.0, "c": np.inf, "rel": 0.0, "n": 0}


@pytest.fixture(scope="module")
def compiled():
    import __graft_entry__
    so = __graft_entry__.build()
    with open(so, "rb") as fh:
        return lm.compiled_instances(fh.read())


def test_every_compiled_instance_has_a_case_or_a_reason(compiled):
    covered, reachable = lm.matrix_instances(), set(lm.reachable_instances())
    excluded = {i: lm.exclusion(i) for i in compiled if lm.exclusion(i) is not None}  # the exclusion table: instance -> reason
    for group in lm.COUNTED:
        n = lambda s: lm.family_count(s, group)
        print("%s: compiled %d, covered %d, reachable %d, excluded %d" % (group, n(compiled), n(covered), n(reachable), n(excluded)))
    for i, r in sorted(excluded.items()):
        print("  excluded %s: %s" % (lm.fmt(i), r))
    assert {i[0] for i in compiled} == set(lm.FAMILIES), "families without an instance name in the library: %s" % sorted(set(lm.FAMILIES) - {i[0] for i in compiled})
    assert not covered & set(excluded), "excluded and covered: %s" % sorted(covered & set(excluded))
    missing = compiled - covered - set(excluded)
    assert not missing, "compiled, but neither launched by the matrix nor excluded with a reason: %s" % sorted(lm.fmt(i) for i in missing)
    assert covered <= compiled, "the matrix expects instances the library does not hold: %s" % sorted(lm.fmt(i) for i in covered - compiled)
    assert covered == reachable, (sorted(lm.fmt(i) for i in covered - reachable), sorted(lm.fmt(i) for i in reachable - covered))
    # the counts the rules give. Lone point mass: k_rollout_mlp 7 (A x DIAG without <1, false>), _mlp2 5 + 3 injected, _mlp_bx3 7 + 4 injected,
    # _mlp32 4, _mlp32_bx3 4, _mlp32_pc 7, _mlp_small 4 x 2. Batched point mass: _mlp2_batch 5, _mlp_small_batch 8. Lone 13-state: _nnauv32 2,
    # _nnauv32_bx3 2, _nnauv_pc 2, _nnspeed32 4, _nnspeed_pc 4, _gen 2 x 2 x 2. Batched 13-state: _nn_batch 8.
    assert [lm.family_count(covered, g) for g in lm.COUNTED] == [49, 13, 22, 8]
    assert [lm.family_count(compiled, g) for g in lm.COUNTED] == [53, 14, 24, 8]
    assert len(excluded) == 7


def test_restated_rules_at_their_thresholds():
    """the rules as the code states them, at every threshold"""
    name = lambda **kw: lm.expected_name(dict(dict(kind="pm", a=3, hid=256, nh=2), **kw))
    inj = lambda **kw: lm.fmt(lm.route(dict(dict(kind="pm", a=3, hid=256, nh=2), **kw), "noise")[0])
    # mlp_v2: a = 3 against a = 4; mlp_v1; the noise source a template argument, injected noise always the dense-Sigma arithmetic
    assert name() == "mppi::k_rollout_mlp2<3, true, 0>" and name(a=4) == "mppi::k_rollout_mlp<4, true>"
    assert name(dense=True) == "mppi::k_rollout_mlp2<3, false, 0>" and name(a=1, dense=True) == "mppi::k_rollout_mlp2<1, true, 0>"
    assert inj() == "mppi::k_rollout_mlp2<3, false, 1>" and inj(a=1) == "mppi::k_rollout_mlp2<1, false, 1>" and inj(a=4, dense=True) == "mppi::k_rollout_mlp<4, false>"
    assert name(tuning={"mlp_v1": 1}) == "mppi::k_rollout_mlp<3, true>" and name(tuning={"mlp_v1": 0}) == "mppi::k_rollout_mlp2<3, true, 0>"
    assert name(a=4, tuning={"mlp_v1": 0}) == "mppi::k_rollout_mlp<4, true>"
    assert name(bx3=True, a=4, dense=True) == "mppi::k_rollout_mlp_bx3<4, false, 0>" and inj(bx3=True) == "mppi::k_rollout_mlp_bx3<3, false, 1>"
    # hidden 16 against 32 against 256, 64 refused; mlp32_valu 0, 1, 2; the split-bf16 flag refused at hidden 16
    small = lambda hid, **kw: name(hid=hid, nh=3, **kw)
    assert small(16) == "mppi::k_rollout_mlp_small<3, 16>" and small(32, dense=True) == "mppi::k_rollout_mlp32_pc<3, false>"
    assert small(32, tuning={"mlp32_valu": 0}) == "mppi::k_rollout_mlp32_pc<3, true>" and small(32, tuning={"mlp32_valu": 1}) == "mppi::k_rollout_mlp_small<3, 32>"
    assert small(32, tuning={"mlp32_valu": 2}) == "mppi::k_rollout_mlp32<3>" and small(32, bx3=True) == "mppi::k_rollout_mlp32_bx3<3>"
    for bad in (dict(hid=64), dict(hid=16, nh=3, bx3=True), dict(hid=256, nh=3), dict(hid=32, nh=4), dict(hid=16, nh=1, tuning={"mlp32_valu": 1}),
                dict(hid=32, nh=1, tuning={"mlp32_valu": 3}), dict(hid=32, nh=1, bx3=True, tuning={"mlp32_valu": 1}), dict(hid=32, nh=1, tuning={"mlp_v1": 1}),
                dict(a=5), dict(a=4, batch=True), dict(batch=True, tuning={"mlp_v1": 1}), dict(batch=True, normalize=True), dict(batch=True, bx3=True),
                dict(kind="nnspeed", a=6, hid=32, nh=1, bx3=True), dict(kind="nnauv", a=6, hid=16, nh=1, tuning={"mlp32_valu": 1}),
                dict(kind="nnauv", a=6, hid=16, nh=1, bx3=True), dict(kind="nnauv", a=6, hid=256, nh=2)):
        with pytest.raises(lm.Refused):
            lm.create(dict(dict(kind="pm", a=3, hid=256, nh=2), **bad))
    # the batched point mass
    assert name(batch=True, dense=True) == "mppi::k_rollout_mlp2_batch<3, false>" and small(32, batch=True, a=4) == "mppi::k_rollout_mlp_small_batch<4, 32>"
    # the 13-state models: pick_gen and its fast_mode
    gen = lambda kind, hid, **kw: dict(kind=kind, a=6, hid=hid, nh=2, **kw)
    assert lm.expected_name(gen("nnauv", 32)) == "mppi::k_rollout_nnauv_pc<true>" and lm.expected_name(gen("nnauv", 16, dense=True)) == "mppi::k_rollout_gen<1, 16, false>"
    assert lm.expected_name(gen("nnauv", 32, tuning={"mlp32_valu": 2})) == "mppi::k_rollout_nnauv32<true>"
    assert lm.expected_name(gen("nnauv", 32, tuning={"mlp32_valu": 1})) == "mppi::k_rollout_gen<1, 32, true>"
    assert lm.expected_name(gen("nnauv", 32, bx3=True, dense=True)) == "mppi::k_rollout_nnauv32_bx3<false>"
    assert lm.expected_name(gen("nnspeed", 16)) == "mppi::k_rollout_nnspeed_pc<16, true>" and lm.expected_name(gen("nnspeed", 32, tuning={"mlp32_valu": 2})) == "mppi::k_rollout_nnspeed32<32, true>"
    assert lm.expected_name(gen("nnspeed", 16, tuning={"mlp32_valu": 1})) == "mppi::k_rollout_gen<2, 16, true>"
    assert lm.expected_name(gen("nnspeed", 32, batch=True, dense=True)) == "mppi::k_rollout_nn_batch<2, 32, false>"
    st = lm.create(gen("nnauv", 32))
    assert lm.pick_gen(gen("nnauv", 32), st, lm.MODE_COST_ONLY, False, 160)[0] == ("nnauv_pc", True)
    assert lm.pick_gen(gen("nnauv", 32), st, lm.MODE_COSTS_GIVEN, False, 160)[0] == ("gen", 1, 32, True)
    assert lm.pick_gen(gen("nnauv", 32), st, lm.MODE_ROLLOUT, True, 160)[0] == ("gen", 1, 32, True)   # a noise export
    assert [lm.fmt(i) for i in lm.route(gen("nnspeed", 32, normalize=True))] == ["mppi::k_rollout_nnspeed_pc<32, true>", "mppi::k_rollout_gen<2, 32, true>"]
    assert lm.route(dict(kind="pm", a=3, hid=32, nh=3, normalize=True)) == [("mlp32_pc", 3, True), ("tile", 3)]
    # the grids: min(nb, n_cu) for the tile walkers, (nb + 1) / 2 for the two-tile pipelines; the balance off at 2 n_cu + 1 workgroups
    grid = lambda cfg, k: lm.route(cfg, "next", k, grids=True)[0][1]
    wide, pipe = dict(kind="pm", a=2, hid=256, nh=2), dict(kind="pm", a=3, hid=32, nh=2)
    assert [grid(wide, k) for k in (1, 64, 65, 64 * 256, 64 * 256 + 1, 65536)] == [1, 1, 2, 256, 256, 256]
    assert [grid(dict(wide, bx3=True), k) for k in (65, 64 * 256 + 1)] == [2, 256] and grid(dict(wide, tuning={"mlp_v1": 1}), 64 * 256 + 1) == 257
    assert [grid(pipe, k) for k in (64, 65, 160, 32768 + 65, 65536, 65536 + 1)] == [1, 1, 2, 257, 512, 513]
    assert [grid(gen("nnspeed", 16), k) for k in (64, 160, 65536 + 1)] == [1, 2, 513] and grid(gen("nnauv", 32, tuning={"mlp32_valu": 2}), 160) == 3
    on, off = lm.create(pipe), lm.create(dict(pipe, tuning={"pc_balance": 0}))
    assert [lm.two_tile_balance(on, w) for w in (1, 257, 512, 513)] == [1, 1, 1, 0] and [lm.two_tile_balance(off, w) for w in (1, 513)] == [0, 0]
    assert lm.two_tile_balance(lm.create(dict(pipe, tuning={"pc_balance": 1})), 512) == 1
    # the shapes: the last workgroup of a pipeline at K = 160 has no second tile; past workgroup 255; 513 workgroups
    assert lm.tiles(160) == 3 and grid(pipe, 160) * 2 > lm.tiles(160) and lm.tiles(32768 + 65) == 514 and lm.tiles(65536 + 1) == 1025
    ids = [c["id"] for g in lm.lone_groups() for c in lm.lone_cases(*g)]
    assert len(ids) == len(set(ids))


def judge(cases, loo):
    bad = []
    for c in cases:
        cond, wmax, move, rel = lm.conditions(c, loo)
        WORST.update(a=max(WORST["a"], cond / lm.u_bar(c)), b=max(WORST["b"], wmax if c["K"] > 1 else 0.0), c=min(WORST["c"], move), rel=max(WORST["rel"], rel), n=WORST["n"] + 1)
        if not (cond <= lm.u_bar(c) / lm.COND_FRACTION and (wmax <= lm.W_MAX or c["K"] == 1) and (move >= lm.TILE_MIN or not loo) and rel <= lm.cost_cond_max(c)):
            bad.append("%s (seed %d, lambda %.4g): (a) %.3g (b) %.4f (c) %.3g (d) %.3g" % (c["key"], c["seed"], lm.lam_of(c), cond, wmax, move, rel))
    print("%d oracle problems; worst so far over %d: (a) %.3g of the bar (b) %.4f (c) %.3g (d) %.3g"
          % (len(cases), WORST["n"], WORST["a"], WORST["b"], WORST["c"], WORST["rel"]))
    assert not bad, "cases that break a condition (give them another seed or multiplier in learned_matrix_util.ADJUST):\n" + "\n".join(bad)


@pytest.mark.parametrize("kind,a", [("pm", 1), ("pm", 2), ("pm", 3), ("pm", 4), ("nnauv", 6), ("nnspeed", 6)])
def test_every_case_meets_the_conditions(kind, a):
    cases = [c for c in lm.oracle_cases().values() if (c["kind"], c["a"]) == (kind, a)]
    assert len(cases) >= 30
    judge(cases, True)


def test_the_other_shapes_are_well_conditioned():
    """K other than 160: (a) and (b) (leaving out a tile of 1025 moves nothing by 5e-4, and K <= 64 has one tile)"""
    cases = list(lm.oracle_cases(None).values())
    assert len(cases) >= 20
    judge(cases, False)
