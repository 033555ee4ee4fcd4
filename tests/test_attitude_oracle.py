"""The attitude matrix (tests/attitude_util.py, run on the GPU by tests/test_attitude_gpu.py), proven on the CPU before a GPU sees it: with the
oracle alone, that every case is fit to judge a kernel and that the set reaches what it claims. Run with -s for the table of cases,
octant counts and straddles.

Conditions: every learned case meets learned_matrix_util.conditions' (a) the fp32 oracle's U' within bar / 4 of the fp64 oracle's, (b) no
sample above 0.9 of the weight, (c) leaving out a tile moves U' by at least 50 x 1e-5, (d) the fp32 oracle's costs within 2e-5 / 4 (split
bf16: / 8) relative of the fp64 oracle's — the learned matrix's bars, unchanged.

Margins, on the fp64 oracle's trajectories: every visited state of an NNAUVModelSpeed case has |roll|, |yaw| <= pi - 1e-3 and |pitch| <=
pi / 2 - 0.05 (asin amplifies by at most 20). Coverage, per NNAUVModelSpeed kernel instance over its cases: each of the eight octants of
yaw and of roll (sign, |angle| > pi / 2, pi / 4 < |angle| < 3 pi / 4) holds at least 64 (sample, step) states, both signs of pitch occur
beyond 1.2. Lane divergence: for each continuous fold of atan2_pose every instance has a case with a horizon step t >= 1 at which one tile
of 64 rollouts has at least 16 samples on each side: the AIMED cases, whose start yaw attitude_util.aim() bisects on the fp64 oracle (the
sample cloud of the matrix's network is ~3e-3 rad wide; no network is scaled).

The Euler path matters: zeroing the three Euler rows of the first layer moves at least a quarter of every speed case's costs by more than
10 x 2e-5 relative; the NNAUVModel attitudes matter: swapping the first layer's rows of q_x and q_y does the same.

The lock case: the fp32 oracle's Euler angles of its x0 are (., -+pi/2, 0) exactly, also with either non-zero component moved by an ulp.

The Fossen cases: the fp32 oracle's costs within attitude_util.FOSSEN_COND of the fp64 oracle's (no sample's cost next to zero); every rk
and cost occurs; the quaternion goal lies on the far hemisphere of every start.

Measured over the 92 learned oracle problems (76 NNAUVModelSpeed, 16 NNAUVModel): worst (a) 0.57 of the bound, worst (b) 0.057, worst (c)
1.6e-2, worst (d) 2.8e-7; no case needed another seed. Every aimed tile splits 31 | 33 or 32 | 32 at its fold. The smallest share of costs
moved: 0.50 without the Euler rows, 0.91 with q_x and q_y swapped. The largest |pitch| visited is 1.36, the nearest approach to the cut
pi - 1.6e-3. The fp32 oracle's Fossen costs: at most 2.0e-7 (quadratic), 2.7e-7 (quat), 1.2e-6 (ellipse3d) relative from the fp64 oracle's.
"""
import numpy as np
import pytest

import attitude_util as au
import learned_matrix_util as lm
from oracle import oracle as orc

F32 = np.float32
PI = np.pi


def test_the_start_attitudes_are_what_their_names_say():
    """by the oracle's own Euler angles, in fp32 and fp64; unit quaternions in fp32; the NNAUVModel ones with every component beyond 0.2"""
    for name, (angles, body) in au.ATTITUDES.items():
        q = au.quaternion(name)
        assert q.dtype == F32 and abs(np.linalg.norm(q.astype(np.float64)) - 1.0) < 1e-7
        for dt in (F32, np.float64):
            # (1e-5: the fp32 rounding of the components, 6e-8, through asin at pitch 1.3 and the fp32 oracle's own arithmetic)
            np.testing.assert_allclose(orc.euler_from_quaternion(q[None], dtype=dt)[0], angles, rtol=0, atol=1e-5, err_msg=name)
        assert 0.5 <= np.linalg.norm(body) <= 2.0
        print("%-10s roll %+.4f pitch %+.4f yaw %+.4f   q = %s   rates %s" % ((name,) + tuple(angles) + (q, body)))
    assert "%.2f" % au.ATTITUDES["roll+3.0"][0][0] == "3.00" and "%.2f" % au.ATTITUDES["roll-1.75"][0][0] == "-1.75"
    assert len({int(au.octant(np.array(a[0][2]))) for a in au.ATTITUDES.values()}) == 8, "the yaw angles: one per octant"
    assert len({int(au.octant(np.array(a[0][0]))) for a in au.ATTITUDES.values()}) == 8, "the roll angles: one per octant"
    qi, qs = au.quaternion("nnauv_inverted"), au.quaternion("nnauv_skew120")
    for q in (qi, qs):
        assert abs(np.linalg.norm(q.astype(np.float64)) - 1.0) < 1e-7 and np.abs(q).min() > 0.2 and (q > 0).any() and (q < 0).any(), q
    assert abs(abs(orc.euler_from_quaternion(qi[None])[0][0]) - PI) < 0.6, "inverted: roll near pi"
    assert abs(2 * np.arccos(qs[3]) - 2 * PI / 3) < 1e-6 and np.abs(qs[:3]).min() > 0.4, "120 degrees about a skew axis"


def test_the_start_hook_changes_no_existing_case():
    """without `start`: the keys, ids, seeds and inputs of the learned matrix as before (its counts are asserted by its own tests)"""
    c = lm.spec("nnspeed", 16, 2)
    assert c["key"] == c["id"] == "nnspeed_a6_16x2_diag_K160_H5_m0" and c["seed"] == 20000 + 6000 + 35 + 100 + 160 % 97 and c["start"] is None
    x, U = lm.inputs(c)
    rng = np.random.default_rng(c["seed"])
    want = lm.X13.copy()
    want[:3] += rng.uniform(-0.5, 0.5, 3)
    want[7:] += rng.uniform(-0.1, 0.1, 6)
    np.testing.assert_array_equal(x, want.astype(F32))
    np.testing.assert_array_equal(U, (0.1 * rng.standard_normal((5, 6))).astype(F32))
    s = au.spec("nnspeed", 16, 5, "yaw+3.0")
    assert s["key"] == c["key"] + "_yaw+3.0" and s["seed"] == c["seed"]
    xs, Us = lm.inputs(s)
    np.testing.assert_array_equal(xs[3:7], au.quaternion("yaw+3.0"))
    np.testing.assert_array_equal(xs[10:], np.array(au.rates("yaw+3.0"), F32))
    np.testing.assert_array_equal(Us, U)
    ids = [c["id"] for inst in au.speed_instances() for c in au.speed_cases(*inst)] + [c["id"] for fam in au.NNAUV_FAMILIES for c in au.nnauv_cases(fam)]
    assert len(ids) == len(set(ids)) == 12 * 11 + (1 + 1 + 1 + 2) * 4


@pytest.mark.parametrize("kind", ["nnspeed", "nnauv"])
def test_every_learned_case_meets_the_conditions(kind):
    cases = [c for c in au.learned_cases().values() if c["kind"] == kind]
    assert len(cases) >= 16
    bad, worst = [], [0.0, 0.0, np.inf, 0.0]
    for c in cases:
        cond, wmax, move, rel = lm.conditions(c)
        worst = [max(worst[0], cond / (lm.u_bar(c) / lm.COND_FRACTION)), max(worst[1], wmax), min(worst[2], move), max(worst[3], rel)]
        if not (cond <= lm.u_bar(c) / lm.COND_FRACTION and wmax <= lm.W_MAX and move >= lm.TILE_MIN and rel <= lm.cost_cond_max(c)):
            bad.append("%s (seed %d, lambda %.4g): (a) %.3g (b) %.4f (c) %.3g (d) %.3g" % (c["key"], c["seed"], lm.lam_of(c), cond, wmax, move, rel))
    print("%s: %d oracle problems; worst (a) %.3g of the bound (b) %.4f (c) %.3g (d) %.3g" % ((kind, len(cases)) + tuple(worst)))
    assert not bad, "cases that break a condition (give them another seed or multiplier in attitude_util.ADJUST):\n" + "\n".join(bad)


def instance_cases():
    """NNAUVModelSpeed kernel instance -> its cases: the lone instances, and k_rollout_nn_batch's by the members of its batches"""
    out = {lm.fmt(lm.route(lm.cfg_of(cs[0]))[0]): cs for cs in (au.speed_cases(*inst) for inst in au.speed_instances())}
    for hid in (16, 32):
        for dense in (False, True):
            bs = au.speed_batches(hid, dense)
            out[lm.expected_name(lm.batch_cfg(bs[0]))] = [c for b in bs for c in b]
    return out


def test_speed_cases_keep_their_margins_and_cover_the_octants_and_the_folds():
    inst = instance_cases()
    assert len(inst) == 16 and sum(n.startswith("mppi::k_rollout_nn_batch<2") for n in inst) == 4
    seen_cut = set()
    for name, cases in sorted(inst.items()):
        counts, pitch, straddled = np.zeros((2, 8), int), [0, 0], {f: [] for f in au.FOLDS}
        for c in cases:
            e = au.euler(au.visited(c))
            worst = np.abs(e).reshape(-1, 3).max(axis=0)
            assert worst[0] <= PI - au.CUT_MARGIN and worst[2] <= PI - au.CUT_MARGIN, "%s: |roll|, |yaw| reach %.5f, %.5f" % (c["key"], worst[0], worst[2])
            assert worst[1] <= au.PITCH_MAX, "%s: |pitch| reaches %.4f" % (c["key"], worst[1])
            ev = e[:, :, :c["H"]]   # the states whose Euler angles the kernel takes
            for j, k in enumerate((2, 0)):
                counts[j] += np.bincount(au.octant(ev[..., k]).ravel(), minlength=8)
                if (np.abs(np.diff(ev[..., k], axis=2)) > PI).any():
                    seen_cut.add(("yaw", "roll")[j])
                for f, hits in au.straddles(ev[..., k]).items():
                    straddled[f] += [(c["start"][0], ("yaw", "roll")[j]) + h for h in hits]
            pitch = [pitch[0] + int((ev[..., 1] > 1.2).sum()), pitch[1] + int((ev[..., 1] < -1.2).sum())]
        print("%s: %d cases\n  octants of yaw  %s\n  octants of roll %s\n  pitch > 1.2: %d states, < -1.2: %d" % (name, len(cases), counts[0], counts[1], pitch[0], pitch[1]))
        for f in au.FOLDS:
            print("  fold %-9s straddled %d times (case, angle, control step, horizon step, tile, smaller side), e.g. %s" % (f, len(straddled[f]), straddled[f][:2]))
            assert straddled[f], "%s: no tile straddles the fold %s" % (name, f)
        assert counts.min() >= au.OCTANT_MIN, (name, counts)
        assert min(pitch) >= 1, (name, pitch)
    print("the +-pi cut is crossed between steps by: %s" % sorted(seen_cut))


def test_the_aimed_clouds_sit_on_their_folds():
    """what aim() promises, and that it is the matrix's own narrow cloud that straddles"""
    for hid, dense, member, fold in ((16, False, 0, "|y| = |x|"), (32, True, 1, "x = 0"), (16, True, 2, "y = 0")):
        c = au.aimed(hid, dense, member, fold)
        yaw = au.euler(au.visited(c))[0, :lm.TILE, au.AIM_T, 2]
        side = au.sides(yaw)[au.FOLDS.index(fold)]
        print("%s: yaw at horizon step %d in [%.5f, %.5f], %d | %d" % (c["key"], au.AIM_T, yaw.min(), yaw.max(), side.sum(), (~side).sum()))
        assert min(side.sum(), (~side).sum()) >= 30 and np.ptp(yaw) < 0.05 and abs(np.median(yaw) - au.AIMS[fold][1]) < 1e-4


def test_the_euler_rows_and_the_quaternion_rows_matter():
    speed = [c for c in au.learned_cases().values() if c["kind"] == "nnspeed"]
    nnauv = [c for c in au.learned_cases().values() if c["kind"] == "nnauv"]
    for cases, change, what in ((speed, au.without_euler_rows, "without the Euler rows"), (nnauv, au.with_qx_qy_swapped, "with the rows of q_x and q_y swapped")):
        shares = {c["key"]: au.moved(c, change) for c in cases}
        print("%s: the smallest share of costs moved by more than %.0e relative is %.2f (%s)" % (what, au.MOVED, min(shares.values()), min(shares, key=shares.get)))
        assert min(shares.values()) >= 0.25, sorted(shares.items(), key=lambda kv: kv[1])[:3]


def test_the_lock_case_takes_the_branch_robustly():
    for sign in (1, -1):
        x = au.lock_x0(sign)
        assert x.dtype == F32 and abs(np.linalg.norm(x[3:7].astype(np.float64)) - (1.0 + 1e-6)) < 2e-7
        for dy in (-1, 0, 1):
            for dw in (-1, 0, 1):
                q = x[3:7].copy()
                for i, d in ((1, dy), (3, dw)):
                    q[i] = q[i] if d == 0 else np.nextafter(q[i], F32(d * np.inf), dtype=F32)
                e = orc.euler_from_quaternion(q[None], dtype=F32)[0]
                assert e[1] == F32(sign * PI / 2) and e[2] == 0.0 and e[0] == 0.0, (sign, dy, dw, e)
        assert np.isnan(orc.euler_from_quaternion(x[None, 3:7], dtype=np.float64)[0][1]), "the fp64 oracle cannot judge this case"
        c, mk = au.lock_case("nnspeed_pc", 16, sign)
        u, Us, costs = orc.Problem(dtype=F32, **mk["problem"]).next_with_noise(mk["x"], mk["U"], lm.noise(c, 0))
        w = lm.softmin(costs.astype(np.float64), mk["lam"], False)
        print("lock %+d: x0 quaternion %s, lambda %.4g, fp32 costs %.4g .. %.4g, largest weight %.3f" % (sign, x[3:7], mk["lam"], costs.min(), costs.max(), w.max()))
        assert np.isfinite(costs).all() and np.isfinite(Us).all() and w.max() <= lm.W_MAX


def test_the_fossen_cases_are_fit_to_judge_a_kernel():
    """no sample's cost lies so near zero that the bar relative to it judges the case: the fp32 oracle's costs within FOSSEN_COND of the fp64
    oracle's, on the oracle's restatement of the noise"""
    from conftest import load_golden
    params, worst = dict(load_golden("model_auv")["params"]), {}
    every = [(i, diag, None, None) for diag in (True, False) for i in range(len(au.NAMES))]
    every += [(i, diag, rk, cost) for diag in (True, False) for rk, cost in au.fossen_batches() for i in range(len(au.NAMES))]
    for i, diag, rk, cost in every:
        case = au.fossen_case(params, i, diag, rk, cost)
        p32, p64 = orc.Problem(dtype=F32, **case["problem"]), orc.Problem(dtype=np.float64, **case["problem"])
        U = case["U"]
        for step in range(au.FOSSEN_STEPS):
            eps = orc.noise(case["seed"], step, 0, au.K_FOSSEN, au.H_FOSSEN, 6, case["handle"]["sigma"])
            c64, (_, U, c32) = p64.next_with_noise(case["x"], U, eps)[2], p32.next_with_noise(case["x"], U, eps)
            rel = float((np.abs(c32 - c64) / np.abs(c64)).max())
            worst[case["cost"]] = max(worst.get(case["cost"], 0.0), rel)
            assert np.isfinite(c64).all() and rel <= au.FOSSEN_COND, (case["name"], case["rk"], case["cost"], diag, step, rel)
    print("the fp32 oracle's Fossen costs from the fp64 oracle's, relative, at worst: %s" % {k: "%.3g" % v for k, v in worst.items()})


def test_the_fossen_cases_show_every_rk_and_cost_and_a_far_goal():
    pairs = [au.fossen_rk_cost(i) for i in range(len(au.NAMES))]
    assert {p[0] for p in pairs} == set(au.FOSSEN_RK) and {p[1] for p in pairs} == set(au.FOSSEN_COSTS) and len(set(pairs)) == 8
    assert {p[0] for p in au.fossen_batches()} == set(au.FOSSEN_RK) and {p[1] for p in au.fossen_batches()} == set(au.FOSSEN_COSTS)
    for name in au.NAMES:
        g = au.fossen_goal(name)
        dot = float(np.dot(g[3:7].astype(np.float64), au.quaternion(name).astype(np.float64)))
        assert abs(np.linalg.norm(g[3:7].astype(np.float64)) - 1.0) < 1e-6 and abs(dot + np.cos(0.45)) < 1e-6, (name, dot)
