"""The attitude matrix on the GPU: every 13-state rollout kernel away from the identity attitude (tests/attitude_util.py), against the CPU oracle.
Every other oracle test of a rollout kernel starts at the quaternion (0, 0, 0, 1), where atan2_pose never folds, three of NNAUVModel's four
quaternion inputs are ~0 and most cross terms of the Fossen model's rotation are multiplied by ~0. That every case here is fit to judge a
kernel, and reaches the octants, folds and lane divergence it claims, is proven on the CPU by tests/test_attitude_oracle.py. Needs an
MI355X: every test is marked `gpu`.

NNAUVModelSpeed: k_rollout_nnspeed_pc, k_rollout_nnspeed32 and k_rollout_gen<2, ..>, each at hidden 16 and 32 and with a diagonal and a dense
Sigma, from the eight start attitudes (K = 160, H = 5 and 9 in turn) and from the three starts aimed at the folds of atan2_pose: two fused
Philox steps and one on injected noise; k_rollout_nn_batch<2, ..> in batches of three members at three different attitudes. NNAUVModel:
k_rollout_nnauv_pc, _nnauv32, _nnauv32_bx3, k_rollout_gen<1, ..> and k_rollout_nn_batch<1, ..> from an inverted attitude and one 120 degrees
about a skew axis. The Fossen model: k_rollout_auv_pc<DIAG>, k_rollout_gen<0, 32, DIAG> from the eight attitudes with rk and the cost
cycled, k_rollout_auv_pc_batch<DIAG> with the eight attitudes as the members of a batch (K = 129, H = 5, one fused Philox step). The lock case:
an x0 of norm 1 + 1e-6 at pitch +-90 degrees takes the gimbal-lock branch of euler_from_quat at t = 0 (H = 1).

Bars, the suite's own: the learned cases learned_gpu_util's check_step (noise 5e-6; costs 2e-5 relative and 4 x max(fp32 oracle, 1e-6), 8 x
for split-bf16; u, U', sequence 1e-5, split-bf16 2e-5; weights sum to 1 within 1e-5), batch members also their lone handles bit for bit. The
Fossen model (tests/test_auv_gpu.py's): the quadratic cost's sample costs bit-identical to the fp32 oracle's, the quaternion / 3D-ellipse
costs' within 3e-6 relative; every cost within 4 x max(the fp32 oracle's own distance, 1e-6) of the fp64 oracle's; u, U' and the sequence
within max(1e-5, 4 x the fp32 oracle's distance) per unit sigma; batch members bit for bit their lone k_rollout_auv_pc. The lock case:
costs rtol 2e-6 to the fp32 oracle (the fp64 oracle gives NaN there), u, U' and the sequence within 1e-5 of the fp32 oracle's.
rollout_kernel_name() is asserted for every case.

Measured on an MI355X over the 36 kernel instances (largest distance per bar): noise 5.1e-7 (Fossen: 1.6e-6 per sigma); NNAUVModelSpeed costs
2.8e-7 relative, 0.07 x their bar relative to the fp32 oracle, u, U', sequence 1.3e-6; NNAUVModel costs 2.1e-7 (split-bf16 4.5e-7, 0.06 x),
u, U', sequence 4.1e-7 (4.0e-7); sum of the weights 1.2e-7; the lock case costs 2.4e-7 from the fp32 oracle's, u, U', sequence 4.5e-8;
the Fossen model: quadratic costs bit-identical, quat 1.7e-7, ellipse3d 2.4e-7 from the fp32 oracle's, 0.25 x the bars relative to the fp32
oracle's own distance; every bit-for-bit comparison of a batch member with its lone handle holds. No case exposed a kernel defect.
"""
import numpy as np
import pytest

import attitude_util as au
import learned_matrix_util as lm
from conftest import load_golden
from learned_gpu_util import NOISE_TOL, Lone, Matrix, Member, assert_same_bits, snapshot
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32
MX = Matrix()        # the learned cases: the names that ran, the largest distance per bar
FOSSEN_RAN = set()


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


@pytest.fixture(scope="module")
def params():
    return dict(load_golden("model_auv")["params"])


# ---- the learned models --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", au.SPEED_FAMILIES)
def test_nnauv_speed_kernels_from_every_attitude(m, fam):
    memo = {}
    for hid in (16, 32):
        for dense in (False, True):
            for c in au.speed_cases(fam, hid, dense):
                assert lm.route(lm.cfg_of(c))[0][0] == lm.kernel_family(fam)
                MX.run_lone(m, c, memo)


def test_nnauv_speed_batches_with_a_different_attitude_per_member(m):
    memo = {}
    for hid in (16, 32):
        for dense in (False, True):
            for members in au.speed_batches(hid, dense):
                assert len({c["start"][0] for c in members}) == lm.B
                MX.run_batch(m, members, memo)


@pytest.mark.parametrize("fam", au.NNAUV_FAMILIES)
def test_nnauv_kernels_from_attitudes_with_four_large_components(m, fam):
    memo = {}
    for c in au.nnauv_cases(fam):
        assert lm.route(lm.cfg_of(c))[0][0] == lm.kernel_family(fam)
        MX.run_lone(m, c, memo)


def test_nnauv_batches_with_a_different_attitude_per_member(m):
    memo = {}
    for members in au.nnauv_batches():
        MX.run_batch(m, members, memo)


@pytest.mark.parametrize("fam", au.SPEED_FAMILIES)
def test_the_gimbal_lock_branch_at_the_first_step(m, fam):
    """x0 at pitch +-90 degrees and norm 1 + 1e-6: euler_from_quat's lock branch answers at t = 0; against the fp32 oracle"""
    for hid, sign in ((16, 1), (32, -1), (16, -1), (32, 1)):
        c, mk = au.lock_case(fam, hid, sign)
        h = m.Handle(**mk["handle"])
        name = h.rollout_kernel_name()
        assert name == lm.expected_name(lm.cfg_of(c)), (c["id"], name)
        h.set_action_sequence(mk["U"])
        u = h.next(mk["x"])
        snap = snapshot(m, Lone(h), u)
        eps = MX.drawn_noise(m, Lone(h), c, 0, c["id"])
        u32, Us32, c32 = orc.Problem(dtype=F32, **mk["problem"]).next_with_noise(mk["x"], mk["U"], eps)
        assert np.isfinite(c32).all() and np.isfinite(snap["costs"]).all(), c["id"]
        rel = float((np.abs(snap["costs"].astype(np.float64) - c32) / np.abs(c32)).max())
        d = max(np.abs(snap["u"] - u32).max(), np.abs(snap["Uupd"] - lm.updated(u32, Us32)).max(), np.abs(snap["seq"] - Us32).max())
        print("%s: costs %.3g relative from the fp32 oracle's; u, U', sequence %.3g" % (c["id"], rel, d))
        MX.see("lock: costs against the fp32 oracle (rtol 2e-6)", rel)
        MX.see("lock: u, U', sequence against the fp32 oracle (1e-5)", d)
        np.testing.assert_allclose(snap["costs"], c32, rtol=2e-6, err_msg=c["id"])
        assert d <= 1e-5, (c["id"], d)
        h.close()
        MX.ran.add(name)


# ---- the Fossen model ----------------------------------------------------------------------------------------------------------------------
def run_fossen(m, case, kernel, diag, memo):
    """one Fossen case on a lone handle (kernel: "pc", the default pipeline, or "gen", tuning gen_one_wave): the fused Philox step
    (au.FOSSEN_STEPS of them) against the oracle on the noise the step drew; -> the steps' snapshots"""
    key = (case["name"], case["rk"], case["cost"], kernel, diag)
    if key in memo:
        return memo[key]
    h = m.Handle(tuning={"gen_one_wave": 1} if kernel == "gen" else None, **case["handle"])
    name = h.rollout_kernel_name()
    assert name == au.FOSSEN_KERNELS[(kernel, diag)], (key, name)
    p32, p64 = orc.Problem(dtype=F32, **case["problem"]), orc.Problem(dtype=np.float64, **case["problem"])
    h.set_action_sequence(case["U"])
    x, U_in, scale, snaps = case["x"], case["U"], au.SIGMA_SCALE, []
    for step in range(au.FOSSEN_STEPS):
        tag = "%s rk %d %s on %s step %d" % (case["name"], case["rk"], case["cost"], name, step)
        snap = snapshot(m, Lone(h), h.next(x))
        eps = h.debug_get(m.DBG_NOISE)
        dn = np.abs(eps - orc.noise(case["seed"], step, 0, au.K_FOSSEN, au.H_FOSSEN, 6, case["handle"]["sigma"])).max() / scale
        u64, Us64, c64 = p64.next_with_noise(x, U_in, eps)
        u32, Us32, c32 = p32.next_with_noise(x, U_in, eps)
        got = snap["costs"].astype(np.float64)
        rel, rel32 = float((np.abs(got - c64) / np.abs(c64)).max()), float((np.abs(c32 - c64) / np.abs(c64)).max())
        to32 = float((np.abs(got - c32) / np.abs(c32)).max())
        dist = lambda u, Us: max(np.abs(u - u64).max(), np.abs(lm.updated(u, Us) - lm.updated(u64, Us64)).max(), np.abs(Us - Us64).max()) / scale
        eu = max(dist(snap["u"], snap["seq"]), np.abs(snap["Uupd"] - lm.updated(u64, Us64)).max() / scale)
        eu_cpu = dist(np.asarray(u32, np.float64), np.asarray(Us32, np.float64))
        w = h.debug_get(m.DBG_WEIGHTS).astype(np.float64)
        print("%s: noise %.3g per sigma; costs %.3g relative from the fp32 oracle's, %.3g from the fp64 oracle's (fp32 oracle %.3g); u, U', sequence "
              "%.3g per sigma (fp32 oracle %.3g); largest weight %.3f" % (tag, dn, to32, rel, rel32, eu, eu_cpu, w.max()))
        MX.see("fossen: noise per sigma (5e-6)", dn)
        MX.see("fossen: %s costs from the fp32 oracle's (%s)" % (case["cost"], "bit-identical" if case["cost"] == "quadratic" else "rtol 3e-6"), to32)
        MX.see("fossen: costs / (4 x max(fp32 oracle, 1e-6))", rel / (4 * max(rel32, 1e-6)))
        MX.see("fossen: u, U', sequence / max(1e-5, 4 x fp32 oracle) per sigma", eu / max(1e-5, 4 * eu_cpu))
        assert dn <= NOISE_TOL, tag
        assert np.isfinite(snap["costs"]).all(), tag
        if case["cost"] == "quadratic":
            np.testing.assert_array_equal(snap["costs"], c32, err_msg=tag)
        else:
            np.testing.assert_allclose(snap["costs"], c32, rtol=3e-6, err_msg=tag)
        assert rel <= 4 * max(rel32, 1e-6), "%s: costs %.3g relative, the fp32 oracle's %.3g" % (tag, rel, rel32)
        assert eu <= max(1e-5, 4 * eu_cpu), "%s: u, U', sequence %.3g per sigma, the fp32 oracle's %.3g" % (tag, eu, eu_cpu)
        assert abs(w.sum() - 1.0) < 1e-5, (tag, w.sum())
        np.testing.assert_array_equal(snap["u"], snap["Uupd"][0], err_msg=tag + ": u is U'[0]")
        snaps.append(snap)
        U_in = snap["seq"]
    h.close()
    FOSSEN_RAN.add(name)
    memo[key] = snaps
    return snaps


@pytest.mark.parametrize("kernel", ["pc", "gen"])
def test_fossen_kernels_from_every_attitude(m, params, kernel):
    memo = {}
    for diag in (True, False):
        seen = set()
        for i in range(len(au.NAMES)):
            case = au.fossen_case(params, i, diag)
            run_fossen(m, case, kernel, diag, memo)
            seen.add((case["rk"], case["cost"]))
        assert {s[0] for s in seen} == set(au.FOSSEN_RK) and {s[1] for s in seen} == set(au.FOSSEN_COSTS)


def test_fossen_batches_whose_members_are_the_attitudes(m, params):
    """k_rollout_auv_pc_batch<DIAG>: the eight start attitudes as the members of one batch, a batch per (rk, cost) pair; every member is
    its lone k_rollout_auv_pc handle bit for bit (which run_fossen holds to the oracle)"""
    memo = {}
    for diag in (True, False):
        for rk, cost in au.fossen_batches():
            cases = [au.fossen_case(params, i, diag, rk, cost) for i in range(len(au.NAMES))]
            shared = {k: v for k, v in cases[0]["handle"].items() if k not in ("seed", "goal")}
            hb = m.BatchHandle(n=len(cases), seeds=[c["seed"] for c in cases], goals=np.stack([c["goal"] for c in cases]), **shared)
            name = hb.rollout_kernel_name()
            assert name == au.FOSSEN_KERNELS[("batch", diag)], name
            hb.set_action_sequences(np.stack([c["U"] for c in cases]))
            lone = [run_fossen(m, c, "pc", diag, memo) for c in cases]
            for step in range(au.FOSSEN_STEPS):
                u = hb.next(np.stack([c["x"] for c in cases]))
                for i, c in enumerate(cases):
                    assert_same_bits(snapshot(m, Member(hb, i), u[i]), lone[i][step], "%s: member %d (%s) rk %d %s step %d against its lone handle" % (name, i, c["name"], rk, cost, step))
            hb.close()
            FOSSEN_RAN.add(name)


def test_the_names_that_ran():
    print("\n".join(sorted(MX.ran | FOSSEN_RAN)))
    print("%d kernel instances ran; largest distances observed:" % len(MX.ran | FOSSEN_RAN))
    for bar in sorted(MX.seen):
        print("  %-75s %.3g" % (bar, MX.seen[bar]))
    if len(FOSSEN_RAN) == len(au.FOSSEN_KERNELS):  # (a run of part of this file has launched part of the set)
        assert FOSSEN_RAN == set(au.FOSSEN_KERNELS.values())
    speed = {lm.fmt(lm.route(lm.cfg_of(c), call)[0]) for inst in au.speed_instances() for c in au.speed_cases(*inst)[:1] for call in ("next", "noise")}
    nnauv = {lm.fmt(lm.route(lm.cfg_of(c), call)[0]) for fam in au.NNAUV_FAMILIES for c in au.nnauv_cases(fam) for call in ("next", "noise")}
    batch = {"mppi::k_rollout_nn_batch<%d, %d, %s>" % (k, hid, d) for k in (1, 2) for hid in (16, 32) for d in ("true", "false")}
    assert len(speed) == 12 and len(nnauv) == 10 and MX.ran <= speed | nnauv | batch, sorted(MX.ran - speed - nnauv - batch)
    if len(MX.ran) >= len(speed | nnauv | batch):
        assert MX.ran == speed | nnauv | batch
