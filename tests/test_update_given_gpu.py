"""The soft-min update on given costs (mppi_update, Handle.update) and the finish kernels behind it, on designed inputs
(tests/update_given_util.py; every case is proven on the CPU first by tests/test_update_given_oracle.py). Needs an MI355X: every test is
marked `gpu`.

B. update() on a default handle (k_finish_cols_cm) and on its MPPI_TUNE_FINISH_GENERIC twin (k_finish_cols) at every record count
   128 .. 1024, full and ragged, one fold, 160 columns and the 13-state a = 6 handle: the two bit for bit, and against the fp64 oracle
   beta exact, nabla within ETA_RTOL, Unew and U + wn within U_TOL, arg / exp / w within the bars update_given_util derives; with narrow
   limits Unew is exactly its own dimension's lo or hi; the handle's sequence and step counter stay as they were.
C. update() between control steps leaves nothing behind: twin handles, one of which calls it, step bit for bit alike on every route.
D. The batched fast path (k_finish_cols_batch<A, true>) against the batched generic kernel (<A, false>) with per-member temperatures,
   and member 1 against its lone handle.

MEASURED (B, the worst over its 257 cases on the first run on an MI355X against the fp64 oracle; beside it the fp32 CPU oracle against the
same reference, from tests/test_update_given_oracle.py):
                                      GPU        fp32 oracle   bar
  Unew, absolute (H = 4 shapes)       1.22e-7    1.22e-7       U_TOL = 1e-5
  Unew, absolute (H = 40, |U| <= 20)  9.46e-7    9.46e-7       U_TOL (half an ulp of 16 .. 32 is 9.5e-7)
  U + wn, absolute                    6.19e-8    -             U_TOL
  nabla, relative                     9.07e-8    5.62e-8       ETA_RTOL = 1e-5
  arg, relative                       1.18e-7    1.18e-7       0.661 of arg_bar (3 roundings: 1.79e-7 |arg|) on both
  exp, relative                       5.26e-6    5.24e-6       0.57 of exp_rbar on both (stairs, |arg| near 61)
  Unew - (U + wn)                     0.968 of unew_bar (2^-24 (4 |wn| + |Unew|)): the rounding of the sum alone reaches half an ulp
beta equal, and every quantity bit for bit between the two finish paths, in all cases. No case exposed a kernel defect.
Run time on the MI355X: the 47 tests of this file 10 s together with start-up; the slowest test function 0.3 s.

Tried on scratch builds, never committed; each fails the test named:
  the fourth slot block's mask of column_combine_cm `<= nb`   B [j6_full_a2], [j7_full_a3] (nbp = 768, 896: the last slot counted twice)
  C[0] for C[m] in the batched fast path                       D [a3_nbp384], [a3_nbp640], [a3_nbp1024] (one record has no temperature: 128 passes)
  the limits indexed c / a                                     test_update_clamps_to_its_own_dimensions_limits [j8_full_a4], [auv_H3_a6_j3_ragged]
  mppi_update without ensure_record_layout                     C [mlp_2x256_tiles_of_32]
"""
import numpy as np
import pytest

import needle_util as nu
import update_given_util as ug
import update_tail_util as ut

pytestmark = pytest.mark.gpu
F32 = np.float32
SEEN = {}


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def twins(m, sh, lam):
    return ug.handle(m, sh, lam), ug.handle(m, sh, lam, finish_generic=1)


# =============================================================== B: update() against fp64, on both finish paths
@pytest.mark.parametrize("sh", ug.SHAPES, ids=ug.SHAPE_IDS)
def test_update_on_given_costs_against_fp64_on_both_finish_paths(m, sh):
    cs = ug.cases(sh)
    for lam in sorted({c[1] for c in cs}):
        hf, hg = twins(m, sh, lam)
        bf, bg = ug.held(hf), ug.held(hg)
        assert bf[0] == bg[0] == 1 and np.array_equal(bf[1], bg[1]) and np.abs(bf[1]).max() > 0
        for case in [c for c in cs if c[1] == lam]:
            inp = ug.inputs(sh, case)
            rf, rg = hf.update(*inp[:3]), hg.update(*inp[:3])
            tag = "%s %s" % (sh["id"], ug.case_id(case))
            ug.assert_held(hf, bf, tag + " (fast path)")
            ug.assert_held(hg, bg, tag + " (generic)")
            ug.check_update(sh, case, rf, rg, inp, ug.reference(*inp), SEEN)
        hf.close(); hg.close()
    print("worst so far over %d cases: %s" % (SEEN["n"], ", ".join("%s %.3g" % kv for kv in sorted(SEEN.items()) if kv[0] != "n")))


LIMIT_SHAPES = [s for s in ug.SHAPES if s["id"] in ("j5_ragged_a3", "j8_full_a4", ug.AUV["id"])]


@pytest.mark.parametrize("sh", LIMIT_SHAPES, ids=[s["id"] for s in LIMIT_SHAPES])
def test_update_clamps_to_its_own_dimensions_limits(m, sh):
    """narrow bands: every element of Unew is exactly lo or hi of ITS action dimension, wn and beta keep the bits they had without limits;
    limits wider than the update: Unew keeps its unclipped bits. On both finish paths."""
    assert sh["a"] in (3, 4, 6)
    lo, hi = ug.limits(sh["a"])
    for h in twins(m, sh, 1.0):
        before = ug.held(h)
        for case in [("spread", 1.0, None), ("needle", 1.0, ug.needles(sh)[-1][0])]:
            tag = "%s %s" % (sh["id"], ug.case_id(case))
            inp = ug.inputs(sh, case)
            raw = ug.reference(*inp)["Unew"]
            off = np.minimum(np.abs(raw - lo), np.abs(raw - hi)).min()
            assert off >= 100 * nu.U_TOL and not ((raw > lo) & (raw < hi)).any(), "%s: an element of U' is only %.3g from its band" % (tag, off)
            free = h.update(*inp[:3])
            h.set_action_limits(lo, hi)
            clamped = h.update(*inp[:3])
            h.set_action_limits(np.full(sh["a"], -100.0), np.full(sh["a"], 100.0))
            wide = h.update(*inp[:3])
            h.set_action_limits(None, None)
            again = h.update(*inp[:3])
            np.testing.assert_array_equal(clamped["Unew"], np.where(raw > hi, hi, lo), err_msg=tag + ": Unew is not its own dimension's lo / hi")
            for key in ("beta", "nabla", "wn", "arg", "exp", "w"):
                np.testing.assert_array_equal(clamped[key], free[key], err_msg="%s: %s changed with the limits" % (tag, key))
            for other, what in ((wide, "wide limits"), (again, "limits off again")):
                for key in ug.KEYS_BITS:
                    np.testing.assert_array_equal(other[key], free[key], err_msg="%s: %s with %s" % (tag, key, what))
            ug.assert_held(h, before, tag)
        h.close()


# =============================================================== C: update() leaves nothing behind
def pm_leak(K, a=3, Hs=4, **kw):
    goal = (nu.GOAL3 + [0.25, 0])[:2 * a]
    x = (np.asarray(goal) + np.asarray(ut.PM_OFF[:2 * a])).astype(F32)
    return dict(dict(k=K, tau=Hs, s_dim=2 * a, a_dim=a, dt=0.1, mass=1.0, lam=1.0, sigma=0.25 * np.eye(a), goal=goal, seed=5), **kw), x


def auv_leak(K):
    c = ug.auv_case(K, 3)
    return dict(nu.config(c), k=K, seed=5, goal=nu.goal_of(c), lam=30.0), ug.AUV_POSE


LEAK_ROUTES = {
    "one_launch_64_tiles": (lambda: pm_leak(64 * 64), "mppi::k_step_pc<3, "),
    "two_launches_257_tiles": (lambda: pm_leak(64 * 257 - 63, tuning={"fused_step": 0}), "mppi::k_rollout_pc<3, "),
    "fold_1025_tiles": (lambda: pm_leak(64 * 1025), "mppi::k_rollout_pc<3, "),
    "normalize_257_tiles": (lambda: pm_leak(64 * 257 - 63, normalize_cost=True, lam=0.1), "mppi::k_rollout_pc<3, "),
    "mlp_2x256": (lambda: pm_leak(130, mlp=ut.mlp_weights(6, 3, 256, 2, 43), sigma=0.5 * np.eye(3)), "mppi::k_rollout_mlp2<3, "),
    # H * a = 768: the tile kernel update() runs cuts K into tiles of 32 rollouts, the learned-model kernel into 64: the record slots change
    # hands with every call (ensure_record_layout), and a slot left over from update() would weigh in the next step
    "mlp_2x256_tiles_of_32": (lambda: pm_leak(130, Hs=256, mlp=ut.mlp_weights(6, 3, 256, 2, 43), sigma=0.5 * np.eye(3)), "mppi::k_rollout_mlp2<3, "),
    "auv_a6": (lambda: auv_leak(64 * 257 - 63), "mppi::k_rollout_"),
}


@pytest.mark.parametrize("route", LEAK_ROUTES, ids=list(LEAK_ROUTES))
def test_update_between_steps_leaves_nothing_behind(m, route):
    """four control steps on twin handles with the same seed; one of them calls update() with a spread case after steps 1 and 3. u, the
    sequence, the step counter, beta and eta are the same bits after every step, and so is the noise of the step after an update"""
    make, kernel = LEAK_ROUTES[route]
    cfg, x = make()
    ha, hb = m.Handle(**cfg), m.Handle(**cfg)
    assert ha.rollout_kernel_name().startswith(kernel), ha.rollout_kernel_name()
    K, Hs, a = cfg["k"], cfg["tau"], cfg["a_dim"]
    sh = ug.shape(route, K, a, Hs=Hs)
    inp = ug.inputs(sh, ("spread", 1.0, None))
    x = x.copy()
    for step in range(4):
        ua, ub = ha.next(x), hb.next(x)
        tag = "%s step %d" % (route, step)
        np.testing.assert_array_equal(ua, ub, err_msg=tag + " u")
        assert np.isfinite(ua).all()
        np.testing.assert_array_equal(ha.get_action_sequence(), hb.get_action_sequence(), err_msg=tag + " sequence")
        assert ha.get_step_counter() == hb.get_step_counter() == step + 1, tag
        for what in (m.DBG_BETA, m.DBG_ETA, m.DBG_U_UPDATED):
            np.testing.assert_array_equal(ha.debug_get(what), hb.debug_get(what), err_msg="%s debug item %d" % (tag, what))
        if step in (1, 3):  # the step after an update
            np.testing.assert_array_equal(ha.debug_get(m.DBG_NOISE), hb.debug_get(m.DBG_NOISE), err_msg=tag + " noise")
        if step in (0, 2):
            before = ug.held(ha)
            r = ha.update(*inp[:3])
            assert r["beta"] == inp[0].min() and np.isfinite(r["Unew"]).all()
            ug.assert_held(ha, before, tag)
        if cfg.get("mlp") is None and a <= 4:
            x[1::2] = ua * F32(0.1)  # (another state every step)
    assert np.abs(ha.get_action_sequence()).max() > 0
    ha.close(); hb.close()


# =============================================================== D: the batched fast path against the batched generic kernel
B, STEPS = 3, 3
BATCH_K = {128: 64, 384: 64 * 257, 640: 64 * 513, 1024: 65536}
AUV_GOAL3 = [-0.25, 0.5, 0.25, 0.0, 0.0, 0.0, 1.0] + [0.0] * 6


def batch_cfg(a, K):
    """-> (keywords shared by the members, per-member goals [B, s], start states [B, s], the lone kernel's name)"""
    if a == 6:
        c = ug.auv_case(K, 3)
        goals = np.array(nu.AUV_GOALS + [AUV_GOAL3], F32)
        X = goals.copy()
        X[:, :3] += [0.5, -0.4, 0.3]
        return dict(nu.config(c), k=K), goals, X, "mppi::k_rollout_"
    goals = np.zeros((B, 2 * a), F32)
    goals[:, 0::2] = np.array([g[0::2] + [0.25] for g in nu.BATCH_GOALS], F32)[:, :a]
    X = goals + np.asarray(ut.PM_OFF[:2 * a], F32)
    return dict(k=K, tau=4, s_dim=2 * a, a_dim=a, dt=0.1, mass=1.0, sigma=0.25 * np.eye(a)), goals, X, "mppi::k_rollout_pc<%d, " % a


def batch_state(m, hb):
    return dict(U=hb.get_action_sequences(), step=hb.get_step_counter(),
                beta=np.array([hb.debug_get(i, m.DBG_BETA) for i in range(B)]), eta=np.array([hb.debug_get(i, m.DBG_ETA) for i in range(B)]))


BATCHES = [(a, nbp) for a in (1, 2, 3, 4) for nbp in sorted(BATCH_K)] + [(6, 128), (6, 384)]  # the instances A = 1..4 and the 13-state A = 6


@pytest.mark.parametrize("a, nbp", BATCHES, ids=["a%d_nbp%d" % b for b in BATCHES])
def test_batched_fast_path_has_the_bits_of_the_batched_generic_kernel(m, a, nbp):
    """B = 3 members with their own lambda, seed and goal, three steps, with and without the narrow limits: every member's u, the sequences,
    the shared step counter and every member's (beta, eta); at nbp = 384 member 1 is also its lone handle on the lone fast path"""
    K = 129 if (a, nbp) == (6, 128) else 64 * 257 - 63 if a == 6 else BATCH_K[nbp]
    assert ut.record_pad((K + 63) // 64) == nbp
    shared, goals, X0, kernel = batch_cfg(a, K)
    per = dict(lams=nu.BATCH_LAMS, seeds=nu.BATCH_SEEDS, goals=goals)
    for clip in (False, True):
        hf, hg = m.BatchHandle(n=B, **shared, **per), m.BatchHandle(n=B, tuning={"finish_generic": 1}, **shared, **per)
        lone = None
        if nbp == 384:
            lone = m.Handle(**shared, lam=nu.BATCH_LAMS[1], seed=nu.BATCH_SEEDS[1], goal=goals[1], tuning={"fused_step": 0})
            assert lone.rollout_kernel_name().startswith(kernel), lone.rollout_kernel_name()
        for h in (hf, hg, lone):
            if clip and h is not None:
                h.set_action_limits(*ug.limits(a))
        X = X0.copy()
        for s in range(STEPS):
            tag = "a = %d nbp = %d %s step %d" % (a, nbp, "limits" if clip else "free", s)
            uf, ugen = hf.next(X), hg.next(X)
            np.testing.assert_array_equal(uf, ugen, err_msg=tag + " u")
            sf, sg = batch_state(m, hf), batch_state(m, hg)
            for key in sg:
                np.testing.assert_array_equal(sf[key], sg[key], err_msg="%s %s" % (tag, key))
            assert sf["step"] == s + 1, tag
            assert np.isfinite(uf).all() and np.isfinite(sf["eta"]).all(), (tag, sf["eta"])
            assert a == 6 or len(set(sf["eta"])) == B, (tag, sf["eta"])  # (the point-mass members are no copies of each other)
            if lone is not None:
                ul = lone.next(X[1])
                np.testing.assert_array_equal(uf[1], ul, err_msg=tag + " member 1 against its lone handle: u")
                np.testing.assert_array_equal(sf["U"][1], lone.get_action_sequence(), err_msg=tag + " member 1 against its lone handle: sequence")
                assert sf["beta"][1] == lone.debug_get(m.DBG_BETA) and sf["eta"][1] == lone.debug_get(m.DBG_ETA), tag
            if a <= 4:
                X[:, 1::2] = uf * F32(0.1)  # (another state every step)
        if clip:  # (the stored sequence is the shift of U': its last row is zero, the others lie in their dimension's band)
            lo, hi = ug.limits(a)
            U = hf.get_action_sequences()
            assert (U[:, :-1] >= lo).all() and (U[:, :-1] <= hi).all(), U
        for h in (hf, hg, lone):
            if h is not None:
                h.close()
