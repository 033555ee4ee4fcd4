"""Needle tests: every sample position must reach the control update. Needs an MI355X: every test is marked `gpu`.

The rest of the suite pins sample COSTS bit for bit but the UPDATE only to U_TOL = 1e-5, and at ordinary temperature one sample moves U'
by sigma/K — below that bar from K = 65536 on, exactly where the combine structure changes (column waves, k_finish_cols, the 16:1 fold,
k_cost_minmax, shard and batch records). Here one chosen sample k* holds (nearly) all the weight (tests/needle_util.py), so U' depends on
that one position whatever K is: a record that is lost, mis-weighted or misplaced moves U' by O(sigma) = 1e4 x U_TOL.

For every case and every k* in it: the replayed step draws the first step's noise bit for bit; DBG_COSTS are the fp32 oracle's bits on
that noise (point mass: cost[k*] == 0 and beta == 0); the case is a needle for the fp64 oracle on that noise (w_ref[k*] >= 0.999, the
update without k* at least 100 x U_TOL away — proven beforehand on the CPU by tests/test_needle_oracle.py); u, DBG_U_UPDATED and the
stored sequence are within U_TOL of the fp64 oracle's; DBG_ETA within 1e-5 relative of the fp64 sum of exponentials; DBG_WEIGHTS[k*]
within 2e-4 relative; rollout_kernel_name() names the instance the case is meant to hit. The Fossen-AUV cases hold their costs to
StaticQuatCost's existing bar (3e-6 relative: device acosf against libm) and their update to U_TOL x sigma (sigma = 200, the convention of
tests/test_auv_gpu.py); they run colder than the rest (tests/needle_util.py says why), so eta and w[k*] there are nearly 1 by construction.

Out of scope: the learned-model kernels (k_rollout_mlp*, k_rollout_nnauv*, k_rollout_nnspeed*) — a learned model has no zero-cost rest
point to build a needle on; their coverage is the learned-model instance matrix (tests/test_learned_matrix_gpu.py, proven on the CPU by
tests/test_learned_matrix_oracle.py), which compares every sample's cost at an ordinary temperature.
"""
import numpy as np
import pytest

import needle_util as nu

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def report(name, seen):
    print("%s | min w_ref %.9f | min leave-one-out %.3g | max eta error %.3g" % (name, seen["w"], seen["loo"], seen["eta"]))


@pytest.mark.parametrize("case", nu.LONE + nu.AUV_LONE, ids=nu.ids(nu.LONE + nu.AUV_LONE))
def test_needle_reaches_the_update(m, case):
    """the lone handle: the one-launch step with seven and five producers, two launches, k_finish_cols up to 1024 tiles, the 16:1 fold,
    normalizeCost on two passes and past 2048 tiles, the dense-Sigma / dense-Q / a = 1, 2, 4 instances, the tile kernels (R = 64 forced,
    R = 32 and R = 16 through injected noise), the Fossen AUV on k_rollout_auv_pc and k_rollout_gen<0>"""
    h, seen = nu.run_lone(m, case)
    report(h.rollout_kernel_name(), seen)
    h.close()


@pytest.mark.parametrize("case", nu.SHARDED, ids=nu.ids(nu.SHARDED))
def test_needle_reaches_the_sharded_update(m, case):
    """shard_partial -> shard_finish in one process: the needle at 0, K - 1 and on both sides of every shard boundary; every shard's u is
    the others' bits and within U_TOL of the fp64 oracle's, every shard's costs are its slice of the fp32 oracle's; after the finish every
    shard holds the global beta (= 0) and eta (within ETA_RTOL of the fp64 sum over all K) and the whole U'; the shard that owns k* reports
    its weight"""
    import torch
    K, H, a, n = case["K"], case["H"], case["a"], case["shards"]
    full = nu.handle(m, dict(case, kernel=("mppi::k_step_pc<3, 7, 3, true", "") if K <= 8192 else case["kernel"]))
    hs = [nu.handle(m, case, shard_rank=g, shard_count=n) for g in range(n)]
    assert [h.k_offset for h in hs] == nu.shard_offsets(K, n) and sum(h.k_local for h in hs) == K
    p32, p64 = nu.problems(case)
    x = nu.goal_of(case)
    xd = torch.tensor(x, device="cuda")
    full.next(x)
    eps0 = full.debug_get(m.DBG_NOISE)
    rs = hs[0].record_size
    assert rs == 2 + H * a
    recs = torch.zeros(n * rs, device="cuda")
    us = [torch.zeros(a, device="cuda") for _ in range(n)]
    seen = {"w": 1.0, "loo": np.inf, "eta": 0.0}
    for k in case["ks"]:
        ref = nu.reference(case, p32, p64, x, eps0, k)
        nu.assert_is_needle(case, k, ref)
        for g, h in enumerate(hs):
            h.set_step_counter(0)
            h.set_action_sequence(ref["U"])
            h.shard_partial(xd.data_ptr(), recs[g * rs:(g + 1) * rs].data_ptr())
            h.synchronize()
        for g, h in enumerate(hs):
            h.shard_finish(recs.data_ptr(), n, us[g].data_ptr())
            h.synchronize()
        owner = max(g for g, h in enumerate(hs) if h.k_offset <= k)
        for g, h in enumerate(hs):
            tag = "%s k* = %d shard %d" % (case["id"], k, g)
            sl = slice(h.k_offset, h.k_offset + h.k_local)
            np.testing.assert_array_equal(h.debug_get(m.DBG_NOISE), eps0[sl], err_msg=tag)
            c = h.debug_get(m.DBG_COSTS)
            np.testing.assert_array_equal(c, ref["c32"][sl], err_msg=tag)
            beta, eta = float(h.debug_get(m.DBG_BETA)), float(h.debug_get(m.DBG_ETA))
            assert beta == 0.0, (tag, beta)
            eta_err = abs(eta - ref["eta"]) / ref["eta"]
            assert eta_err <= nu.ETA_RTOL, "%s: eta %.9g against %.9g: %.3g relative" % (tag, eta, ref["eta"], eta_err)
            np.testing.assert_allclose(h.debug_get(m.DBG_U_UPDATED), ref["Uupd"], rtol=0, atol=nu.U_TOL, err_msg=tag + " U'")
            if g == owner:
                assert c[k - h.k_offset] == 0.0, tag
                w = float(h.debug_get(m.DBG_WEIGHTS)[k - h.k_offset])
                assert abs(w - ref["w"]) <= nu.W_RTOL * ref["w"], "%s: weight %.9g against %.9g" % (tag, w, ref["w"])
            seen["w"], seen["loo"], seen["eta"] = min(seen["w"], ref["w"]), min(seen["loo"], ref["loo"]), max(seen["eta"], eta_err)
            u = us[g].cpu().numpy()
            np.testing.assert_array_equal(u, us[0].cpu().numpy(), err_msg=tag)
            np.testing.assert_allclose(u, ref["u"], rtol=0, atol=nu.U_TOL, err_msg=tag)
            np.testing.assert_allclose(h.get_action_sequence(), ref["Ushift"], rtol=0, atol=nu.U_TOL, err_msg=tag)
        print("%s k* = %d (shard %d): w_ref %.9f loo %.3g max|du| %.3g" % (case["id"], k, owner, ref["w"], ref["loo"], np.abs(us[0].cpu().numpy() - ref["u"]).max()))
    report(hs[0].rollout_kernel_name(), seen)
    for h in hs + [full]:
        h.close()


def batch_step(m, hb, cases, X, eps0, ks, p, seen):
    """one needle per member: the batch's step with U_i = -eps0[i][ks[i]], every member against its own fp64 reference"""
    hb.set_step_counter(0)
    hb.set_action_sequences(np.stack([-eps0[i][k] for i, k in enumerate(ks)]))
    u = hb.next(X)
    for i, (case, k) in enumerate(zip(cases, ks)):
        np.testing.assert_array_equal(hb.debug_get(i, m.DBG_NOISE), eps0[i], err_msg="%s: the replayed step drew other noise" % case["id"])
        nu.check(nu.Member(m, hb, i), case, k, nu.reference(case, p[i][0], p[i][1], X[i], eps0[i], k), u[i], seen)
    return u, hb.get_action_sequences()


def run_batch(m, cases, shared, per, moves):
    """moves: the members' needles, step after step; -> what each step gave"""
    n = len(cases)
    X = np.stack([nu.goal_of(c) for c in cases])
    hb = m.BatchHandle(n=n, k=cases[0]["K"], seeds=[c["seed"] for c in cases], goals=X, **shared, **per)
    nu.assert_kernel(hb, cases[0])
    p = [nu.problems(c) for c in cases]
    hb.next(X)
    eps0 = [hb.debug_get(i, m.DBG_NOISE) for i in range(n)]
    seen = {}
    out = [batch_step(m, hb, cases, X, eps0, ks, p, seen) for ks in moves]
    report(hb.rollout_kernel_name(), seen)
    hb.close()
    return out


def test_needle_reaches_every_member_of_a_batch(m):
    """B = 3 point-mass members with their own goal, seed, lambda and needle (first sample, last sample of the ragged last tile, first sample
    of that tile): each against its own fp64 reference; every member's result is the same bits when the others' needles move (three
    steps: each keeps one or two members' needles and moves the rest)"""
    cases = nu.BATCH
    moves = nu.BATCH_MOVES
    out = run_batch(m, cases, nu.config(cases[0]), dict(lams=nu.BATCH_LAMS), moves)
    kept = set()
    for s1 in range(len(moves)):
        for s2 in range(s1 + 1, len(moves)):
            for i in range(len(cases)):
                (u1, U1), (u2, U2) = out[s1], out[s2]
                if moves[s1][i] == moves[s2][i]:  # member i kept its needle while another member's moved
                    assert moves[s1] != moves[s2]
                    np.testing.assert_array_equal(u1[i], u2[i], err_msg="member %d, steps %d and %d" % (i, s1, s2))
                    np.testing.assert_array_equal(U1[i], U2[i], err_msg="member %d, steps %d and %d" % (i, s1, s2))
                    kept.add(i)
                else:
                    assert not np.array_equal(U1[i], U2[i])
    assert kept == {0, 1, 2}


@pytest.mark.parametrize("cases", nu.AUV_BATCHED, ids=["K%d" % c[0]["K"] for c in nu.AUV_BATCHED])
def test_needle_reaches_every_member_of_an_auv_batch(m, cases):
    """B = 2 Fossen-AUV members with their own goal pose, seed and needle; the two walk the needle positions in opposite order"""
    run_batch(m, cases, nu.config(cases[0]), dict(lam=cases[0]["lam"]), list(zip(cases[0]["ks"], cases[1]["ks"])))


def test_an_auv_batch_past_1024_tiles_per_member_is_refused(m):
    """why the batched AUV needle stops at K = 65536: one sample more is refused at creation, not served by another path"""
    case = nu.AUV_BATCHED[-1][0]
    with pytest.raises(m.MppiError, match="at most 1024 tiles"):
        m.BatchHandle(n=2, k=nu.AUV_BATCH_MAX_K + 1, lam=case["lam"], goals=np.stack([nu.goal_of(c) for c in nu.AUV_BATCHED[-1]]), **nu.config(case))


def armable(m, case):
    h = m.Handle(**dict(nu.config(case), k=128, seed=1, goal=nu.goal_of(case)))
    try:
        h.set_tuning("armed_us", 100)
        return True
    except m.MppiError:
        return False
    finally:
        h.close()


def test_needle_with_armed_launches(m):
    """armed launches (tests/test_step_gpu.py's convention: skipped without a large-BAR device). What this covers: the needle steps run on
    a handle that arms a launch behind every call, but set_action_sequence retires that launch, so no needle step is itself an armed
    launch (the protocol cannot make one: the armed launch's U is the previous step's U', not -eps[k*]); the step after the last needle
    consumes an armed launch and is held to the oracle as any step"""
    case = nu.MODES[0]
    if not armable(m, case):
        pytest.skip("no large-BAR device: MPPI_TUNE_ARMED_US is unsupported here")
    h, seen = nu.run_lone(m, case)
    report(h.rollout_kernel_name(), seen)
    p32, _ = nu.problems(case)
    x, U = nu.goal_of(case), h.get_action_sequence()
    u = h.next(x)  # (the launch armed behind the last needle step)
    u_ref, U_ref, c_ref = p32.next_with_noise(x, U, h.debug_get(m.DBG_NOISE))
    np.testing.assert_array_equal(h.debug_get(m.DBG_COSTS), c_ref)
    np.testing.assert_allclose(u, u_ref, rtol=0, atol=nu.U_TOL)
    np.testing.assert_allclose(h.get_action_sequence(), U_ref, rtol=0, atol=nu.U_TOL)
    h.close()


def test_needle_with_prelaunched_steps(m):
    """the pre-launched pipelined step (mppi_next_device on the handle's own stream, as tests/test_step_gpu.py drives it)"""
    import torch
    case = nu.MODES[1]
    a = case["a"]

    def step(h, x):
        xd, ud = torch.tensor(np.asarray(x, F32), device="cuda"), torch.zeros(a, device="cuda")
        torch.cuda.synchronize()
        h.next_device(xd.data_ptr(), ud.data_ptr(), None)
        h.synchronize()
        torch.cuda.synchronize()
        return ud.cpu().numpy()
    h, seen = nu.run_lone(m, case, step)
    report(h.rollout_kernel_name(), seen)
    h.close()


def test_prelaunch_is_refused_where_a_needle_case_cannot_take_it(m):
    """tests/test_step_gpu.py's refusal convention: normalizeCost is not the step's one pass"""
    case = nu.NORMALIZE[0]
    h = nu.handle(m, case)
    with pytest.raises(m.MppiError, match="the pre-launched step serves the point-mass producer/consumer path"):
        h.set_tuning("prelaunch", 1)
    h.close()
