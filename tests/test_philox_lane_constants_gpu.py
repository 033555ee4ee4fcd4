"""The producers' Philox lane constants (PhiloxLane, mppi_device.hip.h) where they can go wrong: the control steps around the one whose
Philox block indices straddle 2^32. Needs an MI355X: every test is marked `gpu`.

A producer lane computes round 0's M1 * sample and round 1's M0 * a0 once per launch; the second is only valid while the HIGH word of the
block index (step * NG + g) * a + q is the same for every block of the launch (NG = ceil(H / 4) horizon groups). With s* = floor(2^32 / (NG a)):
  step s* - 1   high word 0 everywhere                      the constants' path
  step s*       the word flips inside the launch            the rolled path, group by group
                (H = 64, a = 3: s* = 89478485, inside group 5 between q = 0 and q = 1; H = 60, a = 2: s* = 143165576, at group 8)
  step s* + 1   high word 1 everywhere                      the constants' path with a non-zero word
Each is compared with a handle on k_rollout_tile (tuning force_tile_kernel), whose noise comes from the general 64-bit block function that
knows no lane constants: sample costs and the exported noise bit for bit, and the noise against the CPU restatement of Philox within 5e-6.
"""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32

DENSE_SIGMA3 = np.array([[0.25, 0.05, 0.0], [0.05, 0.3, -0.04], [0.0, -0.04, 0.2]], F32)


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def s_star(H, a):
    return (1 << 32) // (((H + 3) // 4) * a)


def test_s_star_is_where_the_high_word_flips():
    """the issue's two steps, and where in the launch the word flips (no GPU needed, but it documents what the cases below rely on)"""
    assert s_star(64, 3) == 89478485 and s_star(60, 2) == 143165576
    for H, a, group, q in ((64, 3, 5, 1), (60, 2, 8, 0)):
        NG, s = (H + 3) // 4, s_star(H, a)
        blocks = [((s * NG + g) * a + qq, g, qq) for g in range(NG) for qq in range(a)]
        first_hi = next((g, qq) for b, g, qq in blocks if b >> 32)
        assert first_hi == (group, q)
        assert ((s - 1) * NG + NG) * a - 1 < 1 << 32 and ((s + 1) * NG * a) >> 32 == 1


def config(K, H, a, sigma=None, seed=1):
    s = 2 * a
    return dict(k=K, tau=H, s_dim=s, a_dim=a, dt=0.1, mass=1.0, lam=1.0, sigma=(0.25 * np.eye(a) if sigma is None else sigma),
                goal=[1, 0, .5, 0, .75, 0][:s], Q=np.ones(s), seed=seed)


def sequence(H, a):
    """a non-trivial nominal sequence: the action cost and u + eps see non-zero words in every column"""
    return (0.05 * np.sin(0.3 * np.arange(H * a))).astype(F32).reshape(H, a)


CASES = [
    # K, H, a, sigma, tuning of the handle under test, what its kernel's name must hold
    (192, 64, 3, None, None, "k_step_pc<3, "),                                   # the whole step in one launch
    (192, 64, 3, None, {"fused_step": 0}, "k_rollout_pc<3, 5, "),                # two launches, five producers
    (33000, 64, 3, None, None, "k_rollout_pc<3, 3, 6, true, 0, 0>"),             # three producers: the headline's instance
    (90, 64, 3, None, {"fused_step": 0}, "k_rollout_pc<3, "),                    # a partial tile
    (192, 64, 3, DENSE_SIGMA3, {"fused_step": 0}, "false, 0, 0>"),              # dense Sigma: the non-diagonal instance
    (192, 60, 2, None, {"fused_step": 0}, "k_rollout_pc<2, "),                   # a = 2: the word flips between two groups
]


@pytest.mark.parametrize("K,H,a,sigma,tuning,kernel", CASES)
def test_steps_around_the_high_word_flip_equal_the_tile_kernel(m, K, H, a, sigma, tuning, kernel):
    c = config(K, H, a, sigma)
    hp, ht = m.Handle(tuning=tuning, **c), m.Handle(tuning={"force_tile_kernel": 1}, **c)
    x = (0.1 * np.arange(2 * a)).astype(F32)
    U = sequence(H, a)
    st = s_star(H, a)
    for step in (st - 1, st, st + 1):
        for h in (hp, ht):
            h.set_step_counter(step)
            h.set_action_sequence(U)
        up, ut = hp.next(x), ht.next(x)
        assert kernel in hp.rollout_kernel_name() and "k_rollout_tile" in ht.rollout_kernel_name(), (hp.rollout_kernel_name(), ht.rollout_kernel_name())
        assert hp.get_step_counter() == step + 1
        cp, ep = hp.debug_get(m.DBG_COSTS), hp.debug_get(m.DBG_NOISE)
        assert np.isfinite(cp).all() and np.isfinite(ep).all()
        np.testing.assert_array_equal(cp, ht.debug_get(m.DBG_COSTS), err_msg="costs, step %d" % step)
        np.testing.assert_array_equal(ep, ht.debug_get(m.DBG_NOISE), err_msg="noise, step %d" % step)
        np.testing.assert_allclose(ep, orc.noise(1, step, 0, K, H, a, c["sigma"]), rtol=0, atol=5e-6, err_msg="noise against the oracle, step %d" % step)
        np.testing.assert_allclose(up, ut, rtol=0, atol=1e-6)
    hp.close()
    ht.close()


def test_fp_contract_instance_at_the_flip_is_finite_and_deterministic(m):
    """MPPI_FLAG_FP_CONTRACT runs the same producers with another consumer: two handles of it agree bit for bit at step 0 and at s*, and
    their costs are finite (its rounding is not the tile kernel's, so there is nothing else to compare it with)."""
    K, H, a = 33000, 64, 3
    c = config(K, H, a)
    h1, h2 = m.Handle(fp_contract=True, **c), m.Handle(fp_contract=True, **c)
    x = (0.1 * np.arange(2 * a)).astype(F32)
    for step in (0, s_star(H, a)):
        for h in (h1, h2):
            h.set_step_counter(step)
            h.set_action_sequence(sequence(H, a))
        u1, u2 = h1.next(x), h2.next(x)
        assert h1.rollout_kernel_name().endswith("3, 0>"), h1.rollout_kernel_name()
        c1 = h1.debug_get(m.DBG_COSTS)
        assert np.isfinite(c1).all() and np.isfinite(u1).all()
        np.testing.assert_array_equal(c1, h2.debug_get(m.DBG_COSTS))
        np.testing.assert_array_equal(u1, u2)
        np.testing.assert_array_equal(h1.get_action_sequence(), h2.get_action_sequence())
    h1.close()
    h2.close()


def test_batch_at_the_flip_equals_lone_handles(m):
    """k_rollout_pc_batch is the same text: B = 2 members at s* against their lone handles, bit for bit"""
    K, H, a, B = 192, 64, 3, 2
    c = config(K, H, a)
    del c["seed"], c["goal"]
    seeds = [5, 1234567890123]
    G = np.array([[1, 0, .5, 0, .75, 0], [-.5, 0, .25, 0, 1, 0]], F32)
    X = np.array([0.1 * np.arange(2 * a), -0.05 * np.arange(2 * a)], F32)
    U = np.stack([sequence(H, a), -sequence(H, a)])
    st = s_star(H, a)
    hb = m.BatchHandle(n=B, seeds=seeds, goals=G, **c)
    hb.set_action_sequences(U)
    hb.set_step_counter(st)
    ub = hb.next(X)
    assert "k_rollout_pc_batch<3, " in hb.rollout_kernel_name(), hb.rollout_kernel_name()
    Ub = hb.get_action_sequences()
    for i in range(B):
        h = m.Handle(seed=seeds[i], goal=G[i], **c)
        h.set_action_sequence(U[i])
        h.set_step_counter(st)
        u = h.next(X[i])
        np.testing.assert_array_equal(ub[i], u)
        np.testing.assert_array_equal(Ub[i], h.get_action_sequence())
        np.testing.assert_array_equal(hb.debug_get(i, m.DBG_COSTS), h.debug_get(m.DBG_COSTS))
        np.testing.assert_array_equal(hb.debug_get(i, m.DBG_NOISE), h.debug_get(m.DBG_NOISE))
        h.close()
    hb.close()
