"""The trajectory-validation cases of a wide learner batch (wide_rollout_util.py), proven real tests before they reach a GPU (no GPU
here): for every action width the fp32 restatement of the plain-order step stays finite and close to fp64, the members' trajectories
differ in bits, and a kernel of the wrong arithmetic — layer sums in descending j, or fused multiply-adds — would change bits of a single
step, so the GPU test's assert_array_equal tells them apart."""
import numpy as np
import pytest

import wide_rollout_util as U

N, T = 17, 7


@pytest.fixture(scope="module", params=U.A_DIMS, ids=lambda a: "a%d" % a)
def proven(request):
    """(case, x0, V, X32 [B, T+1, n, s], X64 [B, T+1, n, s])"""
    c = U.case(request.param)
    x0, V = U.inputs(c["a"], N, T)
    X32 = np.stack([U.rollout(c, net, x0, V) for net in c["nets"]])
    X64 = np.stack([U.rollout(c, net, x0, V, np.float64) for net in c["nets"]])
    return c, x0, V, X32, X64


def test_the_case_is_the_wide_network(proven):
    c = proven[0]
    assert c["dims"] == [3 * c["a"], 256, 256, 2 * c["a"]] and len(c["nets"]) == 3
    for net in c["nets"]:
        assert [w.shape for w in net["W"]] == [(3 * c["a"], 256), (256, 256), (256, 2 * c["a"])]
        assert not net["W"][1][:, 5].any() and net["b"][1][5] < 0  # the dead unit
    assert (np.asarray(c["norm"]["xstd"]) != 0).all()


def test_the_fp32_restatement_is_finite_and_follows_fp64(proven):
    c, x0, V, X32, X64 = proven
    assert X32.dtype == np.float32 and X32.shape == (3, T + 1, N, c["s"])
    assert np.isfinite(X32).all() and np.abs(X32).max() < 10.0
    assert np.abs(X32.astype(np.float64) - X64).max() < 1e-6


def test_members_differ_in_bits(proven):
    X32 = proven[3]
    for a in range(3):
        for b in range(a + 1, 3):
            assert not np.array_equal(X32[a, 1:], X32[b, 1:])
            assert (X32[a, 1] != X32[b, 1]).mean() > 0.9  # not one stray element: nearly every output of the first step


@pytest.mark.parametrize("how", ("descending", "fma"))
def test_a_wrong_kernel_shows_in_one_step(proven, how):
    c, x0, V, X32, X64 = proven
    flipped = 0
    for i, net in enumerate(c["nets"]):
        wrong = U.wrong_step(c, net, x0, V[0], how)
        assert wrong.dtype == np.float32 and wrong.shape == X32[i, 1].shape
        assert np.abs(wrong.astype(np.float64) - X64[i, 1]).max() < 1e-6  # a legitimate evaluation of the network, not a broken one
        flipped += int((wrong != X32[i, 1]).sum())
        assert (wrong != X32[i, 1]).any(), "member %d: %s order gives the bits of the plain order" % (i, how)
    assert flipped >= 3


def test_the_right_step_restates_itself(proven):
    """wrong_step's own loop in ascending order without the single rounding is learner_rollout_util.step: the two restatements agree"""
    c, x0, V, X32, X64 = proven
    np.testing.assert_array_equal(U.wrong_step(c, c["nets"][0], x0, V[0], "ascending"), X32[0, 1])
