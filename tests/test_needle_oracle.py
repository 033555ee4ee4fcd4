"""Every case of the needle matrix (tests/needle_util.py, run on the GPU by tests/test_needle_gpu.py) IS a needle: proven here on the CPU,
before a GPU sees it, on the oracle's restatement of the noise the step will draw (orc.noise; an injected-noise case's own noise) with the
fp64 oracle: (a) the needle's reference weight is at least 0.999, (b) the fp64 update without the needle is at least 100 x U_TOL away from
the full one — so a kernel that loses that one position cannot pass the GPU test's U_TOL —, (c) the fp32 oracle's own update is
within U_TOL / 4 of the fp64 oracle's, so that the bar tests the kernel and not the conditioning of the case. Each case's lambda and Q scale were chosen here.
"""
import numpy as np
import pytest

import needle_util as nu

MINIMA = {}


@pytest.mark.parametrize("case", nu.EVERY_CASE, ids=nu.ids(nu.EVERY_CASE))
def test_case_is_a_needle(case):
    p32, p64 = nu.problems(case)
    eps, x = nu.oracle_noise(case), nu.goal_of(case)
    assert len(case["ks"]) > 0 and all(0 <= k < case["K"] for k in case["ks"])
    for k in case["ks"]:
        ref = nu.reference(case, p32, p64, x, eps, k)
        print("%s k* = %d: w_ref %.9f, leave-one-out distance %.3g, fp32 oracle off by %.3g" % (case["id"], k, ref["w"], ref["loo"], ref["cond"]))
        nu.assert_is_needle(case, k, ref)
        # the needle itself: zero action, so the point mass stays on the goal at no cost; U' ~ 0
        if case["model"] == "pm" and not case["cpp_form"]:
            assert ref["c32"][k] == 0.0 and ref["c64"][k] == 0.0 and ref["c32"].min() == 0.0
        assert np.abs(ref["Uupd"]).max() / case["scale"] < 10 * (1 - nu.W_MIN)
        MINIMA["w"], MINIMA["loo"] = min(MINIMA.get("w", 1.0), ref["w"]), min(MINIMA.get("loo", np.inf), ref["loo"])
    print("minima so far: w_ref %.9f, leave-one-out %.3g" % (MINIMA["w"], MINIMA["loo"]))


def test_matrix_reaches_every_structure():
    """the matrix holds what it is meant to: ids are unique, the largest case is K = 131073 x H = 4, every fold / shard / tile edge is there"""
    every = nu.EVERY_CASE
    assert len(set(nu.ids(every))) == len(every)
    assert max(c["K"] * c["H"] for c in every) == 131073 * 4
    assert {c["K"] for c in nu.FINISH} == {8193, 32768, 32769, 65536} and {c["K"] for c in nu.FOLD} == {65537, 131073}
    assert set(nu.FOLD_KS) == set(range(0, 512, 64)) | {1023, 1024, 65535, 65536}
    for c in nu.SHARDED:
        offs = nu.shard_offsets(c["K"], c["shards"])
        assert {0, c["K"] - 1} | set(offs) | {o - 1 for o in offs[1:]} == set(c["ks"])
