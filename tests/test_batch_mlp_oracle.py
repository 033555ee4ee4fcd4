"""The cases on which the batched learned point-mass controllers are held to the oracle directly (batch_mlp_util.ORACLE: one wide and one
narrow member set at K = 129, H = 9), judged on the CPU with the oracle alone, before any kernel runs on them. For every member:
  * the case is well conditioned: every fp64 cost is finite, and a correct fp32 evaluation of the same update (the oracle in fp32) sits
    well inside the bars the GPU is held to - costs within a quarter of 2e-5 of fp64 relatively, U' within a quarter of 1e-5;
  * the case is a needle for the one mistake a batch can make - member m reading a neighbour's network: U' of member m computed with
    member j's network differs from its own by at least 100 x the U' bar, and its costs by at least 100 x the cost bar, for every j != m.
The noise is each member's own Philox noise of step 0."""
import numpy as np
import pytest

import batch_mlp_util as N

NEEDLE = 100.0
CIS = N.ids_of(N.ORACLE)


@pytest.mark.parametrize("ci", CIS, ids=[N.IDS[i] for i in CIS])
def test_case_is_well_conditioned_and_a_needle_for_a_swapped_network(ci):
    case, mem = N.CASES[ci], N.members(ci)
    for m in N.checked(case):
        eps = N.first_noise(case, mem, m)
        own = N.oracle_step(case, mem, m, mem["U0"][m], eps)
        assert np.isfinite(own["c64"]).all() and np.isfinite(own["U64"]).all(), "member %d" % m
        assert own["rel32"] <= N.COST_BAR / 4, "member %d: fp32 relative cost error %.3g" % (m, own["rel32"])
        assert own["eu32"] <= N.U_BAR / 4, "member %d: fp32 U' error %.3g" % (m, own["eu32"])
        near_u, near_c = np.inf, np.inf
        for j in range(case["B"]):
            if j == m:
                continue
            other = N.oracle_step(case, mem, m, mem["U0"][m], eps, net=mem["nets"][j])
            near_u = min(near_u, float(np.abs(other["U64"] - own["U64"]).max()))
            near_c = min(near_c, float((np.abs(other["c64"] - own["c64"]) / np.abs(own["c64"])).max()))
        print("%s member %d: fp32 rel cost err %.3g, |dU'| %.3g; nearest swapped network: |dU'| %.3g, rel cost %.3g" % (
            case["id"], m, own["rel32"], own["eu32"], near_u, near_c))
        assert near_u >= NEEDLE * N.U_BAR, "member %d: a swapped network moves U' by %.3g only" % (m, near_u)
        assert near_c >= NEEDLE * N.COST_BAR, "member %d: a swapped network moves the costs by %.3g only" % (m, near_c)
