"""The case matrix of the batched learned-model controllers (batch_nn_util.CASES), judged on the CPU with the oracle alone, before any
kernel runs on it. For every case and checked member:
  * the case is well conditioned: every fp64 cost is finite, and an fp32 CPU evaluation of the same update stays inside the bars the GPU
    is held to (costs within 2e-5 of fp64 relatively; U' within max(1e-5, 4 x its own error));
  * the case is a needle for the one mistake a batch can make — member m reading another member's network: U' of member m computed with
    member j's network differs from its own by at least 100 x the U' bar, for every j != m.
The noise is each member's own Philox noise of step 0."""
import numpy as np
import pytest

import batch_nn_util as N

NEEDLE = 100.0


@pytest.mark.parametrize("ci", range(len(N.CASES)), ids=N.IDS)
def test_case_is_well_conditioned_and_a_needle_for_a_swapped_network(ci):
    case, mem = N.CASES[ci], N.members(ci)
    for m in N.checked(case):
        eps = N.first_noise(case, mem, m)
        own = N.oracle_step(case, mem, m, mem["U0"][m], eps)
        assert np.isfinite(own["c64"]).all() and np.isfinite(own["U64"]).all(), "member %d" % m
        # an fp32 CPU evaluation passes what the GPU must pass: rel < 2e-5 and < 4 x max(its own, 1e-6); |dU'| <= max(1e-5, 4 x its own)
        assert own["rel32"] < N.COST_BAR, "member %d: fp32 relative cost error %.3g" % (m, own["rel32"])
        assert own["eu32"] <= own["u_bar"]
        nearest = np.inf
        for j in range(case["B"]):
            if j == m:
                continue
            other = N.oracle_step(case, mem, m, mem["U0"][m], eps, net=mem["nets"][j])
            nearest = min(nearest, float(np.abs(other["U64"] - own["U64"]).max()))
        print("%s member %d: fp32 rel cost err %.3g, |dU'| %.3g, bar %.3g, nearest swapped network %.3g" % (
            case["id"], m, own["rel32"], own["eu32"], own["u_bar"], nearest))
        assert nearest >= NEEDLE * own["u_bar"], "member %d: a swapped network moves U' by %.3g only, bar %.3g" % (m, nearest, own["u_bar"])
