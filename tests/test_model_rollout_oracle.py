"""The two identities the readout test on the GPU leans on (test_model_rollout_gpu.py::test_readout_needle), proven on the CPU with the
oracle in fp32 at exactly that test's cases (model_rollout_util.readout_case), on the noise the step draws as the oracle restates it:
  1. iterating Problem.model_next and Problem.state_cost along V = U + eps[k] reproduces, bit for bit, the trajectory that
     Problem.rollout_cost(..., traj=True) exports for sample k;
  2. the sequential fp32 recurrence c = c + (C[t] + action_cost(U[t], eps[k, t])) for t = 0 .. H-1, then c = c + C[H-1]
     (orc_rollout_cost's order) equals rollout_cost's value for sample k bit for bit.
So a sample's cost can be rebuilt from the states of its trajectory alone — which is what a readout of the right sample, step and row
gives, and a wrong one does not. No GPU."""
import numpy as np
import pytest

from model_rollout_util import F32, readout_case, rollout_cost_from
from oracle import oracle as orc


@pytest.fixture(scope="module", params=["pm", "auv"])
def setup(request):
    case = readout_case(request.param)
    p = orc.Problem(threads=0, **case["problem"])
    eps = orc.noise(case["seed"], 0, 0, case["K"], case["H"], case["a"], case["sigma"])
    assert eps.dtype == F32 and eps.shape == (case["K"], case["H"], case["a"])
    cost, traj = p.rollout_cost(case["x"], case["U"], eps, traj=True)
    assert np.isfinite(cost).all() and np.isfinite(traj).all()
    return case, p, eps, cost, traj


def _iterate(case, p, eps, k):
    """-> (states [H, s], state costs [H]) of sample k by model_next / state_cost, one call per step"""
    V = (case["U"] + eps[k]).astype(F32)  # v = u + e, an fp32 add
    x, X, Cs = case["x"], [], []
    for t in range(case["H"]):
        x = p.model_next(x, V[t])[0]
        X.append(x)
        Cs.append(p.state_cost(x)[0])
    return np.stack(X), np.asarray(Cs, F32)


def test_iterating_the_model_reproduces_the_exported_trajectory(setup):
    case, p, eps, cost, traj = setup
    for k in range(case["K"]):
        X, _ = _iterate(case, p, eps, k)
        np.testing.assert_array_equal(X, traj[k], err_msg="sample %d" % k)


def test_the_fp32_recurrence_rebuilds_the_rollout_cost(setup):
    case, p, eps, cost, traj = setup
    moved = 0
    for k in range(case["K"]):
        _, Cs = _iterate(case, p, eps, k)
        ac = np.asarray([p.action_cost(case["U"][t], eps[k, t])[0] for t in range(case["H"])], F32)
        assert rollout_cost_from(Cs, ac) == cost[k], "sample %d" % k
        # ... and the state costs of ANOTHER sample's trajectory do not: the recurrence tells samples apart
        _, Co = _iterate(case, p, eps, (k + 1) % case["K"])
        moved += rollout_cost_from(Co, ac) != cost[k]
    assert moved == case["K"]
