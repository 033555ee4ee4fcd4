"""The trajectory-validation cases of a learner batch, proven real tests before they reach a GPU (no GPU here): the fp64 trajectories stay
bounded, the squared errors are large enough for a relative bar to mean something, and a kernel that mixed up two members, lost a
trajectory or stopped a step early would move a sum by far more than the bar the GPU test holds it to. One symbol test: the entry point is
declared, exported and bound."""
import os
import re

import numpy as np
import pytest

import learner_rollout_util as U
from conftest import ROOT

NAMES = sorted(U.CASES)
BAR = U.sse_bar(U.T_SSE)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_entry_point_is_declared_exported_and_bound(pkg):
    txt = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from mppi_tf_amd import _lib
    lib = pkg.load()
    assert re.search(r"\}\s*mppi_learner_model\s*;", txt), "mppi_learner_model is not declared"
    assert re.search(r"\bmppi_learner_batch_rollout\s*\(", txt), "mppi_learner_batch_rollout is not declared"
    assert hasattr(lib, "mppi_learner_batch_rollout"), "mppi_learner_batch_rollout is not exported"
    assert "mppi_learner_batch_rollout" in _lib.SIGNATURES
    assert lib.mppi_abi_version() == 5
    assert callable(pkg.LearnerBatch.rollout) and callable(pkg.LearnerBase.validate_fold)
    assert b"k_lb_rollout" in open(_lib.SO_PATH, "rb").read()


@pytest.fixture(scope="module", params=NAMES)
def proven(request):
    """(case, x0, V, G, X64 [B, T+1, n, s]: the members' fp64 trajectories, sse [B, s])"""
    c, x0, V, G = U.sse_case(request.param)
    X64 = np.stack([U.rollout(c["kind"], net, c["norm"], x0, V, np.float64) for net in c["nets"]])
    return c, x0, V, G, X64, U.sse64(X64, G)


def test_trajectories_stay_finite_and_bounded(proven):
    c, x0, V, G, X64, sse = proven
    assert np.isfinite(X64).all() and np.abs(X64).max() < 1e3
    assert np.isfinite(G).all() and np.abs(G).max() < 1e3
    # the fp32 restatement follows the fp64 one: the case does not sit on an instability
    X32 = U.rollout(c["kind"], c["nets"][0], c["norm"], x0, V)
    assert X32.dtype == np.float32 and np.abs(X32 - X64[0]).max() < 1e-4


def test_squared_errors_are_large_enough(proven):
    sse = proven[5]
    assert sse.shape == (3, proven[0]["s"]) and (sse.mean(axis=0) >= 1e-6).all()


def test_members_differ_by_far_more_than_the_bar(proven):
    sse = proven[5]
    for a in range(3):
        for b in range(a + 1, 3):
            rel = np.abs(sse[a] - sse[b]) / np.maximum(sse[a], sse[b])
            assert (rel > 100 * BAR).all(), (a, b, rel.min())


def test_a_lost_trajectory_or_step_moves_the_sum(proven):
    c, x0, V, G, X64, sse = proven
    d2 = (X64 - G.astype(np.float64)[None]) ** 2                # [B, T+1, n, s]
    per_traj = d2.sum(axis=1) / sse[:, None, :]                  # [B, n, s]: the share of trajectory i
    assert (per_traj > 2 * BAR).all(), per_traj.min()
    last_step = d2[:, -1].sum(axis=1) / sse                      # [B, s]
    assert (last_step > 2 * BAR).all(), last_step.min()


def test_the_dead_unit_is_dead(proven):
    c, x0, V, G, X64, sse = proven
    if c["dead"] is None:
        assert len(c["dims"]) == 2  # the one-layer network has no hidden unit
        return
    l, u = c["dead"]
    for net in c["nets"]:
        assert not net["W"][l][:, u].any() and net["b"][l][u] < 0


def test_no_input_near_the_subnormal_range(proven):
    c, x0, V, G = proven[:4]
    arrays = [x0, V, G] + list(c["norm"].values()) + [a for net in c["nets"] for a in net["W"] + net["b"]]
    for a in arrays:
        a = np.abs(np.asarray(a, np.float64))
        assert ((a == 0) | (a > 1e-30)).all()
    assert (np.asarray(c["norm"]["xstd"]) != 0).all()


def test_k_fold_validation_checks_val_before_any_device(pkg):
    class NoDeviceModel:  # anything but the dimensions would raise AttributeError
        def get_state_dim(self):
            return 13

        def get_action_dim(self):
            return 6

    learner = pkg.LearnerBase(NoDeviceModel())
    for bad in ((np.zeros((2, 5, 12)), np.zeros((2, 5, 6))), (np.zeros((2, 5, 13)), np.zeros((2, 4, 6))), (np.zeros((2, 1, 13)), np.zeros((2, 1, 6))),
                np.zeros((2, 5, 13))):
        with pytest.raises(ValueError, match="val is"):
            learner.k_fold_validation(k=3, val=bad)
    with pytest.raises(ValueError, match='by is "test" or "val"'):
        learner.grid_search([1e-3], by="val")
