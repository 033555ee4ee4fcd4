"""The batched wide learner's boundary without a GPU: every entry point of mppi_learner_wide_batch_* is declared, exported and bound;
create checks the shape and the member count before the device; k_fold_validation refuses `val` and `episode` for a wide model before
anything touches a device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from learner_util import REFUSED_SHAPES, make_net

ENTRY_POINTS = ("create", "destroy", "last_error", "size", "set_data", "set_split", "set_weights", "get_weights", "reset_optimizer", "get_step",
                "train", "evaluate")
WIDE = [9, 256, 256, 6]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_entry_points_are_declared_exported_and_bound(pkg):
    txt = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from mppi_tf_amd import _lib
    lib = pkg.load()
    assert re.search(r"typedef\s+struct\s+mppi_learner_wide_batch\s+mppi_learner_wide_batch\s*;", txt)
    for e in ENTRY_POINTS:
        name = "mppi_learner_wide_batch_" + e
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SIGNATURES, name + " is not bound"
        res, args = _lib.SIGNATURES[name]
        assert (res, args) == _lib.SIGNATURES["mppi_learner_batch_" + e], name + " has another signature than its narrow namesake"
    assert not hasattr(lib, "mppi_learner_wide_batch_rollout") and not hasattr(pkg.WideLearnerBatch, "rollout")
    assert lib.mppi_abi_version() == 5
    assert pkg.WideLearnerBatch is _lib.WideLearnerBatch and "WideLearnerBatch" in pkg.__all__
    for method in ("set_data", "set_split", "set_weights", "get_weights", "train", "evaluate", "reset_optimizer", "step_count", "close"):
        assert callable(getattr(pkg.WideLearnerBatch, method)), method


def test_create_checks_shape_and_member_count_before_the_device(pkg):
    for dims in list(REFUSED_SHAPES) + [[16, 32, 32, 32, 13]]:
        with pytest.raises(pkg.MppiError) as e:
            pkg.WideLearnerBatch(make_net(dims), 3)
        assert e.value.status == 4, dims
    for members in (0, 1025):
        with pytest.raises(pkg.MppiError) as e:
            pkg.WideLearnerBatch(make_net(WIDE), members)
        assert e.value.status == 1, members
    if not has_gpu():  # a legal shape gets as far as the device
        with pytest.raises(pkg.MppiError) as e:
            pkg.WideLearnerBatch(make_net(WIDE), 3)
        assert e.value.status == 2 and "no CPU path" in str(e.value)


def test_the_narrow_batch_still_refuses_the_wide_shape(pkg):
    with pytest.raises(pkg.MppiError) as e:
        pkg.LearnerBatch(make_net(WIDE), 3)
    assert e.value.status == 4 and "is not batched" in str(e.value)


def test_k_fold_validation_refuses_trajectory_validation_of_a_wide_model_before_any_device(pkg):
    model = pkg.NNPointMassModel(stateDim=4, actionDim=2, hidden=(256, 256))
    learner = pkg.LearnerBase(model, bufferSize=8)
    rng = np.random.default_rng(0)
    learner.add_rb(rng.standard_normal((8, 4, 1)), rng.standard_normal((8, 2, 1)), rng.standard_normal((8, 4, 1)))
    val = (np.zeros((1, 3, 4)), np.zeros((1, 3, 2)))
    episode = dict(controller=None, plant=None, x0=np.zeros(4), n_steps=1)
    calls = (lambda: learner.k_fold_validation(k=2, val=val),
             lambda: learner.k_fold_validation(k=2, episode=episode),
             lambda: learner.grid_search([1e-3, 1e-2], k=2, val=val, by="val"),
             lambda: learner.grid_search([1e-3, 1e-2], k=2, by="episode", episode=episode))
    for call in calls:
        with pytest.raises(ValueError, match="trajectory validation of wide members is not built"):
            call()
    assert learner._dev is None and learner.kfold_log is None
    narrow = pkg.LearnerBase(pkg.NNPointMassModel(stateDim=4, actionDim=2, hidden=(32, 32)))
    assert not narrow._is_wide(narrow.model.get_weights()) and learner._is_wide(model.get_weights())
