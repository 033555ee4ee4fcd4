"""The boundary of the wide batch's trajectory validation without a GPU: mppi_learner_wide_batch_validate is declared, exported and bound
under mppi_learner_batch_rollout's signature, the kernel is in the library, WideLearnerBatch.validate and
LearnerBase.k_fold_trajectory_validation exist, and the latter checks `val` before anything touches a device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


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
    name = "mppi_learner_wide_batch_validate"
    assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared"
    assert hasattr(lib, name), name + " is not exported"
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["mppi_learner_batch_rollout"]
    assert lib.mppi_abi_version() == 5
    assert b"k_wb_rollout" in open(_lib.SO_PATH, "rb").read()
    assert callable(pkg.WideLearnerBatch.validate) and callable(pkg.LearnerBase.k_fold_trajectory_validation)
    # one body behind the narrow rollout and the wide validate; the wide batch still has no `rollout`, the narrow one no `validate`
    assert not hasattr(pkg.WideLearnerBatch, "rollout") and not hasattr(pkg.LearnerBatch, "validate")
    assert pkg.WideLearnerBatch._roll is pkg.LearnerBatch._roll


def test_k_fold_trajectory_validation_checks_val_before_any_device(pkg):
    model = pkg.NNPointMassModel(stateDim=4, actionDim=2, hidden=(256, 256))
    learner = pkg.LearnerBase(model, bufferSize=8)
    rng = np.random.default_rng(0)
    learner.add_rb(rng.standard_normal((8, 4, 1)), rng.standard_normal((8, 2, 1)), rng.standard_normal((8, 4, 1)))
    for bad in (None, (np.zeros((2, 5, 3)), np.zeros((2, 5, 2))), (np.zeros((2, 5, 4)), np.zeros((2, 4, 2))), (np.zeros((2, 1, 4)), np.zeros((2, 1, 2))),
                np.zeros((2, 5, 4))):
        with pytest.raises(ValueError, match="val is"):
            learner.k_fold_trajectory_validation(k=2, learningRate=1e-3, epoch=2, val=bad)
    assert learner._dev is None and learner.kfold_log is None
    empty = pkg.LearnerBase(model, bufferSize=8)
    with pytest.raises(ValueError, match="holds no transitions"):
        empty.k_fold_trajectory_validation(k=2, val=(np.zeros((1, 3, 4)), np.zeros((1, 3, 2))))
    # the pinned refusal names the way out
    with pytest.raises(ValueError, match="is not built into this method: use k_fold_trajectory_validation"):
        learner.k_fold_validation(k=2, val=(np.zeros((1, 3, 4)), np.zeros((1, 3, 2))))
