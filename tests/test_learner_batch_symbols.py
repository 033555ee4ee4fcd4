"""The batched learner's boundary without a GPU: every new entry point is declared, exported and bound; mppi_learner_batch_create checks
the shape and the member count before the device; kfold_indices makes sklearn-sized folds; k_fold_validation refuses `val` before
anything touches a device."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from learner_util import REFUSED_SHAPES, make_net

ENTRY_POINTS = ("create", "destroy", "last_error", "size", "set_data", "set_split", "set_weights", "get_weights", "reset_optimizer", "get_step",
                "train", "evaluate")


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
    assert re.search(r"typedef\s+struct\s+mppi_learner_batch\s+mppi_learner_batch\s*;", txt)
    for name in ("mppi_learner_batch_" + e for e in ENTRY_POINTS):
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SIGNATURES, name + " is not bound"
    assert lib.mppi_abi_version() == 5
    assert pkg.LearnerBatch is _lib.LearnerBatch and callable(pkg.kfold_indices)


def test_create_checks_shape_and_member_count_before_the_device(pkg):
    for dims in list(REFUSED_SHAPES) + [[9, 256, 256, 6]]:
        with pytest.raises(pkg.MppiError) as e:
            pkg.LearnerBatch(make_net(dims), 3)
        assert e.value.status == 4, dims
    for members in (0, 1025):
        with pytest.raises(pkg.MppiError) as e:
            pkg.LearnerBatch(make_net([16, 32, 32, 32, 13]), members)
        assert e.value.status == 1, members
    if not has_gpu():  # a legal shape gets as far as the device
        with pytest.raises(pkg.MppiError) as e:
            pkg.LearnerBatch(make_net([16, 32, 32, 32, 13]), 3)
        assert e.value.status == 2 and "no CPU path" in str(e.value)


@pytest.mark.parametrize("n,k", [(10, 2), (11, 3), (264, 10), (7, 7)])
def test_kfold_indices(pkg, n, k):
    folds = pkg.kfold_indices(n, k, 5)
    assert len(folds) == k
    tests = [np.asarray(te) for _, te in folds]
    assert sorted(np.concatenate(tests).tolist()) == list(range(n))  # disjoint and covering
    assert [len(t) for t in tests] == [n // k + 1] * (n % k) + [n // k] * (k - n % k)
    for i, (tr, te) in enumerate(folds):
        assert not set(tr.tolist()) & set(te.tolist())
        assert sorted(tr.tolist() + te.tolist()) == list(range(n))
        np.testing.assert_array_equal(tr, np.concatenate([tests[j] for j in range(k) if j != i]))  # the other folds, in fold order
    np.testing.assert_array_equal(np.concatenate(tests), np.random.default_rng(5).permutation(n))
    again = pkg.kfold_indices(n, k, 5)
    for (a, b), (c, d) in zip(folds, again):
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(b, d)
    for bad in (1, n + 1):
        with pytest.raises(ValueError):
            pkg.kfold_indices(n, bad, 5)


def test_k_fold_validation_refuses_val_before_any_device(pkg):
    class NoDeviceModel:  # anything but the dimensions would raise AttributeError
        def get_state_dim(self):
            return 13

        def get_action_dim(self):
            return 6

    learner = pkg.LearnerBase(NoDeviceModel())
    with pytest.raises(ValueError):
        learner.k_fold_validation(k=3, val=(np.zeros((1, 2, 13)), np.zeros((1, 2, 6))))
