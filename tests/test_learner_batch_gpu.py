"""Batched learners on the GPU (csrc/mppi_learner_batch.hip; LearnerBase.k_fold_validation / grid_search,
scripts/src/learners/learner_base.py:83-216). The reference is the lone learner: member m of a batch must equal, BIT FOR BIT, a lone
Learner created with the same weights, given X[train_idx_m], Y[train_idx_m] and trained with the member's rates — weights, the loss of
every step's forward pass, and the held-out loss of the updated weights (a second lone learner's evaluate() on the test rows). One
tolerance-based check against torch autograd + the Keras update covers a defect both learners would share."""
import numpy as np
import pytest

import learner_batch_util as U
from learner_util import keras_adam, make_net, torch_loss_and_grads

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


@pytest.fixture(scope="module")
def case5():
    return U.five_member_case()


@pytest.fixture(scope="module")
def run5(m, case5):
    """the five-member batch trained once (2 + 1 + 3 steps); shared, never modified"""
    return U.run_batch(m, case5)


def test_members_equal_their_lone_learners(m, case5, run5):
    c = case5
    assert run5["steps"] == 6 and run5["loss_train"].shape == (6, 5) and run5["loss_test"].shape == (6, 5)
    U.check_members_against_lone(m, c["net"], c["X"], c["Y"], c["train"], c["test"], c["lr"], c["hp"], c["calls"], run5)
    assert np.isnan(run5["loss_test"][:, 0]).all() and np.isfinite(run5["loss_test"][:, 1:]).all()
    assert np.isfinite(run5["loss_train"]).all()


@pytest.mark.parametrize("dims", [[9, 16, 6], [4, 8, 8, 8, 2]])
def test_narrow_and_shallow_networks(m, dims):
    """padding columns (widths below 32) and a two-layer net; pool of 64 rows, three members"""
    n = 64
    X, Y = U.pool(dims, n, 21)
    rng = np.random.default_rng(22)
    train = [rng.permutation(n)[:nt] for nt in (64, 17, 33)]
    test = [rng.permutation(n)[:nt] for nt in (0, 47, 5)]
    lr, hp = (1e-3, 5e-3, 2e-4), [U.DEFAULT_HP, (0.7, 0.9, 1e-5), U.DEFAULT_HP]
    case = dict(net=make_net(dims, 20), X=X, Y=Y, train=train, test=test, lr=lr, hp=hp, calls=(2, 2))
    got = U.run_batch(m, case)
    U.check_members_against_lone(m, case["net"], X, Y, train, test, lr, hp, case["calls"], got)


def test_order_of_the_index_list_is_honoured(m):
    """A member on an index list and one on its reverse (513 rows: three loss blocks, two chunks): each equals its own lone learner, and
    the two first losses differ in bits — the reduction runs over positions in the list, not over sorted or pooled rows."""
    dims, n, seed = [16, 32, 32, 32, 13], 600, 97  # the seed: one for which the precondition below holds (most do; 96 does not)
    X, Y = U.pool(dims, n, seed)
    net = make_net(dims, seed + 1)
    idx = np.random.default_rng(seed + 2).permutation(n)[:513]
    rev = idx[::-1].copy()
    # the precondition, on the CPU: summed the way the kernels sum (blocks of 256 by position, butterfly, wave order, block order), the
    # per-row errors of the initial weights give different fp32 losses in the two orders. The rows' predictions come from a lone learner.
    lone = m.Learner(net)
    lone.set_data(X, Y)
    _, pred = lone.evaluate(pred=True)
    lone.close()
    se = U.row_errors_fp32(pred, Y)
    expect = [U.block_loss_fp32(se[idx], dims[-1]), U.block_loss_fp32(se[rev], dims[-1])]
    assert expect[0] != expect[1]
    none = np.zeros(0, np.int64)
    case = dict(net=net, X=X, Y=Y, train=[idx, rev], test=[none, none], lr=(1e-3, 1e-3), hp=[U.DEFAULT_HP] * 2, calls=(2,))
    got = U.run_batch(m, case)
    U.check_members_against_lone(m, net, X, Y, case["train"], case["test"], case["lr"], case["hp"], case["calls"], got)
    assert got["loss_train"][0, 0] != got["loss_train"][0, 1]
    assert [got["loss_train"][0, 0], got["loss_train"][0, 1]] == expect  # the stated order of the reduction, to the bit


def test_members_are_independent(m, case5, run5):
    """the same batch again with member 2's split, rates and weights changed: the other four return the same bits"""
    c = case5
    rng = np.random.default_rng(41)
    change = (2, rng.permutation(1100)[:700], rng.permutation(1100)[:40], 5e-3, (0.85, 0.995, 1e-6), make_net(c["dims"], 42))
    other = U.run_batch(m, c, change=change)
    for mi in (0, 1, 3, 4):
        np.testing.assert_array_equal(other["loss_train"][:, mi], run5["loss_train"][:, mi])
        np.testing.assert_array_equal(other["loss_test"][:, mi], run5["loss_test"][:, mi])
        for call in range(len(c["calls"])):
            U.same_weights(other["weights"][call][mi], run5["weights"][call][mi])
    assert not np.array_equal(other["loss_train"][:, 2], run5["loss_train"][:, 2])
    assert not np.array_equal(other["loss_test"][:, 2], run5["loss_test"][:, 2])
    assert U.weights_differ(other["weights"][-1][2], run5["weights"][-1][2])


def test_default_split_and_set_data(m):
    dims, n = [16, 32, 32, 32, 13], 300
    X, Y = U.pool(dims, n, 51)
    net = make_net(dims, 52)
    lb = m.LearnerBatch(net, 3)
    lb.set_data(X, Y)
    lt, ls = lb.train(3, 2e-3)
    ref = U.lone_history(m, net, X, Y, np.arange(n), np.zeros(0, np.int64), 2e-3, U.DEFAULT_HP, 3)
    assert np.isnan(ls).all()
    for mi in range(3):  # no set_split: the whole pool, in order; equal rates: equal members
        np.testing.assert_array_equal(lt[:, mi], np.array(ref["loss_train"], F32))
        U.same_weights(lb.get_weights(mi), ref["weights"][-1])
    # a split, then a new pool: the split is gone
    lb.set_split(1, np.arange(10, 50), np.arange(5))
    assert np.isfinite(lb.evaluate()[1][1])
    X2, Y2 = U.pool(dims, 130, 53)
    lb.set_data(X2, Y2)
    tr, te = lb.evaluate()
    assert np.isnan(te).all()
    lone = m.Learner(ref["weights"][-1])
    lone.set_data(X2, Y2)
    assert np.all(tr == F32(lone.evaluate()))
    lt2, _ = lb.train(1, 2e-3)
    first, _ = lone.train(1, 2e-3)
    # (the lone learner's Adam starts afresh; the batch's does not: only the forward pass is comparable)
    assert np.all(lt2[0] == F32(first))
    lb.close()


def test_evaluate(m, case5):
    c = case5
    lb = m.LearnerBatch(c["net"], 5)
    lb.set_data(c["X"], c["Y"])
    for mi in range(5):
        lb.set_split(mi, c["train"][mi], c["test"][mi])
    lr = np.array(c["lr"], F32)
    _, ls = lb.train(2, lr)
    before = [lb.get_weights(mi) for mi in range(5)]
    tr, te = lb.evaluate()
    assert lb.step_count() == 2
    for mi in range(5):
        U.same_weights(lb.get_weights(mi), before[mi])
    np.testing.assert_array_equal(te, ls[-1])  # the held-out loss of the last step's weights, again (NaN where there are no test rows)
    lt, _ = lb.train(1, lr)
    np.testing.assert_array_equal(tr, lt[0])
    assert lb.step_count() == 3
    lb.close()


def test_reset_optimizer_and_step_count(m):
    dims, n = [9, 16, 6], 100
    X, Y = U.pool(dims, n, 61)
    net = make_net(dims, 62)
    idx = [np.arange(n), np.arange(n)[::-1][:37]]
    lb = m.LearnerBatch(net, 2)
    lb.set_data(X, Y)
    lb.set_split(1, idx[1])
    assert lb.step_count() == 0
    lb.train(2, 1e-2)
    assert lb.step_count() == 2
    lb.reset_optimizer()
    assert lb.step_count() == 0
    held = [lb.get_weights(mi) for mi in range(2)]
    lt, _ = lb.train(1, 1e-2)
    assert lb.step_count() == 1
    for mi in range(2):  # a fresh Adam from the weights held: a lone learner started there
        ref = U.lone_history(m, net, X, Y, idx[mi], np.zeros(0, np.int64), 1e-2, U.DEFAULT_HP, 1, start=held[mi])
        assert lt[0, mi] == ref["loss_train"][0]
        U.same_weights(lb.get_weights(mi), ref["weights"][0])
    lb.close()


def test_refusals_leave_the_batch_usable(m):
    dims, n = [4, 8, 2], 40
    X, Y = U.pool(dims, n, 71)
    net = make_net(dims, 72)
    lb = m.LearnerBatch(net, 2)

    def refused(fn, *a, **k):
        with pytest.raises(m.MppiError) as e:
            fn(*a, **k)
        assert e.value.status == 1, str(e.value)

    refused(lb.train, 1, 1e-3)  # before set_data
    lb.set_data(X, Y)
    good = np.arange(n)[::-1][:25].copy()
    lb.set_split(1, good, np.arange(3))
    refused(lb.set_split, 1, [0, n], [1])
    refused(lb.set_split, 1, [0, -1])
    refused(lb.set_split, 1, [0, 1], [n])
    refused(lb.set_split, 1, [])
    refused(lb.set_split, 2, [0, 1])
    refused(lb.set_split, -1, [0, 1])
    refused(lb.get_weights, 2)
    refused(lb.set_weights, net, member=2)
    refused(lb.train, 0, 1e-3)
    refused(lb.train, 1, np.array([1e-3, 1e-3, 1e-3], F32))
    refused(lb.train, 1, 1e-3, beta1=np.array([0.9], F32))
    refused(lb.train, 1, -1.0)
    assert lb.step_count() == 0
    # nothing changed: member 1 still holds the split it was given
    lt, ls = lb.train(2, 1e-3)
    for mi, (tr, te) in enumerate([(np.arange(n), np.zeros(0, np.int64)), (good, np.arange(3))]):
        ref = U.lone_history(m, net, X, Y, tr, te, 1e-3, U.DEFAULT_HP, 2)
        np.testing.assert_array_equal(lt[:, mi], np.array(ref["loss_train"], F32))
        np.testing.assert_array_equal(ls[:, mi], np.array(ref["loss_test"], F32))
        U.same_weights(lb.get_weights(mi), ref["weights"][-1])
    lb.close()


def test_member_against_torch_and_the_keras_update(m, case5, run5):
    """The check that does not lean on the lone learner: member 0's rows through torch CPU fp32 autograd and tf.keras' Adam in numpy.
    The device's gradients meet tests/test_learner_gpu.py's gradient bars (rtol 2e-5, atol 2e-6 max|g|); two steps from torch's
    gradients land within that file's bar for two consecutive steps (atol 3e-7: Adam's first steps move each weight by lr m / (sqrt(v)
    + eps), which a relative gradient error of 2e-5 changes by less than lr 2e-5 = 2e-9 here); the weights equal the lone learner's
    bit for bit."""
    c = case5
    X, Y = c["X"][c["train"][0]], c["Y"][c["train"][0]]
    lone = m.Learner(c["net"])
    lone.set_data(X, Y)
    loss, g = lone.evaluate(grads=True)
    tl, tW, tb = torch_loss_and_grads(c["net"], X, Y)
    assert abs(loss - tl) <= 2e-6 * abs(tl)
    for l in range(len(c["dims"]) - 1):
        np.testing.assert_allclose(g["W"][l], tW[l], rtol=2e-5, atol=2e-6 * max(np.abs(tW[l]).max(), 1e-12))
        np.testing.assert_allclose(g["b"][l], tb[l], rtol=2e-5, atol=2e-6 * max(np.abs(tb[l]).max(), 1e-12))
    ref = dict(W=[w.copy() for w in c["net"]["W"]], b=[v.copy() for v in c["net"]["b"]])
    state = dict(W=[(np.zeros_like(w), np.zeros_like(w)) for w in ref["W"]], b=[(np.zeros_like(v), np.zeros_like(v)) for v in ref["b"]])
    for t in (1, 2):
        _, gW, gb = torch_loss_and_grads(ref, X, Y)
        keras_adam(ref, state, gW, gb, t, c["lr"][0], *c["hp"][0])
    lone.train(2, c["lr"][0], *c["hp"][0])
    got = run5["weights"][0][0]  # member 0 after the first call's two steps
    U.same_weights(got, lone.get_weights())
    worst = max(np.abs(got[key][l] - ref[key][l]).max() for key in ("W", "b") for l in range(len(ref["W"])))
    print("member 0 after 2 steps against torch + Keras Adam: max |dw| = %.3g" % worst)
    for l in range(len(ref["W"])):
        np.testing.assert_allclose(got["W"][l], ref["W"][l], rtol=0, atol=3e-7)
        np.testing.assert_allclose(got["b"][l], ref["b"][l], rtol=0, atol=3e-7)
    assert U.weights_differ(got, c["net"])


def test_k_fold_validation_and_grid_search(m):
    n, k, rates, epoch = 264, 3, (1e-3, 1e-2), 5
    x, u, xn = U.fossen_transitions(m, n)
    model = m.NNAUVModel()
    learner = m.LearnerBase(model, bufferSize=n)
    learner.add_rb(x, u, xn)
    learner.stats()
    w0 = [w.copy() for w in model.get_weights()]
    seen = []
    log = learner.k_fold_validation(k=k, learningRate=rates, epoch=epoch, seed=3, writer=lambda e, d: seen.append((e, d["test"].shape)))
    assert log["train"].shape == (epoch, 2, k) and log["test"].shape == (epoch, 2, k) and log is learner.kfold_log
    assert seen == [(e, (2, k)) for e in range(epoch)]
    for a, b in zip(model.get_weights(), w0):  # the reference trains copies
        np.testing.assert_array_equal(a, b)
    assert learner._dev is None
    # the same members, by hand
    X, y = model.prepare_training_data(x, xn, u)
    folds = m.kfold_indices(n, k, 3)
    lb = m.LearnerBatch(dict(W=w0[0::2], b=w0[1::2]), 2 * k)
    lb.set_data(X, y)
    for r in range(2):
        for f, (tr, te) in enumerate(folds):
            lb.set_split(r * k + f, tr, te)
    lt, ls = lb.train(epoch, np.repeat(np.array(rates, F32), k))
    lb.close()
    np.testing.assert_array_equal(log["train"], lt.reshape(epoch, 2, k))
    np.testing.assert_array_equal(log["test"], ls.reshape(epoch, 2, k))
    assert np.isfinite(log["test"]).all()
    one = learner.k_fold_validation(k=k, learningRate=1e-2, epoch=epoch, seed=3)  # a scalar rate keeps the R axis
    assert one["test"].shape == (epoch, 1, k)
    np.testing.assert_array_equal(one["test"][:, 0], log["test"][:, 1])
    best, table = learner.grid_search(rates, k=k, epoch=epoch, seed=3)
    np.testing.assert_allclose(table, log["test"][-1].astype(np.float64).mean(axis=1), rtol=0, atol=0)
    assert table.shape == (2,) and best == rates[int(np.argmin(table))]


def test_learn_loop_chooses_its_rate_by_k_fold(m, capsys):
    """examples/learn_loop.py --kfold K --lrs a,b: one more line per round with the table, and the round trains at the chosen rate"""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import learn_loop
    finally:
        sys.path.pop(0)
    argv = ["--rounds", "2", "--samples", "128", "--horizon", "8", "--steps", "12", "--epochs", "3", "--hidden", "16", "--layers", "1"]
    _, _, figures = learn_loop.main(argv + ["--kfold", "3", "--lrs", "1e-3,1e-2"])
    out = capsys.readouterr().out.splitlines()
    tables = [l for l in out if "3-fold held-out loss" in l]
    assert len(tables) == 2 and len(out) == 4 and all("-> lr 0.01" in l or "-> lr 0.001" in l for l in tables)
    assert np.isfinite(np.array([f[:5] for f in figures])).all()
    learn_loop.main(argv)
    assert len(capsys.readouterr().out.splitlines()) == 2  # without the flags: the rounds' lines alone
