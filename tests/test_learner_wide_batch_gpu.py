"""Batched wide learners on the GPU (csrc/mppi_learner_wide_batch.hip): B learners of the [in, 256, 256, out] network in the launches of
one. The reference is the lone wide learner (csrc/mppi_learner_wide.hip): member m must equal, BIT FOR BIT, a lone Learner created with
the same weights, given X[train_idx_m], Y[train_idx_m] and trained with the member's rates — weights, the loss of every step's forward
pass, and the held-out loss of the updated weights (a second lone learner's evaluate() on the test rows). One check against the edge
matrix's fp64 loss covers a defect both learners would share."""
import numpy as np
import pytest

import learner_batch_util as U
import learner_edges_util as E
from learner_util import make_net

pytestmark = pytest.mark.gpu
F32 = np.float32
NONE = np.zeros(0, np.int64)
POOL = 1100
# the tile (64), slab (32) and chunk (512) edges of learner_edges_util.N_WIDE, three members each
N_TRAIN = ((1, 65, 513), (64, 512, 1025), (63, 511, 33))
DIMS = ([9, 256, 256, 6], [1, 256, 256, 1], [32, 256, 256, 32])
assert all(n in E.N_WIDE for t in N_TRAIN for n in t)


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


def three_member_case(dims, n_train, seed):
    """one pool; permuted index lists of the three lengths, the longest with repeated rows; test lists of 0, 1 and 65 rows in an order that
    turns with the seed; every member its own lr, beta1, beta2, eps"""
    X, Y = U.pool(dims, POOL, seed)
    rng = np.random.default_rng(seed + 1)
    longest = int(np.argmax(n_train))
    train = [rng.integers(0, POOL, nt) if mi == longest and nt > 1 else rng.permutation(POOL)[:nt] for mi, nt in enumerate(n_train)]
    assert len(np.unique(train[longest])) < len(train[longest])  # repeated rows
    n_test = np.roll((0, 1, 65), seed % 3)
    test = [rng.permutation(POOL)[:nt] for nt in n_test]
    lr = (1e-3, 3e-3, 3e-4)
    hp = [U.DEFAULT_HP, (0.8, 0.99, 1e-6), (0.95, 0.9999, 1e-8)]
    return dict(dims=dims, net=make_net(dims, seed + 2), X=X, Y=Y, train=train, test=test, lr=lr, hp=hp, calls=(4,))


def run_batch(m, case, change=None):
    """learner_batch_util.run_batch on a WideLearnerBatch"""
    B = len(case["train"])
    train, test, lr, hp = list(case["train"]), list(case["test"]), list(case["lr"]), list(case["hp"])
    wb = m.WideLearnerBatch(case["net"], B)
    wb.set_data(case["X"], case["Y"])
    if change is not None:
        mi = change[0]
        train[mi], test[mi], lr[mi], hp[mi] = change[1:5]
    for mi in range(B):
        wb.set_split(mi, train[mi], test[mi])
    b1, b2, eps = (np.array([h[q] for h in hp], F32) for q in range(3))
    lt, ls, weights = [], [], []
    for steps in case["calls"]:
        a, b = wb.train(steps, np.array(lr, F32), b1, b2, eps)
        lt.append(a)
        ls.append(b)
        weights.append([wb.get_weights(mi) for mi in range(B)])
    steps_done = wb.step_count()
    wb.close()
    return dict(loss_train=np.concatenate(lt), loss_test=np.concatenate(ls), weights=weights, steps=steps_done)


@pytest.fixture(scope="module")
def case0():
    return three_member_case(DIMS[0], N_TRAIN[1], 40)


@pytest.fixture(scope="module")
def run0(m, case0):
    """the first network's (64, 512, 1025) batch trained once; shared, never modified"""
    return run_batch(m, case0)


@pytest.mark.parametrize("n_train", N_TRAIN, ids=lambda t: "n%d-%d-%d" % t)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "%dx256x256x%d" % (d[0], d[-1]))
def test_members_equal_their_lone_learners(m, dims, n_train):
    """weights of all three layers after the 4 steps and every loss of every step, against lone learners stepped one step at a time"""
    c = three_member_case(dims, n_train, 10 + 3 * DIMS.index(dims) + N_TRAIN.index(n_train))
    got = run_batch(m, c)
    assert got["steps"] == 4 and got["loss_train"].shape == (4, 3) and got["loss_test"].shape == (4, 3)
    assert len(got["weights"][0][0]["W"]) == 3
    U.check_members_against_lone(m, c["net"], c["X"], c["Y"], c["train"], c["test"], c["lr"], c["hp"], c["calls"], got)
    for mi in range(3):
        assert np.isnan(got["loss_test"][:, mi]).all() if len(c["test"][mi]) == 0 else np.isfinite(got["loss_test"][:, mi]).all()
    assert np.isfinite(got["loss_train"]).all()


def test_members_are_independent(m, case0, run0):
    """the same batch again with member 1's split and rates changed: members 0 and 2 return the same bits"""
    c = case0
    rng = np.random.default_rng(41)
    other = run_batch(m, c, change=(1, rng.permutation(POOL)[:700], rng.permutation(POOL)[:40], 5e-3, (0.85, 0.995, 1e-6)))
    for mi in (0, 2):
        np.testing.assert_array_equal(other["loss_train"][:, mi], run0["loss_train"][:, mi])
        np.testing.assert_array_equal(other["loss_test"][:, mi], run0["loss_test"][:, mi])
        U.same_weights(other["weights"][0][mi], run0["weights"][0][mi])
    assert not np.array_equal(other["loss_train"][:, 1], run0["loss_train"][:, 1])
    assert U.weights_differ(other["weights"][0][1], run0["weights"][0][1])


def test_first_loss_against_fp64(m):
    """a member whose rows are exactly a case of the learner edge matrix (513 rows: nine loss blocks, two chunks), beside a member on other
    rows: its first loss_train within the suite's bar of the case's fp64 loss"""
    case = next(c for c in E.WIDE_CASES if c["id"] == "wide-9x256x256x6-n513")
    net, X, Y = E.inputs(case)
    wb = m.WideLearnerBatch(net, 2)
    wb.set_data(X, Y)
    wb.set_split(0, np.arange(40, 140), np.arange(7))
    wb.set_split(1, np.arange(case["n"]))
    lt, _ = wb.train(1, 1e-3)
    wb.close()
    ref = E.reference(case)["loss"]
    print("loss_train %.9g, fp64 %.9g, relative distance %.3g (bar %g)" % (lt[0, 1], ref, abs(lt[0, 1] - ref) / ref, E.LOSS_RTOL))
    assert abs(float(lt[0, 1]) - ref) <= E.LOSS_RTOL * ref


def test_1024_members(m):
    """B = 1024 on two rows each, 2 steps: the first, a middle and the last member against their lone learners"""
    dims, B = [9, 256, 256, 6], 1024
    X, Y = U.pool(dims, 96, 60)
    net = make_net(dims, 61)
    rng = np.random.default_rng(62)
    train = [rng.permutation(96)[:2] for _ in range(B)]
    test = [rng.permutation(96)[:mi % 3] for mi in range(B)]
    lr = (10.0 ** rng.uniform(-4, -2, B)).astype(F32)
    wb = m.WideLearnerBatch(net, B)
    wb.set_data(X, Y)
    for mi in range(B):
        wb.set_split(mi, train[mi], test[mi])
    lt, ls = wb.train(2, lr)
    assert wb.step_count() == 2 and lt.shape == (2, B)
    for mi in (0, 511, 1023):
        ref = U.lone_history(m, net, X, Y, train[mi], test[mi], float(lr[mi]), U.DEFAULT_HP, 2)
        U.same_weights(wb.get_weights(mi), ref["weights"][-1])
        np.testing.assert_array_equal(lt[:, mi], np.array(ref["loss_train"], F32))
        np.testing.assert_array_equal(ls[:, mi], np.array(ref["loss_test"], F32))
    wb.close()


def test_state(m, case0, run0):
    c = case0
    B = 3
    lr = np.array(c["lr"], F32)
    b1, b2, eps = (np.array([h[q] for h in c["hp"]], F32) for q in range(3))
    wb = m.WideLearnerBatch(c["net"], B)
    wb.set_data(c["X"], c["Y"])
    for mi in range(B):
        wb.set_split(mi, c["train"][mi], c["test"][mi])
    # evaluate: both losses of the current weights, nothing changes
    tr, te = wb.evaluate()
    assert wb.step_count() == 0
    for mi in range(B):
        U.same_weights(wb.get_weights(mi), c["net"])
        lone = m.Learner(c["net"])
        lone.set_data(c["X"][c["train"][mi]], c["Y"][c["train"][mi]])
        assert tr[mi] == F32(lone.evaluate())
        if len(c["test"][mi]):
            lone.set_data(c["X"][c["test"][mi]], c["Y"][c["test"][mi]])
            assert te[mi] == F32(lone.evaluate())
        else:
            assert np.isnan(te[mi])
        lone.close()
    np.testing.assert_array_equal(tr, run0["loss_train"][0])  # and it is the loss the first step then reports
    # two calls continue where the first stopped: equal to one call of the summed steps
    lt1, ls1 = wb.train(1, lr, b1, b2, eps)
    assert wb.step_count() == 1
    lt2, ls2 = wb.train(3, lr, b1, b2, eps)
    assert wb.step_count() == 4
    np.testing.assert_array_equal(np.concatenate([lt1, lt2]), run0["loss_train"])
    np.testing.assert_array_equal(np.concatenate([ls1, ls2]), run0["loss_test"])
    for mi in range(B):
        U.same_weights(wb.get_weights(mi), run0["weights"][0][mi])
    # set_weights(member=-1) and get_weights round-trip; reset_optimizer then train equals a fresh batch
    wb.set_weights(c["net"])
    for mi in range(B):
        U.same_weights(wb.get_weights(mi), c["net"])
    wb.reset_optimizer()
    assert wb.step_count() == 0
    lt, ls = wb.train(4, lr, b1, b2, eps)
    np.testing.assert_array_equal(lt, run0["loss_train"])
    np.testing.assert_array_equal(ls, run0["loss_test"])
    for mi in range(B):
        U.same_weights(wb.get_weights(mi), run0["weights"][0][mi])
    # one member's weights alone
    other = make_net(c["dims"], 77)
    wb.set_weights(other, member=1)
    U.same_weights(wb.get_weights(1), other)
    U.same_weights(wb.get_weights(0), run0["weights"][0][0])
    wb.close()


def test_refusals_leave_the_batch_usable(m):
    dims, n = [9, 256, 256, 6], 80
    X, Y = U.pool(dims, n, 70)
    net = make_net(dims, 71)
    wb = m.WideLearnerBatch(net, 2)
    with pytest.raises(m.MppiError) as e:  # no data yet
        wb.train(1, 1e-3)
    assert e.value.status == 1
    wb.set_data(X, Y)
    wb.set_split(0, np.arange(10, 50), np.arange(5))
    before = wb.evaluate()
    for bad_train, bad_test in (([3, n], NONE), ([3, -1], NONE), ([3, 4], [n]), (NONE, [1])):
        with pytest.raises(m.MppiError) as e:
            wb.set_split(0, bad_train, bad_test)
        assert e.value.status == 1
        after = wb.evaluate()  # nothing changed
        np.testing.assert_array_equal(after[0], before[0])
        np.testing.assert_array_equal(after[1], before[1])
    for member in (-1, 2):
        with pytest.raises(m.MppiError) as e:
            wb.set_split(member, [1, 2], NONE)
        assert e.value.status == 1
        with pytest.raises(m.MppiError) as e:
            wb.get_weights(member)
        assert e.value.status == 1
    with pytest.raises(m.MppiError) as e:
        wb.set_weights(net, member=2)
    assert e.value.status == 1
    for bad_lr in (0.0, [1e-3, -1.0]):
        with pytest.raises(m.MppiError) as e:
            wb.train(1, bad_lr)
        assert e.value.status == 1
    assert wb.step_count() == 0
    lt, ls = wb.train(2, 1e-3)  # still the batch it was
    ref = U.lone_history(m, net, X, Y, np.arange(10, 50), np.arange(5), 1e-3, U.DEFAULT_HP, 2)
    np.testing.assert_array_equal(lt[:, 0], np.array(ref["loss_train"], F32))
    np.testing.assert_array_equal(ls[:, 0], np.array(ref["loss_test"], F32))
    U.same_weights(wb.get_weights(0), ref["weights"][-1])
    ref1 = U.lone_history(m, net, X, Y, np.arange(n), NONE, 1e-3, U.DEFAULT_HP, 2)  # member 1: the default split
    np.testing.assert_array_equal(lt[:, 1], np.array(ref1["loss_train"], F32))
    assert np.isnan(ls[:, 1]).all()
    wb.close()


def test_k_fold_validation_of_a_wide_model(m):
    """LearnerBase.k_fold_validation on the hidden-256 point mass: [epoch, R, k] tables equal to lone learners trained per fold and rate"""
    n, k, rates, epoch = 90, 3, (1e-3, 1e-2), 3
    rng = np.random.default_rng(80)
    x, u = rng.standard_normal((n, 4, 1)), rng.standard_normal((n, 2, 1))
    xn = x + 0.1 * np.concatenate([x[:, 1:2], u[:, 0:1], x[:, 3:4], u[:, 1:2]], axis=1)
    model = m.NNPointMassModel(stateDim=4, actionDim=2, hidden=(256, 256), seed=81)
    learner = m.LearnerBase(model, bufferSize=n)
    learner.add_rb(x, u, xn)
    learner.stats()
    w0 = [w.copy() for w in model.get_weights()]
    log = learner.k_fold_validation(k=k, learningRate=rates, epoch=epoch, seed=3)
    assert log["train"].shape == (epoch, 2, k) and log["test"].shape == (epoch, 2, k) and log is learner.kfold_log
    for a, b in zip(model.get_weights(), w0):  # copies were trained
        np.testing.assert_array_equal(a, b)
    X, y = model.prepare_training_data(x, xn, u)
    X, y = np.asarray(X, F32).reshape(n, 6), np.asarray(y, F32).reshape(n, 4)
    net = dict(W=w0[0::2], b=w0[1::2])
    for r, rate in enumerate(rates):
        for f, (tr, te) in enumerate(m.kfold_indices(n, k, 3)):
            ref = U.lone_history(m, net, X, y, tr, te, float(F32(rate)), U.DEFAULT_HP, epoch)
            np.testing.assert_array_equal(log["train"][:, r, f], np.array(ref["loss_train"], F32))
            np.testing.assert_array_equal(log["test"][:, r, f], np.array(ref["loss_test"], F32))
    best, table = learner.grid_search(rates, k=k, epoch=epoch, seed=3)
    np.testing.assert_array_equal(table, log["test"][-1].astype(np.float64).mean(axis=1))
    assert best == rates[int(np.argmin(table))]
    with pytest.raises(ValueError, match="trajectory validation of wide members is not built"):
        learner.k_fold_validation(k=k, val=(np.zeros((1, 3, 4)), np.zeros((1, 3, 2))))


def test_learn_loop_chooses_the_wide_models_rate_by_k_fold(m, capsys):
    """examples/learn_loop.py --model point_mass --hidden 256 --kfold K --lrs a,b: one more line per round with the table, as at --hidden 32"""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import learn_loop
    finally:
        sys.path.pop(0)
    argv = ["--model", "point_mass", "--hidden", "256", "--rounds", "2", "--samples", "128", "--horizon", "8", "--steps", "12", "--epochs", "3"]
    _, _, figures = learn_loop.main(argv + ["--kfold", "3", "--lrs", "1e-3,1e-2"])
    out = capsys.readouterr().out.splitlines()
    tables = [l for l in out if "3-fold held-out loss" in l]
    assert len(tables) == 2 and len(out) == 4 and all("-> lr 0.01" in l or "-> lr 0.001" in l for l in tables)
    assert np.isfinite(np.array([f[:5] for f in figures])).all()
