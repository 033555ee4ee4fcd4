"""The learner edge matrix on the GPU (csrc/mppi_learner.hip, mppi_learner_wide.hip, mppi_learner_batch.hip): every learner kernel against
fp64 numpy at the sample counts and shapes where its structures begin and end (tests/learner_edges_util.py; shown fit to judge a kernel by
tests/test_learner_edges_oracle.py). The bars are the suite's: loss 2e-6 relative; gradients rtol 2e-5, atol 2e-6 max|g| per tensor; one
Adam step from the device's own state 3e-7; the moments 4 ulp. One bar is measured per case: a prediction is within 4 x the distance of
torch CPU fp32's forward pass from fp64, at least 1e-6 max|pred|. Everything about reuse and the batch is bit for bit.

Largest distances measured on the MI355X, in bars: narrow loss 0.10, gradients 0.08, predictions 0.35; wide loss 0.05, gradients 0.27,
predictions 0.62; dead-unit gradients 0.07; one Adam step 0.20 (narrow) and 0.21 (wide); second moment 0.25 and 0.5 (1 and 2 ulp).
The first moment is 0 ulp from fp64: it missed its 4 ulp for beta1 = 0.9 and 0.95 (46 ulp narrow, 18 700 ulp wide, where b1 m and (1 - b1) g
cancel in an fp32 sum) until the three Adam kernels formed it in fp64 (adam_first_moment, csrc/mppi_learner.hip.h).
"""
import numpy as np
import pytest

import learner_batch_util as U
import learner_edges_util as E
from learner_util import F32, data, grad_bar, make_net, numpy_loss_and_grads64

pytestmark = pytest.mark.gpu
ENTERED = set()  # the case ids that ran
SEEN = {}        # bar -> the largest distance observed, in bars


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


def see(bar, value):
    SEEN[bar] = max(SEEN.get(bar, 0.0), float(value))
    return float(value)


def gradients_in_bars(family, g, ref, missed, tag):
    for (name, got), (_, g64) in zip(E.tensors(g), E.tensors(ref)):
        assert got.shape == g64.shape, (tag, name, got.shape)
        r = see("%s gradient / (rtol 2e-5, atol 2e-6 max|g|)" % family, (np.abs(got - g64) / grad_bar(g64)).max())
        if not r <= 1.0:
            missed.append("%s d%s: %.3g bars" % (tag, name, r))


def same_bits(a, b):
    for (name, u), (_, v) in zip(E.tensors(a), E.tensors(b)):
        np.testing.assert_array_equal(u, v, err_msg=name)


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c["id"])
def test_gradients_and_predictions_against_fp64(m, case):
    net, X, Y = E.inputs(case)
    ref, fam, dims, n = E.reference(case), case["family"], case["dims"], case["n"]
    lr = m.Learner(net)
    lr.set_data(X, Y)
    loss, g, pred = lr.evaluate(grads=True, pred=True)
    loss_e, pred_e = lr.evaluate(pred=True)
    lr.close()
    assert loss_e == loss
    np.testing.assert_array_equal(pred_e, pred)
    missed = []
    r = see("%s loss / 2e-6 relative" % fam, abs(loss - ref["loss"]) / (E.LOSS_RTOL * ref["loss"]))
    if not r <= 1.0:
        missed.append("loss %.9g, fp64 %.9g: %.3g bars" % (loss, ref["loss"], r))
    for l in range(len(dims) - 1):
        assert g["W"][l].shape == (dims[l], dims[l + 1]) and g["b"][l].shape == (dims[l + 1],)
    gradients_in_bars(fam, g, ref, missed, case["id"])
    assert pred.shape == (n, dims[-1]) and pred.dtype == F32
    p = see("%s prediction / (4 x torch fp32's distance, floor 1e-6 max|pred|)" % fam, np.abs(pred - ref["pred"]).max() / E.pred_bar(case))
    if not p <= 1.0:
        missed.append("predictions: %.3g bars of %.3g" % (p, E.pred_bar(case)))
    print("%s: loss %.3f bars, predictions %.3f bars" % (case["id"], r, p))
    ENTERED.add(case["id"])
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("case", E.DEAD_CASES, ids=lambda c: c["id"])
def test_dead_and_zero_units(m, case):
    net, X, Y = E.dead_inputs(case)
    _, gW, gb = numpy_loss_and_grads64(net, X, Y)
    lr = m.Learner(net)
    lr.set_data(X, Y)
    _, g = lr.evaluate(grads=True)
    for unit in (E.DEAD_UNIT, E.ZERO_UNIT):
        for e in E.unit_entries(g, unit):
            assert np.all(e == 0.0), (unit, e)
    missed = []
    gradients_in_bars("dead-unit", g, dict(W=gW, b=gb), missed, case["id"])
    lr.train(3, E.LR)
    w = lr.get_weights()
    lr.close()
    for unit in (E.DEAD_UNIT, E.ZERO_UNIT):
        for got, start in zip(E.unit_entries(w, unit), E.unit_entries(net, unit)):
            np.testing.assert_array_equal(got, start)
    assert any(not np.array_equal(u, v) for (_, u), (_, v) in zip(E.tensors(w), E.tensors(net)))  # the rest did move
    ENTERED.add(case["id"])
    assert not missed, "\n".join(missed)


def one_step_from_the_devices_state(lrn, tmp_path, t, lr, hp, fam):
    """save, gradients, one step, save: w' within the update bar of adam_step64 on the saved (w, m, v), the device's g and t; m', v'
    within 4 ulp of the fp64 ones rounded to fp32; the files' steps t - 1 and t"""
    before, after = str(tmp_path / ("before%d" % t)), str(tmp_path / ("after%d" % t))
    lrn.save(before)
    _, g = lrn.evaluate(grads=True)
    lrn.train(1, lr, *hp)
    lrn.save(after)
    s0, s1 = E.read_learner_file(before), E.read_learner_file(after)
    assert (s0["step"], s1["step"]) == (t - 1, t) and lrn.step_count() == t
    missed, missed_m = [], []
    for k, mk, vk in (("W", "mW", "vW"), ("b", "mb", "vb")):
        for l in range(len(s0["W"])):
            w64, m64, v64 = E.adam_step64(s0[k][l], s0[mk][l], s0[vk][l], g[k][l], t, lr, *hp)
            assert np.isfinite(s1[k][l]).all() and np.isfinite(w64).all()
            figures = (see("%s Adam step / 3e-7" % fam, E.distance(s1[k][l], w64) / E.UPDATE_BAR),
                       see("%s first moment / 4 ulp" % fam, E.ulps(s1[mk][l], m64.astype(F32)).max() / 4.0),
                       see("%s second moment / 4 ulp" % fam, E.ulps(s1[vk][l], v64.astype(F32)).max() / 4.0))
            if not max(figures[0], figures[2]) <= 1.0:
                missed.append("t = %d, %s%d: w' %.3g, v' %.3g bars" % (t, k, l, figures[0], figures[2]))
            if not figures[1] <= 1.0:
                missed_m.append("t = %d, %s%d: m' %.3g bars (%d ulp)" % (t, k, l, figures[1], 4 * figures[1]))
    return missed, missed_m


ADAM_RUNS = {}  # (family, HP set) -> what one_step_from_the_devices_state missed: (w', v' and the steps; m')


def adam_run(m, tmp_path, fam, hp):
    if (fam, hp) in ADAM_RUNS:
        return ADAM_RUNS[fam, hp]
    key = (fam, hp)
    dims = E.ADAM_DIMS[fam]
    X, Y = data(dims, E.ADAM_N, 32)
    lrn = m.Learner(make_net(dims, 31))
    lrn.set_data(X, Y)
    (lr,), hp = E.as_fp32((E.LR,)), E.as_fp32(hp)
    missed, missed_m = [], []
    for t in E.ADAM_T:
        if lrn.step_count() < t - 1:
            lrn.train(t - 1 - lrn.step_count(), lr, *hp)
        a, b = one_step_from_the_devices_state(lrn, tmp_path, t, lr, hp, fam)
        missed, missed_m = missed + a, missed_m + b
    # step 100 000: powf of the betas underflows to 0 there
    lrn.save(str(tmp_path / "at10"))
    E.rewrite_step(str(tmp_path / "at10"), str(tmp_path / "late"), 99999)
    lrn.load(str(tmp_path / "late"))
    assert lrn.step_count() == 99999
    a, b = one_step_from_the_devices_state(lrn, tmp_path, 100000, lr, hp, fam)
    lrn.close()
    ADAM_RUNS[key] = (missed + a, missed_m + b)
    return ADAM_RUNS[key]


HP_IDS = lambda hp: "b1=%g-b2=%g-eps=%g" % hp


@pytest.mark.parametrize("hp", E.HP_SETS, ids=HP_IDS)
@pytest.mark.parametrize("fam", ["narrow", "wide"])
def test_the_adam_rule_from_the_devices_own_state(m, tmp_path, fam, hp):
    """w' within 3e-7 of the Keras rule in fp64 on the device's own (w, m, v, g, t), v' within 4 ulp, the files' steps; t = 1, 2, 3, 10
    and 100 000"""
    missed, _ = adam_run(m, tmp_path, fam, hp)
    ENTERED.add("adam-%s-%s" % (fam, hp))
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("hp", E.HP_SETS, ids=HP_IDS)
@pytest.mark.parametrize("fam", ["narrow", "wide"])
def test_the_first_moment_within_4_ulp(m, tmp_path, fam, hp):
    """m' within 4 ulp of the fp64 value rounded to fp32, of the same runs: where b1 m and (1 - b1) g cancel, a sum of two fp32-rounded
    terms is wrong by ulps of the TERMS (it was up to 18 700 ulp of m' on the wide learner); the kernels form it in fp64"""
    _, missed_m = adam_run(m, tmp_path, fam, hp)
    assert not missed_m, "\n".join(missed_m)


def test_hyper_parameters_through_the_batch(m):
    """18 members, n_train = N_NARROW, every HP set: each member bit for bit its lone learner (held to the Keras rule by the test above)"""
    dims, n, B = [16, 32, 32, 32, 13], 1100, len(E.N_NARROW)
    X, Y = U.pool(dims, n, 61)
    rng = np.random.default_rng(62)
    train = [rng.permutation(n)[:nt] for nt in E.N_NARROW]
    test = [rng.permutation(n)[:(0, 1, 255, 256, 257)[i % 5]] for i in range(B)]
    assert all(np.any(np.diff(t) < 0) for t in train if len(t) > 2)
    hp = [E.HP_SETS[i % len(E.HP_SETS)] for i in range(B)]
    case = dict(net=make_net(dims, 60), X=X, Y=Y, train=train, test=test, lr=[E.LR] * B, hp=hp, calls=(1, 2))
    got = U.run_batch(m, case)
    assert got["steps"] == 3
    U.check_members_against_lone(m, case["net"], X, Y, train, test, case["lr"], hp, case["calls"], got)
    ENTERED.add("batch-hp")


@pytest.mark.parametrize("fam,sizes", [("narrow", (1025, 3, 513)), ("wide", (1025, 1, 65))])
def test_set_data_reuses_buffers_without_a_trace(m, tmp_path, fam, sizes):
    """smaller data after larger data on one learner: loss, gradients, predictions and two Adam steps equal, bit for bit, a fresh learner
    loaded from the first one's file and given only the new data"""
    dims = list(E.FAMILY[fam]["dims"][-1])
    a = m.Learner(make_net(dims, 71))
    for i, n in enumerate(sizes):
        X, Y = data(dims, n, 72 + i)
        a.set_data(X, Y)
        path = str(tmp_path / ("state%d" % i))
        a.save(path)
        f, _ = m.Learner.from_file(path)
        f.set_data(X, Y)
        (la, ga, pa), (lf, gf, pf) = a.evaluate(grads=True, pred=True), f.evaluate(grads=True, pred=True)
        assert la == lf and pa.shape == (n, dims[-1])
        same_bits(ga, gf)
        np.testing.assert_array_equal(pa, pf)
        assert a.train(2, E.LR) == f.train(2, E.LR)
        same_bits(a.get_weights(), f.get_weights())
        assert a.step_count() == f.step_count() == 2 * (i + 1)
        f.close()
    a.close()
    ENTERED.add("reuse-" + fam)


def test_set_split_reuses_buffers_without_a_trace(m):
    """member 0 re-split from 1025 rows to 3 while member 1 keeps 513; then member 1 down to 2 rows (the capacity shrinks): after each,
    both members equal lone learners started from their weights"""
    dims, n = [16, 32, 32, 32, 13], 1100
    X, Y = U.pool(dims, n, 81)
    net = make_net(dims, 80)
    rng = np.random.default_rng(82)
    train, test = [rng.permutation(n)[:1025], rng.permutation(n)[:513]], [rng.permutation(n)[:5], np.zeros(0, np.int64)]
    lb = m.LearnerBatch(net, 2)
    lb.set_data(X, Y)
    for mi in range(2):
        lb.set_split(mi, train[mi], test[mi])
    start = [net, net]
    for stage, change in enumerate((None, (0, 3), (1, 2))):
        if change is not None:
            mi, rows = change
            train[mi] = rng.permutation(n)[:rows]
            lb.set_split(mi, train[mi], test[mi])
            lb.reset_optimizer()
        lt, ls = lb.train(2, E.LR)
        for mi in range(2):
            ref = U.lone_history(m, net, X, Y, train[mi], test[mi], E.LR, E.DEFAULT_HP, 2, start=start[mi])
            np.testing.assert_array_equal(lt[:, mi], np.array(ref["loss_train"], F32), err_msg="stage %d member %d" % (stage, mi))
            np.testing.assert_array_equal(ls[:, mi], np.array(ref["loss_test"], F32), err_msg="stage %d member %d" % (stage, mi))
            start[mi] = lb.get_weights(mi)
            U.same_weights(start[mi], ref["weights"][-1])
    lb.close()
    ENTERED.add("reuse-batch")


def test_1024_members(m):
    dims, n, B = [4, 8, 2], 8, 1024
    X, Y = U.pool(dims, n, 91)
    net = make_net(dims, 90)
    rng = np.random.default_rng(92)
    lists = [rng.permutation(n)[:3] for _ in range(4)]
    assert len({tuple(l) for l in lists}) == 4
    lb = m.LearnerBatch(net, B)
    lb.set_data(X, Y)
    for mi in range(B):
        lb.set_split(mi, lists[mi % 4])
    lt, ls = lb.train(2, E.LR)
    assert lb.step_count() == 2 and lt.shape == (2, B) and np.isnan(ls).all()
    weights = [lb.get_weights(mi) for mi in range(B)]
    lb.close()
    for mi in range(4, B):  # members with the same list
        np.testing.assert_array_equal(lt[:, mi], lt[:, mi % 4])
        U.same_weights(weights[mi], weights[mi % 4])
    for mi in (0, 1, 511, 1023):
        ref = U.lone_history(m, net, X, Y, lists[mi % 4], np.zeros(0, np.int64), E.LR, E.DEFAULT_HP, 2)
        np.testing.assert_array_equal(lt[:, mi], np.array(ref["loss_train"], F32))
        U.same_weights(weights[mi], ref["weights"][-1])
    ENTERED.add("1024-members")


def test_every_case_of_the_matrix_was_entered():
    print("largest distances observed, in bars:")
    for bar in sorted(SEEN):
        print("  %-75s %.3g" % (bar, SEEN[bar]))
    every = {c["id"] for c in E.CASES + list(E.DEAD_CASES)}
    if {"1024-members", "batch-hp", "reuse-batch"} <= ENTERED:  # (a run of part of this file has entered part of the set)
        assert every <= ENTERED, sorted(every - ENTERED)
