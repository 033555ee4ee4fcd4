"""The learner edge matrix on the CPU: every case of tests/learner_edges_util.py is shown fit to judge a kernel before a GPU sees it.
fp64 numpy is the reference, torch CPU fp32 the stand-in for a correct fp32 kernel.

(a) torch fp32's loss and gradients are within a quarter of the suite's bars (loss 2e-6 relative; rtol 2e-5 and atol 2e-6 max|g| per
    tensor) of the fp64 ones on every case: the bars test a kernel, not the conditioning of the case.
(b) a gradient that loses one probe row (the first, the last, either side of every unit boundary) moves by at least 100 x its bar in
    some entry of every tensor.
(c) every wrong Adam rule of ALTERNATIVES moves a weight by at least 100 x the update bar (3e-7) away from the Keras rule, and the fp32
    restatement of the Keras rule stays within a quarter of that bar of fp64.
(d) the dead-unit networks: gradients into and out of the dead and the zero unit are exactly 0, every other unit's are not.
(e) the matrix holds every n and every shape it claims, nothing above 1025 rows.

Measured here: (a) torch fp32 within the asserted quarter of a bar on the 56 narrow cases and at most 0.20 on the 38 wide ones; (b) a dropped probe row at least 163 bars (narrow)
and 301 bars (wide) in every tensor; (c) the fp32 restatement at most 0.20 of the update bar with the hyper-parameters rounded to fp32 as
the device receives them (0.10 for the two sets with a large eps), every wrong rule at least 642 bars away at (0.5, 0.9, 1e-2) at every
t of 1, 2, 3, 10. Seeds other than the default (SEEDS) were chosen for eight cases that missed (a) or (b); the one-unit shapes get their
probe rows' targets enlarged, [32, 1, 32] also aligned, since one number per row carries a whole tensor there.
"""
import numpy as np
import pytest

import learner_edges_util as E
from learner_util import F32, copy_net, data, grad_bar, keras_adam, make_net, numpy_forward64, numpy_loss_and_grads64, torch_loss_and_grads

SEEN = {}


def see(key, value, worst=max):
    SEEN[key] = worst(SEEN.get(key, value), value)


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c["id"])
def test_fp32_meets_a_quarter_of_the_bars(case):
    net, X, Y = E.inputs(case)
    ref = E.reference(case)
    tl, tW, tb = torch_loss_and_grads(net, X, Y)
    r = abs(tl - ref["loss"]) / (E.LOSS_RTOL * ref["loss"])
    worst = [("loss", r)]
    for (name, g32), (_, g64) in zip(E.tensors(dict(W=tW, b=tb)), E.tensors(ref)):
        assert g32.shape == g64.shape
        worst.append((name, float((np.abs(g32 - g64) / grad_bar(g64)).max())))
    print("%s: torch fp32 against fp64, in bars: %s" % (case["id"], "  ".join("%s %.3f" % w for w in worst)))
    see("(a) fp32 / bar, " + case["family"], max(w[1] for w in worst))
    assert all(w[1] <= 0.25 for w in worst), worst


@pytest.mark.parametrize("case", E.CASES, ids=lambda c: c["id"])
def test_a_dropped_probe_row_is_far_outside_the_bars(case):
    ref = E.reference(case)
    low = []
    for row in E.probe_rows(case["family"], case["n"]):
        cW, cb = E.row_contribution(case, row)
        for (name, c), (_, g64) in zip(E.tensors(dict(W=cW, b=cb)), E.tensors(ref)):
            low.append((float((np.abs(c) / grad_bar(g64)).max()), row, name))
    print("%s: a dropped probe row moves a tensor by at least %.0f bars (row %d, %s)" % ((case["id"],) + min(low)))
    see("(b) dropped row / bar, " + case["family"], min(low)[0], min)
    assert min(low)[0] >= 100.0, sorted(low)[:5]


def test_probe_rows():
    assert E.probe_rows("narrow", 1) == [0] and E.probe_rows("narrow", 2) == [0, 1] and E.probe_rows("narrow", 3) == [0, 1, 2]
    assert E.probe_rows("narrow", 513) == [0, 1, 2, 7, 8, 63, 64, 255, 256, 511, 512]
    assert E.probe_rows("narrow", 512) == [0, 1, 2, 7, 8, 63, 64, 255, 256, 511]
    assert E.probe_rows("wide", 65) == [0, 31, 32, 63, 64] and E.probe_rows("wide", 1025) == [0, 31, 32, 63, 64, 511, 512, 1024]
    for c in E.CASES:  # a hidden layer of one unit is live on every probe row
        net, X, _ = E.inputs(c)
        zs = numpy_forward64(net, X[E.probe_rows(c["family"], c["n"])])[1]
        for l in range(len(c["dims"]) - 2):
            if c["dims"][l + 1] == 1:
                assert zs[l].min() > 0.2, c["id"]


def flat(net_like):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in list(net_like["W"]) + list(net_like["b"])])


def adam_records(hp, steps=10):
    """ten steps on [9, 16, 6], n = 333, from fp32 state as the device holds it: per step (w, m, v, g, t, w' by the fp32 restatement)"""
    dims = E.ADAM_DIMS["narrow"]
    net = copy_net(make_net(dims, 31))
    X, Y = data(dims, E.ADAM_N, 32)
    state = dict(W=[(np.zeros_like(w), np.zeros_like(w)) for w in net["W"]], b=[(np.zeros_like(b), np.zeros_like(b)) for b in net["b"]])
    lr, hp = E.as_fp32((E.LR,))[0], E.as_fp32(hp)
    out = []
    for t in range(1, steps + 1):
        _, gW, gb = numpy_loss_and_grads64(net, X, Y)
        gW, gb = [g.astype(F32) for g in gW], [g.astype(F32) for g in gb]
        w, g = flat(net), flat(dict(W=gW, b=gb))
        m, v = (flat(dict(W=[s[q] for s in state["W"]], b=[s[q] for s in state["b"]])) for q in (0, 1))
        keras_adam(net, state, gW, gb, t, lr, *hp)
        out.append(dict(w=w, m=m, v=v, g=g, t=t, lr=lr, hp=hp, w32=flat(net)))
    return out


def test_every_wrong_adam_rule_is_far_from_the_keras_rule():
    far = {name: 0.0 for name in E.ALTERNATIVES}
    for hp in E.HP_SETS:
        for r in adam_records(hp):
            if r["t"] not in E.ADAM_T:
                continue
            args = (r["w"], r["m"], r["v"], r["g"], r["t"], r["lr"]) + r["hp"]
            w64 = E.adam_step64(*args)[0]
            assert np.isfinite(w64).all()
            own = E.distance(r["w32"], w64) / E.UPDATE_BAR
            see("(c) fp32 restatement / update bar, %s" % (hp,), own)
            line = []
            for name, rule in E.ALTERNATIVES.items():
                d = E.distance(rule(*args)[0], w64) / E.UPDATE_BAR
                far[name] = max(far[name], d)
                line.append("%s %.3g" % (name, d))
                if hp == (0.5, 0.9, 1e-2):
                    see("(c) a wrong rule / update bar at (0.5, 0.9, 1e-2)", d, min)
            print("%s t = %d: fp32 restatement %.3f bars; %s" % (hp, r["t"], own, "; ".join(line)))
            assert own <= 0.25, (hp, r["t"], own)
    print("the farthest each wrong rule gets, in update bars: %s" % far)
    assert all(d >= 100.0 for d in far.values()), far
    # (0.5, 0.9, 1e-2) alone tells every wrong rule apart at every t
    assert SEEN["(c) a wrong rule / update bar at (0.5, 0.9, 1e-2)"] >= 100.0


@pytest.mark.parametrize("case", E.DEAD_CASES, ids=lambda c: c["id"])
def test_dead_unit_networks(case):
    net, X, Y = E.dead_inputs(case)
    z0 = numpy_forward64(net, X)[1][0]
    assert np.all(z0[:, E.DEAD_UNIT] == -1.0) and np.all(z0[:, E.ZERO_UNIT] == 0.0)
    _, gW, gb = numpy_loss_and_grads64(net, X, Y)
    _, tW, tb = torch_loss_and_grads(net, X, Y)  # relu'(0) = 0 there too
    for g in (dict(W=gW, b=gb), dict(W=tW, b=tb)):
        for unit in range(case["dims"][1]):
            entries = E.unit_entries(g, unit)
            if unit in (E.DEAD_UNIT, E.ZERO_UNIT):
                assert all(np.all(e == 0.0) for e in entries), unit
            else:
                assert all(np.any(e != 0.0) for e in entries), unit


def test_the_matrix_is_what_it_claims():
    ids = [c["id"] for c in E.CASES]
    assert len(set(ids)) == len(ids)
    for family, cases in (("narrow", E.NARROW_CASES), ("wide", E.WIDE_CASES)):
        f = E.FAMILY[family]
        assert {c["n"] for c in cases} == set(f["ns"]) and max(c["n"] for c in cases) == 1025
        assert {tuple(c["dims"]) for c in cases} == {tuple(d) for d in f["dims"]}
        for n in f["ns"]:  # the family's last shape, and one other
            assert [f["dims"][-1] == c["dims"] for c in cases if c["n"] == n].count(True) == 1
            assert [f["dims"][-1] == c["dims"] for c in cases if c["n"] == n].count(False) >= 1
        for dims in f["dims"]:
            assert {c["n"] for c in cases if c["dims"] == list(dims)} >= set(f["n_of_dims"])
        assert all(c["family"] == family for c in cases)
    print("%d narrow and %d wide cases" % (len(E.NARROW_CASES), len(E.WIDE_CASES)))


def test_what_was_measured():
    for key in sorted(SEEN):
        print("  %-60s %.3g" % (key, SEEN[key]))
