"""Trajectory validation of a learner batch on the GPU (csrc/mppi_learner_rollout.hip: k_lb_rollout; mppi_learner_batch_rollout,
LearnerBatch.rollout, LearnerBase.validate_fold, k_fold_validation(val=...)). Two references, both bit for bit: the lone handle holding a
member's weights (Handle.model_rollout: the reference-ordered kernels, one launch per step) and the numpy float32 restatement of the same
plain-order step (learner_rollout_util.py). The squared-error sums are held to fp64 over the returned trajectories by a derived bound."""
import ctypes as C

import numpy as np
import pytest

import learner_rollout_util as U
from model_rollout_util import learned_inputs, learned_kw

pytestmark = pytest.mark.gpu
F32 = np.float32
KINDS = {"mlp": U.MLP, "nnauv": U.NN_AUV, "nnauv_speed": U.NN_AUV_SPEED}
NET_KEY = {"mlp": "mlp", "nnauv": "nnauv", "nnauv_speed": "nnauv_speed"}


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


# ---- 1. members equal their lone handles ---------------------------------------------------------------------------------------------
def member_nets(kind):
    """three networks of the shape of learned_kw(kind)'s, different weights, and that handle's normalisation"""
    from episode_util import make_nnauv
    kw = learned_kw(kind)
    base = kw[NET_KEY[kind]]
    n_in, n_out = base["W"][0].shape[0], base["W"][-1].shape[1]
    hid = base["W"][0].shape[1]
    nets = [dict(W=base["W"], b=base["b"])]
    for seed in (11, 12):
        w = make_nnauv(seed, hid, len(base["W"]) - 1, n_in=n_in, n_out=n_out)
        nets.append(dict(W=w["W"], b=w["b"]))
    norm = {k: base[k] for k in ("xmean", "xstd", "ymean", "ystd")}
    return kw, nets, norm


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_members_equal_their_lone_handles(m, kind):
    kw, nets, norm = member_nets(kind)
    handles = [m.Handle(**dict(kw, **{NET_KEY[kind]: dict(net, **norm)})) for net in nets]
    lb = m.LearnerBatch(nets[0], 3)
    for i, net in enumerate(nets):
        lb.set_weights(net, member=i)
    desc = dict(kind=KINDS[kind], s_dim=handles[0].s, a_dim=handles[0].a, dt=kw["dt"], **norm)
    for n in (1, 63, 64, 65, 129):
        for T in (1, 2, 7):
            x0, V = learned_inputs(kind, n, T)
            for kx in (1, n):
                start = x0[0] if kx == 1 else x0
                X = lb.rollout(desc, start, V, trajectories=True)["X"]
                assert X.shape == (3, T + 1, n, handles[0].s)
                for i, h in enumerate(handles):
                    ref = h.model_rollout(start, V, costs=False)[0]
                    assert np.isfinite(ref).all()
                    np.testing.assert_array_equal(X[i], ref, err_msg="%s member %d n %d T %d kx %d" % (kind, i, n, T, kx))
                assert not np.array_equal(X[0, 1:], X[1, 1:]) and not np.array_equal(X[1, 1:], X[2, 1:])
    # a model object describes itself: the same bits through NNAUVModel / NNAUVModelSpeed / NNPointMassModel
    obj = {"mlp": lambda: m.NNPointMassModel(stateDim=4, actionDim=2, hidden=(32,), weights=nets[0], dt=kw["dt"]),
           "nnauv": lambda: m.NNAUVModel(weights=nets[0], dt=kw["dt"]), "nnauv_speed": lambda: m.NNAUVModelSpeed(weights=nets[0], dt=kw["dt"])}[kind]()
    obj.set_Xmean_Xstd(norm["xmean"], norm["xstd"])
    obj.set_Ymean_Ystd(norm["ymean"], norm["ystd"])
    x0, V = learned_inputs(kind, 65, 2)
    np.testing.assert_array_equal(lb.rollout(obj, x0, V, trajectories=True)["X"], lb.rollout(desc, x0, V, trajectories=True)["X"])
    for h in handles:
        h.close()
    lb.close()


# ---- 2. members equal the fp32 restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_members_equal_the_fp32_restatement(m, name):
    c = U.case(name)
    lb = U.batch_of(m, c)
    for n, T, shared in ((65, 7, False), (129, 2, False), (1, 1, True), (64, 3, True)):
        x0, V = U.inputs(c["kind"], n, T)
        start = x0[0] if shared else x0
        X = lb.rollout(U.model_desc(c), start, V, trajectories=True)["X"]
        for i, net in enumerate(c["nets"]):
            np.testing.assert_array_equal(X[i], U.rollout(c["kind"], net, c["norm"], start, V), err_msg="%s member %d n %d T %d" % (name, i, n, T))
    lb.close()


# ---- 3. the squared-error sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_sse_against_fp64(m, name, capsys):
    """sse[m, j] against the sum of (X - G)^2 in float64 over the RETURNED fp32 trajectories: relative error <= (T + 16) * 2^-23.
    The derivation, with u = 2^-24 (the unit roundoff of fp32): every term is non-negative, so the relative errors of the partial sums
    never amplify — a sum of non-negative terms computed with d roundings on the path of a term is off by at most (1 + u)^d - 1 relative.
      * a term e * e: the difference X - G of two fp32 numbers is rounded once (relative u on e, 2u on e^2) and the square once: 3u.
      * the lane's sum: T + 1 serial fp32 additions (row 0, then the T steps): (T + 1) u on the oldest term.
      * the 64 lanes: a fixed butterfly of 6 levels, one addition each: 6u.
      * the blocks of 64 trajectories: added in float64, then the division by nothing: < u in all.
    (3 + T + 1 + 6 + 1) u = (T + 11) u to first order; (T + 16) * 2^-23 = 2 (T + 16) u leaves the second-order terms and a factor of
    almost two. n = 129: three blocks, the last one with a single live lane."""
    c, x0, V, G = U.sse_case(name)
    lb = U.batch_of(m, c)
    out = lb.rollout(U.model_desc(c), x0, V, gt=G, trajectories=True)
    ref = U.sse64(out["X"], G)
    assert out["sse"].dtype == np.float64 and out["sse"].shape == ref.shape == (3, c["s"])
    rel = np.abs(out["sse"] - ref) / ref
    with capsys.disabled():
        print("\n%s: largest relative distance of sse to fp64 %.3g (bound %.3g)" % (name, rel.max(), U.sse_bar(U.T_SSE)))
    assert (rel <= U.sse_bar(U.T_SSE)).all(), rel.max()
    np.testing.assert_array_equal(lb.rollout(U.model_desc(c), x0, V, gt=G)["sse"], out["sse"])  # the same sums without the trajectories
    for i in range(3):  # a member judged against itself
        own = lb.rollout(U.model_desc(c), x0, V, gt=out["X"][i])["sse"]
        assert (own[i] == 0.0).all() and (own[(i + 1) % 3] > 0.0).all()
    lb.close()


# ---- 4. isolation and determinism ----------------------------------------------------------------------------------------------------------
def test_isolation_and_determinism(m):
    c, x0, V, G = U.sse_case("nnauv_16_32_32_32_13")
    desc = U.model_desc(c)
    rng = np.random.default_rng(3)
    Xd, Yd = rng.standard_normal((40, 16)).astype(F32), rng.standard_normal((40, 13)).astype(F32)
    lb, quiet = U.batch_of(m, c), U.batch_of(m, c)  # `quiet` never rolls out
    for b in (lb, quiet):
        b.set_data(Xd, Yd)
        b.train(2, 1e-3)
    w_before = [lb.get_weights(i) for i in range(3)]
    a = lb.rollout(desc, x0, V, gt=G, trajectories=True)
    b = lb.rollout(desc, x0, V, gt=G, trajectories=True)
    np.testing.assert_array_equal(a["X"], b["X"])
    np.testing.assert_array_equal(a["sse"], b["sse"])
    assert np.isfinite(a["sse"]).all()
    # member 1 overflows: its own sums are not finite, its neighbours' bits stay
    huge = dict(W=[np.full_like(w, 1e30) for w in c["nets"][1]["W"]], b=[np.full_like(v, 1e30) for v in c["nets"][1]["b"]])
    lb.set_weights(huge, member=1)
    d = lb.rollout(desc, x0, V, gt=G, trajectories=True)
    assert not np.isfinite(d["sse"][1]).any()
    for i in (0, 2):
        np.testing.assert_array_equal(d["sse"][i], a["sse"][i])
        np.testing.assert_array_equal(d["X"][i], a["X"][i])
    lb.set_weights(w_before[1], member=1)
    # nothing of the batch moved: weights, step count, and the next training step
    assert lb.step_count() == quiet.step_count() == 2
    for i in range(3):
        for key in ("W", "b"):
            for got, ref in zip(lb.get_weights(i)[key], quiet.get_weights(i)[key]):
                np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(lb.train(1, 1e-3)[0], quiet.train(1, 1e-3)[0])
    for i in range(3):
        for got, ref in zip(lb.get_weights(i)["W"], quiet.get_weights(i)["W"]):
            np.testing.assert_array_equal(got, ref)
    lb.close()
    quiet.close()


def test_1024_members(m):
    c = U.case("mlp_6_7_5_4")
    nets = {0: c["nets"][1], 511: c["nets"][2], 1023: c["truth"]}
    lb = m.LearnerBatch(c["nets"][0], 1024)
    for i, net in nets.items():
        lb.set_weights(net, member=i)
    x0, V = U.inputs(c["kind"], 1, 2)
    G = U.ground_truth(c, x0, V)
    out = lb.rollout(U.model_desc(c), x0, V, gt=G, trajectories=True)
    assert out["X"].shape == (1024, 3, 1, 4) and out["sse"].shape == (1024, 4)
    default = U.rollout(c["kind"], c["nets"][0], c["norm"], x0, V)
    for i in (1, 510, 512, 1022):
        np.testing.assert_array_equal(out["X"][i], default)
    for i, net in nets.items():
        ref = U.rollout(c["kind"], net, c["norm"], x0, V)
        np.testing.assert_array_equal(out["X"][i], ref)
        assert not np.array_equal(ref, default)
    lb.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_usable(m):
    from mppi_tf_amd import _lib
    c = U.case("mlp_6_7_5_4")
    lb = U.batch_of(m, c)
    n, T = 5, 3
    x0, V = U.inputs(c["kind"], n, T)
    G = U.ground_truth(c, x0, V)
    X = np.zeros((3, T + 1, n, 4), F32)
    sse = np.zeros((3, 4), np.float64)
    fp, dp = _lib.fp, lambda a: a.ctypes.data_as(_lib.DP)

    def desc(kind=U.MLP, s=4, a=2, xstd=None):
        held = None if xstd is None else np.ascontiguousarray(xstd, F32)
        return _lib.LearnerModel(kind, s, a, 0.1, None, fp(held), None, None), held

    def call(model, x0_=x0, kx=n, V_=V, G_=G, n_=n, T_=T, sse_=sse, X_=X):
        st = lb.lib.mppi_learner_batch_rollout(lb.h, C.byref(model[0]) if model is not None else None, fp(x0_), kx, fp(V_), fp(G_), n_, T_,
                                               dp(sse_) if sse_ is not None else None, fp(X_))
        return st, (lb.lib.mppi_learner_batch_last_error(lb.h) or b"").decode()

    ok = desc()
    assert call(ok)[0] == 0
    bad_std = np.ones(6, F32)
    bad_std[4] = 0.0
    refused = [
        (call(None), 1, "NULL pointer"), (call(ok, x0_=None), 1, "NULL pointer"), (call(ok, V_=None), 1, "NULL pointer"),
        (call(ok, sse_=None, X_=None), 1, "both NULL"), (call(ok, G_=None), 1, "needs the ground truth"),
        (call(ok, n_=0, kx=0), 1, "n and T must be >= 1"), (call(ok, T_=0), 1, "n and T must be >= 1"),
        (call(ok, n_=1 << 16, kx=1, T_=(1 << 14) + 1), 1, "2^30"), (call(ok, kx=2), 1, "kx in {1, n}"),
        (call(desc(kind=0)), 4, "model_kind"), (call(desc(kind=2)), 4, "model_kind"), (call(desc(kind=5)), 4, "model_kind"),
        (call(desc(U.NN_AUV, 13, 6)), 4, "16 -> 13"), (call(desc(U.NN_AUV_SPEED, 13, 6)), 4, "15 -> 6"),
        (call(desc(U.MLP, 6, 3)), 4, "s_dim = 2 a_dim"), (call(desc(U.MLP, 5, 1)), 4, "s_dim = 2 a_dim"), (call(desc(U.MLP, 10, 5)), 4, "a_dim <= 4"),
        (call(desc(U.NN_AUV, 4, 2)), 4, "s_dim = 13"),
        (call(desc(xstd=bad_std)), 1, "xstd[4] is 0"),
    ]
    for (st, msg), want, text in refused:
        assert st == want and "mppi_learner_batch_rollout" in msg and text in msg, (st, want, msg)
    # the Python wrapper checks shapes before the library
    for args in ((x0, V[:, :, :1]), (x0[:3], V), (x0[:, :3], V)):
        with pytest.raises(ValueError):
            lb.rollout(U.model_desc(c), *args, trajectories=True)
    with pytest.raises(ValueError):
        lb.rollout(U.model_desc(c), x0, V)
    with pytest.raises(ValueError):
        lb.rollout(U.model_desc(c), x0, V, gt=G[:-1])
    # ... and the batch still rolls out and trains
    np.testing.assert_array_equal(lb.rollout(U.model_desc(c), x0, V, trajectories=True)["X"][2], U.rollout(c["kind"], c["nets"][2], c["norm"], x0, V))
    rng = np.random.default_rng(1)
    lb.set_data(rng.standard_normal((20, 6)).astype(F32), rng.standard_normal((20, 4)).astype(F32))
    assert np.isfinite(lb.train(2, 1e-3)[0]).all() and lb.step_count() == 2
    lb.close()


# ---- 6. k-fold validation with trajectories ---------------------------------------------------------------------------------------------
def held_out_trajectories(m, kv=4, tau=5):
    """val = (gtTrajs [kv, tau, 13], actionSeqs [kv, tau, 6]) of the Fossen plant"""
    from conftest import load_golden
    from learner_batch_util import fossen_transitions
    plant = m.AUVModel(actionDim=6, dt=0.1, parameters=load_golden("model_auv")["params"])
    x = fossen_transitions(m, kv, seed=9)[0]
    act = 100.0 * np.random.default_rng(4).standard_normal((kv, tau, 6))
    gt = [x]
    for t in range(tau - 1):
        gt.append(np.asarray(plant.build_step_graph("plant", gt[-1], act[:, t][..., None]), np.float64))
    return np.stack(gt, axis=1)[..., 0], act


def test_k_fold_validation_with_trajectories(m):
    from learner_batch_util import fossen_transitions
    n, k, rates, epoch = 264, 3, (1e-3, 1e-2), 12
    x, u, xn = fossen_transitions(m, n)
    model = m.NNAUVModel()
    learner = m.LearnerBase(model, bufferSize=n)
    learner.add_rb(x, u, xn)
    learner.stats()
    val = held_out_trajectories(m)
    w0 = model.get_weights()
    seen = []
    log = learner.k_fold_validation(k=k, learningRate=rates, epoch=epoch, seed=3, val=val, writer=lambda e, d: seen.append((e, sorted(d))))
    assert log["val"].shape == (2, 2, k) and log["val"].dtype == np.float64 and np.isfinite(log["val"]).all() and (log["val"] > 0).all()
    assert seen == [(e, ["test", "train", "val"] if e % 10 == 0 else ["test", "train"]) for e in range(epoch)]
    plain = learner.k_fold_validation(k=k, learningRate=rates, epoch=epoch, seed=3)
    assert "val" not in plain
    np.testing.assert_array_equal(log["train"], plain["train"])
    np.testing.assert_array_equal(log["test"], plain["test"])
    # the validations again, by hand: fresh batches trained 1 and 11 steps in one call each
    X, y = model.prepare_training_data(x, xn, u)
    folds = m.kfold_indices(n, k, 3)
    for j, steps in enumerate((1, 11)):
        lb = m.LearnerBatch(dict(W=w0[0::2], b=w0[1::2]), 2 * k)
        lb.set_data(X, y)
        for r in range(2):
            for f, (tr, te) in enumerate(folds):
                lb.set_split(r * k + f, tr, te)
        lb.train(steps, np.repeat(np.array(rates, F32), k))
        err, split = learner.validate_fold(lb, val, split=True)
        np.testing.assert_array_equal(err.reshape(2, k), log["val"][j])
        assert split.shape == (2 * k, 13)
        np.testing.assert_allclose(split.mean(axis=1), err, rtol=1e-12)
        # the host path: a model holding the member's weights, rolled step by step and summed in fp64 (LearnerBase.validate)
        for i in range(2 * k):
            w = lb.get_weights(i)
            member = m.NNAUVModel(weights=w)
            member.set_Xmean_Xstd(model.Xmean, model.Xstd)
            member.set_Ymean_Ystd(model.Ymean, model.Ystd)
            host, host_split = learner.validate(member, val[1], val[0], split=True)
            np.testing.assert_allclose(err[i], host, rtol=1e-5)
            np.testing.assert_allclose(split[i], host_split, rtol=1e-5)
        lb.close()
    best, table = learner.grid_search(rates, k=k, epoch=epoch, seed=3, val=val, by="val")
    np.testing.assert_array_equal(table, log["val"][-1].mean(axis=1))
    assert table.shape == (2,) and best == rates[int(np.argmin(table))]
    best_t, table_t = learner.grid_search(rates, k=k, epoch=epoch, seed=3, val=val)  # the default ranks by the held-out loss
    np.testing.assert_array_equal(table_t, log["test"][-1].astype(np.float64).mean(axis=1))
    for a, b in zip(model.get_weights(), w0):  # the reference trains copies
        np.testing.assert_array_equal(a, b)


def test_learn_loop_chooses_its_rate_by_h_step_error(m, capsys):
    """examples/learn_loop.py --kfold K --lrs a,b --kfold-val: a second line per round with the H-step table, whose argmin trains the round"""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import learn_loop
    finally:
        sys.path.pop(0)
    argv = ["--rounds", "2", "--samples", "128", "--horizon", "8", "--steps", "12", "--epochs", "3", "--hidden", "16", "--layers", "1", "--kfold", "3",
            "--lrs", "1e-3,1e-2"]
    _, _, figures = learn_loop.main(argv + ["--kfold-val"])
    out = capsys.readouterr().out.splitlines()
    lines = [l for l in out if "3-fold H-step open-loop squared error (H = 8, 5 windows)" in l]
    assert len(lines) == 2 and len(out) == 6
    for l in lines:
        table = [float(p.split(": ")[1]) for p in l.split("by learning rate: ")[1].split(" -> lr ")[0].split(", ")]
        chosen = float(l.split(" -> lr ")[1])
        assert len(table) == 2 and np.isfinite(table).all() and chosen == (1e-3, 1e-2)[int(np.argmin(table))]
    held = [l for l in out if "3-fold held-out loss" in l]
    assert len(held) == 2 and [l.split(" -> lr ")[1] for l in held] == [l.split(" -> lr ")[1] for l in lines]
    assert np.isfinite(np.array([f[:5] for f in figures])).all()
    learn_loop.main(argv)
    assert len(capsys.readouterr().out.splitlines()) == 4  # without the flag: the held-out table and the round's line
