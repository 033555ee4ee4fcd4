"""Trajectory validation of a WIDE learner batch on the GPU (csrc/mppi_learner_wide_rollout.hip: k_wb_rollout;
mppi_learner_wide_batch_validate, WideLearnerBatch.validate, LearnerBase.validate_fold / k_fold_trajectory_validation). Two references, both
bit for bit: the lone MPPI_MODEL_MLP handle holding a member's weights (Handle.model_rollout: k_mlp_step_ref, one launch per step) and the
numpy float32 restatement of the same plain-order step (learner_rollout_util.py). The squared-error sums are held to fp64 over the returned
trajectories by a derived bound."""
import ctypes as C

import numpy as np
import pytest

import learner_rollout_util as L
import wide_rollout_util as U

pytestmark = pytest.mark.gpu
F32 = np.float32
A_IDS = lambda a: "a%d" % a


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


# ---- 1. members equal their lone handles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", U.A_DIMS, ids=A_IDS)
def test_members_equal_their_lone_handles(m, a):
    """n around the workgroup's R = 16 trajectories (15, 16, 17), one trajectory, several blocks with ragged ends"""
    c = U.case(a)
    handles = [U.lone_handle(m, c, net) for net in c["nets"]]
    wb = U.batch_of(m, c)
    desc = U.model_desc(c)
    assert U.R == 16
    for n in (1, 15, 16, 17, 33, 65, 129):
        for T in (1, 2, 7):
            x0, V = U.inputs(a, n, T)
            for kx in (1, n):
                start = x0[0] if kx == 1 else x0
                X = wb.validate(desc, start, V, trajectories=True)["X"]
                assert X.shape == (3, T + 1, n, c["s"])
                for i, h in enumerate(handles):
                    ref = h.model_rollout(start, V, costs=False)[0]
                    assert np.isfinite(ref).all()
                    np.testing.assert_array_equal(X[i], ref, err_msg="a %d member %d n %d T %d kx %d" % (a, i, n, T, kx))
                assert not np.array_equal(X[0, 1:], X[1, 1:]) and not np.array_equal(X[1, 1:], X[2, 1:])
    # a model object describes itself: the same bits through NNPointMassModel
    obj = m.NNPointMassModel(stateDim=2 * a, actionDim=a, hidden=(256, 256), weights=c["nets"][0], dt=0.1)
    obj.set_Xmean_Xstd(c["norm"]["xmean"], c["norm"]["xstd"])
    obj.set_Ymean_Ystd(c["norm"]["ymean"], c["norm"]["ystd"])
    x0, V = U.inputs(a, 65, 2)
    np.testing.assert_array_equal(wb.validate(obj, x0, V, trajectories=True)["X"], wb.validate(desc, x0, V, trajectories=True)["X"])
    for h in handles:
        h.close()
    wb.close()


# ---- 2. members equal the fp32 restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", U.A_DIMS, ids=A_IDS)
def test_members_equal_the_fp32_restatement(m, a):
    c = U.case(a)
    wb = U.batch_of(m, c)
    for n, T, shared in ((17, 7, False), (129, 2, False), (1, 1, True), (64, 3, True)):
        x0, V = U.inputs(a, n, T)
        start = x0[0] if shared else x0
        X = wb.validate(U.model_desc(c), start, V, trajectories=True)["X"]
        for i, net in enumerate(c["nets"]):
            np.testing.assert_array_equal(X[i], U.rollout(c, net, start, V), err_msg="a %d member %d n %d T %d" % (a, i, n, T))
    wb.close()


# ---- 3. the squared-error sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", U.A_DIMS, ids=A_IDS)
def test_sse_against_fp64(m, a, capsys):
    """sse[m, j] against the sum of (X - G)^2 in float64 over the RETURNED fp32 trajectories: relative error <= 2 (T + 6 + d) 2^-24, d = 4.
    The derivation, with u = 2^-24 (the unit roundoff of fp32): every term is non-negative, so the relative errors of the partial sums
    never amplify — a sum of non-negative terms computed with d roundings on the path of a term is off by at most (1 + u)^d - 1 relative.
      * a term e * e: the difference X - G of two fp32 numbers is rounded once (relative u on e, 2u on e^2) and the square once: 3u.
      * the thread's sum: T + 1 serial fp32 additions (row 0, then the T steps): (T + 1) u on the oldest term.
      * the 16 trajectories of a block: a fixed pairwise tree of d = 4 levels, one addition on a term's path each: 4u.
      * the blocks of 16 trajectories: added in float64: < u in all.
    (3 + T + 1 + 4 + 1) u = (T + 5 + d) u to first order; the bar 2 (T + 6 + d) u leaves the second-order terms and a factor of two.
    n = 129: nine blocks, the last one with a single live trajectory."""
    c, x0, V, G = U.sse_case(a)
    wb = U.batch_of(m, c)
    desc = U.model_desc(c)
    out = wb.validate(desc, x0, V, gt=G, trajectories=True)
    ref = L.sse64(out["X"], G)
    assert out["sse"].dtype == np.float64 and out["sse"].shape == ref.shape == (3, c["s"])
    rel = np.abs(out["sse"] - ref) / ref
    with capsys.disabled():
        print("\na = %d: largest relative distance of sse to fp64 %.3g (bound %.3g)" % (a, rel.max(), U.sse_bar(U.T_SSE)))
    assert (rel <= U.sse_bar(U.T_SSE)).all(), rel.max()
    np.testing.assert_array_equal(wb.validate(desc, x0, V, gt=G)["sse"], out["sse"])  # the same sums without the trajectories
    for i in range(3):  # a member judged against itself
        own = wb.validate(desc, x0, V, gt=out["X"][i])["sse"]
        assert (own[i] == 0.0).all() and (own[(i + 1) % 3] > 0.0).all()
    wb.close()


# ---- 4. isolation and determinism ----------------------------------------------------------------------------------------------------------
def test_isolation_and_determinism(m):
    c, x0, V, G = U.sse_case(2)
    desc = U.model_desc(c)
    rng = np.random.default_rng(3)
    Xd, Yd = rng.standard_normal((40, 6)).astype(F32), rng.standard_normal((40, 4)).astype(F32)
    wb, quiet = U.batch_of(m, c), U.batch_of(m, c)  # `quiet` never validates
    for b in (wb, quiet):
        b.set_data(Xd, Yd)
        b.train(2, 1e-3)
    w_before = [wb.get_weights(i) for i in range(3)]
    a = wb.validate(desc, x0, V, gt=G, trajectories=True)
    b = wb.validate(desc, x0, V, gt=G, trajectories=True)
    np.testing.assert_array_equal(a["X"], b["X"])
    np.testing.assert_array_equal(a["sse"], b["sse"])
    assert np.isfinite(a["sse"]).all()
    # member 1 overflows: its own sums are not finite, its neighbours' bits stay
    huge = dict(W=[np.full_like(w, 1e30) for w in c["nets"][1]["W"]], b=[np.full_like(v, 1e30) for v in c["nets"][1]["b"]])
    wb.set_weights(huge, member=1)
    d = wb.validate(desc, x0, V, gt=G, trajectories=True)
    assert not np.isfinite(d["sse"][1]).any()
    for i in (0, 2):
        np.testing.assert_array_equal(d["sse"][i], a["sse"][i])
        np.testing.assert_array_equal(d["X"][i], a["X"][i])
    wb.set_weights(w_before[1], member=1)
    # nothing of the batch moved: weights, step count, and the next training step
    assert wb.step_count() == quiet.step_count() == 2
    for i in range(3):
        for key in ("W", "b"):
            for got, ref in zip(wb.get_weights(i)[key], quiet.get_weights(i)[key]):
                np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(wb.train(1, 1e-3)[0], quiet.train(1, 1e-3)[0])
    for i in range(3):
        for key in ("W", "b"):
            for got, ref in zip(wb.get_weights(i)[key], quiet.get_weights(i)[key]):
                np.testing.assert_array_equal(got, ref)
    wb.close()
    quiet.close()


# ---- 5. many members --------------------------------------------------------------------------------------------------------------------
def test_300_members(m):
    c = U.case(2)
    nets = {0: c["nets"][1], 149: c["nets"][2], 299: c["truth"]}
    wb = m.WideLearnerBatch(c["nets"][0], 300)
    for i, net in nets.items():
        wb.set_weights(net, member=i)
    x0, V = U.inputs(2, 1, 2)
    G = U.ground_truth(c, x0, V)
    out = wb.validate(U.model_desc(c), x0, V, gt=G, trajectories=True)
    assert out["X"].shape == (300, 3, 1, 4) and out["sse"].shape == (300, 4)
    default = U.rollout(c, c["nets"][0], x0, V)
    for i in (1, 148, 150, 298):
        np.testing.assert_array_equal(out["X"][i], default)
    for i, net in nets.items():
        ref = U.rollout(c, net, x0, V)
        np.testing.assert_array_equal(out["X"][i], ref)
        assert not np.array_equal(ref, default)
    np.testing.assert_array_equal(out["sse"][1], out["sse"][298])
    wb.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_usable(m):
    from mppi_tf_amd import _lib
    c = U.case(2)
    wb = U.batch_of(m, c)
    n, T = 5, 3
    x0, V = U.inputs(2, n, T)
    G = U.ground_truth(c, x0, V)
    X = np.zeros((3, T + 1, n, 4), F32)
    sse = np.zeros((3, 4), np.float64)
    fp, dp = _lib.fp, lambda a: a.ctypes.data_as(_lib.DP)

    def desc(kind=U.MLP, s=4, a=2, xstd=None):
        held = None if xstd is None else np.ascontiguousarray(xstd, F32)
        return _lib.LearnerModel(kind, s, a, 0.1, None, fp(held), None, None), held

    def call(model, x0_=x0, kx=n, V_=V, G_=G, n_=n, T_=T, sse_=sse, X_=X):
        st = wb.lib.mppi_learner_wide_batch_validate(wb.h, C.byref(model[0]) if model is not None else None, fp(x0_), kx, fp(V_), fp(G_), n_, T_,
                                                     dp(sse_) if sse_ is not None else None, fp(X_))
        return st, (wb.lib.mppi_learner_wide_batch_last_error(wb.h) or b"").decode()

    ok = desc()
    assert call(ok)[0] == 0
    bad_std = np.ones(6, F32)
    bad_std[4] = 0.0
    refused = [
        (call(None), 1, "NULL pointer"), (call(ok, x0_=None), 1, "NULL pointer"), (call(ok, V_=None), 1, "NULL pointer"),
        (call(ok, sse_=None, X_=None), 1, "both NULL"), (call(ok, G_=None), 1, "needs the ground truth"),
        (call(ok, n_=0, kx=0), 1, "n and T must be >= 1"), (call(ok, T_=0), 1, "n and T must be >= 1"),
        (call(ok, n_=1 << 16, kx=1, T_=(1 << 14) + 1), 1, "2^30"), (call(ok, kx=2), 1, "kx in {1, n}"),
        (call(desc(kind=0)), 4, "model_kind"), (call(desc(kind=2)), 4, "model_kind"), (call(desc(kind=L.NN_AUV, s=13, a=6)), 4, "model_kind"),
        (call(desc(kind=L.NN_AUV_SPEED, s=13, a=6)), 4, "model_kind"),
        (call(desc(U.MLP, 5, 2)), 4, "s_dim = 2 a_dim"), (call(desc(U.MLP, 10, 5)), 4, "a_dim in 1..4"), (call(desc(U.MLP, 0, 0)), 4, "a_dim in 1..4"),
        (call(desc(U.MLP, 6, 3)), 4, "the batch's widths are [6, 256, 256, 4]"), (call(desc(U.MLP, 2, 1)), 4, "takes [3, 256, 256, 2]"),
        (call(desc(xstd=bad_std)), 1, "xstd[4] is 0"),
    ]
    for (st, msg), want, text in refused:
        assert st == want and msg.startswith("mppi_learner_wide_batch_validate: ") and text in msg, (st, want, msg)
    # the Python wrapper checks shapes before the library
    for args in ((x0, V[:, :, :1]), (x0[:3], V), (x0[:, :3], V)):
        with pytest.raises(ValueError):
            wb.validate(U.model_desc(c), *args, trajectories=True)
    with pytest.raises(ValueError):
        wb.validate(U.model_desc(c), x0, V)
    with pytest.raises(ValueError):
        wb.validate(U.model_desc(c), x0, V, gt=G[:-1])
    with pytest.raises(ValueError):
        wb.validate(dict(U.model_desc(c), xstd=np.ones(5, F32)), x0, V, trajectories=True)
    # ... and the batch still validates and trains
    np.testing.assert_array_equal(wb.validate(U.model_desc(c), x0, V, trajectories=True)["X"][2], U.rollout(c, c["nets"][2], x0, V))
    rng = np.random.default_rng(1)
    wb.set_data(rng.standard_normal((20, 6)).astype(F32), rng.standard_normal((20, 4)).astype(F32))
    assert np.isfinite(wb.train(2, 1e-3)[0]).all() and wb.step_count() == 2
    wb.close()


# ---- 7. the k-fold harness -----------------------------------------------------------------------------------------------------------------
def point_mass_data(n, kv=4, tau=5):
    """n transitions of a unit point mass (x, vx, y, vy), and val = (gtTrajs [kv, tau, 4], actionSeqs [kv, tau, 2]) of the same plant"""
    step = lambda x, u: x + 0.1 * np.concatenate([x[:, 1:2], u[:, 0:1], x[:, 3:4], u[:, 1:2]], axis=1)
    rng = np.random.default_rng(80)
    x, u = rng.standard_normal((n, 4, 1)), rng.standard_normal((n, 2, 1))
    act = rng.standard_normal((kv, tau, 2))
    gt = [rng.standard_normal((kv, 4))]
    for t in range(tau - 1):
        gt.append(step(gt[-1], act[:, t]))
    return x, u, step(x, u), (np.stack(gt, axis=1), act)


def test_k_fold_trajectory_validation(m):
    n, k, rates, epoch = 90, 3, (1e-3, 1e-2), 12
    x, u, xn, val = point_mass_data(n)
    model = m.NNPointMassModel(stateDim=4, actionDim=2, hidden=(256, 256), seed=81)
    learner = m.LearnerBase(model, bufferSize=n)
    learner.add_rb(x, u, xn)
    learner.stats()
    w0 = [w.copy() for w in model.get_weights()]
    seen = []
    log = learner.k_fold_trajectory_validation(k=k, learningRate=rates, epoch=epoch, seed=3, val=val, writer=lambda e, d: seen.append((e, sorted(d))))
    assert log is learner.kfold_log and log["val"].shape == (2, 2, k) and log["val"].dtype == np.float64
    assert np.isfinite(log["val"]).all() and (log["val"] > 0).all()
    assert seen == [(e, ["test", "train", "val"] if e % 10 == 0 else ["test", "train"]) for e in range(epoch)]
    plain = learner.k_fold_validation(k=k, learningRate=rates, epoch=epoch, seed=3)
    assert "val" not in plain
    np.testing.assert_array_equal(log["train"], plain["train"])
    np.testing.assert_array_equal(log["test"], plain["test"])
    # the validations again, by hand: fresh batches trained 1 and 11 steps in one call each
    X, y = model.prepare_training_data(x, xn, u)
    folds = m.kfold_indices(n, k, 3)
    for j, steps in enumerate((1, 11)):
        wb = m.WideLearnerBatch(dict(W=w0[0::2], b=w0[1::2]), 2 * k)
        wb.set_data(X, y)
        for r in range(2):
            for f, (tr, te) in enumerate(folds):
                wb.set_split(r * k + f, tr, te)
        wb.train(steps, np.repeat(np.array(rates, F32), k))
        err, split = learner.validate_fold(wb, val, split=True)
        np.testing.assert_array_equal(err.reshape(2, k), log["val"][j])
        assert split.shape == (2 * k, 4)
        # the host path: a model holding the member's weights, rolled step by step and summed in fp64 (LearnerBase.validate)
        for i in range(2 * k):
            w = wb.get_weights(i)
            member = m.NNPointMassModel(stateDim=4, actionDim=2, hidden=(256, 256), weights=w)
            member.set_Xmean_Xstd(model.Xmean, model.Xstd)
            member.set_Ymean_Ystd(model.Ymean, model.Ystd)
            host, host_split = learner.validate(member, val[1], val[0], split=True)
            np.testing.assert_allclose(err[i], host, rtol=1e-5)
            np.testing.assert_allclose(split[i], host_split, rtol=1e-5)
        wb.close()
    for a, b in zip(model.get_weights(), w0):  # copies were trained
        np.testing.assert_array_equal(a, b)
    # the pinned refusals stay
    with pytest.raises(ValueError, match="trajectory validation of wide members is not built into this method: use k_fold_trajectory_validation"):
        learner.grid_search(rates, k=k, epoch=epoch, val=val, by="val")


def test_k_fold_trajectory_validation_of_a_narrow_model_is_k_fold_validation(m):
    n, k, rates, epoch = 90, 3, (1e-3, 1e-2), 12
    x, u, xn, val = point_mass_data(n)
    model = m.NNPointMassModel(stateDim=4, actionDim=2, hidden=(32, 32), seed=82)
    learner = m.LearnerBase(model, bufferSize=n)
    learner.add_rb(x, u, xn)
    learner.stats()
    new = learner.k_fold_trajectory_validation(k=k, learningRate=rates, epoch=epoch, seed=3, val=val)
    old = learner.k_fold_validation(k=k, learningRate=rates, epoch=epoch, seed=3, val=val)
    assert sorted(new) == sorted(old) == ["test", "train", "val"] and new["val"].shape == (2, 2, k)
    for key in new:
        np.testing.assert_array_equal(new[key], old[key])


# ---- 8. the example --------------------------------------------------------------------------------------------------------------------------
def test_learn_loop_chooses_the_wide_models_rate_by_h_step_error(m, capsys):
    """examples/learn_loop.py --model point_mass --hidden 256 --kfold K --lrs a,b --kfold-val: the narrow run's second line per round with
    the H-step table, whose argmin trains the round"""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import learn_loop
    finally:
        sys.path.pop(0)
    argv = ["--model", "point_mass", "--hidden", "256", "--rounds", "2", "--samples", "128", "--horizon", "8", "--steps", "12", "--epochs", "3",
            "--kfold", "3", "--lrs", "1e-3,1e-2"]
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
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 4 and len([l for l in out if "3-fold held-out loss" in l]) == 2  # without the flag: the held-out table and the round's line
    with pytest.raises(SystemExit):  # the wide folds still have no episode harness
        learn_loop.main(argv + ["--kfold-episode"])
    capsys.readouterr()
