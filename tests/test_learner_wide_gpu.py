"""The wide learner on the GPU (csrc/mppi_learner_wide.hip): the [in, 256, 256, out] network of an MPPI_MODEL_MLP controller trained with
full-batch Adam, every product on the exact-fp32 matrix-core instruction. Against torch CPU fp32 autograd and tf.keras' Adam in numpy,
with the tolerances of tests/test_learner_gpu.py; then the loop it closes: transitions of the analytic point mass ->
LearnerBase(NNPointMassModel) -> trained weights -> the 2 x 256 controller rolls them out, and examples/learn_loop.py --model point_mass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from learner_util import REFUSED_SHAPES, keras_adam, make_net, numpy_loss_and_grads64, torch_loss_and_grads
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


def data(dims, n, seed=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dims[0])).astype(F32), rng.standard_normal((n, dims[-1])).astype(F32)


# the sample chunk of the weight-gradient GEMMs is 512, a divisor of 4096: 4097 is one sample past a chunk boundary. BIG_CASE: 65 chunks,
# one row into the last one and into a last workgroup tile
GRAD_CASES = [([3, 256, 256, 2], 64), ([9, 256, 256, 6], 333), ([6, 256, 256, 4], 1000), ([12, 256, 256, 8], 4097), ([32, 256, 256, 32], 257)]
BIG_CASE = ([9, 256, 256, 6], 32768 + 129)


@pytest.mark.parametrize("dims,n", GRAD_CASES)
def test_gradients_match_torch_autograd(m, dims, n):
    """loss, dLoss/dW, dLoss/db and the predictions against torch CPU fp32 autograd: below one workgroup tile, odd with a partial tile,
    one sample past a chunk boundary, the smallest and the full-width edges. evaluate()'s loss and predictions agree with them."""
    net = make_net(dims, 1)
    X, Y = data(dims, n)
    lr = m.Learner(net)
    lr.set_data(X, Y)
    loss, g, pred = lr.evaluate(grads=True, pred=True)
    loss_e, pred_e = lr.evaluate(pred=True)
    assert loss_e == loss
    np.testing.assert_array_equal(pred_e, pred)
    tl, tW, tb = torch_loss_and_grads(net, X, Y)
    for l in range(3):
        sw, sb = max(np.abs(tW[l]).max(), 1e-12), max(np.abs(tb[l]).max(), 1e-12)
        print("layer %d: worst |dW - torch| / max|dW| = %.3g, worst |db - torch| / max|db| = %.3g"
              % (l, np.abs(g["W"][l] - tW[l]).max() / sw, np.abs(g["b"][l] - tb[l]).max() / sb))
    print("loss %.8g torch %.8g (rel %.3g)" % (loss, tl, abs(loss - tl) / abs(tl)))
    assert abs(loss - tl) <= 2e-6 * abs(tl)
    for l in range(3):
        assert g["W"][l].shape == tuple(dims[l:l + 2]) and g["b"][l].shape == (dims[l + 1],)
        scale = max(np.abs(tW[l]).max(), 1e-12)
        np.testing.assert_allclose(g["W"][l], tW[l], rtol=2e-5, atol=2e-6 * scale)
        np.testing.assert_allclose(g["b"][l], tb[l], rtol=2e-5, atol=2e-6 * max(np.abs(tb[l]).max(), 1e-12))
    assert pred.shape == (n, dims[-1]) and abs(np.mean((pred - Y) ** 2) - tl) <= 1e-5 * tl
    # evaluating changed nothing
    w = lr.get_weights()
    for l in range(3):
        np.testing.assert_array_equal(w["W"][l], net["W"][l])
        np.testing.assert_array_equal(w["b"][l], net["b"][l])
    assert lr.step_count() == 0


def test_gradients_of_a_large_batch_match_fp64(m):
    """33 000 samples, 65 partial tiles per parameter. The same tolerances, against the gradients in fp64 numpy: at this sample count an
    fp32 reference's own summation error is of the order of the tolerance (the device differs from torch by 1.6e-6 max|dW| here and
    from fp64 by 2e-7), so the reference here has none."""
    dims, n = BIG_CASE
    net = make_net(dims, 1)
    X, Y = data(dims, n)
    lr = m.Learner(net)
    lr.set_data(X, Y)
    loss, g, pred = lr.evaluate(grads=True, pred=True)
    rl, rW, rb = numpy_loss_and_grads64(net, X, Y)
    for l in range(3):
        print("layer %d: worst |dW - fp64| / max|dW| = %.3g, worst |db - fp64| / max|db| = %.3g"
              % (l, np.abs(g["W"][l] - rW[l]).max() / np.abs(rW[l]).max(), np.abs(g["b"][l] - rb[l]).max() / np.abs(rb[l]).max()))
    print("loss %.8g fp64 %.8g (rel %.3g)" % (loss, rl, abs(loss - rl) / rl))
    assert abs(loss - rl) <= 2e-6 * rl
    for l in range(3):
        np.testing.assert_allclose(g["W"][l], rW[l], rtol=2e-5, atol=2e-6 * np.abs(rW[l]).max())
        np.testing.assert_allclose(g["b"][l], rb[l], rtol=2e-5, atol=2e-6 * np.abs(rb[l]).max())
    assert abs(np.mean((pred.astype(np.float64) - Y) ** 2) - rl) <= 1e-5 * rl
    # ten steps there: two learners, identical bits
    a, b = m.Learner(net), m.Learner(net)
    a.set_data(X, Y)
    b.set_data(X, Y)
    ra, rb2 = a.train(10, 1e-3), b.train(10, 1e-3)
    assert ra == rb2 and ra[1] < ra[0]
    for wa, wb in zip(a.get_weights()["W"], b.get_weights()["W"]):
        np.testing.assert_array_equal(wa, wb)


def test_gradients_entry_point_on_both_kinds(m):
    """mppi_learner_gradients on a narrow learner = mppi_learner_evaluate's padded grads_out, sliced, bit for bit; on a wide learner
    mppi_learner_evaluate refuses grads_out (status 4, the text names the new call) and still serves the loss and the predictions."""
    from mppi_tf_amd._lib import fp
    dims, n = [16, 32, 32, 32, 13], 1000
    net = make_net(dims, 1)
    X, Y = data(dims, n)
    lr = m.Learner(net)
    lr.set_data(X, Y)
    loss, g = lr.evaluate(grads=True)  # through mppi_learner_gradients
    padded, l2 = np.zeros((4, 33, 32), F32), np.zeros(1, F32)
    assert lr.lib.mppi_learner_evaluate(lr.h, fp(l2), fp(padded), None) == 0
    assert float(l2[0]) == loss
    for l in range(4):
        np.testing.assert_array_equal(g["W"][l], padded[l, :dims[l], :dims[l + 1]])
        np.testing.assert_array_equal(g["b"][l], padded[l, 32, :dims[l + 1]])
    # NULL outputs are allowed
    assert lr.lib.mppi_learner_gradients(lr.h, None, None, None) == 0
    dims, n = GRAD_CASES[1]
    wide = m.Learner(make_net(dims, 1))
    X, Y = data(dims, n)
    wide.set_data(X, Y)
    big = np.zeros((3, 257, 256), F32)
    st = wide.lib.mppi_learner_evaluate(wide.h, fp(l2), fp(big), None)
    assert st == 4 and b"mppi_learner_gradients" in wide.lib.mppi_learner_last_error(wide.h)
    pred = np.zeros((n, dims[-1]), F32)
    assert wide.lib.mppi_learner_evaluate(wide.h, fp(l2), None, fp(pred)) == 0
    loss_g, _, pred_g = wide.evaluate(grads=True, pred=True)
    assert float(l2[0]) == loss_g
    np.testing.assert_array_equal(pred, pred_g)
    tl, _, _ = torch_loss_and_grads(make_net(dims, 1), X, Y)
    assert abs(float(l2[0]) - tl) <= 2e-6 * tl


def test_adam_steps_match_the_keras_update(m):
    """40 full-batch Adam steps on the device against the same 40 steps with torch autograd + the Keras update in numpy (the 2 % drift
    band of the narrow learner's test: Adam normalises by sqrt(v), so where a gradient is of the order of eps its rounding error IS the
    update's); two learners give identical bits; 20 + 20 = 40; the update RULE is checked on the device's own gradients."""
    dims, n, steps, lr_rate = [9, 256, 256, 6], 2000, 40, 1e-3
    net = make_net(dims, 3)
    rng = np.random.default_rng(4)
    X = rng.standard_normal((n, 9)).astype(F32)
    Y = (np.tanh(X @ rng.standard_normal((9, 6)) * 0.3)).astype(F32)
    a, b = m.Learner(net), m.Learner(net)
    a.set_data(X, Y)
    b.set_data(X, Y)
    first, last = a.train(steps, lr_rate)
    b.train(steps // 2, lr_rate)
    b.train(steps - steps // 2, lr_rate)
    wa, wb = a.get_weights(), b.get_weights()
    for l in range(3):
        np.testing.assert_array_equal(wa["W"][l], wb["W"][l])
        np.testing.assert_array_equal(wa["b"][l], wb["b"][l])
    assert a.step_count() == steps and b.step_count() == steps and last < first
    ref = dict(W=[w.copy() for w in net["W"]], b=[v.copy() for v in net["b"]])
    state = dict(W=[(np.zeros_like(w), np.zeros_like(w)) for w in ref["W"]], b=[(np.zeros_like(v), np.zeros_like(v)) for v in ref["b"]])
    losses = []
    for t in range(1, steps + 1):
        tl, gW, gb = torch_loss_and_grads(ref, X, Y)
        losses.append(tl)
        keras_adam(ref, state, gW, gb, t, lr_rate)
    moved = max(np.abs(wa["W"][l] - net["W"][l]).max() for l in range(3))
    print("Adam: loss %.5f -> %.5f (torch %.5f -> %.5f); weights moved by up to %.3g, device vs reference differ by up to %.3g"
          % (first, last, losses[0], losses[-1], moved, max(np.abs(wa["W"][l] - ref["W"][l]).max() for l in range(3))))
    assert abs(first - losses[0]) <= 2e-6 * losses[0] and abs(last - losses[-1]) <= 2e-4 * losses[-1]
    for l in range(3):
        np.testing.assert_allclose(wa["W"][l], ref["W"][l], rtol=0, atol=2e-2 * moved)
        np.testing.assert_allclose(wa["b"][l], ref["b"][l], rtol=0, atol=2e-2 * moved)
    assert moved > 1e-2
    # two consecutive steps from the device's OWN gradients: the Keras update in numpy reproduces the device's weights to fp32 rounding
    c = m.Learner(net)
    c.set_data(X, Y)
    chk = dict(W=[w.copy() for w in net["W"]], b=[v.copy() for v in net["b"]])
    assert max(np.abs(w).max() for w in chk["W"] + chk["b"]) < 1.0
    st2 = dict(W=[(np.zeros_like(w), np.zeros_like(w)) for w in chk["W"]], b=[(np.zeros_like(v), np.zeros_like(v)) for v in chk["b"]])
    for t in (1, 2):
        _, g = c.evaluate(grads=True)
        c.train(1, lr_rate)
        keras_adam(chk, st2, g["W"], g["b"], t, lr_rate)
        wc = c.get_weights()
        for l in range(3):
            np.testing.assert_allclose(wc["W"][l], chk["W"][l], rtol=0, atol=3e-7)
            np.testing.assert_allclose(wc["b"][l], chk["b"][l], rtol=0, atol=3e-7)
    a.reset_optimizer()
    assert a.step_count() == 0


def test_the_wide_learner_survives_a_file(m, tmp_path):
    """save after 20 steps with a normalisation, from_file: weights, both moments, the step count and the normalisation round-trip (the
    moments are shown by ten further steps giving identical bits, and by the file's bytes); the documented size; a narrow learner
    refuses the wide file and a wide learner a narrow one."""
    dims, n = [9, 256, 256, 6], 700
    net = make_net(dims, 5)
    X, Y = data(dims, n, seed=6)
    a = m.Learner(net)
    a.set_data(X, Y)
    a.train(20, 1e-3)
    rng = np.random.default_rng(7)
    norm = dict(xmean=rng.standard_normal(9), xstd=rng.uniform(0.5, 2, 9), ymean=rng.standard_normal(6), ystd=rng.uniform(0.5, 2, 6))
    path = str(tmp_path / "wide")
    a.save(path, norm)
    raw = open(path, "rb").read()
    n_fl = sum(3 * (dims[l] + 1) * dims[l + 1] for l in range(3))
    assert len(raw) == 40 + 4 * n_fl + 8 * 2 * (9 + 6) and raw[:8] == b"MPPILRN1"
    assert list(np.frombuffer(raw, "<i4", 8, 8)) == [3, 9, 256, 256, 6, 0, 20, 1]
    wa = a.get_weights()
    np.testing.assert_array_equal(np.frombuffer(raw, "<f4", 9 * 256, 40).reshape(9, 256), wa["W"][0])
    np.testing.assert_array_equal(np.frombuffer(raw, "<f4", 256, 40 + 4 * 9 * 256), wa["b"][0])
    m0 = np.frombuffer(raw, "<f4", 10 * 256, 40 + 4 * 10 * 256)  # first moment of layer 0: after 20 steps it is not zero
    assert np.abs(m0).max() > 0
    b, got = m.Learner.from_file(path)
    assert b.widths == dims and b.step_count() == 20
    for key in norm:
        np.testing.assert_array_equal(got[key], norm[key])
    wb = b.get_weights()
    for l in range(3):
        np.testing.assert_array_equal(wa["W"][l], wb["W"][l])
        np.testing.assert_array_equal(wa["b"][l], wb["b"][l])
    path2 = str(tmp_path / "wide2")
    b.save(path2, norm)
    assert open(path2, "rb").read() == raw  # both moments too
    b.set_data(X, Y)
    assert a.train(10, 1e-3) == b.train(10, 1e-3)
    wa, wb = a.get_weights(), b.get_weights()
    for l in range(3):
        np.testing.assert_array_equal(wa["W"][l], wb["W"][l])
        np.testing.assert_array_equal(wa["b"][l], wb["b"][l])
    assert a.step_count() == 30 and b.step_count() == 30
    narrow = m.Learner(make_net([9, 32, 32, 6]))
    with pytest.raises(m.MppiError) as e:
        narrow.load(path)
    assert e.value.status == 7
    npath = str(tmp_path / "narrow")
    narrow.save(npath)
    with pytest.raises(m.MppiError) as e:
        a.load(npath)
    assert e.value.status == 7


def test_train_the_point_mass_network_and_control_with_it(m):
    """The loop for the point mass: 4000 transitions of the analytic model -> LearnerBase(NNPointMassModel): statistics, 200 Adam steps on
    the device; the trained model predicts the plant's next state far better than the untrained one, and the 2 x 256 controller built
    from the trained weights produces the sample costs and the control the fp64 oracle computes from the same weights."""
    a_dim, s_dim, n = 2, 4, 4000
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, s_dim)) * np.sqrt(np.array([2.0, 1.0, 2.0, 1.0]))  # states ~ N(0, diag(2, 1, 2, 1)), actions ~ N(0, 2^2)
    u = 2.0 * rng.standard_normal((n, a_dim))
    plant = m.Handle(k=1, tau=1, s_dim=s_dim, a_dim=a_dim, dt=0.1, mass=1.0)
    xn = plant.model_next(x.astype(F32), u.astype(F32)).astype(np.float64)
    model = m.NNPointMassModel(stateDim=s_dim, actionDim=a_dim)
    learner = m.LearnerBase(model, bufferSize=n)
    learner.add_rb(x[..., None], u[..., None], xn[..., None])
    assert learner.rb_trans()["obs"].shape == (n, s_dim, 1)
    learner.stats()
    assert model.Xstd.shape == (6,) and model.Ystd.shape == (4,) and np.all(model.Xstd > 0)
    mse = lambda: float(np.mean((model.predict(x[:500, :, None], u[:500, :, None])[..., 0] - xn[:500]) ** 2))
    before = mse()
    first, last = learner.train_all(learningRate=1e-3, epoch=200, augment=False)
    after = mse()
    print("NNPointMassModel trained on %d transitions: normalised loss %.4g -> %.4g, one-step MSE %.3g -> %.3g" % (n, first, last, before, after))
    assert last < 0.25 * first and after < 0.25 * before
    assert learner.step == 200 and learner._dev.step_count() == 200
    # the controller on the trained weights against the oracle on the same weights
    K, H = 1024, 8
    sigma = np.eye(a_dim)
    goal = [1.0, 0.0, -1.0, 0.0]
    h = m.Handle(k=K, tau=H, s_dim=s_dim, a_dim=a_dim, dt=0.1, lam=1.0, sigma=sigma, goal=goal, mlp=model.mlp(), seed=2)
    p64 = orc.Problem(tau=H, s=s_dim, a=a_dim, lam=1.0, sigma=sigma, goal=goal, mlp=model.mlp(), threads=0, dtype=np.float64)
    p32 = orc.Problem(tau=H, s=s_dim, a=a_dim, lam=1.0, sigma=sigma, goal=goal, mlp=model.mlp(), threads=0)
    x0 = np.array([0.2, 0.0, -0.1, 0.0], F32)
    un = h.next(x0)
    noise = h.debug_get(m.DBG_NOISE)
    u64, _, c64 = p64.next_with_noise(x0, np.zeros((H, a_dim)), noise)
    u32, _, c32 = p32.next_with_noise(x0, np.zeros((H, a_dim)), noise)
    assert np.isfinite(c64).all()
    c = h.debug_get(m.DBG_COSTS).astype(np.float64)
    rel = lambda v: float((np.abs(v - c64) / np.abs(c64)).max())
    e_gpu, e_cpu = np.abs(un - u64).max() / 1.0, np.abs(u32 - u64).max() / 1.0  # sigma = 1
    print("trained controller: rel cost err GPU %.3g / fp32 CPU %.3g; |du|/sigma GPU %.3g / fp32 CPU %.3g" % (rel(c), rel(c32.astype(np.float64)), e_gpu, e_cpu))
    assert rel(c) < 4 * max(rel(c32.astype(np.float64)), 1e-6)
    assert e_gpu <= max(1e-5, 4 * e_cpu)
    # LearnerBase's persistence on this model
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = learner.save_params(learner.step, d)
        other = m.NNPointMassModel(stateDim=s_dim, actionDim=a_dim)
        l2 = m.LearnerBase(other, bufferSize=8)
        l2.load_params(path)
        assert l2.step == 200
        for wa, wb in zip(model.get_weights(), other.get_weights()):
            np.testing.assert_array_equal(wa, wb)
        np.testing.assert_array_equal(other.Xstd, model.Xstd)
        f = model.save_params(os.path.join(d, "model"), 200)
        third = m.NNPointMassModel(stateDim=s_dim, actionDim=a_dim)
        third.load_params(f)
        np.testing.assert_array_equal(third.predict(x[:8, :, None], u[:8, :, None]), model.predict(x[:8, :, None], u[:8, :, None]))


def test_learn_loop_on_the_point_mass(m, capsys):
    """examples/learn_loop.py --model point_mass --hidden 256: two rounds to the end with finite figures; a second identical call prints
    identical figures; after each round the controller's model is the learner's (model_next == NNPointMassModel.predict, bit for bit)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import learn_loop
    finally:
        sys.path.pop(0)
    argv = ["--model", "point_mass", "--hidden", "256", "--rounds", "2", "--samples", "128", "--horizon", "8", "--steps", "16", "--epochs", "5"]
    seen = []

    def on_round(r, cont, model, X, U):
        np.testing.assert_array_equal(cont.model_next(X[:-1], U), model.predict(X[:-1, :, None], U[:, :, None])[..., 0])
        seen.append(r)

    learner, episodes, figures = learn_loop.main(argv, on_round=on_round)
    printed = capsys.readouterr().out.strip().splitlines()
    assert seen == [0, 1] and len(printed) == 2 and printed[0].startswith("round 1:") and printed[1].startswith("round 2:")
    assert len(figures) == 2 and all(len(f) == 7 for f in figures) and np.isfinite(np.asarray(figures, np.float64)).all()
    assert learner.rb.n == 32 and episodes[0][0].shape == (17, 4)
    assert [w.shape for w in learner.model.get_weights()[0::2]] == [(6, 256), (256, 256), (256, 4)]
    _, _, again = learn_loop.main(argv)
    assert capsys.readouterr().out.strip().splitlines() == printed and again == figures


def test_refused_shapes_leave_no_learner_behind(m):
    for dims in REFUSED_SHAPES:
        lib = m.load()
        h = C.c_void_p(0x1)
        net = make_net(dims)
        Ws, bs = [np.ascontiguousarray(w) for w in net["W"]], [np.ascontiguousarray(b) for b in net["b"]]
        wd = (C.c_int32 * len(dims))(*dims)
        st = lib.mppi_learner_create(len(Ws), wd, m.Learner._ptrs(Ws), m.Learner._ptrs(bs), 0, C.byref(h))
        assert st == 4 and not h.value, dims
        with pytest.raises(m.MppiError) as e:
            m.Learner(net)
        assert e.value.status == 4
