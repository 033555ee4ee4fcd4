"""Helpers of the batched-learner tests: the lone-learner reference a member must equal bit for bit, the first test's five-member case,
and a CPU emulation of the kernels' fp32 loss reduction (for the order needle's precondition). No test in here."""
import numpy as np

from learner_util import make_net

F32 = np.float32
DEFAULT_HP = (0.9, 0.999, 1e-7)


def pool(dims, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dims[0])).astype(F32)
    Y = np.tanh(X @ rng.standard_normal((dims[0], dims[-1])) * 0.3).astype(F32)
    return X, Y


def same_weights(a, b):
    for key in ("W", "b"):
        for u, v in zip(a[key], b[key]):
            np.testing.assert_array_equal(u, v)


def weights_differ(a, b):
    return any(not np.array_equal(u, v) for key in ("W", "b") for u, v in zip(a[key], b[key]))


def lone_history(m, net, X, Y, train_idx, test_idx, lr, hp, steps, start=None):
    """A lone Learner driven one step at a time on X[train_idx], Y[train_idx] -> per step: loss_first, the weights after the step, and
    evaluate() of a second lone learner holding those weights on X[test_idx], Y[test_idx] (NaN without test rows)."""
    a = m.Learner(net)
    if start is not None:
        a.set_weights(start)
    a.set_data(X[train_idx], Y[train_idx])
    e = None
    if len(test_idx):
        e = m.Learner(net)
        e.set_data(X[test_idx], Y[test_idx])
    out = dict(loss_train=[], loss_test=[], weights=[])
    for _ in range(steps):
        first, _last = a.train(1, lr, *hp)
        w = a.get_weights()
        out["loss_train"].append(F32(first))
        out["weights"].append(w)
        if e is None:
            out["loss_test"].append(F32(np.nan))
        else:
            e.set_weights(w)
            out["loss_test"].append(F32(e.evaluate()))
    a.close()
    if e is not None:
        e.close()
    return out


def five_member_case():
    """dims [16, 32, 32, 32, 13], pool of 1100 rows, n_train = 1 (one row), 257 (a second loss block), 513 (a second gradient chunk, odd),
    1025 (a third chunk) and 600; test lists of 0, 1, 75, 256 and 300 rows; random unsorted lists, member 3's with repeated rows;
    distinct rates, two members away from Adam's default beta1, beta2, eps."""
    dims, n = [16, 32, 32, 32, 13], 1100
    X, Y = pool(dims, n, 11)
    rng = np.random.default_rng(12)
    n_train, n_test = (1, 257, 513, 1025, 600), (0, 1, 75, 256, 300)
    train = [rng.integers(0, n, nt) if mi == 3 else rng.permutation(n)[:nt] for mi, nt in enumerate(n_train)]
    test = [rng.permutation(n)[:nt] for nt in n_test]
    assert len(np.unique(train[3])) < len(train[3])  # repeated rows
    assert all(np.any(np.diff(t) < 0) for t in train[1:])  # unsorted
    lr = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2)
    hp = [DEFAULT_HP, (0.8, 0.99, 1e-6), DEFAULT_HP, (0.95, 0.9999, 1e-8), DEFAULT_HP]
    return dict(dims=dims, net=make_net(dims, 10), X=X, Y=Y, train=train, test=test, lr=lr, hp=hp, calls=(2, 1, 3))


def run_batch(m, case, change=None):
    """the case's batch from scratch, trained call by call -> loss_train, loss_test [steps, B] and every member's weights after each call.
    change = (member, train_idx, test_idx, lr, hp, weights): that member's split, rates and weights replaced before training."""
    B = len(case["train"])
    train, test, lr, hp = list(case["train"]), list(case["test"]), list(case["lr"]), list(case["hp"])
    lb = m.LearnerBatch(case["net"], B)
    lb.set_data(case["X"], case["Y"])
    if change is not None:
        mi = change[0]
        train[mi], test[mi], lr[mi], hp[mi] = change[1:5]
        lb.set_weights(change[5], member=mi)
    for mi in range(B):
        lb.set_split(mi, train[mi], test[mi])
    b1, b2, eps = (np.array([h[q] for h in hp], F32) for q in range(3))
    lt, ls, weights = [], [], []
    for steps in case["calls"]:
        a, b = lb.train(steps, np.array(lr, F32), b1, b2, eps)
        lt.append(a)
        ls.append(b)
        weights.append([lb.get_weights(mi) for mi in range(B)])
    steps_done = lb.step_count()
    lb.close()
    return dict(loss_train=np.concatenate(lt), loss_test=np.concatenate(ls), weights=weights, steps=steps_done)


def check_members_against_lone(m, net, X, Y, train, test, lr, hp, calls, got):
    """every member of a finished run_batch-style result against its lone learners: weights after each call, every loss"""
    total = sum(calls)
    for mi in range(len(train)):
        ref = lone_history(m, net, X, Y, train[mi], test[mi], lr[mi], hp[mi], total)
        at = 0
        for c, steps in enumerate(calls):
            at += steps
            same_weights(got["weights"][c][mi], ref["weights"][at - 1])
        np.testing.assert_array_equal(got["loss_train"][:, mi], np.array(ref["loss_train"], F32), err_msg="loss_train of member %d" % mi)
        np.testing.assert_array_equal(got["loss_test"][:, mi], np.array(ref["loss_test"], F32), err_msg="loss_test of member %d" % mi)


def row_errors_fp32(pred, Y):
    """per-row sum over the outputs of (pred - y)^2 as the kernels form it: fp32, unfused, outputs in order. With the device's own
    predictions (Learner.evaluate(pred=True)) these are the kernel's per-row values bit for bit."""
    e = (pred.astype(F32) - Y.astype(F32)).astype(F32)
    se = np.zeros(len(e), F32)
    for o in range(e.shape[1]):
        se = (se + (e[:, o] * e[:, o]).astype(F32)).astype(F32)
    return se


def block_loss_fp32(se, n_out):
    """the kernels' reduction of per-row squared errors `se` (in list order) in fp32: blocks of 256 rows by position, in each block four
    waves of 64 lanes reduced by an xor butterfly (offsets 32 .. 1), the waves summed in order, the blocks summed in order, then the mean"""
    n = len(se)
    total = F32(0)
    for b0 in range(0, n, 256):
        blk = np.zeros(256, F32)
        blk[:min(256, n - b0)] = se[b0:b0 + 256]
        waves = blk.reshape(4, 64)
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            waves = (waves + waves[:, lanes ^ off]).astype(F32)
        r = waves[:, 0]
        total = F32(total + F32(F32(F32(r[0] + r[1]) + r[2]) + r[3]))
    return F32(total / F32(F32(n) * F32(n_out)))


def fossen_transitions(m, n, seed=0, scale=300.0):
    """n transitions of the (device) Fossen AUVModel from random states and forces, as tests/test_learner_gpu.py draws them"""
    from conftest import load_golden
    plant = m.AUVModel(actionDim=6, dt=0.1, parameters=load_golden("model_auv")["params"])
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 13)) * np.array([1, 1, 1, 0, 0, 0, 0, .5, .5, .5, .2, .2, .2])
    q = rng.standard_normal((n, 4)) * 0.3 + np.array([0, 0, 0, 1.0])
    x[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    u = scale * rng.standard_normal((n, 6))
    return x[..., None], u[..., None], plant.build_step_graph("plant", x[..., None], u[..., None])
