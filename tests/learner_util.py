"""Helpers of the learner tests (the conventions of tests/test_learner_gpu.py): a random Dense network, its loss and gradients by torch
CPU fp32 autograd, tf.keras.optimizers.Adam's update in numpy. No GPU, no test in here."""
import struct

import numpy as np

F32 = np.float32


def make_net(dims, seed=0):
    rng = np.random.default_rng(seed)
    return dict(W=[(rng.uniform(-1, 1, (dims[i], dims[i + 1])) * np.sqrt(6.0 / (dims[i] + dims[i + 1]))).astype(F32) for i in range(len(dims) - 1)],
                b=[(0.1 * rng.standard_normal(dims[i + 1])).astype(F32) for i in range(len(dims) - 1)])


def torch_loss_and_grads(net, X, Y):
    import torch
    Ws = [torch.tensor(w, requires_grad=True) for w in net["W"]]
    bs = [torch.tensor(b, requires_grad=True) for b in net["b"]]
    h = torch.tensor(X)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ W + b
        if l + 1 < len(Ws):
            h = torch.relu(h)
    loss = torch.mean((h - torch.tensor(Y)) ** 2)
    loss.backward()
    return float(loss.detach()), [w.grad.numpy() for w in Ws], [b.grad.numpy() for b in bs]


def numpy_loss_and_grads64(net, X, Y):
    """the same loss and gradients in fp64 numpy (the fp32 weights and data, exact arithmetic for fp32 purposes)"""
    Ws, bs = [w.astype(np.float64) for w in net["W"]], [b.astype(np.float64) for b in net["b"]]
    acts = [X.astype(np.float64)]
    for l, (W, b) in enumerate(zip(Ws, bs)):
        z = acts[-1] @ W + b
        acts.append(np.maximum(z, 0.0) if l + 1 < len(Ws) else z)
    e = acts[-1] - Y
    d = 2.0 * e / e.size
    gW, gb = [None] * len(Ws), [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        gW[l], gb[l] = acts[l].T @ d, d.sum(axis=0)
        if l:
            d = (d @ Ws[l].T) * (acts[l] > 0)
    return float(np.mean(e ** 2)), gW, gb


def data(dims, n, seed=2):
    """n rows of standard-normal inputs and targets, fp32 (the data of the gradient tests)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dims[0])).astype(F32), rng.standard_normal((n, dims[-1])).astype(F32)


def numpy_forward64(net, X):
    """the forward pass in fp64 numpy -> (predictions, the pre-activations of every layer)"""
    h, zs = X.astype(np.float64), []
    for l, (W, b) in enumerate(zip(net["W"], net["b"])):
        zs.append(h @ W.astype(np.float64) + b.astype(np.float64))
        h = np.maximum(zs[-1], 0.0) if l + 1 < len(net["W"]) else zs[-1]
    return h, zs


def torch_forward(net, X):
    """the forward pass in torch CPU fp32"""
    import torch
    h = torch.tensor(X)
    for l, (W, b) in enumerate(zip(net["W"], net["b"])):
        h = h @ torch.tensor(W) + torch.tensor(b)
        if l + 1 < len(net["W"]):
            h = torch.relu(h)
    return h.numpy()


def grad_bar(ref):
    """the gradient tests' bar of one tensor, per entry: rtol 2e-5 and atol 2e-6 of the tensor's largest entry"""
    ref = np.asarray(ref, np.float64)
    return 2e-5 * np.abs(ref) + 2e-6 * max(np.abs(ref).max(), 1e-12)


def copy_net(net):
    return dict(W=[w.copy() for w in net["W"]], b=[b.copy() for b in net["b"]])


def keras_adam(net, state, gW, gb, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    """tf.keras.optimizers.Adam: m, v, lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), w -= lr_t m / (sqrt(v) + eps); fp32"""
    lr_t = F32(lr) * np.sqrt(F32(1) - F32(b2) ** F32(t)) / (F32(1) - F32(b1) ** F32(t))
    for key, grads in (("W", gW), ("b", gb)):
        for l, g in enumerate(grads):
            mm, vv = state[key][l]
            mm[:] = F32(b1) * mm + F32(1 - b1) * g
            vv[:] = F32(b2) * vv + F32(1 - b2) * g * g
            net[key][l] = (net[key][l] - lr_t * mm / (np.sqrt(vv) + F32(eps))).astype(F32)


def learner_file_header(widths, n_layers=None, step=0, has_norm=0):
    """the 40-byte header of a learner file (include/mppi_c.h): magic, n_layers, widths[5], adam_step, has_norm"""
    widths = list(widths) + [0] * (5 - len(widths))
    n_layers = sum(1 for w in widths if w) - 1 if n_layers is None else n_layers
    return b"MPPILRN1" + struct.pack("<8i", n_layers, *widths, step, has_norm)


# shapes mppi_learner_create must refuse with MPPI_ERR_UNSUPPORTED (4)
REFUSED_SHAPES = ([9, 256, 6], [9, 256, 256, 256, 6], [40, 256, 256, 6], [9, 256, 256, 40], [9, 256, 32, 6], [16, 64, 13])
