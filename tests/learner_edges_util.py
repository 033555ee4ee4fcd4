"""The learner edge matrix (tests/test_learner_edges_oracle.py on the CPU, tests/test_learner_edges_gpu.py on the GPU): the sample counts
and network shapes at which the structures of the learner kernels begin and end, the rows of a case a kernel can lose, the Keras form
of Adam in fp64 with the wrong rules a test must tell apart from it, a reader of the learner file, the dead-unit networks. The fp64
references of a case are computed once and shared. No test in here, no GPU."""
import functools
import struct

import numpy as np

from learner_util import F32, data, learner_file_header, make_net, numpy_forward64, numpy_loss_and_grads64

# csrc/mppi_learner.hip: 256 rows per workgroup of the forward pass, 64 per wave, 512-row chunks of the gradient GEMM, four waves on
# interleaved row pairs (stride 8). csrc/mppi_learner_wide.hip: 64-row tiles of two 32-row waves, 32-sample slabs, 512-sample chunks.
N_NARROW = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
N_WIDE = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)
DIMS_NARROW = ([1, 1], [32, 32], [1, 32, 1], [32, 1, 32], [5, 32, 32, 3], [32, 32, 32, 32, 32], [16, 32, 32, 32, 13])
DIMS_WIDE = ([1, 256, 256, 1], [31, 256, 256, 31], [32, 256, 256, 32], [9, 256, 256, 6])
FAMILY = dict(narrow=dict(ns=N_NARROW, dims=DIMS_NARROW, n_of_dims=(1, 9, 257, 513), units=(2, 8, 64, 256, 512)),
              wide=dict(ns=N_WIDE, dims=DIMS_WIDE, n_of_dims=(1, 33, 65, 513), units=(32, 64, 512)))

# the suite's bars (tests/test_learner_gpu.py, tests/test_learner_wide_gpu.py)
LOSS_RTOL = 2e-6     # loss, relative
UPDATE_BAR = 3e-7    # one Adam step from the device's own gradients, absolute (weights below 1)
PRED_FLOOR = 1e-6    # floor of the forward-pass bar, relative to max|pred|

# seeds of the cases whose default seed misses a condition of the oracle file (named there): id -> seed
SEEDS = {"narrow-1x1-n63": 2126, "narrow-1x1-n511": 33150, "narrow-5x32x32x3-n1024": 2166, "narrow-1x1-n9": 1172,
         "narrow-1x1-n257": 10174, "narrow-1x1-n513": 78176, "narrow-1x32x1-n257": 1190,
         "wide-9x256x256x6-n1025": 1156}


def case_id(family, dims, n):
    return "%s-%s-n%d" % (family, "x".join(str(d) for d in dims), n)


def _family_cases(family):
    f = FAMILY[family]
    pairs, others = [], f["dims"][:-1]
    for i, n in enumerate(f["ns"]):  # every n with the family's last dims and with one other, rotating
        pairs += [(f["dims"][-1], n), (others[i % len(others)], n)]
    for dims in f["dims"]:
        pairs += [(dims, n) for n in f["n_of_dims"]]
    out, seen = [], set()
    for dims, n in pairs:
        cid = case_id(family, dims, n)
        if cid not in seen:
            seen.add(cid)
            out.append(dict(id=cid, family=family, dims=list(dims), n=n, seed=SEEDS.get(cid, 100 + 2 * len(out))))
    return out


NARROW_CASES = _family_cases("narrow")
WIDE_CASES = _family_cases("wide")
CASES = NARROW_CASES + WIDE_CASES


def probe_rows(family, n):
    """the rows a kernel can lose: the first, the last, and the two rows either side of every unit boundary below n"""
    rows = {0, n - 1}
    for u in FAMILY[family]["units"]:
        if u < n:
            rows |= {u - 1, u}
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = next(c for c in CASES if c["id"] == cid)
    dims, n = c["dims"], c["n"]
    net = make_net(dims, c["seed"])
    X, Y = data(dims, n, c["seed"] + 1)
    # a hidden layer of one unit: its bias is raised until the unit is live on every probe row (a dead unit's row gives no gradient to
    # lose); rows that are no probes may still be dead
    rows = probe_rows(c["family"], n)
    for l in range(len(dims) - 2):
        if dims[l + 1] == 1:
            z = numpy_forward64(net, X[rows])[1][l][:, 0] - float(net["b"][l][0])
            net["b"][l][0] = F32(1.0 - z.min())
            if l + 2 == len(dims) - 1:  # its delta is ONE sum over the outputs: the probe rows' errors are given the signs that add up
                Y[rows] = -np.abs(Y[rows]) * np.sign(net["W"][l + 1][0])
    if min(dims) == 1:  # a layer of one unit: one number per row carries everything, so the probe rows' targets are made four times as large
        Y[rows] *= F32(4.0)
    for a in net["W"] + net["b"] + [X, Y]:
        a.setflags(write=False)
    return net, X, Y


def inputs(case):
    """(net, X, Y) of a case; shared, read-only"""
    return _inputs(case["id"])


@functools.lru_cache(maxsize=None)
def _reference(cid):
    net, X, Y = _inputs(cid)
    loss, gW, gb = numpy_loss_and_grads64(net, X, Y)
    pred = numpy_forward64(net, X)[0]
    return dict(loss=loss, W=gW, b=gb, pred=pred)


def reference(case):
    """loss, gradients and predictions of a case in fp64 numpy; shared"""
    return _reference(case["id"])


@functools.lru_cache(maxsize=None)
def _pred_bar(cid):
    from learner_util import torch_forward
    net, X, _ = _inputs(cid)
    p64 = _reference(cid)["pred"]
    return max(4.0 * float(np.abs(torch_forward(net, X) - p64).max()), PRED_FLOOR * float(np.abs(p64).max()))


def pred_bar(case):
    """the forward-pass bar of a case, per element: 4 x the distance of torch CPU fp32's forward pass from fp64 on that case (the margin
    the suite gives fp32 kernels elsewhere), at least 1e-6 of the largest prediction"""
    return _pred_bar(case["id"])


def row_contribution(case, row):
    """what a gradient loses when `row` is dropped and the 1/n normalisation kept: that row's own term, in fp64"""
    net, X, Y = inputs(case)
    _, gW, gb = numpy_loss_and_grads64(net, X[row:row + 1], Y[row:row + 1])  # normalised by 1 x n_out
    return [g / case["n"] for g in gW], [g / case["n"] for g in gb]


def tensors(g):
    """(name, array) of every gradient tensor of dict(W=[...], b=[...])"""
    return [("%s%d" % (k, l), np.asarray(a)) for k in ("W", "b") for l, a in enumerate(g[k])]


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------
LR = 1e-2
HP_SETS = ((0.9, 0.999, 1e-7), (0.0, 0.999, 1e-7), (0.5, 0.9, 1e-2), (0.95, 0.5, 1e-4))  # no eps = 0: a dead unit gives Keras itself 0/0
DEFAULT_HP = HP_SETS[0]
ADAM_T = (1, 2, 3, 10)
ADAM_DIMS = dict(narrow=[9, 16, 6], wide=[9, 256, 256, 6])
ADAM_N = 333


def as_fp32(values):
    """what the device receives of these hyper-parameters: each rounded to fp32, as a Python float"""
    return tuple(float(F32(v)) for v in values)


def adam_moments64(m, v, g, b1, b2):
    m, v, g = (np.asarray(a, np.float64) for a in (m, v, g))
    return b1 * m + (1.0 - b1) * g, b2 * v + (1.0 - b2) * g * g


def adam_step64(w, m, v, g, t, lr, b1, b2, eps):
    """tf.keras.optimizers.Adam in fp64: w - lr sqrt(1 - b2^t) / (1 - b1^t) m' / (sqrt(v') + eps) -> w', m', v'"""
    m1, v1 = adam_moments64(m, v, g, b1, b2)
    with np.errstate(all="ignore"):
        return np.asarray(w, np.float64) - lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) * m1 / (np.sqrt(v1) + eps), m1, v1


def _eps_in_torchs_place(w, m, v, g, t, lr, b1, b2, eps):
    m1, v1 = adam_moments64(m, v, g, b1, b2)
    return np.asarray(w, np.float64) - lr * (m1 / (1.0 - b1 ** t)) / (np.sqrt(v1 / (1.0 - b2 ** t)) + eps), m1, v1


# the wrong rules: each takes adam_step64's arguments
ALTERNATIVES = {
    "eps in PyTorch's place": _eps_in_torchs_place,
    "eps at the default": lambda w, m, v, g, t, lr, b1, b2, eps: adam_step64(w, m, v, g, t, lr, b1, b2, DEFAULT_HP[2]),
    "beta1 and beta2 swapped": lambda w, m, v, g, t, lr, b1, b2, eps: adam_step64(w, m, v, g, t, lr, b2, b1, eps),
    "t + 1": lambda w, m, v, g, t, lr, b1, b2, eps: adam_step64(w, m, v, g, t + 1, lr, b1, b2, eps),
    "t - 1": lambda w, m, v, g, t, lr, b1, b2, eps: adam_step64(w, m, v, g, t - 1, lr, b1, b2, eps),
    "all three at the defaults": lambda w, m, v, g, t, lr, b1, b2, eps: adam_step64(w, m, v, g, t, lr, *DEFAULT_HP),
}


def distance(a, b):
    """the largest |a - b|; infinite where either is not finite (t - 1 = 0 divides by zero)"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(np.where(np.isfinite(d), d, np.inf).max())


def ulps(got, expected):
    """the distance in fp32 units in the last place, per element (the integer image of conftest.assert_float_eq)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(got) - key(expected))


# ---- the learner file (include/mppi_c.h; learner_util.learner_file_header) ---------------------------------------------------------------
FILE_KEYS = ("W", "b", "mW", "mb", "vW", "vb")
STEP_OFFSET = 8 + 4 * 6  # magic, n_layers, widths[5], then the Adam step


def read_learner_file(path):
    """what mppi_learner_save wrote -> dict(widths, step, has_norm, W, b, mW, mb, vW, vb): per layer the compact [in][out] fp32 arrays"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"MPPILRN1", raw[:8]
    n_layers, *rest = struct.unpack("<8i", raw[8:40])
    widths, step, has_norm = list(rest[:n_layers + 1]), rest[5], rest[6]
    assert raw[:40] == learner_file_header(widths, n_layers, step, has_norm)
    out = dict(widths=widths, step=step, has_norm=has_norm, **{k: [] for k in FILE_KEYS})
    at = 40
    for l in range(n_layers):
        i, o = widths[l], widths[l + 1]
        for kW, kb in (("W", "b"), ("mW", "mb"), ("vW", "vb")):
            out[kW].append(np.frombuffer(raw, "<f4", i * o, at).reshape(i, o).copy())
            out[kb].append(np.frombuffer(raw, "<f4", o, at + 4 * i * o).copy())
            at += 4 * (i + 1) * o
    assert len(raw) == at + (16 * (widths[0] + widths[-1]) if has_norm else 0)
    return out


def rewrite_step(src, dst, step):
    """a copy of the learner file `src` with only the header's step field changed"""
    raw = bytearray(open(src, "rb").read())
    raw[STEP_OFFSET:STEP_OFFSET + 4] = struct.pack("<i", step)
    with open(dst, "wb") as fh:
        fh.write(raw)


# ---- dead units ------------------------------------------------------------------------------------------------------------------------
DEAD_UNIT, ZERO_UNIT = 3, 5  # of the first hidden layer: no incoming weights; bias -1 (dead on every row) and bias 0 (pre-activation exactly 0)
DEAD_CASES = (dict(id="dead-narrow", dims=[16, 32, 32, 32, 13], n=257, seed=300), dict(id="dead-wide", dims=[9, 256, 256, 6], n=257, seed=302))


@functools.lru_cache(maxsize=None)
def _dead_inputs(cid):
    c = next(c for c in DEAD_CASES if c["id"] == cid)
    net = make_net(c["dims"], c["seed"])
    for unit, bias in ((DEAD_UNIT, -1.0), (ZERO_UNIT, 0.0)):
        net["W"][0][:, unit] = 0.0
        net["b"][0][unit] = bias
    X, Y = data(c["dims"], c["n"], c["seed"] + 1)
    for a in net["W"] + net["b"] + [X, Y]:
        a.setflags(write=False)
    return net, X, Y


def dead_inputs(case):
    return _dead_inputs(case["id"])


def unit_entries(g, unit):
    """the gradient (or weight) entries into and out of a unit of the first hidden layer"""
    return [g["W"][0][:, unit], g["b"][0][unit:unit + 1], g["W"][1][unit, :]]
