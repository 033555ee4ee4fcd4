"""The wide learner's boundary without a GPU: the new entry point is declared, exported and bound; the file header accepts the
[in, 256, 256, out] shape and nothing else beyond widths <= 32; mppi_learner_create checks the shape before the device; and
NNPointMassModel's data preparation is the formula mppi_c.h states for MPPI_MODEL_MLP."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from learner_util import REFUSED_SHAPES, learner_file_header, make_net


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_gradients_entry_point_is_declared_exported_and_bound(pkg):
    txt = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"mppi_status\s+mppi_learner_gradients\s*\(\s*mppi_learner\s*\*\s*l\s*,\s*float\s*\*\s*loss_out\s*,\s*float\s*\*\s*const\s*\*\s*dW\s*,"
                     r"\s*float\s*\*\s*const\s*\*\s*db\s*\)", txt)
    from mppi_tf_amd import _lib
    assert hasattr(pkg.load(), "mppi_learner_gradients") and "mppi_learner_gradients" in _lib.SIGNATURES
    assert pkg.load().mppi_abi_version() == 5


def peek(pkg, path):
    lib = pkg.load()
    n, w = C.c_int(0), (C.c_int32 * 5)()
    st = lib.mppi_learner_peek(os.fsencode(str(path)), C.byref(n), w)
    return st, n.value, [int(v) for v in w]


def test_peek_accepts_the_wide_shape_and_nothing_else_new(pkg, tmp_path):
    f = tmp_path / "hdr"
    f.write_bytes(learner_file_header([9, 256, 256, 6, 0]))
    assert peek(pkg, f) == (0, 3, [9, 256, 256, 6, 0])
    f.write_bytes(learner_file_header([16, 32, 32, 32, 13]))
    assert peek(pkg, f) == (0, 4, [16, 32, 32, 32, 13])
    for widths in ([9, 64, 64, 6, 0], [9, 256, 32, 6, 0], [9, 256, 6, 0, 0], [40, 256, 256, 6, 0], [9, 256, 256, 40, 0]):
        f.write_bytes(learner_file_header(widths))
        assert peek(pkg, f)[0] == 7, widths
    f.write_bytes(learner_file_header([9, 256, 256, 256, 6]))
    assert peek(pkg, f)[0] == 7


def test_create_checks_the_shape_before_the_device(pkg):
    for dims in REFUSED_SHAPES:
        with pytest.raises(pkg.MppiError) as e:
            pkg.Learner(make_net(dims))
        assert e.value.status == 4, dims
    if not has_gpu():  # a legal wide shape gets as far as the device
        with pytest.raises(pkg.MppiError) as e:
            pkg.Learner(make_net([9, 256, 256, 6]))
        assert e.value.status == 2 and "no CPU path" in str(e.value)


@pytest.mark.parametrize("a", [1, 3])
@pytest.mark.parametrize("norm", [False, True])
def test_point_mass_training_pairs_are_the_stated_formula(pkg, a, norm):
    """X = concat(x, u) [n, s+a], Y = x' - x [n, s], normalised with the model's statistics when asked"""
    s, n = 2 * a, 17
    rng = np.random.default_rng(a)
    x, xn, u = rng.standard_normal((n, s, 1)), rng.standard_normal((n, s, 1)), rng.standard_normal((n, a, 1))
    model = pkg.NNPointMassModel(stateDim=s, actionDim=a)
    assert model.get_state_dim() == s and model.get_action_dim() == a
    assert [w.shape for w in model.get_weights()] == [(s + a, 256), (256,), (256, 256), (256,), (256, s), (s,)]
    assert all(not b.any() for b in model.get_weights()[1::2])
    xm, xs, ym, ys = rng.standard_normal(s + a), rng.uniform(0.5, 2.0, s + a), rng.standard_normal(s), rng.uniform(0.5, 2.0, s)
    model.set_Xmean_Xstd(xm, xs)
    model.set_Ymean_Ystd(ym, ys)
    X, Y = model.prepare_training_data(x, xn, u, norm=norm)
    Xr, Yr = np.concatenate([x[..., 0], u[..., 0]], axis=1), (xn - x)[..., 0]
    if norm:
        Xr, Yr = (Xr - xm) / xs, (Yr - ym) / ys
    assert X.shape == (n, s + a) and Y.shape == (n, s)
    np.testing.assert_array_equal(X, Xr)
    np.testing.assert_array_equal(Y, Yr)
    np.testing.assert_array_equal(model.prepare_data(x, u), (np.concatenate([x[..., 0], u[..., 0]], axis=1) - xm) / xs)
    np.testing.assert_allclose(model.denormalizeY((Yr - ym) / ys if not norm else Yr), (xn - x)[..., 0], rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        pkg.NNPointMassModel(stateDim=4, actionDim=2, hidden=(64, 64))
    with pytest.raises(ValueError):
        pkg.NNPointMassModel(stateDim=5, actionDim=2)
