"""The boundary of the batched learned point-mass controllers without a GPU: mppi_create_batch_mlp is declared, exported and bound with the
creators' signature, the ABI version stays 5, the library carries the two batched kernels, and BatchHandle.learned(model="mlp") checks
the networks' shapes before any device work."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, has_gpu
from episode_util import make_nnauv


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_the_creator_is_declared_exported_and_bound(pkg):
    from mppi_tf_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_c.h")).read(), flags=re.S)
    assert re.search(r"mppi_status\s+mppi_create_batch_mlp\s*\(\s*const\s+mppi_config\s*\*\s*cfgs\s*,\s*int\s+n\s*,\s*mppi_handle\s*\*\*\s*out\s*\)\s*;", txt)
    lib = pkg.load()
    assert hasattr(lib, "mppi_create_batch_mlp")
    assert _lib.SIGNATURES["mppi_create_batch_mlp"] == _lib.SIGNATURES["mppi_create_batch_learned"] == _lib.SIGNATURES["mppi_create_batch_configs"]
    assert lib.mppi_abi_version() == 5
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "mppi_c.h")).read())


def test_the_library_carries_the_batched_kernels(pkg):
    blob = open(os.path.join(ROOT, "mppi-tf_amd", "libmppi_hip.so"), "rb").read()
    for kernel in (b"k_rollout_mlp2_batch", b"k_rollout_mlp_small_batch"):
        assert kernel in blob, kernel


def test_learned_takes_the_mlp_model_and_checks_shapes_before_the_device(pkg):
    a = 2
    good = make_nnauv(1, 32, 2, 3 * a, 2 * a)
    kw = dict(k=64, tau=4)
    # the model and a_dim
    with pytest.raises(ValueError, match="a_dim"):
        pkg.BatchHandle.learned(2, good, "mlp", **kw)
    with pytest.raises(ValueError, match='"mlp"'):
        pkg.BatchHandle.learned(2, good, "point_mass", a_dim=a, **kw)
    with pytest.raises(ValueError, match="a_dim = 6"):
        pkg.BatchHandle.learned(2, good, "nnauv", a_dim=a, **kw)
    # the first kernel's rows, the last one's columns, a chain that does not link, a bias of another width: named by member
    cases = {"inputs": make_nnauv(1, 32, 2, 3 * a + 1, 2 * a), "outputs": make_nnauv(1, 32, 2, 3 * a, 2 * a + 2),
             "chain": dict(good, W=[good["W"][0], good["W"][1][:16], good["W"][2]]),
             "bias": dict(good, b=[good["b"][0][:8]] + good["b"][1:])}
    for name, bad in cases.items():
        with pytest.raises(ValueError, match=r"nets\[1\]"):
            pkg.BatchHandle.learned(2, [good, bad], "mlp", a_dim=a, **kw)
    # every member's network has one shape
    with pytest.raises(ValueError, match=r"nets\[1\].*shape of the first"):
        pkg.BatchHandle.learned(2, [good, make_nnauv(2, 16, 2, 3 * a, 2 * a)], "mlp", a_dim=a, **kw)
    with pytest.raises(pkg.MppiError, match="nets must hold n = 3"):
        pkg.BatchHandle.learned(3, [good, good], "mlp", a_dim=a, **kw)
    if not has_gpu():  # good shapes get as far as the device
        with pytest.raises(pkg.MppiError) as e:
            pkg.BatchHandle.learned(2, good, "mlp", a_dim=a, **kw)
        assert e.value.status == 2 and "no CPU path" in str(e.value)
