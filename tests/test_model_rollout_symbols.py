"""CPU-side checks of the open-loop model rollout (mppi_model_rollout, mppi_model_rollout_device): the header declares them with the
documented argument lists, the library exports them, the ctypes binding lists them, the ABI version stays 5, and Handle.model_rollout
checks its shapes before any library call; BatchHandle.model_rollout refuses. No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HOST_ARGS = ["mppi_handle *h", "const float *x0", "int kx", "const float *V", "int n", "int T", "float *X_out", "float *C_out"]
DEVICE_ARGS = ["mppi_handle *h", "const float *x0_dev", "int kx", "const float *V_dev", "int n", "int T", "float *X_dev", "float *C_dev",
               "void *stream"]
DECLS = {"mppi_model_rollout": HOST_ARGS, "mppi_model_rollout_device": DEVICE_ARGS}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_header_declares_the_rollout_entry_points():
    txt = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, want in DECLS.items():
        decl = re.search(r"mppi_status\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+5\b", txt)


def test_library_exports_and_binding_lists_them(pkg):
    from mppi_tf_amd import _lib
    lib = pkg.load()
    for name, want in DECLS.items():
        assert hasattr(lib, name), "libmppi_hip.so does not export " + name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == len(want)
    assert lib.mppi_abi_version() == 5


class _Stub:
    """stands where the loaded library would: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were checked" % name)


def _stub_of(cls, **attrs):
    h = cls.__new__(cls)
    h.lib, h.h = _Stub(), None
    for k, v in attrs.items():
        setattr(h, k, v)
    return h


def z(*shape):
    return np.zeros(shape, np.float32)


# (x0, V) for a handle of s = 4, a = 2
BAD = ((z(5), z(3, 2)), (z(4), z(3, 3)), (z(4), z(3, 5, 3)), (z(5, 5), z(3, 5, 2)),  # wrong s or a
       (z(4), z(6)), (z(4), z(2)),                                                  # a 1-D V
       (z(3, 4), z(3, 5, 2)), (z(6, 4), z(3, 5, 2)), (z(2, 4), z(3, 2)),            # x0 [m, s] with m not in {1, n}
       (z(4), z(0, 2)), (z(4), z(0, 5, 2)), (z(5, 4), z(0, 5, 2)),                  # T = 0
       (z(4), z(3, 0, 2)), (z(4), z(3, 5, 2, 1)), (z(1, 1, 4), z(3, 2)))


def test_model_rollout_checks_shapes_before_the_library(pkg):
    h = _stub_of(pkg.Handle, s=4, a=2)
    for x0, V in BAD:
        with pytest.raises(ValueError):
            h.model_rollout(x0, V)
        with pytest.raises(ValueError):
            h.model_rollout(x0, V, costs=False)


def test_good_calls_reach_the_entry_point(pkg):
    h = _stub_of(pkg.Handle, s=4, a=2)
    for x0, V in ((z(4), z(3, 2)), (z(1, 4), z(3, 2)), (z(4), z(3, 5, 2)), (z(1, 4), z(3, 5, 2)), (z(5, 4), z(3, 5, 2)), (z(4), z(1, 1, 2))):
        with pytest.raises(AssertionError, match=r"\(mppi_model_rollout\)"):
            h.model_rollout(x0, V)
    with pytest.raises(AssertionError, match=r"\(mppi_model_rollout_device\)"):
        h.model_rollout_device(0, 1, 0, 5, 3, 0)


def test_sample_trajectories_checks_before_the_library(pkg):
    h = _stub_of(pkg.Handle, s=4, a=2, tau=3, k=8, k_local=8)
    for ks in ([], [8], [-1], [0, 9]):
        with pytest.raises(ValueError):
            h.sample_trajectories(z(4), z(3, 2), ks)
    with pytest.raises(ValueError):
        h.sample_trajectories(z(4), z(4, 2), [0])


def test_batch_handle_refuses(pkg):
    hb = _stub_of(pkg.BatchHandle, n=3, s=4, a=2)
    with pytest.raises(pkg.MppiError, match="lone"):
        hb.model_rollout(z(4), z(3, 2))
