"""CPU-side checks of the closed-loop episode entry points (mppi_run_episode, mppi_batch_run_episode): the header declares them, the
library exports them, the ctypes binding lists them, and the Python wrappers check their shapes before any library call. No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("mppi_run_episode", "mppi_batch_run_episode")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_header_declares_the_episode_entry_points():
    txt = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        decl = re.search(r"mppi_status\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared"
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == 9 and args[0] == "mppi_handle *h" and args[2] == "int n_x" and args[3] == "int n_steps", args
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+5\b", txt)


def test_library_exports_and_binding_lists_them(pkg):
    from mppi_tf_amd import _lib
    lib = pkg.load()
    for name in NAMES:
        assert hasattr(lib, name), "libmppi_hip.so does not export " + name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == 9
    assert lib.mppi_abi_version() == 5
    assert callable(pkg.Handle.run_episode) and callable(pkg.BatchHandle.run_episode)


class _Stub:
    """stands where the loaded library would: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the shapes were checked" % name)


def _stub_of(cls, **attrs):
    h = cls.__new__(cls)
    h.lib, h.h = _Stub(), None
    for k, v in attrs.items():
        setattr(h, k, v)
    return h


def test_wrappers_check_shapes_before_the_library(pkg):
    z = lambda *shape: np.zeros(shape, np.float32)
    h = _stub_of(pkg.Handle, s=4, a=2)
    for args in ((z(5), 3), (z(1, 4), 3), (z(4), 0), (z(4), 3, z(3, 5)), (z(4), 3, z(2, 4)), (z(4), 3, z(3, 1, 4)),
                 (z(4), 3, None, z(4, 4)), (z(4), 3, None, z(3, 3)), (z(4), 3, z(3, 4), z(12))):
        with pytest.raises(ValueError):
            h.run_episode(*args)
    hb = _stub_of(pkg.BatchHandle, n=3, s=4, a=2)
    for args in ((z(4), 2), (z(2, 4), 2), (z(3, 5), 2), (z(12), 2), (z(3, 4), -1), (z(3, 4), 2, z(2, 4)), (z(3, 4), 2, z(3, 3, 4)),
                 (z(3, 4), 2, z(2, 3, 5)), (z(3, 4), 2, None, z(2, 2, 4)), (z(3, 4), 2, None, z(2, 12))):
        with pytest.raises(ValueError):
            hb.run_episode(*args)
    # a good shape reaches the library (here: the stub)
    with pytest.raises(AssertionError, match="mppi_run_episode"):
        h.run_episode(z(4), 3, z(3, 4), z(3, 4))
    with pytest.raises(AssertionError, match="mppi_batch_run_episode"):
        hb.run_episode(z(3, 4), 2, z(2, 3, 4), z(2, 3, 4))
