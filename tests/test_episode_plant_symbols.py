"""CPU-side checks of the closed-loop episode against a separate plant (mppi_run_episode_plant, mppi_batch_run_episode_plant): the
header declares them, the library exports them, the ctypes binding lists them, and the Python wrappers check their shapes and the plant
count before any library call; without a plant the wrappers call the entry points they called before. No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("mppi_run_episode_plant", "mppi_batch_run_episode_plant")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_header_declares_the_plant_entry_points():
    txt = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        decl = re.search(r"mppi_status\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared"
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert len(args) == 11, args
        assert args[:6] == ["mppi_handle *h", "mppi_handle *const *plants", "int n_plants", "const float *x0", "int n_x", "int n_steps"], args
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+5\b", txt)


def test_library_exports_and_binding_lists_them(pkg):
    from mppi_tf_amd import _lib
    lib = pkg.load()
    for name in NAMES:
        assert hasattr(lib, name), "libmppi_hip.so does not export " + name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == 11
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


# the bad shapes of the plain wrappers' test (test_episode_symbols.py), which a plant does not excuse
BAD_LONE = ((z(5), 3), (z(1, 4), 3), (z(4), 0), (z(4), 3, z(3, 5)), (z(4), 3, z(2, 4)), (z(4), 3, z(3, 1, 4)),
            (z(4), 3, None, z(4, 4)), (z(4), 3, None, z(3, 3)), (z(4), 3, z(3, 4), z(12)))
BAD_BATCH = ((z(4), 2), (z(2, 4), 2), (z(3, 5), 2), (z(12), 2), (z(3, 4), -1), (z(3, 4), 2, z(2, 4)), (z(3, 4), 2, z(3, 3, 4)),
             (z(3, 4), 2, z(2, 3, 5)), (z(3, 4), 2, None, z(2, 2, 4)), (z(3, 4), 2, None, z(2, 12)))


def test_wrappers_check_plants_and_shapes_before_the_library(pkg):
    h = _stub_of(pkg.Handle, s=4, a=2)
    hb = _stub_of(pkg.BatchHandle, n=3, s=4, a=2)
    p = [_stub_of(pkg.Handle, s=4, a=2) for _ in range(4)]
    for args in BAD_LONE:
        with pytest.raises(ValueError):
            h.run_episode(*args, plant=p[0])
    for args in BAD_BATCH:
        with pytest.raises(ValueError):
            hb.run_episode(*args, plant=p[0])
        with pytest.raises(ValueError):
            hb.run_episode(*args, plant=p[:3])
    # a plant list of the wrong length, a plant that is no Handle
    for bad in (p[:2], [], (p[0], p[1])):
        with pytest.raises(ValueError, match="plant"):
            h.run_episode(z(4), 3, plant=bad)
    for bad in (p[:2], p[:4], []):
        with pytest.raises(ValueError, match="plant"):
            hb.run_episode(z(3, 4), 2, plant=bad)
    for bad in (hb, 7, "plant", [p[0], None, p[1]], [hb, hb, hb], np.zeros(3)):
        with pytest.raises(ValueError, match="plant"):
            hb.run_episode(z(3, 4), 2, plant=bad)
    for bad in (hb, 7, [None], object()):
        with pytest.raises(ValueError, match="plant"):
            h.run_episode(z(4), 3, plant=bad)
    with pytest.raises(TypeError):
        h.run_episode(z(4), 3, None, None, p[0])  # keyword only


def test_good_calls_reach_the_entry_point_they_name(pkg):
    h = _stub_of(pkg.Handle, s=4, a=2)
    hb = _stub_of(pkg.BatchHandle, n=3, s=4, a=2)
    p = [_stub_of(pkg.Handle, s=4, a=2) for _ in range(3)]
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode_plant\)"):
        h.run_episode(z(4), 3, z(3, 4), z(3, 4), plant=p[0])
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode_plant\)"):
        h.run_episode(z(4), 3, plant=[p[0]])
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode_plant\)"):
        h.run_episode(z(4), 3, plant=h)
    for plant in (p[0], p, tuple(p), [p[1]]):
        with pytest.raises(AssertionError, match=r"\(mppi_batch_run_episode_plant\)"):
            hb.run_episode(z(3, 4), 2, z(2, 3, 4), z(2, 3, 4), plant=plant)
    # without a plant: the entry points of before
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode\)"):
        h.run_episode(z(4), 3, z(3, 4), z(3, 4))
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode\)"):
        h.run_episode(z(4), 3, plant=None)
    with pytest.raises(AssertionError, match=r"\(mppi_batch_run_episode\)"):
        hb.run_episode(z(3, 4), 2, z(2, 3, 4), z(2, 3, 4))
