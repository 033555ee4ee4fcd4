"""CPU-side checks of the step-statistics entry points (mppi_step_stats, mppi_batch_step_stats, mppi_run_episode_stats,
mppi_batch_run_episode_stats): the header declares them, the library exports them, the ctypes binding lists them, and
run_episode(..., stats=True) checks its shapes before any library call and reaches the entry point it names. No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LAST = ("mppi_step_stats", "mppi_batch_step_stats")
EPISODE = ("mppi_run_episode_stats", "mppi_batch_run_episode_stats")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in [(n, 4) for n in LAST] + [(n, 14) for n in EPISODE]:
        decl = re.search(r"mppi_status\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared"
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert len(args) == n_args and args[0] == "mppi_handle *h", args
        assert args[-3:] == ["float *%s" % ("stats" if n_args == 4 else "S_out"), "uint32_t *%s" % ("hist_cost" if n_args == 4 else "Hc_out"),
                             "uint32_t *%s" % ("hist_weight" if n_args == 4 else "Hw_out")], args
        if n_args == 14:
            assert args[1:3] == ["mppi_handle *const *plants", "int n_plants"] and args[4:6] == ["int n_x", "int n_steps"], args
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+5\b", txt)
    assert re.search(r"#define\s+MPPI_N_STEP_STATS\s+9\b", txt) and re.search(r"#define\s+MPPI_STEP_STAT_BINS\s+32\b", txt)
    enum = re.search(r"enum\s*\{\s*MPPI_STAT_BETA\s*=\s*0(.*?)\}", txt, flags=re.S).group(0)
    names = re.findall(r"MPPI_STAT_([A-Z_]+)\s*=\s*(\d+)", enum)
    assert names == [(n.upper(), str(i)) for i, n in enumerate(
        ("beta", "eta", "ess", "entropy", "cost_mean", "cost_std", "cost_max", "best_index", "n_nonfinite"))], names


def test_library_exports_and_binding_lists_them(pkg):
    from mppi_tf_amd import _lib
    lib = pkg.load()
    for name in LAST + EPISODE:
        assert hasattr(lib, name), "libmppi_hip.so does not export " + name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == (4 if name in LAST else 14)
        assert args[-2] is _lib.UP and args[-1] is _lib.UP and args[-3] is _lib.FP
    assert lib.mppi_abi_version() == 5
    assert (_lib.N_STEP_STATS, _lib.STEP_STAT_BINS) == (9, 32)
    for cls in (pkg.Handle, pkg.BatchHandle):
        assert callable(cls.step_stats)
    assert callable(pkg.ControllerBase.step_stats)
    assert pkg.StepStats._fields == ("beta", "eta", "ess", "entropy", "cost_mean", "cost_std", "cost_max", "best_index", "n_nonfinite",
                                     "hist_cost", "hist_weight", "k")


def test_step_stats_record_keeps_the_bits(pkg):
    S = np.arange(2 * 3 * 9, dtype=np.float32).reshape(2, 3, 9) + np.float32(0.25)
    Hc, Hw = np.ones((2, 3, 32), np.uint32), np.zeros((2, 3, 32), np.uint32)
    st = pkg.StepStats.from_rows(S, Hc, Hw, 256)
    assert st.k == 256 and st.ess.shape == (2, 3) and st.ess.dtype == np.float32 and st.hist_cost.shape == (2, 3, 32)
    np.testing.assert_array_equal(st.cost_max, S[..., 6])
    assert st.best_index.dtype.kind == "i" and st.n_nonfinite.dtype.kind == "i"
    np.testing.assert_array_equal(st.best_index, S[..., 7].astype(np.int64))
    lone = pkg.StepStats.from_rows(S[0, 0], Hc[0, 0], Hw[0, 0], 64)
    assert np.shape(lone.beta) == () and lone.hist_weight.shape == (32,)


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


def test_stats_episodes_check_shapes_before_the_library(pkg):
    z = lambda *shape: np.zeros(shape, np.float32)
    h = _stub_of(pkg.Handle, s=4, a=2, k_local=64)
    plant = _stub_of(pkg.Handle, s=4, a=2, k_local=1)
    for args in ((z(5), 3), (z(1, 4), 3), (z(4), 0), (z(4), 3, z(3, 5)), (z(4), 3, z(2, 4)), (z(4), 3, None, z(4, 4)), (z(4), 3, z(3, 4), z(12))):
        with pytest.raises(ValueError):
            h.run_episode(*args, stats=True)
    for bad_plant in ("a plant", [plant, plant], 3):
        with pytest.raises(ValueError):
            h.run_episode(z(4), 3, plant=bad_plant, stats=True)
    hb = _stub_of(pkg.BatchHandle, n=3, s=4, a=2, k_local=64)
    for args in ((z(4), 2), (z(2, 4), 2), (z(3, 5), 2), (z(3, 4), -1), (z(3, 4), 2, z(2, 4)), (z(3, 4), 2, z(2, 3, 5)), (z(3, 4), 2, None, z(2, 12))):
        with pytest.raises(ValueError):
            hb.run_episode(*args, stats=True)
    with pytest.raises(ValueError):
        hb.run_episode(z(3, 4), 2, plant=[plant, plant], stats=True)
    # a good shape reaches the entry point it names: the _stats one with stats=True, with or without a plant; today's without
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode_stats\)"):
        h.run_episode(z(4), 3, z(3, 4), z(3, 4), stats=True)
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode_stats\)"):
        h.run_episode(z(4), 3, plant=plant, stats=True)
    with pytest.raises(AssertionError, match=r"\(mppi_batch_run_episode_stats\)"):
        hb.run_episode(z(3, 4), 2, z(2, 3, 4), z(2, 3, 4), stats=True)
    with pytest.raises(AssertionError, match=r"\(mppi_batch_run_episode_stats\)"):
        hb.run_episode(z(3, 4), 2, plant=[plant] * 3, stats=True)
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode\)"):
        h.run_episode(z(4), 3, z(3, 4), z(3, 4))
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode\)"):
        h.run_episode(z(4), 3, stats=False)
    with pytest.raises(AssertionError, match=r"\(mppi_run_episode_plant\)"):
        h.run_episode(z(4), 3, plant=plant)
    with pytest.raises(AssertionError, match=r"\(mppi_batch_run_episode\)"):
        hb.run_episode(z(3, 4), 2)
    with pytest.raises(AssertionError, match=r"\(mppi_step_stats\)"):
        h.step_stats()
    with pytest.raises(AssertionError, match=r"\(mppi_batch_step_stats\)"):
        hb.step_stats()
