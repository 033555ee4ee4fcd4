"""CPU-side checks of the per-member batch parameters (no compute calls): the header declares mppi_create_batch_configs and the binding
matches it, BatchHandle takes the plural keywords, and the Python config builder gives n configs that differ only in the per-member
fields."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_header_declares_create_batch_configs_and_the_binding_matches(pkg):
    from mppi_tf_amd import _lib
    assert "mppi_create_batch_configs" in declared_functions()
    hdr = open(os.path.join(ROOT, "include", "mppi_c.h")).read()
    assert re.search(r"mppi_status\s+mppi_create_batch_configs\s*\(\s*const\s+mppi_config\s*\*\s*cfgs\s*,\s*int\s+n\s*,\s*mppi_handle\s*\*\*\s*out\s*\)\s*;", hdr)
    res, args = _lib.SIGNATURES["mppi_create_batch_configs"]
    assert res is C.c_int and args == [C.POINTER(_lib.Config), C.c_int, C.POINTER(_lib._H)]
    assert hasattr(pkg.load(), "mppi_create_batch_configs")
    # the ABI version and the existing entry point stay as they were
    assert "#define MPPI_ABI_VERSION 5" in hdr
    assert _lib.SIGNATURES["mppi_create_batch"][1] == [C.POINTER(_lib.Config), C.c_int, C.POINTER(C.c_uint64), C.POINTER(_lib._H)]


def test_batch_handle_takes_the_per_member_keywords(pkg):
    sig = inspect.signature(pkg.BatchHandle.__init__).parameters
    for kw in ("lams", "gammas", "upsilons", "sigmas", "Qs"):
        assert kw in sig and sig[kw].default is None, kw


def _contents(cfg, s, a):
    """the fields of one mppi_config, pointers replaced by what they point to"""
    d = {}
    for name, _ in cfg._fields_:
        v = getattr(cfg, name)
        if name == "sigma":
            v = None if not v else tuple(v[i] for i in range(a * a))
        elif name == "goal":
            v = None if not v else tuple(v[i] for i in range(s))
        elif name == "Q":
            v = None if not v else tuple(v[i] for i in range(s * s if cfg.q_is_full else s))
        elif name == "auv":
            v = None if not v else tuple((f, repr(getattr(v.contents, f))) for f, _ in v.contents._fields_ if f not in (
                "cog", "cob", "inertial", "added_mass", "linear_damping", "linear_damping_forward_speed", "quad_damping"))
        elif isinstance(v, C._Pointer) or name in ("mlp", "ellipse", "quat_Q", "ellipse3d"):
            v = bool(v)
        d[name] = v
    return d


def test_config_builder_differs_only_in_the_per_member_fields(pkg):
    from mppi_tf_amd import _lib
    n, a, s = 4, 3, 6
    lams = [0.1, 1.0, 3.0, 10.0]
    sigmas = [np.diag([0.1 * (i + 1)] * a) for i in range(n)]
    Qs = [np.full(s, 1.0 + i, np.float32) for i in range(n)]
    cfgs, keep = _lib.batch_configs(n, 4096, 64, s, a, goal=np.arange(s), action_cost=_lib.ACTION_COST_PY, upsilon_scales_noise=True,
                                    gamma=0.5, upsilons=[1.0, 1.5, 2.0, 2.5], lams=lams, sigmas=sigmas, Qs=Qs, seed=7)
    assert len(cfgs) == n
    per = {"lam", "upsilon", "sigma", "Q", "seed"}
    c0 = _contents(cfgs[0], s, a)
    for i in range(n):
        ci = _contents(cfgs[i], s, a)
        assert {k for k in c0 if c0[k] != ci[k]} <= per, i
        assert cfgs[i].lam == pytest.approx(lams[i]) and cfgs[i].upsilon == pytest.approx(1.0 + 0.5 * i) and cfgs[i].seed == 7 + i
        assert ci["sigma"] == pytest.approx(tuple(np.ravel(sigmas[i]))) and ci["Q"] == pytest.approx(tuple(Qs[i]))
        assert cfgs[i].gamma == pytest.approx(0.5) and cfgs[i].flags == 1 and cfgs[i].action_cost_kind == _lib.ACTION_COST_PY
        assert cfgs[i].struct_size == C.sizeof(_lib.Config) and cfgs[i].q_is_full == 0
    # dense Q per member; explicit seeds; the AUV model's descriptor shared by content
    from mppi_tf_amd.auv import auv_task
    t = auv_task(8)
    cfgs, keep = _lib.batch_configs(2, 1024, 8, 13, 6, auv=t["auv"], sigma=t["sigma"], seeds=[5, 9],
                                    Qs=[np.diag(t["Q"]), np.diag(t["Q"]) + 0.1], lams=[0.5, 2.0])
    assert [c.seed for c in cfgs] == [5, 9] and all(c.q_is_full == 1 and c.model_kind == _lib.MODEL_AUV for c in cfgs)
    c0, c1 = _contents(cfgs[0], 13, 6), _contents(cfgs[1], 13, 6)
    assert {k for k in c0 if c0[k] != c1[k]} == {"lam", "Q", "seed"}


def test_lone_and_batch_configs_come_from_one_filler(pkg, monkeypatch):
    """For the same shared keywords, the config Handle.__init__ passes to mppi_create and member 0 of batch_configs(...) have equal
    contents: both come from _fill_config. mppi_create is replaced by a recorder that answers MPPI_ERR_NO_DEVICE (no GPU is used)."""
    from mppi_tf_amd import _lib
    from mppi_tf_amd.auv import auv_task
    lib, seen = _lib.load(), []

    def recorder(s, a):
        def create(cfg, out):
            seen.append(_contents(cfg._obj, s, a))
            return _lib.ERR_NO_DEVICE
        return create
    rng = np.random.default_rng(3)
    L = rng.uniform(-0.3, 0.3, (6, 6)) + np.eye(6)
    t = auv_task(8)
    cases = [(6, 3, dict(k=4096, tau=64, s_dim=6, a_dim=3, dt=0.05, mass=2.0, lam=0.3, gamma=0.5, upsilon=1.5, sigma=np.diag([0.1, 0.2, 0.3]),
                         goal=np.arange(6), Q=(L @ L.T).astype(np.float32), action_cost=_lib.ACTION_COST_PY, upsilon_scales_noise=True, seed=7)),
             (13, 6, dict(k=1024, tau=8, s_dim=13, a_dim=6, dt=0.1, lam=0.5, sigma=t["sigma"], Q=t["Q"], auv=t["auv"], seed=5))]
    for s, a, kw in cases:
        monkeypatch.setattr(lib, "mppi_create", recorder(s, a))
        with pytest.raises(_lib.MppiError) as e:
            _lib.Handle(**kw)
        assert e.value.status == _lib.ERR_NO_DEVICE
        monkeypatch.undo()
        lone = seen.pop()
        assert not seen
        keep = []
        assert _contents(_lib._fill_config(lib, keep, **kw), s, a) == lone  # the filler, called on its own
        cfgs, keep = _lib.batch_configs(2, **kw)
        assert _contents(cfgs[0], s, a) == lone
        assert lone["sigma"] is not None and lone["Q"] is not None and lone["seed"] == kw["seed"]
    assert lone["model_kind"] == _lib.MODEL_AUV and lone["auv"] is not None
    assert not hasattr(_lib, "_batch_config")


def test_config_builder_checks_the_list_lengths(pkg):
    from mppi_tf_amd import _lib
    for kw in (dict(lams=[1.0]), dict(gammas=[1.0] * 3), dict(upsilons=[]), dict(sigmas=[np.eye(2)] * 3), dict(Qs=[np.ones(4)]),
               dict(seeds=[1, 2, 3])):
        with pytest.raises(_lib.MppiError) as e:
            _lib.batch_configs(2, 256, 16, 4, 2, **kw)
        assert e.value.status == _lib.ERR_INVALID_ARG, kw
