"""CPU-side checks of the batched AUV controllers (no compute calls): the library carries the batched AUV rollout kernel and BatchHandle
takes the 13-state model and costs with Handle's keywords."""
import inspect

import pytest


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_library_carries_the_batched_auv_kernel(pkg):
    from mppi_tf_amd import _lib
    blob = open(_lib.SO_PATH, "rb").read()
    assert b"k_rollout_auv_pc_batch" in blob
    assert b"k_finish_cols_batchILi6E" in blob  # k_finish_cols_batch<6>


def test_batch_handle_takes_the_13_state_keywords(pkg):
    sig = inspect.signature(pkg.BatchHandle.__init__).parameters
    hsig = inspect.signature(pkg.Handle.__init__).parameters
    for kw in ("auv", "quat_cost", "ellipse3d"):
        assert kw in sig, kw
        assert sig[kw].default == hsig[kw].default, kw


def test_13_state_config_is_filled_alike(pkg):
    """BatchHandle and Handle fill the AUV / StaticQuatCost / ElipseCost3D fields of mppi_config through the same helper"""
    import numpy as np
    from mppi_tf_amd import _lib
    from mppi_tf_amd.auv import auv_task
    cfg, keep = _lib.Config(), []
    Q = _lib._fill_13state(cfg, keep, auv_task(8)["auv"], True, None, np.ones(10))
    assert Q is None and cfg.model_kind == _lib.MODEL_AUV and cfg.state_cost_kind == _lib.STATE_COST_QUAT
    assert cfg.auv.contents.rk == 2 and abs(cfg.auv.contents.mass - 1862.87) < 1e-3
    cfg2, keep2 = _lib.Config(), []
    e3 = dict(normal=[0, 0, 1], aVec=[1, 0, 0], axis=[2, 1], speed=1.0, m_state=50.0, m_vel=5.0)
    assert _lib._fill_13state(cfg2, keep2, None, False, e3, [1.0] * 13) == [1.0] * 13
    assert cfg2.state_cost_kind == _lib.STATE_COST_ELLIPSE3D and cfg2.model_kind == 0
