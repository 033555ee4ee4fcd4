"""CPU-side checks of the batched-controller surface (no compute calls): the header declares the batch entry points, the library exports
them, the binding covers them and the package exports BatchHandle."""
import pytest

from test_capi_symbols import declared_functions

BATCH = ["mppi_create_batch", "mppi_batch_size", "mppi_batch_set_goals", "mppi_batch_next", "mppi_batch_next_device",
         "mppi_batch_get_action_sequences", "mppi_batch_set_action_sequences", "mppi_batch_debug_get"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import mppi_tf_amd
    return mppi_tf_amd


def test_header_declares_the_batch_entry_points():
    names = declared_functions()
    for n in BATCH:
        assert n in names, n


def test_library_and_binding_cover_the_batch_entry_points(pkg):
    from mppi_tf_amd import _lib
    lib = pkg.load()
    for n in BATCH:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.mppi_batch_size(None) == 0
    assert "BatchHandle" in pkg.__all__ and pkg.BatchHandle is _lib.BatchHandle
    assert b"k_rollout_pc_batch" in open(_lib.SO_PATH, "rb").read()
