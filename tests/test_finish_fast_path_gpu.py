"""The finish kernel's column-major fast path (k_finish_cols_cm, k_finish_cols_batch<A, true>) against the kernel it replaces
(MPPI_TUNE_FINISH_GENERIC = 1: k_finish_cols). Needs an MI355X: every test is marked `gpu`.

column_combine's association is the definition of the result, so the two paths must agree bit for bit: point-mass handles with
H = 4, a in {1, 2, 3, 4}. What the kernel receives as its record count is not the tile count nb but record_pad(nb), a multiple of 128
(the slots no tile owns hold pads, scattered between the real records by record_slot): the tile counts below reach it as every multiple
of 128 up to 1024 (1, 63, 64, 65 -> 128; 255, 256 -> 256; 257 -> 384; 385 -> 512; 513 -> 640; 641 -> 768; 769 -> 896; 1023, 1024 -> 1024),
so every `< nb` mask of the four-slots-per-thread layout is met with a block of slots full, half full and empty, and one count above
1024 (the 16:1 fold, then the generic kernel on row-major records on both handles). Two launches per step everywhere (fused_step = 0: at
128 tiles and below the default step is one launch and has no finish kernel). tests/test_update_given_gpu.py holds the same kernels to
fp64 on designed inputs.
"""
import numpy as np
import pytest

from update_given_util import limits

pytestmark = pytest.mark.gpu
F32 = np.float32
H, STEPS = 4, 3
NB = (1, 63, 64, 65, 255, 256, 257, 385, 513, 641, 769, 1023, 1024, 1025)
VARIANTS = ("plain", "clip", "normalize")


@pytest.fixture(scope="module")
def m():
    import mppi_tf_amd
    assert mppi_tf_amd.load().mppi_device_count() >= 1, "no GPU visible to libmppi_hip.so"
    return mppi_tf_amd


def handle(m, nb, a, variant, **tuning):
    goal = np.zeros(2 * a, F32)
    goal[0::2] = [1.0, 0.5, 0.75, 0.25][:a]
    h = m.Handle(k=64 * nb, tau=H, s_dim=2 * a, a_dim=a, dt=0.1, mass=1.0, lam=1.0, sigma=0.25 * np.eye(a, dtype=F32), goal=goal,
                 normalize_cost=variant == "normalize", tuning=dict(tuning, fused_step=0))
    if variant == "clip":
        h.set_action_limits(*limits(a))
    return h


def state(m, h):
    return dict(U=h.get_action_sequence(), step=h.get_step_counter(), beta=h.debug_get(m.DBG_BETA), eta=h.debug_get(m.DBG_ETA))


def assert_same(got, want, what):
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (what, key))


def start(a):
    x = np.zeros(2 * a, F32)
    x[0::2] = [0.1, -0.2, 0.3, -0.4][:a]
    return x


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("a", (1, 2, 3, 4))
@pytest.mark.parametrize("nb", NB, ids=["nb%d" % n for n in NB])
def test_fast_path_has_the_bits_of_the_generic_kernel(m, nb, a, variant):
    """three steps from the same start: every u, the sequence, the step counter and the debug (beta, eta) after each step"""
    hf, hg = handle(m, nb, a, variant), handle(m, nb, a, variant, finish_generic=1)
    x = start(a)
    for s in range(STEPS):
        uf, ug = hf.next(x), hg.next(x)
        np.testing.assert_array_equal(uf, ug, err_msg="u of step %d" % s)
        assert_same(state(m, hf), state(m, hg), "step %d" % s)
        x[1::2] = uf * F32(0.1)  # (another state every step)
    assert hf.get_step_counter() == STEPS
    U = hf.get_action_sequence()
    assert np.isfinite(U).all() and np.abs(U).max() > 0
    if variant == "clip":  # (the stored sequence is the shift of U': its last row is zero, the others lie in their dimension's band)
        lo, hi = limits(a)
        assert (U[:-1] >= lo).all() and (U[:-1] <= hi).all(), U
    hf.close(); hg.close()


def armable(m):
    h = handle(m, 2, 1, "plain")
    try:
        h.set_tuning("armed_us", 100)
        return True
    except Exception:
        return False
    finally:
        h.close()


@pytest.mark.parametrize("a", (1, 3))
def test_an_armed_launch_that_aborts_changes_nothing(m, a):
    """257 tiles: rollout + finish behind every armed launch. Two steps, the second fed to the launch armed behind the first; reading the
    state then retires the launch armed behind the second: tile 0 aborts, and its finish (the verdict gates the stores, no longer the
    loads) leaves u, the sequence, the step counter and (beta, eta) where the generic kernel on a handle that never arms has them"""
    if not armable(m):
        pytest.skip("no large-BAR device: MPPI_TUNE_ARMED_US is unsupported here")
    ha, hg = handle(m, 257, a, "clip", armed_us=20000, armed_always=1), handle(m, 257, a, "clip", finish_generic=1)
    x = start(a)
    for s in range(2):
        ua, ug = ha.next(x), hg.next(x)
        np.testing.assert_array_equal(ua, ug, err_msg="u of step %d" % s)
    want = state(m, hg)
    assert_same(state(m, ha), want, "after the abort")
    assert want["step"] == 2
    assert_same(state(m, ha), want, "read again")
    np.testing.assert_array_equal(ha.next(x), hg.next(x))  # and on: the step after the abort draws the noise it would have drawn
    assert_same(state(m, ha), state(m, hg), "the step after")
    ha.close(); hg.close()
